// The LDS-DMA primitives shared by gemm_glds.hip, gemm_8ph.hip, relattn.hip, attn_map.hip and conv1d_wgrad.hip: what every kernel
// that stages with global_load_lds_dwordx4 needs around the instruction itself.  Nothing here knows a tile shape or an operand kind.
#pragma once
#include "common.h"
#include "../../include/s2svc_hip.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;

namespace {

// the operand types of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gbl_void;

// counted waits: the DMAs issued after the N oldest outstanding ones stay in flight
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// 16 bytes of zeros: the DMA source of every piece outside the matrix / the conv input (one copy per translation unit)
__device__ __attribute__((aligned(16))) uint4 g_zero16 = {0u, 0u, 0u, 0u};

// address of the zero block as an opaque per-lane value: keeps `ok ? src : zero` a plain 64-bit select, so ONE DMA /
// load instruction serves valid and padding lanes alike (a visible global address makes hipcc split every load in two
// EXEC-masked halves with a branch around each)
__device__ __forceinline__ uint64_t zero_addr() {
  uint64_t z = reinterpret_cast<uint64_t>(&g_zero16);
  asm volatile("" : "+v"(z));
  return z;
}

// LDS image of K-contiguous rows of 64 bf16 (128-B rows, 8 pieces of 16 B), lane-linear per DMA instruction as the instruction
// requires: piece c of row r lives at r*128 + ((c ^ lds_swz(r)) << 4).  The XOR goes into the per-lane SOURCE address and,
// identically, into the read address; it puts the 16 lanes of every ds_read_b128 lane group (rows r..r+15 at pieces c / c^1) on 16
// distinct 16-byte bank slots of the 256-byte LDS row.
__device__ __forceinline__ int lds_swz(int r) { return (r >> 1) & 7; }
__device__ __forceinline__ int lds_off(int r, int c) { return r * 128 + ((c ^ lds_swz(r)) << 4); }

// Transposing fragment read (ds_read_b64_tr_b16) of a k-major image: 32-byte k rows of 16 bf16, from k row `row0` on.  Lane l gets column
// (l & 15) at k = row0 + 4g..4g+3 and row0 + 16+4g..16+4g+3 (g = l >> 4) -- a PERMUTATION of the MFMA's k positions, harmless while both operands
// of the product use it.  Every kernel that must sum in the same order as another one takes its k positions from here.
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;
typedef __attribute__((address_space(3))) s16x4_t lds_s16x4_t;
__device__ __forceinline__ bf16x8_t tr_fragment_read(const char* img, int row0, int lane) {
  const char* p = img + (row0 + (lane >> 4) * 4 + ((lane & 15) >> 2)) * 32 + (lane & 3) * 8;
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)p);
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(p + 512));
  const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}

// XCD-aware work order.  The dispatcher deals consecutive workgroup ids round-robin to the 8 XCDs (each with its own L2); handing
// XCD x the x-th CONTIGUOUS run of the nwg work items makes the workgroups that run side by side on one XCD share operand panels
// through that L2 instead of each pulling them over the fabric.  Bijective for any nwg.
__device__ __forceinline__ int xcd_contiguous_id(int id, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = id & 7, j = id >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}

// Grouped launch: up to GROUP_MAX independent GEMMs as ONE grid.  tile_start[p] .. tile_start[p+1] are the workgroups of problem p.
// The descriptors travel BY VALUE in the kernel-argument segment (nothing to upload; hipGraph capture records them with the node).
// (The kernels find their problem with a loop of their own: behind a shared function the compiler schedules the nine compares
// differently, and the grouped kernels are kept instruction for instruction.)
constexpr int GROUP_MAX = 10;                              // 10 * 392 B + 44 B of prefix sums + n = 3968 B < the 4 KB kernarg limit
struct group_args {
  s2svc_gemm_desc d[GROUP_MAX];
  int32_t tile_start[GROUP_MAX + 1];
  int32_t n;
};
static_assert(sizeof(group_args) <= 4096, "kernel arguments are limited to 4 KB");

}  // namespace
