// Weight gradients of 'same'-padded stride-1 Conv1d layers (channel-last bf16 activations), several layers in ONE launch that
// takes at most `max_workgroups` CUs: the Postnet's five k = 5 convolutions beside the data-gradient chain of a training step.
//
//   dw[o][i][j] += sum_{b,t} dy[b,t,o] * x[b, t + j - pad, i]          (taps outside [0, T) of the same utterance count as zero)
//
// A unit is (item, 64 output channels, 64 input channels) and keeps all KS taps of its block: 4 waves x (32 x 32 x KS) = 80 fp32
// accumulators per lane at KS = 5.  It walks the utterances in order and every utterance in 64-frame steps, so one accumulator set
// sums all B*T rows ascending: no split-K across workgroups, no fp32 temporary, no reduction pass, and the result lands in the
// parameter's own (Cout, Cin, KS) gradient slot.  An item may ask for the sum to be taken in runs of `chunk_steps` steps (each run
// from zero, the runs added in order into a second register set): with T % 64 == 0 the steps are the 64-row K tiles of the split-K
// GEMM this launch stands in for, the runs its split-K partials and their sum its reduction pass, MFMA for MFMA -- the same bits.
// That equality is a property of the CALLER's choice of chunk_steps, and holds only while the replaced launches keep what it
// mirrors: 64-row K tiles on the 16x16x32 bf16 MFMA, the split-K plan, and splitk_reduce adding partials in ascending order.
// (The fragment k positions are gemm_glds_kernel's TR operands' by construction: both read through tr_fragment_read, lds_dma.h.)  The kernel itself promises the formula, the order stated
// here, and the rule of its check; tests/gpu_conv1d_wgrad_check.py fails when the plan or the route drifts.
// Workgroups walk the units in order (u = blockIdx.x, += gridDim.x): the grid size changes which workgroup computes a unit,
// never how, so the bits do not depend on the cap.
//
// Both operands are reduced over their slow axis (frames).  A step stages 64 dy rows and ONE slab of 64 + KS - 1 x rows
// [t0 - pad, t0 + 64 + pad) k-major in LDS: per 16 channels an image of 32-byte frame rows, the layout of the TR stages of
// gemm_glds.hip, so that a half-wave of a transposing read (ds_read_b64_tr_b16) covers 8 consecutive frame rows = 256 contiguous
// bytes.  Tap j reads the slab j rows further down; rows outside the utterance and channels past the tensor are stored as zero,
// and nothing outside [0, T) of the utterance at hand is read from memory.  Both operands take the same permuted k positions of
// a 32-frame half (4g..4g+3 and 16+4g..16+4g+3 for lane group g), which a product that sums over k does not see.
// LDS: 4 * (2112 + 2240) = 17 408 bytes (single stage; the next step's rows wait in registers).
#include "lds_dma.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4_t;

constexpr int CW_MAX_ITEMS = 16;
constexpr int CW_ROWS = 64;                 // frames per reduction step
constexpr int CW_BLK = 64;                  // channels per unit, both ways

struct cw_item {
  const bf16_t* dy;
  const bf16_t* x;
  float* dw;
  int B, T, Cin, Cout;
  int unit0, nci;                           // first unit of the item; Cin blocks per Cout block
  int chunk;                                // steps per partial sum (0: one sum over all steps)
};
struct cw_args {
  cw_item it[CW_MAX_ITEMS];
  int n, units;
};

template <int KS>
struct cw_geom {
  static constexpr int PAD = (KS - 1) / 2;
  static constexpr int XROWS = CW_ROWS + KS - 1;
  static constexpr int DY_SUB = CW_ROWS * 32 + 64;     // bytes per 16-channel image (+64: the four images start in different banks)
  static constexpr int X_SUB = XROWS * 32 + 64;
  static constexpr int X_OFF = 4 * DY_SUB;
  static constexpr int BYTES = 4 * DY_SUB + 4 * X_SUB;
  static constexpr int XEXTRA = (XROWS - 64) * 8;      // 16-byte pieces of the slab's last KS - 1 rows
};

// 8 frames of 16 channels, transposed: lane l of the wave gets channel (l & 15), frames k = 4g..4g+3 and 16+4g..16+4g+3 (g = l >> 4)
__device__ __forceinline__ bf16x8_t cw_fragment(const char* img, int row0, int lane) {
  return tr_fragment_read(img, row0, lane);
}

template <int KS>
__global__ __launch_bounds__(256) void conv1d_wgrad_kernel(const cw_args a) {
  typedef cw_geom<KS> G;
  __shared__ __attribute__((aligned(256))) char smem[G::BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;       // the wave's 32 x 32 corner of the (Cout, Cin) block
  const int pc = tid & 7, pr = tid >> 3;                        // staging: 16-byte piece (8 channels) pc of rows pr, pr + 32 (, pr + 64)
  const int st_off = pr * 32 + (pc & 1) * 16;            // byte offset inside a 16-channel image (image index: pc >> 1)

  for (int u = blockIdx.x; u < a.units; u += gridDim.x) {
    int ii = 0;
#pragma unroll 1
    for (int q = 1; q < a.n; ++q)
      if (u >= a.it[q].unit0) ii = q;
    const cw_item& it = a.it[ii];
    const int lu = u - it.unit0;
    const int o0 = (lu / it.nci) * CW_BLK, c0 = (lu % it.nci) * CW_BLK;
    const int T = it.T, Cin = it.Cin, Cout = it.Cout;
    const int tsteps = (T + CW_ROWS - 1) / CW_ROWS, nsteps = it.B * tsteps;
    const bool dy_col = o0 + pc * 8 < Cout, x_col = c0 + pc * 8 < Cin;      // (channel counts are multiples of 16: whole pieces)
    const bf16_t* dyp = it.dy + o0 + pc * 8;
    const bf16_t* xp = it.x + c0 + pc * 8;

    f32x4_t acc[KS][2][2], tot[KS][2][2];
#pragma unroll
    for (int j = 0; j < KS; ++j)
#pragma unroll
      for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int fn = 0; fn < 2; ++fn) acc[j][fm][fn] = tot[j][fm][fn] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    int run_end = it.chunk > 0 && it.chunk < nsteps ? it.chunk : nsteps;        // (uniform) the step behind the current run

    uint4 rdy[2], rx[3];
    auto fetch = [&](int s) {
      const int b = s / tsteps, t0 = (s - b * tsteps) * CW_ROWS;
      const int64_t row0 = (int64_t)b * T;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int t = t0 + pr + h * 32;
        rdy[h] = (dy_col && t < T) ? *reinterpret_cast<const uint4*>(dyp + (row0 + t) * Cout) : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int h = 0; h < 3; ++h) {
        const int t = t0 - G::PAD + pr + h * 32;
        const bool mine = h < 2 || tid < G::XEXTRA;
        rx[h] = (mine && x_col && t >= 0 && t < T) ? *reinterpret_cast<const uint4*>(xp + (row0 + t) * Cin) : make_uint4(0u, 0u, 0u, 0u);
      }
    };

    fetch(0);
    for (int s = 0; s < nsteps; ++s) {
      __syncthreads();                                   // the fragments of the step before are read
      {
        char* dimg = smem + (pc >> 1) * G::DY_SUB + st_off;
        char* ximg = smem + G::X_OFF + (pc >> 1) * G::X_SUB + st_off;
        *reinterpret_cast<uint4*>(dimg) = rdy[0];
        *reinterpret_cast<uint4*>(dimg + 32 * 32) = rdy[1];
        *reinterpret_cast<uint4*>(ximg) = rx[0];
        *reinterpret_cast<uint4*>(ximg + 32 * 32) = rx[1];
        if (tid < G::XEXTRA) *reinterpret_cast<uint4*>(ximg + 64 * 32) = rx[2];
      }
      __syncthreads();
      const int tleft = T - (s % tsteps) * CW_ROWS;      // frames of this step (uniform): an all-zero second half is skipped
      if (s + 1 < nsteps) fetch(s + 1);
      const int halves = tleft > 32 ? 2 : 1;
      for (int kh = 0; kh < halves; ++kh) {
        bf16x8_t fa[2];
#pragma unroll
        for (int fm = 0; fm < 2; ++fm) fa[fm] = cw_fragment(smem + ((wm >> 4) + fm) * G::DY_SUB, kh * 32, lane);
#pragma unroll
        for (int j = 0; j < KS; ++j) {
          bf16x8_t fb[2];
#pragma unroll
          for (int fn = 0; fn < 2; ++fn) fb[fn] = cw_fragment(smem + G::X_OFF + ((wn >> 4) + fn) * G::X_SUB, kh * 32 + j, lane);
#pragma unroll
          for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fn = 0; fn < 2; ++fn)
              acc[j][fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[fm], fb[fn], acc[j][fm][fn], 0, 0, 0);
        }
      }
      if (s + 1 == run_end) {                            // a run is complete: add it to the total, start the next one from zero
#pragma unroll
        for (int j = 0; j < KS; ++j)
#pragma unroll
          for (int fm = 0; fm < 2; ++fm)
#pragma unroll
            for (int fn = 0; fn < 2; ++fn) {
#pragma unroll
              for (int e = 0; e < 4; ++e) tot[j][fm][fn][e] += acc[j][fm][fn][e];      // (scalar adds: no packed fp32, see _lib.py)
              acc[j][fm][fn] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
            }
        run_end = run_end + it.chunk < nsteps ? run_end + it.chunk : nsteps;
      }
    }

    // accumulator register e of fragment (fm, fn): output channel o0 + wm + 16 fm + 4 (lane >> 4) + e, input channel c0 + wn + 16 fn + (lane & 15)
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
      for (int fn = 0; fn < 2; ++fn) {
        const int ci = c0 + wn + fn * 16 + (lane & 15);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int o = o0 + wm + fm * 16 + (lane >> 4) * 4 + e;
          if (o < Cout && ci < Cin) {
            float* p = it.dw + ((int64_t)o * Cin + ci) * KS;
#pragma unroll
            for (int j = 0; j < KS; ++j) p[j] += tot[j][fm][fn][e];
          }
        }
      }
  }
}

bool cw_supported(int Cout, int Cin, int ks, int dtype) {
  return dtype == S2S_BF16 && ks == 5 && Cout >= 16 && Cin >= 16 && (Cout % 16) == 0 && (Cin % 16) == 0;
}

}  // namespace

extern "C" int s2svc_conv1d_wgrad_supported(int Cout, int Cin, int ks, int dtype) { return cw_supported(Cout, Cin, ks, dtype) ? 1 : 0; }

extern "C" int s2svc_conv1d_wgrad_grouped(const s2svc_conv1d_wgrad_item* items, int n, int max_workgroups, void* stream) {
  S2S_REQUIRE(items != nullptr && n >= 1, "conv1d_wgrad_grouped: no items");
  S2S_REQUIRE(max_workgroups >= 0, "conv1d_wgrad_grouped: max_workgroups must be >= 0");
  // every check of every item comes before the first launch
  for (int i = 0; i < n; ++i) {
    const s2svc_conv1d_wgrad_item& p = items[i];
    S2S_REQUIRE(cw_supported(p.Cout, p.Cin, p.ks, p.dtype), "conv1d_wgrad_grouped: unsupported item (bf16, ks 5, Cin and Cout multiples of 16)");
    S2S_REQUIRE(p.chunk_steps >= 0, "conv1d_wgrad_grouped: chunk_steps must be >= 0");
    S2S_REQUIRE(p.B >= 1 && p.T >= 1 && (int64_t)p.B * p.T < (1ll << 31), "conv1d_wgrad_grouped: bad B / T");
    S2S_REQUIRE(p.dy != nullptr && p.x != nullptr && p.dw != nullptr, "conv1d_wgrad_grouped: null operand");
    S2S_REQUIRE((reinterpret_cast<uintptr_t>(p.dy) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.x) & 15) == 0,
                "conv1d_wgrad_grouped: dy and x must be 16-byte aligned");
    S2S_REQUIRE((reinterpret_cast<uintptr_t>(p.dw) & 3) == 0, "conv1d_wgrad_grouped: dw must be 4-byte aligned");
  }
  // items that add into overlapping dw ranges never share a launch (launches on one stream run in order)
  int i = 0;
  while (i < n) {
    cw_args a;
    uintptr_t dw_bytes[CW_MAX_ITEMS];           // extent of every queued item's slot
    a.n = 0;
    a.units = 0;
    for (; i < n && a.n < CW_MAX_ITEMS; ++i) {
      const s2svc_conv1d_wgrad_item& p = items[i];
      const uintptr_t lo = reinterpret_cast<uintptr_t>(p.dw), hi = lo + (uintptr_t)p.Cout * p.Cin * p.ks * 4;
      bool clash = false;
      for (int q = 0; q < a.n; ++q) {
        const uintptr_t qlo = reinterpret_cast<uintptr_t>(a.it[q].dw);
        const uintptr_t qhi = qlo + dw_bytes[q];
        clash = clash || (lo < qhi && qlo < hi);
      }
      if (clash) break;
      dw_bytes[a.n] = hi - lo;
      cw_item& c = a.it[a.n++];
      c.dy = static_cast<const bf16_t*>(p.dy);
      c.x = static_cast<const bf16_t*>(p.x);
      c.dw = p.dw;
      c.B = p.B; c.T = p.T; c.Cin = p.Cin; c.Cout = p.Cout;
      c.unit0 = a.units;
      c.nci = (p.Cin + CW_BLK - 1) / CW_BLK;
      c.chunk = p.chunk_steps;
      a.units += c.nci * ((p.Cout + CW_BLK - 1) / CW_BLK);
    }
    const int grid = (max_workgroups > 0 && max_workgroups < a.units) ? max_workgroups : a.units;
    hipLaunchKernelGGL(conv1d_wgrad_kernel<5>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    S2S_CHECK_LAUNCH("conv1d_wgrad_kernel");
  }
  return 0;
}
