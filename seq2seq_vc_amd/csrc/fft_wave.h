// The one-wavefront-per-frame real FFT that the log-mel front-end (stft_fft.hip), Griffin-Lim (griffin_lim.hip) and the mel L1 loss
// (melspec.hip) share: complex helpers, the Stockham transform, the real-FFT unpack and its inverse pack, the view of the packed
// host table, librosa's centre-reflect index (the reflect-pad kernels of frontend.hip use it too), the overlap-add frame range and
// the sizing of the persistent grids.
//
// Contract.  A real frame of N samples is the complex sequence z[n] = x[2n] + i x[2n+1] of H = N / 2 points in one of a wavefront's
// two private LDS buffers of H points; a lane owns H / 64 points.  LDS operations of one wavefront execute in order, so a wave
// barrier between the passes is all the synchronisation the transform needs.  The table is built on the host in float64 and
// rounded once (ops/fft_tables.py):
//   w_half [H] complex exp(-2 pi i m / H) | w_full [H + 1] complex exp(-2 pi i k / N) | win [N] (zero-padded periodic Hann)
// The kernels keep w_half in LDS (fft_forward's `tw`); w_full and win are read where the table lies.
#pragma once
#include "common.h"

namespace {

struct c32 { float x, y; };
__device__ __forceinline__ c32 cadd(c32 a, c32 b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ c32 csub(c32 a, c32 b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ c32 cmul(c32 a, c32 b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ c32 mul_mi(c32 a) { return {a.y, -a.x}; }          // a * (-i)

// ---- the packed table ----
struct FftTable {
  const c32* tw;               // w_half [H]
  const c32* tf;               // w_full [H + 1]
  const float* win;            // [N]
};
constexpr int fft_table_floats(int N) { return 2 * (N / 2) + 2 * (N / 2 + 1) + N; }
__host__ __device__ __forceinline__ FftTable fft_table(const float* tables, int N) {
  const int H = N / 2;
  const c32* tw = reinterpret_cast<const c32*>(tables);
  return {tw, tw + H, tables + 2 * H + 2 * (H + 1)};
}

// w_half into LDS, by all THREADS threads of the workgroup; the caller's __syncthreads() publishes it
template <int H, int THREADS>
__device__ __forceinline__ void load_twiddles(c32* tw, const FftTable& tab) {
  for (int i = threadIdx.x; i < H; i += THREADS) tw[i] = tab.tw[i];
}

// ---- the transform ----
// H-point forward complex FFT of one wavefront between its two LDS buffers (Stockham autosort: radix-4 passes and one radix-2 pass
// if log2(H) is odd).  Returns the buffer that holds the result in natural order; the other one is free.
template <int H>
__device__ __forceinline__ c32* fft_forward(c32* src, c32* dst, const c32* tw, int lane) {
  int p = 1;
#pragma unroll 1
  for (; p * 4 <= H; p *= 4) {
    __builtin_amdgcn_wave_barrier();
    constexpr int T = H / 4;
    const int st = T / p;
#pragma unroll
    for (int q = 0; q < T / 64; ++q) {
      const int i = lane + 64 * q;
      const int k = i & (p - 1);
      const int j = ((i - k) << 2) + k;
      const c32 u0 = src[i];
      c32 u1 = src[i + T], u2 = src[i + 2 * T], u3 = src[i + 3 * T];
      if (p > 1) {                                            // (uniform) the first pass has k = 0: all twiddles are 1
        u1 = cmul(u1, tw[k * st]);
        u2 = cmul(u2, tw[2 * k * st]);
        u3 = cmul(u3, tw[3 * k * st]);
      }
      const c32 v0 = cadd(u0, u2), v1 = csub(u0, u2), v2 = cadd(u1, u3), v3 = mul_mi(csub(u1, u3));
      dst[j] = cadd(v0, v2);
      dst[j + p] = cadd(v1, v3);
      dst[j + 2 * p] = csub(v0, v2);
      dst[j + 3 * p] = csub(v1, v3);
    }
    c32* tmp = src; src = dst; dst = tmp;
  }
  if constexpr (__builtin_ctz(H) & 1) {                       // one radix-2 pass left (p = H / 2)
    __builtin_amdgcn_wave_barrier();
    constexpr int T = H / 2;
#pragma unroll
    for (int q = 0; q < T / 64; ++q) {
      const int i = lane + 64 * q;
      const int k = i & (p - 1);
      const int j = ((i - k) << 1) + k;
      const c32 u0 = src[i], u1 = cmul(src[i + T], tw[k * (T / p)]);
      dst[j] = cadd(u0, u1);
      dst[j + p] = csub(u0, u1);
    }
    c32* tmp = src; src = dst; dst = tmp;
  }
  __builtin_amdgcn_wave_barrier();
  return src;
}

// ---- real FFT <-> packed complex FFT ----
// xa = X[k] and xb = X[H - k] of the real frame from its packed transform Z: X[k] = E + w^k O, X[H - k] = conj(E - w^k O) with
// E = (Z[k] + conj Z[H-k]) / 2, O = -i (Z[k] - conj Z[H-k]) / 2: one twiddle product gives two bins.  k = 0 .. H / 2; k = 0 gives
// X[0] and X[N/2] (both real), k = H / 2 gives the same bin twice.
template <int H>
__device__ __forceinline__ void unpack_pair(const c32* z, const c32* tf, int k, c32& xa, c32& xb) {
  const c32 zk = z[k];
  c32 zc = z[(H - k) & (H - 1)];
  zc.y = -zc.y;
  const c32 xe = {0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y)};
  const c32 xo = mul_mi({0.5f * (zk.x - zc.x), 0.5f * (zk.y - zc.y)});
  const c32 wx = cmul(tf[k], xo);
  xa = cadd(xe, wx);
  const c32 a1 = csub(xe, wx);
  xb = {a1.x, -a1.y};
}

// The inverse: conj of the packed input Z[k] = E + i O, E = (xa + conj xb) / 2, O = (xa - conj xb) / 2 * exp(+2 pi i k / N), for the
// pair xa = Y[k], xb = Y[H - k] of a one-sided spectrum Y; w = w_full[k].  The inverse transform is conj(FFT(conj Z)) / H.
__device__ __forceinline__ c32 pack_conj(c32 xa, c32 xb, c32 w) {
  const c32 xe = {0.5f * (xa.x + xb.x), 0.5f * (xa.y - xb.y)};
  const c32 d = {0.5f * (xa.x - xb.x), 0.5f * (xa.y + xb.y)};
  const c32 xo = cmul(d, {w.x, -w.y});
  return {xe.x - xo.y, -(xe.y + xo.x)};
}

// ---- index arithmetic ----
// Sample j of a signal of n samples under librosa's centre mode (numpy's pad "reflect", any number of reflections);
// period = n > 1 ? 2 (n - 1) : 1 is the caller's, computed once per frame.
__device__ __forceinline__ int64_t reflect_index(int64_t j, int64_t n, int64_t period) {
  if (n <= 1) return 0;
  j %= period;
  if (j < 0) j += period;
  if (j >= n) j = period - j;
  return j;
}

// Frames t_lo .. t_hi (ascending; empty if t_lo > t_hi) of T frames of N samples, hop apart, that cover position pos >= 0:
// t_lo = ceil((pos - N + 1) / hop), t_hi = min(pos / hop, T - 1), so 0 <= pos - t hop < N for every t of the range.
__device__ __forceinline__ void ola_frame_range(int64_t pos, int N, int hop, int T, int& t_lo, int& t_hi) {
  const int64_t lo_num = pos - N + hop;
  t_lo = lo_num > 0 ? (int)(lo_num / hop) : 0;
  int64_t hi = pos / hop;
  if (hi > T - 1) hi = T - 1;
  t_hi = (int)hi;
}

// ---- host: the persistent grids ----
// Workgroups of `lds` bytes the chip holds at once: 256 CUs x min(160 KB / lds, cap), cap = what the kernel's registers allow.
inline int64_t fft_resident_groups(size_t lds, int cap) {
  const int per_cu = (int)(160 * 1024 / lds) > 0 ? (int)(160 * 1024 / lds) : 1;
  return 256 * (per_cu < cap ? per_cu : cap);
}
inline dim3 fft_persistent_grid(int64_t groups, size_t lds, int cap) {
  const int64_t resident = fft_resident_groups(lds, cap);
  return dim3((unsigned)(groups < resident ? groups : resident));
}

// Raises the dynamic LDS limit of Kernel to `lds` bytes when that is above what it already has (64 KB without asking).
template <auto Kernel>
inline int fft_raise_lds_limit(size_t lds, const char* err) {
  static size_t have = 64 * 1024;
  if (lds <= have) return 0;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    s2svc_set_error(err);
    return -2;
  }
  have = lds;
  return 0;
}

}  // namespace
