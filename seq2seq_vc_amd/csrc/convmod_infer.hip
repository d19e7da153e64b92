// Core of the Conformer convolution module in INFERENCE mode, fp32 or bf16, channel-last, one launch, per-row lengths:
//     (pointwise conv 1) -> GLU -> depthwise conv k -> BatchNorm1d (running statistics) -> Swish -> (pointwise conv 2)
// reference: modules/conformer/convolution.py:68-75 in eval().  The separate ops take four launches (GLU, depthwise conv, 1 / sqrt(var + eps),
// BatchNorm-apply + Swish) and two intermediate tensors; csrc/convmod.hip fuses the TRAINING core (batch statistics, bf16 only).  Here:
//     out[b, t, c] = swish(bn_eval(bias[c] + sum_j w[c, j] * g[b, t + j - (k - 1) / 2, c]))      t <  vlens[b]
//     out[b, t, c] = 0                                                                              t >= vlens[b]
//     g = glu(y2) at frames 0 <= t' < vlens[b], 0 elsewhere
// so that row b of a padded batch is what the utterance gives when it is processed alone (AASVC.inference_batch): frames >= vlens[b] of y2
// are never LOADED, whatever they hold.
// A workgroup owns 64 frames x 64 channels of one utterance (+ (k - 1) / 2 halo frames each side).  HBM-bound: y2 is read once per tile
// (+ halo) and out written once, all in 16-byte accesses; g lives in LDS as [frame][channel] and a lane reads down its own column
// (conflict-free).  k = 7 / 15 / 31 keep the taps and a sliding window in registers; any other odd k <= 31 reads taps and window from LDS.
// fp32 accumulation in a fixed order, no atomics, no workspace, every output element written exactly once.
#include "common.h"
#include "../../include/s2svc_hip.h"

namespace {

constexpr int TT = 64, CT = 64, FR = TT / 4, KS_MAX = 31;

__device__ __forceinline__ void ld8(const float* p, float (&f)[8]) { load_f32x8(p, f); }
__device__ __forceinline__ void ld8(const bf16_t* p, float (&f)[8]) { unpack_bf16x8(*reinterpret_cast<const uint4*>(p), f); }

// KS > 0: the kernel size at compile time; KS == 0: any odd ks <= KS_MAX at run time
template <typename T, int KS>
__global__ __launch_bounds__(256) void convmod_infer_kernel(int Tn, int C, int ks_rt, const T* __restrict__ y2, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ run_mean,
                                                            const float* __restrict__ run_var, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, T* __restrict__ out, int tchunks,
                                                            const int32_t* __restrict__ vlens) {
  constexpr int KM = KS ? KS : KS_MAX, ROWS_M = TT + KM - 1, NP = (ROWS_M + 31) / 32;
  const int ks = KS ? KS : ks_rt, PAD = (ks - 1) / 2, ROWS = TT + 2 * PAD;
  __shared__ __attribute__((aligned(16))) float G[ROWS_M * CT];
  __shared__ float Wl[KS ? 1 : KS_MAX * CT];
  const int c0 = blockIdx.x * CT;
  const int b = blockIdx.y / tchunks, t0 = (blockIdx.y % tchunks) * TT;
  int Te = Tn;                                                       // frames >= Te are absent: zero padding on the way in, zero on the way out
  if (vlens) Te = vlens[b] < 0 ? 0 : (vlens[b] < Tn ? vlens[b] : Tn);
  const int v = threadIdx.x & 7, r8 = threadIdx.x >> 3;
  const int cl = threadIdx.x & 63, rq = threadIdx.x >> 6;
  const bool cv = c0 + v * 8 < C;                                    // C % 8 == 0: a lane's 8 channels are inside C or all outside
  T* ob = out + (int64_t)b * Tn * C + c0 + v * 8;
  if (t0 >= Te) {                                                    // the whole tile is absent (uniform over the workgroup)
    const float zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < TT / 32; ++i) {
      const int t = t0 + r8 + 32 * i;
      if (cv && t < Tn) st8(ob + (int64_t)t * C, zero);
    }
    return;
  }
  const T* yb = y2 + (int64_t)b * Tn * 2 * C + c0 + v * 8;
  // ---- phase 1: g = a * sigmoid(gate) for the tile's frames and its halo -> LDS
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int p = r8 + 32 * i, t = t0 - PAD + p;
    if (p < ROWS) {
      float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (cv && t >= 0 && t < Te) {
        float a[8], gt[8];
        ld8(yb + (int64_t)t * 2 * C, a);
        ld8(yb + (int64_t)t * 2 * C + C, gt);
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = a[e] / (1.f + expf(-gt[e]));
      }
      *reinterpret_cast<float4*>(&G[p * CT + v * 8]) = make_float4(g[0], g[1], g[2], g[3]);
      *reinterpret_cast<float4*>(&G[p * CT + v * 8 + 4]) = make_float4(g[4], g[5], g[6], g[7]);
    }
  }
  const bool cc = c0 + cl < C;
  const int ch = cc ? c0 + cl : 0;
  const float bs = (bias && cc) ? bias[ch] : 0.f;
  const float mu = run_mean[ch], rstd = 1.0f / sqrtf(run_var[ch] + eps);
  const float ga = gamma ? gamma[ch] : 1.f, be = beta ? beta[ch] : 0.f;
  float res[FR];
  if constexpr (KS != 0) {
    // ---- phase 2: a lane owns one channel and FR consecutive frames; taps and sliding window in registers
    constexpr int WIN = FR + KM - 1;
    float wr[KM], win[WIN];
#pragma unroll
    for (int j = 0; j < KM; ++j) wr[j] = cc ? w[(int64_t)ch * KM + j] : 0.f;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < WIN; ++i) win[i] = G[(rq * FR + i) * CT + cl];
#pragma unroll
    for (int o = 0; o < FR; ++o) {
      float acc = bs;
#pragma unroll
      for (int j = 0; j < KM; ++j) acc += wr[j] * win[o + j];
      res[o] = act_apply((acc - mu) * rstd * ga + be, S2S_ACT_SWISH);
    }
  } else {
    for (int j = rq; j < ks; j += 4) Wl[j * CT + cl] = cc ? w[(int64_t)ch * ks + j] : 0.f;
    __syncthreads();
#pragma unroll
    for (int o = 0; o < FR; ++o) {
      float acc = bs;
      for (int j = 0; j < ks; ++j) acc += Wl[j * CT + cl] * G[(rq * FR + o + j) * CT + cl];
      res[o] = act_apply((acc - mu) * rstd * ga + be, S2S_ACT_SWISH);
    }
  }
  __syncthreads();                                                   // every window is read: the tile's rows of G become the output image
#pragma unroll
  for (int o = 0; o < FR; ++o) G[(rq * FR + o) * CT + cl] = res[o];
  __syncthreads();
  // ---- phase 3: the output tile, 16 bytes per access; absent frames are written as zero
#pragma unroll
  for (int i = 0; i < TT / 32; ++i) {
    const int r = r8 + 32 * i, t = t0 + r;
    if (cv && t < Tn) {
      float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (t < Te) load_f32x8(&G[r * CT + v * 8], f);
      st8(ob + (int64_t)t * C, f);
    }
  }
}

template <typename T>
int launch_infer(int B, int Tn, int C, int ks, const void* y2, const float* w, const float* bias, const float* run_mean, const float* run_var,
                 const float* gamma, const float* beta, float eps, void* out, const int32_t* vlens, hipStream_t st) {
  const int tchunks = (Tn + TT - 1) / TT;
  const dim3 grid((C + CT - 1) / CT, B * tchunks);
#define S2S_CMI(K)                                                                                                                        \
  hipLaunchKernelGGL((convmod_infer_kernel<T, K>), grid, dim3(256), 0, st, Tn, C, ks, (const T*)y2, w, bias, run_mean, run_var, gamma, \
                     beta, eps, (T*)out, tchunks, vlens)
  if (ks == 7) S2S_CMI(7);
  else if (ks == 15) S2S_CMI(15);
  else if (ks == 31) S2S_CMI(31);
  else S2S_CMI(0);
#undef S2S_CMI
  S2S_CHECK_LAUNCH("convmod_infer_kernel");
  return 0;
}

}  // namespace

extern "C" int s2svc_convmod_infer_supported(int C, int ks) { return (C > 0 && C % 8 == 0 && ks >= 1 && ks <= KS_MAX && ks % 2 == 1) ? 1 : 0; }

extern "C" int s2svc_convmod_infer(int dtype, int B, int Tn, int C, int ks, const void* y2, const float* w, const float* bias,
                                   const float* run_mean, const float* run_var, const float* gamma, const float* beta, float eps, void* out,
                                   const int32_t* vlens, void* stream) {
  S2S_REQUIRE(dtype == S2S_F32 || dtype == S2S_BF16, "convmod_infer: dtype must be fp32 or bf16");
  S2S_REQUIRE(s2svc_convmod_infer_supported(C, ks), "convmod_infer: unsupported shape (C % 8 == 0, odd ks <= 31)");
  S2S_REQUIRE(B > 0 && Tn > 0 && y2 && w && run_mean && run_var && out, "convmod_infer: bad args");
  S2S_REQUIRE((int64_t)B * ((Tn + TT - 1) / TT) <= 65535, "convmod_infer: B * ceil(Tn / 64) exceeds the grid");
  S2S_REQUIRE(((uintptr_t)y2) % 16 == 0 && ((uintptr_t)out) % 16 == 0, "convmod_infer: y2 and out must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == S2S_F32) return launch_infer<float>(B, Tn, C, ks, y2, w, bias, run_mean, run_var, gamma, beta, eps, out, vlens, st);
  return launch_infer<bf16_t>(B, Tn, C, ks, y2, w, bias, run_mean, run_var, gamma, beta, eps, out, vlens, st);
}
