// HuBERT-Soft content encoder (urhythmic/hubert.py): the kernels that are not GEMMs, LayerNorms or attention.
// replaces: bshall/hubert model.py FeatureExtractor layer 0 (Conv1d(1, 512, 10, 5, bias=False) -> GroupNorm(512, 512) -> GELU) and
// Hubert.logits + the log_softmax of urhythmic/model.py:33-35.
//
// Layer 0.  The waveform of row b is wav[b][0 .. lens[b]); HubertSoft.units pads it by 40 zero samples on both sides, which is index
// arithmetic here (`pad` = 40; 0 for Hubert.encode, which takes the waveform as it is): padded sample p is wav[p - pad] for
// pad <= p < lens[b] + pad, else 0.  Frame f of the L0_b = (lens[b] + 2 pad - 10) / 5 + 1
// frames of the row is the 10-tap product at p = 5 f, one fmaf chain in tap order, the same in both launches:
//   conv0_stats  per (row, channel) the sums of y and y^2 over the row's OWN frames, in double.  A row is cut into HB_CHUNKS chunks of
//                ceil(L0_b / HB_CHUNKS) frames (a function of the row's own length); a thread adds its channel's frames of one chunk one
//                after the other and writes the pair ws[b][chunk][2][512]; no atomics.
//   conv0_apply  adds the chunk pairs in chunk order, recomputes the product, normalises ((y - mean) * rstd * gamma + beta, biased
//                variance), applies the exact GELU and writes (B, L0, 512) channel-last; frames at or beyond L0_b are +0.
// Logits.  One wavefront per frame: lane k (k, k + 64, ..) holds unit k's dot product with the frame and the unit's squared norm, each
// as eight interleaved partial sums over the 256 features, added pairwise (a third of the rounding error of one running sum); cosine = dot / (max(|x|, eps) * max(|e_k|, eps)) with eps = 1e-8 (the rule of
// torch.cosine_similarity), divided by 0.1 (log_softmax = 0: written as it is), then log_softmax over the K units.  fp32 arithmetic; rows beyond a length are +0.
#include "common.h"
#include "../../include/s2svc_hip.h"

namespace {

constexpr int HB_C0 = 512, HB_TAPS = 10, HB_STRIDE = 5, HB_CHUNKS = 32;
constexpr int HB_FT = 256;                                  // frames per LDS tile of the statistics kernel
constexpr int HB_AT = 64;                                   // frames per workgroup of the apply kernel
constexpr int HB_D = 256, HB_KMAX = 256;

__device__ __forceinline__ int hb_frames0(int len, int pad) { return len + 2 * pad < HB_TAPS ? 0 : (len + 2 * pad - HB_TAPS) / HB_STRIDE + 1; }

// padded samples [5 f0, 5 f0 + 5 nf + 5) of row b -> LDS
__device__ __forceinline__ void hb_stage_wav(const float* __restrict__ wav, int len, int pad, int f0, int nf, float* sx) {
  for (int i = threadIdx.x; i < nf * HB_STRIDE + HB_STRIDE; i += blockDim.x) {
    const int p = f0 * HB_STRIDE + i - pad;
    sx[i] = p >= 0 && p < len ? wav[p] : 0.f;
  }
}
__device__ __forceinline__ float hb_conv0(const float (&w)[HB_TAPS], const float* sx) {
  float y = 0.f;
#pragma unroll
  for (int j = 0; j < HB_TAPS; ++j) y = __builtin_fmaf(w[j], sx[j], y);
  return y;
}

__global__ __launch_bounds__(256) void hubert_conv0_stats_kernel(int Nmax, int pad, const float* __restrict__ wav, const int32_t* __restrict__ lens,
                                                                 const float* __restrict__ w, double* __restrict__ ws) {
  __shared__ float sx[HB_FT * HB_STRIDE + HB_STRIDE];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int len = min(max(lens[b], 0), Nmax), L0 = hb_frames0(len, pad);
  const int cs = (L0 + HB_CHUNKS - 1) / HB_CHUNKS;
  const int fa = min(chunk * cs, L0), fb = min(fa + cs, L0);
  float w0[HB_TAPS], w1[HB_TAPS];
#pragma unroll
  for (int j = 0; j < HB_TAPS; ++j) { w0[j] = w[tid * HB_TAPS + j]; w1[j] = w[(tid + 256) * HB_TAPS + j]; }
  double s0 = 0., q0 = 0., s1 = 0., q1 = 0.;
  for (int f0 = fa; f0 < fb; f0 += HB_FT) {                  // block-uniform bounds
    const int nf = min(HB_FT, fb - f0);
    __syncthreads();
    hb_stage_wav(wav + (int64_t)b * Nmax, len, pad, f0, nf, sx);
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
      const double y0 = hb_conv0(w0, sx + f * HB_STRIDE), y1 = hb_conv0(w1, sx + f * HB_STRIDE);
      s0 += y0; q0 += y0 * y0;
      s1 += y1; q1 += y1 * y1;
    }
  }
  double* o = ws + ((int64_t)b * HB_CHUNKS + chunk) * 2 * HB_C0;
  o[tid] = s0; o[tid + 256] = s1;
  o[HB_C0 + tid] = q0; o[HB_C0 + tid + 256] = q1;
}

template <typename T>
__global__ __launch_bounds__(256) void hubert_conv0_apply_kernel(int Nmax, int pad, int L0max, const float* __restrict__ wav,
                                                                 const int32_t* __restrict__ lens, const float* __restrict__ w,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                 const double* __restrict__ ws, T* __restrict__ out) {
  __shared__ float sx[HB_AT * HB_STRIDE + HB_STRIDE];
  const int b = blockIdx.y, f0 = blockIdx.x * HB_AT, tid = threadIdx.x;
  const int len = min(max(lens[b], 0), Nmax), L0 = hb_frames0(len, pad);
  const int nf = min(HB_AT, L0max - f0);
  T* const orow = out + ((int64_t)b * L0max + f0) * HB_C0;
  if (f0 >= L0) {                                            // the whole tile is beyond the row
    for (int f = 0; f < nf; ++f) { stf(orow + (int64_t)f * HB_C0 + tid, 0.f); stf(orow + (int64_t)f * HB_C0 + tid + 256, 0.f); }
    return;
  }
  hb_stage_wav(wav + (int64_t)b * Nmax, len, pad, f0, min(nf, L0 - f0), sx);
  float wv[2][HB_TAPS], mean[2], rstd[2], ga[2], be[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int c = tid + e * 256;
#pragma unroll
    for (int j = 0; j < HB_TAPS; ++j) wv[e][j] = w[c * HB_TAPS + j];
    double s = 0., q = 0.;
    for (int k = 0; k < HB_CHUNKS; ++k) {                    // chunk order
      const double* p = ws + ((int64_t)b * HB_CHUNKS + k) * 2 * HB_C0;
      s += p[c];
      q += p[HB_C0 + c];
    }
    const double mu = s / L0, var = fmax(q / L0 - mu * mu, 0.);
    mean[e] = (float)mu;
    rstd[e] = (float)(1. / sqrt(var + (double)eps));
    ga[e] = gamma[c];
    be[e] = beta[c];
  }
  __syncthreads();
  for (int f = 0; f < nf; ++f) {
    const bool present = f0 + f < L0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      float r = 0.f;
      if (present) {
        const float y = hb_conv0(wv[e], sx + f * HB_STRIDE);
        r = act_apply(__builtin_fmaf((y - mean[e]) * rstd[e], ga[e], be[e]), S2S_ACT_GELU);
      }
      stf(orow + (int64_t)f * HB_C0 + tid + e * 256, r);
    }
  }
}

// eight interleaved partial sums (feature d goes to sum d & 7), added pairwise
__device__ __forceinline__ float hb_sum8(const float (&a)[8]) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])); }

template <typename T>
__global__ __launch_bounds__(256) void hubert_logits_kernel(int rows, int L, int K, int log_softmax, const T* __restrict__ units, const int32_t* __restrict__ lens,
                                                            const float* __restrict__ emb, float* __restrict__ out) {
  __shared__ float sx[4][HB_D];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wave;
  const bool live = r < rows;
  bool present = live;
  if (live && lens) { const int b = r / L; present = r - b * L < lens[b]; }
  if (live && present) {
#pragma unroll
    for (int e = 0; e < 4; ++e) sx[wave][lane + 64 * e] = ldf(units + (int64_t)r * HB_D + lane + 64 * e);
  }
  __syncthreads();
  if (!live) return;                                         // wave-uniform from here on
  float* const orow = out + (int64_t)r * K;
  if (!present) {
    for (int k = lane; k < K; k += 64) orow[k] = 0.f;
    return;
  }
  float xa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int d = 0; d < HB_D; d += 8) {
#pragma unroll
    for (int c = 0; c < 8; ++c) xa[c] = __builtin_fmaf(sx[wave][d + c], sx[wave][d + c], xa[c]);
  }
  const float nx = fmaxf(sqrtf(hb_sum8(xa)), 1e-8f);
  float z[HB_KMAX / 64];
  float zmax = -INFINITY;
#pragma unroll
  for (int i = 0; i < HB_KMAX / 64; ++i) {
    const int k = lane + 64 * i;
    z[i] = -INFINITY;
    if (k < K) {
      const float* e = emb + (int64_t)k * HB_D;
      float da[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ea[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int d = 0; d < HB_D; d += 8) {
        const float4 e0 = *reinterpret_cast<const float4*>(e + d), e1 = *reinterpret_cast<const float4*>(e + d + 4);
        const float ev[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          da[c] = __builtin_fmaf(sx[wave][d + c], ev[c], da[c]);
          ea[c] = __builtin_fmaf(ev[c], ev[c], ea[c]);
        }
      }
      const float dot = hb_sum8(da), ee = hb_sum8(ea);
      z[i] = dot / (nx * fmaxf(sqrtf(ee), 1e-8f)) / 0.1f;
      zmax = fmaxf(zmax, z[i]);
    }
  }
  if (!log_softmax) {                                       // wave-uniform: the raw logits of Hubert.logits
#pragma unroll
    for (int i = 0; i < HB_KMAX / 64; ++i)
      if (lane + 64 * i < K) orow[lane + 64 * i] = z[i];
    return;
  }
  zmax = wave_max(zmax);
  float se = 0.f;
#pragma unroll
  for (int i = 0; i < HB_KMAX / 64; ++i) se += lane + 64 * i < K ? expf(z[i] - zmax) : 0.f;
  se = wave_sum(se);
  const float lse = zmax + logf(se);
#pragma unroll
  for (int i = 0; i < HB_KMAX / 64; ++i)
    if (lane + 64 * i < K) orow[lane + 64 * i] = z[i] - lse;
}

}  // namespace

extern "C" int64_t s2svc_hubert_conv0_ws_bytes(int B) { return (int64_t)B * HB_CHUNKS * 2 * HB_C0 * (int64_t)sizeof(double); }

extern "C" int s2svc_hubert_conv0_stats(int B, int Nmax, int pad, const float* wav, const int32_t* lens, const float* w, double* ws, void* stream) {
  S2S_REQUIRE(B >= 1 && B <= 65535 && Nmax >= 1 && Nmax < (1 << 30), "hubert_conv0_stats: 1 <= B <= 65535, 1 <= Nmax < 2^30");
  S2S_REQUIRE(pad >= 0 && pad <= 4096, "hubert_conv0_stats: 0 <= pad <= 4096");
  S2S_REQUIRE(wav && lens && w && ws, "hubert_conv0_stats: wav, lens, w and ws are required");
  hipLaunchKernelGGL(hubert_conv0_stats_kernel, dim3(HB_CHUNKS, B), dim3(256), 0, (hipStream_t)stream, Nmax, pad, wav, lens, w, ws);
  S2S_CHECK_LAUNCH("hubert_conv0_stats");
  return 0;
}

extern "C" int s2svc_hubert_conv0_apply(int dtype, int B, int Nmax, int pad, int L0max, const float* wav, const int32_t* lens, const float* w,
                                        const float* gamma, const float* beta, float eps, const double* ws, void* out, void* stream) {
  S2S_REQUIRE(dtype == S2S_F32 || dtype == S2S_BF16, "hubert_conv0_apply: fp32 or bf16 output");
  S2S_REQUIRE(B >= 1 && B <= 65535 && Nmax >= 1 && Nmax < (1 << 30) && L0max >= 1, "hubert_conv0_apply: 1 <= B <= 65535, 1 <= Nmax < 2^30, L0max >= 1");
  S2S_REQUIRE(pad >= 0 && pad <= 4096, "hubert_conv0_apply: 0 <= pad <= 4096");
  S2S_REQUIRE(wav && lens && w && gamma && beta && ws && out, "hubert_conv0_apply: every pointer is required");
  const dim3 grid((L0max + HB_AT - 1) / HB_AT, B);
  if (dtype == S2S_F32)
    hipLaunchKernelGGL(hubert_conv0_apply_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, Nmax, pad, L0max, wav, lens, w, gamma, beta, eps, ws,
                       (float*)out);
  else
    hipLaunchKernelGGL(hubert_conv0_apply_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, Nmax, pad, L0max, wav, lens, w, gamma, beta, eps, ws,
                       (bf16_t*)out);
  S2S_CHECK_LAUNCH("hubert_conv0_apply");
  return 0;
}

extern "C" int s2svc_hubert_logits(int dtype, int B, int L, int K, int log_softmax, const void* units, const int32_t* lens, const float* emb, float* out,
                                   void* stream) {
  S2S_REQUIRE(dtype == S2S_F32 || dtype == S2S_BF16, "hubert_logits: fp32 or bf16 units");
  S2S_REQUIRE(B >= 1 && L >= 1 && (int64_t)B * L < (1ll << 31) - 4 && K >= 1 && K <= HB_KMAX, "hubert_logits: B, L >= 1, 1 <= K <= 256");
  S2S_REQUIRE(units && emb && out && aligned16(emb), "hubert_logits: units, emb (16-byte aligned) and out are required");
  const int rows = B * L;
  if (dtype == S2S_F32)
    hipLaunchKernelGGL(hubert_logits_kernel<float>, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, rows, L, K, log_softmax, (const float*)units, lens,
                       emb, out);
  else
    hipLaunchKernelGGL(hubert_logits_kernel<bf16_t>, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, rows, L, K, log_softmax, (const bf16_t*)units,
                       lens, emb, out);
  S2S_CHECK_LAUNCH("hubert_logits");
  return 0;
}
