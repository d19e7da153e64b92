// BatchNorm1d over (B*T) channel-last rows: the scalar kernels (fp32 / bf16, any C) and the 16-byte bf16 family with the activation
// and dropout of the Postnet fused in.  Statistics are the two-stage column sums of colsum.h; stage 1 of the scalar path is
// colreduce mode 6 (norm.hip).
#include "colsum.h"
#include "../../include/s2svc_hip.h"

namespace {

constexpr int CT = 64;

// ------------------------------------------------------------------------------------------------
// BatchNorm1d apply (channel-last rows): y = dropout(act((x-mean[c])*rstd[c]*gamma[c]+beta[c]))
// reference: modules/pre_postnets.py:108-165 (Conv1d->BatchNorm1d->Tanh->Dropout) and
// modules/conformer/convolution.py:73-75 (BatchNorm1d -> Swish).  Padded frames are part of the
// statistics exactly as in the reference (no masking).
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void bn_apply_kernel(int64_t total, int C, const T* __restrict__ x, const float* __restrict__ mean,
                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                const float* __restrict__ beta, int act, float p, const uint64_t* seed_base, uint64_t seed_off, T* __restrict__ y,
                                T* __restrict__ pre_act, int Tn, const int32_t* __restrict__ vlens) {
  const uint64_t seed = (seed_base ? *seed_base : 0ull) + seed_off;
  const float inv_keep = p > 0.f ? 1.f / (1.f - p) : 1.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    if (vlens && !row_present((int)(i / C), Tn, vlens)) {      // absent frame (common.h): the next convolution's zero padding
      if (pre_act) stf(pre_act + i, 0.f);
      stf(y + i, 0.f);
      continue;
    }
    float v = (ldf(x + i) - mean[c]) * rstd[c] * gamma[c] + beta[c];
    if (pre_act) stf(pre_act + i, v);
    v = act_apply(v, act);
    if (p > 0.f) v = drop_mul(v, dropout_scale(seed, (uint64_t)i, p, inv_keep));
    stf(y + i, v);
  }
}

// dx = gamma*rstd*(dy - sum_dy/N - xhat*sum_dy_xhat/N)   (training-mode BatchNorm backward)
// eval mode (use_batch_stats = 0): dx = gamma*rstd*dy
template <typename T>
__global__ void bn_bwd_kernel(int64_t total, int C, float inv_n, const T* __restrict__ dy, const T* __restrict__ x,
                              const float* __restrict__ mean, const float* __restrict__ rstd,
                              const float* __restrict__ gamma, const float* __restrict__ sum_dy,
                              const float* __restrict__ sum_dy_xhat, int use_batch_stats, T* __restrict__ dx, int Tn,
                              const int32_t* __restrict__ vlens) {
  if (vlens) inv_n = 1.0f / (float)rows_present((int)(total / C), Tn, vlens);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    if (vlens && !row_present((int)(i / C), Tn, vlens)) {      // absent frame: no gradient leaves it
      stf(dx + i, 0.f);
      continue;
    }
    float g = ldf(dy + i);
    float v;
    if (use_batch_stats) {
      float xh = (ldf(x + i) - mean[c]) * rstd[c];
      v = gamma[c] * rstd[c] * (g - sum_dy[c] * inv_n - xh * sum_dy_xhat[c] * inv_n);
    } else {
      v = gamma[c] * rstd[c] * g;
    }
    stf(dx + i, v);
  }
}

// var (biased; var_is_ex2: E[x^2] of the one-pass statistics) -> rstd, and the running-statistics update of torch.nn.BatchNorm1d
// (colsum.h: bn_finalize_channel)
__global__ void bn_finalize_kernel(int C, int n, float eps, float momentum, const float* __restrict__ mean,
                                   const float* __restrict__ var, float* __restrict__ rstd, float* __restrict__ run_mean,
                                   float* __restrict__ run_var, int64_t* __restrict__ num_batches, int var_is_ex2, int Tn,
                                   const int32_t* __restrict__ vlens) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  n = rows_present(n, Tn, vlens);
  if (c == 0 && num_batches) *num_batches += 1;
  if (c >= C) return;
  bn_finalize_channel<false>(c, mean[c], var[c], var_is_ex2 != 0, n, eps, momentum, rstd, run_mean, run_var);
}

// One-pass training statistics, second half: the stage-2 sum of the chunk partials (sum x, sum x^2 -- colsum.h, the same order of
// additions as colreduce_stage2) and bn_finalize_kernel's arithmetic in ONE launch.
__global__ __launch_bounds__(256) void bn_stage2_finalize_kernel(int C, int chunks, const float* __restrict__ ws, int n, float eps,
                                                                 float momentum, float* __restrict__ mean, float* __restrict__ rstd,
                                                                 float* __restrict__ run_mean, float* __restrict__ run_var,
                                                                 int64_t* __restrict__ num_batches, int Tn,
                                                                 const int32_t* __restrict__ vlens) {
  __shared__ float sh[2][4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  n = rows_present(n, Tn, vlens);
  float t0, t1;
  const bool mine = colsum_finish(C, chunks, ws, blockIdx.x, sh, t0, t1);
  if (blockIdx.x == 0 && threadIdx.x == 0 && num_batches) *num_batches += 1;
  if (!mine) return;
  const float scale = 1.0f / (float)n;
  const float m = t0 * scale;
  mean[c] = m;
  bn_finalize_channel<true>(c, m, t1 * scale, true, n, eps, momentum, rstd, run_mean, run_var);
}

// sum of the chunk partials -> sdy, sdyx; optionally accumulated into the gradient slots of beta / gamma
__global__ __launch_bounds__(256) void colsum_pair_kernel(int C, int chunks, const float* __restrict__ ws, float* __restrict__ sdy,
                                                          float* __restrict__ sdyx, float* __restrict__ dbeta_acc,
                                                          float* __restrict__ dgamma_acc) {
  __shared__ float sh[2][4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  float t0, t1;
  if (!colsum_finish(C, chunks, ws, blockIdx.x, sh, t0, t1)) return;
  sdy[c] = t0;
  sdyx[c] = t1;
  if (dbeta_acc) dbeta_acc[c] += t0;
  if (dgamma_acc) dgamma_acc[c] += t1;
}

__global__ void rstd_from_var_kernel(int C, float eps, const float* __restrict__ var, float* __restrict__ rstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) rstd[c] = 1.0f / sqrtf(var[c] + eps);
}

// ---------------------------------------------------------------------------------------------------------
// BatchNorm1d (training) + activation + dropout on channel-last rows, bf16, C % 8 == 0, in 16-byte accesses -- the Postnet layers
// (pre_postnets.py:108-165: Conv1d -> BatchNorm1d -> Tanh -> Dropout).  Same launch count forward as the scalar kernels above
// (statistics, finalize, apply) but vector loads; backward 3 launches instead of 4 + 2: the activation / dropout derivative is
// recomputed inside the statistics pass and inside the data-gradient pass instead of being written by a kernel of its own, and the
// BatchNorm parameter gradients are added to their slots by the reduction's second stage.
// A workgroup = 64 channels (8 vector lanes) x 64 rows; sums in a fixed order (colsum.h: colsum_reduce8).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_stats_vec_kernel(int rows, int C, const bf16_t* __restrict__ x, float* __restrict__ ws, int rpc,
                                                           int Tn, const int32_t* __restrict__ vlens) {
  __shared__ float sh[2][4][CT];
  const int v = threadIdx.x & 7, r8 = threadIdx.x >> 3;
  const int c = blockIdx.x * CT + v * 8;
  const int r0 = blockIdx.y * rpc;
  const int r1 = r0 + rpc < rows ? r0 + rpc : rows;
  float a0[8], a1[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a0[e] = a1[e] = 0.f;
  if (c < C) {
#pragma unroll 4
    for (int r = r0 + r8; r < r1; r += 32) {
      if (!row_present(r, Tn, vlens)) continue;
      float f[8];
      unpack_bf16x8(*reinterpret_cast<const uint4*>(x + (int64_t)r * C + c), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) { a0[e] += f[e]; a1[e] += f[e] * f[e]; }
    }
  }
  colsum_reduce8(a0, a1, sh, blockIdx.y, C, blockIdx.x * CT, ws);
}

// y = dropout(act((x - mean) * rstd * gamma + beta)); pre_act (optional) = the BatchNorm output before the activation
__global__ __launch_bounds__(256) void bn_act_apply_vec_kernel(int rows, int C, const bf16_t* __restrict__ x, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, int act, float p,
                                                               const uint64_t* seed_base, uint64_t seed_off, bf16_t* __restrict__ y,
                                                               bf16_t* __restrict__ pre_act, int rows_per_wg, int Tn,
                                                               const int32_t* __restrict__ vlens) {
  const int v = threadIdx.x & 7, r8 = threadIdx.x >> 3;
  const int c = blockIdx.x * CT + v * 8;
  if (c >= C) return;
  const int r0 = blockIdx.y * rows_per_wg;
  const int r1 = r0 + rows_per_wg < rows ? r0 + rows_per_wg : rows;
  const uint64_t seed = (seed_base ? *seed_base : 0ull) + seed_off;
  const float inv_keep = p > 0.f ? 1.f / (1.f - p) : 1.f;
  float m[8], rs[8], ga[8], be[8];
  ldp8(mean + c, m);
  ldp8(rstd + c, rs);
  ldp8(gamma + c, ga);
  ldp8(beta + c, be);
#pragma unroll 2
  for (int r = r0 + r8; r < r1; r += 32) {
    const int64_t o = (int64_t)r * C + c;
    float f[8], mk[8];
    if (!row_present(r, Tn, vlens)) {               // absent frame: the next convolution's zero padding
      if (pre_act) *reinterpret_cast<uint4*>(pre_act + o) = make_uint4(0, 0, 0, 0);
      *reinterpret_cast<uint4*>(y + o) = make_uint4(0, 0, 0, 0);
      continue;
    }
    unpack_bf16x8(*reinterpret_cast<const uint4*>(x + o), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (f[e] - m[e]) * rs[e] * ga[e] + be[e];
    if (pre_act) *reinterpret_cast<uint4*>(pre_act + o) = pack_bf16x8(f);
    if (p > 0.f) dropout_scale8(seed, (uint64_t)o, p, inv_keep, mk);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      f[e] = act_apply(f[e], act);
      if (p > 0.f) f[e] = drop_mul(f[e], mk[e]);
    }
    *reinterpret_cast<uint4*>(y + o) = pack_bf16x8(f);
  }
}

// g = dz * mask * act'(saved);  per-chunk sums of g and g * xhat
__global__ __launch_bounds__(256) void bn_act_bwd_stats_kernel(int rows, int C, const bf16_t* __restrict__ dz, const bf16_t* __restrict__ saved,
                                                               const bf16_t* __restrict__ x, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, int act, float p,
                                                               const uint64_t* seed_base, uint64_t seed_off, float* __restrict__ ws, int rpc,
                                                               int Tn, const int32_t* __restrict__ vlens) {
  __shared__ float sh[2][4][CT];
  const int v = threadIdx.x & 7, r8 = threadIdx.x >> 3;
  const int c = blockIdx.x * CT + v * 8;
  const int r0 = blockIdx.y * rpc;
  const int r1 = r0 + rpc < rows ? r0 + rpc : rows;
  const uint64_t seed = (seed_base ? *seed_base : 0ull) + seed_off;
  const float inv_keep = p > 0.f ? 1.f / (1.f - p) : 1.f;
  float a0[8], a1[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a0[e] = a1[e] = 0.f;
  if (c < C) {
    float m[8], rs[8];
    ldp8(mean + c, m);
    ldp8(rstd + c, rs);
#pragma unroll 2
    for (int r = r0 + r8; r < r1; r += 32) {
      if (!row_present(r, Tn, vlens)) continue;
      const int64_t o = (int64_t)r * C + c;
      float g[8], sd[8], xx[8], mk[8];
      unpack_bf16x8(*reinterpret_cast<const uint4*>(dz + o), g);
      if (saved) unpack_bf16x8(*reinterpret_cast<const uint4*>(saved + o), sd);
      unpack_bf16x8(*reinterpret_cast<const uint4*>(x + o), xx);
      if (p > 0.f) dropout_scale8(seed, (uint64_t)o, p, inv_keep, mk);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float mm = p > 0.f ? mk[e] : 1.f;
        const float gg = g[e] * mm * (saved ? act_grad_from_saved(sd[e], mm, act) : 1.f);
        a0[e] += gg;
        a1[e] += gg * (xx[e] - m[e]) * rs[e];
      }
    }
  }
  colsum_reduce8(a0, a1, sh, blockIdx.y, C, blockIdx.x * CT, ws);
}

// dx = gamma * rstd * (g - sum_g / N - xhat * sum_g_xhat / N), g recomputed as above
__global__ __launch_bounds__(256) void bn_act_bwd_apply_kernel(int rows, int C, const bf16_t* __restrict__ dz,
                                                               const bf16_t* __restrict__ saved, const bf16_t* __restrict__ x,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ gamma, const float* __restrict__ sdy,
                                                               const float* __restrict__ sdyx, int act, float p,
                                                               const uint64_t* seed_base, uint64_t seed_off, bf16_t* __restrict__ dx,
                                                               int rows_per_wg, int Tn, const int32_t* __restrict__ vlens) {
  const int v = threadIdx.x & 7, r8 = threadIdx.x >> 3;
  const int c = blockIdx.x * CT + v * 8;
  if (c >= C) return;
  const float inv_n = 1.0f / (float)rows_present(rows, Tn, vlens);
  const int r0 = blockIdx.y * rows_per_wg;
  const int r1 = r0 + rows_per_wg < rows ? r0 + rows_per_wg : rows;
  const uint64_t seed = (seed_base ? *seed_base : 0ull) + seed_off;
  const float inv_keep = p > 0.f ? 1.f / (1.f - p) : 1.f;
  float m[8], rs[8], k1[8], k2[8], k3[8];
  ldp8(mean + c, m);
  ldp8(rstd + c, rs);
  ldp8(gamma + c, k1);
  ldp8(sdy + c, k2);
  ldp8(sdyx + c, k3);
#pragma unroll
  for (int e = 0; e < 8; ++e) { k1[e] *= rs[e]; k2[e] *= inv_n; k3[e] *= inv_n; }
#pragma unroll 2
  for (int r = r0 + r8; r < r1; r += 32) {
    const int64_t o = (int64_t)r * C + c;
    float g[8], sd[8], xx[8], mk[8];
    if (!row_present(r, Tn, vlens)) {               // absent frame: no gradient leaves it
      *reinterpret_cast<uint4*>(dx + o) = make_uint4(0, 0, 0, 0);
      continue;
    }
    unpack_bf16x8(*reinterpret_cast<const uint4*>(dz + o), g);
    if (saved) unpack_bf16x8(*reinterpret_cast<const uint4*>(saved + o), sd);
    unpack_bf16x8(*reinterpret_cast<const uint4*>(x + o), xx);
    if (p > 0.f) dropout_scale8(seed, (uint64_t)o, p, inv_keep, mk);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float mm = p > 0.f ? mk[e] : 1.f;
      const float gg = g[e] * mm * (saved ? act_grad_from_saved(sd[e], mm, act) : 1.f);
      g[e] = k1[e] * (gg - k2[e] - (xx[e] - m[e]) * rs[e] * k3[e]);
    }
    *reinterpret_cast<uint4*>(dx + o) = pack_bf16x8(g);
  }
}

// rows per statistics chunk: 64 for short inputs, more (a multiple of 32) so that there are at most 64 chunk partials to sum
int bn_rows_per_chunk(int rows) {
  int rpc = ((rows + 63) / 64 + 31) / 32 * 32;
  return rpc < 64 ? 64 : rpc;
}

}  // namespace

int s2s_bn_stage2_finalize(int C, int chunks, const float* ws, int rows, float eps, float momentum, float* mean, float* rstd,
                           float* run_mean, float* run_var, int64_t* num_batches, int Tn, const int32_t* vlens, hipStream_t st) {
  hipLaunchKernelGGL(bn_stage2_finalize_kernel, dim3((C + 63) / 64), dim3(256), 0, st, C, chunks, ws, rows, eps, momentum, mean, rstd,
                     run_mean, run_var, num_batches, Tn, vlens);
  S2S_CHECK_LAUNCH("bn_stage2_finalize_kernel");
  return 0;
}

int s2s_colsum_pair(int C, int chunks, const float* ws, float* sdy, float* sdyx, float* dbeta_acc, float* dgamma_acc, hipStream_t st) {
  hipLaunchKernelGGL(colsum_pair_kernel, dim3((C + 63) / 64), dim3(256), 0, st, C, chunks, ws, sdy, sdyx, dbeta_acc, dgamma_acc);
  S2S_CHECK_LAUNCH("colsum_pair_kernel");
  return 0;
}

extern "C" int s2svc_bn_finalize(int C, int n, float eps, float momentum, const float* mean, const float* var,
                                 float* rstd, float* run_mean, float* run_var, int64_t* num_batches, int var_is_ex2, int Tn,
                                 const int32_t* vlens, void* stream) {
  S2S_REQUIRE(!vlens || (Tn > 0 && n % Tn == 0), "bn_finalize: vlens needs n = B * Tn");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, C, n, eps, momentum,
                     mean, var, rstd, run_mean, run_var, num_batches, var_is_ex2, Tn, vlens);
  S2S_CHECK_LAUNCH("bn_finalize_kernel");
  return 0;
}

// mean / rstd of a training-mode BatchNorm1d over (rows, C) in TWO launches (one pass over x: fp32 sums of x and x^2 per chunk,
// then sum of the partials + variance + rstd + running statistics); ws >= ws_chunks*2*C floats.  Same values as
// s2svc_colreduce(mode 6, scale 1/rows) + s2svc_bn_finalize(var_is_ex2 = 1), one launch less.  (Stage 1 never takes the 16-byte
// kernel: s2svc_bn_stats_vec is the 16-byte path.)
extern "C" int s2svc_bn_stats(int dtype, int rows, int C, const void* x, float eps, float momentum, float* mean, float* rstd,
                              float* run_mean, float* run_var, int64_t* num_batches, float* ws, int ws_chunks, int Tn,
                              const int32_t* vlens, void* stream) {
  S2S_REQUIRE(rows > 0 && C > 0 && x && mean && rstd && ws && ws_chunks > 0, "bn_stats: bad args");
  S2S_REQUIRE(!vlens || (Tn > 0 && rows % Tn == 0), "bn_stats: vlens needs rows = B * Tn");
  S2S_REQUIRE(dtype == S2S_F32 || dtype == S2S_BF16, "bn_stats: bad dtype");
  hipStream_t st = (hipStream_t)stream;
  int chunks = 0;
  if (const int rc = s2s_colreduce_stage1(dtype, rows, C, 6, nullptr, x, nullptr, nullptr, ws, ws_chunks, Tn, vlens, false, st, &chunks))
    return rc;
  return s2s_bn_stage2_finalize(C, chunks, ws, rows, eps, momentum, mean, rstd, run_mean, run_var, num_batches, Tn, vlens, st);
}

extern "C" int s2svc_rstd_from_var(int C, float eps, const float* var, float* rstd, void* stream) {
  hipLaunchKernelGGL(rstd_from_var_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, C, eps, var, rstd);
  S2S_CHECK_LAUNCH("rstd_from_var_kernel");
  return 0;
}

extern "C" int s2svc_bn_apply(int dtype, int64_t rows, int C, const void* x, const float* mean, const float* rstd,
                              const float* gamma, const float* beta, int act, float drop_p, const uint64_t* seed_base, uint64_t seed_off, void* y,
                              void* pre_act, int Tn, const int32_t* vlens, void* stream) {
  const int64_t total = rows * C;
  if (total == 0) return 0;
  S2S_REQUIRE(!vlens || (Tn > 0 && rows % Tn == 0 && rows < (1ll << 31)), "bn_apply: vlens needs rows = B * Tn");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == S2S_F32)
    hipLaunchKernelGGL(bn_apply_kernel<float>, dim3(ew_blocks(total)), dim3(256), 0, st, total, C, (const float*)x, mean,
                       rstd, gamma, beta, act, drop_p, seed_base, seed_off, (float*)y, (float*)pre_act, Tn, vlens);
  else
    hipLaunchKernelGGL(bn_apply_kernel<bf16_t>, dim3(ew_blocks(total)), dim3(256), 0, st, total, C, (const bf16_t*)x, mean,
                       rstd, gamma, beta, act, drop_p, seed_base, seed_off, (bf16_t*)y, (bf16_t*)pre_act, Tn, vlens);
  S2S_CHECK_LAUNCH("bn_apply_kernel");
  return 0;
}

extern "C" int s2svc_bn_bwd(int dtype, int64_t rows, int C, const void* dy, const void* x, const float* mean,
                            const float* rstd, const float* gamma, const float* sum_dy, const float* sum_dy_xhat,
                            int use_batch_stats, void* dx, int Tn, const int32_t* vlens, void* stream) {
  const int64_t total = rows * C;
  if (total == 0) return 0;
  S2S_REQUIRE(!vlens || (Tn > 0 && rows % Tn == 0 && rows < (1ll << 31)), "bn_bwd: vlens needs rows = B * Tn");
  hipStream_t st = (hipStream_t)stream;
  const float inv_n = 1.0f / (float)rows;
  if (dtype == S2S_F32)
    hipLaunchKernelGGL(bn_bwd_kernel<float>, dim3(ew_blocks(total)), dim3(256), 0, st, total, C, inv_n, (const float*)dy,
                       (const float*)x, mean, rstd, gamma, sum_dy, sum_dy_xhat, use_batch_stats, (float*)dx, Tn, vlens);
  else
    hipLaunchKernelGGL(bn_bwd_kernel<bf16_t>, dim3(ew_blocks(total)), dim3(256), 0, st, total, C, inv_n, (const bf16_t*)dy,
                       (const bf16_t*)x, mean, rstd, gamma, sum_dy, sum_dy_xhat, use_batch_stats, (bf16_t*)dx, Tn, vlens);
  S2S_CHECK_LAUNCH("bn_bwd_kernel");
  return 0;
}

// ---- BatchNorm1d (training) + activation + dropout, bf16, C % 8 == 0 (see above) ----
// mean / rstd of x (rows, C) + running statistics: two launches.  ws >= ceil(rows / 64) * 2 * C floats.
extern "C" int s2svc_bn_stats_vec(int rows, int C, const void* x, float eps, float momentum, float* mean, float* rstd, float* run_mean,
                                  float* run_var, int64_t* num_batches, float* ws, int Tn, const int32_t* vlens, void* stream) {
  S2S_REQUIRE(rows > 0 && C > 0 && C % 8 == 0 && x && mean && rstd && ws && aligned16(x), "bn_stats_vec: bad args (bf16, C % 8 == 0)");
  S2S_REQUIRE(!vlens || (Tn > 0 && rows % Tn == 0), "bn_stats_vec: vlens needs rows = B * Tn");
  hipStream_t st = (hipStream_t)stream;
  const int rpc = bn_rows_per_chunk(rows), chunks = (rows + rpc - 1) / rpc, ct = (C + CT - 1) / CT;
  hipLaunchKernelGGL(bn_stats_vec_kernel, dim3(ct, chunks), dim3(256), 0, st, rows, C, (const bf16_t*)x, ws, rpc, Tn, vlens);
  S2S_CHECK_LAUNCH("bn_stats_vec_kernel");
  return s2s_bn_stage2_finalize(C, chunks, ws, rows, eps, momentum, mean, rstd, run_mean, run_var, num_batches, Tn, vlens, st);
}

extern "C" int s2svc_bn_act_apply_vec(int rows, int C, const void* x, const float* mean, const float* rstd, const float* gamma,
                                      const float* beta, int act, float drop_p, const uint64_t* seed_base, uint64_t seed_off, void* y,
                                      void* pre_act, int Tn, const int32_t* vlens, void* stream) {
  S2S_REQUIRE(!vlens || (Tn > 0 && rows % Tn == 0), "bn_act_apply_vec: vlens needs rows = B * Tn");
  S2S_REQUIRE(rows > 0 && C > 0 && C % 8 == 0 && x && mean && rstd && gamma && beta && y && aligned16(x) && aligned16(y) &&
              aligned16(pre_act), "bn_act_apply_vec: bad args (bf16, C % 8 == 0)");
  const int rpw = 128;
  hipLaunchKernelGGL(bn_act_apply_vec_kernel, dim3((C + CT - 1) / CT, (rows + rpw - 1) / rpw), dim3(256), 0, (hipStream_t)stream, rows, C,
                     (const bf16_t*)x, mean, rstd, gamma, beta, act, drop_p, seed_base, seed_off, (bf16_t*)y, (bf16_t*)pre_act, rpw, Tn,
                     vlens);
  S2S_CHECK_LAUNCH("bn_act_apply_vec_kernel");
  return 0;
}

// dz = gradient of y = dropout(act(BN(x))); saved = y (relu / tanh / sigmoid) or the pre-activation (swish / gelu), NULL for act none
// without dropout.  -> dx, sdy = sum g, sdyx = sum g * xhat (the gradients of beta / gamma, also ADDED to dbeta_acc / dgamma_acc when
// given).  Three launches.  ws >= ceil(rows / 64) * 2 * C floats.
extern "C" int s2svc_bn_act_bwd_vec(int rows, int C, const void* dz, const void* saved, const void* x, const float* mean, const float* rstd,
                                    const float* gamma, int act, float drop_p, const uint64_t* seed_base, uint64_t seed_off, void* dx,
                                    float* sdy, float* sdyx, float* dgamma_acc, float* dbeta_acc, float* ws, int Tn, const int32_t* vlens,
                                    void* stream) {
  S2S_REQUIRE(!vlens || (Tn > 0 && rows % Tn == 0), "bn_act_bwd_vec: vlens needs rows = B * Tn");
  S2S_REQUIRE(rows > 0 && C > 0 && C % 8 == 0 && dz && x && mean && rstd && gamma && dx && sdy && sdyx && ws && aligned16(dz) &&
              aligned16(saved) && aligned16(x) && aligned16(dx) && (saved || act == S2S_ACT_NONE), "bn_act_bwd_vec: bad args (bf16, C % 8 == 0)");
  hipStream_t st = (hipStream_t)stream;
  const int rpc = bn_rows_per_chunk(rows), chunks = (rows + rpc - 1) / rpc, ct = (C + CT - 1) / CT;
  hipLaunchKernelGGL(bn_act_bwd_stats_kernel, dim3(ct, chunks), dim3(256), 0, st, rows, C, (const bf16_t*)dz, (const bf16_t*)saved,
                     (const bf16_t*)x, mean, rstd, act, drop_p, seed_base, seed_off, ws, rpc, Tn, vlens);
  S2S_CHECK_LAUNCH("bn_act_bwd_stats_kernel");
  if (const int rc = s2s_colsum_pair(C, chunks, ws, sdy, sdyx, dbeta_acc, dgamma_acc, st)) return rc;
  const int rpw = 128;
  hipLaunchKernelGGL(bn_act_bwd_apply_kernel, dim3(ct, (rows + rpw - 1) / rpw), dim3(256), 0, st, rows, C,
                     (const bf16_t*)dz, (const bf16_t*)saved, (const bf16_t*)x, mean, rstd, gamma, sdy, sdyx, act, drop_p, seed_base,
                     seed_off, (bf16_t*)dx, rpw, Tn, vlens);
  S2S_CHECK_LAUNCH("bn_act_bwd_apply_kernel");
  return 0;
}
