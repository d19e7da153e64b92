// The two-stage per-channel column sum of the training path, once: one partial-sum format, one order of additions, one BatchNorm
// finalisation.  Used by norm.hip (colreduce: the LayerNorm / BatchNorm / bias gradients), batchnorm.hip (the BatchNorm statistics,
// scalar and 16-byte), convmod.hip (the statistics inside the Conformer convolution module) and dwconv.hip.
//   stage 1  a workgroup of four waves owns a chunk of rows and writes a PAIR of partial rows ws[chunk][2][C] (two sums per column, e.g.
//            sum x and sum x^2): every wave adds its rows one after the other, the four waves are added as ((w0 + w1) + w2) + w3.
//   stage 2  64 columns x 4 chunk groups per workgroup: group kg adds the chunks k = kg, kg + 4, ... (independent loads), the four
//            groups are added as ((g0 + g1) + g2) + g3.
// The order is fixed, so a training step is reproducible bit for bit; tests/colsum_ref.py restates it in float32 on the CPU and
// tests/gpu_colsum_check.py holds the kernels to that restatement bit for bit.
#pragma once
#include "common.h"

// the four waves' (stage 1) or four chunk groups' (stage 2) sums of one column, in THE order
template <int W>
__device__ __forceinline__ float colsum_comb4(const float (&sh)[4][W], int col) {
  return ((sh[0][col] + sh[1][col]) + sh[2][col]) + sh[3][col];
}

// Stage-1 tail, one column per lane (c = c0 + cl, wave = the row group): the wave's two sums -> LDS, wave 0 adds the four waves and
// stores the pair of partial rows.
__device__ __forceinline__ void colsum_store_pair(float s0, float s1, float (&sh)[2][4][64], int wave, int cl, int chunk, int C, int c,
                                                  float* __restrict__ ws) {
  sh[0][wave][cl] = s0;
  sh[1][wave][cl] = s1;
  __syncthreads();
  if (wave == 0 && c < C) {
    ws[((int64_t)chunk * 2 + 0) * C + c] = colsum_comb4(sh[0], cl);
    ws[((int64_t)chunk * 2 + 1) * C + c] = colsum_comb4(sh[1], cl);
  }
}
// ... eight consecutive columns per lane (a wave covers 512 columns from c0): 512 columns x 2 sums, thread t combines column t
// (sum 0) and column t (sum 1) of its half
__device__ __forceinline__ void colsum_store_pair(const float (&s0)[8], const float (&s1)[8], float (&sh)[2][4][512], int wave, int lane,
                                                  int chunk, int C, int c0, float* __restrict__ ws) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sh[0][wave][lane * 8 + e] = s0[e];
    sh[1][wave][lane * 8 + e] = s1[e];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 1024; i += 256) {
    const int which = i >> 9, col = i & 511;
    if (c0 + col < C) ws[((int64_t)chunk * 2 + which) * C + c0 + col] = colsum_comb4(sh[which], col);
  }
}

// Stage-1 tail of the 16-byte kernels whose workgroup is 8 vector lanes (8 channels each, from c0) x 32 rows: a0 / a1 hold a lane's
// sums over its rows; lanes with the same vector lane hold the wave's 8 rows: butterfly over lane bits 3..5, then the four waves.
// ALL 64 LANES of every wave must arrive here (common.h): callers keep it outside their `c < C` branches.
__device__ __forceinline__ void colsum_reduce8(float (&a0)[8], float (&a1)[8], float (&sh)[2][4][64], int chunk, int C, int c0,
                                               float* __restrict__ ws) {
  const int v = threadIdx.x & 7, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    a0[e] = xor32_sum(xor16_sum(xor8_sum(a0[e])));      // (DPP / permlane swaps instead of ds_bpermute, common.h)
    a1[e] = xor32_sum(xor16_sum(xor8_sum(a1[e])));
  }
  if (lane < 8) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { sh[0][wave][v * 8 + e] = a0[e]; sh[1][wave][v * 8 + e] = a1[e]; }
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int cl = threadIdx.x, cc = c0 + cl;
    if (cc < C) {
      ws[((int64_t)chunk * 2 + 0) * C + cc] = colsum_comb4(sh[0], cl);
      ws[((int64_t)chunk * 2 + 1) * C + cc] = colsum_comb4(sh[1], cl);
    }
  }
}

// Stage 2 for the 64 columns from bx * 64 (256 threads): each thread sums every 4th chunk partial, the four groups are combined
// through LDS.  True for the lanes (group 0, c < C) that then hold the column's two totals in t0 / t1.
__device__ __forceinline__ bool colsum_finish(int C, int chunks, const float* __restrict__ ws, int bx, float (&sh)[2][4][64], float& t0,
                                              float& t1) {
  const int cl = threadIdx.x & 63, kg = threadIdx.x >> 6;
  const int c = bx * 64 + cl;
  t0 = 0.f;
  t1 = 0.f;
  if (c < C) {
#pragma unroll 8
    for (int k = kg; k < chunks; k += 4) {        // same order of additions, 16 loads in flight
      t0 += ws[((int64_t)k * 2 + 0) * C + c];
      t1 += ws[((int64_t)k * 2 + 1) * C + c];
    }
  }
  sh[0][kg][cl] = t0;
  sh[1][kg][cl] = t1;
  __syncthreads();
  if (kg != 0 || c >= C) return false;
  t0 = colsum_comb4(sh[0], cl);
  t1 = colsum_comb4(sh[1], cl);
  return true;
}

// Single partial rows ws[chunk][n] (the depthwise weight gradients): the sum over the chunks of value i, one after the other.
__device__ __forceinline__ float colsum_partials(const float* __restrict__ ws, int chunks, int n, int i) {
  float t = 0.f;
#pragma unroll 16
  for (int k = 0; k < chunks; ++k) t += ws[(int64_t)k * n + i];      // same order of additions, 16 loads in flight
  return t;
}

// torch.nn.BatchNorm1d's finalisation for channel c: m = the batch mean, v = the biased variance, or E[x^2] (one-pass statistics:
// biased variance = E[x^2] - mean^2, clamped at 0) -> rstd and the running statistics (momentum 0.1 in the models; the UNBIASED
// variance goes into the running buffer, n = the number of rows the statistics are over).
// The running mean (1 - momentum) * run_mean + momentum * m is one multiply and one fused multiply-add, and the two kernels have
// always differed in which product the fma absorbs (the compiler chose by the order of their loads).  Written out, so that each keeps
// its bits whatever the compiler does: FMA_ON_MEAN (the stage-2 kernel) = fma(momentum, m, (1 - momentum) * run_mean), else
// (bn_finalize_kernel) fma(1 - momentum, run_mean, momentum * m).  tests/gpu_colsum_check.py dumps both for a byte comparison.
template <bool FMA_ON_MEAN>
__device__ __forceinline__ void bn_finalize_channel(int c, float m, float v, bool v_is_ex2, int n, float eps, float momentum,
                                                    float* __restrict__ rstd, float* __restrict__ run_mean, float* __restrict__ run_var) {
  float vc = v;
  if (v_is_ex2) {
    vc -= m * m;
    vc = vc > 0.f ? vc : 0.f;
  }
  rstd[c] = 1.0f / sqrtf(vc + eps);
  if (run_mean) {
    run_mean[c] = FMA_ON_MEAN ? __builtin_fmaf(momentum, m, (1.f - momentum) * run_mean[c])
                              : __builtin_fmaf(1.f - momentum, run_mean[c], momentum * m);
    const float unb = n > 1 ? vc * ((float)n / (float)(n - 1)) : vc;
    run_var[c] = (1.f - momentum) * run_var[c] + momentum * unb;
  }
}

// Host launchers that cross translation units (C++ linkage, like s2s_gemm_route of gemm_common.h; 0 or the S2S_CHECK_LAUNCH code).
// ws[chunks][2][C] as above.
//   s2s_colreduce_stage1    (norm.hip; also s2svc_bn_stats) stage 1 of a column reduction in `mode`, *chunks = the partial rows written
//   s2s_bn_stage2_finalize  (batchnorm.hip; also convmod.hip) sum x, sum x^2 over `rows` rows -> mean, rstd, running statistics,
//                           num_batches += 1
//   s2s_colsum_pair         (batchnorm.hip; also convmod.hip) the two totals -> sdy, sdyx, ADDED to dbeta_acc / dgamma_acc where given
int s2s_colreduce_stage1(int dtype, int rows, int D, int mode, const void* dy, const void* x, const float* mean, const float* rstd,
                         float* ws, int ws_chunks, int Tn, const int32_t* vlens, bool allow_vec, hipStream_t st, int* chunks);
int s2s_bn_stage2_finalize(int C, int chunks, const float* ws, int rows, float eps, float momentum, float* mean, float* rstd,
                           float* run_mean, float* run_var, int64_t* num_batches, int Tn, const int32_t* vlens, hipStream_t st);
int s2s_colsum_pair(int C, int chunks, const float* ws, float* sdy, float* sdyx, float* dbeta_acc, float* dgamma_acc, hipStream_t st);
