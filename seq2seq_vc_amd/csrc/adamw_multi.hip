// Multi-tensor AdamW (decoupled weight decay, torch.optim.AdamW's formula) over a table of tensors: one launch per group of up to
// S2SVC_ADAMW_GROUP (80) tensors, 3 launches for the HiFi-GAN generator's 234 parameters, 2 for the discriminator's 154.
//
// reference: torch.optim.AdamW as urhythmic_fine_tune_vocoder.py:99-110 builds it (betas 0.8 / 0.99, weight decay 1e-2), stepped per
// tensor by stock torch.  The parameters and their gradients stay the caller's own tensors (gradients are fresh tensors every step),
// so their addresses travel as kernel arguments, a fixed-size table by value: no device table, no copy, no stream stop.  The two
// moments live in two flat fp32 buffers; tensor i owns [off[i], off[i] + numel[i]), off[i] a multiple of 4 elements.
//
// Per element, in fp32 and in torch's order:
//   p <- p * (1 - lr * wd);  m <- m + (1 - beta1) * (g - m);  v <- beta2 * v + (1 - beta2) * g * g
//   p <- p - step_size * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps)),  step_size = lr / (1 - beta1^t)
// `decay` = 1 - lr * wd, `omb1` = 1 - beta1, `omb2` = 1 - beta2 (in fp32 1.f - 0.99f is 3e-6 off: the difference cancels), step_size[i]
// and bc2_sqrt[i] = sqrt(1 - beta2^t_i) are computed by the host in double and rounded once (every tensor has its own step count: a
// tensor without a gradient is not in the table and does not advance).
// A workgroup updates one chunk of 4096 elements of one tensor (1024 and 16384 measured the same, profiles/AB_LOG.md): float4
// accesses when p and g are 16-byte aligned (the moments' chunks always are), element-wise otherwise; the last numel % 4 elements of
// a tensor are handled element-wise, inside its own range.
#include "common.h"
#include "../../include/s2svc_hip.h"

namespace {

constexpr int GROUP = 80;
#ifndef S2SVC_ADAMW_CHUNK
#define S2SVC_ADAMW_CHUNK 4096
#endif
constexpr int CHUNK = S2SVC_ADAMW_CHUNK;   // elements per workgroup, a multiple of 4
constexpr int THREADS = 256;

struct Table {
  float* p[GROUP];
  const float* g[GROUP];
  int64_t off[GROUP];
  int32_t numel[GROUP];
  float step_size[GROUP];
  float bc2_sqrt[GROUP];
  int32_t prefix[GROUP + 1];         // first workgroup of every tensor; prefix[n] = the grid
  int32_t n;
};

__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float decay, float omb1, float beta2, float omb2, float eps,
                                          float step_size, float bc2_sqrt) {
  p = p * decay;
  m = m + omb1 * (g - m);
  v = beta2 * v + omb2 * g * g;
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p = p - step_size * (m / denom);
}

__global__ __launch_bounds__(THREADS) void adamw_multi_kernel(const Table t, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                              float decay, float omb1, float beta2, float omb2, float eps) {
  int lo_e = 0, hi_e = t.n - 1;
  while (lo_e < hi_e) {              // the last tensor whose first workgroup is <= this one
    const int mid = (lo_e + hi_e + 1) >> 1;
    if (t.prefix[mid] <= (int)blockIdx.x) lo_e = mid; else hi_e = mid - 1;
  }
  const int e = lo_e;
  float* __restrict__ p = t.p[e];
  const float* __restrict__ g = t.g[e];
  float* __restrict__ m = exp_avg + t.off[e];
  float* __restrict__ v = exp_avg_sq + t.off[e];
  const float ss = t.step_size[e], bs = t.bc2_sqrt[e];
  const int64_t numel = t.numel[e];
  const int64_t lo = (int64_t)(blockIdx.x - t.prefix[e]) * CHUNK;
  const int64_t hi = lo + CHUNK < numel ? lo + CHUNK : numel;
  int64_t i = lo;
  if ((((uintptr_t)p | (uintptr_t)g) & 15) == 0) {
    const int n4 = (int)((hi - lo) >> 2);
    for (int q = threadIdx.x; q < n4; q += THREADS) {
      const int64_t j = lo + 4 * q;
      float4 pp = *reinterpret_cast<const float4*>(p + j);
      const float4 gg = *reinterpret_cast<const float4*>(g + j);
      float4 mm = *reinterpret_cast<const float4*>(m + j);
      float4 vv = *reinterpret_cast<const float4*>(v + j);
      adamw_one(pp.x, gg.x, mm.x, vv.x, decay, omb1, beta2, omb2, eps, ss, bs);
      adamw_one(pp.y, gg.y, mm.y, vv.y, decay, omb1, beta2, omb2, eps, ss, bs);
      adamw_one(pp.z, gg.z, mm.z, vv.z, decay, omb1, beta2, omb2, eps, ss, bs);
      adamw_one(pp.w, gg.w, mm.w, vv.w, decay, omb1, beta2, omb2, eps, ss, bs);
      *reinterpret_cast<float4*>(m + j) = mm;
      *reinterpret_cast<float4*>(v + j) = vv;
      *reinterpret_cast<float4*>(p + j) = pp;
    }
    i = lo + (n4 << 2);
  }
  for (int64_t j = i + threadIdx.x; j < hi; j += THREADS) {   // the tensor's own tail (or all of it when p / g are not aligned)
    float pj = p[j], mj = m[j], vj = v[j];
    adamw_one(pj, g[j], mj, vj, decay, omb1, beta2, omb2, eps, ss, bs);
    m[j] = mj;
    v[j] = vj;
    p[j] = pj;
  }
}

}  // namespace

extern "C" int s2svc_adamw_multi_group(void) { return GROUP; }
extern "C" int s2svc_adamw_multi_chunk(void) { return CHUNK; }

// table: n rows of 4 int64 on the HOST: address of the parameter, address of its gradient, offset of its moments, numel.
// A refused call launches nothing.
extern "C" int s2svc_adamw_multi(int n, const int64_t* table, const int32_t* prefix, const float* step_size, const float* bc2_sqrt,
                                 int64_t moment_numel, float* exp_avg, float* exp_avg_sq, float decay, float one_minus_beta1, float beta2,
                                 float one_minus_beta2, float eps, void* stream) {
  S2S_REQUIRE(n >= 1 && n <= GROUP && table && prefix && step_size && bc2_sqrt && exp_avg && exp_avg_sq && prefix[0] == 0,
              "adamw_multi: 1 .. 80 tensors per call, host tables, device moments");
  S2S_REQUIRE((((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0, "adamw_multi: 16-byte aligned moment buffers");
  Table t;
  t.n = n;
  for (int e = 0; e < n; ++e) {
    const int64_t* r = table + 4 * e;
    const int64_t off = r[2], numel = r[3];
    S2S_REQUIRE(r[0] && r[1] && numel >= 1 && numel < (1ll << 31) && off >= 0 && off % 4 == 0 && off + numel <= moment_numel &&
                    (int64_t)prefix[e + 1] - (int64_t)prefix[e] == (numel + CHUNK - 1) / CHUNK && (r[0] % 4 == 0) && (r[1] % 4 == 0),
                "adamw_multi: every row is (parameter, gradient, moment offset a multiple of 4 inside the buffers, numel >= 1) and the "
                "prefix table counts its 4096-element chunks");
    t.p[e] = (float*)(uintptr_t)r[0];
    t.g[e] = (const float*)(uintptr_t)r[1];
    t.off[e] = off;
    t.numel[e] = (int32_t)numel;
    t.step_size[e] = step_size[e];
    t.bc2_sqrt[e] = bc2_sqrt[e];
    t.prefix[e] = prefix[e];
  }
  t.prefix[n] = prefix[n];
  for (int e = n; e < GROUP; ++e) {
    t.p[e] = nullptr;
    t.g[e] = nullptr;
    t.off[e] = 0;
    t.numel[e] = 0;
    t.step_size[e] = t.bc2_sqrt[e] = 0.f;
    t.prefix[e + 1] = prefix[n];
  }
  hipLaunchKernelGGL(adamw_multi_kernel, dim3((unsigned)prefix[n]), dim3(THREADS), 0, (hipStream_t)stream, t, exp_avg, exp_avg_sq, decay,
                     one_minus_beta1, beta2, one_minus_beta2, eps);
  S2S_CHECK_LAUNCH("adamw_multi_kernel");
  return 0;
}
