// The three GAN losses of the HiFi-GAN fine-tuning loop, table-driven: every tensor (pair) of a call goes through ONE launch.
//
// reference: urhythmic/vocoder.py:428-465 -- feature_loss (54 means of |r - g| and their sum), discriminator_loss (eight pairs
// mean((1 - r)^2) + mean(g^2)), generator_loss (eight means of (1 - x)^2) -- each a subtract / abs / mean / add chain per tensor
// in stock torch, forward and backward.
//
// An ENTRY is one mean: kind 0 mean((1 - a)^2), kind 1 mean(a^2), kind 2 mean(|a - b|).  The entries' pointers travel as kernel
// arguments (a fixed-size table by value: nothing is copied to the device, nothing can be overwritten while a launch is in flight);
// a prefix table maps a workgroup to (entry, chunk), a chunk being S2SVC_GAN_LOSS_CHUNK consecutive elements of the entry's
// physical storage (the tensors are dense, a and b of an entry equally strided: the element order does not matter to a mean).
// Forward: the chunk sums in double (each lane its strided elements, the wave by xor-shuffles, the four waves in order), then a
// finish launch that adds every entry's chunks in a fixed order, divides by numel and writes the fp32 means and the fp32 sum of
// the double means -- one rounding each, no atomics, the same bits on every call.
// Backward: ONE launch over the same table, recomputing the sign / the residual from the inputs:
//   kind 2: t = fl(up / numel) * sgn(a - b), sgn(0) = 0; grad_a = t, grad_b = -t   (stock torch's fp32 chain, signed zeros included)
//   kind 0: grad_a = fl(2 up (a - 1) / numel), kind 1: grad_a = fl(2 up a / numel), the product and the division in double
// `up` is read from device memory; a NULL gradient pointer is not written.
#include "common.h"
#include "../../include/s2svc_hip.h"

namespace {

constexpr int MAXE = 64;             // entries per call (s2svc_gan_loss_max)
constexpr int CHUNK = 8192;          // elements per workgroup (s2svc_gan_loss_chunk): 256 lanes x 8 float4
constexpr int THREADS = 256;

struct Table {
  const float* a[MAXE];
  const float* b[MAXE];
  float* ga[MAXE];
  float* gb[MAXE];
  int64_t numel[MAXE];
  int32_t kind[MAXE];
  int32_t prefix[MAXE + 1];          // first workgroup of every entry; prefix[n] = the grid
  int32_t n;
};

// the entry whose chunks hold workgroup `blk`: the last e with prefix[e] <= blk (entries without elements own no workgroup)
__device__ __forceinline__ int find_entry(const Table& t, int blk) {
  int lo = 0, hi = t.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.prefix[mid] <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ double term(int kind, float a, float b) {
  if (kind == 2) return fabs((double)a - (double)b);
  const double d = kind == 0 ? 1.0 - (double)a : (double)a;
  return d * d;
}

__global__ __launch_bounds__(THREADS) void gan_loss_partial_kernel(const Table t, double* __restrict__ partials) {
  __shared__ double sh[THREADS / 64];
  const int e = find_entry(t, blockIdx.x);
  const int kind = t.kind[e];
  const float* __restrict__ a = t.a[e];
  const float* __restrict__ b = t.b[e];
  const int64_t lo = (int64_t)(blockIdx.x - t.prefix[e]) * CHUNK;
  const int64_t hi = lo + CHUNK < t.numel[e] ? lo + CHUNK : t.numel[e];
  double acc = 0.0;
  const bool vec = (((uintptr_t)a | (uintptr_t)(kind == 2 ? b : a)) & 15) == 0;
  int64_t i = lo;
  if (vec) {                          // lo is a multiple of 4: whole float4 inside [lo, hi)
    const int64_t n4 = (hi - lo) >> 2;
    for (int64_t q = threadIdx.x; q < n4; q += THREADS) {
      const float4 va = *reinterpret_cast<const float4*>(a + lo + 4 * q);
      const float4 vb = kind == 2 ? *reinterpret_cast<const float4*>(b + lo + 4 * q) : va;
      acc += (term(kind, va.x, vb.x) + term(kind, va.y, vb.y)) + (term(kind, va.z, vb.z) + term(kind, va.w, vb.w));
    }
    i = lo + (n4 << 2);
  }
  for (int64_t j = i + threadIdx.x; j < hi; j += THREADS) acc += term(kind, a[j], kind == 2 ? b[j] : 0.f);
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// one workgroup: wave w adds the chunks of entries w, w + 4, ... (lane l the chunks l, l + 64, ... in ascending order, then the
// xor-shuffles); out[e] = fp32(sum / numel) and out[n] = fp32(the double means added in ascending entry order)
__global__ __launch_bounds__(THREADS) void gan_loss_finish_kernel(const Table t, const double* __restrict__ partials, float* __restrict__ out) {
  __shared__ double mean[MAXE];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int e = w; e < t.n; e += THREADS / 64) {
    double acc = 0.0;
    for (int c = t.prefix[e] + lane; c < t.prefix[e + 1]; c += 64) acc += partials[c];
    acc = wave_sum_d(acc);
    if (lane == 0) {
      const double m = t.numel[e] > 0 ? acc / (double)t.numel[e] : 0.0;
      mean[e] = m;
      out[e] = (float)m;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int e = 0; e < t.n; ++e) total += mean[e];
    out[t.n] = (float)total;
  }
}

__device__ __forceinline__ void grad_one(int kind, float a, float b, float c32, double c64, float& ga, float& gb) {
  if (kind == 2) {
    const float s = a > b ? 1.f : (a < b ? -1.f : (a == b ? 0.f : a - b));      // NaN stays NaN
    ga = c32 * s;
    gb = -ga;
  } else {
    ga = (float)(c64 * (kind == 0 ? (double)a - 1.0 : (double)a));
    gb = 0.f;
  }
}

__global__ __launch_bounds__(THREADS) void gan_loss_bwd_kernel(const Table t, const float* __restrict__ upstream) {
  const int e = find_entry(t, blockIdx.x);
  const int kind = t.kind[e];
  const float* __restrict__ a = t.a[e];
  const float* __restrict__ b = kind == 2 ? t.b[e] : t.a[e];
  float* __restrict__ ga = t.ga[e];
  float* __restrict__ gb = kind == 2 ? t.gb[e] : nullptr;
  if (!ga && !gb) return;
  const float up = upstream[0];
  const float c32 = up / (float)t.numel[e];
  const double c64 = 2.0 * (double)up / (double)t.numel[e];
  const int64_t lo = (int64_t)(blockIdx.x - t.prefix[e]) * CHUNK;
  const int64_t hi = lo + CHUNK < t.numel[e] ? lo + CHUNK : t.numel[e];
  const bool vec = (((uintptr_t)a | (uintptr_t)b | (uintptr_t)ga | (uintptr_t)gb) & 15) == 0;
  int64_t i = lo;
  if (vec) {
    const int64_t n4 = (hi - lo) >> 2;
    for (int64_t q = threadIdx.x; q < n4; q += THREADS) {
      const float4 va = *reinterpret_cast<const float4*>(a + lo + 4 * q);
      const float4 vb = *reinterpret_cast<const float4*>(b + lo + 4 * q);
      float4 xa, xb;
      grad_one(kind, va.x, vb.x, c32, c64, xa.x, xb.x);
      grad_one(kind, va.y, vb.y, c32, c64, xa.y, xb.y);
      grad_one(kind, va.z, vb.z, c32, c64, xa.z, xb.z);
      grad_one(kind, va.w, vb.w, c32, c64, xa.w, xb.w);
      if (ga) *reinterpret_cast<float4*>(ga + lo + 4 * q) = xa;
      if (gb) *reinterpret_cast<float4*>(gb + lo + 4 * q) = xb;
    }
    i = lo + (n4 << 2);
  }
  for (int64_t j = i + threadIdx.x; j < hi; j += THREADS) {
    float xa, xb;
    grad_one(kind, a[j], b[j], c32, c64, xa, xb);
    if (ga) ga[j] = xa;
    if (gb) gb[j] = xb;
  }
}

// table: n rows of 6 int64 on the HOST: a, b, grad_a, grad_b (addresses; b and the gradients may be 0), numel, kind.
// Every argument is checked before the first launch.  -> the grid, or a negative error code.
int fill_table(const char* who, int n, const int64_t* table, const int32_t* prefix, bool pairs_only, bool scores_only, Table& t) {
  if (!(n >= 1 && n <= MAXE && table && prefix && prefix[0] == 0)) { s2svc_set_error(who); return -1; }
  t.n = n;
  for (int e = 0; e < n; ++e) {
    const int64_t* r = table + 6 * e;
    const int64_t numel = r[4], kind = r[5];
    const int64_t chunks = (numel + CHUNK - 1) / CHUNK;
    const bool ok = r[0] && numel >= 1 && kind >= 0 && kind <= 2 && (kind != 2 || r[1]) && (kind == 2 || !r[3]) &&
                    (!pairs_only || kind == 2) && (!scores_only || kind != 2) && chunks < (1ll << 30) &&
                    (int64_t)prefix[e + 1] - (int64_t)prefix[e] == chunks;
    if (!ok) { s2svc_set_error(who); return -1; }
    t.a[e] = (const float*)(uintptr_t)r[0];
    t.b[e] = (const float*)(uintptr_t)r[1];
    t.ga[e] = (float*)(uintptr_t)r[2];
    t.gb[e] = (float*)(uintptr_t)r[3];
    t.numel[e] = numel;
    t.kind[e] = (int32_t)kind;
    t.prefix[e] = prefix[e];
  }
  t.prefix[n] = prefix[n];
  for (int e = n; e < MAXE; ++e) {
    t.a[e] = t.b[e] = nullptr;
    t.ga[e] = t.gb[e] = nullptr;
    t.numel[e] = 0;
    t.kind[e] = 0;
    t.prefix[e + 1] = prefix[n];
  }
  return prefix[n];
}

int forward(const char* who, int n, const int64_t* table, const int32_t* prefix, bool pairs, double* partials, float* out, void* stream) {
  Table t;
  const int grid = fill_table(who, n, table, prefix, pairs, !pairs, t);
  if (grid < 0) return grid;
  S2S_REQUIRE(partials && out, "gan loss: partials (one double per chunk) and out (n + 1 floats) are needed");
  hipLaunchKernelGGL(gan_loss_partial_kernel, dim3((unsigned)grid), dim3(THREADS), 0, (hipStream_t)stream, t, partials);
  S2S_CHECK_LAUNCH("gan_loss_partial_kernel");
  hipLaunchKernelGGL(gan_loss_finish_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, t, (const double*)partials, out);
  S2S_CHECK_LAUNCH("gan_loss_finish_kernel");
  return 0;
}

int backward(const char* who, int n, const int64_t* table, const int32_t* prefix, bool pairs, const float* upstream, void* stream) {
  Table t;
  const int grid = fill_table(who, n, table, prefix, pairs, !pairs, t);
  if (grid < 0) return grid;
  S2S_REQUIRE(upstream, "gan loss backward: the upstream scalar lives in device memory");
  hipLaunchKernelGGL(gan_loss_bwd_kernel, dim3((unsigned)grid), dim3(THREADS), 0, (hipStream_t)stream, t, upstream);
  S2S_CHECK_LAUNCH("gan_loss_bwd_kernel");
  return 0;
}

}  // namespace

extern "C" int s2svc_gan_loss_chunk(void) { return CHUNK; }
extern "C" int s2svc_gan_loss_max(void) { return MAXE; }

extern "C" int s2svc_gan_feature_loss(int n, const int64_t* table, const int32_t* prefix, double* partials, float* out, void* stream) {
  return forward("gan_feature_loss: 1 .. 64 pairs (a, b, numel >= 1, kind 2) and the chunk prefix table of their numels", n, table, prefix, true,
                 partials, out, stream);
}

extern "C" int s2svc_gan_feature_loss_bwd(int n, const int64_t* table, const int32_t* prefix, const float* upstream, void* stream) {
  return backward("gan_feature_loss_bwd: 1 .. 64 pairs (a, b, numel >= 1, kind 2) and the chunk prefix table of their numels", n, table, prefix,
                  true, upstream, stream);
}

extern "C" int s2svc_gan_score_loss(int n, const int64_t* table, const int32_t* prefix, double* partials, float* out, void* stream) {
  return forward("gan_score_loss: 1 .. 64 tensors (a, numel >= 1, kind 0 or 1) and the chunk prefix table of their numels", n, table, prefix, false,
                 partials, out, stream);
}

extern "C" int s2svc_gan_score_loss_bwd(int n, const int64_t* table, const int32_t* prefix, const float* upstream, void* stream) {
  return backward("gan_score_loss_bwd: 1 .. 64 tensors (a, numel >= 1, kind 0 or 1) and the chunk prefix table of their numels", n, table, prefix,
                  false, upstream, stream);
}
