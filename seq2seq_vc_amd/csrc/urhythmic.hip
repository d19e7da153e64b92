// Urhythmic on the GPU: the segmentation search (span scores, dynamic programme, backtrack, cluster merge), the stretch plan (merged
// clusters + the rhythm model's duration table -> the stretcher's segment table) and the segment-wise linear resampling of the time
// stretcher.
//
// reference: seq2seq_vc/urhythmic/segmenter.py:138-191 (_segment, numba-JIT on the host over a dense (T, T, K) fp32 table; _backtrack;
// cluster_merge) and seq2seq_vc/urhythmic/stretcher.py:23-71 (F.interpolate per segment + torch.cat).
//
// Span scores (useg_span_kernel): one wave per start frame a, lanes over the units k (K <= 256: up to four per lane, in registers).
// The wave walks the end frame e = a, a + 1, .. and keeps r[k] = ((lp[a,k] + lp[a+1,k]) + ..) + lp[e,k]: the reference's fp32
// additions in the reference's order, one rounding each.  Per end frame it stores max_k r[k] and the smallest k that attains it, at
// [e][a], so that the search reads one contiguous line per frame.  The other layout (a lane per start frame, the K sums of a lane in
// registers) needs K = 100 .. 256 live fp32 per lane behind a run-time K: it cannot stay in registers.  (T, T, K) is never stored.
//
// Search (useg_search_kernel): one wave per utterance.  The reference's loop for frame t keeps a running maximum that is ROUNDED TO
// FLOAT32 after every update, so the chosen candidate is not an argmax:
//     c_s = float64(alpha[t-s] +f32 M[t][t-s]) + gamma * s          (float64 product and sum, no fma)
//     alpha[t+1] = float32(max_s c_s);  the chosen s is the LARGEST s with c_s > float64(float32(max_{i<s} c_i))   (max of nothing: -inf)
// which is an exclusive prefix maximum per chunk of 64 candidates (DPP row shifts + v_readlane across rows, a carried maximum across
// chunks) and a ballot.  alpha and the back-pointers live in LDS; the same wave backtracks, writes codes / boundaries and merges
// adjacent segments of the same cluster.  Frames >= lens[b] are never read, in log_probs or in the workspace.
#include "common.h"
#include "../../include/s2svc_hip.h"

// the search is compared bit for bit: no x + g * s -> fma anywhere in this file
#pragma clang fp contract(off)

namespace {

constexpr int USEG_MAX_K = 256, USEG_MAX_T = 4096;

template <int KS>   // KS >= ceil(K / 64) units per lane
__global__ __launch_bounds__(256) void useg_span_kernel(int Tmax, int K, const float* __restrict__ logp, const int32_t* __restrict__ lens,
                                                        float* __restrict__ M, uint16_t* __restrict__ Kx) {
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int a = blockIdx.x * 4 + (threadIdx.x >> 6);
  int len = lens[b];
  len = len < 0 ? 0 : (len > Tmax ? Tmax : len);
  if (a >= len) return;                                          // wave-uniform: the waves that stay are full
  const float* lp = logp + (int64_t)b * Tmax * K;
  float* Mb = M + (int64_t)b * Tmax * Tmax;
  uint16_t* Kb = Kx + (int64_t)b * Tmax * Tmax;
  const float NINF = -__builtin_huge_valf();

  constexpr int U = 4;                                           // end frames in flight (loads of the next U while these U are summed)
  float r[KS], nxt[U][KS];
  auto fetch = [&](int e0) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int k = s * 64 + lane, e = e0 + u;
        nxt[u][s] = (e < len && k < K) ? lp[(int64_t)e * K + k] : 0.f;
      }
  };
  fetch(a);
  for (int e0 = a; e0 < len; e0 += U) {
    float val[U][KS];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int s = 0; s < KS; ++s) val[u][s] = nxt[u][s];
    if (e0 + U < len) fetch(e0 + U);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + u;
      if (e < len) {                                             // wave-uniform
        float m = NINF;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const int k = s * 64 + lane;
          if (e == a) r[s] = k < K ? val[u][s] : NINF;
          else r[s] = r[s] + val[u][s];                          // -inf + 0 stays -inf on the lanes past K
          m = fmaxf(m, r[s]);
        }
        const float mx = wave_max(m);
        int kbest = -1;
#pragma unroll
        for (int s = 0; s < KS; ++s) {                           // numpy's argmax: the smallest k among the maxima
          const uint64_t hit = __ballot(r[s] == mx);
          if (kbest < 0 && hit) kbest = s * 64 + __builtin_ctzll(hit);
        }
        if (lane == 0) {
          Mb[(int64_t)e * Tmax + a] = mx;
          Kb[(int64_t)e * Tmax + a] = (uint16_t)(kbest < 0 ? 0 : kbest);
        }
      }
    }
  }
}

template <int CTRL>
__device__ __forceinline__ double dpp_own_d(double v) {          // DPP move of a double; a lane without a source keeps its own value
  S2S_ASSERT_FULL_EXEC();
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int slo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  const int shi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(shi, slo);
}
__device__ __forceinline__ double readlane_d(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

struct Cursor { int t, j; };                                     // chunk j of frame t: candidates s = 64 j .. 64 j + 63
__device__ __forceinline__ void advance(Cursor& c) {
  ++c.j;
  if (c.j * 64 > c.t) { ++c.t; c.j = 0; }
}

__global__ __launch_bounds__(64) void useg_search_kernel(int Tmax, double gamma, const int32_t* __restrict__ lens,
                                                         const float* __restrict__ M, const uint16_t* __restrict__ Kx,
                                                         const int32_t* __restrict__ labels, int32_t* __restrict__ codes,
                                                         int32_t* __restrict__ boundaries, int32_t* __restrict__ nseg,
                                                         float* __restrict__ alpha_out, int32_t* __restrict__ P_out,
                                                         int32_t* __restrict__ clusters, int32_t* __restrict__ cboundaries,
                                                         int32_t* __restrict__ ncl) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int T1 = Tmax + 1;
  float* alpha_l = reinterpret_cast<float*>(smem);               // alpha[0 .. len]; afterwards the cluster of every segment
  int32_t* start_l = reinterpret_cast<int32_t*>(smem) + T1;      // P[t][0]
  int32_t* back_l = start_l + T1;                                // boundaries in backtrack (descending) order
  int32_t* count_l = back_l + T1;                                // [0] = number of segments
  int len = lens[b];
  len = len < 0 ? 0 : (len > Tmax ? Tmax : len);
  const float* Mb = M + (int64_t)b * Tmax * Tmax;
  const uint16_t* Kb = Kx + (int64_t)b * Tmax * Tmax;
  int32_t* cod = codes + (int64_t)b * Tmax;
  int32_t* bnd = boundaries + (int64_t)b * T1;
  const double NINF = -__builtin_huge_val();

  if (lane == 0) { alpha_l[0] = 0.f; start_l[0] = 0; }
  __syncthreads();

  constexpr int U = 4;
  float nxt[U];
  Cursor cf = {0, 0}, cp = {0, 0};
  auto fetch = [&]() {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int s = cf.j * 64 + lane;
      nxt[u] = (cf.t < len && s <= cf.t) ? Mb[(int64_t)cf.t * Tmax + (cf.t - s)] : 0.f;
      advance(cf);
    }
  };
  fetch();
  double carry = NINF;
  int best = 0;
  while (cp.t < len) {
    float val[U];
#pragma unroll
    for (int u = 0; u < U; ++u) val[u] = nxt[u];
    if (cf.t < len) fetch();
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (cp.t < len) {                                          // wave-uniform
        const int t = cp.t, s = cp.j * 64 + lane;
        if (cp.j == 0) { carry = NINF; best = 0; }
        double c = NINF;
        if (s <= t) {
          const float sum = alpha_l[t - s] + val[u];             // float32 sum
          c = (double)sum + gamma * (double)s;                   // float64 product, float64 sum
        }
        // inclusive prefix maximum over the 64 candidates: inside every row of 16 lanes by DPP shifts, across rows by v_readlane
        double v = c;
        v = fmax(v, dpp_own_d<0x111>(v));                        // row_shr:1
        v = fmax(v, dpp_own_d<0x112>(v));                        // row_shr:2
        v = fmax(v, dpp_own_d<0x114>(v));                        // row_shr:4
        v = fmax(v, dpp_own_d<0x118>(v));                        // row_shr:8
        const double r0 = readlane_d(v, 15), r1 = readlane_d(v, 31), r2 = readlane_d(v, 47), r3 = readlane_d(v, 63);
        const int row = lane >> 4;
        double pre = NINF;
        if (row >= 1) pre = r0;
        if (row >= 2) pre = fmax(pre, r1);
        if (row >= 3) pre = fmax(pre, r2);
        v = fmax(v, pre);
        double ex = dpp_own_d<0x138>(v);                         // wave_shr:1
        if (lane == 0) ex = NINF;
        ex = fmax(ex, carry);
        const bool accept = s <= t && c > (double)(float)ex;     // the running maximum is held in float32
        const uint64_t acc = __ballot(accept);
        if (acc) best = cp.j * 64 + 63 - __builtin_clzll(acc);
        carry = fmax(carry, fmax(fmax(r0, r1), fmax(r2, r3)));
        if ((cp.j + 1) * 64 > t) {                               // last chunk of the frame
          alpha_l[t + 1] = (float)carry;
          start_l[t + 1] = t - best;
          __syncthreads();
        }
        advance(cp);
      }
    }
  }
  __syncthreads();

  // optional tables: alpha (Tmax + 1) and P (Tmax + 1, 2), zero past the row's length
  if (alpha_out)
    for (int i = lane; i < T1; i += 64) alpha_out[(int64_t)b * T1 + i] = i <= len ? alpha_l[i] : 0.f;
  if (P_out)
    for (int i = lane; i < T1; i += 64) {
      int lhs = 0, code = 0;
      if (i >= 1 && i <= len) { lhs = start_l[i]; code = Kb[(int64_t)(i - 1) * Tmax + lhs]; }
      P_out[((int64_t)b * T1 + i) * 2] = lhs;
      P_out[((int64_t)b * T1 + i) * 2 + 1] = code;
    }
  __syncthreads();

  // backtrack from rhs = len
  if (lane == 0) {
    int n = 0, rhs = len;
    back_l[n++] = rhs;
    while (rhs != 0) { rhs = start_l[rhs]; back_l[n++] = rhs; }
    count_l[0] = n - 1;
  }
  __syncthreads();
  const int ns = count_l[0];
  for (int i = lane; i < T1; i += 64) bnd[i] = i <= ns ? back_l[ns - i] : 0;
  for (int i = lane; i < Tmax; i += 64)
    if (i >= len) cod[i] = 0;
  if (lane == 0) nseg[b] = ns;
  int32_t* segcl = reinterpret_cast<int32_t*>(alpha_l);          // alpha has been written out
  for (int i = lane; i < ns; i += 64) {
    const int lhs = back_l[ns - i], rhs = back_l[ns - i - 1];
    const int code = Kb[(int64_t)(rhs - 1) * Tmax + lhs];
    for (int f = lhs; f < rhs; ++f) cod[f] = code;
    segcl[i] = labels ? labels[code] : code;
  }
  __syncthreads();
  if (!labels) return;

  // cluster merge: a segment opens a cluster where its label differs from the segment before it
  int32_t* cl = clusters + (int64_t)b * Tmax;
  int32_t* cb = cboundaries + (int64_t)b * T1;
  int base = 0;
  for (int i0 = 0; i0 < ns; i0 += 64) {
    const int i = i0 + lane;
    const bool open = i < ns && (i == 0 || segcl[i] != segcl[i - 1]);
    const uint64_t m = __ballot(open);
    if (open) {
      const int pos = base + __builtin_popcountll(m & ((1ull << lane) - 1ull));
      cl[pos] = segcl[i];
      cb[pos] = back_l[ns - i];
    }
    base += __builtin_popcountll(m);
  }
  for (int i = base + lane; i < Tmax; i += 64) cl[i] = 0;
  for (int i = base + lane; i < T1; i += 64) cb[i] = i == base ? len : 0;
  if (lane == 0) ncl[b] = base;
}

// Segment-wise linear resampling.  Block = FR output frames of one row; the first FR threads find their frame's segment (binary search
// over the exclusive prefix sums of the target lengths), then all threads run over (frame, channel).
constexpr int STRETCH_FR = 16;

template <typename T>
__global__ __launch_bounds__(256) void useg_stretch_kernel(int N, int C, const T* __restrict__ x, int64_t sb, int64_t st, int64_t sc,
                                                           const int32_t* __restrict__ seg, const int32_t* __restrict__ nsegs, int Smax,
                                                           int Nmax, float scale_given, float* __restrict__ out) {
  __shared__ int s_i0[STRETCH_FR], s_i1[STRETCH_FR];
  __shared__ float s_w1[STRETCH_FR];
  const int b = blockIdx.y, n0 = blockIdx.x * STRETCH_FR;
  const int32_t* sg = seg + (int64_t)b * Smax * 4;               // (source start, source length, target length, target offset)
  int ns = nsegs[b];
  ns = ns < 0 ? 0 : (ns > Smax ? Smax : ns);
  if (threadIdx.x < STRETCH_FR) {
    const int n = n0 + threadIdx.x;
    int i0 = -1, i1 = -1;
    float w1 = 0.f;
    if (n < Nmax && ns > 0) {
      int lo = 0, hi = ns - 1;                                   // the last segment whose offset is <= n
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sg[mid * 4 + 3] <= n) lo = mid; else hi = mid - 1;
      }
      const int start = sg[lo * 4], L = sg[lo * 4 + 1], tl = sg[lo * 4 + 2], i = n - sg[lo * 4 + 3];
      if (i >= 0 && i < tl && L > 0 && start >= 0 && start + L <= N) {
        const float scale = scale_given > 0.f ? scale_given : (float)L / (float)tl;
        float src = scale * ((float)i + 0.5f) - 0.5f;
        src = src < 0.f ? 0.f : src;
        int j0 = (int)floorf(src);
        j0 = j0 > L - 1 ? L - 1 : j0;
        w1 = fminf(fmaxf(src - (float)j0, 0.f), 1.f);
        i0 = start + j0;
        i1 = start + (j0 + 1 > L - 1 ? L - 1 : j0 + 1);          // never across the segment's end
      }
    }
    s_i0[threadIdx.x] = i0;
    s_i1[threadIdx.x] = i1;
    s_w1[threadIdx.x] = w1;
  }
  __syncthreads();
  const T* xb = x + (int64_t)b * sb;
  float* ob = out + (int64_t)b * Nmax * C;
  for (int idx = threadIdx.x; idx < STRETCH_FR * C; idx += 256) {
    const int f = idx / C, c = idx - f * C, n = n0 + f;
    if (n >= Nmax) break;
    float y = 0.f;
    if (s_i0[f] >= 0) {
      const float w1 = s_w1[f], w0 = 1.f - w1;
      y = w0 * ldf(xb + (int64_t)s_i0[f] * st + (int64_t)c * sc) + w1 * ldf(xb + (int64_t)s_i1[f] * st + (int64_t)c * sc);
    }
    ob[(int64_t)n * C + c] = y;
  }
}

// The stretch plan: the search's merged clusters of one row -> the stretcher's segment table, through the rhythm model's duration
// table.  One wave per row, a lane per segment, chunks of 64.  Two passes over the row: the first only judges it (malformed input,
// an unmapped length, the 64-bit total of the targets), the second writes -- so a row that is refused is written as zeros once and no
// store depends on the order of another.  Every index is checked before it is used: nothing is assumed about what the tables hold.
constexpr int32_t USEG_UNMAPPED = INT32_MIN;

struct PlanItem { int start, n, target; bool bad, unmapped; };

__device__ __forceinline__ PlanItem useg_plan_item(int i, int ncl, int Tmax, int n_clusters, int Lmax, const int32_t* __restrict__ cl,
                                                   const int32_t* __restrict__ cb, const int32_t* __restrict__ table, int silence_cluster,
                                                   int short_silence) {
  PlanItem it = {0, 0, 0, false, false};
  if (i >= ncl) return it;                                       // i + 1 <= ncl <= Tmax: cb[i + 1] exists
  const int lo = cb[i], hi = cb[i + 1], c = cl[i];
  if (lo < 0 || lo > Tmax || hi < 0 || hi > Tmax || hi - lo < 1 || hi - lo > Lmax || c < 0 || c >= n_clusters) {
    it.bad = true;
    return it;
  }
  it.start = lo;
  it.n = hi - lo;
  if (c == silence_cluster && it.n <= short_silence) return it;  // a short silence: dropped before the durations pair up
  const int32_t t = table[(int64_t)c * (Lmax + 1) + it.n];
  it.unmapped = t == USEG_UNMAPPED;
  it.target = t > 0 ? t : 0;                                     // a target <= 0 drops its segment
  return it;
}

__global__ __launch_bounds__(64) void useg_plan_kernel(int Tmax, int n_clusters, int Lmax, const int32_t* __restrict__ clusters,
                                                       const int32_t* __restrict__ cboundaries, const int32_t* __restrict__ ncls,
                                                       const int32_t* __restrict__ table, int silence_cluster, int short_silence,
                                                       int32_t* __restrict__ seg, int32_t* __restrict__ nsegs, int32_t* __restrict__ totals,
                                                       int32_t* __restrict__ status) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int32_t* cl = clusters + (int64_t)b * Tmax;
  const int32_t* cb = cboundaries + (int64_t)b * (Tmax + 1);
  int32_t* sg = seg + (int64_t)b * Tmax * 4;
  int ncl = ncls[b];
  ncl = ncl < 0 ? 0 : (ncl > Tmax ? Tmax : ncl);

  bool bad = false, unmapped = false;
  int64_t sum = 0;
  for (int i0 = 0; i0 < ncl; i0 += 64) {
    const PlanItem it = useg_plan_item(i0 + lane, ncl, Tmax, n_clusters, Lmax, cl, cb, table, silence_cluster, short_silence);
    bad |= it.bad;
    unmapped |= it.unmapped;
    sum += it.target;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  int st = 0;
  if (__ballot(bad)) st = 2;
  else if (__ballot(unmapped)) st = 1;
  else if (sum > (int64_t)INT32_MAX) st = 3;

  int base = 0;
  if (st == 0) {                                                 // wave-uniform; every partial sum below is <= sum <= INT32_MAX
    int run = 0;
    for (int i0 = 0; i0 < ncl; i0 += 64) {
      const PlanItem it = useg_plan_item(i0 + lane, ncl, Tmax, n_clusters, Lmax, cl, cb, table, silence_cluster, short_silence);
      const bool keep = it.target > 0;
      const uint64_t m = __ballot(keep);
      int incl = it.target;                                      // inclusive prefix sum of the chunk's targets
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      if (keep) {
        const int pos = base + __builtin_popcountll(m & ((1ull << lane) - 1ull));      // pos <= i0 + lane < Tmax
        sg[pos * 4] = it.start;
        sg[pos * 4 + 1] = it.n;
        sg[pos * 4 + 2] = it.target;
        sg[pos * 4 + 3] = run + incl - it.target;
      }
      base += __builtin_popcountll(m);
      run += __shfl(incl, 63, 64);
    }
  }
  for (int i = base * 4 + lane; i < Tmax * 4; i += 64) sg[i] = 0;
  if (lane == 0) {
    nsegs[b] = base;
    totals[b] = st == 0 ? (int32_t)sum : 0;
    status[b] = st;
  }
}

}  // namespace

extern "C" int64_t s2svc_useg_ws_bytes(int B, int Tmax, int K) {
  (void)K;
  const int64_t cells = (int64_t)B * Tmax * Tmax;
  return ((cells * 4 + 15) / 16) * 16 + cells * 2 + 16;
}

static inline uint16_t* useg_kx(void* ws, int B, int Tmax) {
  const int64_t cells = (int64_t)B * Tmax * Tmax;
  return reinterpret_cast<uint16_t*>(reinterpret_cast<unsigned char*>(ws) + ((cells * 4 + 15) / 16) * 16);
}

extern "C" int s2svc_useg_spans(int B, int Tmax, int K, const float* log_probs, const int32_t* lens, void* ws, void* stream) {
  S2S_REQUIRE(B >= 0 && Tmax > 0 && K > 0, "useg_spans: bad shape");
  S2S_REQUIRE(K <= USEG_MAX_K, "useg_spans: K > 256 not supported");
  S2S_REQUIRE(Tmax <= USEG_MAX_T, "useg_spans: Tmax > 4096 not supported");
  S2S_REQUIRE(B <= 65535, "useg_spans: B > 65535 not supported");
  S2S_REQUIRE(log_probs && lens && ws, "useg_spans: null argument");
  if (B == 0) return 0;
  float* M = (float*)ws;
  uint16_t* Kx = useg_kx(ws, B, Tmax);
  const dim3 grid((Tmax + 3) / 4, B);
  hipStream_t st = (hipStream_t)stream;
  switch ((K + 63) / 64) {
    case 1: hipLaunchKernelGGL(useg_span_kernel<1>, grid, dim3(256), 0, st, Tmax, K, log_probs, lens, M, Kx); break;
    case 2: hipLaunchKernelGGL(useg_span_kernel<2>, grid, dim3(256), 0, st, Tmax, K, log_probs, lens, M, Kx); break;
    case 3: hipLaunchKernelGGL(useg_span_kernel<3>, grid, dim3(256), 0, st, Tmax, K, log_probs, lens, M, Kx); break;
    default: hipLaunchKernelGGL(useg_span_kernel<4>, grid, dim3(256), 0, st, Tmax, K, log_probs, lens, M, Kx); break;
  }
  S2S_CHECK_LAUNCH("useg_span_kernel");
  return 0;
}

extern "C" int s2svc_useg_search(int B, int Tmax, double gamma, const int32_t* lens, const void* ws, const int32_t* labels, int32_t* codes,
                                 int32_t* boundaries, int32_t* nseg, float* alpha, int32_t* P, int32_t* clusters, int32_t* cboundaries,
                                 int32_t* ncl, void* stream) {
  S2S_REQUIRE(B >= 0 && Tmax > 0, "useg_search: bad shape");
  S2S_REQUIRE(Tmax <= USEG_MAX_T, "useg_search: Tmax > 4096 not supported");
  S2S_REQUIRE(lens && ws && codes && boundaries && nseg, "useg_search: null argument");
  S2S_REQUIRE(!labels || (clusters && cboundaries && ncl), "useg_search: labels need clusters, cboundaries and ncl");
  if (B == 0) return 0;
  const size_t lds = ((size_t)(Tmax + 1) * 3 + 4) * 4;            // <= 49188 bytes at Tmax = 4096
  hipLaunchKernelGGL(useg_search_kernel, dim3(B), dim3(64), lds, (hipStream_t)stream, Tmax, gamma, lens, (const float*)ws,
                     (const uint16_t*)useg_kx(const_cast<void*>(ws), B, Tmax), labels, codes, boundaries, nseg, alpha, P, clusters,
                     cboundaries, ncl);
  S2S_CHECK_LAUNCH("useg_search_kernel");
  return 0;
}

extern "C" int s2svc_useg_plan(int B, int Tmax, int n_clusters, int Lmax, const int32_t* clusters, const int32_t* cboundaries,
                               const int32_t* ncl, const int32_t* table, int silence_cluster, int short_silence, int32_t* seg,
                               int32_t* nsegs, int32_t* totals, int32_t* status, void* stream) {
  S2S_REQUIRE(B >= 0 && Tmax > 0 && n_clusters > 0 && Lmax >= 0, "useg_plan: bad shape");
  S2S_REQUIRE(Tmax <= USEG_MAX_T, "useg_plan: Tmax > 4096 not supported");
  S2S_REQUIRE(B <= 65535, "useg_plan: B > 65535 not supported");
  S2S_REQUIRE(clusters && cboundaries && ncl && table && seg && nsegs && totals && status, "useg_plan: null argument");
  if (B == 0) return 0;
  hipLaunchKernelGGL(useg_plan_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, Tmax, n_clusters, Lmax, clusters, cboundaries, ncl, table,
                     silence_cluster, short_silence, seg, nsegs, totals, status);
  S2S_CHECK_LAUNCH("useg_plan_kernel");
  return 0;
}

extern "C" int s2svc_useg_stretch(int dtype, int B, int N, int C, const void* x, int64_t sb, int64_t st, int64_t sc, const int32_t* seg,
                                  const int32_t* nsegs, int Smax, int Nmax, float scale, float* out, void* stream) {
  S2S_REQUIRE(B >= 0 && N > 0 && C > 0 && Smax > 0 && Nmax >= 0, "useg_stretch: bad shape");
  S2S_REQUIRE(dtype == S2S_F32 || dtype == S2S_BF16, "useg_stretch: dtype must be float32 or bfloat16");
  S2S_REQUIRE(B <= 65535, "useg_stretch: B > 65535 not supported");
  S2S_REQUIRE(x && seg && nsegs && (out || Nmax == 0), "useg_stretch: null argument");
  if (B == 0 || Nmax == 0) return 0;
  const dim3 grid((Nmax + STRETCH_FR - 1) / STRETCH_FR, B);
  if (dtype == S2S_F32)
    hipLaunchKernelGGL(useg_stretch_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, N, C, (const float*)x, sb, st, sc, seg, nsegs,
                       Smax, Nmax, scale, out);
  else
    hipLaunchKernelGGL(useg_stretch_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, N, C, (const bf16_t*)x, sb, st, sc, seg, nsegs,
                       Smax, Nmax, scale, out);
  S2S_CHECK_LAUNCH("useg_stretch_kernel");
  return 0;
}
