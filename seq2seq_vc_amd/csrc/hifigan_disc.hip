// HiFi-GAN multi-period discriminator, forward and backward, fp32 (reference: seq2seq_vc/urhythmic/vocoder.py:211-327 --
// PeriodDiscriminator, MultiPeriodDiscriminator; urhythmic_fine_tune_vocoder.py:191-222 calls it four times per step and
// backpropagates through it twice).
//
// A period discriminator folds the waveform (B, 1, T) into (B, 1, T / p, p) and convolves along the first of the two axes only, so
// every column w < p is a sequence of its own.  Activations are channel-last (B, L, p, C): a GEMM row is (b, l, w) and the reduction
// index is tap * C + c.  Output row (b, lo, w) of a convolution with stride s reads input rows (b, s * lo + j - 2, w), j < 5; rows
// outside [0, L) are the zero padding of THAT sequence -- the staging below decodes (l, w) of every row it loads and never steps
// into the neighbouring sequence or utterance.
//
//   input layer       hifigan_disc_input_kernel: 1 -> 32 channels straight from x; the reflect pad to a multiple of p and the
//                     (T / p, p) view are index arithmetic.  Bias and leaky_relu in the same launch.
//   convolution       hifigan_disc_tile_kernel: implicit GEMM on v_mfma_f32_16x16x4_f32 (HgFrag<float>), 128 rows x 64 columns per
//                     workgroup, 16 channels per step.  The input rows a tile needs (all taps, <= 480) are staged ONCE per step.
//                     The same kernel is the data gradient: the stride-3 one is phase-decomposed (input row l receives only the taps
//                     j = l + 2 mod 3: 1, 2 or 2 of the 5), one grid plane per phase; its epilogue adds the feature's own gradient
//                     and applies leaky_relu' from the sign of the stored post-activation output.
//   conv_post         hifigan_disc_post_kernel (1024 -> 1, k = 3, one wavefront per output) and its backward.
//   weight gradient   hifigan_disc_wgrad_kernel: partials per chunk of 256 rows, laid out as s2svc_hifigan_wgrad_finish mode 0 / 2
//                     sums them; the bias partials ride along.
//
// The stored activations are POST-activation (they are the features the caller receives), so no loader applies leaky_relu.  Every
// sum runs in an order fixed by the shapes; there are no atomics: two calls give the same bits.
#include "hifigan_tile.h"

namespace {

constexpr int DT_BM = 128, DT_BN = 64, DT_KC = 16, DT_TAPS = 5, DT_MAXR = 480;
constexpr int DT_ROWB = DT_KC * 4 + 16;                  // LDS row in bytes, padded
constexpr int DW_TS = 32, DW_ROW = 36, DW_CHUNK = 256;   // wgrad: rows per step, floats per LDS row, rows per partial
constexpr int DP_CHUNK = 256, DP_CB = 64;                // conv_post backward: rows per partial, channels per workgroup
constexpr int DI_C = 32, DI_CHUNK = 256;                 // input layer: output channels, rows per partial

// -----------------------------------------------------------------------------------------------------------------------------
// the tile: out[(b, so * g + ph, w)][n] = epi( sum_t sum_c a[(b, sa * g + off[ph][t], w)][c] * W[n][wtap[ph][t] * Kap + c] )
// -----------------------------------------------------------------------------------------------------------------------------
struct DtArgs {
  const float* a;        // (B, La, p, Ka)
  const float* w;        // [N][DT_TAPS * Kap]
  const float* bias;     // [N] or NULL
  const float* mask;     // (B, Lo, p, N) or NULL: multiply by leaky_relu'(mask)
  const float* add;      // (B, Lo, p, N) or NULL: added before the mask
  float* out;            // (B, Lo, p, N)
  int B, La, Lo, p, Ka, Kap, N;
  int sa, so, nph, tiles;
  int ntaps[3], off[3][DT_TAPS], wtap[3][DT_TAPS];
  float slope;
  int act;               // 1: out = leaky_relu(acc + bias)
};

__global__ __launch_bounds__(256) void hifigan_disc_tile_kernel(const DtArgs a) {
  typedef HgFrag<float> F;
  __shared__ __attribute__((aligned(16))) unsigned char sA[DT_MAXR * DT_ROWB];
  __shared__ __attribute__((aligned(16))) unsigned char sB[DT_TAPS * DT_BN * DT_ROWB];
  constexpr int VPR = DT_KC / 4, NT = DT_BN / 16;

  const int ph = blockIdx.z, p = a.p;
  const int G = a.Lo > ph ? (a.Lo - ph + a.so - 1) / a.so : 0;      // rows l = so * g + ph < Lo of this phase
  const int rows = G * p;
  const int b = blockIdx.x / a.tiles;
  const int i0 = (blockIdx.x - b * a.tiles) * DT_BM;
  if (i0 >= rows) return;
  const int n0 = blockIdx.y * DT_BN;
  const int nt_ = a.ntaps[ph];
  int offmin = a.off[ph][0], offmax = a.off[ph][0];
  for (int t = 1; t < nt_; ++t) { offmin = min(offmin, a.off[ph][t]); offmax = max(offmax, a.off[ph][t]); }
  const int ilast = min(i0 + DT_BM, rows) - 1;
  const int g0 = i0 / p, g1 = ilast / p;
  const int lbase = a.sa * g0 + offmin;
  const int R = min((a.sa * (g1 - g0) + offmax - offmin + 1) * p, DT_MAXR);      // the launcher has checked the bound

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int Kp = DT_TAPS * a.Kap;
  const float* ab = a.a + (int64_t)b * a.La * p * a.Ka;

  int abase[2];                                           // LDS row of (g, w) of the lane's A rows at offset offmin
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int i = min(i0 + wave * 32 + mt * 16 + lr, ilast);
    const int g = i / p, w = i - g * p;
    abase[mt] = (a.sa * (g - g0) - offmin) * p + w;
  }

  // Three levels of accumulation, so that no fp32 chain is longer than 20 MFMA results + 8 + K / 128 additions (one chain over
  // K = 5 * 1024 products loses two more bits than stock float32 convolutions do): acc = this step's 16 channels x taps,
  // grp = 8 steps, tot = the groups.  The order depends on the shapes only.
  const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
  float tot[2][NT][4], grp[2][NT][4];                     // plain floats, added one by one: the library holds no packed-fp32 adds
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) tot[mt][nt][e] = grp[mt][nt][e] = 0.f;

  int step = 0;
  for (int c0 = 0; c0 < a.Ka; c0 += DT_KC) {
    f32x4_t acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = zero4;
    __syncthreads();                                      // the previous step's fragments have been read
    for (int idx = tid; idx < R * VPR; idx += 256) {
      const int r = idx / VPR, v = idx - r * VPR;
      const int dl = r / p, w = r - dl * p;
      const int l = lbase + dl, c = c0 + v * 4;
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (l >= 0 && l < a.La && c + 4 <= a.Ka) val = *reinterpret_cast<const uint4*>(ab + ((int64_t)l * p + w) * a.Ka + c);
      *reinterpret_cast<uint4*>(sA + r * DT_ROWB + v * 16) = val;
    }
    for (int idx = tid; idx < nt_ * DT_BN * VPR; idx += 256) {
      const int tapi = idx / (DT_BN * VPR), rem = idx - tapi * (DT_BN * VPR);
      const int nn = rem / VPR, v = rem - nn * VPR;
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (n0 + nn < a.N) val = *reinterpret_cast<const uint4*>(a.w + (int64_t)(n0 + nn) * Kp + a.wtap[ph][tapi] * a.Kap + c0 + v * 4);
      *reinterpret_cast<uint4*>(sB + (tapi * DT_BN + nn) * DT_ROWB + v * 16) = val;
    }
    __syncthreads();
    for (int tapi = 0; tapi < nt_; ++tapi) {
      const int toff = a.off[ph][tapi] * p;
      f32x4_t fa[2], fb[NT];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) fa[mt] = *reinterpret_cast<const f32x4_t*>(sA + (abase[mt] + toff) * DT_ROWB + lg * 16);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) fb[nt] = *reinterpret_cast<const f32x4_t*>(sB + (tapi * DT_BN + nt * 16 + lr) * DT_ROWB + lg * 16);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = F::mma(fa[mt], fb[nt], acc[mt][nt]);
    }
    const bool fold = (++step & 7) == 0;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          grp[mt][nt][e] += acc[mt][nt][e];
          if (fold) { tot[mt][nt][e] += grp[mt][nt][e]; grp[mt][nt][e] = 0.f; }
        }
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) tot[mt][nt][e] += grp[mt][nt][e];

  const int64_t ob = (int64_t)b * a.Lo * p * a.N;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = n0 + nt * 16 + lr;
    if (n >= a.N) continue;
    const float bv = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wave * 32 + mt * 16 + lg * 4 + r;
        if (i >= rows) continue;
        const int g = i / p, w = i - g * p;
        const int64_t at = ob + ((int64_t)(a.so * g + ph) * p + w) * a.N + n;
        float v = tot[mt][nt][r] + bv;
        if (a.act) v = hg_lrelu(v, a.slope);
        if (a.add) v += a.add[at];
        if (a.mask) v = a.mask[at] > 0.f ? v : v * a.slope;
        a.out[at] = v;
      }
  }
}

// the staged rows of one tile at the widest: sa * (rows of g a tile can span) + the taps' span + 1, times p
inline int dt_max_staged(int p, int sa, int span) { return (sa * ((DT_BM + p - 2) / p) + span + 1) * p; }

int dt_launch(const char* who, DtArgs& a, hipStream_t st) {
  int span = 0, gmax = 0;
  for (int ph = 0; ph < a.nph; ++ph) {
    int lo = a.off[ph][0], hi = a.off[ph][0];
    for (int t = 1; t < a.ntaps[ph]; ++t) { lo = a.off[ph][t] < lo ? a.off[ph][t] : lo; hi = a.off[ph][t] > hi ? a.off[ph][t] : hi; }
    span = hi - lo > span ? hi - lo : span;
    const int G = a.Lo > ph ? (a.Lo - ph + a.so - 1) / a.so : 0;
    gmax = G > gmax ? G : gmax;
  }
  if (dt_max_staged(a.p, a.sa, span) > DT_MAXR) return hg_fail(who, "period too large for the staged tile (480 rows)");
  const int64_t rows = (int64_t)gmax * a.p;
  a.tiles = (int)((rows + DT_BM - 1) / DT_BM);
  if ((int64_t)a.B * a.tiles >= (1ll << 31) || (a.N + DT_BN - 1) / DT_BN > 65535) return hg_fail(who, "grid too large");
  if ((int64_t)a.B * a.La * a.p * a.Ka >= (1ll << 40) || (int64_t)a.B * a.Lo * a.p * a.N >= (1ll << 40)) return hg_fail(who, "tensor too large");
  const dim3 grid(a.B * a.tiles, (a.N + DT_BN - 1) / DT_BN, a.nph), block(256);
  hipLaunchKernelGGL(hifigan_disc_tile_kernel, grid, block, 0, st, a);
  S2S_CHECK_LAUNCH("hifigan_disc_tile_kernel");
  return 0;
}

// -----------------------------------------------------------------------------------------------------------------------------
// input layer: x (B, 1, T) -> (B, L1, p, 32); padded sample t >= T is x[2 (T - 1) - t] (F.pad "reflect" on the right)
// -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int di_src(int t, int T) { return t < T ? t : 2 * (T - 1) - t; }

__global__ __launch_bounds__(256) void hifigan_disc_input_kernel(int B, int T, int p, int L0, int L1, const float* __restrict__ x,
                                                                 const float* __restrict__ w, const float* __restrict__ bias, float slope,
                                                                 float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t M = (int64_t)B * L1 * p;
  if (idx >= M * DI_C) return;
  const int o = (int)(idx % DI_C);
  const int64_t i = idx / DI_C;
  const int w_ = (int)(i % p);
  const int64_t q = i / p;
  const int lo = (int)(q % L1), b = (int)(q / L1);
  float v = bias[o];
#pragma unroll
  for (int j = 0; j < DT_TAPS; ++j) {
    const int l = 3 * lo + j - 2;
    if (l < 0 || l >= L0) continue;
    v += w[o * DT_TAPS + j] * x[(int64_t)b * T + di_src(l * p + w_, T)];
  }
  out[idx] = hg_lrelu(v, slope);
}

// weight / bias partials of the input layer: wpart [chunk][32][5], bpart [chunk][32] over chunks of DI_CHUNK global rows
__global__ __launch_bounds__(256) void hifigan_disc_input_wgrad_kernel(int B, int T, int p, int L0, int L1, const float* __restrict__ dy,
                                                                       const float* __restrict__ x, float* __restrict__ wpart,
                                                                       float* __restrict__ bpart) {
  __shared__ float sX[DI_CHUNK][DT_TAPS];
  __shared__ float red[8][DI_C][DT_TAPS + 1];
  const int tid = threadIdx.x;
  const int64_t M = (int64_t)B * L1 * p;
  const int64_t r0 = (int64_t)blockIdx.x * DI_CHUNK;
  const int nrows = M - r0 < DI_CHUNK ? (int)(M - r0) : DI_CHUNK;
  for (int idx = tid; idx < nrows * DT_TAPS; idx += 256) {
    const int r = idx / DT_TAPS, j = idx - r * DT_TAPS;
    const int64_t i = r0 + r;
    const int w_ = (int)(i % p);
    const int64_t q = i / p;
    const int lo = (int)(q % L1), b = (int)(q / L1);
    const int l = 3 * lo + j - 2;
    sX[r][j] = (l >= 0 && l < L0) ? x[(int64_t)b * T + di_src(l * p + w_, T)] : 0.f;
  }
  __syncthreads();
  const int o = tid & 31, rl = tid >> 5;
  float acc[DT_TAPS + 1] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = rl; r < nrows; r += 8) {
    const float d = dy[(r0 + r) * DI_C + o];
#pragma unroll
    for (int j = 0; j < DT_TAPS; ++j) acc[j] += d * sX[r][j];
    acc[DT_TAPS] += d;
  }
#pragma unroll
  for (int j = 0; j <= DT_TAPS; ++j) red[rl][o][j] = acc[j];
  __syncthreads();
  if (tid < DI_C * (DT_TAPS + 1)) {
    const int oo = tid / (DT_TAPS + 1), j = tid - oo * (DT_TAPS + 1);
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) s += red[q][oo][j];
    if (j < DT_TAPS) wpart[((int64_t)blockIdx.x * DI_C + oo) * DT_TAPS + j] = s;
    else bpart[(int64_t)blockIdx.x * DI_C + oo] = s;
  }
}

// gradient of the padded sample t of utterance b: the taps j = l + 2 mod 3 of its row l = t / p
__device__ __forceinline__ float di_gpad(int b, int t, int p, int L1, const float* __restrict__ dy, const float* __restrict__ w) {
  const int l = t / p, w_ = t - l * p;
  float s = 0.f;
  for (int j = 0; j < DT_TAPS; ++j) {
    const int num = l + 2 - j;
    if (num < 0 || num % 3) continue;
    const int lo = num / 3;
    if (lo >= L1) continue;
    const float* d = dy + (((int64_t)b * L1 + lo) * p + w_) * DI_C;
    float q = 0.f;
#pragma unroll 8
    for (int o = 0; o < DI_C; ++o) q += d[o] * w[o * DT_TAPS + j];
    s += q;
  }
  return s;
}

// dx (B, T): every sample gathers its own padded position and, where the reflect pad copied it, its mirror image 2 (T - 1) - t
__global__ __launch_bounds__(256) void hifigan_disc_input_dgrad_kernel(int B, int T, int p, int L0, int L1, const float* __restrict__ dy,
                                                                       const float* __restrict__ w, float* __restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * T) return;
  const int b = (int)(idx / T), t = (int)(idx - (int64_t)b * T);
  float s = di_gpad(b, t, p, L1, dy, w);
  const int tm = 2 * (T - 1) - t;
  if (tm >= T && tm < L0 * p) s += di_gpad(b, tm, p, L1, dy, w);
  dx[idx] = s;
}

// -----------------------------------------------------------------------------------------------------------------------------
// conv_post: C -> 1, k = 3, padding 1 along L, no activation.  w [3][C] (s2svc_hifigan_fold mode 2).
// -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hifigan_disc_post_kernel(int B, int L, int p, int C, const float* __restrict__ x,
                                                                const float* __restrict__ w, const float* __restrict__ bias,
                                                                float* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);          // wave-uniform
  if (i >= (int64_t)B * L * p) return;
  const int l = (int)((i / p) % L);
  float acc = 0.f;
  for (int j = 0; j < 3; ++j) {
    const int ll = l + j - 1;
    if (ll < 0 || ll >= L) continue;
    const float* xr = x + (i + (int64_t)(j - 1) * p) * C;
    const float* wr = w + j * C;
    for (int c = lane * 4; c < C; c += 256) {
      const float4 xv = *reinterpret_cast<const float4*>(xr + c);
      const float4 wv = *reinterpret_cast<const float4*>(wr + c);
      acc += xv.x * wv.x + xv.y * wv.y + xv.z * wv.z + xv.w * wv.w;
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) y[i] = acc + bias[0];
}

// backward: d = dy1 + dy2 (either may be NULL); dx = leaky_relu'(x) * (add + sum_j d[(l - j + 1, w)] w[j][c]);
// wpart [chunk][3][C] = sum over the chunk's rows of d[(l, w)] x[(l + j - 1, w)][c]; bpart [chunk] = sum d
__global__ __launch_bounds__(256) void hifigan_disc_post_bwd_kernel(int B, int L, int p, int C, const float* __restrict__ x,
                                                                    const float* __restrict__ w, const float* __restrict__ dy1,
                                                                    const float* __restrict__ dy2, const float* __restrict__ add,
                                                                    float slope, float* __restrict__ dx, float* __restrict__ wpart,
                                                                    float* __restrict__ bpart) {
  __shared__ float sT[DP_CHUNK][3];        // d of row (l - j + 1, w), zero outside the sequence
  __shared__ int sV[DP_CHUNK][3];          // row (l + j - 1, w) exists
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int64_t M = (int64_t)B * L * p;
  const int64_t r0 = (int64_t)blockIdx.x * DP_CHUNK;
  const int nrows = M - r0 < DP_CHUNK ? (int)(M - r0) : DP_CHUNK;
  for (int idx = tid; idx < nrows * 3; idx += 256) {
    const int r = idx / 3, j = idx - r * 3;
    const int64_t i = r0 + r;
    const int l = (int)((i / p) % L);
    const int ls = l - j + 1;
    float d = 0.f;
    if (ls >= 0 && ls < L) {
      const int64_t is = i + (int64_t)(1 - j) * p;
      d = (dy1 ? dy1[is] : 0.f) + (dy2 ? dy2[is] : 0.f);
    }
    sT[r][j] = d;
    const int lx = l + j - 1;
    sV[r][j] = lx >= 0 && lx < L;
  }
  __syncthreads();
  // blockIdx.y owns DP_CB channels: the serial loop over the chunk's rows below is spread over C / DP_CB workgroups
  const int cl = blockIdx.y * DP_CB, cw = min(DP_CB, C - cl);
  for (int idx = tid; idx < nrows * cw; idx += 256) {
    const int r = idx / cw, c = cl + idx - r * cw;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) s += sT[r][j] * w[j * C + c];
    const int64_t at = (r0 + r) * C + c;
    if (add) s += add[at];
    dx[at] = x[at] > 0.f ? s : s * slope;
  }
  for (int idx = tid; idx < 3 * cw; idx += 256) {
    const int j = idx / cw, c = cl + idx - j * cw;
    float s[4] = {0.f, 0.f, 0.f, 0.f};                    // four interleaved sums: chains of 64, not 256
    for (int r = 0; r < nrows; ++r)
      if (sV[r][j]) s[r & 3] += sT[r][1] * x[(r0 + r + (int64_t)(j - 1) * p) * C + c];
    wpart[((int64_t)blockIdx.x * 3 + j) * C + c] = (s[0] + s[1]) + (s[2] + s[3]);
  }
  if (blockIdx.y != 0) return;
  float bs = 0.f;
  for (int r = tid; r < nrows; r += 256) bs += sT[r][1];
  bs = wave_sum(bs);
  if ((tid & 63) == 0) red[tid >> 6] = bs;
  __syncthreads();
  if (tid == 0) bpart[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// -----------------------------------------------------------------------------------------------------------------------------
// weight and bias gradient partials of the strided convolution: wpart [chunk][C_out][5][C_in], bpart [chunk][C_out]
// -----------------------------------------------------------------------------------------------------------------------------
struct DwArgs {
  const float* dy;       // (B, Lo, p, Cout): gradient of the pre-activation
  const float* x;        // (B, Li, p, Cin): the layer's input
  float* wpart;
  float* bpart;
  int64_t M;             // B * Lo * p
  int B, Li, Lo, p, Cin, Cout, stride, ctiles;
};

__device__ __forceinline__ f32x4_t dw_frag(const float* s, int col, int ks, int lg) {
  f32x4_t f;
#pragma unroll
  for (int e = 0; e < 4; ++e) f[e] = s[(ks * 16 + 4 * lg + e) * DW_ROW + col];
  return f;
}

__global__ __launch_bounds__(256) void hifigan_disc_wgrad_kernel(const DwArgs a) {
  typedef HgFrag<float> F;
  __shared__ __attribute__((aligned(16))) float sD[DW_TS * DW_ROW];
  __shared__ __attribute__((aligned(16))) float sX[DT_TAPS * DW_TS * DW_ROW];
  __shared__ float sBias[8][32];
  constexpr int KS = DW_TS / F::KSTEP, NITEMS = 2 * DT_TAPS, NQ = (NITEMS + 3) / 4;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int mt = blockIdx.y / a.ctiles, ct = blockIdx.y - mt * a.ctiles;
  const int m0 = mt * 32, c0 = ct * 32;
  const int64_t r0 = (int64_t)blockIdx.x * DW_CHUNK, r1 = r0 + DW_CHUNK < a.M ? r0 + DW_CHUNK : a.M;
  const int p = a.p;

  float acc[NQ][2][4];                                    // plain floats, added one by one: the library holds no packed-fp32 adds
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int ci = 0; ci < 2; ++ci)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[q][ci][e] = 0.f;
  float bsum = 0.f;

  for (int64_t tk = r0; tk < r1; tk += DW_TS) {
    __syncthreads();
    {
      const int r = tid >> 3, v = tid & 7;
      const int64_t i = tk + r;
      const int m = m0 + v * 4;
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (i < r1 && m + 4 <= a.Cout) val = *reinterpret_cast<const uint4*>(a.dy + i * a.Cout + m);
      *reinterpret_cast<uint4*>(sD + r * DW_ROW + v * 4) = val;
      const int c = c0 + v * 4;
      int lo = 0, w = 0;
      int64_t b = 0;
      if (i < r1) {
        w = (int)(i % p);
        const int64_t q = i / p;
        lo = (int)(q % a.Lo);
        b = q / a.Lo;
      }
#pragma unroll
      for (int j = 0; j < DT_TAPS; ++j) {
        const int l = a.stride * lo + j - 2;
        uint4 xv = make_uint4(0u, 0u, 0u, 0u);
        if (i < r1 && l >= 0 && l < a.Li && c + 4 <= a.Cin) xv = *reinterpret_cast<const uint4*>(a.x + ((b * a.Li + l) * p + w) * a.Cin + c);
        *reinterpret_cast<uint4*>(sX + (j * DW_TS + r) * DW_ROW + v * 4) = xv;
      }
    }
    __syncthreads();
    if (ct == 0) {
      const int col = tid & 31;
      for (int r = tid >> 5; r < DW_TS; r += 8) bsum += sD[r * DW_ROW + col];
    }
    f32x4_t stp[NQ][2];                                   // this step's 32 rows on their own, then one addition into the chunk's sum
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int ci = 0; ci < 2; ++ci) stp[q][ci] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int item = wave + 4 * q;
        if (item < NITEMS) {
          const int j = item >> 1, mi = item & 1;
          const f32x4_t fa = dw_frag(sD, mi * 16 + lr, ks, lg);
#pragma unroll
          for (int ci = 0; ci < 2; ++ci) {
            const f32x4_t fb = dw_frag(sX + j * DW_TS * DW_ROW, ci * 16 + lr, ks, lg);
            stp[q][ci] = F::mma(fa, fb, stp[q][ci]);
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int ci = 0; ci < 2; ++ci)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[q][ci][e] += stp[q][ci][e];
  }

  const int64_t pbase = (int64_t)blockIdx.x * a.Cout;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int item = wave + 4 * q;
    if (item >= NITEMS) continue;
    const int j = item >> 1, mi = item & 1;
#pragma unroll
    for (int ci = 0; ci < 2; ++ci) {
      const int c = c0 + ci * 16 + lr;
      if (c >= a.Cin) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + mi * 16 + lg * 4 + r;
        if (m < a.Cout) a.wpart[((pbase + m) * DT_TAPS + j) * a.Cin + c] = acc[q][ci][r];
      }
    }
  }
  if (ct == 0) {
    sBias[tid >> 5][tid & 31] = bsum;
    __syncthreads();
    if (tid < 32 && m0 + tid < a.Cout) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) s += sBias[q][tid];
      a.bpart[pbase + m0 + tid] = s;
    }
  }
}

inline bool disc_shape_ok(int B, int L, int p, int Cin, int Cout, int stride) {
  return B >= 1 && L >= 1 && p >= 1 && Cin >= 4 && Cin % 4 == 0 && Cout >= 4 && Cout % 4 == 0 && Cin <= 4096 && Cout <= 4096 &&
         (stride == 1 || stride == 3) && (int64_t)B * L * p < (1ll << 31);
}

}  // namespace

extern "C" int s2svc_hifigan_disc_input(int B, int T, int p, const float* x, const float* w32, const float* bias, float slope, float* out,
                                        void* stream) {
  S2S_REQUIRE(B >= 1 && T >= 1 && p >= 1 && p <= T && (int64_t)B * (T + p) < (1ll << 31) / DI_C, "hifigan_disc_input: 1 <= p <= T, B * T * 32 < 2^31");
  S2S_REQUIRE(x && w32 && bias && out, "hifigan_disc_input: null pointer");
  const int L0 = (T + p - 1) / p, L1 = (L0 - 1) / 3 + 1;
  const int64_t n = (int64_t)B * L1 * p * DI_C;
  hipLaunchKernelGGL(hifigan_disc_input_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, T, p, L0, L1, x, w32,
                     bias, slope, out);
  S2S_CHECK_LAUNCH("hifigan_disc_input_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_disc_conv(int B, int L, int p, int Cin, int Cout, int stride, const float* x, const float* w_op, const float* bias,
                                       float slope, float* out, void* stream) {
  S2S_REQUIRE(disc_shape_ok(B, L, p, Cin, Cout, stride) && Cin % DT_KC == 0, "hifigan_disc_conv: stride 1 or 3, C_in a multiple of 16, C_out of 4");
  S2S_REQUIRE(x && w_op && bias && out && hg_aligned16(x) && hg_aligned16(w_op), "hifigan_disc_conv: null or unaligned pointer");
  DtArgs a = {};
  a.a = x; a.w = w_op; a.bias = bias; a.out = out;
  a.B = B; a.La = L; a.Lo = (L - 1) / stride + 1; a.p = p; a.Ka = Cin; a.Kap = hg_pad32(Cin); a.N = Cout;
  a.sa = stride; a.so = 1; a.nph = 1; a.ntaps[0] = DT_TAPS;
  for (int t = 0; t < DT_TAPS; ++t) { a.off[0][t] = t - 2; a.wtap[0][t] = t; }
  a.slope = slope; a.act = 1;
  return dt_launch("hifigan_disc_conv", a, (hipStream_t)stream);
}

extern "C" int s2svc_hifigan_disc_dgrad(int B, int L, int p, int Cin, int Cout, int stride, const float* dy, const float* w_opT,
                                        const float* mask_src, const float* add, float slope, float* dx, void* stream) {
  S2S_REQUIRE(disc_shape_ok(B, L, p, Cin, Cout, stride) && Cout % DT_KC == 0, "hifigan_disc_dgrad: stride 1 or 3, C_out a multiple of 16, C_in of 4");
  S2S_REQUIRE(dy && w_opT && dx && hg_aligned16(dy) && hg_aligned16(w_opT), "hifigan_disc_dgrad: null or unaligned pointer");
  DtArgs a = {};
  a.a = dy; a.w = w_opT; a.mask = mask_src; a.add = add; a.out = dx;
  a.B = B; a.La = (L - 1) / stride + 1; a.Lo = L; a.p = p; a.Ka = Cout; a.Kap = hg_pad32(Cout); a.N = Cin;
  a.sa = 1; a.slope = slope; a.act = 0;
  if (stride == 1) {
    a.so = 1; a.nph = 1; a.ntaps[0] = DT_TAPS;
    for (int t = 0; t < DT_TAPS; ++t) { a.off[0][t] = t - 2; a.wtap[0][t] = t; }
  } else {
    // input row l = 3 g + r receives forward tap j from output row lo with 3 lo + j - 2 = l; the operand holds tap j at slot 4 - j
    a.so = 3; a.nph = 3;
    a.ntaps[0] = 1; a.off[0][0] = 0; a.wtap[0][0] = 2;                                   // r = 0: j = 2
    a.ntaps[1] = 2; a.off[1][0] = 0; a.wtap[1][0] = 1; a.off[1][1] = 1; a.wtap[1][1] = 4;   // r = 1: j = 3 (lo = g), j = 0 (lo = g + 1)
    a.ntaps[2] = 2; a.off[2][0] = 0; a.wtap[2][0] = 0; a.off[2][1] = 1; a.wtap[2][1] = 3;   // r = 2: j = 4 (lo = g), j = 1 (lo = g + 1)
  }
  return dt_launch("hifigan_disc_dgrad", a, (hipStream_t)stream);
}

extern "C" int s2svc_hifigan_disc_wgrad(int B, int L, int p, int Cin, int Cout, int stride, const float* dy, const float* x, float* wpart,
                                        float* bpart, void* stream) {
  S2S_REQUIRE(disc_shape_ok(B, L, p, Cin, Cout, stride), "hifigan_disc_wgrad: stride 1 or 3, channels multiples of 4");
  S2S_REQUIRE(dy && x && wpart && bpart && hg_aligned16(dy) && hg_aligned16(x), "hifigan_disc_wgrad: null or unaligned pointer");
  DwArgs a = {};
  a.dy = dy; a.x = x; a.wpart = wpart; a.bpart = bpart;
  a.B = B; a.Li = L; a.Lo = (L - 1) / stride + 1; a.p = p; a.Cin = Cin; a.Cout = Cout; a.stride = stride;
  a.M = (int64_t)B * a.Lo * p;
  a.ctiles = (Cin + 31) / 32;
  const int64_t gy = (int64_t)((Cout + 31) / 32) * a.ctiles;
  S2S_REQUIRE(gy <= 65535, "hifigan_disc_wgrad: grid too large");
  const dim3 grid((unsigned)((a.M + DW_CHUNK - 1) / DW_CHUNK), (unsigned)gy), block(256);
  hipLaunchKernelGGL(hifigan_disc_wgrad_kernel, grid, block, 0, (hipStream_t)stream, a);
  S2S_CHECK_LAUNCH("hifigan_disc_wgrad_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_disc_input_wgrad(int B, int T, int p, const float* dy, const float* x, float* wpart, float* bpart, void* stream) {
  S2S_REQUIRE(B >= 1 && T >= 1 && p >= 1 && p <= T && (int64_t)B * (T + p) < (1ll << 31) / DI_C, "hifigan_disc_input_wgrad: 1 <= p <= T, B * T * 32 < 2^31");
  S2S_REQUIRE(dy && x && wpart && bpart, "hifigan_disc_input_wgrad: null pointer");
  const int L0 = (T + p - 1) / p, L1 = (L0 - 1) / 3 + 1;
  const int64_t M = (int64_t)B * L1 * p;
  hipLaunchKernelGGL(hifigan_disc_input_wgrad_kernel, dim3((unsigned)((M + DI_CHUNK - 1) / DI_CHUNK)), dim3(256), 0, (hipStream_t)stream, B, T, p,
                     L0, L1, dy, x, wpart, bpart);
  S2S_CHECK_LAUNCH("hifigan_disc_input_wgrad_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_disc_input_dgrad(int B, int T, int p, const float* dy, const float* w32, float* dx, void* stream) {
  S2S_REQUIRE(B >= 1 && T >= 1 && p >= 1 && p <= T && (int64_t)B * (T + p) < (1ll << 31) / DI_C, "hifigan_disc_input_dgrad: 1 <= p <= T, B * T * 32 < 2^31");
  S2S_REQUIRE(dy && w32 && dx, "hifigan_disc_input_dgrad: null pointer");
  const int L0 = (T + p - 1) / p, L1 = (L0 - 1) / 3 + 1;
  const int64_t n = (int64_t)B * T;
  hipLaunchKernelGGL(hifigan_disc_input_dgrad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, T, p, L0, L1, dy,
                     w32, dx);
  S2S_CHECK_LAUNCH("hifigan_disc_input_dgrad_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_disc_post(int B, int L, int p, int C, const float* x, const float* w, const float* bias, float* y, void* stream) {
  S2S_REQUIRE(B >= 1 && L >= 1 && p >= 1 && C >= 4 && C % 4 == 0 && (int64_t)B * L * p < (1ll << 31), "hifigan_disc_post: bad shape (C a multiple of 4)");
  S2S_REQUIRE(x && w && bias && y && hg_aligned16(x) && hg_aligned16(w), "hifigan_disc_post: null or unaligned pointer");
  const int64_t M = (int64_t)B * L * p;
  hipLaunchKernelGGL(hifigan_disc_post_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, B, L, p, C, x, w, bias, y);
  S2S_CHECK_LAUNCH("hifigan_disc_post_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_disc_post_bwd(int B, int L, int p, int C, const float* x, const float* w, const float* dy1, const float* dy2,
                                           const float* add, float slope, float* dx, float* wpart, float* bpart, void* stream) {
  S2S_REQUIRE(B >= 1 && L >= 1 && p >= 1 && C >= 1 && (int64_t)B * L * p < (1ll << 31), "hifigan_disc_post_bwd: bad shape");
  S2S_REQUIRE(x && w && dx && wpart && bpart, "hifigan_disc_post_bwd: null pointer");
  const int64_t M = (int64_t)B * L * p;
  hipLaunchKernelGGL(hifigan_disc_post_bwd_kernel, dim3((unsigned)((M + DP_CHUNK - 1) / DP_CHUNK), (unsigned)((C + DP_CB - 1) / DP_CB)), dim3(256), 0,
                     (hipStream_t)stream, B, L, p, C, x, w, dy1, dy2, add, slope, dx, wpart, bpart);
  S2S_CHECK_LAUNCH("hifigan_disc_post_bwd_kernel");
  return 0;
}
