// HiFi-GAN multi-scale discriminator, forward and backward, fp32 (reference: seq2seq_vc/urhythmic/vocoder.py:330-402 --
// ScaleDiscriminator, MultiScaleDiscriminator; urhythmic_fine_tune_vocoder.py:191-222 calls it four times per step and
// backpropagates through it twice).
//
// A scale discriminator is eight Conv1d layers over x (B, 1, T), the middle five grouped with 41 taps and strides 2, 2, 4, 4, 1.
// Activations are channel-last (B, L, C) and hold the POST-activation values (they are the features the caller receives).  A
// convolution (k taps, padding (k - 1) / 2, stride s) maps L to (L - 1) / s + 1; rows outside [0, L) of an utterance are zero: every
// loader decodes (b, l) of the row it fetches and never steps into the neighbouring utterance, and a column tile lies inside one group.
//
//   pool              hifigan_msd_pool_kernel / _pool_bwd_kernel: AvgPool1d(4, 2, padding 2) (the padding counts) and its adjoint.
//   input layer       hifigan_msd_input_kernel: 1 -> 128 channels, 15 taps, straight from x, bias and leaky_relu in the launch; weight
//                     partials per chunk of 256 rows; dx is a gather, one wavefront per sample.
//   grouped conv      hifigan_msd_tile_kernel: implicit GEMM on v_mfma_f32_16x16x4_f32 (HgFrag<float>), 128 rows x (16 | 32 | 64)
//                     columns of ONE group per workgroup, 16 channels per step.  The input rows a tile needs for all 41 taps (<= 549 at
//                     stride 4) are staged once per step; the weight fragments come from global memory (41 taps x 64 columns do not
//                     fit beside the rows), the next tap's in flight while this tap's MFMAs run.  The same kernel is the data gradient,
//                     phase-decomposed: input row l receives only the taps j = l + 20 (mod s), one grid plane per phase.
//   weight gradient   hifigan_msd_wgrad_kernel: partials per chunk of rows of one utterance, laid out as s2svc_hifigan_wgrad_finish
//                     mode 0 sums them ([chunks][C_out][41][C_in / groups]); seven taps per grid plane.
//   spectral norm     the power iteration, sigma, W / sigma and the backward of the division: small launches, every norm and dot
//                     product in double, summed in an order fixed by the shapes.
//
// Layer 6 (1024 -> 1024, 5 taps) and conv_post are the multi-period discriminator's kernels at p = 1 (hifigan_disc.hip).
// There are no atomics: two calls give the same bits.
#include "hifigan_tile.h"

namespace {

constexpr int MT_BM = 128, MT_KC = 16, MT_TAPS = 41, MT_PAD = 20, MT_MAXR = 552, MT_OCT = 8;
constexpr int MT_ROWB = MT_KC * 4 + 16;                  // LDS row in bytes, padded
constexpr int MW_TS = 32, MW_ROW = 36, MW_TG = 7, MW_MAXS = 4;   // wgrad: rows per step, floats per LDS row, taps per grid plane
constexpr int MW_WIN = MW_MAXS * (MW_TS - 1) + MW_TG;    // input rows one step of one plane reads
constexpr int MI_C = 128, MI_TAPS = 15, MI_PAD = 7, MI_CHUNK = 256;

// -----------------------------------------------------------------------------------------------------------------------------
// the tile, group grp, phase ph, tap t < nt:
//   out[(b, so * q + ph)][grp * Ng + n] = epi( sum_t sum_c a[(b, sa * q + off0 + doff * t)][grp * Kag + c] * W[grp * Ng + n][(w0 + dw * t) * Kap + c] )
// forward: sa = stride, so = 1, off0 = -20, doff = 1, w0 = 0, dw = 1.  data gradient: sa = 1, so = stride, tap j = j0 + stride * t with
// j0 = (ph + 20) mod stride reads output row q + (ph + 20 - j) / stride: off0 = (ph + 20 - j0) / stride, doff = -1, w0 = j0, dw = stride.
// -----------------------------------------------------------------------------------------------------------------------------
struct MtArgs {
  const float* a;        // (B, La, Ca)
  const float* w;        // [groups * Ng][MT_TAPS * Kap]
  const float* bias;     // [groups * Ng] or NULL
  const float* mask;     // (B, Lo, groups * Ng) or NULL: multiply by leaky_relu'(mask)
  const float* add;      // (B, Lo, groups * Ng) or NULL: added before the mask
  float* out;            // (B, Lo, groups * Ng)
  int B, La, Lo, groups, Kag, Kap, Ng;
  int sa, so, stride, dgrad, tiles, ctiles;
  float slope;
  int act;               // 1: out = leaky_relu(acc + bias)
};

struct MtPhase { int nt, off0, doff, w0, dw; };

__host__ __device__ inline MtPhase mt_phase(int dgrad, int stride, int ph) {
  MtPhase p;
  if (!dgrad) { p.nt = MT_TAPS; p.off0 = -MT_PAD; p.doff = 1; p.w0 = 0; p.dw = 1; return p; }
  const int j0 = (ph + MT_PAD) % stride;
  p.nt = (MT_TAPS - 1 - j0) / stride + 1; p.off0 = (ph + MT_PAD - j0) / stride; p.doff = -1; p.w0 = j0; p.dw = stride;
  return p;
}

template <int NT>
__global__ __launch_bounds__(256) void hifigan_msd_tile_kernel(const MtArgs a) {
  typedef HgFrag<float> F;
  __shared__ __attribute__((aligned(16))) unsigned char sA[MT_MAXR * MT_ROWB];
  constexpr int VPR = MT_KC / 4, BN = NT * 16;

  const int ph = blockIdx.z;
  const int G = a.Lo > ph ? (a.Lo - ph + a.so - 1) / a.so : 0;      // rows l = so * q + ph < Lo of this phase
  const int b = blockIdx.x / a.tiles;
  const int i0 = (blockIdx.x - b * a.tiles) * MT_BM;
  if (i0 >= G) return;
  const int grp = blockIdx.y / a.ctiles;
  const int n0 = (blockIdx.y - grp * a.ctiles) * BN;
  const MtPhase P = mt_phase(a.dgrad, a.stride, ph);
  const int offl = P.off0 + P.doff * (P.nt - 1);
  const int offmin = min(P.off0, offl), offmax = max(P.off0, offl);
  const int ilast = min(i0 + MT_BM, G) - 1;
  const int lbase = a.sa * i0 + offmin;
  const int R = min(a.sa * (ilast - i0) + offmax - offmin + 1, MT_MAXR);         // the launcher has checked the bound

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int Kp = MT_TAPS * a.Kap;
  const int Ca = a.groups * a.Kag, Nall = a.groups * a.Ng;
  const float* ab = a.a + (int64_t)b * a.La * Ca + grp * a.Kag;

  int abase[2];                                           // LDS row of the lane's A rows at offset offmin
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) abase[mt] = a.sa * (min(i0 + wave * 32 + mt * 16 + lr, ilast) - i0) - offmin;
  const float* wrow[NT];                                  // the lane's weight rows (its column of every column tile), NULL past the group
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = n0 + nt * 16 + lr;
    wrow[nt] = n < a.Ng ? a.w + (int64_t)(grp * a.Ng + n) * Kp + lg * 4 : nullptr;
  }

  // Three levels of accumulation, so that no fp32 chain is longer than 32 MFMA results + 8 + 3 additions: acc = eight taps of this
  // step's 16 channels, grp8 = eight of those, tot = the rest.  The order depends on the shapes only.
  const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
  float tot[2][NT][4], grp8[2][NT][4];                    // plain floats, added one by one: the library holds no packed-fp32 adds
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) tot[mt][nt][e] = grp8[mt][nt][e] = 0.f;

  int octets = 0;
  for (int c0 = 0; c0 < a.Kag; c0 += MT_KC) {
    __syncthreads();                                      // the previous step's fragments have been read
    for (int idx = tid; idx < R * VPR; idx += 256) {
      const int r = idx / VPR, v = idx - r * VPR;
      const int l = lbase + r, c = c0 + v * 4;
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (l >= 0 && l < a.La && c + 4 <= a.Kag) val = *reinterpret_cast<const uint4*>(ab + (int64_t)l * Ca + c);
      *reinterpret_cast<uint4*>(sA + r * MT_ROWB + v * 16) = val;
    }
    __syncthreads();
    const bool kin = c0 + lg * 4 + 4 <= a.Kag;            // the lane's four reduction columns lie inside the group
    f32x4_t fbn[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      fbn[nt] = (kin && wrow[nt]) ? *reinterpret_cast<const f32x4_t*>(wrow[nt] + P.w0 * a.Kap + c0) : zero4;
    for (int t0 = 0; t0 < P.nt; t0 += MT_OCT) {
      f32x4_t acc[2][NT];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = zero4;
      const int t1 = min(t0 + MT_OCT, P.nt);
      for (int t = t0; t < t1; ++t) {
        f32x4_t fa[2], fb[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) fb[nt] = fbn[nt];
        if (t + 1 < P.nt) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            fbn[nt] = (kin && wrow[nt]) ? *reinterpret_cast<const f32x4_t*>(wrow[nt] + (P.w0 + P.dw * (t + 1)) * a.Kap + c0) : zero4;
        }
        const int toff = P.off0 + P.doff * t;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) fa[mt] = *reinterpret_cast<const f32x4_t*>(sA + (abase[mt] + toff) * MT_ROWB + lg * 16);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = F::mma(fa[mt], fb[nt], acc[mt][nt]);
      }
      const bool fold = (++octets & 7) == 0;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            grp8[mt][nt][e] += acc[mt][nt][e];
            if (fold) { tot[mt][nt][e] += grp8[mt][nt][e]; grp8[mt][nt][e] = 0.f; }
          }
    }
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) tot[mt][nt][e] += grp8[mt][nt][e];

  const int64_t ob = (int64_t)b * a.Lo * Nall;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = n0 + nt * 16 + lr;
    if (n >= a.Ng) continue;
    const int ng = grp * a.Ng + n;
    const float bv = a.bias ? a.bias[ng] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wave * 32 + mt * 16 + lg * 4 + r;
        if (i >= G) continue;
        const int64_t at = ob + (int64_t)(a.so * i + ph) * Nall + ng;
        float v = tot[mt][nt][r] + bv;
        if (a.act) v = hg_lrelu(v, a.slope);
        if (a.add) v += a.add[at];
        if (a.mask) v = a.mask[at] > 0.f ? v : v * a.slope;
        a.out[at] = v;
      }
  }
}

int mt_launch(const char* who, MtArgs& a, hipStream_t st) {
  const int nph = a.dgrad ? a.stride : 1;
  int gmax = 0;
  for (int ph = 0; ph < nph; ++ph) {
    const MtPhase P = mt_phase(a.dgrad, a.stride, ph);
    const int span = (P.nt - 1);                          // |doff| = 1
    if (a.sa * (MT_BM - 1) + span + 1 > MT_MAXR) return hg_fail(who, "stride too large for the staged tile (552 rows)");
    const int G = a.Lo > ph ? (a.Lo - ph + a.so - 1) / a.so : 0;
    gmax = G > gmax ? G : gmax;
  }
  a.tiles = (gmax + MT_BM - 1) / MT_BM;
  const int bn = a.Ng > 32 ? 64 : (a.Ng > 16 ? 32 : 16);
  a.ctiles = (a.Ng + bn - 1) / bn;
  if ((int64_t)a.B * a.tiles >= (1ll << 31) || (int64_t)a.groups * a.ctiles > 65535) return hg_fail(who, "grid too large");
  if ((int64_t)a.B * a.La * a.groups * a.Kag >= (1ll << 40) || (int64_t)a.B * a.Lo * a.groups * a.Ng >= (1ll << 40)) return hg_fail(who, "tensor too large");
  const dim3 grid(a.B * a.tiles, a.groups * a.ctiles, nph), block(256);
  if (bn == 64) hipLaunchKernelGGL(hifigan_msd_tile_kernel<4>, grid, block, 0, st, a);
  else if (bn == 32) hipLaunchKernelGGL(hifigan_msd_tile_kernel<2>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(hifigan_msd_tile_kernel<1>, grid, block, 0, st, a);
  S2S_CHECK_LAUNCH("hifigan_msd_tile_kernel");
  return 0;
}

// operand of the data gradient: w32 (O, Cg, 41), O = groups * Og -> [groups * Cg][41 * Ogp], [(g, c)][j * Ogp + o] = w32[g * Og + o][c][j]
__global__ __launch_bounds__(256) void hifigan_msd_fold_bwd_kernel(int Og, int Cg, int Ogp, const float* __restrict__ w32, float* __restrict__ opT) {
  const int row = blockIdx.x, g = row / Cg, c = row - g * Cg;
  for (int idx = threadIdx.x; idx < MT_TAPS * Ogp; idx += 256) {
    const int j = idx / Ogp, o = idx - j * Ogp;
    opT[(int64_t)row * MT_TAPS * Ogp + idx] = o < Og ? w32[((int64_t)(g * Og + o) * Cg + c) * MT_TAPS + j] : 0.f;
  }
}

// -----------------------------------------------------------------------------------------------------------------------------
// weight and bias gradient partials of the grouped convolution: wpart [chunk][C_out][41][Cg], bpart [chunk][C_out]; chunk q of
// utterance b covers output rows [q * chunk, q * chunk + chunk) of that utterance
// -----------------------------------------------------------------------------------------------------------------------------
struct MwArgs {
  const float* dy;       // (B, Lo, Cout): gradient of the pre-activation
  const float* x;        // (B, L, Cin): the layer's input
  float* wpart;
  float* bpart;
  int B, L, Lo, Cin, Cout, groups, Cg, Mg, stride, chunk, ncpu, mtiles, ctiles;
};

__global__ __launch_bounds__(256) void hifigan_msd_wgrad_kernel(const MwArgs a) {
  typedef HgFrag<float> F;
  __shared__ __attribute__((aligned(16))) float sD[MW_TS * MW_ROW];
  __shared__ __attribute__((aligned(16))) float sX[MW_WIN * MW_ROW];
  __shared__ float sBias[8][32];
  constexpr int KS = MW_TS / F::KSTEP, NITEMS = 2 * MW_TG, NQ = (NITEMS + 3) / 4;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  int y = blockIdx.y;
  const int ct = y % a.ctiles; y /= a.ctiles;
  const int mt = y % a.mtiles;
  const int grp = y / a.mtiles;
  const int m0 = mt * 32, c0 = ct * 32, j0 = blockIdx.z * MW_TG, s = a.stride;
  const int b = blockIdx.x / a.ncpu, q = blockIdx.x - b * a.ncpu;
  const int r0 = q * a.chunk, r1 = min(r0 + a.chunk, a.Lo);
  const int win = s * (MW_TS - 1) + MW_TG;
  const float* dyb = a.dy + (int64_t)b * a.Lo * a.Cout + grp * a.Mg;
  const float* xb = a.x + (int64_t)b * a.L * a.Cin + grp * a.Cg;
  const bool bias_owner = ct == 0 && blockIdx.z == 0;

  float acc[NQ][2][4];                                    // plain floats, added one by one: the library holds no packed-fp32 adds
#pragma unroll
  for (int qq = 0; qq < NQ; ++qq)
#pragma unroll
    for (int ci = 0; ci < 2; ++ci)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[qq][ci][e] = 0.f;
  float bsum = 0.f;

  for (int tk = r0; tk < r1; tk += MW_TS) {
    __syncthreads();
    {
      const int r = tid >> 3, v = tid & 7;
      const int m = m0 + v * 4;
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (tk + r < r1 && m + 4 <= a.Mg) val = *reinterpret_cast<const uint4*>(dyb + (int64_t)(tk + r) * a.Cout + m);
      *reinterpret_cast<uint4*>(sD + r * MW_ROW + v * 4) = val;
    }
    const int lw = s * tk + j0 - MT_PAD;                  // input row of window row 0
    for (int idx = tid; idx < win * 8; idx += 256) {
      const int r = idx >> 3, v = idx & 7;
      const int l = lw + r, c = c0 + v * 4;
      uint4 xv = make_uint4(0u, 0u, 0u, 0u);
      if (l >= 0 && l < a.L && c + 4 <= a.Cg) xv = *reinterpret_cast<const uint4*>(xb + (int64_t)l * a.Cin + c);
      *reinterpret_cast<uint4*>(sX + r * MW_ROW + v * 4) = xv;
    }
    __syncthreads();
    if (bias_owner) {
      const int col = tid & 31;
      for (int r = tid >> 5; r < MW_TS; r += 8) bsum += sD[r * MW_ROW + col];
    }
    f32x4_t stp[NQ][2];                                   // this step's 32 rows on their own, then one addition into the chunk's sum
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq)
#pragma unroll
      for (int ci = 0; ci < 2; ++ci) stp[qq][ci] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int qq = 0; qq < NQ; ++qq) {
        const int item = wave + 4 * qq;
        if (item < NITEMS) {
          const int jj = item >> 1, mi = item & 1;
          f32x4_t fa;
#pragma unroll
          for (int e = 0; e < 4; ++e) fa[e] = sD[(ks * 16 + 4 * lg + e) * MW_ROW + mi * 16 + lr];
#pragma unroll
          for (int ci = 0; ci < 2; ++ci) {
            f32x4_t fb;
#pragma unroll
            for (int e = 0; e < 4; ++e) fb[e] = sX[(s * (ks * 16 + 4 * lg + e) + jj) * MW_ROW + ci * 16 + lr];
            stp[qq][ci] = F::mma(fa, fb, stp[qq][ci]);
          }
        }
      }
    }
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq)
#pragma unroll
      for (int ci = 0; ci < 2; ++ci)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[qq][ci][e] += stp[qq][ci][e];
  }

  const int64_t pbase = (int64_t)blockIdx.x * a.Cout + grp * a.Mg;
#pragma unroll
  for (int qq = 0; qq < NQ; ++qq) {
    const int item = wave + 4 * qq;
    if (item >= NITEMS) continue;
    const int j = j0 + (item >> 1), mi = item & 1;
    if (j >= MT_TAPS) continue;
#pragma unroll
    for (int ci = 0; ci < 2; ++ci) {
      const int c = c0 + ci * 16 + lr;
      if (c >= a.Cg) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + mi * 16 + lg * 4 + r;
        if (m < a.Mg) a.wpart[((pbase + m) * MT_TAPS + j) * a.Cg + c] = acc[qq][ci][r];
      }
    }
  }
  if (bias_owner) {
    sBias[tid >> 5][tid & 31] = bsum;
    __syncthreads();
    if (tid < 32 && m0 + tid < a.Mg) {
      float sum = 0.f;
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) sum += sBias[qq][tid];
      a.bpart[pbase + m0 + tid] = sum;
    }
  }
}

// -----------------------------------------------------------------------------------------------------------------------------
// the average pool between the scales and its adjoint: y[t] = 0.25 * sum_{j < 4} x[2 t - 2 + j], zeros outside, To = T / 2 + 1
// -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hifigan_msd_pool_kernel(int B, int T, int To, const float* __restrict__ x, float* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * To) return;
  const int b = (int)(idx / To), t = (int)(idx - (int64_t)b * To);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = 2 * t - 2 + j;
    if (i >= 0 && i < T) s += x[(int64_t)b * T + i];
  }
  y[idx] = 0.25f * s;
}

// dx[i] = 0.25 * sum of dy[t] over the (t, j) with 2 t - 2 + j = i: t = (i + 2 - j) / 2 for the two j of i's parity, in ascending j
__global__ __launch_bounds__(256) void hifigan_msd_pool_bwd_kernel(int B, int T, int To, const float* __restrict__ dy, float* __restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * T) return;
  const int b = (int)(idx / T), i = (int)(idx - (int64_t)b * T);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int num = i + 2 - j;
    if (num < 0 || (num & 1)) continue;
    const int t = num >> 1;
    if (t < To) s += dy[(int64_t)b * To + t];
  }
  dx[idx] = 0.25f * s;
}

// -----------------------------------------------------------------------------------------------------------------------------
// input layer: x (B, T) -> (B, T, 128), 15 taps, padding 7
// -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hifigan_msd_input_kernel(int B, int T, const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float slope, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * T * MI_C) return;
  const int o = (int)(idx % MI_C);
  const int64_t i = idx / MI_C;
  const int t = (int)(i % T);
  float v = bias[o];
#pragma unroll
  for (int j = 0; j < MI_TAPS; ++j) {
    const int l = t + j - MI_PAD;
    if (l < 0 || l >= T) continue;
    v += w[o * MI_TAPS + j] * x[i + (j - MI_PAD)];
  }
  out[idx] = hg_lrelu(v, slope);
}

// weight / bias partials of the input layer: wpart [chunk][128][15], bpart [chunk][128] over chunks of MI_CHUNK rows of B * T
__global__ __launch_bounds__(256) void hifigan_msd_input_wgrad_kernel(int B, int T, const float* __restrict__ dy, const float* __restrict__ x,
                                                                      float* __restrict__ wpart, float* __restrict__ bpart) {
  __shared__ float sX[MI_CHUNK][MI_TAPS + 1];
  __shared__ float red[2][MI_C][MI_TAPS + 2];
  const int tid = threadIdx.x;
  const int64_t M = (int64_t)B * T;
  const int64_t r0 = (int64_t)blockIdx.x * MI_CHUNK;
  const int nrows = M - r0 < MI_CHUNK ? (int)(M - r0) : MI_CHUNK;
  for (int idx = tid; idx < nrows * MI_TAPS; idx += 256) {
    const int r = idx / MI_TAPS, j = idx - r * MI_TAPS;
    const int64_t i = r0 + r;
    const int l = (int)(i % T) + j - MI_PAD;
    sX[r][j] = (l >= 0 && l < T) ? x[i + (j - MI_PAD)] : 0.f;
  }
  __syncthreads();
  const int o = tid & (MI_C - 1), rl = tid >> 7;
  float acc[MI_TAPS + 1];
#pragma unroll
  for (int j = 0; j <= MI_TAPS; ++j) acc[j] = 0.f;
  for (int r = rl; r < nrows; r += 2) {
    const float d = dy[(r0 + r) * MI_C + o];
#pragma unroll
    for (int j = 0; j < MI_TAPS; ++j) acc[j] += d * sX[r][j];
    acc[MI_TAPS] += d;
  }
#pragma unroll
  for (int j = 0; j <= MI_TAPS; ++j) red[rl][o][j] = acc[j];
  __syncthreads();
  for (int idx = tid; idx < MI_C * (MI_TAPS + 1); idx += 256) {
    const int oo = idx / (MI_TAPS + 1), j = idx - oo * (MI_TAPS + 1);
    const float sum = red[0][oo][j] + red[1][oo][j];
    if (j < MI_TAPS) wpart[((int64_t)blockIdx.x * MI_C + oo) * MI_TAPS + j] = sum;
    else bpart[(int64_t)blockIdx.x * MI_C + oo] = sum;
  }
}

// dx (B, T): sample t gathers dy[t + 7 - j][o] * w[o][j] over the 15 taps and 128 channels; one wavefront per sample
__global__ __launch_bounds__(256) void hifigan_msd_input_dgrad_kernel(int B, int T, const float* __restrict__ dy, const float* __restrict__ w,
                                                                      float* __restrict__ dx) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);            // wave-uniform
  if (i >= (int64_t)B * T) return;
  const int t = (int)(i % T);
  float s = 0.f;
  for (int j = 0; j < MI_TAPS; ++j) {
    const int lo = t + MI_PAD - j;
    if (lo < 0 || lo >= T) continue;
    const float* d = dy + (i + (MI_PAD - j)) * MI_C;
    s += d[lane] * w[lane * MI_TAPS + j] + d[lane + 64] * w[(lane + 64) * MI_TAPS + j];
  }
  s = wave_sum(s);
  if (lane == 0) dx[i] = s;
}

// -----------------------------------------------------------------------------------------------------------------------------
// spectral norm: W (O, K) = weight_orig viewed from dim 0, u (O), v (K).  Sums in double, block-wide in a fixed tree.
// -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double* sh) {          // all 256 threads call it; every thread gets the sum
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(256) void msd_sn_wtu_kernel(int O, int K, const float* __restrict__ W, const float* __restrict__ u, double* __restrict__ t) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  double s = 0.0;
  for (int o = 0; o < O; ++o) s += (double)W[(int64_t)o * K + k] * (double)u[o];
  t[k] = s;
}

__global__ __launch_bounds__(256) void msd_sn_normv_kernel(int K, double eps, const double* __restrict__ t, float* __restrict__ v) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) s += t[k] * t[k];
  const double nrm = fmax(sqrt(block_sum(s, sh)), eps);
  for (int k = threadIdx.x; k < K; k += 256) v[k] = (float)(t[k] / nrm);
}

__global__ __launch_bounds__(256) void msd_sn_wv_kernel(int K, const float* __restrict__ W, const float* __restrict__ v, double* __restrict__ sv) {
  __shared__ double sh[256];
  const int o = blockIdx.x;
  double s = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) s += (double)W[(int64_t)o * K + k] * (double)v[k];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) sv[o] = s;
}

__global__ __launch_bounds__(256) void msd_sn_sigma_kernel(int O, int iterate, double eps, const double* __restrict__ sv, float* __restrict__ u,
                                                           float* __restrict__ sigma) {
  __shared__ double sh[256];
  if (iterate) {
    double s = 0.0;
    for (int o = threadIdx.x; o < O; o += 256) s += sv[o] * sv[o];
    const double nrm = fmax(sqrt(block_sum(s, sh)), eps);
    for (int o = threadIdx.x; o < O; o += 256) u[o] = (float)(sv[o] / nrm);      // each thread reads back only what it wrote
  }
  double d = 0.0;
  for (int o = threadIdx.x; o < O; o += 256) d += (double)u[o] * sv[o];
  d = block_sum(d, sh);
  if (threadIdx.x == 0) sigma[0] = (float)d;
}

__global__ __launch_bounds__(256) void msd_sn_scale_kernel(int64_t n, const float* __restrict__ W, const float* __restrict__ sigma, float* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) w[i] = W[i] / sigma[0];
}

__global__ __launch_bounds__(256) void msd_sn_rowdot_kernel(int K, const float* __restrict__ dW, const float* __restrict__ W, double* __restrict__ rd) {
  __shared__ double sh[256];
  const int o = blockIdx.x;
  double s = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) s += (double)dW[(int64_t)o * K + k] * (double)W[(int64_t)o * K + k];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) rd[o] = s;
}

// grad_orig = dW / sigma - (sum(dW o W) / sigma^2) u v^T; every workgroup sums the O row products itself, in the same order
__global__ __launch_bounds__(256) void msd_sn_apply_kernel(int O, int K, const float* __restrict__ dW, const float* __restrict__ u,
                                                           const float* __restrict__ v, const float* __restrict__ sigma, const double* __restrict__ rd,
                                                           float* __restrict__ grad) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int o = threadIdx.x; o < O; o += 256) s += rd[o];
  const double sg = (double)sigma[0];
  const double coef = block_sum(s, sh) / (sg * sg);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)O * K) return;
  const int o = (int)(i / K), k = (int)(i - (int64_t)o * K);
  grad[i] = (float)((double)dW[i] / sg - coef * (double)u[o] * (double)v[k]);
}

inline bool msd_gshape_ok(int B, int L, int Cin, int Cout, int groups, int stride) {
  if (!(B >= 1 && L >= 1 && groups >= 1 && Cin >= 1 && Cout >= 1 && Cin % groups == 0 && Cout % groups == 0)) return false;
  const int cg = Cin / groups, og = Cout / groups;
  return cg % 4 == 0 && og % 4 == 0 && cg <= 64 && og <= 64 && (stride == 1 || stride == 2 || stride == 4) && (int64_t)B * L < (1ll << 31) / 4;
}

}  // namespace

extern "C" int s2svc_hifigan_msd_gconv_chunk(int Lo) {
  const int c = 32 * ((Lo + 255) / 256);
  return c > 256 ? c : 256;
}

extern "C" int s2svc_hifigan_msd_pool(int B, int T, const float* x, float* y, void* stream) {
  S2S_REQUIRE(B >= 1 && T >= 1 && (int64_t)B * (T + 2) < (1ll << 31), "hifigan_msd_pool: B, T >= 1, B * T < 2^31");
  S2S_REQUIRE(x && y, "hifigan_msd_pool: null pointer");
  const int To = T / 2 + 1;
  const int64_t n = (int64_t)B * To;
  hipLaunchKernelGGL(hifigan_msd_pool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, T, To, x, y);
  S2S_CHECK_LAUNCH("hifigan_msd_pool_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_msd_pool_bwd(int B, int T, const float* dy, float* dx, void* stream) {
  S2S_REQUIRE(B >= 1 && T >= 1 && (int64_t)B * (T + 2) < (1ll << 31), "hifigan_msd_pool_bwd: B, T >= 1, B * T < 2^31");
  S2S_REQUIRE(dy && dx, "hifigan_msd_pool_bwd: null pointer");
  const int64_t n = (int64_t)B * T;
  hipLaunchKernelGGL(hifigan_msd_pool_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, T, T / 2 + 1, dy, dx);
  S2S_CHECK_LAUNCH("hifigan_msd_pool_bwd_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_msd_input(int B, int T, const float* x, const float* w32, const float* bias, float slope, float* out, void* stream) {
  S2S_REQUIRE(B >= 1 && T >= 1 && (int64_t)B * T < (1ll << 31) / MI_C, "hifigan_msd_input: B, T >= 1, B * T * 128 < 2^31");
  S2S_REQUIRE(x && w32 && bias && out, "hifigan_msd_input: null pointer");
  const int64_t n = (int64_t)B * T * MI_C;
  hipLaunchKernelGGL(hifigan_msd_input_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, T, x, w32, bias, slope, out);
  S2S_CHECK_LAUNCH("hifigan_msd_input_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_msd_input_wgrad(int B, int T, const float* dy, const float* x, float* wpart, float* bpart, void* stream) {
  S2S_REQUIRE(B >= 1 && T >= 1 && (int64_t)B * T < (1ll << 31) / MI_C, "hifigan_msd_input_wgrad: B, T >= 1, B * T * 128 < 2^31");
  S2S_REQUIRE(dy && x && wpart && bpart, "hifigan_msd_input_wgrad: null pointer");
  const int64_t M = (int64_t)B * T;
  hipLaunchKernelGGL(hifigan_msd_input_wgrad_kernel, dim3((unsigned)((M + MI_CHUNK - 1) / MI_CHUNK)), dim3(256), 0, (hipStream_t)stream, B, T, dy, x,
                     wpart, bpart);
  S2S_CHECK_LAUNCH("hifigan_msd_input_wgrad_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_msd_input_dgrad(int B, int T, const float* dy, const float* w32, float* dx, void* stream) {
  S2S_REQUIRE(B >= 1 && T >= 1 && (int64_t)B * T < (1ll << 31) / MI_C, "hifigan_msd_input_dgrad: B, T >= 1, B * T * 128 < 2^31");
  S2S_REQUIRE(dy && w32 && dx, "hifigan_msd_input_dgrad: null pointer");
  const int64_t n = (int64_t)B * T;
  hipLaunchKernelGGL(hifigan_msd_input_dgrad_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, B, T, dy, w32, dx);
  S2S_CHECK_LAUNCH("hifigan_msd_input_dgrad_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_msd_gconv(int B, int L, int Cin, int Cout, int groups, int stride, const float* x, const float* w_op, const float* bias,
                                       float slope, float* out, void* stream) {
  S2S_REQUIRE(msd_gshape_ok(B, L, Cin, Cout, groups, stride), "hifigan_msd_gconv: stride 1, 2 or 4; channels per group multiples of 4, <= 64");
  S2S_REQUIRE(x && w_op && bias && out && hg_aligned16(x) && hg_aligned16(w_op), "hifigan_msd_gconv: null or unaligned pointer");
  MtArgs a = {};
  a.a = x; a.w = w_op; a.bias = bias; a.out = out;
  a.B = B; a.La = L; a.Lo = (L - 1) / stride + 1; a.groups = groups; a.Kag = Cin / groups; a.Kap = hg_pad32(a.Kag); a.Ng = Cout / groups;
  a.sa = stride; a.so = 1; a.stride = stride; a.dgrad = 0; a.slope = slope; a.act = 1;
  return mt_launch("hifigan_msd_gconv", a, (hipStream_t)stream);
}

extern "C" int s2svc_hifigan_msd_fold_bwd(int Cin, int Cout, int groups, const float* w32, float* w_opT, void* stream) {
  S2S_REQUIRE(groups >= 1 && Cin >= 1 && Cout >= 1 && Cin % groups == 0 && Cout % groups == 0, "hifigan_msd_fold_bwd: channels divisible by the groups");
  S2S_REQUIRE(w32 && w_opT, "hifigan_msd_fold_bwd: null pointer");
  const int Og = Cout / groups;
  hipLaunchKernelGGL(hifigan_msd_fold_bwd_kernel, dim3(Cin), dim3(256), 0, (hipStream_t)stream, Og, Cin / groups, hg_pad32(Og), w32, w_opT);
  S2S_CHECK_LAUNCH("hifigan_msd_fold_bwd_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_msd_gconv_dgrad(int B, int L, int Cin, int Cout, int groups, int stride, const float* dy, const float* w_opT,
                                             const float* mask_src, const float* add, float slope, float* dx, void* stream) {
  S2S_REQUIRE(msd_gshape_ok(B, L, Cin, Cout, groups, stride), "hifigan_msd_gconv_dgrad: stride 1, 2 or 4; channels per group multiples of 4, <= 64");
  S2S_REQUIRE(dy && w_opT && dx && hg_aligned16(dy) && hg_aligned16(w_opT), "hifigan_msd_gconv_dgrad: null or unaligned pointer");
  MtArgs a = {};
  a.a = dy; a.w = w_opT; a.mask = mask_src; a.add = add; a.out = dx;
  a.B = B; a.La = (L - 1) / stride + 1; a.Lo = L; a.groups = groups; a.Kag = Cout / groups; a.Kap = hg_pad32(a.Kag); a.Ng = Cin / groups;
  a.sa = 1; a.so = stride; a.stride = stride; a.dgrad = 1; a.slope = slope; a.act = 0;
  return mt_launch("hifigan_msd_gconv_dgrad", a, (hipStream_t)stream);
}

extern "C" int s2svc_hifigan_msd_gconv_wgrad(int B, int L, int Cin, int Cout, int groups, int stride, int chunk, const float* dy, const float* x,
                                             float* wpart, float* bpart, void* stream) {
  S2S_REQUIRE(msd_gshape_ok(B, L, Cin, Cout, groups, stride), "hifigan_msd_gconv_wgrad: stride 1, 2 or 4; channels per group multiples of 4, <= 64");
  S2S_REQUIRE(dy && x && wpart && bpart && hg_aligned16(dy) && hg_aligned16(x), "hifigan_msd_gconv_wgrad: null or unaligned pointer");
  MwArgs a = {};
  a.dy = dy; a.x = x; a.wpart = wpart; a.bpart = bpart;
  a.B = B; a.L = L; a.Lo = (L - 1) / stride + 1; a.Cin = Cin; a.Cout = Cout; a.groups = groups; a.Cg = Cin / groups; a.Mg = Cout / groups;
  a.stride = stride; a.chunk = chunk;
  S2S_REQUIRE(chunk == s2svc_hifigan_msd_gconv_chunk(a.Lo), "hifigan_msd_gconv_wgrad: chunk is s2svc_hifigan_msd_gconv_chunk(output rows)");
  a.ncpu = (a.Lo + chunk - 1) / chunk;
  a.mtiles = (a.Mg + 31) / 32; a.ctiles = (a.Cg + 31) / 32;
  const int64_t gy = (int64_t)groups * a.mtiles * a.ctiles;
  S2S_REQUIRE(gy <= 65535 && (int64_t)B * a.ncpu < (1ll << 31), "hifigan_msd_gconv_wgrad: grid too large");
  const dim3 grid((unsigned)(B * a.ncpu), (unsigned)gy, (MT_TAPS + MW_TG - 1) / MW_TG), block(256);
  hipLaunchKernelGGL(hifigan_msd_wgrad_kernel, grid, block, 0, (hipStream_t)stream, a);
  S2S_CHECK_LAUNCH("hifigan_msd_wgrad_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_msd_sn_power(int O, int K, int iterate, float eps, const float* W, float* u, float* v, float* sigma, double* ws,
                                          void* stream) {
  S2S_REQUIRE(O >= 1 && K >= 1 && (int64_t)O * K < (1ll << 31), "hifigan_msd_sn_power: bad shape");
  S2S_REQUIRE(W && u && v && sigma && ws, "hifigan_msd_sn_power: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (iterate) {
    hipLaunchKernelGGL(msd_sn_wtu_kernel, dim3((K + 255) / 256), dim3(256), 0, st, O, K, W, u, ws);
    S2S_CHECK_LAUNCH("msd_sn_wtu_kernel");
    hipLaunchKernelGGL(msd_sn_normv_kernel, dim3(1), dim3(256), 0, st, K, (double)eps, ws, v);
    S2S_CHECK_LAUNCH("msd_sn_normv_kernel");
  }
  hipLaunchKernelGGL(msd_sn_wv_kernel, dim3(O), dim3(256), 0, st, K, W, v, ws + K);
  S2S_CHECK_LAUNCH("msd_sn_wv_kernel");
  hipLaunchKernelGGL(msd_sn_sigma_kernel, dim3(1), dim3(256), 0, st, O, iterate, (double)eps, ws + K, u, sigma);
  S2S_CHECK_LAUNCH("msd_sn_sigma_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_msd_sn_scale(int64_t n, const float* W, const float* sigma, float* w, void* stream) {
  S2S_REQUIRE(n >= 1 && n < (1ll << 31) && W && sigma && w, "hifigan_msd_sn_scale: bad size or null pointer");
  hipLaunchKernelGGL(msd_sn_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, W, sigma, w);
  S2S_CHECK_LAUNCH("msd_sn_scale_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_msd_sn_finish(int O, int K, const float* dW, const float* W, const float* u, const float* v, const float* sigma,
                                           float* grad, double* ws, void* stream) {
  S2S_REQUIRE(O >= 1 && K >= 1 && (int64_t)O * K < (1ll << 31), "hifigan_msd_sn_finish: bad shape");
  S2S_REQUIRE(dW && W && u && v && sigma && grad && ws, "hifigan_msd_sn_finish: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(msd_sn_rowdot_kernel, dim3(O), dim3(256), 0, st, K, dW, W, ws);
  S2S_CHECK_LAUNCH("msd_sn_rowdot_kernel");
  const int64_t n = (int64_t)O * K;
  hipLaunchKernelGGL(msd_sn_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, O, K, dW, u, v, sigma, ws, grad);
  S2S_CHECK_LAUNCH("msd_sn_apply_kernel");
  return 0;
}
