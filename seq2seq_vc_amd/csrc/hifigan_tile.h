// The implicit-GEMM tile of the HiFi-GAN convolutions: ONE body for the forward (hifigan.hip, hifigan_gemm_kernel) and the data
// gradient (hifigan_bwd.hip, hifigan_dgrad_kernel), and the tap geometry that both and the weight gradient are launched with.
//
// Tile: 128 rows x BN columns per workgroup of 4 wavefronts (32 rows x BN columns each), 32 reduction columns per step.  The A
// tile is staged once per step WITH its halo (<= 50 rows: k = 11, dil = 5) and every tap reads it from LDS at a row offset, so an
// element of A is fetched (and passed through whatever its loader applies) once for all taps; the weight operand of up to 4 taps is
// staged beside it.  LDS rows are padded by 16 bytes.  A kernel decodes its arguments and supplies two functors:
//   loadA(r, c)  the 16-byte vector of A at halo row r (the tile's row i0 + r + offmin) and reduction column c, zero where absent
//   epi(n)       called once per column n < N of the lane; returns store(i, acc), called for every row i < rows the lane holds
#pragma once
#include "gemm_common.h"

namespace {

constexpr int HG_BM = 128, HG_KC = 32, HG_TG = 4, HG_MAXSPAN = 50;

template <typename T> struct HgFrag;
template <> struct HgFrag<bf16_t> {
  static constexpr int VEC = 8, KSTEP = 32;      // one v_mfma_f32_16x16x32_bf16 per step
  typedef bf16x8_t type;
  static __device__ __forceinline__ f32x4_t mma(type a, type b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct HgFrag<float> {
  static constexpr int VEC = 4, KSTEP = 16;      // four v_mfma_f32_16x16x4_f32 per step (lane element e <-> k = 4 * (lane >> 4) + e)
  typedef f32x4_t type;
  static __device__ __forceinline__ f32x4_t mma(type a, type b, f32x4_t c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], c, 0, 0, 0);
    return c;
  }
};

__device__ __forceinline__ float hg_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

inline int hg_pad32(int c) { return (c + HG_KC - 1) / HG_KC * HG_KC; }
inline bool hg_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// Tap j of row i pairs it with row i + j * tstep + toff0 of A; offmin = the smallest such offset, span = the largest - the smallest.
// rows = GEMM rows per utterance, tiles = row tiles per utterance, pad = the transposed convolution's padding (k - u) / 2.
struct HgGeom {
  int ntaps, tstep, toff0, offmin, span, rows, tiles, pad;
};

inline int hg_fail(const char* who, const char* msg) {           // "<entry point>: <msg>", as S2S_REQUIRE reports
  s2svc_set_error(who);
  s2svc_set_error(msg);
  return -1;
}

inline int hg_geom_tiles(const char* who, int B, HgGeom& g) {
  g.tiles = (g.rows + HG_BM - 1) / HG_BM;
  return (int64_t)B * g.tiles < (1ll << 31) ? 0 : hg_fail(who, "too many row tiles");
}

// Conv1d(k, dilation dil, padding (k - 1) / 2 * dil) over T frames: tap j reads frame i + (j - (k - 1) / 2) * dil.
inline int hg_conv1d_geom(const char* who, int B, int T, int k, int dil, HgGeom& g) {
  if (!(k >= 1 && k <= 11 && (k & 1) && dil >= 1 && dil <= 5)) return hg_fail(who, "k odd <= 11, dil 1..5");
  g.ntaps = k; g.tstep = dil; g.toff0 = g.offmin = -((k - 1) / 2) * dil; g.span = (k - 1) * dil; g.rows = T; g.pad = 0;
  return hg_geom_tiles(who, B, g);
}

// ConvTranspose1d(k, stride u, padding (k - u) / 2) over T input frames as a GEMM with columns (phase, channel) and ceil(k / u) taps.
// Forward direction (the forward, the weight gradient): row i reads input frames i, i - 1, ..; ceil(pad / u) rows past T hold the
// tail taps of the last frames.  Transposed (the data gradient): row i of T reads rows i, i + 1, .. of the forward's own GEMM view.
inline int hg_tconv1d_geom(const char* who, int B, int T, int k, int u, bool transposed, HgGeom& g) {
  if (!(u >= 1 && k >= u && ((k - u) & 1) == 0)) return hg_fail(who, "k >= u and (k - u) even (padding (k - u) / 2 gives T_out = u T_in)");
  g.ntaps = (k + u - 1) / u; g.pad = (k - u) / 2; g.span = g.ntaps - 1; g.toff0 = 0;
  if (g.span > HG_MAXSPAN) return hg_fail(who, "more than 51 taps per phase");
  if ((int64_t)T * u >= (1ll << 31) / 512) return hg_fail(who, "output too long");
  g.tstep = transposed ? 1 : -1; g.offmin = transposed ? 0 : -g.span; g.rows = transposed ? T : T + (g.pad + u - 1) / u;
  return hg_geom_tiles(who, B, g);
}

template <typename T, int BN, typename LoadA, typename Epi>
__device__ __forceinline__ void hg_tile(const HgGeom& g, const T* W, int Kap, int N, int i0, int n0, LoadA loadA, Epi epi) {
  typedef HgFrag<T> F;
  typedef typename F::type frag_t;
  constexpr int VEC = F::VEC;
  constexpr int VPR = HG_KC / VEC;                       // 16-byte vectors per LDS row
  constexpr int ROWB = HG_KC * (int)sizeof(T) + 16;      // LDS row in bytes, padded
  constexpr int NT = BN / 16;
  constexpr int KS = HG_KC / F::KSTEP;
  __shared__ __attribute__((aligned(16))) unsigned char sA[(HG_BM + HG_MAXSPAN) * ROWB];
  __shared__ __attribute__((aligned(16))) unsigned char sB[HG_TG * BN * ROWB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int Kp = g.ntaps * Kap;                          // W is [N][ntaps * Kap], reduction index tap * Kap + column
  const int R = HG_BM + g.span;

  f32x4_t acc[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < Kap; c0 += HG_KC) {
    __syncthreads();                                     // the previous step's fragments have been read
    for (int idx = tid; idx < R * VPR; idx += 256) {
      const int r = idx / VPR, v = idx - r * VPR;
      *reinterpret_cast<uint4*>(sA + r * ROWB + v * 16) = loadA(r, c0 + v * VEC);
    }
    for (int tg = 0; tg < g.ntaps; tg += HG_TG) {
      const int gn = min(HG_TG, g.ntaps - tg);
      if (tg > 0) __syncthreads();
      for (int idx = tid; idx < gn * BN * VPR; idx += 256) {
        const int tapi = idx / (BN * VPR), rem = idx - tapi * (BN * VPR);
        const int nn = rem / VPR, v = rem - nn * VPR;
        uint4 val = make_uint4(0u, 0u, 0u, 0u);
        if (n0 + nn < N) val = *reinterpret_cast<const uint4*>(W + (int64_t)(n0 + nn) * Kp + (tg + tapi) * Kap + c0 + v * VEC);
        *reinterpret_cast<uint4*>(sB + (tapi * BN + nn) * ROWB + v * 16) = val;
      }
      __syncthreads();
      for (int tapi = 0; tapi < gn; ++tapi) {
        const int arow = wave * 32 + lr + (tg + tapi) * g.tstep + g.toff0 - g.offmin;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int koff = ks * 64 + lg * 16;
          frag_t fa[2], fb[NT];
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) fa[mt] = *reinterpret_cast<const frag_t*>(sA + (arow + mt * 16) * ROWB + koff);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) fb[nt] = *reinterpret_cast<const frag_t*>(sB + (tapi * BN + nt * 16 + lr) * ROWB + koff);
#pragma unroll
          for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = F::mma(fa[mt], fb[nt], acc[mt][nt]);
        }
      }
    }
  }

#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = n0 + nt * 16 + lr;
    if (n >= N) continue;
    const auto store = epi(n);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wave * 32 + mt * 16 + lg * 4 + r;
        if (i < g.rows) store(i, acc[mt][nt][r]);
      }
  }
}

// The dtype x BN dispatch of a tile kernel.  K: `name` and the variable template `fn<T, BN>` = the __global__ function.
template <typename K, typename Args>
int hg_launch(int dtype, const Args& a, hipStream_t st) {
  const int bn = a.N > 32 ? 64 : (a.N > 16 ? 32 : 16);
  const dim3 grid(a.B * a.g.tiles, (a.N + bn - 1) / bn), block(256);
  void (*fn)(const Args);
  if (dtype == S2S_F32) fn = bn == 64 ? K::template fn<float, 64> : (bn == 32 ? K::template fn<float, 32> : K::template fn<float, 16>);
  else fn = bn == 64 ? K::template fn<bf16_t, 64> : (bn == 32 ? K::template fn<bf16_t, 32> : K::template fn<bf16_t, 16>);
  hipLaunchKernelGGL(fn, grid, block, 0, st, a);
  S2S_CHECK_LAUNCH(K::name);
  return 0;
}

}  // namespace
