// Attention forward that never writes the (B, H, T1, T2) map: online softmax over key tiles (inference; no dropout, no backward).
// replaces, for the HuBERT-Soft content encoder (urhythmic/hubert.py), torch.nn.MultiheadAttention's scaled-dot-product core.
//
// One workgroup = 4 wavefronts = 64 query rows of one (utterance, head); a wavefront owns 16 query rows and walks the keys in tiles
// of 64.  dk = 64.
//   Q    in registers for the whole key loop, as the B operand of the score product.
//   K, V register-staged into LDS (the next tile's global loads are issued before the current tile's arithmetic); K by rows, V
//        TRANSPOSED ([d][key]), both with rows padded by 16 bytes.
//   S^T  = K . Q^T ("swapped"): lane (g = lane >> 4, q = lane & 15) holds the 16 scores of query q with keys 16 j + 4 g + r of the
//        tile, so every lane carries scores, the row maximum is 15 in-lane fmax + partners 16 and 32, and the probabilities ARE the
//        B operand of O^T = V^T . P with no cross-lane move: bf16 packs the blocks j = 2 s, 2 s + 1 into one 32-key step, fp32 uses
//        block j as one 16-key step.
//   O^T  accumulates in 16 registers per lane for the same query q, so the running-maximum rescale is in-lane as well.
// The rescale is applied at every tile (no deferred threshold).  The key loop is bounded by min(klen[b], T2) and keys at or beyond
// it inside the last tile are staged as zeros, so nothing beyond a row's length is read into the arithmetic and the result of one
// (utterance, head, query tile) depends neither on B nor on the padded length.
#include "common.h"
#include "../../include/s2svc_hip.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 fa_bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float fa_f32x4_t;

constexpr int FA_DK = 64, FA_KT = 64, FA_QB = 64;

template <typename T> struct FaFrag;
template <> struct FaFrag<bf16_t> {
  static constexpr int VEC = 8;                    // elements per 16-byte vector; one v_mfma_f32_16x16x32_bf16 contracts 32
  typedef fa_bf16x8_t type;
  static __device__ __forceinline__ fa_f32x4_t mma(type a, type b, fa_f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct FaFrag<float> {
  static constexpr int VEC = 4;                    // four v_mfma_f32_16x16x4_f32 contract 16 (lane element e <-> k = 4 * (lane >> 4) + e)
  typedef fa_f32x4_t type;
  static __device__ __forceinline__ fa_f32x4_t mma(type a, type b, fa_f32x4_t c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], c, 0, 0, 0);
    return c;
  }
};

__device__ __forceinline__ float fa_max4(float v) {          // over the four lanes that share lane & 15
  lane_pair p = swap16(v);
  v = fmaxf(p.a, p.b);
  p = swap32(v);
  return fmaxf(p.a, p.b);
}

template <typename T>
__global__ __launch_bounds__(256) void attn_flash_kernel(int T1, int T2, const T* __restrict__ q, int64_t qbs, int64_t ldq,
                                                         const T* __restrict__ k, int64_t kbs, int64_t ldk, const T* __restrict__ v,
                                                         int64_t vbs, int64_t ldv, const int32_t* __restrict__ klen, float scale_log2,
                                                         T* __restrict__ ctx, int64_t obs, int64_t ldo) {
  typedef FaFrag<T> F;
  typedef typename F::type frag_t;
  constexpr int VEC = F::VEC;
  constexpr int VPR = FA_DK / VEC;                          // 16-byte vectors per K / V row
  constexpr int NV = FA_KT * VPR / 256;                     // vectors of each of K and V a thread stages per tile
  constexpr int NKS = FA_DK * (int)sizeof(T) / 64;          // score-product steps (64 bytes of d each)
  constexpr int KROWB = FA_DK * (int)sizeof(T) + 16;        // LDS row of K: 64 d + pad
  constexpr int VROWB = FA_KT * (int)sizeof(T) + 16;        // LDS row of V^T: 64 keys + pad
  __shared__ __attribute__((aligned(16))) unsigned char sK[FA_KT * KROWB];
  __shared__ __attribute__((aligned(16))) unsigned char sV[FA_DK * VROWB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, t = blockIdx.x * FA_QB + wave * 16 + lr;
  const int kl = klen ? klen[b] : T2;
  const int nk = kl < T2 ? kl : T2;
  T* const orow = ctx + b * obs + (int64_t)t * ldo + h * FA_DK;

  if (nk <= 0) {                                            // an utterance without keys: +0
    if (t < T1) {
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) stf(orow + db * 16 + lg * 4 + r, 0.f);
    }
    return;
  }

  frag_t qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (t < T1) w = *reinterpret_cast<const uint4*>(q + b * qbs + (int64_t)t * ldq + h * FA_DK + ks * (64 / (int)sizeof(T)) + lg * VEC);
    qf[ks] = __builtin_bit_cast(frag_t, w);
  }

  const T* const kb = k + b * kbs + h * FA_DK;
  const T* const vb = v + b * vbs + h * FA_DK;
  uint4 kr[NV], vr[NV];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256, row = idx / VPR, vv = idx - row * VPR;
      kr[i] = vr[i] = make_uint4(0u, 0u, 0u, 0u);
      if (k0 + row < nk) {
        kr[i] = *reinterpret_cast<const uint4*>(kb + (int64_t)(k0 + row) * ldk + vv * VEC);
        vr[i] = *reinterpret_cast<const uint4*>(vb + (int64_t)(k0 + row) * ldv + vv * VEC);
      }
    }
  };

  fa_f32x4_t o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) o[db] = (fa_f32x4_t){0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;                             // running maximum (log2 domain) of query t; this lane's share of its sum

  fetch(0);
  for (int k0 = 0; k0 < nk; k0 += FA_KT) {
    __syncthreads();                                        // the previous tile's fragments have been read
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256, row = idx / VPR, vv = idx - row * VPR;
      *reinterpret_cast<uint4*>(sK + row * KROWB + vv * 16) = kr[i];
      const T* e = reinterpret_cast<const T*>(&vr[i]);
#pragma unroll
      for (int c = 0; c < VEC; ++c) *reinterpret_cast<T*>(sV + (vv * VEC + c) * VROWB + row * (int)sizeof(T)) = e[c];
    }
    __syncthreads();
    if (k0 + FA_KT < nk) fetch(k0 + FA_KT);

    // scores of query t with the tile's keys 16 j + 4 lg + r
    fa_f32x4_t s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = (fa_f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const frag_t a = *reinterpret_cast<const frag_t*>(sK + (j * 16 + lr) * KROWB + ks * 64 + lg * 16);
        s[j] = F::mma(a, qf[ks], s[j]);
      }
    }
    float mt = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sv = k0 + j * 16 + lg * 4 + r < nk ? s[j][r] * scale_log2 : -INFINITY;
        s[j][r] = sv;
        mt = fmaxf(mt, sv);
      }
    mt = fa_max4(mt);                                       // finite: the tile's first key is below nk
    const float mn = fmaxf(m, mt);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);     // 0 at the first tile (m = -inf)
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(s[j][r] - mn);
        s[j][r] = p;
        ps += p;
      }
    l = __builtin_fmaf(l, alpha, ps);
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[db][r] *= alpha;

    // O^T += V^T . P
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        uint4 pw;
        pw.x = f2bf2(s[2 * st][0], s[2 * st][1]);
        pw.y = f2bf2(s[2 * st][2], s[2 * st][3]);
        pw.z = f2bf2(s[2 * st + 1][0], s[2 * st + 1][1]);
        pw.w = f2bf2(s[2 * st + 1][2], s[2 * st + 1][3]);
        const frag_t pb = __builtin_bit_cast(frag_t, pw);
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          const unsigned char* vrow = sV + (db * 16 + lr) * VROWB + (st * 32 + lg * 4) * 2;
          const uint2 lo = *reinterpret_cast<const uint2*>(vrow), hi = *reinterpret_cast<const uint2*>(vrow + 32);
          const frag_t a = __builtin_bit_cast(frag_t, make_uint4(lo.x, lo.y, hi.x, hi.y));
          o[db] = F::mma(a, pb, o[db]);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          const frag_t a = *reinterpret_cast<const frag_t*>(sV + (db * 16 + lr) * VROWB + (j * 16 + lg * 4) * 4);
          o[db] = F::mma(a, __builtin_bit_cast(frag_t, s[j]), o[db]);
        }
    }
  }

  l = xor32_sum(xor16_sum(l));
  if (t >= T1) return;
  const bool absent = klen && t >= kl;                      // a query row beyond the utterance: +0
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    float f[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) f[r] = absent ? 0.f : o[db][r] / l;
    T* p = orow + db * 16 + lg * 4;
    if constexpr (sizeof(T) == 2) *reinterpret_cast<uint2*>(p) = make_uint2(f2bf2(f[0], f[1]), f2bf2(f[2], f[3]));
    else *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  }
}

inline bool fa_ld_ok(int dtype, int64_t ld) { return ld >= FA_DK && ld % (dtype == S2S_F32 ? 4 : 8) == 0; }

}  // namespace

extern "C" int s2svc_attn_flash_supported(int dtype, int dk, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo) {
  return (dtype == S2S_F32 || dtype == S2S_BF16) && dk == FA_DK && fa_ld_ok(dtype, ldq) && fa_ld_ok(dtype, ldk) && fa_ld_ok(dtype, ldv) &&
                 fa_ld_ok(dtype, ldo)
             ? 1
             : 0;
}

extern "C" int s2svc_attn_flash_fwd(int dtype, int B, int H, int T1, int T2, int dk, const void* q, int64_t qbs, int64_t ldq, const void* k,
                                    int64_t kbs, int64_t ldk, const void* v, int64_t vbs, int64_t ldv, const int32_t* klen, float scale,
                                    void* ctx, int64_t obs, int64_t ldo, void* stream) {
  S2S_REQUIRE(s2svc_attn_flash_supported(dtype, dk, ldq, ldk, ldv, ldo), "attn_flash_fwd: fp32 or bf16, dk = 64, row strides of whole 16-byte vectors");
  S2S_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && H <= 65535 && T1 >= 1 && T2 >= 1, "attn_flash_fwd: 1 <= B, H <= 65535 and T1, T2 >= 1");
  const int vec = dtype == S2S_F32 ? 4 : 8;
  S2S_REQUIRE(qbs % vec == 0 && kbs % vec == 0 && vbs % vec == 0 && obs % vec == 0 && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(ctx),
              "attn_flash_fwd: 16-byte aligned views expected");
  S2S_REQUIRE((int64_t)H * FA_DK <= ldq && (int64_t)H * FA_DK <= ldk && (int64_t)H * FA_DK <= ldv && (int64_t)H * FA_DK <= ldo,
              "attn_flash_fwd: a row holds at least H * dk elements");
  const dim3 grid((T1 + FA_QB - 1) / FA_QB, H, B);
  const float sl2 = scale * 1.44269504088896340736f;
  if (dtype == S2S_F32)
    hipLaunchKernelGGL(attn_flash_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, T1, T2, (const float*)q, qbs, ldq, (const float*)k, kbs,
                       ldk, (const float*)v, vbs, ldv, klen, sl2, (float*)ctx, obs, ldo);
  else
    hipLaunchKernelGGL(attn_flash_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, T1, T2, (const bf16_t*)q, qbs, ldq, (const bf16_t*)k,
                       kbs, ldk, (const bf16_t*)v, vbs, ldv, klen, sl2, (bf16_t*)ctx, obs, ldo);
  S2S_CHECK_LAUNCH("attn_flash_fwd");
  return 0;
}
