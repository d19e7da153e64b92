// HiFi-GAN generator, backward with respect to the PARAMETERS (fine-tuning; reference: urhythmic_fine_tune_vocoder.py:191-222 calls
// loss_generator.backward() through seq2seq_vc/urhythmic/vocoder.py:23-202).  The forward is csrc/hifigan.hip, unchanged; the stored
// activations are the raw pre-activations (channel-last), leaky_relu is applied as they are staged.
//
//   data gradient     hifigan_dgrad_kernel: the forward's implicit-GEMM tile (csrc/hifigan_tile.h, the same body) over a flipped /
//                     transposed operand (hifigan_fold_bwd_kernel); this file supplies the A loader (a flat view with bounds) and
//                     the epilogue out = [out +] scale * (lrelu'(mask_src) * acc [+ res]).  The transposed convolution's data gradient
//                     is the same kernel on the forward's own GEMM view of dy: (rows, u * C_out) at a flat offset of -pad * C_out.
//   weight gradient   hifigan_wgrad_kernel: dw[m][tap][c] = sum over frames of dy[i][m] * lrelu(x)[i + off(tap)][c], both operands
//                     reduced over their slow axis.  A workgroup owns a 32 x 32 x taps block of the result and ONE chunk of frames
//                     (chunk edges depend on the shapes only); it writes an fp32 partial, and the column sums of dy (the bias
//                     gradient) ride along.  No atomics.
//   finish            hifigan_wgrad_finish_kernel: partials summed in ascending chunk order, laid out in the parameter's shape,
//                     weight-norm backward, bias.
//   conv_post         hifigan_conv_out_bwd_kernel: tanh derivative, the C -> 1 data gradient with its mask, weight / bias partials.
//
// Every sum runs in one order that depends on the shapes only: two passes over the same inputs give the same bits.
#include "hifigan_tile.h"

namespace {

constexpr int HW_TS = 32, HW_MAXTAPS = 12, HW_ITEMS = 6;      // wgrad: frames per step; (tap, 16-row half) items per wavefront
constexpr int HO_CHUNK = 256, HO_MAXK = 11;                   // conv_post backward: frames per workgroup

template <typename T> __device__ __forceinline__ uint4 hb_pack(const float (&f)[8]);
template <> __device__ __forceinline__ uint4 hb_pack<float>(const float (&f)[8]) {
  return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
}
template <> __device__ __forceinline__ uint4 hb_pack<bf16_t>(const float (&f)[8]) { return pack_bf16x8(f); }

// One 16-byte vector of a (rows, cols) view of a flat tensor of L elements: element `col + e` of the vector lives at flat index
// flat + e and counts as zero where that index lies outside [0, L) or col + e >= cols.  vec: the whole view is 16-byte granular.
template <typename T>
__device__ __forceinline__ uint4 hb_load_view(const T* base, int64_t flat, int64_t L, int col, int cols, bool vec, float slope) {
  constexpr int VEC = 16 / (int)sizeof(T);
  float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (vec && flat >= 0 && flat + VEC <= L && col + VEC <= cols) {
    const uint4 v = *reinterpret_cast<const uint4*>(base + flat);
    if (slope == 0.f) return v;
    if (sizeof(T) == 4) { f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w); }
    else unpack_bf16x8(v, f);
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      if (col + e < cols && flat + e >= 0 && flat + e < L) f[e] = ldf(base + flat + e);
  }
  if (slope != 0.f) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) f[e] = hg_lrelu(f[e], slope);
  }
  return hb_pack<T>(f);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// data gradient
// ---------------------------------------------------------------------------------------------------------------------------------
struct HbArgs {
  const void* a;         // the gradient: per utterance a flat tensor of La elements, viewed as rows of Ka columns at offset -aoff
  const void* w;         // [N][ntaps * Kap], reduction index tap * Kap + column (hifigan_fold_bwd)
  const void* mask;      // (B, rows, N) or NULL: the forward's raw input of the layer
  const void* res;       // (B, rows, N) or NULL
  void* out;             // (B, rows, N)
  int64_t La;
  HgGeom g;              // tap j reads view row i + j * tstep + toff0
  int B, Ka, Kap, aoff, N;
  float slope, scale;
  int accumulate, vec_ok;
};

template <typename T, int BN>
__global__ __launch_bounds__(256) void hifigan_dgrad_kernel(const HbArgs a) {
  const int b = blockIdx.x / a.g.tiles;
  const int i0 = (blockIdx.x - b * a.g.tiles) * HG_BM;
  const T* ab = (const T*)a.a + (int64_t)b * a.La;
  const int64_t ob = (int64_t)b * a.g.rows * a.N;
  T* outb = (T*)a.out + ob;
  const T* maskb = a.mask ? (const T*)a.mask + ob : nullptr;
  const T* resb = a.res ? (const T*)a.res + ob : nullptr;
  hg_tile<T, BN>(
      a.g, (const T*)a.w, a.Kap, a.N, i0, blockIdx.y * BN,
      [&](int r, int c) {
        if (c >= a.Ka) return make_uint4(0u, 0u, 0u, 0u);
        return hb_load_view<T>(ab, (int64_t)(i0 + r + a.g.offmin) * a.Ka + c - a.aoff, a.La, c, a.Ka, a.vec_ok != 0, 0.f);
      },
      // epilogue: out = [out +] scale * (lrelu'(mask) * acc [+ res]) in fp32, one rounding at the store
      [&](int n) {
        return [&, n](int i, float v) {
          const int64_t at = (int64_t)i * a.N + n;
          if (maskb) v = ldf(maskb + at) > 0.f ? v : v * a.slope;
          if (resb) v += ldf(resb + at);
          v *= a.scale;
          if (a.accumulate) v += ldf(outb + at);
          stf(outb + at, v);
        };
      });
}

struct HbDgrad {
  static constexpr const char* name = "hifigan_dgrad_kernel";
  template <typename T, int BN> static constexpr auto fn = hifigan_dgrad_kernel<T, BN>;
};

// ---------------------------------------------------------------------------------------------------------------------------------
// weight and bias gradients: partials per chunk of frames
// ---------------------------------------------------------------------------------------------------------------------------------
struct HwArgs {
  const void* dy;        // per utterance a flat tensor of Ldy elements, viewed as rows of Na columns at offset -aoff
  const void* x;         // (B, Tin, Cin): the layer's raw input
  float* wpart;          // [B * ncpu][Na][ntaps][Cin]
  float* bpart;          // [B * ncpu][Na]
  int64_t Ldy;
  int B, Na, aoff, Tin, Cin, ntaps;
  int tstep, toff0, offmin, span;    // tap j pairs view row i with input frame i + j * tstep + toff0 (HgGeom's fields)
  int rows, chunk, ncpu, ctiles;
  float slope;
  int vec_dy, vec_x;
};

template <typename T> struct HwLds;
template <> struct HwLds<float> {
  static constexpr int ROW = 36;                           // floats per LDS row: lanes (lg, lr) of a scalar read hit 64 banks
  static __device__ __forceinline__ f32x4_t frag(const float* s, int row0, int col, int ks, int lg) {
    f32x4_t f;
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = s[(row0 + ks * 16 + 4 * lg + e) * ROW + col];
    return f;
  }
};
template <> struct HwLds<bf16_t> {
  static constexpr int ROW = 40;
  static __device__ __forceinline__ bf16x8_t frag(const bf16_t* s, int row0, int col, int ks, int lg) {
    typedef __attribute__((ext_vector_type(8))) unsigned short u16x8_t;
    u16x8_t f;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = s[(row0 + 8 * lg + e) * ROW + col];
    return __builtin_bit_cast(bf16x8_t, f);
  }
};

template <typename T>
__global__ __launch_bounds__(256) void hifigan_wgrad_kernel(const HwArgs a) {
  typedef HgFrag<T> F;
  typedef typename F::type frag_t;
  typedef HwLds<T> L;
  constexpr int VEC = F::VEC;
  constexpr int VPR = HG_KC / VEC;
  constexpr int KS = HW_TS / F::KSTEP;
  __shared__ __attribute__((aligned(16))) T sD[HW_TS * L::ROW];
  __shared__ __attribute__((aligned(16))) T sX[(HW_TS + HG_MAXSPAN) * L::ROW];
  __shared__ float sBias[8][32];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int b = blockIdx.x / a.ncpu, ch = blockIdx.x - b * a.ncpu;
  const int mt = blockIdx.y / a.ctiles, ct = blockIdx.y - mt * a.ctiles;
  const int m0 = mt * 32, c0 = ct * 32;
  const int r0 = ch * a.chunk, r1 = min(r0 + a.chunk, a.rows);
  const T* dyb = (const T*)a.dy + (int64_t)b * a.Ldy;
  const T* xb = (const T*)a.x + (int64_t)b * a.Tin * a.Cin;
  const int64_t Lx = (int64_t)a.Tin * a.Cin;
  const int nitems = 2 * a.ntaps;

  f32x4_t acc[HW_ITEMS][2];
#pragma unroll
  for (int q = 0; q < HW_ITEMS; ++q)
#pragma unroll
    for (int ci = 0; ci < 2; ++ci) acc[q][ci] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  const int RX = HW_TS + a.span;

  for (int tk = r0; tk < r1; tk += HW_TS) {
    __syncthreads();
    for (int idx = tid; idx < HW_TS * VPR; idx += 256) {
      const int r = idx / VPR, v = idx - r * VPR;
      const int i = tk + r, m = m0 + v * VEC;
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (i < r1 && m < a.Na) val = hb_load_view<T>(dyb, (int64_t)i * a.Na + m - a.aoff, a.Ldy, m, a.Na, a.vec_dy != 0, 0.f);
      *reinterpret_cast<uint4*>(sD + r * L::ROW + v * VEC) = val;
    }
    for (int idx = tid; idx < RX * VPR; idx += 256) {
      const int r = idx / VPR, v = idx - r * VPR;
      const int t = tk + r + a.offmin, c = c0 + v * VEC;
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (t >= 0 && t < a.Tin && c < a.Cin) val = hb_load_view<T>(xb, (int64_t)t * a.Cin + c, Lx, c, a.Cin, a.vec_x != 0, a.slope);
      *reinterpret_cast<uint4*>(sX + r * L::ROW + v * VEC) = val;
    }
    __syncthreads();
    if (ct == 0) {
      const int col = tid & 31;
      for (int r = tid >> 5; r < HW_TS; r += 8) bsum += ldf(sD + r * L::ROW + col);
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int q = 0; q < HW_ITEMS; ++q) {
        const int item = wave + 4 * q;
        if (item < nitems) {
          const int j = item >> 1, mi = item & 1;
          const int off = j * a.tstep + a.toff0 - a.offmin;
          const frag_t fa = L::frag(sD, 0, mi * 16 + lr, ks, lg);
#pragma unroll
          for (int ci = 0; ci < 2; ++ci) {
            const frag_t fb = L::frag(sX, off, ci * 16 + lr, ks, lg);
            acc[q][ci] = F::mma(fa, fb, acc[q][ci]);
          }
        }
      }
    }
  }

  const int64_t pbase = (int64_t)blockIdx.x * a.Na;
#pragma unroll
  for (int q = 0; q < HW_ITEMS; ++q) {
    const int item = wave + 4 * q;
    if (item >= nitems) continue;
    const int j = item >> 1, mi = item & 1;
#pragma unroll
    for (int ci = 0; ci < 2; ++ci) {
      const int c = c0 + ci * 16 + lr;
      if (c >= a.Cin) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + mi * 16 + lg * 4 + r;
        if (m < a.Na) a.wpart[((pbase + m) * a.ntaps + j) * a.Cin + c] = acc[q][ci][r];
      }
    }
  }
  if (ct == 0) {
    sBias[tid >> 5][tid & 31] = bsum;
    __syncthreads();
    if (tid < 32 && m0 + tid < a.Na) {
      float s = 0.f;
#pragma unroll
      for (int p = 0; p < 8; ++p) s += sBias[p][tid];
      a.bpart[pbase + m0 + tid] = s;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// finish: sum of the partials in ascending order, the parameter's layout, weight-norm backward, bias.  One workgroup per slice d0.
//   mode 0, Conv1d v (O, C, k):           partial [p][o][j][c]
//   mode 1, ConvTranspose1d v (C, O, k):  partial [p][ph * O + o][n][c], tap j = ph + u * n (slots ph + u * n >= k are dropped)
//   mode 2, output convolution (1, C, k): partial [p][j][c]
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hifigan_wgrad_finish_kernel(int mode, int D0, int D1, int k, int u, int nparts, const float* __restrict__ wpart,
                                                                   const float* __restrict__ bpart, const float* __restrict__ g,
                                                                   const float* __restrict__ v, float* __restrict__ gw, float* __restrict__ gg,
                                                                   float* __restrict__ gb, int nbias) {
  __shared__ float red[8];
  const int d0 = blockIdx.x, n = D1 * k;
  const int ntaps = (k + u - 1) / u;
  const int Na = mode == 0 ? D0 : (mode == 1 ? u * D1 : 1);
  const int64_t pstride = mode == 0 ? (int64_t)D0 * k * D1 : (mode == 1 ? (int64_t)Na * ntaps * D0 : (int64_t)k * D1);
  const float* vs = v ? v + (int64_t)d0 * n : nullptr;
  float* gws = gw + (int64_t)d0 * n;
  float dot = 0.f, q = 0.f;
  // i walks the PARTIAL's element order where the slice is contiguous there (modes 0, 2), so neighbouring lanes read neighbouring
  // floats; oi is the element's place in the parameter.  The loads of 8 chunks are issued together, the adds stay in chunk order.
  auto place = [&](int i, int& oi) -> int64_t {
    if (mode == 1) {
      const int d1 = i / k, j = i - d1 * k, nn = j / u, ph = j - nn * u;
      oi = i;
      return ((int64_t)(ph * D1 + d1) * ntaps + nn) * D0 + d0;
    }
    const int j = i / D1, d1 = i - j * D1;
    oi = d1 * k + j;
    return (mode == 0 ? (int64_t)d0 * k * D1 : 0) + i;
  };
  for (int i = threadIdx.x; i < n; i += 256) {
    int oi;
    const float* src = wpart + place(i, oi);
    float s = 0.f;
    int p = 0;
    for (; p + 8 <= nparts; p += 8) {
      float t[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = src[(p + e) * pstride];
#pragma unroll
      for (int e = 0; e < 8; ++e) s += t[e];
    }
    for (; p < nparts; ++p) s += src[p * pstride];
    gws[oi] = s;
    if (g) { dot += s * vs[oi]; q += vs[oi] * vs[oi]; }
  }
  if (g) {
    dot = wave_sum(dot);
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = dot; red[4 + (threadIdx.x >> 6)] = q; }
    __syncthreads();
    dot = (red[0] + red[1]) + (red[2] + red[3]);
    q = (red[4] + red[5]) + (red[6] + red[7]);
    const float nrm = sqrtf(q), gv = g[d0];
    const float c1 = gv / nrm, c2 = gv * dot / (nrm * nrm * nrm);
    for (int i = threadIdx.x; i < n; i += 256) {             // each thread re-reads what it wrote itself
      int oi;
      place(i, oi);
      gws[oi] = c1 * gws[oi] - c2 * vs[oi];
    }
    if (threadIdx.x == 0) gg[d0] = dot / nrm;
  }
  if (gb && threadIdx.x < 64) {
    const int reps = mode == 1 ? u : 1;
    for (int o = d0; o < nbias; o += D0) {
      float s = 0.f;
      for (int e = threadIdx.x; e < nparts * reps; e += 64) {
        const int p = e / reps, ph = e - p * reps;
        s += bpart[(int64_t)p * Na + ph * D1 * (mode == 1) + o];
      }
      s = wave_sum(s);
      if (threadIdx.x == 0) gb[o] = s;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// conv_post backward (vocoder.py:103-105 in reverse): dpre = dy (1 - y^2); dx = scale * lrelu'(x) * sum_j dpre[t - j + half] w[j][c];
// weight partial [j][c] = sum_t dpre[t] lrelu(x)[t + j - half][c]; bias partial = sum_t dpre[t].  One workgroup per HO_CHUNK frames.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void hifigan_conv_out_bwd_kernel(int B, int Tn, int C, int k, int ncpu, const T* __restrict__ x,
                                                                   const float* __restrict__ w, const float* __restrict__ y,
                                                                   const float* __restrict__ dy, float slope, float scale,
                                                                   T* __restrict__ dx, float* __restrict__ wpart, float* __restrict__ bpart) {
  __shared__ float sD[HO_CHUNK + 2 * (HO_MAXK / 2) + 2];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / ncpu, ch = blockIdx.x - b * ncpu;
  const int r0 = ch * HO_CHUNK, nrows = min(HO_CHUNK, Tn - r0);
  const int half = (k - 1) / 2;
  for (int r = tid; r < nrows + 2 * half; r += 256) {
    const int t = r0 + r - half;
    float d = 0.f;
    if (t >= 0 && t < Tn) {
      const float yv = y[(int64_t)b * Tn + t];
      d = dy[(int64_t)b * Tn + t] * (1.f - yv * yv);
    }
    sD[r] = d;
  }
  __syncthreads();
  const T* xb = x + (int64_t)b * Tn * C;
  T* dxb = dx + (int64_t)b * Tn * C;
  for (int idx = tid; idx < nrows * C; idx += 256) {
    const int r = idx / C, c = idx - r * C;
    float s = 0.f;
    for (int j = 0; j < k; ++j) s += sD[r - j + 2 * half] * w[j * C + c];
    const int64_t at = (int64_t)(r0 + r) * C + c;
    s = ldf(xb + at) > 0.f ? s : s * slope;
    stf(dxb + at, s * scale);
  }
  for (int idx = tid; idx < k * C; idx += 256) {
    const int j = idx / C, c = idx - j * C;
    float s = 0.f;
    for (int r = 0; r < nrows; ++r) {
      const int t = r0 + r + j - half;
      if (t < 0 || t >= Tn) continue;
      float xv = hg_lrelu(ldf(xb + (int64_t)t * C + c), slope);
      if (sizeof(T) == 2) xv = bf2f(f2bf(xv));               // the rounding the forward's staging applies
      s += sD[r + half] * xv;
    }
    wpart[((int64_t)blockIdx.x * k + j) * C + c] = s;
  }
  float bs = 0.f;
  for (int r = tid; r < nrows; r += 256) bs += sD[r + half];
  bs = wave_sum(bs);
  if ((tid & 63) == 0) red[tid >> 6] = bs;
  __syncthreads();
  if (tid == 0) bpart[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Operand of the data gradient from the folded fp32 weight w (D0, D1, k); the operand buffer is zero-filled by the caller.
//   mode 0, Conv1d w (O, C, k):           op[c][j * Op + o]             = w[o, c, k - 1 - j]     (Op = O rounded up to 32)
//   mode 1, ConvTranspose1d w (C, O, k):  op[c][n * Kp + ph * O + o]    = w[c, o, ph + u * n]    (Kp = u * O rounded up to 32)
template <typename TO>
__global__ __launch_bounds__(256) void hifigan_fold_bwd_kernel(int mode, int D0, int D1, int k, int u, int Kp, const float* __restrict__ w,
                                                               TO* __restrict__ op) {
  const int d0 = blockIdx.x, n = D1 * k;
  const int ntaps = (k + u - 1) / u;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int d1 = i / k, j = i - d1 * k;
    int64_t at;
    if (mode == 0) at = (int64_t)d1 * k * Kp + (int64_t)(k - 1 - j) * Kp + d0;
    else { const int nn = j / u, ph = j - nn * u; at = (int64_t)d0 * ntaps * Kp + (int64_t)nn * Kp + ph * D1 + d1; }
    stf(op + at, w[(int64_t)d0 * n + i]);
  }
}

}  // namespace

extern "C" int s2svc_hifigan_conv1d_dgrad(int dtype, int B, int T, int Cin, int Cout, int k, int dil, const void* dy, const void* w_opT,
                                          const void* mask_src, float slope, const void* res, int accumulate, float scale, void* dx,
                                          void* stream) {
  S2S_REQUIRE(dtype == S2S_F32 || dtype == S2S_BF16, "hifigan_conv1d_dgrad: dtype 0 (float32) or 1 (bfloat16)");
  S2S_REQUIRE(B >= 1 && T >= 1 && Cin >= 1 && Cin <= 512 && Cout >= 1 && Cout <= 512, "hifigan_conv1d_dgrad: 1 <= C_in, C_out <= 512");
  S2S_REQUIRE(dy && w_opT && dx && hg_aligned16(w_opT), "hifigan_conv1d_dgrad: null pointer or unaligned operand");
  const int vec = dtype == S2S_F32 ? 4 : 8;
  HbArgs a = {};
  if (const int rc = hg_conv1d_geom("hifigan_conv1d_dgrad", B, T, k, dil, a.g)) return rc;
  a.a = dy; a.w = w_opT; a.mask = mask_src; a.res = res; a.out = dx;
  a.La = (int64_t)T * Cout; a.B = B; a.Ka = Cout; a.Kap = hg_pad32(Cout); a.aoff = 0; a.N = Cin;
  a.slope = slope; a.scale = scale; a.accumulate = accumulate;
  a.vec_ok = (Cout % vec) == 0 && hg_aligned16(dy);
  return hg_launch<HbDgrad>(dtype, a, (hipStream_t)stream);
}

extern "C" int s2svc_hifigan_tconv1d_dgrad(int dtype, int B, int Tin, int Cin, int Cout, int k, int u, const void* dy, const void* w_opT,
                                           const void* mask_src, float slope, float scale, void* dx, void* stream) {
  S2S_REQUIRE(dtype == S2S_F32 || dtype == S2S_BF16, "hifigan_tconv1d_dgrad: dtype 0 (float32) or 1 (bfloat16)");
  S2S_REQUIRE(B >= 1 && Tin >= 1 && Cin >= 1 && Cin <= 512 && Cout >= 1 && Cout <= 512, "hifigan_tconv1d_dgrad: 1 <= C_in, C_out <= 512");
  S2S_REQUIRE((int64_t)u * Cout < (1 << 20), "hifigan_tconv1d_dgrad: u * C_out too large");
  S2S_REQUIRE(dy && w_opT && dx && hg_aligned16(w_opT), "hifigan_tconv1d_dgrad: null pointer or unaligned operand");
  const int vec = dtype == S2S_F32 ? 4 : 8;
  HbArgs a = {};
  if (const int rc = hg_tconv1d_geom("hifigan_tconv1d_dgrad", B, Tin, k, u, true, a.g)) return rc;
  a.a = dy; a.w = w_opT; a.mask = mask_src; a.res = nullptr; a.out = dx;
  a.La = (int64_t)u * Tin * Cout; a.B = B; a.Ka = u * Cout; a.Kap = hg_pad32(u * Cout); a.aoff = a.g.pad * Cout; a.N = Cin;
  a.slope = slope; a.scale = scale; a.accumulate = 0;
  a.vec_ok = (Cout % vec) == 0 && hg_aligned16(dy);          // then u * C_out, pad * C_out and the utterance stride are vector multiples too
  return hg_launch<HbDgrad>(dtype, a, (hipStream_t)stream);
}

// kind 0: Conv1d (dy (B, T, C_out), x (B, T, C_in), u ignored); kind 1: ConvTranspose1d (dy (B, u T, C_out), x (B, T, C_in)).
// Partials: wpart [B * ncpu][Na][ntaps][C_in], bpart [B * ncpu][Na]; Na = C_out (kind 0) or u * C_out, ntaps = k or ceil(k / u);
// ncpu = ceil(rows / chunk), rows = T (kind 0) or T + ceil(pad / u); chunk a multiple of 32.
extern "C" int s2svc_hifigan_wgrad(int dtype, int kind, int B, int T, int Cin, int Cout, int k, int dil_or_u, int chunk, const void* dy,
                                   const void* x, float slope, float* wpart, float* bpart, void* stream) {
  S2S_REQUIRE(dtype == S2S_F32 || dtype == S2S_BF16, "hifigan_wgrad: dtype 0 (float32) or 1 (bfloat16)");
  S2S_REQUIRE(kind == 0 || kind == 1, "hifigan_wgrad: kind 0 (Conv1d) or 1 (ConvTranspose1d)");
  S2S_REQUIRE(B >= 1 && T >= 1 && Cin >= 1 && Cin <= 512 && Cout >= 1 && Cout <= 512, "hifigan_wgrad: 1 <= C_in, C_out <= 512");
  S2S_REQUIRE(chunk >= HW_TS && chunk % HW_TS == 0, "hifigan_wgrad: chunk is a positive multiple of 32 frames");
  S2S_REQUIRE(dy && x && wpart && bpart, "hifigan_wgrad: null pointer");
  const int vec = dtype == S2S_F32 ? 4 : 8;
  HwArgs a = {};
  a.dy = dy; a.x = x; a.wpart = wpart; a.bpart = bpart; a.B = B; a.Tin = T; a.Cin = Cin; a.slope = slope; a.chunk = chunk;
  HgGeom g;
  if (kind == 0) {
    if (const int rc = hg_conv1d_geom("hifigan_wgrad", B, T, k, dil_or_u, g)) return rc;
    a.Ldy = (int64_t)T * Cout; a.Na = Cout;
  } else {
    const int u = dil_or_u;
    if (const int rc = hg_tconv1d_geom("hifigan_wgrad", B, T, k, u, false, g)) return rc;
    S2S_REQUIRE(g.ntaps <= HW_MAXTAPS, "hifigan_wgrad: more than 12 taps per phase");
    S2S_REQUIRE((int64_t)u * Cout < (1 << 20), "hifigan_wgrad: u * C_out too large");
    a.Ldy = (int64_t)u * T * Cout; a.Na = u * Cout;
  }
  a.aoff = g.pad * Cout; a.ntaps = g.ntaps; a.tstep = g.tstep; a.toff0 = g.toff0; a.offmin = g.offmin; a.span = g.span; a.rows = g.rows;
  a.ncpu = (a.rows + chunk - 1) / chunk;
  a.ctiles = (Cin + 31) / 32;
  const int64_t gy = (int64_t)((a.Na + 31) / 32) * a.ctiles;
  S2S_REQUIRE((int64_t)B * a.ncpu < (1ll << 31) && gy <= 65535, "hifigan_wgrad: grid too large");
  a.vec_dy = (Cout % vec) == 0 && hg_aligned16(dy);
  a.vec_x = (Cin % vec) == 0 && hg_aligned16(x);
  dim3 grid((unsigned)(B * a.ncpu), (unsigned)gy), block(256);
  if (dtype == S2S_F32) hipLaunchKernelGGL(hifigan_wgrad_kernel<float>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(hifigan_wgrad_kernel<bf16_t>, grid, block, 0, (hipStream_t)stream, a);
  S2S_CHECK_LAUNCH("hifigan_wgrad_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_wgrad_finish(int mode, int D0, int D1, int k, int u, int nparts, const float* wpart, const float* bpart,
                                          const float* g, const float* v, float* grad_w, float* grad_g, float* grad_bias, void* stream) {
  S2S_REQUIRE(mode >= 0 && mode <= 2 && D0 >= 1 && D1 >= 1 && k >= 1 && u >= 1 && nparts >= 1, "hifigan_wgrad_finish: bad mode / shape");
  S2S_REQUIRE(mode != 2 || D0 == 1, "hifigan_wgrad_finish: the output convolution has one output channel");
  S2S_REQUIRE(mode != 1 || k >= u, "hifigan_wgrad_finish: ConvTranspose1d k >= u");
  S2S_REQUIRE(wpart && grad_w && (!g || (v && grad_g)) && (!grad_bias || bpart), "hifigan_wgrad_finish: null pointer");
  const int nbias = mode == 1 ? D1 : D0;
  hipLaunchKernelGGL(hifigan_wgrad_finish_kernel, dim3(D0), dim3(256), 0, (hipStream_t)stream, mode, D0, D1, k, mode == 1 ? u : 1, nparts,
                     wpart, bpart, g, v, grad_w, grad_g, grad_bias, nbias);
  S2S_CHECK_LAUNCH("hifigan_wgrad_finish_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_conv_out_bwd(int dtype, int B, int T, int C, int k, int chunk, const void* x, const float* w, const float* y,
                                          const float* dy, float slope, float scale, void* dx, float* wpart, float* bpart, void* stream) {
  S2S_REQUIRE(dtype == S2S_F32 || dtype == S2S_BF16, "hifigan_conv_out_bwd: dtype 0 (float32) or 1 (bfloat16)");
  S2S_REQUIRE(B >= 1 && T >= 1 && C >= 1 && C <= 512 && k >= 1 && (k & 1) && k <= HO_MAXK, "hifigan_conv_out_bwd: bad shape (k odd <= 11, C <= 512)");
  S2S_REQUIRE(chunk == HO_CHUNK, "hifigan_conv_out_bwd: chunk is 256 frames");
  S2S_REQUIRE(x && w && y && dy && dx && wpart && bpart, "hifigan_conv_out_bwd: null pointer");
  const int ncpu = (T + HO_CHUNK - 1) / HO_CHUNK;
  S2S_REQUIRE((int64_t)B * ncpu < (1ll << 31), "hifigan_conv_out_bwd: too many chunks");
  dim3 grid((unsigned)(B * ncpu)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == S2S_F32)
    hipLaunchKernelGGL(hifigan_conv_out_bwd_kernel<float>, grid, block, 0, st, B, T, C, k, ncpu, (const float*)x, w, y, dy, slope, scale, (float*)dx, wpart, bpart);
  else
    hipLaunchKernelGGL(hifigan_conv_out_bwd_kernel<bf16_t>, grid, block, 0, st, B, T, C, k, ncpu, (const bf16_t*)x, w, y, dy, slope, scale, (bf16_t*)dx, wpart, bpart);
  S2S_CHECK_LAUNCH("hifigan_conv_out_bwd_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_fold_bwd(int mode, int D0, int D1, int k, int u, const float* w32, int op_dtype, void* w_opT, void* stream) {
  S2S_REQUIRE((mode == 0 || mode == 1) && D0 >= 1 && D1 >= 1 && k >= 1 && u >= 1 && w32 && w_opT, "hifigan_fold_bwd: bad mode / shape or null pointer");
  S2S_REQUIRE(op_dtype == S2S_F32 || op_dtype == S2S_BF16, "hifigan_fold_bwd: operand dtype 0 / 1");
  S2S_REQUIRE(mode != 1 || k >= u, "hifigan_fold_bwd: ConvTranspose1d k >= u");
  const int Kp = mode == 0 ? hg_pad32(D0) : hg_pad32(u * D1);
  hipStream_t st = (hipStream_t)stream;
  if (op_dtype == S2S_F32)
    hipLaunchKernelGGL(hifigan_fold_bwd_kernel<float>, dim3(D0), dim3(256), 0, st, mode, D0, D1, k, mode == 1 ? u : 1, Kp, w32, (float*)w_opT);
  else
    hipLaunchKernelGGL(hifigan_fold_bwd_kernel<bf16_t>, dim3(D0), dim3(256), 0, st, mode, D0, D1, k, mode == 1 ? u : 1, Kp, w32, (bf16_t*)w_opT);
  S2S_CHECK_LAUNCH("hifigan_fold_bwd_kernel");
  return 0;
}
