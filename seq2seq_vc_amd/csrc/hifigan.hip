// HiFi-GAN generator, inference (reference: seq2seq_vc/urhythmic/vocoder.py:23-202 -- HifiganGenerator, ResBlock).
//
// Activations are channel-last (B, T, C).  Every convolution of the generator is ONE launch of hifigan_gemm_kernel, an implicit
// GEMM whose rows are time frames m = (b, i) and whose reduction index is tap * C_in + c:
//   Conv1d (dilated):   tap j reads frame i + (j - (k-1)/2) * dil;                 columns n = output channel
//   ConvTranspose1d:    tap n reads frame i - n through weight tap p + u * n;       columns (p, o), stored at t = u*i + p - pad
// so the transposed convolution needs no scatter and no col2im pass.  What the reference runs as separate element-wise passes rides
// along: leaky_relu on the A operand as it is staged into LDS (the raw x stays in memory for the residual), bias / residual /
// `out += scale * v` (the MRF average) / tanh in the epilogue.  Frames t >= vlens[b] * vmul are ABSENT (include/s2svc_hip.h): read as
// the zero padding the reference applies at the utterance's own end, written as zero.  The reduction of one output element runs in
// one fixed order that does not depend on the batch, so a row of a batch gets the bits it gets alone.
//
// The tile (128 frames x BN columns per workgroup, the A tile staged once per channel step with its halo) is csrc/hifigan_tile.h,
// shared with the data gradient; this file supplies its A loader (frames with vlens, leaky_relu) and its epilogue.
#include "hifigan_tile.h"

namespace {

// one 16-byte vector of the A operand: load (vector or element-wise with a channel bound), leaky_relu, back to 16 bytes
__device__ __forceinline__ uint4 hg_load_act(const float* p, int nvalid, bool vec, float slope) {
  float f[4] = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (e < nvalid) f[e] = p[e];
  }
  if (slope != 0.f) {
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = hg_lrelu(f[e], slope);
  }
  return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
}
__device__ __forceinline__ uint4 hg_load_act(const bf16_t* p, int nvalid, bool vec, float slope) {
  float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (vec) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    if (slope == 0.f) return v;
    unpack_bf16x8(v, f);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) if (e < nvalid) f[e] = bf2f(p[e]);
  }
  if (slope != 0.f) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = hg_lrelu(f[e], slope);
  }
  return pack_bf16x8(f);
}

struct HgArgs {
  const void* x;         // (B, Tin, Cin)
  const void* w;         // [N][ntaps * Cinp], reduction index tap * Cinp + c, Cinp = Cin rounded up to 32 (zero filled)
  const float* bias;     // [Cout] or NULL
  const void* res;       // (B, Tout, Cout) or NULL
  void* out;             // (B, Tout, Cout)
  const int32_t* vlens;  // (B) or NULL
  HgGeom g;              // tap j reads frame i + j * tstep + toff0
  int B, Tin, Cin, Cinp, Cout, N, Tout, u;
  int vmul_in, vmul_out;
  float slope, scale;
  int accumulate, act_tanh;
};

template <typename T, int BN>
__global__ __launch_bounds__(256) void hifigan_gemm_kernel(const HgArgs a) {
  const int b = blockIdx.x / a.g.tiles;
  const int i0 = (blockIdx.x - b * a.g.tiles) * HG_BM;
  int vlen_in = a.Tin, vlen_out = a.Tout;
  if (a.vlens) {
    const int l = a.vlens[b] > 0 ? a.vlens[b] : 0;
    vlen_in = min(l * a.vmul_in, a.Tin);
    vlen_out = min(l * a.vmul_out, a.Tout);
  }
  const T* xb = (const T*)a.x + (int64_t)b * a.Tin * a.Cin;
  const bool vec_ok = (a.Cin % HgFrag<T>::VEC) == 0;
  T* outb = (T*)a.out + (int64_t)b * a.Tout * a.Cout;
  const T* resb = a.res ? (const T*)a.res + (int64_t)b * a.Tout * a.Cout : nullptr;
  hg_tile<T, BN>(
      a.g, (const T*)a.w, a.Cinp, a.N, i0, blockIdx.y * BN,
      [&](int r, int c) {
        const int t = i0 + r + a.g.offmin;
        if (t < 0 || t >= vlen_in || c >= a.Cin) return make_uint4(0u, 0u, 0u, 0u);
        return hg_load_act(xb + (int64_t)t * a.Cin + c, a.Cin - c, vec_ok, a.slope);
      },
      // epilogue: bias, residual, scale / accumulate, tanh in fp32; one rounding at the store; absent frames are written as zero
      [&](int n) {
        int p = 0, o = n;
        if (a.u > 1) { p = n / a.Cout; o = n - p * a.Cout; }
        const float bv = a.bias ? a.bias[o] : 0.f;
        return [&, p, o, bv](int i, float acc) {
          const int t = a.u * i + p - a.g.pad;
          if (t < 0 || t >= a.Tout) return;
          const int64_t at = (int64_t)t * a.Cout + o;
          float v = 0.f;
          if (t < vlen_out) {
            v = acc + bv;
            if (resb) v += ldf(resb + at);
            v *= a.scale;
            if (a.accumulate) v += ldf(outb + at);
            if (a.act_tanh) v = tanhf(v);
          }
          stf(outb + at, v);
        };
      });
}

struct HgGemm {
  static constexpr const char* name = "hifigan_gemm_kernel";
  template <typename T, int BN> static constexpr auto fn = hifigan_gemm_kernel<T, BN>;
};

// The output convolution C -> 1 (vocoder.py:85, 103-105: leaky_relu, conv_post, tanh): a dot product of k * C values per sample,
// bandwidth bound -- one lane per output sample, a wavefront per 64 consecutive samples, no MFMA tile with 15 dead columns.
template <typename T>
__global__ __launch_bounds__(256) void hifigan_conv_out_kernel(int B, int Tn, int C, int k, const T* __restrict__ x,
                                                               const float* __restrict__ w, const float* __restrict__ bias, float slope,
                                                               int act_tanh, float* __restrict__ y, float* __restrict__ y_pre,
                                                               const int32_t* __restrict__ vlens, int vmul) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * Tn) return;
  const int b = (int)(idx / Tn), t = (int)(idx - (int64_t)b * Tn);
  int vlen = Tn;
  if (vlens) vlen = min((vlens[b] > 0 ? vlens[b] : 0) * vmul, Tn);
  float pre = 0.f, out = 0.f;
  if (t < vlen) {
    float acc = bias ? bias[0] : 0.f;
    const bool vec_ok = (C % VEC) == 0;
    const int half = (k - 1) / 2;
    for (int j = 0; j < k; ++j) {
      const int tt = t + j - half;
      if (tt < 0 || tt >= vlen) continue;
      const T* xr = x + ((int64_t)b * Tn + tt) * C;
      const float* wr = w + j * C;
      if (vec_ok) {
        for (int c = 0; c < C; c += VEC) {
          const uint4 raw = hg_load_act(xr + c, VEC, true, slope);
          if (sizeof(T) == 4) {
            acc += __uint_as_float(raw.x) * wr[c] + __uint_as_float(raw.y) * wr[c + 1] + __uint_as_float(raw.z) * wr[c + 2] +
                   __uint_as_float(raw.w) * wr[c + 3];
          } else {
            float f[8];
            unpack_bf16x8(raw, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc += f[e] * wr[c + e];
          }
        }
      } else {
        for (int c = 0; c < C; ++c) {
          float v = ldf(xr + c);
          if (slope != 0.f) v = hg_lrelu(v, slope);
          if (sizeof(T) == 2) v = bf2f(f2bf(v));          // the rounding the vector path's repacking applies
          acc += v * wr[c];
        }
      }
    }
    pre = acc;
    out = act_tanh ? tanhf(acc) : acc;
  }
  y[idx] = out;
  if (y_pre) y_pre[idx] = pre;
}

// Input launch: x element (b, t, c) at b * sb + t * st + c * sc (the reference's (B, C, N) or the collaters' (B, N, C)) ->
// channel-last (B, T, C) in the compute dtype, with the per-channel affine map a[c] * x + bb[c] of the vocoder wrapper
// (vocoder/vocoder.py:50-55: de-normalise with the target statistics, normalise with the vocoder's).
// The walk is output-major (c fastest): writes are coalesced, and so are the reads of a channel-last input; the reference's
// (B, C, N) input is then read at stride N -- uncoalesced on purpose: the mel is 80 x N values, 0.01 % of the call's traffic,
// and a tiled transpose through LDS would be more code than it saves time.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void hifigan_input_kernel(int B, int Tn, int C, const TI* __restrict__ x, int64_t sb, int64_t st,
                                                            int64_t sc, const float* __restrict__ a, const float* __restrict__ bb,
                                                            TO* __restrict__ out, const int32_t* __restrict__ vlens) {
  const int64_t n = (int64_t)B * Tn * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t r = i / C;
    const int t = (int)(r % Tn), b = (int)(r / Tn);
    float v = 0.f;
    if (!vlens || t < vlens[b]) {
      v = ldf(x + b * sb + t * st + c * sc);
      if (a) v = v * a[c];
      if (bb) v = v + bb[c];
    }
    stf(out + i, v);
  }
}

// Weight-norm fold (torch.nn.utils.weight_norm, vocoder.py:56-85, 125-193): w = v * (g / ||v||), the norm over every dim but 0.
// One workgroup per slice d0 of v (D0, D1, k).  Writes the fp32 weight in the parameter's layout and the kernels' operand:
//   mode 0, Conv1d v (O, C, k):            op[o][j * Cinp + c]                    = w[o, c, j]
//   mode 1, ConvTranspose1d v (C, O, k):   op[p * O + o][n * Cinp + c]            = w[c, o, p + u * n]   (d0 is the INPUT channel)
//   mode 2, output convolution v (1, C, k): op[j * C + c] (fp32)                  = w[0, c, j]
// The operand buffer is zero-filled by the caller (channel padding, taps p + u * n >= k).  g == NULL: v already is the weight.
template <typename TO>
__global__ __launch_bounds__(256) void hifigan_fold_kernel(int mode, int D0, int D1, int k, int u, int Cinp, const float* __restrict__ g,
                                                           const float* __restrict__ v, float* __restrict__ w32, TO* __restrict__ op) {
  __shared__ float red[4];
  const int d0 = blockIdx.x, n = D1 * k;
  const float* vs = v + (int64_t)d0 * n;
  float s = 1.f;
  if (g) {
    float q = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) q += vs[i] * vs[i];
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = q;
    __syncthreads();
    s = g[d0] / sqrtf((red[0] + red[1]) + (red[2] + red[3]));
  }
  const int ntaps = (k + u - 1) / u;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int d1 = i / k, j = i - d1 * k;
    const float wv = vs[i] * s;
    if (w32) w32[(int64_t)d0 * n + i] = wv;
    if (!op) continue;
    int64_t at;
    if (mode == 0) at = (int64_t)d0 * k * Cinp + (int64_t)j * Cinp + d1;
    else if (mode == 1) { const int nn = j / u, p = j - nn * u; at = ((int64_t)p * D1 + d1) * ntaps * Cinp + (int64_t)nn * Cinp + d0; }
    else at = (int64_t)j * D1 + d1;
    stf(op + at, wv);
  }
}

}  // namespace

extern "C" int s2svc_hifigan_cin_padded(int C) { return hg_pad32(C); }

extern "C" int s2svc_hifigan_conv1d(int dtype, int B, int T, int Cin, int Cout, int k, int dil, const void* x, const void* w_op,
                                    const float* bias, float slope, const void* res, int accumulate, float scale, int act_tanh,
                                    void* out, const int32_t* vlens, int vmul, void* stream) {
  S2S_REQUIRE(dtype == S2S_F32 || dtype == S2S_BF16, "hifigan_conv1d: dtype 0 (float32) or 1 (bfloat16)");
  S2S_REQUIRE(B >= 1 && T >= 1 && Cin >= 1 && Cin <= 512 && Cout >= 1 && Cout <= 512, "hifigan_conv1d: 1 <= C_in, C_out <= 512");
  S2S_REQUIRE(x && w_op && out && vmul >= 1, "hifigan_conv1d: null pointer or vmul < 1");
  HgArgs a = {};
  if (const int rc = hg_conv1d_geom("hifigan_conv1d", B, T, k, dil, a.g)) return rc;
  a.x = x; a.w = w_op; a.bias = bias; a.res = res; a.out = out; a.vlens = vlens;
  a.B = B; a.Tin = T; a.Cin = Cin; a.Cinp = hg_pad32(Cin); a.Cout = Cout; a.N = Cout; a.Tout = T; a.u = 1;
  a.vmul_in = vmul; a.vmul_out = vmul;
  a.slope = slope; a.scale = scale; a.accumulate = accumulate; a.act_tanh = act_tanh;
  return hg_launch<HgGemm>(dtype, a, (hipStream_t)stream);
}

extern "C" int s2svc_hifigan_tconv1d(int dtype, int B, int Tin, int Cin, int Cout, int k, int u, const void* x, const void* w_op,
                                     const float* bias, float slope, void* out, const int32_t* vlens, int vmul, void* stream) {
  S2S_REQUIRE(dtype == S2S_F32 || dtype == S2S_BF16, "hifigan_tconv1d: dtype 0 (float32) or 1 (bfloat16)");
  S2S_REQUIRE(B >= 1 && Tin >= 1 && Cin >= 1 && Cin <= 512 && Cout >= 1 && Cout <= 512, "hifigan_tconv1d: 1 <= C_in, C_out <= 512");
  S2S_REQUIRE(x && w_op && out && vmul >= 1, "hifigan_tconv1d: null pointer or vmul < 1");
  HgArgs a = {};
  if (const int rc = hg_tconv1d_geom("hifigan_tconv1d", B, Tin, k, u, false, a.g)) return rc;
  a.x = x; a.w = w_op; a.bias = bias; a.res = nullptr; a.out = out; a.vlens = vlens;
  a.B = B; a.Tin = Tin; a.Cin = Cin; a.Cinp = hg_pad32(Cin); a.Cout = Cout; a.N = u * Cout; a.Tout = u * Tin; a.u = u;
  a.vmul_in = vmul; a.vmul_out = vmul * u;
  a.slope = slope; a.scale = 1.f; a.accumulate = 0; a.act_tanh = 0;
  return hg_launch<HgGemm>(dtype, a, (hipStream_t)stream);
}

extern "C" int s2svc_hifigan_conv_out(int dtype, int B, int T, int C, int k, const void* x, const float* w, const float* bias,
                                      float slope, int act_tanh, float* y, float* y_pre, const int32_t* vlens, int vmul, void* stream) {
  S2S_REQUIRE(dtype == S2S_F32 || dtype == S2S_BF16, "hifigan_conv_out: dtype 0 (float32) or 1 (bfloat16)");
  S2S_REQUIRE(B >= 1 && T >= 1 && C >= 1 && k >= 1 && (k & 1) && x && w && y && vmul >= 1, "hifigan_conv_out: bad shape or null pointer");
  const int64_t n = (int64_t)B * T;
  S2S_REQUIRE((n + 255) / 256 < (1ll << 31), "hifigan_conv_out: too many samples for one grid");
  dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == S2S_F32)
    hipLaunchKernelGGL(hifigan_conv_out_kernel<float>, grid, block, 0, st, B, T, C, k, (const float*)x, w, bias, slope, act_tanh, y, y_pre, vlens, vmul);
  else
    hipLaunchKernelGGL(hifigan_conv_out_kernel<bf16_t>, grid, block, 0, st, B, T, C, k, (const bf16_t*)x, w, bias, slope, act_tanh, y, y_pre, vlens, vmul);
  S2S_CHECK_LAUNCH("hifigan_conv_out_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_input(int in_dtype, int out_dtype, int B, int T, int C, const void* x, int64_t sb, int64_t st_, int64_t sc,
                                   const float* a, const float* b, void* out, const int32_t* vlens, void* stream) {
  S2S_REQUIRE((in_dtype == S2S_F32 || in_dtype == S2S_BF16) && (out_dtype == S2S_F32 || out_dtype == S2S_BF16), "hifigan_input: dtypes 0 / 1");
  S2S_REQUIRE(B >= 1 && T >= 1 && C >= 1 && x && out, "hifigan_input: bad shape or null pointer");
  const int64_t n = (int64_t)B * T * C;
  dim3 grid((unsigned)((n + 255) / 256 < 65535 ? (n + 255) / 256 : 65535)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (in_dtype == S2S_F32 && out_dtype == S2S_F32)
    hipLaunchKernelGGL((hifigan_input_kernel<float, float>), grid, block, 0, st, B, T, C, (const float*)x, sb, st_, sc, a, b, (float*)out, vlens);
  else if (in_dtype == S2S_F32)
    hipLaunchKernelGGL((hifigan_input_kernel<float, bf16_t>), grid, block, 0, st, B, T, C, (const float*)x, sb, st_, sc, a, b, (bf16_t*)out, vlens);
  else if (out_dtype == S2S_F32)
    hipLaunchKernelGGL((hifigan_input_kernel<bf16_t, float>), grid, block, 0, st, B, T, C, (const bf16_t*)x, sb, st_, sc, a, b, (float*)out, vlens);
  else
    hipLaunchKernelGGL((hifigan_input_kernel<bf16_t, bf16_t>), grid, block, 0, st, B, T, C, (const bf16_t*)x, sb, st_, sc, a, b, (bf16_t*)out, vlens);
  S2S_CHECK_LAUNCH("hifigan_input_kernel");
  return 0;
}

extern "C" int s2svc_hifigan_fold(int mode, int D0, int D1, int k, int u, const float* g, const float* v, float* w32, int op_dtype,
                                  void* w_op, void* stream) {
  S2S_REQUIRE(mode >= 0 && mode <= 2 && D0 >= 1 && D1 >= 1 && k >= 1 && u >= 1 && v, "hifigan_fold: bad mode / shape or null pointer");
  S2S_REQUIRE(op_dtype == S2S_F32 || op_dtype == S2S_BF16, "hifigan_fold: operand dtype 0 / 1");
  S2S_REQUIRE(mode != 2 || (D0 == 1 && op_dtype == S2S_F32), "hifigan_fold: the output convolution's operand is fp32, one output channel");
  const int Cinp = hg_pad32(mode == 1 ? D0 : D1);
  hipStream_t st = (hipStream_t)stream;
  if (op_dtype == S2S_F32)
    hipLaunchKernelGGL(hifigan_fold_kernel<float>, dim3(D0), dim3(256), 0, st, mode, D0, D1, k, mode == 1 ? u : 1, Cinp, g, v, w32, (float*)w_op);
  else
    hipLaunchKernelGGL(hifigan_fold_kernel<bf16_t>, dim3(D0), dim3(256), 0, st, mode, D0, D1, k, mode == 1 ? u : 1, Cinp, g, v, w32, (bf16_t*)w_op);
  S2S_CHECK_LAUNCH("hifigan_fold_kernel");
  return 0;
}
