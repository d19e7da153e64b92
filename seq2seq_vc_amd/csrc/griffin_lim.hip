// Griffin-Lim phase reconstruction (librosa.griffinlim with init="random", as the reference's vocoder/griffin_lim.py:53-106 calls
// it) for a batch of spectrograms with per-row lengths, fp32, in 2 n_iter + 3 launches whatever the batch:
//
//   prepare   one workgroup per (row, frame): optional x * scale + mean, 10^x, the product with the pseudo-inverse of the mel basis,
//             the clamp (vocoder/griffin_lim.py:20-50) -> S;  X0 = S exp(2 pi i u), u given or drawn from a counter-based generator
//   synth     one wavefront per frame: inverse real FFT of X[t] in LDS (fft_wave.h: the Stockham passes on the packed half-size
//             complex sequence), times the window -> frame buffer (B, Tmax, n_fft)
//   analyse   one wavefront per frame t: the n_fft samples of the centre-padded waveform that frame t of the forward STFT covers are
//             GATHERED from the overlapping windowed frames of that buffer in ascending frame order (no atomics: the order of every sum
//             is fixed, whatever the scheduling or the batch), divided by the squared-window envelope of the frames this row has,
//             zero / reflect padded by index arithmetic, windowed, transformed; then A = R - c R_prev, X = S A / (|A| + tiny),
//             R_prev = R, written in place (a frame's workgroup reads the frame buffer and writes only its own X / R_prev row)
//   ola       the final waveform by the same gather, one lane per sample
//
// The waveform is materialised once, by ola.  Frames t >= lens[b] are absent (the header's notion): they contribute to no sum, their S / X
// are written as zero by prepare and nothing else touches them.  A row with fewer than 2 frames has no samples and is absent as a whole.
// The transform, its (un)pack steps, the table of twiddle factors and window, the reflect index and the overlap-add frame range are
// those of fft_wave.h.
#include "fft_wave.h"
#include "../../include/s2svc_hip.h"
#include <float.h>

namespace {

constexpr int WAVES = 4;       // frames per workgroup

// frames this row has: fewer than two give no sample (n_shift * (T - 1) = 0), the row is absent as a whole
__device__ __forceinline__ int row_frames(const int32_t* __restrict__ lens, int b, int Tmax) {
  const int T = lens ? lens[b] : Tmax;
  return T < 2 ? 0 : (T < Tmax ? T : Tmax);
}

// Sample `pos` of the overlap-added, envelope-normalised signal of one row BEFORE the centre trim (pos in [0, hop (T - 1) + N)):
// the windowed frames that cover it, summed in ascending frame order, over the sum of their squared window values where that
// exceeds the smallest normal fp32 (librosa.istft).  fr = the row's (Tmax, N) windowed frames.
__device__ __forceinline__ float ola_sample(const float* __restrict__ fr, const float* __restrict__ win, int64_t pos, int T, int hop, int N) {
  int t_lo, t_hi;
  ola_frame_range(pos, N, hop, T, t_lo, t_hi);
  float acc = 0.f, env = 0.f;
  for (int t = t_lo; t <= t_hi; ++t) {
    const int o = (int)(pos - (int64_t)t * hop);              // 0 <= o < N by the range
    const float w = win[o];
    acc += fr[(int64_t)t * N + o];
    env += w * w;
  }
  return env > FLT_MIN ? acc / env : acc;
}

struct gl_args {
  int B, Tmax, hop, reflect, have_prev;
  float coef;
  const int32_t* lens;
  const float* tables;
  const float* S;              // (B, Tmax, H + 1)
  float* X;                    // (B, Tmax, H + 1) complex
  float* Rprev;                // (B, Tmax, H + 1) complex
  float* frames;               // (B, Tmax, N)
};

// ---- synth: frames[b, t, :] = win * irfft(X[b, t, :]) ----
template <int LOG2N>
__global__ __launch_bounds__(64 * WAVES) void gl_synth_kernel(gl_args a) {
  constexpr int N = 1 << LOG2N, H = N / 2, PPL = H / 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  c32* tw = reinterpret_cast<c32*>(smem_raw);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  c32* bx = tw + H + wave * 2 * H;
  c32* by = bx + H;
  const FftTable tab = fft_table(a.tables, N);
  load_twiddles<H, 64 * WAVES>(tw, tab);
  __syncthreads();
  const int gpb = (a.Tmax + WAVES - 1) / WAVES;
#pragma unroll 1
  for (int g = blockIdx.x; g < a.B * gpb; g += gridDim.x) {
    const int b = g / gpb, t = (g - b * gpb) * WAVES + wave;
    if (t >= row_frames(a.lens, b, a.Tmax)) continue;         // (wave-uniform) absent frame: never read
    const c32* X = reinterpret_cast<const c32*>(a.X) + ((int64_t)b * a.Tmax + t) * (H + 1);
    // the imaginary parts of X[0] and X[H] are ignored (numpy's irfft)
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
      const int k = lane + 64 * q;
      c32 xa = X[k], xb = X[H - k];
      if (k == 0) { xa.y = 0.f; xb.y = 0.f; }
      bx[k] = pack_conj(xa, xb, tab.tf[k]);
    }
    const c32* r = fft_forward<H>(bx, by, tw, lane);
    float* fo = a.frames + ((int64_t)b * a.Tmax + t) * N;
    const float inv = 1.0f / H;
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
      const int n = lane + 64 * q;
      const c32 v = r[n];
      const float2 wv = *reinterpret_cast<const float2*>(tab.win + 2 * n);
      *reinterpret_cast<float2*>(fo + 2 * n) = make_float2(v.x * inv * wv.x, -v.y * inv * wv.y);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// one bin of the projection step
__device__ __forceinline__ void project(const gl_args& a, int64_t idx, c32 R) {
  c32* X = reinterpret_cast<c32*>(a.X);
  c32* P = reinterpret_cast<c32*>(a.Rprev);
  c32 A = R;
  if (a.have_prev) {
    const c32 p = P[idx];
    A = {R.x - a.coef * p.x, R.y - a.coef * p.y};
  }
  const float s = a.S[idx] / (sqrtf(A.x * A.x + A.y * A.y) + FLT_MIN);
  X[idx] = {s * A.x, s * A.y};
  P[idx] = R;
}

// ---- analyse: R = stft(istft(X)) for frame t, momentum, projection ----
template <int LOG2N>
__global__ __launch_bounds__(64 * WAVES) void gl_analyse_kernel(gl_args a) {
  constexpr int N = 1 << LOG2N, H = N / 2, PPL = H / 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  c32* tw = reinterpret_cast<c32*>(smem_raw);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  c32* bx = tw + H + wave * 2 * H;
  c32* by = bx + H;
  const FftTable tab = fft_table(a.tables, N);
  load_twiddles<H, 64 * WAVES>(tw, tab);
  __syncthreads();
  const int gpb = (a.Tmax + WAVES - 1) / WAVES;
#pragma unroll 1
  for (int g = blockIdx.x; g < a.B * gpb; g += gridDim.x) {
    const int b = g / gpb, t = (g - b * gpb) * WAVES + wave;
    const int T = row_frames(a.lens, b, a.Tmax);
    if (t >= T) continue;
    const float* fr = a.frames + (int64_t)b * a.Tmax * N;
    const int64_t L = (int64_t)a.hop * (T - 1);               // samples of the trimmed waveform
    const int64_t period = L > 1 ? 2 * (L - 1) : 1;
    const int64_t s0 = (int64_t)t * a.hop - H;                // first sample of frame t in the trimmed waveform's coordinates
#pragma unroll 1
    for (int q = 0; q < PPL; ++q) {
      const int p = lane + 64 * q;
      float v[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        int64_t j = s0 + 2 * p + e;
        bool zero = false;
        if (j < 0 || j >= L) {
          if (a.reflect) j = reflect_index(j, L, period);
          else zero = true;
        }
        v[e] = zero ? 0.f : ola_sample(fr, tab.win, j + H, T, a.hop, N) * tab.win[2 * p + e];
      }
      bx[p] = {v[0], v[1]};
    }
    const c32* z = fft_forward<H>(bx, by, tw, lane);
    const int64_t row = ((int64_t)b * a.Tmax + t) * (H + 1);
    for (int k = lane; k <= H / 2; k += 64) {
      c32 xa, xb;
      unpack_pair<H>(z, tab.tf, k, xa, xb);
      project(a, row + k, xa);
      if (k != H - k) project(a, row + H - k, xb);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- ola: y[b, j] = sample j + N / 2 of the normalised overlap-add, zero past the row's n_shift * (T - 1) samples ----
__global__ __launch_bounds__(256) void gl_ola_kernel(int B, int Tmax, int N, int hop, const float* __restrict__ frames, const int32_t* __restrict__ lens,
                                                     const float* __restrict__ win, float* __restrict__ y) {
  const int64_t Lmax = (int64_t)hop * (Tmax - 1);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * Lmax) return;
  const int b = (int)(i / Lmax);
  const int64_t j = i - (int64_t)b * Lmax;
  const int T = row_frames(lens, b, Tmax);
  float v = 0.f;
  if (j < (int64_t)hop * (T - 1)) v = ola_sample(frames + (int64_t)b * Tmax * N, win, j + N / 2, T, hop, N);
  y[i] = v;
}

// ---- prepare ----
struct prep_args {
  int B, Tmax, nb, D, nmel;
  const float* x;              // (B, Tmax, D)
  const float* scale;          // [D] or NULL
  const float* mean;           // [D] or NULL
  const float* pinv_t;         // (nmel, nb): transposed pseudo-inverse of the mel basis, or NULL: x is a linear spectrogram (D = nb)
  float eps;
  const float* u;              // (B, Tmax, nb) or NULL: drawn from (seed, row, frame, bin)
  uint64_t seed;
  const int32_t* lens;
  float* S;
  float* X;                    // or NULL
  float* Rprev;                // or NULL: absent frames are zero-filled
  int32_t* nsamp;              // or NULL: [B] hop * (frames - 1)
  int hop;
};

__global__ __launch_bounds__(256) void gl_prepare_kernel(prep_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* m = reinterpret_cast<float*>(smem_raw);              // [nmel] linear mel magnitudes of this frame
  const int b = blockIdx.x / a.Tmax, t = blockIdx.x - b * a.Tmax;
  const int T = row_frames(a.lens, b, a.Tmax);
  if (t == 0 && threadIdx.x == 0 && a.nsamp) a.nsamp[b] = T > 0 ? a.hop * (T - 1) : 0;
  const int64_t row = (int64_t)blockIdx.x * a.nb;
  c32* X = reinterpret_cast<c32*>(a.X);
  c32* P = reinterpret_cast<c32*>(a.Rprev);
  if (t >= T) {
    for (int k = threadIdx.x; k < a.nb; k += blockDim.x) {
      a.S[row + k] = 0.f;
      if (X) X[row + k] = {0.f, 0.f};
      if (P) P[row + k] = {0.f, 0.f};
    }
    return;
  }
  const float* x = a.x + (int64_t)blockIdx.x * a.D;
  if (a.pinv_t) {
    // de-normalisation and 10^x in double: n_mels values per frame, rounded once to the fp32 the product reads
    for (int i = threadIdx.x; i < a.nmel; i += blockDim.x) {
      double v = x[i];
      if (a.scale) v = v * (double)a.scale[i] + (double)a.mean[i];
      m[i] = (float)exp10(v);
    }
    __syncthreads();
  }
  for (int k = threadIdx.x; k < a.nb; k += blockDim.x) {
    float s;
    if (a.pinv_t) {
      // the pseudo-inverse has entries of both signs: the products (exact in double) are summed in double, in mel order
      double acc = 0.0;
      for (int i = 0; i < a.nmel; ++i) acc += (double)a.pinv_t[(int64_t)i * a.nb + k] * (double)m[i];
      s = fmaxf(a.eps, (float)acc);
    } else {
      float v = x[k];
      if (a.scale) v = v * a.scale[k] + a.mean[k];
      s = fabsf(v);
    }
    a.S[row + k] = s;
    if (X) {
      float u;
      if (a.u) {
        u = a.u[row + k];
      } else {
        const uint64_t r = dropout_draw(a.seed, ((uint64_t)b << 40) + (uint64_t)t * a.nb + k);
        u = (float)(r >> 40) * (1.0f / 16777216.0f);         // 24 bits: uniform on [0, 1)
      }
      float sn, cs;
      sincospif(2.0f * u, &sn, &cs);
      X[row + k] = {s * cs, s * sn};
    }
  }
}

template <int LOG2N>
int launch_frames(bool analyse, const gl_args& a, hipStream_t st) {
  constexpr int H = (1 << LOG2N) / 2;
  const size_t lds = sizeof(c32) * (H + (size_t)WAVES * 2 * H);
  const char* err = "griffin_lim: cannot raise the dynamic LDS limit";
  if (int rc = analyse ? fft_raise_lds_limit<gl_analyse_kernel<LOG2N>>(lds, err) : fft_raise_lds_limit<gl_synth_kernel<LOG2N>>(lds, err)) return rc;
  const dim3 grid = fft_persistent_grid((int64_t)a.B * ((a.Tmax + WAVES - 1) / WAVES), lds, 8);
  if (analyse) hipLaunchKernelGGL(gl_analyse_kernel<LOG2N>, grid, dim3(64 * WAVES), lds, st, a);
  else hipLaunchKernelGGL(gl_synth_kernel<LOG2N>, grid, dim3(64 * WAVES), lds, st, a);
  S2S_CHECK_LAUNCH(analyse ? "gl_analyse_kernel" : "gl_synth_kernel");
  return 0;
}

int dispatch_frames(bool analyse, int n_fft, const gl_args& a, hipStream_t st) {
  if (n_fft == 512) return launch_frames<9>(analyse, a, st);
  if (n_fft == 1024) return launch_frames<10>(analyse, a, st);
  return launch_frames<11>(analyse, a, st);
}

bool fft_ok(int n_fft) { return n_fft == 512 || n_fft == 1024 || n_fft == 2048; }

}  // namespace

extern "C" int s2svc_gl_supported(int n_fft) { return fft_ok(n_fft) ? 1 : 0; }

extern "C" int s2svc_gl_prepare(int B, int Tmax, int nb, int D, int nmel, int hop, const float* x, const float* scale, const float* mean,
                                const float* pinv_t, float eps, const float* u, uint64_t seed, const int32_t* lens, float* S, float* X,
                                float* Rprev, int32_t* nsamp, void* stream) {
  S2S_REQUIRE(B > 0 && Tmax > 0 && nb > 0 && D > 0 && hop > 0 && x && S && (int64_t)B * Tmax < (1ll << 31), "gl_prepare: bad args");
  S2S_REQUIRE((scale == nullptr) == (mean == nullptr), "gl_prepare: scale and mean come together");
  S2S_REQUIRE(pinv_t ? (nmel == D && nmel <= 16384) : D == nb, "gl_prepare: x is (B, Tmax, n_mels) with a pseudo-inverse, (B, Tmax, bins) without");
  prep_args a;
  a.B = B; a.Tmax = Tmax; a.nb = nb; a.D = D; a.nmel = nmel; a.x = x; a.scale = scale; a.mean = mean; a.pinv_t = pinv_t; a.eps = eps;
  a.u = u; a.seed = seed; a.lens = lens; a.S = S; a.X = X; a.Rprev = Rprev; a.nsamp = nsamp; a.hop = hop;
  hipLaunchKernelGGL(gl_prepare_kernel, dim3(B * Tmax), dim3(256), pinv_t ? sizeof(float) * nmel : 0, (hipStream_t)stream, a);
  S2S_CHECK_LAUNCH("gl_prepare_kernel");
  return 0;
}

extern "C" int s2svc_gl_synth(int B, int Tmax, int n_fft, const float* X, const int32_t* lens, const float* tables, float* frames,
                              void* stream) {
  S2S_REQUIRE(fft_ok(n_fft), "gl_synth: n_fft must be 512 / 1024 / 2048");
  S2S_REQUIRE(B > 0 && Tmax > 0 && X && tables && frames && ((uintptr_t)tables) % 8 == 0 && ((uintptr_t)frames) % 8 == 0 && ((uintptr_t)X) % 8 == 0,
              "gl_synth: bad args");
  gl_args a = {};
  a.B = B; a.Tmax = Tmax; a.lens = lens; a.tables = tables; a.X = const_cast<float*>(X); a.frames = frames;
  return dispatch_frames(false, n_fft, a, (hipStream_t)stream);
}

extern "C" int s2svc_gl_analyse(int B, int Tmax, int n_fft, int hop, int reflect, const float* frames, const float* S, const int32_t* lens,
                                const float* tables, float coef, int have_prev, float* X, float* Rprev, void* stream) {
  S2S_REQUIRE(fft_ok(n_fft), "gl_analyse: n_fft must be 512 / 1024 / 2048");
  S2S_REQUIRE(B > 0 && Tmax > 0 && hop > 0 && frames && S && tables && X && Rprev && ((uintptr_t)tables) % 8 == 0 && ((uintptr_t)X) % 8 == 0 &&
              ((uintptr_t)Rprev) % 8 == 0, "gl_analyse: bad args");
  gl_args a = {};
  a.B = B; a.Tmax = Tmax; a.hop = hop; a.reflect = reflect; a.have_prev = have_prev; a.coef = coef; a.lens = lens; a.tables = tables; a.S = S;
  a.X = X; a.Rprev = Rprev; a.frames = const_cast<float*>(frames);
  return dispatch_frames(true, n_fft, a, (hipStream_t)stream);
}

extern "C" int s2svc_gl_ola(int B, int Tmax, int n_fft, int hop, const float* frames, const int32_t* lens, const float* tables, float* y,
                            void* stream) {
  S2S_REQUIRE(fft_ok(n_fft), "gl_ola: n_fft must be 512 / 1024 / 2048");
  S2S_REQUIRE(B > 0 && Tmax > 1 && hop > 0 && frames && tables && y, "gl_ola: bad args (Tmax >= 2)");
  const int64_t total = (int64_t)B * hop * (Tmax - 1);
  S2S_REQUIRE((total + 255) / 256 < (1ll << 31), "gl_ola: too many samples for one launch");
  hipLaunchKernelGGL(gl_ola_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, Tmax, n_fft, hop, frames, lens,
                     fft_table(tables, n_fft).win, y);
  S2S_CHECK_LAUNCH("gl_ola_kernel");
  return 0;
}
