// Differentiable log-mel spectrogram and its fused L1 loss, fp32, n_fft = 1024 (HiFi-GAN generator fine-tuning).
//
// replaces: urhythmic/dataset.py:23-50 (LogMelSpectrogram: F.pad reflect -> torchaudio MelSpectrogram(center=False, power=1, Slaney
// scale and norm) -> log(clamp(., 1e-5))) and the F.l1_loss behind it (urhythmic_fine_tune_vocoder.py:191-222), forward and backward.
//
//   forward      one wavefront per frame (b, t): windowed load (the reflect padding is index arithmetic on the raw waveform, no padded
//                copy exists), 512-point complex FFT of the even / odd packed frame in LDS (fft_wave.h), unpack, magnitude, mel
//                projection by SEGMENTS (a bin has at most two non-zero weights, in neighbouring filters), mel and
//                log(max(mel, eps)) stored as (B, n_mels, T); with a target also one partial sum_m |logmel - tgt| per frame, in double
//   loss finish  the B T partials summed in ascending order in double, scaled, rounded once to fp32
//   bwd frames   one wavefront per frame: the spectrum is RECOMPUTED from the waveform; g_mel = g_logmel / mel where mel >= eps (ties
//                included), 0 below; g_mag[k] = the two-weight projection back to the bins; G = g_mag X / |X| (0 where |X| = 0, as
//                torch.abs of a complex tensor); frame gradient = win[n] Re sum_{k = 0 .. N/2} G[k] exp(+2 pi i k n / N) -- a one-sided
//                sum, interior bins NOT doubled -- = N irfft(H), H[0] = Re G[0], H[k] = G[k] / 2, H[N/2] = Re G[N/2], by the packed
//                inverse transform (fft_wave.h: pack_conj) -> frames (B, T, N)
//   bwd ola      one lane per waveform sample: the up-to-three padded positions that read it (left mirror, itself, right mirror),
//                each gathered from the frames that cover it, in ascending (position, frame) order -> dwav
//
// No atomics: the order of every sum is fixed, whatever the scheduling or the batch, so two calls give the same bits and a batch row
// equals its own B = 1 call.  The transform, its (un)pack steps, the table of twiddle factors and window and the overlap-add
// frame range are those of fft_wave.h.
#include "fft_wave.h"
#include "../../include/s2svc_hip.h"

namespace {

constexpr int N = 1024, H = N / 2, PPL = H / 64;
constexpr int WAVES = 4;       // frames per workgroup
constexpr int WUD_N = 520;     // [H + 1] bin weights, padded

struct mel_args {
  int B, T, hop, pad, nmel;
  int64_t Nw;                  // samples of every row
  const float* wav;            // (B, Nw)
  const float* tables;         // the packed table of fft_wave.h
  const int32_t* seg_lo;       // [nmel + 1] first bin of segment s: the bins between the peaks of filters s - 1 and s
  const int32_t* seg_len;      // [nmel + 1]
  const float* wud;            // [H + 1][2]: weight of filter s(k) (rising side) and of filter s(k) - 1 (falling side) at bin k
  const int32_t* bin_seg;      // [H + 1] s(k)
  float eps;
  float* mel;                  // (B, nmel, T)
  float* logmel;               // (B, nmel, T)
  const float* tgt;            // (B, nmel, T) or NULL
  double* partials;            // [B T] or NULL
  const float* g_logmel;       // (B, nmel, T) or NULL: the fused loss, g = sign(logmel - tgt) * gscale * gout[0]
  const float* gout;           // [1]
  float gscale;
  float* frames;               // (B, T, N)
};

// the LDS of both frame kernels: twiddles | bin weights | segments | bin -> segment | per wave: two FFT buffers and a scratch row
struct lds_view {
  c32* tw;
  float2* wud;
  int32_t *seg_lo, *seg_len, *bin_seg;
  c32 *bx, *by;
  float* row;                  // [row_n]
};
__host__ __device__ __forceinline__ int row_floats(int nmel) { return (2 * (nmel + 1) + 3) & ~3; }
__host__ __device__ __forceinline__ int seg_ints(int nmel) { return (nmel + 1 + 1) & ~1; }
size_t lds_bytes(int nmel) {
  return sizeof(c32) * H + sizeof(float2) * WUD_N + sizeof(int32_t) * (2 * seg_ints(nmel) + WUD_N) +
         (size_t)WAVES * (sizeof(c32) * 2 * H + sizeof(float) * row_floats(nmel));
}

__device__ __forceinline__ lds_view carve(unsigned char* smem, const mel_args& a, int wave) {
  lds_view v;
  v.tw = reinterpret_cast<c32*>(smem);
  v.wud = reinterpret_cast<float2*>(v.tw + H);
  v.seg_lo = reinterpret_cast<int32_t*>(v.wud + WUD_N);
  v.seg_len = v.seg_lo + seg_ints(a.nmel);
  v.bin_seg = v.seg_len + seg_ints(a.nmel);
  c32* bufs = reinterpret_cast<c32*>(v.bin_seg + WUD_N);
  v.bx = bufs + wave * 2 * H;
  v.by = v.bx + H;
  v.row = reinterpret_cast<float*>(bufs + WAVES * 2 * H) + wave * row_floats(a.nmel);
  return v;
}

__device__ __forceinline__ void load_tables(const lds_view& v, const mel_args& a, const FftTable& tab) {
  load_twiddles<H, 64 * WAVES>(v.tw, tab);
  for (int i = threadIdx.x; i < H + 1; i += 64 * WAVES) {
    v.wud[i] = reinterpret_cast<const float2*>(a.wud)[i];
    if (a.bin_seg) {
      const int s = a.bin_seg[i];
      v.bin_seg[i] = s < 0 ? 0 : (s > a.nmel ? a.nmel : s);
    }
  }
  if (a.seg_lo)
    for (int i = threadIdx.x; i < a.nmel + 1; i += 64 * WAVES) {
      // a segment stays inside the H + 1 bins whatever the table says
      int lo = a.seg_lo[i], n = a.seg_len[i];
      lo = lo < 0 ? 0 : (lo > H ? H : lo);
      n = n < 0 ? 0 : (n > H + 1 - lo ? H + 1 - lo : n);
      v.seg_lo[i] = lo;
      v.seg_len[i] = n;
    }
  __syncthreads();
}

// frame t of row b: samples [t hop - pad, t hop - pad + N) of the reflect-padded row, windowed, even / odd packed.  The launcher has
// checked Nw > pad and T = (Nw + 2 pad - N) / hop + 1, so one reflection lands inside the row.
__device__ __forceinline__ void load_frame(const mel_args& a, int b, int t, c32* bx, const float* win, int lane) {
  const float* xb = a.wav + (int64_t)b * a.Nw;
  const int64_t s0 = (int64_t)t * a.hop - a.pad;
#pragma unroll
  for (int q = 0; q < PPL; ++q) {
    const int p = lane + 64 * q;
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      int64_t j = s0 + 2 * p + e;
      if (j < 0) j = -j;
      if (j >= a.Nw) j = 2 * (a.Nw - 1) - j;
      j = j < 0 ? 0 : (j >= a.Nw ? a.Nw - 1 : j);
      v[e] = xb[j] * win[2 * p + e];
    }
    bx[p] = {v[0], v[1]};
  }
}

// ---- forward ----
__global__ __launch_bounds__(64 * WAVES) void melspec_fwd_kernel(mel_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const lds_view v = carve(smem_raw, a, wave);
  const FftTable tab = fft_table(a.tables, N);
  load_tables(v, a, tab);
  const int nseg = a.nmel + 1;
  float* up = v.row;
  float* dn = up + nseg;
  const int gpb = (a.T + WAVES - 1) / WAVES;
#pragma unroll 1
  for (int g = blockIdx.x; g < a.B * gpb; g += gridDim.x) {
    const int b = g / gpb, t = (g - b * gpb) * WAVES + wave;
    if (t >= a.T) continue;                                   // (wave-uniform)
    load_frame(a, b, t, v.bx, tab.win, lane);
    c32* z = fft_forward<H>(v.bx, v.by, v.tw, lane);
    float* mag = reinterpret_cast<float*>(z == v.bx ? v.by : v.bx);      // [H + 1] <= 2 H floats
    for (int k = lane; k <= H / 2; k += 64) {
      c32 xa, xb;
      unpack_pair<H>(z, tab.tf, k, xa, xb);
      mag[k] = sqrtf(xa.x * xa.x + xa.y * xa.y);
      mag[H - k] = sqrtf(xb.x * xb.x + xb.y * xb.y);
    }
    __builtin_amdgcn_wave_barrier();
    // mel by segments: up[s] = the rising side of filter s, dn[s] = the falling side of filter s - 1, over the bins of segment s
    for (int s = lane; s < nseg; s += 64) {
      const int lo = v.seg_lo[s], n = v.seg_len[s];
      float su = 0.f, sd = 0.f;
      for (int it = 0; it < n; ++it) {
        const float2 w = v.wud[lo + it];
        const float mg = mag[lo + it];
        su += w.x * mg;
        sd += w.y * mg;
      }
      up[s] = su;
      dn[s] = sd;
    }
    __builtin_amdgcn_wave_barrier();
    double part = 0.0;
    for (int m = lane; m < a.nmel; m += 64) {
      const float ml = up[m] + dn[m + 1];
      const float lm = logf(fmaxf(ml, a.eps));
      const int64_t idx = ((int64_t)b * a.nmel + m) * a.T + t;
      a.mel[idx] = ml;
      a.logmel[idx] = lm;
      if (a.tgt) part += (double)fabsf(lm - a.tgt[idx]);
    }
    if (a.tgt) {                                              // (wave-uniform) a fixed butterfly: the same bits on every call
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
      if (lane == 0) a.partials[(int64_t)b * a.T + t] = part;
    }
    __builtin_amdgcn_wave_barrier();                          // the next frame of this wave reuses its buffers
  }
}

// ---- loss finish: sum of n partials in ascending order, in double; one rounding ----
__global__ __launch_bounds__(256) void melspec_loss_finish_kernel(int64_t n, const double* __restrict__ partials, double inv_count,
                                                                  float* __restrict__ loss) {
  __shared__ double chunk[256];
  double acc = 0.0;
  for (int64_t i0 = 0; i0 < n; i0 += 256) {
    const int64_t i = i0 + threadIdx.x;
    chunk[threadIdx.x] = i < n ? partials[i] : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = n - i0 < 256 ? (int)(n - i0) : 256;
      for (int j = 0; j < m; ++j) acc += chunk[j];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(acc * inv_count);
}

// ---- backward, launch 1: frames[b, t, :] = the gradient of the windowed frame ----
__global__ __launch_bounds__(64 * WAVES) void melspec_bwd_frames_kernel(mel_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const lds_view v = carve(smem_raw, a, wave);
  const FftTable tab = fft_table(a.tables, N);
  load_tables(v, a, tab);
  float* gm = v.row;                                          // [nmel] gradient of the linear mel
  const float gs = a.g_logmel ? 0.f : a.gscale * a.gout[0];
  const int gpb = (a.T + WAVES - 1) / WAVES;
  // G[k] = g_mag[k] X[k] / |X[k]|, 0 where |X| = 0;  g_mag[k] = w_up[k] g_mel[s(k)] + w_dn[k] g_mel[s(k) - 1]
  auto grad_bin = [&](c32 X, int k) -> c32 {
    const int s = v.bin_seg[k];
    const float2 w = v.wud[k];
    float g = 0.f;
    if (s < a.nmel) g = w.x * gm[s];
    if (s >= 1) g += w.y * gm[s - 1];
    const float mg = sqrtf(X.x * X.x + X.y * X.y);
    const float r = mg > 0.f ? g / mg : 0.f;
    return {r * X.x, r * X.y};
  };
#pragma unroll 1
  for (int g = blockIdx.x; g < a.B * gpb; g += gridDim.x) {
    const int b = g / gpb, t = (g - b * gpb) * WAVES + wave;
    if (t >= a.T) continue;                                   // (wave-uniform)
    for (int m = lane; m < a.nmel; m += 64) {
      const int64_t idx = ((int64_t)b * a.nmel + m) * a.T + t;
      const float ml = a.mel[idx];
      float gl;
      if (a.g_logmel) {
        gl = a.g_logmel[idx];
      } else {
        const float d = a.logmel[idx] - a.tgt[idx];
        gl = d > 0.f ? gs : (d < 0.f ? -gs : 0.f);
      }
      gm[m] = ml >= a.eps ? gl / ml : 0.f;                    // clamp(min = eps): the gradient passes at a tie
    }
    load_frame(a, b, t, v.bx, tab.win, lane);
    c32* z = fft_forward<H>(v.bx, v.by, v.tw, lane);
    c32* y = z == v.bx ? v.by : v.bx;
    for (int k = lane; k <= H / 2; k += 64) {
      c32 xa, xb;
      unpack_pair<H>(z, tab.tf, k, xa, xb);
      const c32 ga = grad_bin(xa, k), gb = grad_bin(xb, H - k);
      if (k == 0) {                                           // bins 0 and N/2: real parts, not halved
        y[0] = pack_conj({2.f * ga.x, 0.f}, {2.f * gb.x, 0.f}, tab.tf[0]);
      } else if (k == H / 2) {
        y[k] = pack_conj(ga, ga, tab.tf[k]);
      } else {
        y[k] = pack_conj(ga, gb, tab.tf[k]);
        y[H - k] = pack_conj(gb, ga, tab.tf[H - k]);
      }
    }
    const c32* r = fft_forward<H>(y, z, v.tw, lane);
    float* fo = a.frames + ((int64_t)b * a.T + t) * N;
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
      const int n = lane + 64 * q;
      const c32 rv = r[n];
      const float2 wv = *reinterpret_cast<const float2*>(tab.win + 2 * n);
      *reinterpret_cast<float2*>(fo + 2 * n) = make_float2(rv.x * wv.x, -rv.y * wv.y);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- backward, launch 2: overlap-add and the adjoint of the reflect pad, one lane per sample ----
__global__ __launch_bounds__(256) void melspec_bwd_ola_kernel(int B, int64_t Nw, int T, int hop, int pad, const float* __restrict__ frames,
                                                              float* __restrict__ dwav) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * Nw) return;
  const int b = (int)(i / Nw);
  const int64_t j = i - (int64_t)b * Nw;
  const float* fr = frames + (int64_t)b * T * N;
  // padded positions that read sample j, ascending: the left mirror pad - j (1 <= j <= pad), j + pad itself, the right mirror
  // pad + 2 (Nw - 1) - j (Nw - 1 - pad <= j <= Nw - 2); for short rows both mirrors apply to the same sample
  int64_t pos[3];
  int np = 0;
  if (j >= 1 && j <= pad) pos[np++] = pad - j;
  pos[np++] = j + pad;
  if (j >= Nw - 1 - pad && j <= Nw - 2) pos[np++] = pad + 2 * (Nw - 1) - j;
  float acc = 0.f;
  for (int q = 0; q < np; ++q) {
    const int64_t p = pos[q];
    int t_lo, t_hi;
    ola_frame_range(p, N, hop, T, t_lo, t_hi);
    for (int t = t_lo; t <= t_hi; ++t) acc += fr[(int64_t)t * N + (p - (int64_t)t * hop)];     // 0 <= p - t hop < N by the range
  }
  dwav[i] = acc;
}

bool geometry_ok(int B, int64_t Nw, int T, int hop, int pad, int nmel) {
  return B > 0 && hop > 0 && pad >= 0 && nmel >= 1 && nmel <= 128 && Nw > pad && Nw + 2 * (int64_t)pad >= N &&
         T == (Nw + 2 * (int64_t)pad - N) / hop + 1 && (int64_t)B * T < (1ll << 31);
}

int launch_frames(bool bwd, const mel_args& a, hipStream_t st) {
  const size_t lds = lds_bytes(a.nmel);                       // 46 - 48 KB for n_mels <= 128: no limit to raise, three per CU
  S2S_REQUIRE(lds <= 64 * 1024 && fft_resident_groups(lds, 3) == 256 * 3, "melspec: the LDS layout no longer fits three workgroups per CU");
  const dim3 grid = fft_persistent_grid((int64_t)a.B * ((a.T + WAVES - 1) / WAVES), lds, 3);
  if (bwd) hipLaunchKernelGGL(melspec_bwd_frames_kernel, grid, dim3(64 * WAVES), lds, st, a);
  else hipLaunchKernelGGL(melspec_fwd_kernel, grid, dim3(64 * WAVES), lds, st, a);
  S2S_CHECK_LAUNCH(bwd ? "melspec_bwd_frames_kernel" : "melspec_fwd_kernel");
  return 0;
}

}  // namespace

extern "C" int s2svc_melspec_supported(int n_fft, int win_length, int nmel) {
  return n_fft == N && win_length == n_fft && nmel >= 1 && nmel <= 128;
}

extern "C" int s2svc_melspec_fwd(int B, int64_t Nw, int T, int hop, int pad, int nmel, const float* wav, const float* tables,
                                 const int32_t* seg_lo, const int32_t* seg_len, const float* wud, float eps, float* mel, float* logmel,
                                 const float* tgt, double* partials, void* stream) {
  S2S_REQUIRE(geometry_ok(B, Nw, T, hop, pad, nmel), "melspec_fwd: bad geometry (n_mels <= 128, N > pad, T = (N + 2 pad - 1024) / hop + 1)");
  S2S_REQUIRE(wav && tables && seg_lo && seg_len && wud && mel && logmel && ((uintptr_t)tables) % 8 == 0 && ((uintptr_t)wud) % 8 == 0 &&
              (tgt == nullptr) == (partials == nullptr) && ((uintptr_t)partials) % 8 == 0, "melspec_fwd: bad args");
  mel_args a = {};
  a.B = B; a.T = T; a.hop = hop; a.pad = pad; a.nmel = nmel; a.Nw = Nw; a.wav = wav; a.tables = tables; a.seg_lo = seg_lo;
  a.seg_len = seg_len; a.wud = wud; a.eps = eps; a.mel = mel; a.logmel = logmel; a.tgt = tgt; a.partials = partials;
  return launch_frames(false, a, (hipStream_t)stream);
}

extern "C" int s2svc_melspec_loss_finish(int64_t n, const double* partials, double inv_count, float* loss, void* stream) {
  S2S_REQUIRE(n > 0 && partials && loss && ((uintptr_t)partials) % 8 == 0, "melspec_loss_finish: bad args");
  hipLaunchKernelGGL(melspec_loss_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n, partials, inv_count, loss);
  S2S_CHECK_LAUNCH("melspec_loss_finish_kernel");
  return 0;
}

extern "C" int s2svc_melspec_bwd_frames(int B, int64_t Nw, int T, int hop, int pad, int nmel, const float* wav, const float* tables,
                                        const float* wud, const int32_t* bin_seg, float eps, const float* mel, const float* g_logmel,
                                        const float* logmel, const float* tgt, const float* gout, float gscale, float* frames,
                                        void* stream) {
  S2S_REQUIRE(geometry_ok(B, Nw, T, hop, pad, nmel), "melspec_bwd_frames: bad geometry (n_mels <= 128, N > pad, T = (N + 2 pad - 1024) / hop + 1)");
  S2S_REQUIRE(wav && tables && wud && bin_seg && mel && frames && ((uintptr_t)tables) % 8 == 0 && ((uintptr_t)wud) % 8 == 0 &&
              ((uintptr_t)frames) % 8 == 0 && (g_logmel || (logmel && tgt && gout)), "melspec_bwd_frames: bad args");
  mel_args a = {};
  a.B = B; a.T = T; a.hop = hop; a.pad = pad; a.nmel = nmel; a.Nw = Nw; a.wav = wav; a.tables = tables; a.wud = wud; a.bin_seg = bin_seg;
  a.eps = eps; a.mel = const_cast<float*>(mel); a.g_logmel = g_logmel; a.logmel = const_cast<float*>(logmel); a.tgt = tgt; a.gout = gout;
  a.gscale = gscale; a.frames = frames;
  return launch_frames(true, a, (hipStream_t)stream);
}

extern "C" int s2svc_melspec_bwd_ola(int B, int64_t Nw, int T, int hop, int pad, const float* frames, float* dwav, void* stream) {
  S2S_REQUIRE(geometry_ok(B, Nw, T, hop, pad, 1) && frames && dwav, "melspec_bwd_ola: bad args");
  const int64_t total = (int64_t)B * Nw;
  S2S_REQUIRE((total + 255) / 256 < (1ll << 31), "melspec_bwd_ola: too many samples for one launch");
  hipLaunchKernelGGL(melspec_bwd_ola_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, Nw, T, hop, pad,
                     frames, dwav);
  S2S_CHECK_LAUNCH("melspec_bwd_ola_kernel");
  return 0;
}
