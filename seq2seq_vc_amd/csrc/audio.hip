// Waveform conditioning on the GPU: batched polyphase resampling (torchaudio.functional.resample at its defaults) and silence trimming
// (librosa.effects.trim), for padded batches with per-row lengths.  fp32, inference only, no atomics; samples at or beyond lens[b]
// are never read; every output of a row depends on that row's own samples and on its own index only, so a batched row equals its
// B = 1 call bit for bit.
//
// reference: urhythmic/urhythmic_resample.py:27-31 (torchaudio.functional.resample), urhythmic/urhythmic_convert.py:160-171,
// urhythmic/urhythmic_encode.py:122-133, bin/preprocess.py:207-221 (librosa.effects.trim) and :250 (global_gain_scale).
//
// Resampler (resample_poly_kernel).  torchaudio evaluates y[q new + p] = sum_j taps[p][j] x[q orig + j - width] as a dense conv1d of
// 2 width + orig taps per output, of which only the <= Kb taps inside the Hann window differ from ~1e-35.  Here the table is banded:
// per phase p the first tap index first[p] and Kb taps, stored [k][p] so that lanes of consecutive phase read consecutive addresses.
// A workgroup owns RS_TILE consecutive outputs of one row, stages the input span they need into LDS (coalesced loads, zeros outside
// [0, lens[b])) and every lane accumulates its Kb products with fp32 FMA in ascending tap order.
//
// Trim.  trim_frames_kernel: one wavefront per centred frame, mean(x^2) as an ordered double sum (lane l adds samples l, l + 64, ..
// in order, then the lanes are added by a fixed butterfly).  trim_intervals_kernel: one wave per row: maximum of the row's frame
// powers, the threshold test max(amin^2, p_i) > max(amin^2, p_max) * 10^(-top_db / 10) in double, first and last non-silent frame
// -> (start, end).  wav_gather_rows_kernel moves every row's [start, end) to offset 0 of a fresh padded batch, times a gain.
#include "common.h"
#include "../../include/s2svc_hip.h"

namespace {

constexpr int RS_TILE = 1024;                     // outputs per workgroup: 4 per lane
constexpr int RS_THREADS = 256;
constexpr int RS_MAX_SPAN = 12288;                // floats of LDS (48 KiB) a workgroup may stage

__global__ __launch_bounds__(RS_THREADS) void resample_poly_kernel(int Nmax, int Mmax, int orig, int nw, int width, int Kb, int fmin, int fmax,
                                                                   int span, const float* __restrict__ wav, const int32_t* __restrict__ lens,
                                                                   const int32_t* __restrict__ out_lens, const float* __restrict__ taps,
                                                                   const int32_t* __restrict__ first, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int m0 = blockIdx.x * RS_TILE;             // Mmax <= INT32_MAX: m0 < Mmax fits
  int len = lens[b], olen = out_lens[b];
  len = len < 0 ? 0 : (len > Nmax ? Nmax : len);
  olen = olen < 0 ? 0 : (olen > Mmax ? Mmax : olen);
  float* y = out + (int64_t)b * Mmax;
  if (m0 >= olen) {                                // workgroup-uniform: nothing of the row is read
    for (int i = tid; i < RS_TILE && m0 + i < Mmax; i += RS_THREADS) y[m0 + i] = 0.f;
    return;
  }
  const float* x = wav + (int64_t)b * Nmax;
  const int q0 = m0 / nw;
  const int64_t s0 = (int64_t)q0 * orig - width + fmin;         // the first input sample any output of this tile can touch
  for (int i = tid; i < span; i += RS_THREADS) {
    const int64_t g = s0 + i;
    xs[i] = (g >= 0 && g < len) ? x[g] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < RS_TILE / RS_THREADS; ++u) {
    const int i = u * RS_THREADS + tid;
    if (i >= Mmax - m0) continue;                  // m0 + i without overflow
    const int m = m0 + i;
    float acc = 0.f;
    if (m < olen) {
      const int q = m / nw, p = m - q * nw;
      int f = first[p];
      f = f < fmin ? fmin : (f > fmax ? fmax : f);                // a table that lies cannot take the reads out of the staged span
      const float* xl = xs + (q - q0) * orig + (f - fmin);        // < span by the launcher's formula
      const float* tp = taps + p;
      for (int k = 0; k < Kb; ++k) acc = __builtin_fmaf(tp[(int64_t)k * nw], xl[k], acc);
    }
    y[m] = acc;
  }
}

// index of sample g of the row's reflect-padded extension (numpy's pad mode "reflect": period 2 (len - 1)); len >= 1
__device__ __forceinline__ int64_t reflect_index(int64_t g, int64_t len) {
  if (len == 1) return 0;
  const int64_t period = 2 * (len - 1);
  g %= period;
  if (g < 0) g += period;
  return g < len ? g : period - g;
}

__global__ __launch_bounds__(256) void trim_frames_kernel(int Nmax, int nfmax, int frame_length, int hop, int reflect,
                                                          const float* __restrict__ wav, const int32_t* __restrict__ lens,
                                                          double* __restrict__ power) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);             // wave-uniform
  if (i >= nfmax) return;
  int len = lens[b];
  len = len < 0 ? 0 : (len > Nmax ? Nmax : len);
  double* pw = power + (int64_t)b * nfmax;
  if (i > len / hop) {                                           // beyond the row's 1 + len / hop frames
    if (lane == 0) pw[i] = 0.0;
    return;
  }
  const float* x = wav + (int64_t)b * Nmax;
  const int64_t g0 = (int64_t)i * hop - frame_length / 2;
  double s = 0.0;
  for (int k = lane; k < frame_length; k += 64) {
    int64_t g = g0 + k;
    float v = 0.f;
    if (reflect) {
      if (len > 0) v = x[reflect_index(g, len)];
    } else if (g >= 0 && g < len) {
      v = x[g];
    }
    s += (double)v * (double)v;
  }
  s = wave_sum_d(s);
  if (lane == 0) pw[i] = s / (double)frame_length;
}

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(64) void trim_intervals_kernel(int Nmax, int nfmax, int hop, double amin, double ratio,
                                                            const int32_t* __restrict__ lens, const double* __restrict__ power,
                                                            int32_t* __restrict__ intervals) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int len = lens[b];
  len = len < 0 ? 0 : (len > Nmax ? Nmax : len);
  int nf = 1 + len / hop;
  nf = nf > nfmax ? nfmax : nf;
  const double* pw = power + (int64_t)b * nfmax;
  double mx = 0.0;                                               // powers are >= 0
  for (int i = lane; i < nf; i += 64) mx = fmax(mx, pw[i]);
  mx = wave_max_d(mx);
  const double thr = fmax(amin, mx) * ratio;
  int first = -1, last = -1;
  for (int c = 0; c < nf; c += 64) {                             // wave-uniform trip count
    const int i = c + lane;
    const bool loud = i < nf && fmax(amin, pw[i]) > thr;
    const uint64_t hit = __ballot(loud);
    if (hit) {
      if (first < 0) first = c + __builtin_ctzll(hit);
      last = c + 63 - __builtin_clzll(hit);
    }
  }
  if (lane == 0) {
    int64_t start = 0, end = 0;
    if (first >= 0) {
      start = (int64_t)first * hop;
      end = (int64_t)(last + 1) * hop;
      end = end > len ? len : end;
      start = start > end ? end : start;
    }
    intervals[2 * b] = (int32_t)start;
    intervals[2 * b + 1] = (int32_t)end;
  }
}

__global__ __launch_bounds__(256) void wav_gather_rows_kernel(int Nmax, int Mmax, float gain, const float* __restrict__ wav,
                                                              const int32_t* __restrict__ intervals, float* __restrict__ out) {
  const int b = blockIdx.y;
  int start = intervals[2 * b], end = intervals[2 * b + 1];
  start = start < 0 ? 0 : (start > Nmax ? Nmax : start);
  end = end < start ? start : (end > Nmax ? Nmax : end);
  const int n = end - start;
  const float* x = wav + (int64_t)b * Nmax + start;
  float* y = out + (int64_t)b * Mmax;
  const int i0 = blockIdx.x * RS_TILE;
#pragma unroll
  for (int u = 0; u < RS_TILE / 256; ++u) {
    const int i = u * 256 + (int)threadIdx.x;
    if (i >= Mmax - i0) continue;
    y[i0 + i] = i0 + i < n ? x[i0 + i] * gain : 0.f;
  }
}

}  // namespace

extern "C" int s2svc_resample_tile(void) { return RS_TILE; }
extern "C" int s2svc_resample_max_span(void) { return RS_MAX_SPAN; }

extern "C" int s2svc_resample_poly(int B, int Nmax, int Mmax, int orig, int new_, int width, int Kb, int fmin, int fmax, const float* wav,
                                   const int32_t* lens, const int32_t* out_lens, const float* taps, const int32_t* first, float* out,
                                   void* stream) {
  S2S_REQUIRE(B >= 0 && Nmax >= 0 && Mmax >= 0, "resample_poly: bad shape");
  S2S_REQUIRE(orig > 0 && new_ > 0 && width >= 0 && Kb > 0, "resample_poly: bad table shape");
  S2S_REQUIRE(fmin >= 0 && fmax >= fmin && fmax <= 2 * (int64_t)width + orig, "resample_poly: first tap indices outside [0, 2 width + orig]");
  S2S_REQUIRE(B <= 65535, "resample_poly: B > 65535 not supported");
  if (B == 0 || Mmax == 0) return 0;
  S2S_REQUIRE(wav || Nmax == 0, "resample_poly: null argument");
  S2S_REQUIRE(lens && out_lens && taps && first && out, "resample_poly: null argument");
  // outputs m0 .. m0 + TILE - 1 span at most (new + TILE - 2) / new + 1 values of q
  const int64_t span = ((int64_t)(new_ + RS_TILE - 2) / new_) * orig + (fmax - fmin) + Kb;
  S2S_REQUIRE(span <= RS_MAX_SPAN, "resample_poly: the input span of one workgroup exceeds 48 KiB of LDS (orig / new too large)");
  const dim3 grid((unsigned)(((int64_t)Mmax + RS_TILE - 1) / RS_TILE), B);
  hipLaunchKernelGGL(resample_poly_kernel, grid, dim3(RS_THREADS), (size_t)span * 4, (hipStream_t)stream, Nmax, Mmax, orig, new_, width, Kb,
                     fmin, fmax, (int)span, wav, lens, out_lens, taps, first, out);
  S2S_CHECK_LAUNCH("resample_poly_kernel");
  return 0;
}

extern "C" int s2svc_trim_frames(int B, int Nmax, int nfmax, int frame_length, int hop, int reflect, const float* wav, const int32_t* lens,
                                 double* power, void* stream) {
  S2S_REQUIRE(B >= 0 && Nmax >= 0 && nfmax > 0 && frame_length > 0 && hop > 0, "trim_frames: bad shape");
  S2S_REQUIRE(B <= 65535, "trim_frames: B > 65535 not supported");
  if (B == 0) return 0;
  S2S_REQUIRE((wav || Nmax == 0) && lens && power, "trim_frames: null argument");
  hipLaunchKernelGGL(trim_frames_kernel, dim3((nfmax + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, Nmax, nfmax, frame_length, hop,
                     reflect ? 1 : 0, wav, lens, power);
  S2S_CHECK_LAUNCH("trim_frames_kernel");
  return 0;
}

extern "C" int s2svc_trim_intervals(int B, int Nmax, int nfmax, int hop, double amin, double ratio, const int32_t* lens, const double* power,
                                    int32_t* intervals, void* stream) {
  S2S_REQUIRE(B >= 0 && Nmax >= 0 && nfmax > 0 && hop > 0, "trim_intervals: bad shape");
  if (B == 0) return 0;
  S2S_REQUIRE(lens && power && intervals, "trim_intervals: null argument");
  hipLaunchKernelGGL(trim_intervals_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, Nmax, nfmax, hop, amin, ratio, lens, power, intervals);
  S2S_CHECK_LAUNCH("trim_intervals_kernel");
  return 0;
}

extern "C" int s2svc_wav_gather_rows(int B, int Nmax, int Mmax, float gain, const float* wav, const int32_t* intervals, float* out,
                                     void* stream) {
  S2S_REQUIRE(B >= 0 && Nmax >= 0 && Mmax >= 0, "wav_gather_rows: bad shape");
  S2S_REQUIRE(B <= 65535, "wav_gather_rows: B > 65535 not supported");
  if (B == 0 || Mmax == 0) return 0;
  S2S_REQUIRE((wav || Nmax == 0) && intervals && out, "wav_gather_rows: null argument");
  hipLaunchKernelGGL(wav_gather_rows_kernel, dim3((unsigned)(((int64_t)Mmax + RS_TILE - 1) / RS_TILE), B), dim3(256), 0, (hipStream_t)stream,
                     Nmax, Mmax, gain, wav, intervals, out);
  S2S_CHECK_LAUNCH("wav_gather_rows_kernel");
  return 0;
}
