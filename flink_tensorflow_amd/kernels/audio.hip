// Audio front end (TF AudioSpectrogram + Mfcc): one launch takes PCM to coefficients, with
// the frames, the spectrogram and the mel energies in LDS only.
//
//   frame f of clip b = samples [f stride, f stride + window) times the periodic Hann window,
//                       zero-padded to N (the FFT length, a power of two in 256..2048)
//   P[k]   = |DFT_N(frame)[k]|^2,  k = 0 .. N/2                       (the spectrogram)
//   mel[c] = sum over the channel's bins, ascending, of sqrt(P[i]) w   (mfcc_tables)
//   out[d] = sum_j dct[d][j] log(max(mel[j], 1e-12))
//
// A 256-thread workgroup owns FPW = 8 consecutive frames of one clip.  They are packed in
// pairs: frame 2s is the real part and frame 2s + 1 the imaginary part of complex FFT s (four
// FFTs per workgroup, one per wave when N = 512), separated afterwards by conjugate symmetry:
//
//   X1[k] = (Z[k] + conj(Z[N-k])) / 2      X2[k] = (Z[k] - conj(Z[N-k])) / 2i
//
// The last frame of an odd count rides alone (imaginary part zero).  LDS holds, per FFT, re[N]
// and im[N] as separate fp32 arrays (consecutive lanes hit consecutive banks): 8 N floats per
// workgroup, 16 KiB at N = 512 and 64 KiB at N = 2048.  The FFT is radix-2 decimation in time:
// the windowed samples are stored at their bit-reversed index, then log2 N butterfly passes
// run in place, every pass behind a workgroup barrier (no lockstep assumption).  The thread
// that separates bin k owns the pair {k, N-k} of its FFT alone, so the powers overwrite the
// transform in place: frame 2s at re[0 .. N/2], frame 2s + 1 at im[0 .. N/2].  That leaves
// frame fi of the workgroup at lds[fi N ..].  The mel sums are held in registers across a
// barrier and their logs then overwrite the head of the same rows.
//
// Every table is fp32, built on the host in float64: hann[window], twiddle[N/2] = exp(-2 pi i
// k / N) as (cos, -sin) pairs, chan[C] = (lo, mid, hi) bin ranges, wb[bins] (the weight of bin
// i in channel band(i) + 1, read over [lo, mid)) and wa[bins] (its weight in channel band(i),
// read over [mid, hi)), dct[D][C].  No device sin / cos; sqrtf and logf, not the fast forms.
// Each channel sums its bins in ascending order in one thread: no atomics, same bits on every
// launch.
//
//   in    fp32 or int16 (times `scale`), sample s of clip b at in[b clip_stride + s sample_stride]
//   mode  0 MFCC fp32 [B, F, D]      1 MFCC bf16 [B, F, D]
//         2 MFCC bf16 [B, F, D, 8]: channel 0, channels 1..7 zero (one 16-byte store)
//         3 spectrogram fp32 [B, F, N/2 + 1], squared       4 the same, square root
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace {

constexpr int kFramesPerWg = 8;
constexpr int kThreads = 256;
constexpr int kMaxChannels = 128;
constexpr int kMelPerThread = kFramesPerWg * kMaxChannels / kThreads;  // 4

enum AudioMode : int { MFCC_F32 = 0, MFCC_BF16 = 1, MFCC_BF16_PAD8 = 2, SPEC_SQUARED = 3, SPEC_MAGNITUDE = 4 };

struct AudioParams {
  const void* in;
  const float* hann;
  const float* twiddle;
  const int* chan;
  const float* wa;
  const float* wb;
  const float* dct;
  void* out;
  long sample_stride, clip_stride;
  int B, F, window, stride, log2n, C, D, mode, in_i16;
  float scale;
};

template <bool I16>
FTM_DEVICE float load_sample(const AudioParams& p, long off) {
  if constexpr (I16) return (float)reinterpret_cast<const int16_t*>(p.in)[off] * p.scale;
  else return reinterpret_cast<const float*>(p.in)[off];
}

template <bool I16>
__global__ __launch_bounds__(kThreads) void audio_frontend_kernel(const AudioParams p) {
  extern __shared__ float lds[];  // [4 FFTs][re N | im N]
  const int tid = threadIdx.x;
  const int N = 1 << p.log2n, half_n = N >> 1, bins = half_n + 1;
  const int groups = (p.F + kFramesPerWg - 1) / kFramesPerWg;
  const int b = blockIdx.x / groups;
  const int f_base = (blockIdx.x % groups) * kFramesPerWg;
  const int nframes = min(kFramesPerWg, p.F - f_base);  // >= 1

  // ---- windowed frames, at their bit-reversed positions; rows past nframes are zero
  for (int idx = tid; idx < kFramesPerWg * N; idx += kThreads) {
    const int fi = idx >> p.log2n, n = idx & (N - 1);
    float v = 0.f;
    if (fi < nframes && n < p.window) {
      const long s = (long)(f_base + fi) * p.stride + n;  // < S: the frame lies inside the clip
      v = load_sample<I16>(p, (long)b * p.clip_stride + s * p.sample_stride) * p.hann[n];
    }
    const int r = (int)(__brev((unsigned)n) >> (32 - p.log2n));
    lds[fi * N + r] = v;
  }
  __syncthreads();

  // ---- four N-point complex FFTs, radix 2, in place
  for (int pass = 0; pass < p.log2n; ++pass) {
    const int half = 1 << pass;
    const int tw_shift = p.log2n - 1 - pass;
    for (int idx = tid; idx < 4 * half_n; idx += kThreads) {
      const int s = idx / half_n, j = idx - s * half_n;
      if (2 * s >= nframes) continue;
      const int pos = j & (half - 1);
      const int i0 = ((j >> pass) << (pass + 1)) + pos, i1 = i0 + half;
      float* re = lds + s * 2 * N;
      float* im = re + N;
      const float wr = p.twiddle[2 * (pos << tw_shift)], wi = p.twiddle[2 * (pos << tw_shift) + 1];
      const float ar = re[i0], ai = im[i0], br = re[i1], bi = im[i1];
      const float tr = br * wr - bi * wi, ti = br * wi + bi * wr;
      re[i0] = ar + tr, im[i0] = ai + ti;
      re[i1] = ar - tr, im[i1] = ai - ti;
    }
    __syncthreads();
  }

  // ---- separate the two frames of each FFT; powers (or magnitudes) overwrite the transform
  const bool root = p.mode != SPEC_SQUARED;
  for (int idx = tid; idx < 4 * bins; idx += kThreads) {
    const int s = idx / bins, k = idx - s * bins;
    if (2 * s >= nframes) continue;
    float* re = lds + s * 2 * N;
    float* im = re + N;
    const int kk = (N - k) & (N - 1);
    const float zr = re[k], zi = im[k], yr = re[kk], yi = im[kk];
    const float x1r = 0.5f * (zr + yr), x1i = 0.5f * (zi - yi);
    const float x2r = 0.5f * (zi + yi), x2i = 0.5f * (yr - zr);
    float p1 = x1r * x1r + x1i * x1i, p2 = x2r * x2r + x2i * x2i;
    if (root) p1 = sqrtf(p1), p2 = sqrtf(p2);
    re[k] = p1, im[k] = p2;  // {k, N-k} belong to this thread alone
  }
  __syncthreads();

  if (p.mode >= SPEC_SQUARED) {
    float* out = reinterpret_cast<float*>(p.out) + ((long)b * p.F + f_base) * bins;
    for (int idx = tid; idx < nframes * bins; idx += kThreads) {
      const int fi = idx / bins, k = idx - fi * bins;
      out[idx] = lds[fi * N + k];
    }
    return;
  }

  // ---- mel filter bank: one thread per (frame, channel), bins in ascending order
  float mel[kMelPerThread];
#pragma unroll
  for (int it = 0; it < kMelPerThread; ++it) {
    const int item = tid + it * kThreads;
    const int fi = item / p.C, c = item - fi * p.C;
    float acc = 0.f;
    if (fi < nframes) {
      const float* v = lds + fi * N;
      // clamped to the row: a malformed table gives wrong numbers, never a read outside wa / wb
      const int lo = min(max(p.chan[3 * c], 0), bins), mid = min(max(p.chan[3 * c + 1], lo), bins);
      const int hi = min(max(p.chan[3 * c + 2], mid), bins);
      for (int i = lo; i < mid; ++i) acc += v[i] * p.wb[i];
      for (int i = mid; i < hi; ++i) acc += v[i] * p.wa[i];
    }
    mel[it] = acc;
  }
  __syncthreads();  // every magnitude has been read: the rows may be overwritten
#pragma unroll
  for (int it = 0; it < kMelPerThread; ++it) {
    const int item = tid + it * kThreads;
    const int fi = item / p.C, c = item - fi * p.C;
    if (fi < nframes) lds[fi * N + c] = logf(fmaxf(mel[it], 1e-12f));
  }
  __syncthreads();

  // ---- DCT-II and the store
  for (int item = tid; item < nframes * p.D; item += kThreads) {
    const int fi = item / p.D, d = item - fi * p.D;
    const float* lm = lds + fi * N;
    const float* row = p.dct + d * p.C;
    float acc = 0.f;
    for (int j = 0; j < p.C; ++j) acc += row[j] * lm[j];
    const long o = ((long)b * p.F + f_base + fi) * p.D + d;
    if (p.mode == MFCC_F32) reinterpret_cast<float*>(p.out)[o] = acc;
    else if (p.mode == MFCC_BF16) reinterpret_cast<bf16*>(p.out)[o] = f2bf(acc);
    else {
      bf16x8 px = {};
      px[0] = f2bf(acc);
      reinterpret_cast<bf16x8*>(p.out)[o] = px;
    }
  }
}

}  // namespace

// Strides are in elements of the input type.  `samples` is the clip length the strides were
// made for; the tables are those of mfcc_tables (chan / wa / wb / dct may be 0 in the
// spectrogram modes).
void audio_frontend(uintptr_t in, int in_i16, float scale, long sample_stride, long clip_stride, long samples, int B,
                    int window, int stride, int fft_len, uintptr_t hann, uintptr_t twiddle, uintptr_t chan, uintptr_t wa,
                    uintptr_t wb, uintptr_t dct, int C, int D, uintptr_t out, int mode, uintptr_t stream) {
  if (fft_len != 256 && fft_len != 512 && fft_len != 1024 && fft_len != 2048)
    throw std::invalid_argument("audio: the FFT length must be 256, 512, 1024 or 2048");
  if (window > fft_len || 2 * window <= fft_len || stride < 1)
    throw std::invalid_argument("audio: window must be in (N/2, N] and stride >= 1");
  if (B < 1 || samples < window) throw std::invalid_argument("audio: empty problem");
  if (sample_stride < 1 || clip_stride < 1) throw std::invalid_argument("audio: strides must be positive");
  if (mode < MFCC_F32 || mode > SPEC_MAGNITUDE) throw std::invalid_argument("audio: unknown output mode");
  if (!in || !hann || !twiddle || !out) throw std::invalid_argument("audio: null operand");
  if (in % (in_i16 ? 2 : 4) || hann % 4 || twiddle % 4 || out % (mode == MFCC_BF16_PAD8 ? 16 : mode == MFCC_BF16 ? 2 : 4))
    throw std::invalid_argument("audio: misaligned operand");
  if (mode < SPEC_SQUARED) {
    if (!chan || !wa || !wb || !dct || chan % 4 || wa % 4 || wb % 4 || dct % 4)
      throw std::invalid_argument("audio: the MFCC modes need the filter-bank and DCT tables");
    if (C < 1 || C > kMaxChannels || D < 1 || D > C) throw std::invalid_argument("audio: 1 <= D <= C <= 128");
  }
  const long F = 1 + (samples - window) / stride;
  const long wgs = (long)B * ((F + kFramesPerWg - 1) / kFramesPerWg);
  if (F > (1L << 24) || wgs > 0x7fffffffL) throw std::invalid_argument("audio: too many frames");
  AudioParams p;
  p.in = reinterpret_cast<const void*>(in);
  p.hann = reinterpret_cast<const float*>(hann);
  p.twiddle = reinterpret_cast<const float*>(twiddle);
  p.chan = reinterpret_cast<const int*>(chan);
  p.wa = reinterpret_cast<const float*>(wa);
  p.wb = reinterpret_cast<const float*>(wb);
  p.dct = reinterpret_cast<const float*>(dct);
  p.out = reinterpret_cast<void*>(out);
  p.sample_stride = sample_stride, p.clip_stride = clip_stride;
  p.B = B, p.F = (int)F, p.window = window, p.stride = stride, p.C = C, p.D = D, p.mode = mode, p.in_i16 = in_i16;
  p.log2n = fft_len == 256 ? 8 : fft_len == 512 ? 9 : fft_len == 1024 ? 10 : 11;
  p.scale = scale;
  const size_t shmem = (size_t)kFramesPerWg * fft_len * sizeof(float);
  auto s = reinterpret_cast<hipStream_t>(stream);
  if (in_i16) hipLaunchKernelGGL(audio_frontend_kernel<true>, dim3((unsigned)wgs), dim3(kThreads), shmem, s, p);
  else hipLaunchKernelGGL(audio_frontend_kernel<false>, dim3((unsigned)wgs), dim3(kThreads), shmem, s, p);
  FTM_CHECK_LAUNCH();
}

void register_audio(pybind11::module_& m) { m.def("audio_frontend", &audio_frontend); }
