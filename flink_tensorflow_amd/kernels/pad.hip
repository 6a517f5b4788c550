// Two copy-class kernels of the generator networks (style transfer, CycleGAN / pix2pix).
//
//   pad_nhwc_bf16   y[n, i, j, :] = x[n, src(i - pt), src(j - pl), :] over the 8-channel vectors of
//       a bf16 NHWC tensor: TF's Pad / PadV2 (constant) and MirrorPad (REFLECT, SYMMETRIC) of the
//       two spatial axes, low and high pads independent per axis.  One thread per (output pixel,
//       channel vector), consecutive lanes on consecutive vectors of a pixel, a workgroup inside
//       one output row: one 16-byte load, one 16-byte store.  src of an index r outside [0, size):
//           reflect     r < 0: -r            r >= size: 2 (size - 1) - r     (pads <= size - 1)
//           symmetric   r < 0: -r - 1        r >= size: 2 size - 1 - r       (pads <= size)
//           constant    no source: the load is predicated off and the vector is the fill value
//       so every address read is inside x without a clamp.  x may be channel-padded (pitch ldx,
//       CV physical vectors, Cl logical channels): physical vectors are copied, so a mirror of zero
//       pad channels is zero, and a constant fill writes the value to the Cl logical channels and
//       zero behind them.  The result goes to channel offset y_coff of a pixel of pitch ldy (a
//       concat slot, or a plain buffer with y_coff = 0).  Offsets are 64-bit.
//
//   image_out_bf16  the output stage of a generator: out[p, c] = clamp(act(x[p, c]) * a + b, lo, hi)
//       for the Cl = 1, 3 or 4 logical channels of a bf16 buffer of pixel pitch ldx, written
//       compactly as fp32 or uint8 [pixels, Cl].  act is none / tanh / sigmoid.  Every operation
//       is fp32 and rounded on its own (no fma), as TF's Tanh -> Mul -> Add -> ClipByValue
//       computes it; the uint8 form truncates after the clamp (TF's Cast), which the launcher only
//       allows for 0 <= lo <= hi <= 255.  One thread owns 4 consecutive pixels: one 8-byte load
//       per pixel, and the 4 Cl results leave as Cl dwords (uint8; an RGB row needs no byte
//       stores, as in jpeg_idct_rgb) or Cl 16-byte vectors (fp32).  The last 1..3 pixels of the
//       tensor are stored element by element.
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace {

enum PadMode : int { PAD_CONSTANT = 0, PAD_REFLECT = 1, PAD_SYMMETRIC = 2 };

struct PadParams {
  int N, H, W, CV, Cl, Ho, Wo, ldx, ldy, y_coff, pt, pl;
  float value;
};

// source index of r = (output index - low pad) on an axis of `size`; -1: none (constant mode)
template <int MODE>
FTM_DEVICE int pad_src(int r, int size) {
  if (r >= 0 && r < size) return r;
  if constexpr (MODE == PAD_REFLECT) return r < 0 ? -r : 2 * (size - 1) - r;
  else if constexpr (MODE == PAD_SYMMETRIC) return r < 0 ? -r - 1 : 2 * size - 1 - r;
  else return -1;
}

// grid.x = N * Ho output rows, grid.y = blocks of 256 vectors of a row: the row's (n, oy) are
// uniform per workgroup (scalar), a thread divides one 32-bit index by CV, and only the row bases
// are 64-bit
template <int MODE>
__global__ __launch_bounds__(256) void pad_nhwc_kernel(const bf16* __restrict__ x, bf16* __restrict__ y,
                                                       const PadParams q) {
  const unsigned t = blockIdx.y * 256u + threadIdx.x;
  if (t >= (unsigned)q.Wo * (unsigned)q.CV) return;
  const int ox = (int)(t / (unsigned)q.CV);
  const int cv = (int)(t - (unsigned)ox * (unsigned)q.CV);
  const unsigned row = blockIdx.x;
  const int oy = (int)(row % (unsigned)q.Ho);
  const size_t n = row / (unsigned)q.Ho;
  const int iy = pad_src<MODE>(oy - q.pt, q.H), ix = pad_src<MODE>(ox - q.pl, q.W);
  bf16x8 v;
  if (MODE != PAD_CONSTANT || (iy >= 0 && ix >= 0)) {
    v = *reinterpret_cast<const bf16x8*>(x + ((n * q.H + iy) * q.W + ix) * q.ldx + (size_t)cv * 8);
  } else {
    const bf16 fill = f2bf(q.value), zero = f2bf(0.f);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = cv * 8 + e < q.Cl ? fill : zero;
  }
  *reinterpret_cast<bf16x8*>(y + ((size_t)row * q.Wo + ox) * q.ldy + q.y_coff + (size_t)cv * 8) = v;
}

enum ImgAct : int { IMG_NONE = 0, IMG_TANH = 1, IMG_SIGMOID = 2 };

struct ImgParams {
  long pixels;
  int ldx, clamp;
  float a, b, lo, hi;
};

template <int ACT>
FTM_DEVICE float img_value(float v, const ImgParams& q) {
#pragma clang fp contract(off)
  if constexpr (ACT == IMG_TANH) v = tanhf(v);
  else if constexpr (ACT == IMG_SIGMOID) v = 1.f / (1.f + expf(-v));
  v = v * q.a;
  v = v + q.b;
  if (q.clamp) v = fminf(fmaxf(v, q.lo), q.hi);
  return v;
}

template <typename T>
FTM_DEVICE T img_cast(float v) {
  return (T)v;  // uint8: truncation of a value the clamp keeps inside [0, 255]
}

template <int CL, int ACT, typename T>
__global__ __launch_bounds__(256) void image_out_kernel(const bf16* __restrict__ x, T* __restrict__ out,
                                                        const ImgParams q) {
  const long quads = (q.pixels + 3) / 4;
  const long step = (long)gridDim.x * blockDim.x;
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < quads; g += step) {
    const long p0 = g * 4;
    const int np = q.pixels - p0 < 4 ? (int)(q.pixels - p0) : 4;
    float v[4 * CL];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < np) {
        const bf16x4 u = *reinterpret_cast<const bf16x4*>(x + (size_t)(p0 + k) * q.ldx);
#pragma unroll
        for (int c = 0; c < CL; ++c) v[k * CL + c] = img_value<ACT>(bf2f(u[c]), q);
      } else {
#pragma unroll
        for (int c = 0; c < CL; ++c) v[k * CL + c] = 0.f;
      }
    }
    T* o = out + (size_t)p0 * CL;
    if (np == 4) {
      if constexpr (sizeof(T) == 1) {
        uint32_t w[CL];
#pragma unroll
        for (int d = 0; d < CL; ++d) {
          w[d] = (uint32_t)img_cast<T>(v[4 * d]) | (uint32_t)img_cast<T>(v[4 * d + 1]) << 8 |
                 (uint32_t)img_cast<T>(v[4 * d + 2]) << 16 | (uint32_t)img_cast<T>(v[4 * d + 3]) << 24;
        }
#pragma unroll
        for (int d = 0; d < CL; ++d) reinterpret_cast<uint32_t*>(o)[d] = w[d];
      } else {
#pragma unroll
        for (int d = 0; d < CL; ++d) {
          f32x4 w;
#pragma unroll
          for (int e = 0; e < 4; ++e) w[e] = v[4 * d + e];
          reinterpret_cast<f32x4*>(o)[d] = w;
        }
      }
    } else {
      for (int e = 0; e < np * CL; ++e) o[e] = img_cast<T>(v[e]);
    }
  }
}

template <int CL, typename T>
void launch_image_out(const bf16* X, T* O, const ImgParams& q, int act, hipStream_t s) {
  long g = ((q.pixels + 3) / 4 + 255) / 256;
  g = g > 2048 * 8 ? 2048 * 8 : g;
  const dim3 grid((unsigned)g), block(256);
  if (act == IMG_TANH) hipLaunchKernelGGL((image_out_kernel<CL, IMG_TANH, T>), grid, block, 0, s, X, O, q);
  else if (act == IMG_SIGMOID) hipLaunchKernelGGL((image_out_kernel<CL, IMG_SIGMOID, T>), grid, block, 0, s, X, O, q);
  else hipLaunchKernelGGL((image_out_kernel<CL, IMG_NONE, T>), grid, block, 0, s, X, O, q);
}

template <typename T>
void launch_image_out_cl(const bf16* X, T* O, const ImgParams& q, int cl, int act, hipStream_t s) {
  if (cl == 1) launch_image_out<1, T>(X, O, q, act, s);
  else if (cl == 3) launch_image_out<3, T>(X, O, q, act, s);
  else launch_image_out<4, T>(X, O, q, act, s);
}

}  // namespace

// pads = (top, bottom, left, right); C = physical channels copied (a multiple of 8), Cl <= C the
// logical ones (they differ only in what a constant fill writes)
void pad_nhwc_bf16(uintptr_t x, uintptr_t y, int N, int H, int W, int C, int Cl, int pt, int pb, int pl, int pr,
                   int mode, float value, int ldx, int ldy, int y_coff, uintptr_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) throw std::invalid_argument("pad_nhwc: empty problem");
  if (C % 8 || ldx % 8 || ldy % 8 || y_coff % 8)
    throw std::invalid_argument("pad_nhwc: C, ldx, ldy, y_coff must be multiples of 8");
  if (Cl < 1 || Cl > C || ldx < C || y_coff < 0 || y_coff + C > ldy)
    throw std::invalid_argument("pad_nhwc: channel slot exceeds the row");
  if (x % 16 || y % 16) throw std::invalid_argument("pad_nhwc: pointers must be 16-byte aligned");
  if (pt < 0 || pb < 0 || pl < 0 || pr < 0) throw std::invalid_argument("pad_nhwc: negative pad");
  if (mode < PAD_CONSTANT || mode > PAD_SYMMETRIC) throw std::invalid_argument("pad_nhwc: mode must be 0..2");
  const int lim_h = mode == PAD_REFLECT ? H - 1 : H, lim_w = mode == PAD_REFLECT ? W - 1 : W;
  if (mode != PAD_CONSTANT && (pt > lim_h || pb > lim_h || pl > lim_w || pr > lim_w))
    throw std::invalid_argument("pad_nhwc: a mirror pad exceeds the axis");
  const long Ho = (long)H + pt + pb, Wo = (long)W + pl + pr;
  if (Ho > 0x7fffffffL || Wo > 0x7fffffffL) throw std::invalid_argument("pad_nhwc: output too large");
  const PadParams q{N, H, W, C / 8, Cl, (int)Ho, (int)Wo, ldx, ldy, y_coff, pt, pl, value};
  const long rows = (long)N * Ho, per_row = Wo * (long)(C / 8);
  if (rows > 0x7fffffffL || (per_row + 255) / 256 > 65535)
    throw std::invalid_argument("pad_nhwc: grid too large");
  auto s = reinterpret_cast<hipStream_t>(stream);
  auto X = reinterpret_cast<const bf16*>(x);
  auto Y = reinterpret_cast<bf16*>(y);
  const dim3 grid((unsigned)rows, (unsigned)((per_row + 255) / 256)), block(256);
  if (mode == PAD_REFLECT) hipLaunchKernelGGL(pad_nhwc_kernel<PAD_REFLECT>, grid, block, 0, s, X, Y, q);
  else if (mode == PAD_SYMMETRIC) hipLaunchKernelGGL(pad_nhwc_kernel<PAD_SYMMETRIC>, grid, block, 0, s, X, Y, q);
  else hipLaunchKernelGGL(pad_nhwc_kernel<PAD_CONSTANT>, grid, block, 0, s, X, Y, q);
  FTM_CHECK_LAUNCH();
}

// out_bytes: 1 (uint8, needs the clamp inside [0, 255]) or 4 (fp32)
void image_out_bf16(uintptr_t x, uintptr_t out, long pixels, int ldx, int cl, int act, float a, float b, bool clamp,
                    float lo, float hi, int out_bytes, uintptr_t stream) {
  if (pixels <= 0) throw std::invalid_argument("image_out: empty problem");
  if (cl != 1 && cl != 3 && cl != 4) throw std::invalid_argument("image_out: channels must be 1, 3 or 4");
  if (ldx % 8 || ldx < cl) throw std::invalid_argument("image_out: ldx must be a multiple of 8 and at least channels");
  if (act < IMG_NONE || act > IMG_SIGMOID) throw std::invalid_argument("image_out: act must be 0..2");
  if (out_bytes != 1 && out_bytes != 4) throw std::invalid_argument("image_out: out_bytes must be 1 or 4");
  if (clamp && !(lo <= hi)) throw std::invalid_argument("image_out: empty clamp range");
  if (out_bytes == 1 && !(clamp && lo >= 0.f && hi <= 255.f))
    throw std::invalid_argument("image_out: uint8 output needs a clamp inside [0, 255]");
  if (x % 16 || out % (out_bytes == 1 ? 4 : 16)) throw std::invalid_argument("image_out: misaligned pointer");
  const ImgParams q{pixels, ldx, clamp ? 1 : 0, a, b, lo, hi};
  auto s = reinterpret_cast<hipStream_t>(stream);
  auto X = reinterpret_cast<const bf16*>(x);
  if (out_bytes == 1) launch_image_out_cl<uint8_t>(X, reinterpret_cast<uint8_t*>(out), q, cl, act, s);
  else launch_image_out_cl<float>(X, reinterpret_cast<float*>(out), q, cl, act, s);
  FTM_CHECK_LAUNCH();
}

void register_pad(pybind11::module_& m) {
  m.def("pad_nhwc_bf16", &pad_nhwc_bf16);
  m.def("image_out_bf16", &image_out_bf16);
}
