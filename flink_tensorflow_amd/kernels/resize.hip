// Bilinear resize of bf16 NHWC activations, and the same resize fused with a channel ArgMax
// (semantic segmentation: DeepLab's ASPP image-pooling broadcast and its logits upsample).
// Both are bound by memory or instruction issue: there is no reduction an MFMA could take.
//
//   resize_bilinear_nhwc_bf16  x [N, H, W, C] bf16, pixel pitch ldx  ->  out [N, Ho, Wo, C] bf16
//       at channel offset y_coff of a row of pitch ldy (a concat slot).  One thread per (output
//       pixel, 8-channel vector): four 16-byte corner loads, fp32 lerps, one rounding, one
//       16-byte store; consecutive lanes take consecutive channel vectors of a pixel.
//   resize_argmax_nhwc_bf16    logits x [N, H, W, C] bf16 (C <= 256, pixel pitch ldx, the columns
//       C .. ldx-1 are padding and never compared)  ->  out [N, Ho, Wo] uint8 / int32 / int64:
//       the channel of the largest interpolated value.  Values are interpolated and compared
//       in fp32 (nothing is rounded to bf16 in between), ties go to the lowest channel.  With
//       Ho == H and Wo == W every lerp weight is 0: a plain channel ArgMax.
//
// Coordinates are TF's ResizeBilinear as graph/ops_nn.py:resize_bilinear_tf computes them: an
// fp32 scale (the quotient rounded from double), src = dst * scale or (dst + 0.5) * scale -
// 0.5 with every operation rounded to fp32 (contraction is off in coord()), floor, the low
// corner clamped to [0, size-1], the high one to size-1, the weight clipped to [0, 1].  Corner
// indices are clamped, so no address is ever outside x.
//
// The ArgMax has two kernels:
//   staged  (an upsample whose window fits): a workgroup owns a 16 x 64 tile of output
//       pixels, copies the input window the tile touches (tile * scale + 2 pixels per axis) to
//       LDS once and every thread walks the channels of its 4 consecutive pixels from there,
//       so an input pixel is not fetched from L2 scale^2 times.  A thread's 4 pixels start at
//       a 4-byte aligned output address, so a uint8 result is one dword store.
//   simple  (a downsample, or a window that does not fit the LDS budget): one thread per
//       output pixel, the four corners read from global memory.
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace {

struct RsParams {
  int N, H, W, C, Ho, Wo, ldx, ldy, y_coff;
  float sy, sx;
  int half_pixel;
};

struct Coord {
  int i0, i1;
  float w;
};

// source coordinate of output index o along an axis of `size` input pixels
FTM_DEVICE Coord coord(int o, float scale, int half_pixel, int size) {
#pragma clang fp contract(off)
  float f;
  if (half_pixel) {
    const float t = ((float)o + 0.5f) * scale;
    f = t - 0.5f;
  } else {
    f = (float)o * scale;
  }
  const float fl = floorf(f);
  int i0 = (int)fl;
  i0 = i0 < 0 ? 0 : i0;
  float w = half_pixel ? f - (float)i0 : f - fl;
  w = fminf(fmaxf(w, 0.f), 1.f);
  Coord c;
  c.i0 = i0 > size - 1 ? size - 1 : i0;
  c.i1 = i0 + 1 > size - 1 ? size - 1 : i0 + 1;
  c.w = w;
  return c;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// 8 bf16 -> 4 float pairs: a bf16 is the high half of its fp32, so one shift or one mask per
// element; the pairs feed v_pk_mul_f32 / v_pk_fma_f32
FTM_DEVICE void unpack8(const bf16x8 v, f32x2 (&f)[4]) {
  const u32x4 u = __builtin_bit_cast(u32x4, v);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[i][0] = __builtin_bit_cast(float, u[i] << 16);
    f[i][1] = __builtin_bit_cast(float, u[i] & 0xffff0000u);
  }
}

// the four corners of 8 channels, interpolated as resize_bilinear_tf does: along x, then y
FTM_DEVICE void lerp8(const bf16x8 tl, const bf16x8 tr, const bf16x8 bl, const bf16x8 br, float wx, float wy,
                      float (&v)[8]) {
  f32x2 a[4], b[4], c[4], d[4];
  unpack8(tl, a);
  unpack8(tr, b);
  unpack8(bl, c);
  unpack8(br, d);
  const float ux = 1.f - wx, uy = 1.f - wy;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 top = a[i] * ux + b[i] * wx;
    const f32x2 bot = c[i] * ux + d[i] * wx;
    const f32x2 r = top * uy + bot * wy;
    v[2 * i] = r[0];
    v[2 * i + 1] = r[1];
  }
}

__global__ __launch_bounds__(256) void resize_bilinear_kernel(const bf16* __restrict__ x, bf16* __restrict__ y,
                                                              const RsParams q) {
  const unsigned cchunks = q.C / 8;
  const unsigned total = (unsigned)q.N * q.Ho * q.Wo * cchunks;  // < 2^31: the launcher checks
  for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % cchunks) * 8;
    unsigned r = idx / cchunks;
    const int ox = (int)(r % q.Wo);
    r /= q.Wo;
    const int oy = (int)(r % q.Ho);
    const int n = (int)(r / q.Ho);
    const Coord cy = coord(oy, q.sy, q.half_pixel, q.H), cx = coord(ox, q.sx, q.half_pixel, q.W);
    const bf16* r0 = x + ((size_t)n * q.H + cy.i0) * q.W * q.ldx + c0;
    const bf16* r1 = x + ((size_t)n * q.H + cy.i1) * q.W * q.ldx + c0;
    const size_t o0 = (size_t)cx.i0 * q.ldx, o1 = (size_t)cx.i1 * q.ldx;
    float v[8];
    lerp8(*reinterpret_cast<const bf16x8*>(r0 + o0), *reinterpret_cast<const bf16x8*>(r0 + o1),
          *reinterpret_cast<const bf16x8*>(r1 + o0), *reinterpret_cast<const bf16x8*>(r1 + o1), cx.w, cy.w, v);
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(v[e]);
    *reinterpret_cast<bf16x8*>(y + (((size_t)n * q.Ho + oy) * q.Wo + ox) * q.ldy + q.y_coff + c0) = o;
  }
}

// Channel of the largest interpolated value of one output pixel.  p00 .. p11 point at channel 0
// of the four corners (LDS or global; 16-byte aligned, at least ceil8(C) channels readable).
FTM_DEVICE int argmax_pixel(const bf16* p00, const bf16* p01, const bf16* p10, const bf16* p11, float wx, float wy,
                            int C) {
  // strictly greater: a tie keeps the lower channel (all -inf: channel 0)
  float best = -__builtin_inff();
  int arg = 0;
  int c0 = 0;
  for (; c0 + 8 <= C; c0 += 8) {
    float v[8];
    lerp8(*reinterpret_cast<const bf16x8*>(p00 + c0), *reinterpret_cast<const bf16x8*>(p01 + c0),
          *reinterpret_cast<const bf16x8*>(p10 + c0), *reinterpret_cast<const bf16x8*>(p11 + c0), wx, wy, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (v[e] > best) {
        best = v[e];
        arg = c0 + e;
      }
    }
  }
  if (c0 < C) {  // the last, partial vector: its padding channels never compete
    float v[8];
    lerp8(*reinterpret_cast<const bf16x8*>(p00 + c0), *reinterpret_cast<const bf16x8*>(p01 + c0),
          *reinterpret_cast<const bf16x8*>(p10 + c0), *reinterpret_cast<const bf16x8*>(p11 + c0), wx, wy, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (c0 + e < C && v[e] > best) {
        best = v[e];
        arg = c0 + e;
      }
    }
  }
  return arg;
}

template <typename T>
FTM_DEVICE void store_label(T* out, size_t i, int v) {
  out[i] = (T)v;
}

template <typename T>
__global__ __launch_bounds__(256) void argmax_simple_kernel(const bf16* __restrict__ x, T* __restrict__ out,
                                                            const RsParams q) {
  const unsigned total = (unsigned)q.N * q.Ho * q.Wo;  // < 2^31: the launcher checks
  for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int ox = (int)(idx % q.Wo);
    const unsigned r = idx / q.Wo;
    const int oy = (int)(r % q.Ho);
    const int n = (int)(r / q.Ho);
    const Coord cy = coord(oy, q.sy, q.half_pixel, q.H), cx = coord(ox, q.sx, q.half_pixel, q.W);
    const bf16* r0 = x + ((size_t)n * q.H + cy.i0) * q.W * q.ldx;
    const bf16* r1 = x + ((size_t)n * q.H + cy.i1) * q.W * q.ldx;
    const size_t o0 = (size_t)cx.i0 * q.ldx, o1 = (size_t)cx.i1 * q.ldx;
    store_label(out, idx, argmax_pixel(r0 + o0, r0 + o1, r1 + o0, r1 + o1, cx.w, cy.w, q.C));
  }
}

constexpr int AM_TH = 16, AM_TW = 64, AM_PX = 4;  // output tile of a workgroup; pixels per thread
constexpr int AM_LDS_BYTES = 64 * 1024;           // window budget: two workgroups share a CU's 160 KiB

// grid: (tiles_x, tiles_y, N).  `cap` is the window capacity in pixels the launcher sized the
// dynamic LDS for; a tile whose window is larger (it cannot be, by the launcher's bound, for a
// scale <= 1) reads global memory instead of overrunning it.
template <typename T>
__global__ __launch_bounds__(256) void argmax_staged_kernel(const bf16* __restrict__ x, T* __restrict__ out,
                                                            const RsParams q, const int cap) {
  extern __shared__ __attribute__((aligned(16))) unsigned char am_lds[];
  bf16* win = reinterpret_cast<bf16*>(am_lds);
  const int n = blockIdx.z;
  const int oy_lo = blockIdx.y * AM_TH;
  const int oy_hi = min(oy_lo + AM_TH, q.Ho) - 1;
  // A thread's 4 pixels start `shift` pixels left of its tile column, so that their output
  // address is a multiple of 4 bytes whatever Wo and the row are: the tile covers the output
  // columns [tx * TW - 3, tx * TW + TW - 1].
  const int ox_lo = max((int)blockIdx.x * AM_TW - (AM_PX - 1), 0);
  const int ox_hi = min((int)blockIdx.x * AM_TW + AM_TW, q.Wo) - 1;
  if (ox_hi < ox_lo) return;  // the extra column of tiles, where no row needs it (uniform)
  const int iy_lo = coord(oy_lo, q.sy, q.half_pixel, q.H).i0, iy_hi = coord(oy_hi, q.sy, q.half_pixel, q.H).i1;
  const int ix_lo = coord(ox_lo, q.sx, q.half_pixel, q.W).i0, ix_hi = coord(ox_hi, q.sx, q.half_pixel, q.W).i1;
  const int wh = iy_hi - iy_lo + 1, ww = ix_hi - ix_lo + 1;
  const int vpp = (q.C + 7) / 8;  // staged 8-channel vectors per pixel
  const bool staged = wh * ww <= cap;
  if (staged) {
    const int nvec = wh * ww * vpp;
    for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
      const int v = i % vpp, p = i / vpp;
      const int wy = p / ww, wx = p % ww;
      const bf16* src = x + (((size_t)n * q.H + iy_lo + wy) * q.W + ix_lo + wx) * q.ldx + v * 8;
      *reinterpret_cast<bf16x8*>(win + (size_t)i * 8) = *reinterpret_cast<const bf16x8*>(src);
    }
  }
  __syncthreads();
  const int oy = oy_lo + (int)threadIdx.x / (AM_TW / AM_PX);
  if (oy > oy_hi) return;
  const size_t row = ((size_t)n * q.Ho + oy) * q.Wo;
  const int shift = (int)((reinterpret_cast<uintptr_t>(out + row) / sizeof(T)) & (AM_PX - 1)) * (sizeof(T) == 1);
  const int ox0 = (int)blockIdx.x * AM_TW + ((int)threadIdx.x % (AM_TW / AM_PX)) * AM_PX - shift;
  const Coord cy = coord(oy, q.sy, q.half_pixel, q.H);
  int lab[AM_PX];
#pragma unroll
  for (int j = 0; j < AM_PX; ++j) {
    const int ox = ox0 + j;
    lab[j] = 0;
    if (ox < ox_lo || ox > ox_hi) continue;
    const Coord cx = coord(ox, q.sx, q.half_pixel, q.W);
    if (staged) {
      const bf16* r0 = win + (size_t)(cy.i0 - iy_lo) * ww * vpp * 8;
      const bf16* r1 = win + (size_t)(cy.i1 - iy_lo) * ww * vpp * 8;
      const int o0 = (cx.i0 - ix_lo) * vpp * 8, o1 = (cx.i1 - ix_lo) * vpp * 8;
      lab[j] = argmax_pixel(r0 + o0, r0 + o1, r1 + o0, r1 + o1, cx.w, cy.w, q.C);
    } else {
      const bf16* r0 = x + ((size_t)n * q.H + cy.i0) * q.W * q.ldx;
      const bf16* r1 = x + ((size_t)n * q.H + cy.i1) * q.W * q.ldx;
      const size_t o0 = (size_t)cx.i0 * q.ldx, o1 = (size_t)cx.i1 * q.ldx;
      lab[j] = argmax_pixel(r0 + o0, r0 + o1, r1 + o0, r1 + o1, cx.w, cy.w, q.C);
    }
  }
  if constexpr (sizeof(T) == 1) {
    if (ox0 >= ox_lo && ox0 + AM_PX - 1 <= ox_hi) {
      const uint32_t packed =
          (uint32_t)lab[0] | (uint32_t)lab[1] << 8 | (uint32_t)lab[2] << 16 | (uint32_t)lab[3] << 24;
      *reinterpret_cast<uint32_t*>(out + row + ox0) = packed;
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < AM_PX; ++j) {
    const int ox = ox0 + j;
    if (ox >= ox_lo && ox <= ox_hi) store_label(out, row + ox, lab[j]);
  }
}

float rs_scale(int in, int out, bool align_corners) {
  if (align_corners && out > 1) return (float)((double)(in - 1) / (double)(out - 1));
  return (float)((double)in / (double)out);
}

// most input pixels along an axis that `t` consecutive output pixels touch, for a scale <= 1:
// their low corners span at most (t - 1) * scale, plus the rounding of floor, plus the high corner
int window_bound(int t, float scale, int size) {
  const long b = (long)((double)(t - 1) * (double)scale) + 3;
  return (int)(b < size ? b : size);
}

template <typename T>
void launch_argmax(const bf16* X, void* out, const RsParams& q, int path, hipStream_t s) {
  const bool upsample = q.Ho >= q.H && q.Wo >= q.W && q.sy <= 1.f && q.sx <= 1.f;
  const int vpp = (q.C + 7) / 8;
  const long cap = (long)window_bound(AM_TH, q.sy, q.H) * window_bound(AM_TW + AM_PX - 1, q.sx, q.W);
  const long lds = cap * vpp * 16;
  const bool fits = upsample && lds <= AM_LDS_BYTES;
  if (path == 1 && !fits)
    throw std::invalid_argument("resize_argmax: the staged kernel needs an upsample whose window fits");
  if (path == 1 || (path == 0 && fits)) {
    // uint8: one more column of tiles may be needed for the pixels shifted right of the last
    const int tx = (q.Wo + (sizeof(T) == 1 ? AM_PX - 1 : 0) + AM_TW - 1) / AM_TW;
    const int ty = (q.Ho + AM_TH - 1) / AM_TH;
    if (q.N > 65535 || ty > 65535) throw std::invalid_argument("resize_argmax: grid too large");
    const dim3 grid(tx, ty, q.N), block(256);
    hipLaunchKernelGGL(argmax_staged_kernel<T>, grid, block, (size_t)lds, s, X, reinterpret_cast<T*>(out), q, (int)cap);
  } else {
    const long work = (long)q.N * q.Ho * q.Wo;
    long g = (work + 255) / 256;
    g = g > 2048 * 8 ? 2048 * 8 : g;
    hipLaunchKernelGGL(argmax_simple_kernel<T>, dim3((unsigned)g), dim3(256), 0, s, X, reinterpret_cast<T*>(out), q);
  }
}

}  // namespace

void resize_bilinear_nhwc_bf16(uintptr_t x, uintptr_t y, int N, int H, int W, int C, int Ho, int Wo, int ldx, int ldy,
                               int y_coff, bool align_corners, bool half_pixel, uintptr_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || Ho <= 0 || Wo <= 0)
    throw std::invalid_argument("resize_bilinear: empty problem");
  if (C % 8 || ldx % 8 || ldy % 8 || y_coff % 8)
    throw std::invalid_argument("resize_bilinear: C, ldx, ldy, y_coff must be multiples of 8");
  if (ldx < C || y_coff < 0 || y_coff + C > ldy)
    throw std::invalid_argument("resize_bilinear: channel slot exceeds the row");
  if (x % 16 || y % 16) throw std::invalid_argument("resize_bilinear: pointers must be 16-byte aligned");
  const long work = (long)N * Ho * Wo * (C / 8);
  if (work >= (1L << 31)) throw std::invalid_argument("resize_bilinear: more than 2^31 output vectors");
  const RsParams q{N, H, W, C, Ho, Wo, ldx, ldy, y_coff, rs_scale(H, Ho, align_corners), rs_scale(W, Wo, align_corners),
                   half_pixel ? 1 : 0};
  long g = (work + 255) / 256;
  g = g > 2048 * 8 ? 2048 * 8 : g;
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)g), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const bf16*>(x), reinterpret_cast<bf16*>(y), q);
  FTM_CHECK_LAUNCH();
}

// out_bytes: element size of the label map, 1 (uint8), 4 (int32) or 8 (int64).  path: 0 = chosen
// here, 1 = the staged kernel (an error where its window does not fit), -1 = the simple kernel.
void resize_argmax_nhwc_bf16(uintptr_t x, uintptr_t out, int N, int H, int W, int C, int Ho, int Wo, int ldx,
                             int out_bytes, bool align_corners, bool half_pixel, int path, uintptr_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) throw std::invalid_argument("resize_argmax: empty problem");
  if (C < 1 || C > 256) throw std::invalid_argument("resize_argmax: C must be 1..256");
  if (ldx % 8 || ldx < C) throw std::invalid_argument("resize_argmax: ldx must be a multiple of 8 and at least C");
  if (out_bytes != 1 && out_bytes != 4 && out_bytes != 8)
    throw std::invalid_argument("resize_argmax: out_bytes must be 1, 4 or 8");
  if (x % 16 || out % out_bytes) throw std::invalid_argument("resize_argmax: misaligned pointer");
  if (path < -1 || path > 1) throw std::invalid_argument("resize_argmax: path must be -1..1");
  if ((long)N * Ho * Wo >= (1L << 31)) throw std::invalid_argument("resize_argmax: more than 2^31 output pixels");
  const RsParams q{N, H, W, C, Ho, Wo, ldx, 0, 0, rs_scale(H, Ho, align_corners), rs_scale(W, Wo, align_corners),
                   half_pixel ? 1 : 0};
  auto s = reinterpret_cast<hipStream_t>(stream);
  auto X = reinterpret_cast<const bf16*>(x);
  auto O = reinterpret_cast<void*>(out);
  if (out_bytes == 1) launch_argmax<uint8_t>(X, O, q, path, s);
  else if (out_bytes == 4) launch_argmax<int32_t>(X, O, q, path, s);
  else launch_argmax<int64_t>(X, O, q, path, s);
  FTM_CHECK_LAUNCH();
}

void register_resize(pybind11::module_& m) {
  m.def("resize_bilinear_nhwc_bf16", &resize_bilinear_nhwc_bf16);
  m.def("resize_argmax_nhwc_bf16", &resize_argmax_nhwc_bf16);
}
