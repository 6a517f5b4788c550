// Depthwise conv, bf16 NHWC (MobileNet / Xception / EfficientNet-lite): y[n, oy, ox, c] =
// act(sum_taps x[n, iy, ix, c] * w[tap, c] + bias[c]).  There is no reduction over
// channels, so there is no MFMA in it: the layer streams its input once and is bound by
// memory.  Each thread owns one 8-channel vector (16-B loads and stores, guide Guideline
// 13); consecutive lanes take consecutive channel vectors of the same pixel, so a wave
// reads and writes contiguous runs of the NHWC rows.
//
//   x    [N, H, W, C] bf16, dense
//   w    [KH * KW, C] bf16, tap-major (TF's [KH, KW, C, 1] filter as it stands)
//   bias [C] fp32 or null
//   out  bf16, row pitch ldy >= C, channel offset y_coff (a concat slot)
//
// Taps accumulate in fp32; the bias is added in fp32, then the activation, then one
// round-to-nearest-even to bf16.  A tap outside the image is not loaded (the load is
// predicated, the address is never clamped): it contributes exactly zero and no lane
// reads outside x, w or bias.  Element offsets are 64-bit.
//
// Two kernels, chosen by the host launcher:
//   dwconv3x3_kernel<S, TH, TW, ACT>  3x3, dilation 1, stride S in {1, 2}: a thread owns a
//       TH x TW tile of adjacent output pixels, loads each input vector of the tile's
//       ((TH-1) S + 3) x ((TW-1) S + 3) window once and feeds it to every tap and output
//       that needs it; the 9 weight vectors and the bias stay in registers while the
//       thread walks its tiles (its channel vector never changes).
//   dwconv_generic_kernel<ACT>        runtime KH, KW <= 7, any stride and dilation: one
//       output pixel x 8 channels per thread, the weight vector of each tap read through L1.
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// 8 bf16 -> 4 float pairs: a bf16 is the high half of its fp32, so one shift or one mask
// per element; the pairs feed v_pk_fma_f32
FTM_DEVICE void unpack8(const bf16x8 v, f32x2 (&f)[4]) {
  const u32x4 u = __builtin_bit_cast(u32x4, v);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[i][0] = __builtin_bit_cast(float, u[i] << 16);
    f[i][1] = __builtin_bit_cast(float, u[i] & 0xffff0000u);
  }
}

FTM_DEVICE void load_bias(const float* bias, int c0, f32x2 (&b)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    b[i][0] = bias ? bias[c0 + 2 * i] : 0.f;
    b[i][1] = bias ? bias[c0 + 2 * i + 1] : 0.f;
  }
}

template <int ACT>
FTM_DEVICE void store8(bf16* p, const f32x2 (&acc)[4], const f32x2 (&b)[4]) {
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 v = acc[i] + b[i];
    o[2 * i] = f2bf(apply_act<ACT>(v[0]));
    o[2 * i + 1] = f2bf(apply_act<ACT>(v[1]));
  }
  *reinterpret_cast<bf16x8*>(p) = o;
}

struct DwParams {
  int N, H, W, C, Ho, Wo, KH, KW, sh, sw, dh, dw, pt, pl, ldy, y_coff;
};

// Thread t owns channel vector t % (C/8) for its whole life and walks the tiles
// slot, slot + nslots, ... (slot = t / (C/8)); threads past the last whole slot idle.
// Tile and thread counts are 32-bit (the launcher checks); element offsets are 64-bit.
template <int S, int TH, int TW, int ACT>
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w,
                                                        const float* __restrict__ bias, bf16* __restrict__ y,
                                                        const DwParams q) {
  constexpr int IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3;
  const unsigned cchunks = q.C / 8;
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned nslots = (gridDim.x * blockDim.x) / cchunks;
  const unsigned slot = t / cchunks;
  if (slot >= nslots) return;
  const int c0 = (int)(t % cchunks) * 8;

  bf16x8 wv[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) wv[k] = *reinterpret_cast<const bf16x8*>(w + (size_t)k * q.C + c0);
  f32x2 b[4];
  load_bias(bias, c0, b);

  const unsigned tiles_x = (q.Wo + TW - 1) / TW, tiles_y = (q.Ho + TH - 1) / TH;
  const unsigned ntiles = (unsigned)q.N * tiles_y * tiles_x;
  const long row_pitch = (long)q.W * q.C;
  for (unsigned tile = slot; tile < ntiles; tile += nslots) {
    const unsigned tx = tile % tiles_x;
    const unsigned r = tile / tiles_x;
    const unsigned ty = r % tiles_y;
    const unsigned n = r / tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const int iy0 = oy0 * S - q.pt, ix0 = ox0 * S - q.pl;
    // element offset of the window's first pixel: an offset, not a pointer, since the
    // window may start above or left of the image; only in-image pixels are dereferenced
    const long base = ((long)n * q.H + iy0) * row_pitch + (long)ix0 * q.C + c0;

    f32x2 acc[TH][TW][4];
#pragma unroll
    for (int i = 0; i < TH; ++i)
#pragma unroll
      for (int j = 0; j < TW; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][j][e] = f32x2{0.f, 0.f};

#pragma unroll
    for (int ry = 0; ry < IH; ++ry) {
      const bool row_ok = (unsigned)(iy0 + ry) < (unsigned)q.H;
      f32x2 xf[IW][4];
#pragma unroll
      for (int rx = 0; rx < IW; ++rx) {
        bf16x8 z = {};
        if (row_ok && (unsigned)(ix0 + rx) < (unsigned)q.W)
          z = *reinterpret_cast<const bf16x8*>(x + (base + ry * row_pitch + (long)rx * q.C));
        unpack8(z, xf[rx]);
      }
#pragma unroll
      for (int i = 0; i < TH; ++i) {
        const int kh = ry - i * S;  // compile-time after unrolling
        if (kh < 0 || kh > 2) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          f32x2 wf[4];
          unpack8(wv[kh * 3 + kw], wf);
#pragma unroll
          for (int j = 0; j < TW; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][e] = xf[j * S + kw][e] * wf[e] + acc[i][j][e];
        }
      }
    }

#pragma unroll
    for (int i = 0; i < TH; ++i) {
      const int oy = oy0 + i;
      if (oy >= q.Ho) continue;
#pragma unroll
      for (int j = 0; j < TW; ++j) {
        const int ox = ox0 + j;
        if (ox >= q.Wo) continue;
        store8<ACT>(y + (((size_t)n * q.Ho + oy) * q.Wo + ox) * q.ldy + q.y_coff + c0, acc[i][j], b);
      }
    }
  }
}

template <int ACT>
__global__ __launch_bounds__(256) void dwconv_generic_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w,
                                                             const float* __restrict__ bias, bf16* __restrict__ y,
                                                             const DwParams q) {
  const unsigned cchunks = q.C / 8;
  const unsigned total = (unsigned)q.N * q.Ho * q.Wo * cchunks;  // < 2^31: the launcher checks
  for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % cchunks) * 8;
    unsigned r = idx / cchunks;
    const int ox = (int)(r % q.Wo);
    r /= q.Wo;
    const int oy = (int)(r % q.Ho);
    const int n = (int)(r / q.Ho);
    f32x2 acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = f32x2{0.f, 0.f};
    const int iy0 = oy * q.sh - q.pt, ix0 = ox * q.sw - q.pl;
    for (int kh = 0; kh < q.KH; ++kh) {
      const int iy = iy0 + kh * q.dh;
      if ((unsigned)iy >= (unsigned)q.H) continue;
      for (int kw = 0; kw < q.KW; ++kw) {
        const int ix = ix0 + kw * q.dw;
        if ((unsigned)ix >= (unsigned)q.W) continue;
        f32x2 xf[4], wf[4];
        unpack8(*reinterpret_cast<const bf16x8*>(x + (((size_t)n * q.H + iy) * q.W + ix) * q.C + c0), xf);
        unpack8(*reinterpret_cast<const bf16x8*>(w + (size_t)(kh * q.KW + kw) * q.C + c0), wf);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = xf[e] * wf[e] + acc[e];
      }
    }
    f32x2 b[4];
    load_bias(bias, c0, b);
    store8<ACT>(y + (((size_t)n * q.Ho + oy) * q.Wo + ox) * q.ldy + q.y_coff + c0, acc, b);
  }
}

// blocks of 256 threads for `work` threads, at most `cap`; at least enough for one slot
int dw_grid(long work, long cap, int cchunks) {
  long g = (work + 255) / 256;
  const long lo = (cchunks + 255) / 256;
  g = g > cap ? cap : g;
  return (int)(g < lo ? lo : g);
}

template <int S, int TH, int TW>
void launch3x3(const bf16* x, const bf16* w, const float* b, bf16* y, const DwParams& q, int act, hipStream_t s) {
  const long tiles = (long)q.N * ((q.Ho + TH - 1) / TH) * ((q.Wo + TW - 1) / TW);
  if (tiles >= (1L << 31)) throw std::invalid_argument("dwconv: more than 2^31 output tiles");
  // 2048 blocks = 8 per CU: every thread walks several tiles with its weights in registers
  const dim3 grid(dw_grid(tiles * (q.C / 8), 2048, q.C / 8)), block(256);
  if (act == ACT_RELU6) hipLaunchKernelGGL((dwconv3x3_kernel<S, TH, TW, ACT_RELU6>), grid, block, 0, s, x, w, b, y, q);
  else if (act == ACT_RELU) hipLaunchKernelGGL((dwconv3x3_kernel<S, TH, TW, ACT_RELU>), grid, block, 0, s, x, w, b, y, q);
  else hipLaunchKernelGGL((dwconv3x3_kernel<S, TH, TW, ACT_NONE>), grid, block, 0, s, x, w, b, y, q);
}

}  // namespace

// tile: the 3x3 kernel's output tile per thread, 0 = chosen here, 1 = 1x4, 2 = 2x2; -1 = the
// generic kernel whatever the shape.
void dwconv_nhwc_bf16(uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t y, int N, int H, int W, int C, int Ho, int Wo,
                      int KH, int KW, int sh, int sw, int dh, int dw, int pt, int pl, int act, int ldy, int y_coff,
                      int tile, uintptr_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) throw std::invalid_argument("dwconv: empty problem");
  if (C % 8 || ldy % 8 || y_coff % 8) throw std::invalid_argument("dwconv: C, ldy, y_coff must be multiples of 8");
  if (y_coff < 0 || y_coff + C > ldy) throw std::invalid_argument("dwconv: channel slot exceeds the output row");
  if (x % 16 || w % 16 || y % 16 || bias % 4) throw std::invalid_argument("dwconv: pointers must be 16-byte aligned");
  if (KH < 1 || KW < 1 || KH > 7 || KW > 7) throw std::invalid_argument("dwconv: filter must be 1..7 x 1..7");
  if (sh < 1 || sw < 1 || dh < 1 || dw < 1 || pt < 0 || pl < 0) throw std::invalid_argument("dwconv: bad geometry");
  // every output's first tap starts at or before the last input row / column
  if ((long)(Ho - 1) * sh - pt >= H || (long)(Wo - 1) * sw - pl >= W)
    throw std::invalid_argument("dwconv: output larger than the padded input allows");
  if (act != ACT_NONE && act != ACT_RELU && act != ACT_RELU6)
    throw std::invalid_argument("dwconv: act must be none, relu or relu6");
  if (tile < -1 || tile > 2) throw std::invalid_argument("dwconv: tile must be -1..2");
  const DwParams q{N, H, W, C, Ho, Wo, KH, KW, sh, sw, dh, dw, pt, pl, ldy, y_coff};
  auto s = reinterpret_cast<hipStream_t>(stream);
  auto X = reinterpret_cast<const bf16*>(x);
  auto Wt = reinterpret_cast<const bf16*>(w);
  auto B = reinterpret_cast<const float*>(bias);
  auto Y = reinterpret_cast<bf16*>(y);
  const bool k3 = KH == 3 && KW == 3 && dh == 1 && dw == 1 && sh == sw && (sh == 1 || sh == 2);
  if (tile > 0 && !k3) throw std::invalid_argument("dwconv: a tile needs 3x3, dilation 1, stride 1 or 2");
  if (k3 && tile >= 0) {
    if (tile == 0) {
      // 2x2 reads 4 input vectors per output at stride 1 (1x4: 4.5) and measured faster on
      // every MobileNet layer but the 7x7 one, where its tiles cover 8x8 pixels against 1x4's
      // 7x8: take 1x4 only where it pads the output less
      auto up = [](int v, int t) { return (v + t - 1) / t * t; };
      tile = (long)Ho * up(Wo, 4) < (long)up(Ho, 2) * up(Wo, 2) ? 1 : 2;
    }
    if (tile == 1 && sh == 1) launch3x3<1, 1, 4>(X, Wt, B, Y, q, act, s);
    else if (tile == 1) launch3x3<2, 1, 4>(X, Wt, B, Y, q, act, s);
    else if (sh == 1) launch3x3<1, 2, 2>(X, Wt, B, Y, q, act, s);
    else launch3x3<2, 2, 2>(X, Wt, B, Y, q, act, s);
  } else {
    const long work = (long)N * Ho * Wo * (C / 8);
    if (work >= (1L << 31)) throw std::invalid_argument("dwconv: more than 2^31 output vectors");
    const dim3 grid(dw_grid(work, 2048 * 8, 1)), block(256);
    if (act == ACT_RELU6) hipLaunchKernelGGL(dwconv_generic_kernel<ACT_RELU6>, grid, block, 0, s, X, Wt, B, Y, q);
    else if (act == ACT_RELU) hipLaunchKernelGGL(dwconv_generic_kernel<ACT_RELU>, grid, block, 0, s, X, Wt, B, Y, q);
    else hipLaunchKernelGGL(dwconv_generic_kernel<ACT_NONE>, grid, block, 0, s, X, Wt, B, Y, q);
  }
  FTM_CHECK_LAUNCH();
}

void register_dwconv(pybind11::module_& m) { m.def("dwconv_nhwc_bf16", &dwconv_nhwc_bf16); }
