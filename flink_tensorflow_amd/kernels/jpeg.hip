// The arithmetic half of baseline JPEG decoding on the device: quantised coefficients (the
// host's entropy decoder, csrc/jpeg.cpp jpeg_entropy_into) -> RGB rows of the staging slot.
//
// Per image a coefficient row (int16, de-zigzagged, component planes of MCU-padded 8x8
// blocks) and a JpegCoeffHeader (csrc/jpeg_coeffs.h).  The arithmetic is the host decoder's,
// operation by operation (csrc/jpeg.cpp pass8 / Idct::run_avx2, upsample, convert's scalar
// loop; its scalar mirror there is idct_exact / coeffs_to_rgb_one): int32 dequantisation,
// the float LLM IDCT over rows then columns with an FMA exactly where the host has one,
// int(fma(v, 0.125, 128.5)) clamped, the integer triangle filter with edges replicated at
// the valid chroma size, and the 16.16 colour formula.  Grayscale and R / B of colour files
// come out bit-identical to jpeg_decode_into, G within one count of its Q15 AVX2 path.
//
// One workgroup per 128 x 32 pixel tile of one image (a whole number of MCUs for every
// supported sampling).  Phase 1: every 8 lanes transform one block — a lane loads one row of
// coefficients with a 16-byte load, runs the row pass, the 8 x 8 transpose goes through LDS,
// then the lane runs one column and writes its samples to the tile's planes in LDS.  The
// chroma planes take one block of halo on each upsampled side, recomputed from the
// neighbouring blocks' coefficients (the filter reads one sample beyond the tile).  Phase 2:
// a lane per 4 pixels upsamples, converts and writes 12 bytes of RGB to an LDS row buffer.
// Phase 3: the rows go out as aligned dwords, whatever the row's byte offset (an odd W puts
// rows at any alignment), with byte stores only for a row's ragged first and last dword.
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "../csrc/jpeg_coeffs.h"
#include "common.h"

namespace {

constexpr int JT_W = 128, JT_H = 32;       // pixel tile
constexpr int JT_NT = 256;                 // threads: 32 blocks in flight
constexpr int JT_YP = JT_W + 4;            // luma plane pitch (bytes)
constexpr int JT_CBC = JT_W / 8 + 2;       // chroma blocks per tile row / column incl. halo
constexpr int JT_CBR = JT_H / 8 + 2;
constexpr int JT_CP = JT_CBC * 8 + 4;      // chroma plane pitch
constexpr int JT_TP = 9;                   // transpose pitch (floats): conflict-free both ways
constexpr int JT_RP = JT_W * 3 + 8;        // RGB row pitch: a dword of slack for the funnel read

__constant__ uint8_t kJpegZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                        12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                        35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                        58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

typedef short s16x8 __attribute__((ext_vector_type(8)));

// the 1-D 8-point LLM transform of csrc/jpeg.cpp pass8, in place.  The library builds with
// -ffp-contract=fast: contraction is off in here, every FMA is written
FTM_DEVICE void jpeg_pass(float* v) {
#pragma clang fp contract(off)
  const float z1 = (v[2] + v[6]) * 0.541196100f;
  const float t2 = __builtin_fmaf(-v[6], 1.847759065f, z1);
  const float t3 = __builtin_fmaf(v[2], 0.765366865f, z1);
  const float t0 = v[0] + v[4], t1 = v[0] - v[4];
  const float t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  float o0 = v[7], o1 = v[5], o2 = v[3], o3 = v[1];
  const float q1 = o0 + o3, q2 = o1 + o2, q3 = o0 + o2, q4 = o1 + o3;
  const float q5 = (q3 + q4) * 1.175875602f;
  const float k1 = -0.899976223f, k2 = -2.562915447f;
  const float r3 = __builtin_fmaf(q3, -1.961570560f, q5), r4 = __builtin_fmaf(q4, -0.390180644f, q5);
  o0 = __builtin_fmaf(o0, 0.298631336f, __builtin_fmaf(q1, k1, r3));
  o1 = __builtin_fmaf(o1, 2.053119869f, __builtin_fmaf(q2, k2, r4));
  o2 = __builtin_fmaf(o2, 3.072711026f, __builtin_fmaf(q2, k2, r3));
  o3 = __builtin_fmaf(o3, 1.501321110f, __builtin_fmaf(q1, k1, r4));
  v[0] = t10 + o3;
  v[7] = t10 - o3;
  v[1] = t11 + o2;
  v[6] = t11 - o2;
  v[2] = t12 + o1;
  v[5] = t12 - o1;
  v[3] = t13 + o0;
  v[4] = t13 - o0;
}

FTM_DEVICE int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// what the tile needs of one component: blocks [r0, r1) x [c0, c1) of its plane, block
// (r, c) landing at sample ((r - ro) * 8, (c - co) * 8) of the LDS plane
struct TileBlocks {
  int r0, r1, c0, c1, ro, co;
  FTM_DEVICE int rows() const { return r1 - r0; }
  FTM_DEVICE int cols() const { return c1 - c0; }
  FTM_DEVICE int count() const { return rows() * cols(); }
};

// component with subsampling (sx, sy) under the tile at pixel (ty0, tx0): its own blocks,
// plus one block of halo on each side of an upsampled axis, within the bw x bh plane
FTM_DEVICE TileBlocks tile_blocks(int ty0, int tx0, int sx, int sy, int bw, int bh) {
  TileBlocks t;
  const int r = ty0 / (8 * sy), c = tx0 / (8 * sx);
  t.ro = r - 1;
  t.co = c - 1;
  t.r0 = max(r - (sy == 2 ? 1 : 0), 0);
  t.c0 = max(c - (sx == 2 ? 1 : 0), 0);
  t.r1 = min(r + JT_H / (8 * sy) + (sy == 2 ? 1 : 0), bh);
  t.c1 = min(c + JT_W / (8 * sx) + (sx == 2 ? 1 : 0), bw);
  return t;
}

__global__ __launch_bounds__(JT_NT) void jpeg_idct_rgb_kernel(const int16_t* __restrict__ coef,
                                                              const JpegCoeffHeader* __restrict__ headers,
                                                              uint8_t* __restrict__ out, int H, int W,
                                                              long coef_stride /* int16 elements */) {
  __shared__ __attribute__((aligned(16))) uint8_t s_y[JT_H * JT_YP];
  __shared__ __attribute__((aligned(16))) uint8_t s_c[2][JT_CBR * 8 * JT_CP];
  __shared__ __attribute__((aligned(16))) float s_t[JT_NT / 8][8 * JT_TP];
  __shared__ __attribute__((aligned(16))) uint8_t s_rgb[JT_H * JT_RP];
  __shared__ uint16_t s_q[3][64];  // quantisation tables in natural order

  const int img = blockIdx.z, tid = threadIdx.x;
  const JpegCoeffHeader& hd = headers[img];
  if (hd.status != 0) return;  // not taken by the entropy decoder: the row is the host's
  // the header comes from the host; nothing is read or written on the strength of a record
  // that does not describe an H x W image inside its coefficient row
  const int nc = hd.ncomp;
  if (nc != 1 && nc != 3) return;
  const int hmax = hd.comp[0].h, vmax = hd.comp[0].v;
  if (hmax < 1 || hmax > 2 || vmax < 1 || vmax > 2 || (nc == 1 && (hmax != 1 || vmax != 1))) return;
  const int mcux = (W + 8 * hmax - 1) / (8 * hmax), mcuy = (H + 8 * vmax - 1) / (8 * vmax);
  for (int i = 0; i < nc; ++i) {
    const JpegCoeffComponent& c = hd.comp[i];
    const int ch = i ? 1 : hmax, cv = i ? 1 : vmax;
    if (c.h != ch || c.v != cv || c.bw != mcux * ch || c.bh != mcuy * cv || c.offset < 0 || (c.offset & 7) ||
        (long)c.offset + (long)c.bw * c.bh * 64 > coef_stride)
      return;
  }
  const int sx = hmax, sy = vmax;  // chroma subsampling (chroma is 1x1)
  const int ty0 = blockIdx.y * JT_H, tx0 = blockIdx.x * JT_W;
  const int16_t* row = coef + (size_t)img * coef_stride;

  if (tid < 64 * nc) s_q[tid >> 6][kJpegZigzag[tid & 63]] = hd.qt[tid >> 6][tid & 63];
  __syncthreads();

  // ---- phase 1: IDCT of the tile's blocks into the LDS planes
  const TileBlocks by = tile_blocks(ty0, tx0, 1, 1, hd.comp[0].bw, hd.comp[0].bh);
  TileBlocks bc = by;
  if (nc == 3) bc = tile_blocks(ty0, tx0, sx, sy, hd.comp[1].bw, hd.comp[1].bh);
  const int n_y = by.count(), n_c = nc == 3 ? bc.count() : 0, n_jobs = n_y + 2 * n_c;
  const int grp = tid >> 3, ln = tid & 7;
  for (int base = 0; base < n_jobs; base += JT_NT / 8) {
    const int j = base + grp;
    const bool live = j < n_jobs;
    int comp = 0, k = j;
    if (k >= n_y) {
      k -= n_y;
      comp = 1;
      if (k >= n_c) {
        k -= n_c;
        comp = 2;
      }
    }
    TileBlocks tb;  // by value, field by field: a reference to one of the two would put both in scratch
    tb.r0 = comp ? bc.r0 : by.r0;
    tb.r1 = comp ? bc.r1 : by.r1;
    tb.c0 = comp ? bc.c0 : by.c0;
    tb.c1 = comp ? bc.c1 : by.c1;
    tb.ro = comp ? bc.ro : by.ro;
    tb.co = comp ? bc.co : by.co;
    const int br = live ? tb.r0 + k / tb.cols() : 0, bcol = live ? tb.c0 + k % tb.cols() : 0;
    float v[8];
    if (live) {  // row pass: lane ln takes the block's row ln (vertical frequency ln)
      const JpegCoeffComponent& c = hd.comp[comp];
      const s16x8 cf = *reinterpret_cast<const s16x8*>(row + c.offset + ((size_t)br * c.bw + bcol) * 64 + ln * 8);
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = (float)((int)cf[u] * (int)s_q[comp][ln * 8 + u]);
      jpeg_pass(v);
#pragma unroll
      for (int y = 0; y < 8; ++y) s_t[grp][ln * JT_TP + y] = v[y];
    }
    __syncthreads();
    if (live) {  // column pass: lane ln takes column ln
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = s_t[grp][u * JT_TP + ln];
      jpeg_pass(v);
      // the chroma planes keep room for the halo block before the tile's own, the luma plane has none
      const int pitch = comp ? JT_CP : JT_YP;
      uint8_t* d = comp ? s_c[comp - 1] + (br - tb.ro) * 8 * JT_CP + (bcol - tb.co) * 8 + ln
                        : s_y + (br - tb.r0) * 8 * JT_YP + (bcol - tb.c0) * 8 + ln;
#pragma unroll
      for (int x = 0; x < 8; ++x) d[x * pitch] = (uint8_t)clamp255(__float2int_rz(__builtin_fmaf(v[x], 0.125f, 128.5f)));
    }
    __syncthreads();
  }

  // ---- phase 2: 4 pixels per lane -> RGB bytes in the LDS row buffer
  const int th = min(JT_H, H - ty0), tw = min(JT_W, W - tx0);  // valid pixels of the tile
  const int vw = (W + sx - 1) / sx, vh = (H + sy - 1) / sy;    // valid chroma samples
  const int cy0 = bc.ro * 8, cx0 = bc.co * 8;                  // plane coordinates of the LDS chroma origin
  for (int it = tid; it < JT_H * (JT_W / 4); it += JT_NT) {
    const int r = it / (JT_W / 4), xq = (it % (JT_W / 4)) * 4;
    if (r >= th || xq >= tw) continue;
    const int y = ty0 + r;
    uint32_t pb[12];  // R G B of the 4 pixels
    const uint8_t* yr = s_y + r * JT_YP + xq;
    if (nc == 1) {
#pragma unroll
      for (int p = 0; p < 4; ++p) pb[3 * p] = pb[3 * p + 1] = pb[3 * p + 2] = yr[p];
    } else {
      // vertical 3:1 (scale 4) of the two chroma rows nearest to y, edges replicated
      int yc = y, yf = y, wv = 4;
      if (sy == 2) {
        yc = y >> 1;
        yf = (y & 1) ? (yc + 1 < vh ? yc + 1 : yc) : (yc > 0 ? yc - 1 : 0);
        wv = 3;
      }
      const int o0 = (yc - cy0) * JT_CP - cx0, o1 = (yf - cy0) * JT_CP - cx0;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int x = tx0 + xq + p;
        int cc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const uint8_t* pl = s_c[i];
          if (sx == 2) {
            const int xc = x >> 1;
            const int xn = (x & 1) ? (xc + 1 < vw ? xc + 1 : xc) : (xc > 0 ? xc - 1 : 0);
            const int a = wv * pl[o0 + xc] + (4 - wv) * pl[o1 + xc];
            const int b = wv * pl[o0 + xn] + (4 - wv) * pl[o1 + xn];
            cc[i] = (3 * a + b + 8) >> 4;
          } else if (sy == 2) {
            cc[i] = (wv * pl[o0 + x] + (4 - wv) * pl[o1 + x] + 2) >> 2;
          } else {
            cc[i] = pl[o0 + x];
          }
        }
        const int Y = (int)yr[p] << 16, B = cc[0] - 128, R = cc[1] - 128;
        pb[3 * p] = clamp255((Y + 91881 * R + 32768) >> 16);
        pb[3 * p + 1] = clamp255((Y - 22554 * B - 46802 * R + 32768) >> 16);
        pb[3 * p + 2] = clamp255((Y + 116130 * B + 32768) >> 16);
      }
    }
    uint32_t* d = reinterpret_cast<uint32_t*>(s_rgb + r * JT_RP + xq * 3);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = pb[4 * k] | (pb[4 * k + 1] << 8) | (pb[4 * k + 2] << 16) | (pb[4 * k + 3] << 24);
  }
  __syncthreads();

  // ---- phase 3: rows out as aligned dwords
  const int nbytes = tw * 3;
  constexpr int DW = JT_W * 3 / 4 + 1;  // aligned dwords a row can touch
  for (int it = tid; it < th * DW; it += JT_NT) {
    const int r = it / DW, dw = it % DW;
    uint8_t* g = out + (((size_t)img * H + (ty0 + r)) * W + tx0) * 3;  // the row's first byte
    const int mis = (int)(reinterpret_cast<uintptr_t>(g) & 3);
    const int s = dw * 4 - mis;  // this dword's first byte, as an offset into the row
    if (s >= nbytes) continue;
    const uint8_t* src = s_rgb + r * JT_RP;
    if (s >= 0 && s + 4 <= nbytes) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(src + (s & ~3));
      const uint64_t two = ((uint64_t)w[1] << 32) | w[0];
      *reinterpret_cast<uint32_t*>(g + s) = (uint32_t)(two >> ((s & 3) * 8));
    } else {
      for (int b = max(s, 0); b < min(s + 4, nbytes); ++b) g[b] = src[b];
    }
  }
}

}  // namespace

// n coefficient rows (coef_stride bytes each) + headers -> n RGB rows [H, W, 3] at out
void jpeg_idct_rgb(uintptr_t coef, uintptr_t headers, uintptr_t out, int n, int H, int W, long coef_stride,
                   uintptr_t stream) {
  if (n < 0 || H <= 0 || W <= 0) throw std::invalid_argument("jpeg_idct_rgb: bad shape");
  if (coef % 16 || coef_stride % 16 || coef_stride <= 0)
    throw std::invalid_argument("jpeg_idct_rgb: coefficient rows must be 16-byte aligned");
  if (headers % alignof(JpegCoeffHeader)) throw std::invalid_argument("jpeg_idct_rgb: headers must be 16-byte aligned");
  if (n > 65535 || (H + JT_H - 1) / JT_H > 65535) throw std::invalid_argument("jpeg_idct_rgb: batch or image too large");
  if (n == 0) return;
  const dim3 grid((W + JT_W - 1) / JT_W, (H + JT_H - 1) / JT_H, n);
  hipLaunchKernelGGL(jpeg_idct_rgb_kernel, grid, dim3(JT_NT), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const int16_t*>(coef), reinterpret_cast<const JpegCoeffHeader*>(headers),
                     reinterpret_cast<uint8_t*>(out), H, W, coef_stride / 2);
  FTM_CHECK_LAUNCH();
}

void register_jpeg(pybind11::module_& m) {
  m.def("jpeg_idct_rgb", &jpeg_idct_rgb, pybind11::arg("coef"), pybind11::arg("headers"), pybind11::arg("out"),
        pybind11::arg("n"), pybind11::arg("h"), pybind11::arg("w"), pybind11::arg("coef_stride"),
        pybind11::arg("stream"));
}
