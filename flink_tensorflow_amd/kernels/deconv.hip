// Transposed convolution (TF Conv2DBackpropInput / Keras Conv2DTranspose) on CDNA4 MFMA:
// bf16 NHWC in, fp32 accumulate, one rounding, y = act(deconv(x, w) + bias[c]).
//
//   y[n, oy, ox, co] = sum x[n, iy, ix, ci] * w[ky, kx, co, ci]
// over the taps with oy + pt - ky == iy * sh, 0 <= iy < Hi (likewise in x).  Gather
// formulation, decomposed by output phase: for (py, px) in [0, sh) x [0, sw) the pixels
// (qy * sh + py, qx * sw + px) form one implicit GEMM whose taps are ky == (py + pt) mod sh,
// kx == (px + pl) mod sw, read at the input pixel (qy + dy, qx + dx) with the constant shifts
// dy = (py + pt - ky) / sh, dx = (px + pl - kx) / sw.  So a stride-s layer does 1 / (s * s) of
// the MACs of the same layer run as a conv over a zero-stuffed input, reads x instead of the
// stuffed buffer, and needs no scatter and no atomics: every output element is written once,
// by one thread.
//
//   x    [N, Hi, Wi, Cin] bf16, dense, Cin % 8 == 0
//   w    packed by ops/kernels.py deconv_pack_weights: phase-major (py * sw + px); per phase a
//        [Cout][taps * Cin] matrix, K-contiguous rows, taps in (ky, kx) order.  The per-phase
//        table (tap shifts, tap count, matrix offset) is rebuilt here on the host from the
//        geometry and travels in the kernel arguments.
//   bias [Cout] fp32
//   y    bf16, pixel pitch ldo >= coff + Cout, channel offset coff (a concat slot)
//
// GEMM view per phase: C^T[Cout, M] = W[Cout, K] . X^T[K, M], M = N * Hq * Wq pixels of the
// phase, K = taps * Cin.  One launch covers (pixel tile, phase, channel tile), in that order,
// so that the phases of one pixel tile, which read the same input rows, run next to each
// other; a block past its phase's pixels (phases differ when Ho % sh != 0) leaves at once.  A
// phase without taps (KH < sh) has K = 0: its pixels are act(bias).
//
// Tiles, staging and the epilogue follow igemm_bf16.hip: 4 waves, each 64 channels x TM pixels
// of v_mfma_f32_16x16x32_bf16 fragments, <BM=128, BN=128> or <BM=256, BN=64> (Cout <= 64);
// K staged 64 deep through registers into one LDS stage of 128-byte rows, chunk-XOR swizzled
// so every ds_read_b128 fragment read is conflict-free; the (acc + bias, act) tile is rounded
// into LDS and streamed out as 16-byte channel-row segments.  The K walk goes tap by tap and,
// inside a tap, over ceil(Cin / 64) tiles: no divide in the loop.  A tap outside the input, a
// pixel row past M, a weight row past Cout and the channels past Cin of a tap's last tile
// (Cin % 64 != 0) are predicated zero loads: no address is clamped, nothing is over-read.
// Offsets into x and y are 64-bit.
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace {

constexpr int BK = 64;   // K per stage
constexpr int NT = 256;  // threads
constexpr int MAX_PHASES = 16;
constexpr int MAX_TAPS = 64;

struct DeconvParams {
  const bf16* x;
  const bf16* w;
  const float* bias;
  bf16* y;
  int N, Hi, Wi, Cin, Ho, Wo, Cout, sh, sw, ldo, coff;
  int tiles_m, tiles_n, nph;
  int ctiles;              // K tiles per tap: ceil(Cin / BK)
  int woff[MAX_PHASES];    // element offset of the phase's weight matrix
  int tap0[MAX_PHASES];    // first entry of the phase in dy / dx
  int ntap[MAX_PHASES];
  int dy[MAX_TAPS], dx[MAX_TAPS];  // input shift of each tap, all phases back to back
};

FTM_DEVICE int swz(int row, int chunk) { return row * BK + ((chunk ^ (row & 7)) << 3); }

template <int BM, int BN, int ACT>
__global__ __launch_bounds__(NT, 2) void deconv_bf16_kernel(const DeconvParams p) {
  constexpr int WAVES_N = BN / 64;
  constexpr int WAVES_M = 4 / WAVES_N;
  constexpr int TM = BM / WAVES_M;  // pixels per wave
  constexpr int J = TM / 16;        // pixel fragments per wave
  constexpr int XR = BM / 32;       // X chunks staged per thread
  constexpr int WR = BN / 32;       // W chunks staged per thread
  constexpr int OPAD = 8;           // epilogue row padding (bf16)
  constexpr int STAGE_ELEMS = (BM + BN) * BK;
  constexpr int EPI_ELEMS = BM * (BN + OPAD);
  constexpr int LDS_ELEMS = STAGE_ELEMS > EPI_ELEMS ? STAGE_ELEMS : EPI_ELEMS;
  __shared__ __attribute__((aligned(16))) bf16 smem[LDS_ELEMS];
  bf16* Xs = smem;            // [BM][BK]
  bf16* Ws = smem + BM * BK;  // [BN][BK]

  const int nwg = p.tiles_m * p.nph * p.tiles_n;
  const int tile = xcd_remap(blockIdx.x, nwg);
  const int tn = tile % p.tiles_n;
  const int tp = tile / p.tiles_n;
  const int ph = tp % p.nph;
  const int tm = tp / p.nph;
  const int py = ph / p.sw, px = ph - py * p.sw;
  // pixels of this phase: oy = qy * sh + py < Ho
  const int Hq = py < p.Ho ? (p.Ho - py + p.sh - 1) / p.sh : 0;
  const int Wq = px < p.Wo ? (p.Wo - px + p.sw - 1) / p.sw : 0;
  const int M = p.N * Hq * Wq;  // < 2^31: the launcher checks N * ceil(Ho/sh) * ceil(Wo/sw)
  const int m0 = tm * BM;
  const int n0 = tn * BN;
  if (m0 >= M) return;  // block-uniform

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wp = wave % WAVES_M;  // pixel slab of the tile
  const int wc = wave / WAVES_M;  // channel slab

  // per-thread staging assignment: fixed k-chunk, rows r0 + 32 i
  const int kc = tid & 7;
  const int r0 = tid >> 3;

  // per staged pixel row: the element offset of input pixel (n, qy, qx) and (qy, qx); a row
  // past M gets a qy no tap shift brings back into the image
  long xbase[XR];
  int rqy[XR], rqx[XR];
#pragma unroll
  for (int i = 0; i < XR; ++i) {
    const int m = m0 + r0 + 32 * i;
    const bool mv = m < M;
    const int mm = mv ? m : 0;
    const int qx = mm % Wq;
    const int t = mm / Wq;
    const int qy = t % Hq;
    const int n = t / Hq;
    xbase[i] = (((long)n * p.Hi + qy) * p.Wi + qx) * p.Cin;
    rqy[i] = mv ? qy : -(1 << 20);
    rqx[i] = qx;
  }
  const int ntap = p.ntap[ph];
  const int tap0 = p.tap0[ph];
  const int Kp = ntap * p.Cin;  // row length of the phase's weight matrix
  const bf16* wph = p.w + p.woff[ph];
  int wrow[WR];  // element offset of this thread's weight rows, -1 past Cout
#pragma unroll
  for (int i = 0; i < WR; ++i) {
    const int co = n0 + r0 + 32 * i;
    wrow[i] = co < p.Cout ? co * Kp : -1;
  }

  u32x4 xr[XR], wr[WR];
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // K walk: tile kt covers channels [c0, c0 + 64) of tap `tap`
  int tap = 0, c0 = 0;
  auto load_tile = [&]() {
    const int ci = c0 + kc * 8;
    const bool cv = ci < p.Cin;  // the tap's last tile: channels past Cin are zeros
    const int dy = p.dy[tap0 + tap], dx = p.dx[tap0 + tap];
    const long toff = ((long)dy * p.Wi + dx) * p.Cin + ci;
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const bool ok = cv && (unsigned)(rqy[i] + dy) < (unsigned)p.Hi && (unsigned)(rqx[i] + dx) < (unsigned)p.Wi;
      xr[i] = ok ? *reinterpret_cast<const u32x4*>(p.x + (xbase[i] + toff)) : zero4;
    }
    const int wk = tap * p.Cin + ci;
#pragma unroll
    for (int i = 0; i < WR; ++i) {
      const bool ok = cv && wrow[i] >= 0;
      wr[i] = ok ? *reinterpret_cast<const u32x4*>(wph + wrow[i] + wk) : zero4;
    }
    c0 += BK;
    if (c0 >= p.Cin) { c0 = 0; ++tap; }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < XR; ++i) *reinterpret_cast<u32x4*>(Xs + swz(r0 + 32 * i, kc)) = xr[i];
#pragma unroll
    for (int i = 0; i < WR; ++i) *reinterpret_cast<u32x4*>(Ws + swz(r0 + 32 * i, kc)) = wr[i];
  };

  f32x4 acc[4][J];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < J; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = ntap * p.ctiles;  // 0 for a phase without taps
  if (nk > 0) {
    load_tile();
    store_tile();
  }
  __syncthreads();

  const int frow = lane & 15;
  const int fchunk = lane >> 4;  // 0..3 -> k offset 8 * fchunk within a 32-deep substep

  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) load_tile();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 a[4], b[J];
      const int chunk = ks * 4 + fchunk;
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bf16x8*>(Ws + swz(wc * 64 + i * 16 + frow, chunk));
#pragma unroll
      for (int j = 0; j < J; ++j) b[j] = *reinterpret_cast<const bf16x8*>(Xs + swz(wp * TM + j * 16 + frow, chunk));
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) {
      __syncthreads();  // single buffer: everyone done reading
      store_tile();
    }
    __syncthreads();
  }

  // ---- epilogue phase 1: act(acc + bias) -> bf16 LDS tile [BM][BN + OPAD]
  constexpr int OLD = BN + OPAD;
  bf16* Os = smem;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int cl = wc * 64 + i * 16 + (lane >> 4) * 4;  // local channel of this lane's 4 rows
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (n0 + cl < p.Cout) bv = *reinterpret_cast<const f32x4*>(p.bias + n0 + cl);  // Cout % 8 == 0
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int pl = wp * TM + j * 16 + (lane & 15);
      const f32x4 v = acc[i][j] + bv;
      bf16x4 o;
      o[0] = f2bf(apply_act<ACT>(v[0]));
      o[1] = f2bf(apply_act<ACT>(v[1]));
      o[2] = f2bf(apply_act<ACT>(v[2]));
      o[3] = f2bf(apply_act<ACT>(v[3]));
      *reinterpret_cast<bf16x4*>(Os + pl * OLD + cl) = o;
    }
  }
  __syncthreads();

  // ---- epilogue phase 2: 16-B channel-row segments to pixel (n, qy * sh + py, qx * sw + px)
  constexpr int CPR = BN / 8;  // 16-B chunks per tile row
#pragma unroll
  for (int it = 0; it < (BM * CPR + NT - 1) / NT; ++it) {
    const int q = tid + it * NT;
    const int pl = q / CPR;
    const int cc = q % CPR;
    const int m = m0 + pl;
    const int c = n0 + cc * 8;
    if (q >= BM * CPR || m >= M || c >= p.Cout) continue;
    const int qx = m % Wq;
    const int t = m / Wq;
    const int qy = t % Hq;
    const int n = t / Hq;
    const long pix = ((long)n * p.Ho + (qy * p.sh + py)) * p.Wo + (qx * p.sw + px);
    *reinterpret_cast<bf16x8*>(p.y + (pix * p.ldo + p.coff + c)) = *reinterpret_cast<const bf16x8*>(Os + pl * OLD + cc * 8);
  }
}

template <int BM, int BN>
void launch_tile(DeconvParams p, int act, hipStream_t s) {
  const long mq = (long)p.N * ((p.Ho + p.sh - 1) / p.sh) * ((p.Wo + p.sw - 1) / p.sw);  // the largest phase
  p.tiles_m = (int)((mq + BM - 1) / BM);
  p.tiles_n = (p.Cout + BN - 1) / BN;
  const long blocks = (long)p.tiles_m * p.nph * p.tiles_n;
  if (blocks >= (1L << 31)) throw std::invalid_argument("deconv: more than 2^31 blocks");
  const dim3 grid((unsigned)blocks), block(NT);
  switch (act) {
    case ACT_NONE: hipLaunchKernelGGL((deconv_bf16_kernel<BM, BN, ACT_NONE>), grid, block, 0, s, p); break;
    case ACT_RELU: hipLaunchKernelGGL((deconv_bf16_kernel<BM, BN, ACT_RELU>), grid, block, 0, s, p); break;
    case ACT_RELU6: hipLaunchKernelGGL((deconv_bf16_kernel<BM, BN, ACT_RELU6>), grid, block, 0, s, p); break;
    default: throw std::invalid_argument("deconv: act must be none, relu or relu6");
  }
}

// Tile configurations: 0 = 128 pixels x 128 channels, 1 = 256 pixels x 64 channels.
constexpr int NCFG = 2;

}  // namespace

// cfg: -1 = chosen here (256 x 64 for Cout <= 64, where a 128-channel tile would waste half of
// its MFMAs), else the tile configuration: measurement and tests only.  w_elems is the element
// count of the packed weight tensor, checked against the geometry.
void deconv_nhwc_bf16(uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t y, int N, int Hi, int Wi, int Cin, int Ho,
                      int Wo, int Cout, int KH, int KW, int sh, int sw, int pt, int pl, int act, int ldo, int coff,
                      long w_elems, int cfg, uintptr_t stream) {
  if (N <= 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Ho <= 0 || Wo <= 0 || Cout <= 0)
    throw std::invalid_argument("deconv: empty problem");
  if (Cin % 8 || Cout % 8 || ldo % 8 || coff % 8) throw std::invalid_argument("deconv: Cin, Cout, ldo, coff must be multiples of 8");
  if (coff < 0 || coff + Cout > ldo) throw std::invalid_argument("deconv: channel slot exceeds the output row");
  if (KH < 1 || KW < 1 || KH > 8 || KW > 8) throw std::invalid_argument("deconv: filter must be 1..8 x 1..8");
  if (sh < 1 || sw < 1 || sh > 4 || sw > 4) throw std::invalid_argument("deconv: strides must be 1..4");
  if (pt < 0 || pl < 0 || pt >= KH || pl >= KW) throw std::invalid_argument("deconv: pads must be below the filter size");
  if (!x || !w || !bias || !y) throw std::invalid_argument("deconv: null pointer (pass zeros for no bias)");
  if (x % 16 || w % 16 || y % 16 || bias % 16) throw std::invalid_argument("deconv: pointers must be 16-byte aligned");
  if (act != ACT_NONE && act != ACT_RELU && act != ACT_RELU6) throw std::invalid_argument("deconv: act must be none, relu or relu6");
  if (cfg < -1 || cfg >= NCFG) throw std::invalid_argument("deconv: unknown tile configuration " + std::to_string(cfg));
  if (w_elems != (long)KH * KW * Cout * Cin) throw std::invalid_argument("deconv: packed weights do not match the geometry");
  if (w_elems >= (1L << 31)) throw std::invalid_argument("deconv: weights too large for 32-bit indexing");
  if ((long)N * ((Ho + sh - 1) / sh) * ((Wo + sw - 1) / sw) >= (1L << 31))
    throw std::invalid_argument("deconv: more than 2^31 pixels per phase");
  DeconvParams p{};
  p.x = reinterpret_cast<const bf16*>(x);
  p.w = reinterpret_cast<const bf16*>(w);
  p.bias = reinterpret_cast<const float*>(bias);
  p.y = reinterpret_cast<bf16*>(y);
  p.N = N; p.Hi = Hi; p.Wi = Wi; p.Cin = Cin; p.Ho = Ho; p.Wo = Wo; p.Cout = Cout;
  p.sh = sh; p.sw = sw; p.ldo = ldo; p.coff = coff;
  p.nph = sh * sw;
  p.ctiles = (Cin + BK - 1) / BK;
  // the phase table, in the order deconv_pack_weights lays the matrices out
  int nt = 0;
  long off = 0;
  for (int py = 0; py < sh; ++py)
    for (int px = 0; px < sw; ++px) {
      const int ph = py * sw + px;
      p.woff[ph] = (int)off;
      p.tap0[ph] = nt;
      for (int ky = 0; ky < KH; ++ky) {
        if ((py + pt - ky) % sh) continue;
        for (int kx = 0; kx < KW; ++kx) {
          if ((px + pl - kx) % sw) continue;
          p.dy[nt] = (py + pt - ky) / sh;  // exact: the remainder is 0
          p.dx[nt] = (px + pl - kx) / sw;
          ++nt;
        }
      }
      p.ntap[ph] = nt - p.tap0[ph];
      off += (long)p.ntap[ph] * Cin * Cout;
    }
  // every (ky, kx) lands in exactly one phase: nt == KH * KW <= MAX_TAPS
  auto s = reinterpret_cast<hipStream_t>(stream);
  if (cfg < 0) cfg = Cout <= 64 ? 1 : 0;
  if (cfg == 0) launch_tile<128, 128>(p, act, s);
  else launch_tile<256, 64>(p, act, s);
  FTM_CHECK_LAUNCH();
}

void register_deconv(pybind11::module_& m) {
  m.def("deconv_nhwc_bf16", &deconv_nhwc_bf16);
  m.attr("deconv_num_configs") = NCFG;
}
