// 3-D convolution and 3-D pooling (TF Conv3D / MaxPool3D / AvgPool3D, NDHWC) on CDNA4: the
// video family (C3D, I3D, R(2+1)D).
//
// conv3d_ndhwc_bf16: bf16 in, fp32 accumulate, one rounding, y = act(conv3d(x, w) + bias[c]).
//
//   y[n, od, oh, ow, co] = sum x[n, od sd + kd - pf, oh sh + kh - pt, ow sw + kw - pl, ci]
//                              * w[co, (kd, kh, kw), ci]
// over the taps whose input index is inside x on all three axes.
//
//   x    [N, D, H, W, Cin] bf16, dense, Cin % 8 == 0
//   w    packed by ops/kernels.py conv3d_pack_weights: [Cout][KD * KH * KW * Cin], K-contiguous
//        rows, taps in (kd, kh, kw) order
//   bias [Cout] fp32
//   y    bf16, pixel pitch ldo >= coff + Cout, channel offset coff (a concat slot)
//
// GEMM view: C^T[Cout, M] = W[Cout, K] . X^T[K, M], M = N * Do * Ho * Wo output pixels,
// K = KD * KH * KW * Cin.  One launch covers (pixel tile, channel tile).
//
// Tiles, staging and the epilogue follow deconv.hip / igemm_bf16.hip: 4 waves, each 64 channels x
// TM pixels of v_mfma_f32_16x16x32_bf16 fragments, <BM=128, BN=128> or <BM=256, BN=64>
// (Cout <= 64); K staged 64 deep through registers into one LDS stage of 128-byte rows,
// chunk-XOR swizzled so every ds_read_b128 fragment read is conflict-free; the (acc + bias, act)
// tile is rounded into LDS and streamed out as 16-byte channel-row segments.  The K walk goes
// tap by tap in (kd, kh, kw) order and, inside a tap, over ceil(Cin / 64) tiles, on incremental
// counters: no divide in the loop.  A tap outside the input on any axis, a pixel row past M, a
// weight row past Cout and the channels past Cin of a tap's last tile (Cin % 64 != 0) are
// predicated zero loads: no address is clamped, nothing is over-read.  Offsets into x and y are
// 64-bit: a [256, 16, 112, 112, 64] activation has 3.3 G elements.
//
// pool3d_ndhwc_bf16: max or average over a (kd, kh, kw) window; one thread per output pixel and
// 8-channel vector (16-byte loads and stores, consecutive lanes on consecutive channel vectors
// of a pixel).  Window elements outside the input are predicated out: never clamped, never read
// as zeros.  The average is the fp32 sum over the window in (kd, kh, kw) order divided by the
// valid count with `/` (no fast-math: the correctly rounded quotient), one rounding to bf16.
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace {

constexpr int BK = 64;   // K per stage
constexpr int NT = 256;  // threads

struct Conv3dParams {
  const bf16* x;
  const bf16* w;
  const float* bias;
  bf16* y;
  int N, D, H, W, Cin, Do, Ho, Wo, Cout;
  int KD, KH, KW, sd, sh, sw, pf, pt, pl, ldo, coff;
  int M;       // N * Do * Ho * Wo
  int Ktot;    // KD * KH * KW * Cin: row length of the weight matrix
  int ctiles;  // K tiles per tap: ceil(Cin / BK)
  int tiles_m, tiles_n;
};

FTM_DEVICE int swz(int row, int chunk) { return row * BK + ((chunk ^ (row & 7)) << 3); }

template <int BM, int BN, int ACT>
__global__ __launch_bounds__(NT, 2) void conv3d_bf16_kernel(const Conv3dParams p) {
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

  const int nwg = p.tiles_m * p.tiles_n;
  const int tile = xcd_remap(blockIdx.x, nwg);
  const int tn = tile % p.tiles_n;
  const int tm = tile / p.tiles_n;
  const int M = p.M;
  const int m0 = tm * BM;
  const int n0 = tn * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wp = wave % WAVES_M;  // pixel slab of the tile
  const int wc = wave / WAVES_M;  // channel slab

  // per-thread staging assignment: fixed k-chunk, rows r0 + 32 i
  const int kc = tid & 7;
  const int r0 = tid >> 3;

  // per staged pixel row: the input coordinates of tap (0, 0, 0) and their element offset (the
  // offset may point in front of x: it is only used once a tap brings it inside); a row past M
  // gets a depth no tap brings back into the input
  long xbase[XR];
  int rd[XR], rh[XR], rw[XR];
#pragma unroll
  for (int i = 0; i < XR; ++i) {
    const int m = m0 + r0 + 32 * i;
    const bool mv = m < M;
    const int mm = mv ? m : 0;
    const int ow = mm % p.Wo;
    int t = mm / p.Wo;
    const int oh = t % p.Ho;
    t /= p.Ho;
    const int od = t % p.Do;
    const int n = t / p.Do;
    const int id = od * p.sd - p.pf, ih = oh * p.sh - p.pt, iw = ow * p.sw - p.pl;
    xbase[i] = ((((long)n * p.D + id) * p.H + ih) * p.W + iw) * p.Cin;
    rd[i] = mv ? id : -(1 << 20);
    rh[i] = ih;
    rw[i] = iw;
  }
  int wrow[WR];  // element offset of this thread's weight rows, -1 past Cout
#pragma unroll
  for (int i = 0; i < WR; ++i) {
    const int co = n0 + r0 + 32 * i;
    wrow[i] = co < p.Cout ? co * p.Ktot : -1;
  }

  u32x4 xr[XR], wr[WR];
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // K walk: tile kt covers channels [c0, c0 + 64) of tap (kd, kh, kw); wk is the tap's first
  // column of the weight matrix
  int kd = 0, kh = 0, kw = 0, c0 = 0, wk = 0;
  auto load_tile = [&]() {
    const int ci = c0 + kc * 8;
    const bool cv = ci < p.Cin;  // the tap's last tile: channels past Cin are zeros
    const long toff = (((long)kd * p.H + kh) * p.W + kw) * p.Cin + ci;
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const bool ok = cv && (unsigned)(rd[i] + kd) < (unsigned)p.D && (unsigned)(rh[i] + kh) < (unsigned)p.H &&
                      (unsigned)(rw[i] + kw) < (unsigned)p.W;
      xr[i] = ok ? *reinterpret_cast<const u32x4*>(p.x + (xbase[i] + toff)) : zero4;
    }
#pragma unroll
    for (int i = 0; i < WR; ++i) {
      const bool ok = cv && wrow[i] >= 0;
      wr[i] = ok ? *reinterpret_cast<const u32x4*>(p.w + (wrow[i] + wk + ci)) : zero4;
    }
    c0 += BK;
    if (c0 >= p.Cin) {
      c0 = 0;
      wk += p.Cin;
      if (++kw == p.KW) {
        kw = 0;
        if (++kh == p.KH) { kh = 0; ++kd; }
      }
    }
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

  const int nk = p.KD * p.KH * p.KW * p.ctiles;  // >= 1
  load_tile();
  store_tile();
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

  // ---- epilogue phase 2: 16-B channel-row segments; output pixel m is row m of y
  constexpr int CPR = BN / 8;  // 16-B chunks per tile row
#pragma unroll
  for (int it = 0; it < (BM * CPR + NT - 1) / NT; ++it) {
    const int q = tid + it * NT;
    const int pl = q / CPR;
    const int cc = q % CPR;
    const int m = m0 + pl;
    const int c = n0 + cc * 8;
    if (q >= BM * CPR || m >= M || c >= p.Cout) continue;
    *reinterpret_cast<bf16x8*>(p.y + ((long)m * p.ldo + p.coff + c)) = *reinterpret_cast<const bf16x8*>(Os + pl * OLD + cc * 8);
  }
}

template <int BM, int BN>
void launch_conv3d(Conv3dParams p, int act, hipStream_t s) {
  p.tiles_m = (p.M + BM - 1) / BM;
  p.tiles_n = (p.Cout + BN - 1) / BN;
  const long blocks = (long)p.tiles_m * p.tiles_n;
  if (blocks >= (1L << 31)) throw std::invalid_argument("conv3d: more than 2^31 blocks");
  const dim3 grid((unsigned)blocks), block(NT);
  switch (act) {
    case ACT_NONE: hipLaunchKernelGGL((conv3d_bf16_kernel<BM, BN, ACT_NONE>), grid, block, 0, s, p); break;
    case ACT_RELU: hipLaunchKernelGGL((conv3d_bf16_kernel<BM, BN, ACT_RELU>), grid, block, 0, s, p); break;
    case ACT_RELU6: hipLaunchKernelGGL((conv3d_bf16_kernel<BM, BN, ACT_RELU6>), grid, block, 0, s, p); break;
    default: throw std::invalid_argument("conv3d: act must be none, relu or relu6");
  }
}

// Tile configurations: 0 = 128 pixels x 128 channels, 1 = 256 pixels x 64 channels.
constexpr int NCFG = 2;

struct Pool3dParams {
  const bf16* x;
  bf16* y;
  int D, H, W, C, Do, Ho, Wo;
  int kd, kh, kw, sd, sh, sw, pf, pt, pl, ldo, coff;
  int cv;      // 8-channel vectors per pixel
  long total;  // N * Do * Ho * Wo * cv threads
};

template <bool AVG>
__global__ __launch_bounds__(NT) void pool3d_bf16_kernel(const Pool3dParams p) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= p.total) return;
  const int c = (int)(idx % p.cv) * 8;
  long m = idx / p.cv;  // output pixel
  const long pix = m;
  const int ow = (int)(m % p.Wo);
  m /= p.Wo;
  const int oh = (int)(m % p.Ho);
  m /= p.Ho;
  const int od = (int)(m % p.Do);
  const long n = m / p.Do;
  const int d0 = od * p.sd - p.pf, h0 = oh * p.sh - p.pt, w0 = ow * p.sw - p.pl;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = AVG ? 0.f : -__builtin_inff();
  int cnt = 0;
  for (int i = 0; i < p.kd; ++i) {
    const int id = d0 + i;
    if ((unsigned)id >= (unsigned)p.D) continue;
    for (int j = 0; j < p.kh; ++j) {
      const int ih = h0 + j;
      if ((unsigned)ih >= (unsigned)p.H) continue;
      const long rowoff = ((n * p.D + id) * p.H + ih) * p.W;
      for (int k = 0; k < p.kw; ++k) {
        const int iw = w0 + k;
        if ((unsigned)iw >= (unsigned)p.W) continue;
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(p.x + ((rowoff + iw) * p.C + c));
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = AVG ? acc[e] + bf2f(v[e]) : fmaxf(acc[e], bf2f(v[e]));
        ++cnt;
      }
    }
  }
  bf16x8 o;
  const float fc = (float)cnt;  // >= 1: the launcher checks that every window meets the input
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = f2bf(AVG ? acc[e] / fc : acc[e]);
  *reinterpret_cast<bf16x8*>(p.y + (pix * p.ldo + p.coff + c)) = o;
}

}  // namespace

// cfg: -1 = chosen here (256 x 64 for Cout <= 64, where a 128-channel tile would waste half of
// its MFMAs), else the tile configuration: measurement and tests only.  w_elems is the element
// count of the packed weight tensor, checked against the geometry.
void conv3d_ndhwc_bf16(uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t y, int N, int D, int H, int W, int Cin,
                       int Do, int Ho, int Wo, int Cout, int KD, int KH, int KW, int sd, int sh, int sw, int pf, int pt,
                       int pl, int act, int ldo, int coff, long w_elems, int cfg, uintptr_t stream) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0 || Cout <= 0)
    throw std::invalid_argument("conv3d: empty problem");
  if (Cin % 8 || Cout % 8 || ldo % 8 || coff % 8) throw std::invalid_argument("conv3d: Cin, Cout, ldo, coff must be multiples of 8");
  if (coff < 0 || coff + Cout > ldo) throw std::invalid_argument("conv3d: channel slot exceeds the output row");
  if (KD < 1 || KH < 1 || KW < 1 || KD > 7 || KH > 7 || KW > 7) throw std::invalid_argument("conv3d: filter extents must be 1..7");
  if (sd < 1 || sh < 1 || sw < 1 || sd > 4 || sh > 4 || sw > 4) throw std::invalid_argument("conv3d: strides must be 1..4");
  if (pf < 0 || pt < 0 || pl < 0 || pf >= KD || pt >= KH || pl >= KW) throw std::invalid_argument("conv3d: pads must be below the filter size");
  // every output pixel's tap (pf, pt, pl)-corner window starts at or in front of the input's end
  if ((long)(Do - 1) * sd - pf >= D || (long)(Ho - 1) * sh - pt >= H || (long)(Wo - 1) * sw - pl >= W)
    throw std::invalid_argument("conv3d: output extent reads past the input");
  if (!x || !w || !bias || !y) throw std::invalid_argument("conv3d: null pointer (pass zeros for no bias)");
  if (x % 16 || w % 16 || y % 16 || bias % 16) throw std::invalid_argument("conv3d: pointers must be 16-byte aligned");
  if (act != ACT_NONE && act != ACT_RELU && act != ACT_RELU6) throw std::invalid_argument("conv3d: act must be none, relu or relu6");
  if (cfg < -1 || cfg >= NCFG) throw std::invalid_argument("conv3d: unknown tile configuration " + std::to_string(cfg));
  if (w_elems != (long)KD * KH * KW * Cout * Cin) throw std::invalid_argument("conv3d: packed weights do not match the geometry");
  if (w_elems >= (1L << 31)) throw std::invalid_argument("conv3d: weights too large for 32-bit indexing");
  const long M = (long)N * Do * Ho * Wo;
  if (M >= (1L << 31)) throw std::invalid_argument("conv3d: more than 2^31 output pixels");
  Conv3dParams p{};
  p.x = reinterpret_cast<const bf16*>(x);
  p.w = reinterpret_cast<const bf16*>(w);
  p.bias = reinterpret_cast<const float*>(bias);
  p.y = reinterpret_cast<bf16*>(y);
  p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Do = Do; p.Ho = Ho; p.Wo = Wo; p.Cout = Cout;
  p.KD = KD; p.KH = KH; p.KW = KW; p.sd = sd; p.sh = sh; p.sw = sw; p.pf = pf; p.pt = pt; p.pl = pl;
  p.ldo = ldo; p.coff = coff;
  p.M = (int)M;
  p.Ktot = KD * KH * KW * Cin;
  p.ctiles = (Cin + BK - 1) / BK;
  auto s = reinterpret_cast<hipStream_t>(stream);
  if (cfg < 0) cfg = Cout <= 64 ? 1 : 0;
  if (cfg == 0) launch_conv3d<128, 128>(p, act, s);
  else launch_conv3d<256, 64>(p, act, s);
  FTM_CHECK_LAUNCH();
}

// mode: 0 = max, 1 = average over the window elements inside the input.
void pool3d_ndhwc_bf16(uintptr_t x, uintptr_t y, int N, int D, int H, int W, int C, int Do, int Ho, int Wo, int kd, int kh,
                       int kw, int sd, int sh, int sw, int pf, int pt, int pl, int mode, int ldo, int coff,
                       uintptr_t stream) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0)
    throw std::invalid_argument("pool3d: empty problem");
  if (C % 8 || ldo % 8 || coff % 8) throw std::invalid_argument("pool3d: C, ldo, coff must be multiples of 8");
  if (coff < 0 || coff + C > ldo) throw std::invalid_argument("pool3d: channel slot exceeds the output row");
  if (kd < 1 || kh < 1 || kw < 1 || kd > 8 || kh > 8 || kw > 8) throw std::invalid_argument("pool3d: window extents must be 1..8");
  if (sd < 1 || sh < 1 || sw < 1 || sd > 8 || sh > 8 || sw > 8) throw std::invalid_argument("pool3d: strides must be 1..8");
  if (pf < 0 || pt < 0 || pl < 0 || pf >= kd || pt >= kh || pl >= kw) throw std::invalid_argument("pool3d: pads must be below the window size");
  // every window holds at least one input element: it starts before the input's end (and, with
  // pad < window, ends behind its start)
  if ((long)(Do - 1) * sd - pf >= D || (long)(Ho - 1) * sh - pt >= H || (long)(Wo - 1) * sw - pl >= W)
    throw std::invalid_argument("pool3d: a window lies outside the input");
  if (!x || !y) throw std::invalid_argument("pool3d: null pointer");
  if (x % 16 || y % 16) throw std::invalid_argument("pool3d: pointers must be 16-byte aligned");
  if (mode != 0 && mode != 1) throw std::invalid_argument("pool3d: mode must be 0 (max) or 1 (avg)");
  Pool3dParams p{};
  p.x = reinterpret_cast<const bf16*>(x);
  p.y = reinterpret_cast<bf16*>(y);
  p.D = D; p.H = H; p.W = W; p.C = C; p.Do = Do; p.Ho = Ho; p.Wo = Wo;
  p.kd = kd; p.kh = kh; p.kw = kw; p.sd = sd; p.sh = sh; p.sw = sw; p.pf = pf; p.pt = pt; p.pl = pl;
  p.ldo = ldo; p.coff = coff;
  p.cv = C / 8;
  p.total = (long)N * Do * Ho * Wo * p.cv;
  const long blocks = (p.total + NT - 1) / NT;
  if (blocks >= (1L << 31)) throw std::invalid_argument("pool3d: more than 2^31 blocks");
  auto s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)blocks), block(NT);
  if (mode == 1) hipLaunchKernelGGL((pool3d_bf16_kernel<true>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((pool3d_bf16_kernel<false>), grid, block, 0, s, p);
  FTM_CHECK_LAUNCH();
}

void register_conv3d(pybind11::module_& m) {
  m.def("conv3d_ndhwc_bf16", &conv3d_ndhwc_bf16);
  m.def("pool3d_ndhwc_bf16", &pool3d_ndhwc_bf16);
  m.attr("conv3d_num_configs") = NCFG;
}
