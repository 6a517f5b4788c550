// Fused ResNet bottleneck boundary in the 64/256-channel stage (ResNet-50 stage 1):
//
//   y3  = relu(x2 . W3^T + b3 + r)        1x1 expand 64 -> 256 with residual (block k)
//   y1  = relu(y3 . W1^T + b1)            1x1 reduce 256 -> CN              (block k + 1)
//
// CN = 64 inside stage 1, CN = 128 where stage 1 hands over to stage 2 (ResNet v1.5 keeps
// stage 2's first 1x1 at stride 1).  The first block's expand conv, whose shortcut is a
// stride-1 projection of the block input, runs as the dual variant: K = 64 + 64 over
// [x2 | x] (the projection never reaches HBM) and no residual read.  Unfused, the 256-channel y3 (411 MB at micro-batch
// 256 x 56 x 56) is written by one kernel and read back whole by the next; here each tile
// of y3 is produced into LDS, stored once (it is still the next block's residual) and
// consumed from LDS by the reduce GEMM.  Persistent: one workgroup per CU (8 waves) keeps
// its share of BOTH weight matrices in VGPRs and streams pixel tiles (TP = 128 for CN 64,
// 64 for CN 128):
//
//   VGPR  wave w: the W3 rows of y3 channels 32w .. 32w + 31 (MFMA A fragments, 16 or 32
//         registers) and the W1 rows of one 16-channel fragment of y1 (32 registers), with
//         their biases: no weight is read from LDS
//   LDS   X: two x2 stages [TP][CM] | O: y1 staging [TP][CN] | Y tile [TP][256]  = 64 KB
//         (CN 128), 112 KB (CN 64), 72 KB (dual); 16-B chunks XOR-swizzled per row so every
//         ds_read_b128 fragment read is bank-conflict free
//   top      barrier; y1 of the previous tile out of O (coalesced 16-B stores); the next
//            tile's x2 rows -> registers
//   phase 1  wave w x (32 channels x TP pixels), K = CM; acc + b3 -> bf16 into Y
//   pass     coalesced 16-B chunks: Y + r -> relu -> y3 global store, and back into Y; then
//            the next tile's residual rows -> registers
//   phase 2  wave w x (one channel fragment x TP / WPC pixels), K = 256; + b1, relu -> O;
//            the next tile's x2 registers -> the other X stage
//   three barriers per tile (top, after phase 1, after the pass).
//
// Schedule.  Each MFMA loop reads the B fragments of step s + 1 into a second register set
// before the MFMAs of step s issue (sched_barrier pins that order), so the waits in front
// of the MFMAs are counted lgkmcnt waits for reads issued a step earlier; the pass issues
// its Y reads in groups of four before finishing the first.  Global loads and stores are
// branch-free buffer operations (see the descriptors below), so the two register
// prefetches are awaited with counted vmcnt waits and no wave waits for a store it has
// just issued.
#include <pybind11/pybind11.h>

#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "common.h"

namespace {

constexpr int CX = 64;    // channels of each GEMM-1 source (x2, and the shortcut input xs)
constexpr int CO = 256;   // y3 channels
constexpr int NT = 512;   // threads (8 waves)

// 16-B chunk index in a row-major LDS tile, XOR-swizzled per row so 16 consecutive rows
// read at the same logical chunk land on distinct banks
template <int CPR>
FTM_DEVICE int swz(int row, int c) {
  if constexpr (CPR == 8) return row * 8 + (c ^ ((row >> 1) & 7));
  else return row * CPR + (c ^ (row & 15));
}

// LDS bytes: two x2 stages [TP][CM], the y1 staging tile O [TP][CN], the Y tile [TP][256]
template <int TP, int CN, bool DUAL>
constexpr int tail_lds_bytes() {
  constexpr int CM = DUAL ? 2 * CX : CX;
  return 2 * TP * CM * 2 + TP * CN * 2 + TP * CO * 2;
}

// TP pixels per tile, CN channels of the reduce output y1 (64 within stage 1, 128 for the
// stage-2 entry block).  DUAL: stage 1's first block, whose shortcut is a stride-1 1x1
// projection of the block input xs instead of an identity residual — GEMM 1 runs over
// K = 64 + 64 ([x2 | xs] . [W3 | Wsc]^T, bias summed) and there is no residual read.
template <int TP, int CN, bool DUAL>
__global__ __launch_bounds__(NT, 1) void bottleneck_tail_kernel(const bf16* __restrict__ x2, const bf16* __restrict__ xs,
                                                                const bf16* __restrict__ res,
                                                                const bf16* __restrict__ w3, const float* __restrict__ b3,
                                                                const bf16* __restrict__ w1, const float* __restrict__ b1,
                                                                bf16* __restrict__ y3, bf16* __restrict__ y1, int M,
                                                                int dec_h, int dec_w) {
  constexpr int CM = DUAL ? 2 * CX : CX;  // GEMM-1 depth
  constexpr int KS1 = CM / 32;            // phase-1 K-steps
  constexpr int KS2 = CO / 32;            // phase-2 K-steps
  constexpr int XB = TP * CM * 2;         // one x2 stage
  constexpr int OB = TP * CN * 2;         // y1 staging tile
  constexpr int XCH = TP * CM / 8, OCH = TP * CN / 8, YCH = TP * CO / 8;
  constexpr int PF = TP / 16;        // 16-pixel fragments per tile
  constexpr int G1 = PF > 4 ? 2 : 4; // phase 1: pixel fragments read per pipeline step (registers)
  constexpr int NG = PF / G1;        // phase-1 steps per K-step
  constexpr int CF = CN / 16;        // phase-2 channel fragments (4 or 8)
  constexpr int WPC = 8 / CF;        // waves per channel fragment (2 or 1)
  constexpr int PPW = PF / WPC;      // phase-2 pixel fragments per wave (2 or 4)
  static_assert(CF * WPC == 8 && PPW * WPC == PF && NG * G1 == PF && XCH % NT == 0 && OCH % NT == 0 && YCH % NT == 0,
                "tile shape");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  u32x4* Os = reinterpret_cast<u32x4*>(smem + 2 * XB);
  u32x4* Ys = reinterpret_cast<u32x4*>(smem + 2 * XB + OB);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int prow = lane & 15, kg = lane >> 4;
  const int ntiles = (M + TP - 1) / TP;
  if ((int)blockIdx.x >= ntiles) return;  // block-uniform, before any barrier

  // ---- resident weights in VGPRs (1x1 OHWI = row-major [co][ci]): the MFMA A fragments of
  // this wave's 32 y3 channels (w3 [256][CM]) and of its phase-2 channel fragment
  // (w1 [CN][256]), with their biases
  constexpr int XC = CM / 8;  // 16-B chunks per X row
  bf16x8 wa[2][KS1], wb[KS2];
  f32x4 bv3[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int co = wave * 32 + i * 16;
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks)
      wa[i][ks] = *reinterpret_cast<const bf16x8*>(w3 + (size_t)(co + prow) * CM + ks * 32 + kg * 8);
    bv3[i] = *reinterpret_cast<const f32x4*>(b3 + co + kg * 4);
  }
  const int cf = wave / WPC;           // phase-2 channel fragment
  const int pf0 = (wave % WPC) * PPW;  // phase-2 first pixel fragment
#pragma unroll
  for (int ks = 0; ks < KS2; ++ks)
    wb[ks] = *reinterpret_cast<const bf16x8*>(w1 + (size_t)(cf * 16 + prow) * CO + ks * 32 + kg * 8);
  const f32x4 bv1 = *reinterpret_cast<const f32x4*>(b1 + cf * 16 + kg * 4);

  // Global traffic goes through raw buffer descriptors: a load past the buffer returns
  // zeros and a store past it is dropped, so the partial tile, the decimated y3 store and
  // the tile after the last need no branch.  Every wave then issues the same loads and
  // stores per tile, and each register prefetch is waited for with a counted vmcnt that
  // leaves the younger stores and loads in flight (a branch around any of them forces
  // vmcnt(0): a store acknowledgement awaited every tile)
  auto rsrc = [](const void* ptr, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ptr), 0, (int)bytes, 0x00020000);
  };
  constexpr unsigned DROP = 0xFFFFFF00u;  // an offset past every buffer (each is below 2^32 - 512 bytes)
  const unsigned y3rows = dec_w ? (unsigned)M / 4u : (unsigned)M;
  const __amdgpu_buffer_rsrc_t rx2 = rsrc(x2, (unsigned)M * CX * 2u), rxs = rsrc(DUAL ? xs : x2, (unsigned)M * CX * 2u);
  const __amdgpu_buffer_rsrc_t rres = rsrc(DUAL ? (const bf16*)y3 : res, (unsigned)M * CO * 2u);
  const __amdgpu_buffer_rsrc_t ry3 = rsrc(y3, y3rows * CO * 2u), ry1 = rsrc(y1, (unsigned)M * CN * 2u);

  constexpr int XIT = XCH / NT;
  u32x4 xr[XIT];
  auto load_x = [&](int t) {  // tiles past the last read zeros
#pragma unroll
    for (int it = 0; it < XIT; ++it) {
      const int q = tid + it * NT;
      const unsigned px = (unsigned)(t * TP + q / XC), c = q % XC;
      const unsigned off = px < (unsigned)M ? px * (CX * 2u) + (c & 7) * 16u : DROP;
      xr[it] = __builtin_amdgcn_raw_buffer_load_b128((DUAL && c >= 8) ? rxs : rx2, off, 0, 0);
    }
  };
  auto store_x = [&](int stage) {
    u32x4* Xn = reinterpret_cast<u32x4*>(smem + stage * XB);
#pragma unroll
    for (int it = 0; it < XIT; ++it) {
      const int q = tid + it * NT;
      Xn[swz<XC>(q / XC, q % XC)] = xr[it];
    }
  };
  // y1 of the previous tile out of O (coalesced 16-B chunks)
  auto store_y1 = [&](int pt) {
#pragma unroll
    for (int it = 0; it < OCH / NT; ++it) {
      const int q = tid + it * NT;
      const int pl = q / (CN / 8), c = q % (CN / 8);
      const unsigned px = (unsigned)(pt * TP + pl);  // pt = -1 (no tile yet): dropped
      __builtin_amdgcn_raw_buffer_store_b128(Os[swz<CN / 8>(pl, c)], ry1,
                                             pt >= 0 && px < (unsigned)M ? px * (CN * 2u) + c * 16u : DROP, 0, 0);
    }
  };

  // residual rows of a tile, 16-B chunks in the pass's thread order; loaded one tile ahead
  // (after the previous tile's pass has used the registers) so the pass never waits on HBM
  constexpr int YIT = YCH / NT;
  constexpr int YG = 4;  // pass: chunks read ahead as one group
  static_assert(NT / (CO / 8) == 16 && YIT % YG == 0, "pass: 16 pixels per iteration, groups of YG");
  u32x4 rv[YIT];
  auto load_r = [&](int tt) {
#pragma unroll
    for (int it = 0; it < YIT; ++it) {
      const int q = tid + it * NT;
      const unsigned px = (unsigned)(tt * TP + (q >> 5));
      if constexpr (DUAL) rv[it] = u32x4{0u, 0u, 0u, 0u};
      else rv[it] = __builtin_amdgcn_raw_buffer_load_b128(rres, px < (unsigned)M ? px * (CO * 2u) + (q & 31) * 16u : DROP, 0, 0);
    }
  };

  const int nwg = gridDim.x;  // read once: the asm memory clobber below would reload it per tile
  int t = blockIdx.x;
  int stage = 0;
  int prev = -1;  // tile whose y1 waits in O
  load_r(t);
  load_x(t);
  store_x(0);
  while (true) {
    const int p0 = t * TP;
    // this tile's x2 stage and the previous tile's O (the last LDS writes before the loop's
    // back edge) are written: the wait is explicit because the compiler's own lgkmcnt wait
    // for a barrier at a loop's head has been missing on the back edge (bottleneck_chain.hip)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    store_y1(prev);  // O is read before phase 2 rewrites it (two barriers between)
    const int tn = t + nwg;
    const bool more = tn < ntiles;
    load_x(tn);  // the next tile's x2, in flight during this whole tile
    const u32x4* Xs = reinterpret_cast<const u32x4*>(smem + stage * XB);
    // ---- phase 1: y3 tile = x2 tile . W3^T  (wave: channels 32*wave .. +32, all TP px).
    // Step s = (K-step s / NG, pixel fragments G1 (s % NG) ..): the X fragments of step s + 1
    // are read into the other half of xb before the MFMAs of step s issue
    f32x4 acc[2][PF];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < PF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
      bf16x8 xb[2][G1];
      auto read_x = [&](int s, bf16x8(&dst)[G1]) {
        const int c = (s / NG) * 4 + kg, j0 = (s % NG) * G1;
#pragma unroll
        for (int g = 0; g < G1; ++g) dst[g] = __builtin_bit_cast(bf16x8, Xs[swz<XC>((j0 + g) * 16 + prow, c)]);
      };
      read_x(0, xb[0]);
#pragma unroll
      for (int s = 0; s < KS1 * NG; ++s) {
        if (s + 1 < KS1 * NG) read_x(s + 1, xb[(s + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);  // pins the order: reads of s + 1, then MFMAs of s
        const int ks = s / NG, j0 = (s % NG) * G1;
#pragma unroll
        for (int g = 0; g < G1; ++g)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            acc[i][j0 + g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[i][ks], xb[s & 1][g], acc[i][j0 + g], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // acc[i][j][r] = channel 32*wave + 16i + 4kg + r of pixel 16j + prow: + b3 -> bf16 into Y
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int co = wave * 32 + i * 16 + kg * 4;
      const f32x4 bv = bv3[i];
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f2bf(acc[i][j][r] + bv[r]);
        const int px = j * 16 + prow;
        bf16* chunk = reinterpret_cast<bf16*>(Ys + swz<32>(px, co >> 3));
        *reinterpret_cast<bf16x4*>(chunk + (co & 7)) = o;  // 8-byte half of the chunk
      }
    }
    __syncthreads();
    // ---- pass: + residual, relu -> y3 (global) and back into Y (coalesced 16-B chunks)
    {
      // decimated y3: (n, h, w) of this thread's first pass pixel, advanced by 16 pixels per
      // iteration (one divide pair per tile, not per store)
      int dn = 0, dh = 0, dw = 0;
      if (dec_w) {
        const int o0 = p0 + (tid >> 5);
        dw = o0 % dec_w;
        const int tt = o0 / dec_w;
        dh = tt % dec_h;
        dn = tt / dec_h;
      }
      bf16x8 yv[YG];  // the Y reads of YG chunks are issued before the first of them is finished
#pragma unroll
      for (int it = 0; it < YIT; ++it) {
        if (it % YG == 0) {
#pragma unroll
          for (int g = 0; g < YG; ++g) {
            const int q = tid + (it + g) * NT;
            yv[g] = __builtin_bit_cast(bf16x8, Ys[swz<32>(q >> 5, q & 31)]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        const int q = tid + it * NT;
        const int pl = q >> 5, c = q & 31;
        const int si = swz<32>(pl, c);
        bf16x8 v = yv[it % YG];
        const bf16x8 r = __builtin_bit_cast(bf16x8, rv[it]);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = f2bf(fmaxf((float)v[e] + (float)r[e], 0.f));
        Ys[si] = __builtin_bit_cast(u32x4, v);
        int o = p0 + pl;
        bool st = o < M;
        if (dec_w) {  // decimated y3: only the even (h, w) pixels, compact [N, H/2, W/2, 256]
          if (it) {
            dw += 16;
            while (dw >= dec_w) {
              dw -= dec_w;
              if (++dh == dec_h) { dh = 0; ++dn; }
            }
          }
          st = st && !((dh | dw) & 1);
          o = (dn * (dec_h >> 1) + (dh >> 1)) * (dec_w >> 1) + (dw >> 1);
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ry3,
                                               st ? (unsigned)o * (CO * 2u) + c * 16u : DROP, 0, 0);
      }
    }
    if constexpr (!DUAL) load_r(tn);  // the next tile's residual, in flight until its pass
    __syncthreads();
    // ---- phase 2: y1 tile = relu(Y . W1^T + b1)  (wave: channel fragment cf, pixel fragments
    // pf0 .. pf0 + PPW - 1).  The Y fragments of K-step ks + 1 are read into the other half of
    // yb before the MFMAs of ks issue
    f32x4 acc2[PPW];
#pragma unroll
    for (int q = 0; q < PPW; ++q) acc2[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
      bf16x8 yb[2][PPW];
      auto read_y = [&](int ks, bf16x8(&dst)[PPW]) {
#pragma unroll
        for (int q = 0; q < PPW; ++q) dst[q] = __builtin_bit_cast(bf16x8, Ys[swz<32>((pf0 + q) * 16 + prow, ks * 4 + kg)]);
      };
      read_y(0, yb[0]);
#pragma unroll
      for (int ks = 0; ks < KS2; ++ks) {
        if (ks + 1 < KS2) read_y(ks + 1, yb[(ks + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);  // pins the order: reads of ks + 1, then MFMAs of ks
#pragma unroll
        for (int q = 0; q < PPW; ++q) acc2[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[ks], yb[ks & 1][q], acc2[q], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // stage y1 in O: acc2[q][r] = channel 16 cf + 4kg + r of pixel 16 (pf0 + q) + prow
    {
      const int co = cf * 16 + kg * 4;
#pragma unroll
      for (int q = 0; q < PPW; ++q) {
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f2bf(fmaxf(acc2[q][r] + bv1[r], 0.f));
        bf16* chunk = reinterpret_cast<bf16*>(Os + swz<CN / 8>((pf0 + q) * 16 + prow, co >> 3));
        *reinterpret_cast<bf16x4*>(chunk + (co & 7)) = o;
      }
    }
    prev = t;
    if (!more) break;
    // the next tile's x2 into the other stage: its last readers (the previous tile's phase 1)
    // are two barriers back
    store_x(stage ^ 1);
    t = tn;
    stage ^= 1;
  }
  __syncthreads();  // the last tile's O
  store_y1(prev);
}

template <int TP, int CN, bool DUAL>
void launch_tail(const bf16* x2, const bf16* xs, const bf16* res, const bf16* w3, const float* b3, const bf16* w1,
                 const float* b1, bf16* y3, bf16* y1, int M, int num_cu, hipStream_t stream, int dec_h, int dec_w) {
  const int tiles = (M + TP - 1) / TP;
  const int grid = tiles < num_cu ? tiles : num_cu;
  constexpr size_t lds = tail_lds_bytes<TP, CN, DUAL>();
  static_assert(lds <= 160 * 1024, "LDS");
  hipFuncSetAttribute((const void*)bottleneck_tail_kernel<TP, CN, DUAL>, hipFuncAttributeMaxDynamicSharedMemorySize,
                      lds);
  hipLaunchKernelGGL((bottleneck_tail_kernel<TP, CN, DUAL>), dim3(grid), dim3(NT), lds, stream, x2, xs, res, w3, b3, w1,
                     b1, y3, y1, M, dec_h, dec_w);
}


}  // namespace

// x2 [M, 64], res [M, 256] (or, dual: xs [M, 64] and no residual), w3 [256, 64] (dual:
// [256, 128] = [W3 | Wsc]), b3 [256], w1 [cn, 256], b1 [cn] -> y3 [M, 256], y1 [M, cn]
// (all bf16 rows contiguous; biases fp32); cn = 64 or 128 (128: identity residual only).
void bottleneck_tail_bf16(uintptr_t x2, uintptr_t xs, uintptr_t res, uintptr_t w3, uintptr_t b3, uintptr_t w1,
                          uintptr_t b1, uintptr_t y3, uintptr_t y1, int M, int cn, int num_cu, uintptr_t stream,
                          int dec_h, int dec_w) {
  if (M <= 0) throw std::invalid_argument("bottleneck_tail: empty problem");
  if ((long)M * CO >= (1L << 31)) throw std::invalid_argument("bottleneck_tail: tensor too large for 32-bit indexing");
  const bool dual = xs != 0;
  if (dual == (res != 0)) throw std::invalid_argument("bottleneck_tail: pass exactly one of xs (dual) and res");
  for (uintptr_t p : {x2, dual ? xs : res, w3, w1, y3, y1, b3, b1})
    if (!p || p % 16) throw std::invalid_argument("bottleneck_tail: null or non-16-byte-aligned pointer");
  // dec_h x dec_w > 0: y3 is stored decimated (its only other reader is a stride-2 1x1
  // projection shortcut, ResNet's stage-1 -> stage-2 boundary): 1/4 of the y3 bytes
  if (dec_w < 0 || dec_h < 0 || (dec_w > 0) != (dec_h > 0) || dec_w % 2 || dec_h % 2 ||
      (dec_w > 0 && M % (dec_h * dec_w)))
    throw std::invalid_argument("bottleneck_tail: decimation needs even H, W dividing the pixel count");
  auto s = reinterpret_cast<hipStream_t>(stream);
  auto bp = [](uintptr_t p) { return reinterpret_cast<bf16*>(p); };
  auto fp = [](uintptr_t p) { return reinterpret_cast<const float*>(p); };
  if (dual && cn == 64)
    launch_tail<64, 64, true>(bp(x2), bp(xs), nullptr, bp(w3), fp(b3), bp(w1), fp(b1), bp(y3), bp(y1), M, num_cu, s, dec_h, dec_w);
  else if (!dual && cn == 64)
    launch_tail<128, 64, false>(bp(x2), nullptr, bp(res), bp(w3), fp(b3), bp(w1), fp(b1), bp(y3), bp(y1), M, num_cu, s, dec_h, dec_w);
  else if (!dual && cn == 128)
    launch_tail<64, 128, false>(bp(x2), nullptr, bp(res), bp(w3), fp(b3), bp(w1), fp(b1), bp(y3), bp(y1), M, num_cu, s, dec_h, dec_w);
  else
    throw std::invalid_argument("bottleneck_tail: unsupported variant (dual " + std::to_string(dual) + ", cn " +
                                std::to_string(cn) + ")");
  FTM_CHECK_LAUNCH();
}

void register_bottleneck(pybind11::module_& m) {
  m.def("bottleneck_tail_bf16", &bottleneck_tail_bf16);
}
