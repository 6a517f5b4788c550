// LDS tile helpers shared by the attention kernels (attention.hip, attention_causal.hip,
// attention_causal_packed.hip): K rows
// chunk-swizzled for conflict-free b128 fragment reads, V and P^T read through the hardware
// transpose read as MFMA operands.  The 64-wide kernels use the constants right below; the 32- and
// 128-wide kernels use tile<DH> and the key_step / store_ctx pieces at the end of this header.
//
// Bank model used throughout: 64 banks of 4 B (one 256-B window); a 16-lane group is what one
// ds_read_b128 / ds_read_b64_tr_b16 pass serves, so the aim is that the 16 addresses of such a
// group fall into distinct 16-B (b128) or distinct 8-bank (tr-read, 32 B per row) slots of the
// window.  None of this is measured per width; it is address arithmetic.
//
//   64-wide (D, VP, OP, kswz below): a K row is 128 B = 8 chunks, so rows r and r + 2 start on the
//   same bank; chunk ^ (row & 7) spreads 8 consecutive rows of one chunk column over 8 slots.  A
//   tr-read group touches 4 consecutive V rows x 32 B; pitch 72 el = 36 banks puts them at banks
//   0, 36, 8, 44 (+8 each wide): disjoint.
//
//   32-wide (tile<32>): the LDS row is the row of a head PAIR, 2 x 32 el = 128 B = 8 chunks (head
//   hp of the pair owns chunks 4 hp .. 4 hp + 3), because a lone 64-B head row would put 4 rows
//   into one window and leave only 4 chunk values to XOR with.  A fragment read is 16 rows of one
//   chunk column; rows r, r + 1 fill the two 128-B halves of a window, so the XOR term advances
//   every second row: chunk ^ ((row >> 1) & 7) gives 16 distinct slots for 16 consecutive rows (the
//   64-wide mask repeats after 8).  The staging write (8 chunks of 2 rows per 16 lanes) is a
//   permutation within each half: distinct too.  V pitch 72 as for 64: same 4-row argument.
//
//   128-wide (tile<128>): a K row is 256 B = 16 chunks = the whole window, so unswizzled every row
//   of a chunk column hits the same slot (16-way).  chunk ^ (row & 15) is a bijection on the 16
//   slots for 16 consecutive rows.  V: pitch D + 8 = 136 el = 68 banks = 4 (mod 64) would start 4
//   consecutive rows at banks 0, 4, 8, 12 and their 8-bank reads would overlap pairwise; pitch
//   D + 16 = 144 el = 72 banks = 8 (mod 64) starts them at 0, 8, 16, 24: disjoint.
//
//   Output staging pitch OP = row + 8 el for every width: the four lane groups of an accumulator
//   store write rows 4 apart, 4 * OP * 2 B = 16 banks (mod 64) apart for 72 and for 136.
#pragma once
#include "common.h"

namespace attn {

constexpr int D = 64;       // head dim
constexpr int VP = D + 8;   // V row pitch (elements): tr-read rows land on distinct banks
constexpr int OP = D + 8;   // output staging row pitch
constexpr int QP = 16 + 4;  // P^T row pitch: [key][16 q] tiles, 40-B rows (tr-read friendly)

typedef short v4s __attribute__((ext_vector_type(4)));

FTM_DEVICE int kswz(int row, int chunk) { return row * D + ((chunk ^ (row & 7)) << 3); }

// 4 consecutive keys x 1 d column per lane (a 16-lane group reads 4 keys x 16 d columns)
FTM_DEVICE v4s tr_read(const bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)p);
}

// two transposed reads 4 rows apart -> one 8-element MFMA operand (whole-vector
// reinterpretation: element-wise short->bf16 inserts miscompile here)
FTM_DEVICE bf16x8 tr_read8(const bf16* p, int pitch) {
  const v4s lo = tr_read(p), hi = tr_read(p + 4 * pitch);
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ---------------------------------------------------------------------------------------------
// Head dims 32 and 128.  A workgroup serves HP adjacent heads of one (batch, query block): HP = 2
// at 32 (the pair's 64 columns are contiguous in qkv and in ctx, so staging and the ctx store move
// whole 128-B rows), HP = 1 at 128 (256-B rows).  Wave w of the workgroup is head hp = w % HP of
// the group and query group w / HP (16 rows).
template <int DH>
struct tile {
  // tile<64> is the 64-wide constants above (D, VP, OP, kswz) under the names of this struct, for
  // kernels templated over the head dim (attention_causal_packed.hip)
  static_assert(DH == 32 || DH == 64 || DH == 128, "head dims the attention kernels are built for");
  static constexpr int HP = DH == 32 ? 2 : 1;        // heads per workgroup = heads per LDS row
  static constexpr int RW = DH * HP;                 // LDS row width (elements): 64 or 128
  static constexpr int NCH = RW / 8;                 // 16-B chunks per row: 8 or 16
  static constexpr int VP = RW + (DH == 128 ? 16 : 8);
  static constexpr int OP = RW + 8;
  static constexpr int NKS = DH / 32;                // MFMA K-steps of S = Q K^T per key fragment
  static constexpr int NO = DH / 16;                 // output fragments per wave
  static FTM_DEVICE int kswz(int row, int chunk) {
    return row * RW + ((chunk ^ (DH == 32 ? (row >> 1) & 7 : DH == 64 ? row & 7 : row & 15)) << 3);
  }
  // per-wave P^T slot for KB keys; it must also hold the wave's share of the O staging tile
  // ([16][OP], shared by the HP waves of a query group)
  static constexpr int pslot(int KB) { return KB * QP > 16 * OP / HP ? KB * QP : 16 * OP / HP; }
};

// One key block for one wave: NF key fragments of 16 staged in Ks / Vs / km (a multiple of 32 keys
// is staged, so the PV step of an odd NF reads a zeroed P fragment against real V rows).  With
// DIAG the last fragment, n == NF - 1, is the wave's own 16 x 16 diagonal tile and takes the
// key > query compare; the fragments before it lie wholly below the diagonal.
//
// PACKED (token-packed causal attention): there is no key mask (``km`` is not read); with LOWER a
// key is also masked when it lies before the start of the row's sequence, ``key0 + key <
// start[r]`` with ``key0`` the block's first row of the token stream and ``start`` the sequence
// starts of the lane's four accumulator rows.  Both flags off is the code of the padded kernels.
template <int DH, int NF, bool DIAG, bool PACKED = false, bool LOWER = false>
FTM_DEVICE void key_step(const bf16* Ks, const bf16* Vs, const float* km, bf16* ps,
                         const bf16x8 (&qa)[tile<DH>::NKS], f32x4 (&o)[tile<DH>::NO], float (&mrow)[4],
                         float (&lrow)[4], int lane, int hp, float scale_log2e, int key0 = 0,
                         const int* start = nullptr) {
  using T = tile<DH>;
  constexpr int NPV = (NF + 1) / 2;  // PV steps of 32 keys
  const int col = lane & 15, rbase = (lane >> 4) * 4;
  // ---- S = Q K^T: lane holds S[q = rbase + r][key = n*16 + col]
  f32x4 s[NF];
#pragma unroll
  for (int n = 0; n < NF; ++n) {
    s[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < T::NKS; ++ks) {
      const bf16x8 kf =
          *reinterpret_cast<const bf16x8*>(Ks + T::kswz(n * 16 + col, hp * (DH / 8) + ks * 4 + (lane >> 4)));
      s[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[ks], kf, s[n], 0, 0, 0);
    }
  }
  float mnew[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float mx = -INFINITY;
#pragma unroll
    for (int n = 0; n < NF; ++n) {
      float v;
      if constexpr (PACKED) v = s[n][r] * scale_log2e;
      else v = s[n][r] * scale_log2e + km[n * 16 + col];
      if (DIAG && n == NF - 1 && col > rbase + r) v = -INFINITY;  // key > query, same 16 x 16 tile
      if (LOWER && key0 + n * 16 + col < start[r]) v = -INFINITY;  // key of an earlier sequence
      s[n][r] = v;
      mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    mnew[r] = fmaxf(mrow[r], mx);
  }
  float alpha[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float mref = mnew[r] == -INFINITY ? 0.f : mnew[r];
    alpha[r] = __builtin_amdgcn_exp2f(mrow[r] - mref);
    float sum = 0.f;
#pragma unroll
    for (int n = 0; n < NF; ++n) {
      const float pv = __builtin_amdgcn_exp2f(s[n][r] - mref);
      s[n][r] = pv;
      sum += pv;
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) sum += __shfl_xor(sum, off, 64);
    lrow[r] = lrow[r] * alpha[r] + sum;
    mrow[r] = mnew[r];
  }
#pragma unroll
  for (int n = 0; n < T::NO; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[n][r] *= alpha[r];
  // ---- P^T -> per-wave LDS tile [key][16 q]: a lane's 4 rows are 4 consecutive q of one key
#pragma unroll
  for (int n = 0; n < NF; ++n) {
    bf16x4 pk;
    pk[0] = f2bf(s[n][0]); pk[1] = f2bf(s[n][1]); pk[2] = f2bf(s[n][2]); pk[3] = f2bf(s[n][3]);
    *reinterpret_cast<bf16x4*>(ps + (n * 16 + col) * QP + rbase) = pk;
  }
  if constexpr (NF < 2 * NPV)
    *reinterpret_cast<bf16x4*>(ps + (NF * 16 + col) * QP + rbase) = bf16x4{f2bf(0.f), f2bf(0.f), f2bf(0.f), f2bf(0.f)};
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's P writes landed
  __builtin_amdgcn_wave_barrier();
  // ---- O += P V  (A = P[q][key] and B = V[key][d], both by transposed reads)
  const int trq = (lane & 15) >> 2, trp = lane & 3;
#pragma unroll
  for (int ks = 0; ks < NPV; ++ks) {
    const int key0 = ks * 32 + (lane >> 4) * 8;  // this lane group's 8 keys
    const bf16x8 pa = tr_read8(ps + (key0 + trq) * QP + trp * 4, QP);
#pragma unroll
    for (int n = 0; n < T::NO; ++n) {
      const bf16x8 vb = tr_read8(Vs + (key0 + trq) * T::VP + hp * DH + n * 16 + trp * 4, T::VP);
      o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vb, o[n], 0, 0, 0);
    }
  }
}

// Normalise a wave's [16 q][DH] tile into the query group's staging tile ``os`` ([16][OP]: the P
// slots of the group's HP waves, which all of them are done with) and store whole rows of the head
// group: rows q0 .. q0 + 15 below ``rows``, 16-B chunks below ``vch`` (an odd H leaves the last
// pair half a row: the absent head's columns are not written).  At HP = 2 the two waves of a query
// group meet at workgroup barriers, so every wave of the workgroup must come here.
template <int DH>
FTM_DEVICE void store_ctx(bf16* os, const f32x4 (&o)[tile<DH>::NO], const float (&lrow)[4], bf16* __restrict__ dst,
                          int ldo, int q0, int rows, int vch, int lane, int hp) {
  using T = tile<DH>;
  constexpr int CPW = 16 * T::NCH / T::HP / 64;  // 64-lane store rounds per wave: 1 or 4
  if constexpr (T::HP > 1) __syncthreads();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float inv = lrow[r] > 0.f ? 1.f / lrow[r] : 0.f;
#pragma unroll
    for (int n = 0; n < T::NO; ++n)
      os[((lane >> 4) * 4 + r) * T::OP + hp * DH + n * 16 + (lane & 15)] = f2bf(o[n][r] * inv);
  }
  if constexpr (T::HP > 1) __syncthreads();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int it = 0; it < CPW; ++it) {
    const int c = lane + (hp * CPW + it) * 64;  // 16 rows x NCH chunks
    const int r = c / T::NCH, ch = c % T::NCH;
    if (q0 + r < rows && ch < vch)
      *reinterpret_cast<u32x4*>(dst + (size_t)(q0 + r) * ldo + ch * 8) =
          *reinterpret_cast<const u32x4*>(os + r * T::OP + ch * 8);
  }
}

}  // namespace attn
