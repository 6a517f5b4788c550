// Causal multi-head self-attention forward (flash-style, online softmax) for transformers over an
// ordered history (next-item / next-event models, GPT-style scoring): query i of a sequence
// attends key j iff j <= i and key j is not padding.
//
// Same buffers as attention.hip: qkv [T = B*S, 3*H*64] bf16 from the fused QKV projection GEMM
// (Q | K | V column blocks, head h at columns h*64), key-padding mask from the token ids
// (id == pad_id -> masked), ctx [T, H*64] bf16.  A query with no admissible key gets a zero row.
//
// Work split: one workgroup = one (batch, head, 64-query block), four waves x 16 query rows, Q
// fragments resident in registers.  The workgroup walks the key blocks 0 .. qb (its diagonal
// block) and never touches a key past the diagonal, so query block qb costs qb + 1 steps; the grid
// is ordered heaviest query block first, so the launch tail is made of one- and two-step blocks.
//
// Pipeline: K/V are double-buffered in LDS.  At step j the global loads of block j + 1 (2 K + 2 V
// 16-B chunks and one id per thread) are issued into registers, then ONE barrier publishes buffer
// j & 1 (written during step j - 1) and retires every read of the other buffer; the MFMAs of block
// j run while the loads fly, and the registers are written to buffer (j + 1) & 1 after them.
//
// K rows are chunk-swizzled (conflict-free b128 fragment reads), V is consumed through
// ds_read_b64_tr_b16, P reaches the PV operand through a per-wave P^T tile, both products run on
// v_mfma_f32_16x16x32_bf16, the online softmax works in the exp2 domain with fp32 statistics.
//
// Diagonal block: wave w owns queries 16w .. 16w+15 of the block, so it multiplies only the key
// fragments n <= w, runs the key > query compare only in fragment n == w (fragments n < w lie
// wholly below the diagonal) and only the PV steps those fragments reach.  Off-diagonal blocks run
// no causal compare at all; the key-padding mask applies everywhere.
#include <pybind11/pybind11.h>

#include <climits>
#include <stdexcept>

#include "attention_tiles.h"
#include "common.h"

namespace {

using namespace attn;

constexpr int QB = 64;      // queries per workgroup
constexpr int KB = 64;      // keys per step
constexpr int NTH = 256;    // 4 waves
constexpr int MAX_S = 2048;

// One thread's share of a key block in flight: chunks tid and tid + 256 of the 64 x 8 16-B chunks
// of K and of V, and (threads 0..63) the key's mask term.
struct Staged {
  u32x4 k[2], v[2];
  float mask;
};

FTM_DEVICE void load_block(Staged& st, const bf16* __restrict__ kbase, const int* __restrict__ ids, int kb, int S,
                           int ld, int HD, int pad_id, int tid) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int q = tid + it * NTH;
    const int kg = kb * KB + (q >> 3);
    st.k[it] = u32x4{0u, 0u, 0u, 0u};
    st.v[it] = u32x4{0u, 0u, 0u, 0u};
    if (kg < S) {
      const bf16* row = kbase + (size_t)kg * ld + (q & 7) * 8;
      st.k[it] = *reinterpret_cast<const u32x4*>(row);
      st.v[it] = *reinterpret_cast<const u32x4*>(row + HD);
    }
  }
  st.mask = 0.f;
  if (tid < KB) {
    const int kg = kb * KB + tid;
    st.mask =(kg < S && ids[kg] != pad_id) ? 0.f : -INFINITY;
  }
}

FTM_DEVICE void store_block(const Staged& st, bf16* Ks, bf16* Vs, float* km, int tid) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int q = tid + it * NTH;
    const int key = q >> 3, ch = q & 7;
    *reinterpret_cast<u32x4*>(Ks + kswz(key, ch)) = st.k[it];
    *reinterpret_cast<u32x4*>(Vs + key * VP + ch * 8) = st.v[it];
  }
  if (tid < KB) km[tid] = st.mask;
}

// One key block for one wave: NF key fragments of 16 (4 off the diagonal; w + 1 on it, where the
// last one, n == NF - 1, straddles the diagonal and takes the causal compare).
template <int NF, bool DIAG>
FTM_DEVICE void key_block(const bf16* Ks, const bf16* Vs, const float* km, bf16* ps, const bf16x8 (&qa)[2],
                          f32x4 (&o)[4], float (&mrow)[4], float (&lrow)[4], int lane, float scale_log2e) {
  constexpr int NKS = (NF + 1) / 2;  // PV steps of 32 keys
  const int col = lane & 15, rbase = (lane >> 4) * 4;
  // ---- S = Q K^T: lane holds S[q = rbase + r][key = n*16 + col]
  f32x4 s[NF];
#pragma unroll
  for (int n = 0; n < NF; ++n) {
    s[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + kswz(n * 16 + col, ks * 4 + (lane >> 4)));
      s[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[ks], kf, s[n], 0, 0, 0);
    }
  }
  float mnew[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float mx = -INFINITY;
#pragma unroll
    for (int n = 0; n < NF; ++n) {
      float v = s[n][r] * scale_log2e + km[n * 16 + col];
      if (DIAG && n == NF - 1 && col > rbase + r) v = -INFINITY;  // key > query, same 16 x 16 tile
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
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[n][r] *= alpha[r];
  // ---- P^T -> per-wave LDS tile [key][16 q]: a lane's 4 rows are 4 consecutive q of one key, one
  // 8-byte store per fragment; a fragment past the diagonal that a PV step still reads is zeros
#pragma unroll
  for (int n = 0; n < NF; ++n) {
    bf16x4 pk;
    pk[0] = f2bf(s[n][0]); pk[1] = f2bf(s[n][1]); pk[2] = f2bf(s[n][2]); pk[3] = f2bf(s[n][3]);
    *reinterpret_cast<bf16x4*>(ps + (n * 16 + col) * QP + rbase) = pk;
  }
  if constexpr (NF < 2 * NKS)
    *reinterpret_cast<bf16x4*>(ps + (NF * 16 + col) * QP + rbase) = bf16x4{f2bf(0.f), f2bf(0.f), f2bf(0.f), f2bf(0.f)};
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's P writes landed
  __builtin_amdgcn_wave_barrier();
  // ---- O += P V  (A = P[q][key] and B = V[key][d], both by transposed reads)
  const int trq = (lane & 15) >> 2, trp = lane & 3;
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int key0 = ks * 32 + (lane >> 4) * 8;  // this lane group's 8 keys
    const bf16x8 pa = tr_read8(ps + (key0 + trq) * QP + trp * 4, QP);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const bf16x8 vb = tr_read8(Vs + (key0 + trq) * VP + n * 16 + trp * 4, VP);
      o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vb, o[n], 0, 0, 0);
    }
  }
}

__global__ __launch_bounds__(NTH) void attention_causal_kernel(const bf16* __restrict__ qkv,
                                                               const int* __restrict__ ids, bf16* __restrict__ out,
                                                               int BH, int S, int H, int pad_id, float scale_log2e) {
  __shared__ __attribute__((aligned(16))) bf16 Ks[2][KB * D];   // [key][d] swizzled
  __shared__ __attribute__((aligned(16))) bf16 Vs[2][KB * VP];  // [key][d] (+pad)
  __shared__ __attribute__((aligned(16))) bf16 Ps[4][KB * QP];  // per-wave P^T, reused for O staging
  __shared__ float kmask[2][KB];

  // heaviest first: the first BH workgroups take the last query block (most key blocks)
  const int qblocks = (S + QB - 1) / QB;
  const int qb = qblocks - 1 - (int)(blockIdx.x / BH);
  const int bh = blockIdx.x % BH;
  const int b = bh / H, h = bh % H;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int HD = H * D, ld = 3 * HD;
  const size_t tok0 = (size_t)b * S;
  const bf16* kbase = qkv + tok0 * ld + HD + h * D;  // K of key 0; V lies HD further
  const int* idb = ids + tok0;

  Staged st;
  load_block(st, kbase, idb, 0, S, ld, HD, pad_id, tid);

  // Q fragments for this wave's 16 rows (A operand: row = lane&15, k = 8*(lane>>4) + j)
  const int qrow = qb * QB + wave * 16 + (lane & 15);
  bf16x8 qa[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    if (qrow < S)
      qa[ks] = *reinterpret_cast<const bf16x8*>(qkv + (tok0 + qrow) * ld + h * D + ks * 32 + (lane >> 4) * 8);
    else
      qa[ks] = bf16x8{};
  }
  f32x4 o[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrow[4], lrow[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mrow[r] = -INFINITY;
    lrow[r] = 0.f;
  }
  store_block(st, Ks[0], Vs[0], kmask[0], tid);

  bf16* ps = Ps[wave];
  for (int j = 0; j < qb; ++j) {  // blocks wholly below the diagonal
    const int cur = j & 1;
    load_block(st, kbase, idb, j + 1, S, ld, HD, pad_id, tid);
    __syncthreads();
    key_block<4, false>(Ks[cur], Vs[cur], kmask[cur], ps, qa, o, mrow, lrow, lane, scale_log2e);
    store_block(st, Ks[cur ^ 1], Vs[cur ^ 1], kmask[cur ^ 1], tid);
  }
  {  // the diagonal block
    const int cur = qb & 1;
    __syncthreads();
    switch (wave) {
      case 0: key_block<1, true>(Ks[cur], Vs[cur], kmask[cur], ps, qa, o, mrow, lrow, lane, scale_log2e); break;
      case 1: key_block<2, true>(Ks[cur], Vs[cur], kmask[cur], ps, qa, o, mrow, lrow, lane, scale_log2e); break;
      case 2: key_block<3, true>(Ks[cur], Vs[cur], kmask[cur], ps, qa, o, mrow, lrow, lane, scale_log2e); break;
      default: key_block<4, true>(Ks[cur], Vs[cur], kmask[cur], ps, qa, o, mrow, lrow, lane, scale_log2e); break;
    }
  }

  // ---- normalise, stage the wave's [16 q][64 d] tile in its P slot, store 128-B rows
  bf16* os = ps;
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float inv = lrow[r] > 0.f ? 1.f / lrow[r] : 0.f;
#pragma unroll
    for (int n = 0; n < 4; ++n) os[((lane >> 4) * 4 + r) * OP + n * 16 + (lane & 15)] = f2bf(o[n][r] * inv);
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int c = lane + it * 64;  // 16 rows x 8 chunks
    const int r = c >> 3, ch = c & 7;
    const int q = qb * QB + wave * 16 + r;
    if (q < S)
      *reinterpret_cast<u32x4*>(out + (tok0 + q) * HD + h * D + ch * 8) =
          *reinterpret_cast<const u32x4*>(os + r * OP + ch * 8);
  }
}

// ---------------------------------------------------------------------------------------------
// Head dims 32 and 128 (tile<DH>, key_step and store_ctx of attention_tiles.h): the same
// double-buffered pipeline, four waves, heaviest query block first, with the key block KB chosen so
// that one ring stage stays 512 16-B chunks of K and of V (two of each per thread, as at 64):
//   DH = 32:  a workgroup owns the head pair (2p, 2p+1) and 32 queries: wave w is head w & 1 and
//             query group w >> 1.  KB = 64 keys of 128-B pair rows; LDS as at 64 (44.5 KB, three
//             workgroups per CU).  An odd H: as in attention.hip, the absent head is zeros in LDS
//             and is not stored.
//   DH = 128: one head, 64 queries, 256-B rows, and KB = 32: the ring is 2 x (8 + 9 KB) and the
//             four P/O slots 17 KB (sized by the 16 x 136 O tile), 52 KB in all, three workgroups
//             per CU; KB = 64 would take 86 KB and leave one workgroup of four waves on a CU.
// QB and KB differ now, so the diagonal is walked per 16-key FRAGMENT: wave rows start at fragment
// fd = (qb QB) / 16 + query group, and in key block j (fragments j F .. j F + F - 1, F = KB / 16) the
// wave multiplies nf = fd + 1 - j F fragments: nf > F is a block wholly below its diagonal, 1 <= nf
// <= F holds its diagonal tile as the last fragment, nf <= 0 lies above it and is skipped (the wave
// still stages and meets the barrier).  Blocks past the end of the sequence are not walked: only
// rows >= S, which are not stored, could see them.
template <int DH, int KB>
struct StagedHd {
  u32x4 k[2], v[2];
  float mask;
};

template <int DH, int KB>
FTM_DEVICE void load_block_hd(StagedHd<DH, KB>& st, const bf16* __restrict__ kbase, const int* __restrict__ ids, int kb,
                              int S, int ld, int HD, int vch, int pad_id, int tid) {
  constexpr int NCH = tile<DH>::NCH;
  static_assert(KB * NCH == 2 * NTH, "two K and two V chunks per thread and stage");
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int q = tid + it * NTH;
    const int kg = kb * KB + q / NCH, ch = q % NCH;
    st.k[it] = u32x4{0u, 0u, 0u, 0u};
    st.v[it] = u32x4{0u, 0u, 0u, 0u};
    if (kg < S && ch < vch) {
      const bf16* row = kbase + (size_t)kg * ld + ch * 8;
      st.k[it] = *reinterpret_cast<const u32x4*>(row);
      st.v[it] = *reinterpret_cast<const u32x4*>(row + HD);
    }
  }
  st.mask = 0.f;
  if (tid < KB) {
    const int kg = kb * KB + tid;
    st.mask = (kg < S && ids[kg] != pad_id) ? 0.f : -INFINITY;
  }
}

template <int DH, int KB>
FTM_DEVICE void store_block_hd(const StagedHd<DH, KB>& st, bf16* Ks, bf16* Vs, float* km, int tid) {
  using T = tile<DH>;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int q = tid + it * NTH;
    const int key = q / T::NCH, ch = q % T::NCH;
    *reinterpret_cast<u32x4*>(Ks + T::kswz(key, ch)) = st.k[it];
    *reinterpret_cast<u32x4*>(Vs + key * T::VP + ch * 8) = st.v[it];
  }
  if (tid < KB) km[tid] = st.mask;
}

template <int DH, int KB>
__global__ __launch_bounds__(NTH) void attention_causal_hd_kernel(const bf16* __restrict__ qkv,
                                                                  const int* __restrict__ ids,
                                                                  bf16* __restrict__ out, int BG, int S, int H,
                                                                  int pad_id, float scale_log2e) {
  using T = tile<DH>;
  constexpr int HP = T::HP;
  constexpr int QBH = 64 / HP;  // queries per workgroup
  constexpr int F = KB / 16;    // fragments per key block
  constexpr int PSLOT = T::pslot(KB);
  static_assert(F == 2 || F == 4, "the fragment dispatch below");
  __shared__ __attribute__((aligned(16))) bf16 Ks[2][KB * T::RW];
  __shared__ __attribute__((aligned(16))) bf16 Vs[2][KB * T::VP];
  __shared__ __attribute__((aligned(16))) bf16 Ps[4 * PSLOT];
  __shared__ float kmask[2][KB];

  const int qblocks = (S + QBH - 1) / QBH;
  const int HG = (H + HP - 1) / HP;
  const int qb = qblocks - 1 - (int)(blockIdx.x / BG);
  const int bg = blockIdx.x % BG;
  const int b = bg / HG, h0 = (bg % HG) * HP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hp = wave % HP, qg = wave / HP;
  const int HD = H * DH, ld = 3 * HD;
  const int vch = min(HP, H - h0) * (DH / 8);
  const size_t tok0 = (size_t)b * S;
  const bf16* kbase = qkv + tok0 * ld + HD + h0 * DH;
  const int* idb = ids + tok0;

  StagedHd<DH, KB> st;
  load_block_hd<DH, KB>(st, kbase, idb, 0, S, ld, HD, vch, pad_id, tid);

  const int qrow = qb * QBH + qg * 16 + (lane & 15);
  bf16x8 qa[T::NKS];
#pragma unroll
  for (int ks = 0; ks < T::NKS; ++ks) {
    if (qrow < S && h0 + hp < H)
      qa[ks] = *reinterpret_cast<const bf16x8*>(qkv + (tok0 + qrow) * ld + (h0 + hp) * DH + ks * 32 + (lane >> 4) * 8);
    else
      qa[ks] = bf16x8{};
  }
  f32x4 o[T::NO];
#pragma unroll
  for (int n = 0; n < T::NO; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrow[4], lrow[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mrow[r] = -INFINITY;
    lrow[r] = 0.f;
  }
  store_block_hd<DH, KB>(st, Ks[0], Vs[0], kmask[0], tid);

  bf16* ps = Ps + wave * PSLOT;
  const int fd = qb * (QBH / 16) + qg;                                 // the wave's diagonal fragment
  const int nblk = min((qb * QBH + QBH - 1) / KB + 1, (S + KB - 1) / KB);  // key blocks to walk
  for (int j = 0; j < nblk; ++j) {
    const int cur = j & 1;
    const bool more = j + 1 < nblk;  // block-uniform
    if (more) load_block_hd<DH, KB>(st, kbase, idb, j + 1, S, ld, HD, vch, pad_id, tid);
    __syncthreads();
    const int nf = fd + 1 - j * F;  // wave-uniform
    if (nf > F) {
      key_step<DH, F, false>(Ks[cur], Vs[cur], kmask[cur], ps, qa, o, mrow, lrow, lane, hp, scale_log2e);
    } else if (nf == F) {
      key_step<DH, F, true>(Ks[cur], Vs[cur], kmask[cur], ps, qa, o, mrow, lrow, lane, hp, scale_log2e);
    } else if (nf == 1) {
      key_step<DH, 1, true>(Ks[cur], Vs[cur], kmask[cur], ps, qa, o, mrow, lrow, lane, hp, scale_log2e);
    } else if constexpr (F == 4) {
      if (nf == 2) key_step<DH, 2, true>(Ks[cur], Vs[cur], kmask[cur], ps, qa, o, mrow, lrow, lane, hp, scale_log2e);
      if (nf == 3) key_step<DH, 3, true>(Ks[cur], Vs[cur], kmask[cur], ps, qa, o, mrow, lrow, lane, hp, scale_log2e);
    }
    if (more) store_block_hd<DH, KB>(st, Ks[cur ^ 1], Vs[cur ^ 1], kmask[cur ^ 1], tid);
  }
  store_ctx<DH>(Ps + (wave - hp) * PSLOT, o, lrow, out + tok0 * HD + h0 * DH, HD, qb * QBH + qg * 16, S, vch, lane, hp);
}

}  // namespace

void attention_causal_fwd_bf16(uintptr_t qkv, uintptr_t ids, uintptr_t out, int B, int S, int H, int Dh, int pad_id,
                               float scale, uintptr_t stream) {
  if (Dh != 32 && Dh != 64 && Dh != 128)
    throw std::invalid_argument("attention_causal_fwd: head dim must be 32, 64 or 128");
  if (B <= 0 || H <= 0) throw std::invalid_argument("attention_causal_fwd: empty problem");
  if (S < 1 || S > MAX_S) throw std::invalid_argument("attention_causal_fwd: need 1 <= S <= 2048");
  if (!qkv || !ids || !out) throw std::invalid_argument("attention_causal_fwd: null pointer");
  // rows are H * Dh * 2 bytes, a multiple of 16 for every width: aligned bases suffice
  if (qkv % 16 || out % 16 || ids % 4) throw std::invalid_argument("attention_causal_fwd: misaligned pointers");
  const int qbh = Dh == 32 ? 32 : QB;                      // queries per workgroup
  const long long BG = (long long)B * (Dh == 32 ? (H + 1) / 2 : H);  // (batch, head group): pairs at 32
  const long long grid = BG * ((S + qbh - 1) / qbh);
  if (BG > INT_MAX || grid > INT_MAX) throw std::invalid_argument("attention_causal_fwd: grid too large");
  const auto kern = Dh == 32    ? attention_causal_hd_kernel<32, 64>
                    : Dh == 128 ? attention_causal_hd_kernel<128, 32>
                                : attention_causal_kernel;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NTH), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const bf16*>(qkv), reinterpret_cast<const int*>(ids),
                     reinterpret_cast<bf16*>(out), (int)BG, S, H, pad_id, scale * 1.4426950408889634f);
  FTM_CHECK_LAUNCH();
}

void register_attention_causal(pybind11::module_& m) { m.def("attention_causal_fwd_bf16", &attention_causal_fwd_bf16); }
