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

}  // namespace

void attention_causal_fwd_bf16(uintptr_t qkv, uintptr_t ids, uintptr_t out, int B, int S, int H, int Dh, int pad_id,
                               float scale, uintptr_t stream) {
  if (Dh != D) throw std::invalid_argument("attention_causal_fwd: head dim must be 64");
  if (B <= 0 || H <= 0) throw std::invalid_argument("attention_causal_fwd: empty problem");
  if (S < 1 || S > MAX_S) throw std::invalid_argument("attention_causal_fwd: need 1 <= S <= 2048");
  if (!qkv || !ids || !out) throw std::invalid_argument("attention_causal_fwd: null pointer");
  if (qkv % 16 || out % 16 || ids % 4) throw std::invalid_argument("attention_causal_fwd: misaligned pointers");
  const long long grid = (long long)B * H * ((S + QB - 1) / QB);
  if ((long long)B * H > INT_MAX || grid > INT_MAX) throw std::invalid_argument("attention_causal_fwd: grid too large");
  hipLaunchKernelGGL(attention_causal_kernel, dim3((unsigned)grid), dim3(NTH), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const bf16*>(qkv), reinterpret_cast<const int*>(ids),
                     reinterpret_cast<bf16*>(out), B * H, S, H, pad_id, scale * 1.4426950408889634f);
  FTM_CHECK_LAUNCH();
}

void register_attention_causal(pybind11::module_& m) { m.def("attention_causal_fwd_bf16", &attention_causal_fwd_bf16); }
