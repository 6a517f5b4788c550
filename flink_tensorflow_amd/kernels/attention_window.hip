// Sliding-window causal self-attention forward (local attention over an ordered history: long
// event streams of next-item models, long-context encoders): query i of a sequence attends key j
// iff i - W < j <= i and key j is not padding.  W >= S is plain causal attention.
//
// Same buffers as attention_causal.hip: qkv [T = B*S, 3*H*DH] bf16 from the fused QKV projection
// (Q | K | V column blocks, head h at columns h*DH), key-padding mask from the token ids (id ==
// pad_id -> masked), ctx [T, H*DH] bf16.  A query with no admissible key gets a zero row.
//
// Work split: one workgroup = one (batch, head group, query block): four waves x 16 query rows, Q
// fragments resident in registers; 64 queries of one head at DH = 64 and 128, 32 queries of the
// head pair (2p, 2p + 1) at DH = 32 (wave w: head w & 1, query group w >> 1): tile<DH> of
// attention_tiles.h, KB = 64 keys per step, 32 at DH = 128, as in attention_causal.hip.  The key
// walk starts at the block that holds key qb QB - (W - 1), clamped at 0, and ends at the block of
// the workgroup's last row that exists: at most ceil((QB + W - 1) / KB) steps whatever S is, one
// more at DH = 32, where a 32-query block can end in the middle of a 64-key block.
//
// Grid order: workgroup id = qi * BG + (batch, head group), query blocks from the LAST one down.
// Steps per workgroup are equal but for the first ceil((W - 1) / QB) query blocks, whose walk is
// clamped at key 0; going down puts those few lighter ones at the launch tail, which is all that
// is left of the causal kernel's heaviest-first order.  Within a query block the (batch, head
// group) index runs fastest, so with workgroup ids dealt round-robin over the eight XCDs and BG a
// multiple of 8, the query blocks of one (batch, head group), whose windows overlap in W - 1 keys,
// stay on one XCD's L2.  That is id arithmetic, not a measurement.
//
// Masks, per 16-key FRAGMENT and wave-uniform.  A wave's rows r0 .. r0 + 15 lie in fragment fd =
// r0 / 16 of the sequence and their windows begin in fragment fa = max(r0 - (W - 1), 0) / 16.  Of
// key block j (fragments j F .. j F + F - 1, F = KB / 16) the wave multiplies only fragments lo =
// max(fa, j F) .. hi = min(fd, j F + F - 1); none: the block lies outside the wave's windows and
// is skipped (the wave still stages and meets the barrier).  The lower edges of the 16 windows,
// keys r0 - W + 1 .. r0 - W + 16, fall into fragments fa and fa + 1 only, and key > query only in
// fragment fd.  So
//   lo > fa + 1 and hi < fd: every fragment is wholly inside every window of the wave; this is a
//     whole block and runs key_step<DH, F, false> of attention_tiles.h: no compare at all (the
//     inside of a long window);
//   else edge_step below: the fragments lo .. hi only, from fragment offset f0 = lo - j F of the
//     staged block; its first two fragments take the lower compare (key - query <= -W), its last
//     one the diagonal compare (key - query > 0), the ones between neither.  For W <= 16 one
//     fragment is both the diagonal and a lower edge and takes both.
// The key-padding mask applies everywhere.
//
// Pipeline (attention_causal.hip): K/V double-buffered in LDS; at step j the global loads of block
// j + 1 (2 K + 2 V 16-B chunks and one id per thread) are issued into registers, ONE barrier
// publishes buffer j & 1 and retires every read of the other, the MFMAs run while the loads fly,
// and the registers are written to the other buffer after them.  K rows chunk-swizzled, V through
// ds_read_b64_tr_b16, P through the per-wave P^T tile, both products on v_mfma_f32_16x16x32_bf16,
// online softmax in the exp2 domain with fp32 statistics.  With f0 = 0 an edge step issues the
// operations of key_step in key_step's order, so W >= S gives the bits of attention_causal.hip.
#include <pybind11/pybind11.h>

#include <climits>
#include <stdexcept>

#include "attention_tiles.h"
#include "common.h"

namespace {

using namespace attn;

constexpr int NTH = 256;     // 4 waves
constexpr int MAX_S = 8192;  // a choice, not a measurement: no index depends on S beyond size_t row offsets

// One thread's share of a key block in flight: two K and two V 16-B chunks, and (threads 0 .. KB - 1)
// the key's mask term.
struct Staged {
  u32x4 k[2], v[2];
  float mask;
};

template <int DH, int KB>
FTM_DEVICE void load_block(Staged& st, const bf16* __restrict__ kbase, const int* __restrict__ ids, int kb, int S,
                           int ld, int HD, int vch, int pad_id, int tid) {
  constexpr int NCH = tile<DH>::NCH;
  static_assert(KB * NCH == 2 * NTH, "two K and two V chunks per thread and stage");
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int q = tid + it * NTH;
    const int kg = kb * KB + q / NCH, ch = q % NCH;
    st.k[it] = u32x4{0u, 0u, 0u, 0u};
    st.v[it] = u32x4{0u, 0u, 0u, 0u};
    if (kg < S && ch < vch) {  // keys past the sequence and absent heads are staged as zeros
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
FTM_DEVICE void store_block(const Staged& st, bf16* Ks, bf16* Vs, float* km, int tid) {
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

// NF key fragments of the staged block for one wave, starting at fragment f0 of the block (wave-
// uniform, f0 + NF <= KB / 16).  d0 is key - query of (fragment f0, this lane's key column) and the
// lane's first accumulator row, so element (n, r) has key - query = d0 + 16 n - r: masked below
// the window when <= -W (fragments 0 and 1 of the step only) and above the diagonal when > 0 (the
// last fragment only).  The swizzle term of a K row does not change when 16 is added to the row
// (tile<DH>::kswz), so the fragments are addressed from row pointers moved by f0 fragments.  P^T
// is written at the fragments' own places in the block's [KB][16 q] tile and PV runs over the
// 32-key pairs that hold them; the fragment that completes a pair at either end is zeros.
template <int DH, int NF>
FTM_DEVICE void edge_step(const bf16* Ks, const bf16* Vs, const float* km, bf16* ps,
                          const bf16x8 (&qa)[tile<DH>::NKS], f32x4 (&o)[tile<DH>::NO], float (&mrow)[4],
                          float (&lrow)[4], int lane, int hp, float scale_log2e, int f0, int d0, int W) {
  using T = tile<DH>;
  const int col = lane & 15, rbase = (lane >> 4) * 4;
  const bf16* kf0 = Ks + f0 * 16 * T::RW;
  const float* km0 = km + f0 * 16;
  bf16* ps0 = ps + f0 * 16 * QP;
  // ---- S = Q K^T: lane holds S[q = rbase + r][key = (f0 + n)*16 + col]
  f32x4 s[NF];
#pragma unroll
  for (int n = 0; n < NF; ++n) {
    s[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < T::NKS; ++ks) {
      const bf16x8 kf =
          *reinterpret_cast<const bf16x8*>(kf0 + T::kswz(n * 16 + col, hp * (DH / 8) + ks * 4 + (lane >> 4)));
      s[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[ks], kf, s[n], 0, 0, 0);
    }
  }
  float mnew[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float mx = -INFINITY;
#pragma unroll
    for (int n = 0; n < NF; ++n) {
      float v = s[n][r] * scale_log2e + km0[n * 16 + col];
      const int d = d0 + n * 16 - r;
      if (n == NF - 1 && d > 0) v = -INFINITY;  // key > query: the diagonal fragment
      if (n < 2 && d <= -W) v = -INFINITY;      // key <= query - W: the fragments of the lower edge
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
    *reinterpret_cast<bf16x4*>(ps0 + (n * 16 + col) * QP + rbase) = pk;
  }
  const bf16x4 zero{f2bf(0.f), f2bf(0.f), f2bf(0.f), f2bf(0.f)};
  if (f0 & 1) *reinterpret_cast<bf16x4*>(ps0 + (col - 16) * QP + rbase) = zero;           // fragment f0 - 1
  if ((f0 + NF) & 1) *reinterpret_cast<bf16x4*>(ps0 + (NF * 16 + col) * QP + rbase) = zero;  // fragment f0 + NF
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's P writes landed
  __builtin_amdgcn_wave_barrier();
  // ---- O += P V over the 32-key pairs f0 / 2 .. (f0 + NF - 1) / 2 of the block (wave-uniform bounds)
  const int trq = (lane & 15) >> 2, trp = lane & 3;
  for (int ks = f0 >> 1; ks <= (f0 + NF - 1) >> 1; ++ks) {
    const int key0 = ks * 32 + (lane >> 4) * 8;  // this lane group's 8 keys
    const bf16x8 pa = tr_read8(ps + (key0 + trq) * QP + trp * 4, QP);
#pragma unroll
    for (int n = 0; n < T::NO; ++n) {
      const bf16x8 vb = tr_read8(Vs + (key0 + trq) * T::VP + hp * DH + n * 16 + trp * 4, T::VP);
      o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vb, o[n], 0, 0, 0);
    }
  }
}

template <int DH, int KB>
__global__ __launch_bounds__(NTH) void attention_window_kernel(const bf16* __restrict__ qkv,
                                                               const int* __restrict__ ids, bf16* __restrict__ out,
                                                               int BG, int S, int H, int W, int pad_id,
                                                               float scale_log2e) {
  using T = tile<DH>;
  constexpr int HP = T::HP;
  constexpr int QB = 64 / HP;  // queries per workgroup
  constexpr int F = KB / 16;   // fragments per key block
  constexpr int PSLOT = T::pslot(KB);
  static_assert(F == 2 || F == 4, "the fragment dispatch below");
  __shared__ __attribute__((aligned(16))) bf16 Ks[2][KB * T::RW];
  __shared__ __attribute__((aligned(16))) bf16 Vs[2][KB * T::VP];
  __shared__ __attribute__((aligned(16))) bf16 Ps[4 * PSLOT];
  __shared__ float kmask[2][KB];

  const int qblocks = (S + QB - 1) / QB;
  const int HG = (H + HP - 1) / HP;
  const int qb = qblocks - 1 - (int)(blockIdx.x / BG);  // last query block first: the clamped walks end the launch
  const int bg = blockIdx.x % BG;
  const int b = bg / HG, h0 = (bg % HG) * HP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hp = wave % HP, qg = wave / HP;
  const int HD = H * DH, ld = 3 * HD;
  const int vch = min(HP, H - h0) * (DH / 8);
  const size_t tok0 = (size_t)b * S;
  const bf16* kbase = qkv + tok0 * ld + HD + h0 * DH;  // K of key 0, group row; V lies HD further
  const int* idb = ids + tok0;

  // key blocks: from the one holding the first key of the first row's window to the last row's own
  const int q0 = qb * QB;
  const int j0 = max(q0 - (W - 1), 0) / KB;
  const int j1 = min(q0 + QB - 1, S - 1) / KB;
  Staged st;
  load_block<DH, KB>(st, kbase, idb, j0, S, ld, HD, vch, pad_id, tid);

  const int r0 = q0 + qg * 16;  // the wave's first row
  const bool active = r0 < S && h0 + hp < H;  // wave-uniform: rows that are stored, a head that exists
  const int qrow = r0 + (lane & 15);
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
  store_block<DH, KB>(st, Ks[0], Vs[0], kmask[0], tid);

  bf16* ps = Ps + wave * PSLOT;
  const int fd = r0 / 16;                     // the wave's diagonal fragment
  const int fa = max(r0 - (W - 1), 0) / 16;  // the fragment its first window begins in
  const int dlane = (lane & 15) - (lane >> 4) * 4 - r0;  // key column - accumulator row base - r0
  for (int j = j0; j <= j1; ++j) {
    const int cur = (j - j0) & 1;
    const bool more = j < j1;  // block-uniform
    if (more) load_block<DH, KB>(st, kbase, idb, j + 1, S, ld, HD, vch, pad_id, tid);
    __syncthreads();
    const int lo = max(fa, j * F), hi = min(fd, j * F + F - 1);  // wave-uniform
    const int nf = hi - lo + 1;
    const bf16 *ks = Ks[cur], *vs = Vs[cur];
    const float* km = kmask[cur];
    if (active && nf >= 1) {  // else: outside the wave's windows
      const int f0 = lo - j * F, d0 = lo * 16 + dlane;
      if (lo > fa + 1 && hi < fd) {  // a whole block inside every window: nf == F, f0 == 0
        key_step<DH, F, false>(ks, vs, km, ps, qa, o, mrow, lrow, lane, hp, scale_log2e);
      } else if (nf == 1) {
        edge_step<DH, 1>(ks, vs, km, ps, qa, o, mrow, lrow, lane, hp, scale_log2e, f0, d0, W);
      } else if (nf == 2) {
        edge_step<DH, 2>(ks, vs, km, ps, qa, o, mrow, lrow, lane, hp, scale_log2e, f0, d0, W);
      } else if constexpr (F == 4) {
        if (nf == 3) edge_step<DH, 3>(ks, vs, km, ps, qa, o, mrow, lrow, lane, hp, scale_log2e, f0, d0, W);
        else edge_step<DH, 4>(ks, vs, km, ps, qa, o, mrow, lrow, lane, hp, scale_log2e, f0, d0, W);
      }
    }
    if (more) store_block<DH, KB>(st, Ks[cur ^ 1], Vs[cur ^ 1], kmask[cur ^ 1], tid);
  }
  store_ctx<DH>(Ps + (wave - hp) * PSLOT, o, lrow, out + tok0 * HD + h0 * DH, HD, r0, S, vch, lane, hp);
}

}  // namespace

void attention_window_fwd_bf16(uintptr_t qkv, uintptr_t ids, uintptr_t out, int B, int S, int H, int Dh, int window,
                               int pad_id, float scale, uintptr_t stream) {
  if (Dh != 32 && Dh != 64 && Dh != 128)
    throw std::invalid_argument("attention_window_fwd: head dim must be 32, 64 or 128");
  if (B <= 0 || H <= 0) throw std::invalid_argument("attention_window_fwd: empty problem");
  if (S < 1 || S > MAX_S) throw std::invalid_argument("attention_window_fwd: need 1 <= S <= 8192");
  if (window < 1) throw std::invalid_argument("attention_window_fwd: need window >= 1");
  if (!qkv || !ids || !out) throw std::invalid_argument("attention_window_fwd: null pointer");
  // rows are H * Dh * 2 bytes, a multiple of 16 for every width: aligned bases suffice
  if (qkv % 16 || out % 16 || ids % 4) throw std::invalid_argument("attention_window_fwd: misaligned pointers");
  const int qbh = Dh == 32 ? 32 : 64;                                // queries per workgroup
  const long long BG = (long long)B * (Dh == 32 ? (H + 1) / 2 : H);  // (batch, head group): pairs at 32
  const long long grid = BG * ((S + qbh - 1) / qbh);
  if (BG > INT_MAX || grid > INT_MAX) throw std::invalid_argument("attention_window_fwd: grid too large");
  const int W = window < S ? window : S;  // no query has more than S keys: the kernel's arithmetic stays below 2 S
  const auto kern = Dh == 32    ? attention_window_kernel<32, 64>
                    : Dh == 128 ? attention_window_kernel<128, 32>
                                : attention_window_kernel<64, 64>;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NTH), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const bf16*>(qkv), reinterpret_cast<const int*>(ids),
                     reinterpret_cast<bf16*>(out), (int)BG, S, H, W, pad_id, scale * 1.4426950408889634f);
  FTM_CHECK_LAUNCH();
}

void register_attention_window(pybind11::module_& m) { m.def("attention_window_fwd_bf16", &attention_window_fwd_bf16); }
