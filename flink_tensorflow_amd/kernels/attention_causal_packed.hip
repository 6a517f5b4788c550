// Causal multi-head self-attention of a TOKEN-PACKED batch (padding-free next-item / next-event
// transformers), and the row bookkeeping it needs.
//
// Buffers: qkv [T_cap, 3*H*DH] bf16 from the fused QKV projection on packed rows (Q | K | V column
// blocks, head h at columns h*DH), cu [B + 1] int32 row offsets (sequence b is rows cu[b] ..
// cu[b+1] - 1 of the token stream), seq_start [T_cap] int32 (the first row of the sequence that
// row t belongs to; packed_rows_kernel below writes it from cu), ctx [T_cap, H*DH] bf16.  Query
// row t < cu[B] attends key row j iff seq_start[t] <= j <= t.  There is no pad mask: pack_tokens
// has dropped every pad id.  Rows >= cu[B] are neither read as queries or keys nor written.
//
// Work split: the TOKEN STREAM is tiled, not the sequences.  Workgroup (qb, head group) owns the
// packed rows [qb QB, qb QB + QB) whichever sequences they belong to, so a tile of 64 rows holds
// 64 real queries even when histories are 7 events long, and the grid, ceil(T_cap / QB) x head
// groups, depends on the token capacity alone (a captured graph replays it for every batch).  A
// workgroup whose first row is >= cu[B] returns before any barrier.  Four waves x 16 query rows,
// Q fragments resident in registers.  QB = 64 rows of one head (DH = 64, 128) or 32 rows of the
// head pair (2p, 2p + 1) at DH = 32 (wave w: head w & 1, query group w >> 1), KB = 64 keys per
// step, 32 at DH = 128: the per-width choices, LDS rows and swizzles of attention_causal.hip.
//
// Key walk: key blocks lie on the same stream grid, KB rows each.  The workgroup walks from the
// block that holds seq_start[its first row] (starts are non-decreasing along the stream, so no
// row of the tile sees an earlier key) up to the block of its last row that exists.  The diagonal
// is walked per 16-key fragment as in attention_causal.hip: the wave's rows are fragment fd of the
// stream, in key block j it multiplies nf = fd + 1 - j F fragments, nf > F is a block wholly
// below its diagonal, 1 <= nf <= F holds its diagonal tile as the last fragment, nf <= 0 lies
// above it and is skipped.
//
// Pipeline (attention_causal.hip): K/V double-buffered in LDS; at step j the global loads of
// block j + 1 are issued into registers, ONE barrier publishes buffer j & 1 and retires every read
// of the other, the MFMAs (v_mfma_f32_16x16x32_bf16, P through the per-wave P^T tile, exp2-domain
// online softmax with fp32 statistics) run while the loads fly, and the registers are written to
// the other buffer after them.
//
// Mask: a lane keeps the sequence starts of its four accumulator rows in registers, loaded once.
// An element is masked when key < start[row], and in the diagonal fragment when key > row.  Two
// wave-uniform shortcuts follow from the monotone starts: a block below the diagonal whose first
// key is >= the start of the wave's LAST row needs no lower-bound compare (the inside of a long
// sequence runs the unmasked step), and a block wholly before the start of the wave's FIRST row is
// skipped by that wave (it still stages and meets the barrier).  The diagonal block always takes
// the compare: it is one step per tile.  A wave whose rows all lie past cu[B], or whose head does
// not exist (odd H at DH = 32), multiplies nothing.
#include <pybind11/pybind11.h>

#include <climits>
#include <stdexcept>

#include "attention_tiles.h"
#include "common.h"

namespace {

using namespace attn;

constexpr int NTH = 256;  // 4 waves

// One thread's share of a key block in flight: two K and two V 16-B chunks.
struct Staged {
  u32x4 k[2], v[2];
};

template <int DH, int KB>
FTM_DEVICE void load_block(Staged& st, const bf16* __restrict__ kbase, int kb, int ntok, int ld, int HD, int vch,
                           int tid) {
  constexpr int NCH = tile<DH>::NCH;
  static_assert(KB * NCH == 2 * NTH, "two K and two V chunks per thread and stage");
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int q = tid + it * NTH;
    const int kg = kb * KB + q / NCH, ch = q % NCH;
    st.k[it] = u32x4{0u, 0u, 0u, 0u};
    st.v[it] = u32x4{0u, 0u, 0u, 0u};
    if (kg < ntok && ch < vch) {  // rows past the batch and absent heads are staged as zeros
      const bf16* row = kbase + (size_t)kg * ld + ch * 8;
      st.k[it] = *reinterpret_cast<const u32x4*>(row);
      st.v[it] = *reinterpret_cast<const u32x4*>(row + HD);
    }
  }
}

template <int DH>
FTM_DEVICE void store_block(const Staged& st, bf16* Ks, bf16* Vs, int tid) {
  using T = tile<DH>;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int q = tid + it * NTH;
    const int key = q / T::NCH, ch = q % T::NCH;
    *reinterpret_cast<u32x4*>(Ks + T::kswz(key, ch)) = st.k[it];
    *reinterpret_cast<u32x4*>(Vs + key * T::VP + ch * 8) = st.v[it];
  }
}

template <int DH, int KB>
__global__ __launch_bounds__(NTH) void attention_causal_packed_kernel(const bf16* __restrict__ qkv,
                                                                      const int* __restrict__ cu,
                                                                      const int* __restrict__ seq_start,
                                                                      bf16* __restrict__ out, int B, int T_cap, int H,
                                                                      float scale_log2e) {
  using T = tile<DH>;
  constexpr int HP = T::HP;
  constexpr int QB = 64 / HP;  // stream rows per workgroup
  constexpr int F = KB / 16;   // fragments per key block
  constexpr int PSLOT = T::pslot(KB);
  static_assert(F == 2 || F == 4, "the fragment dispatch below");
  __shared__ __attribute__((aligned(16))) bf16 Ks[2][KB * T::RW];
  __shared__ __attribute__((aligned(16))) bf16 Vs[2][KB * T::VP];
  __shared__ __attribute__((aligned(16))) bf16 Ps[4 * PSLOT];

  const int ntok = min(cu[B], T_cap);  // rows of the stream that exist
  const int qb = blockIdx.x, row0 = qb * QB;
  if (row0 >= ntok) return;  // block-uniform, before any barrier: an idle tile of the capacity
  const int h0 = blockIdx.y * HP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hp = wave % HP, qg = wave / HP;
  const int HD = H * DH, ld = 3 * HD;
  const int vch = min(HP, H - h0) * (DH / 8);
  const bf16* kbase = qkv + HD + h0 * DH;  // K of stream row 0, group row; V lies HD further

  // key blocks: from the one holding the start of the tile's first row to the last row's own
  const int j0 = min(max(seq_start[row0], 0), row0) / KB;
  const int j1 = min(row0 + QB - 1, ntok - 1) / KB;
  Staged st;
  load_block<DH, KB>(st, kbase, j0, ntok, ld, HD, vch, tid);

  const int wrow0 = row0 + qg * 16;  // the wave's first row
  const bool active = wrow0 < ntok && h0 + hp < H;  // wave-uniform
  const int qrow = wrow0 + (lane & 15);
  bf16x8 qa[T::NKS];
#pragma unroll
  for (int ks = 0; ks < T::NKS; ++ks) {
    if (qrow < ntok && h0 + hp < H)
      qa[ks] = *reinterpret_cast<const bf16x8*>(qkv + (size_t)qrow * ld + (h0 + hp) * DH + ks * 32 + (lane >> 4) * 8);
    else
      qa[ks] = bf16x8{};
  }
  // sequence starts of the lane's accumulator rows; a row past the batch starts at itself
  int start[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = wrow0 + (lane >> 4) * 4 + r;
    start[r] = row < ntok ? seq_start[row] : row;
  }
  const int sfirst = active ? seq_start[wrow0] : 0;                              // wave-uniform
  const int slast = wrow0 + 15 < ntok ? seq_start[wrow0 + 15] : wrow0 + 15;  // wave-uniform
  f32x4 o[T::NO];
#pragma unroll
  for (int n = 0; n < T::NO; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrow[4], lrow[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mrow[r] = -INFINITY;
    lrow[r] = 0.f;
  }
  store_block<DH>(st, Ks[0], Vs[0], tid);

  bf16* ps = Ps + wave * PSLOT;
  const int fd = wrow0 / 16;  // the wave's diagonal fragment of the stream
  for (int j = j0; j <= j1; ++j) {
    const int cur = (j - j0) & 1;
    const bool more = j < j1;  // block-uniform
    if (more) load_block<DH, KB>(st, kbase, j + 1, ntok, ld, HD, vch, tid);
    __syncthreads();
    const int nf = fd + 1 - j * F;  // wave-uniform
    const int key0 = j * KB;
    const bf16 *ks = Ks[cur], *vs = Vs[cur];
    if (active && nf >= 1 && key0 + KB > sfirst) {  // else: above the diagonal, or all keys of earlier sequences
      if (nf > F) {
        if (key0 >= slast)
          key_step<DH, F, false, true, false>(ks, vs, nullptr, ps, qa, o, mrow, lrow, lane, hp, scale_log2e);
        else
          key_step<DH, F, false, true, true>(ks, vs, nullptr, ps, qa, o, mrow, lrow, lane, hp, scale_log2e, key0, start);
      } else if (nf == F) {
        key_step<DH, F, true, true, true>(ks, vs, nullptr, ps, qa, o, mrow, lrow, lane, hp, scale_log2e, key0, start);
      } else if (nf == 1) {
        key_step<DH, 1, true, true, true>(ks, vs, nullptr, ps, qa, o, mrow, lrow, lane, hp, scale_log2e, key0, start);
      } else if constexpr (F == 4) {
        if (nf == 2)
          key_step<DH, 2, true, true, true>(ks, vs, nullptr, ps, qa, o, mrow, lrow, lane, hp, scale_log2e, key0, start);
        else
          key_step<DH, 3, true, true, true>(ks, vs, nullptr, ps, qa, o, mrow, lrow, lane, hp, scale_log2e, key0, start);
      }
    }
    if (more) store_block<DH>(st, Ks[cur ^ 1], Vs[cur ^ 1], tid);
  }
  // a query always sees itself, so l > 0 for every stored row; store_ctx keeps the l > 0 guard
  store_ctx<DH>(Ps + (wave - hp) * PSLOT, o, lrow, out + h0 * DH, HD, wrow0, ntok, vch, lane, hp);
}

// Row bookkeeping of a packed batch, once per replay behind pack_tokens: seq_start[t] = cu[b] of
// the sequence b that holds row t (a row past cu[B]: t itself), last[b] = the row of sequence b's
// last token, clamped into [0, T_cap - 1] (an empty sequence has none; its value is not used as a
// query by last_attention, only as a gather index that must stay inside the buffer).  Thread t
// finds the first b with cu[b + 1] > t by bisection (cu is non-decreasing; empty sequences share a
// start and are passed over).  window > 0 (sliding-window causal attention): row t sees its last
// ``window`` rows only, seq_start[t] = max(cu[b], t - window + 1), which is still non-decreasing
// along the stream, so the attention kernel above serves it unchanged.
__global__ __launch_bounds__(256) void packed_rows_kernel(const int* __restrict__ cu, int B, int T_cap,
                                                          int* __restrict__ seq_start, int* __restrict__ last,
                                                          int window) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < B) last[t] = min(max(cu[t + 1] - 1, 0), T_cap - 1);
  if (t >= T_cap) return;
  int v = t;
  if (t < cu[B]) {
    int lo = 0, hi = B - 1;  // cu[hi + 1] > t holds
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cu[mid + 1] > t) hi = mid;
      else lo = mid + 1;
    }
    v = cu[lo];
    if (window > 0) v = max(v, t - window + 1);
  }
  seq_start[t] = v;
}

}  // namespace

void attention_causal_packed_fwd_bf16(uintptr_t qkv, uintptr_t cu, uintptr_t seq_start, uintptr_t out, int B, int T_cap,
                                      int H, int Dh, float scale, uintptr_t stream) {
  if (Dh != 32 && Dh != 64 && Dh != 128)
    throw std::invalid_argument("attention_causal_packed_fwd: head dim must be 32, 64 or 128");
  if (B <= 0 || H <= 0 || T_cap <= 0) throw std::invalid_argument("attention_causal_packed_fwd: empty problem");
  if (!qkv || !cu || !seq_start || !out) throw std::invalid_argument("attention_causal_packed_fwd: null pointer");
  // rows are H * Dh * 2 bytes, a multiple of 16 for every width: aligned bases suffice
  if (qkv % 16 || out % 16 || cu % 4 || seq_start % 4)
    throw std::invalid_argument("attention_causal_packed_fwd: misaligned pointers");
  const int qb = Dh == 32 ? 32 : 64;              // stream rows per workgroup
  const int hg = Dh == 32 ? (H + 1) / 2 : H;      // head groups: pairs at 32
  if (hg > 65535) throw std::invalid_argument("attention_causal_packed_fwd: too many heads");
  const auto kern = Dh == 32    ? attention_causal_packed_kernel<32, 64>
                    : Dh == 128 ? attention_causal_packed_kernel<128, 32>
                                : attention_causal_packed_kernel<64, 64>;
  hipLaunchKernelGGL(kern, dim3((unsigned)((T_cap + qb - 1) / qb), (unsigned)hg), dim3(NTH), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const bf16*>(qkv),
                     reinterpret_cast<const int*>(cu), reinterpret_cast<const int*>(seq_start),
                     reinterpret_cast<bf16*>(out), B, T_cap, H, scale * 1.4426950408889634f);
  FTM_CHECK_LAUNCH();
}

void packed_rows(uintptr_t cu, int B, int T_cap, uintptr_t seq_start, uintptr_t last, uintptr_t stream, int window) {
  if (B <= 0 || T_cap <= 0 || !cu || !seq_start || !last) throw std::invalid_argument("packed_rows: empty problem");
  if (window < 0) throw std::invalid_argument("packed_rows: window must be >= 1, or 0 for none");
  const int n = T_cap > B ? T_cap : B;
  hipLaunchKernelGGL(packed_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const int*>(cu), B, T_cap,
                     reinterpret_cast<int*>(seq_start), reinterpret_cast<int*>(last), window);
  FTM_CHECK_LAUNCH();
}

void register_attention_causal_packed(pybind11::module_& m) {
  m.def("attention_causal_packed_fwd_bf16", &attention_causal_packed_fwd_bf16);
  namespace py = pybind11;  // ``window`` is optional and last: the six-argument call is unchanged
  m.def("packed_rows", &packed_rows, py::arg("cu"), py::arg("B"), py::arg("T_cap"), py::arg("seq_start"),
        py::arg("last"), py::arg("stream"), py::arg("window") = 0);
}
