// Retrieval: the k best of N items per query, scores = q . items^T (+ bias), without a score
// matrix (a two-tower model's MatMul -> [BiasAdd] -> TopKV2; ops/kernels.py:retrieve_topk holds
// the host definition).  Two launches, deterministic: no atomics, nothing depends on how
// workgroups are scheduled.
//
//   q      [B, D] bf16          items [N, D] bf16, dense rows, K-contiguous as they lie in memory
//   bias   [N] fp32 or null     scratch [B, chunks, kpad] 8-byte keys, kpad = k rounded up to 2^n
//   values [B, k] fp32          indices [B, k] int32
//
// Keys (the construction of detection.hip): (order-preserving uint32 image of the fp32 score)
// << 32 | ~item.  Keys are unique, a larger key is a better item and equal scores order lower
// index first; key 0 is an empty slot (a real item's low word is >= 2^31).  The score inside a
// key is the fp32 accumulator (+ bias) bit for bit: it is never rounded to bf16 and never stored.
// The accumulator starts at +0, so a score is never -0.  A NaN score has no defined rank.
//
// retrieve_partial<NKF, CAP>   NKF = D / 32; one workgroup per (query tile, item chunk), the
//   query tile fastest and the pair remapped so that the tiles of a chunk share an XCD's L2.
//   QT = 64 queries and 4 waves (CAP 64 or 128), or 32 queries and 2 waves (CAP 256).
//   * scores   v_mfma_f32_16x16x32_bf16, items on M, queries on N.  A wave owns 16 queries for
//              the whole chunk: its NKF B-fragments (NKF x 4 VGPRs, 32 at D = 256) are loaded
//              once.  Item tiles of RETRIEVE_ITEM_TILE = 64 rows go through registers into a
//              double-buffered LDS stage, 16-byte chunks XOR-swizzled by the row (by row & 7
//              when a row has a multiple of 8 chunks, else by row & 3), one barrier per tile;
//              every wave reads the same tile, so a query tile reads each item row once.  The
//              tile's 64 biases ride in the same stage.  Rows past N and queries past B are
//              predicated zero loads, and their keys are forced to 0.
//   * select   in the 16x16 accumulator a lane holds 4 item scores of one query (4 lanes per
//              query).  Each query carries its threshold, the key of its k-th best so far, in
//              registers, with the threshold's score as a float: a fragment whose 16 x 16 scores
//              are all below it costs 4 adds, a max and a ballot.  Otherwise the lanes build
//              the keys, the 4 lanes of a query agree on positions by shuffles and append the
//              keys above the threshold to that query's LDS buffer of CAP keys.  When a buffer
//              could overflow on the next fragment (count + 16 > CAP) the wave prunes its 16
//              buffers: zero the tail, bitonic sort of CAP keys per query (4 lanes per query,
//              wave-synchronous), keep the best k, threshold = key k - 1: CAP - 16 - k appends
//              fit before the next prune.  After warm-up a query appends about k ln(chunk / k)
//              keys per chunk.  (Keeping kpad keys in a buffer of 2 kpad left a k = 10 buffer
//              full after every prune, one prune per append: 6816 us against 1092 us for N = 4M,
//              D = 64, B = 256; profiles/r18_retrieval.)
//   * out      one last prune, then the sorted kpad keys of every query < B go to scratch.
//
//   Static LDS = 2 * 64 * D * 2 (stages) + 512 (biases) + QT * (CAP + 2) * 8 (candidates; the
//   pitch of CAP + 2 keys spreads the 16 buffers of a wave over the banks):
//       k <= 16   CAP  64, QT 64:   33,792 B + 256 D  ->  41.0 KiB at D = 32,  97.0 KiB at D = 256
//       k <= 64   CAP 128, QT 64:   66,560 B + 256 D  ->  73.5 KiB at D = 32, 129.5 KiB at D = 256
//       k <= 128  CAP 256, QT 32:   66,048 B + 256 D  ->  73.0 KiB at D = 32, 129.0 KiB at D = 256
//   (+ 512 B each), all within gfx950's 160 KiB; CAP >= kpad + 16 in every class.
//
// retrieve_merge   one workgroup of 256 threads per query: the k best of the chunks * kpad keys.
//   The chunk lists arrive sorted, so this is a k-round tournament over list heads (the
//   nms_merge design): thread t holds the heads of lists t, t + 256, ... (at most 8: chunks <=
//   2048) in registers, a round takes the workgroup's largest head (wave shuffles, one barrier)
//   and the one list that owns it moves on, reading its next key from scratch.  Cost grows with
//   k, not with chunks * kpad (which can exceed LDS).  Thread t < k then decodes key t.
//
// Every offset into items and scratch is 64-bit.
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace {

constexpr int IT = 64;              // RETRIEVE_ITEM_TILE: item rows per LDS stage
constexpr int MERGE_THREADS = 256;
constexpr int MERGE_LISTS = 8;      // chunk lists per merge thread
constexpr int MAX_CHUNKS = MERGE_THREADS * MERGE_LISTS;

struct RetrieveParams {
  const bf16* q;
  const bf16* items;
  const float* bias;  // null: none
  unsigned long long* scratch;
  int B, N, k, kpad, chunk, chunks, qtiles;
};

FTM_DEVICE uint32_t score_image(float s) {
  const uint32_t u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
FTM_DEVICE float image_score(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// LDS traffic inside one wave: DS operations of a wave complete in order, so this only has to
// keep the compiler from moving accesses across it (lgkmcnt(0), no wait on global loads)
FTM_DEVICE void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

template <int NKF, int CAP>
__global__ __launch_bounds__(CAP == 256 ? 128 : 256) void retrieve_partial_kernel(const RetrieveParams p) {
  constexpr int QT = CAP == 256 ? 32 : 64;  // queries per workgroup
  constexpr int NT = QT * 4;                // threads: a wave per 16 queries
  constexpr int D = NKF * 32;
  constexpr int RC = NKF * 4;               // 16-byte chunks per item row
  constexpr int SW = NKF % 2 == 0 ? 7 : 3;  // swizzle mask: stays inside a row's RC chunks
  constexpr int CPT = IT * RC / NT;         // chunks staged per thread and tile
  constexpr int CST = CAP + 2;              // candidate buffer pitch (keys)
  static_assert(IT * RC % NT == 0 && IT <= NT, "staging assignment");
  __shared__ __attribute__((aligned(16))) bf16 stage[2][IT * D];
  __shared__ __attribute__((aligned(16))) float sbias[2][IT];
  __shared__ unsigned long long cand[QT * CST];

  const int tile = xcd_remap(blockIdx.x, p.qtiles * p.chunks);
  const int qt = tile % p.qtiles;
  const int ch = tile / p.qtiles;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int ql = lane & 15;  // accumulator column: the query of the wave's 16
  const int g = lane >> 4;   // accumulator rows 4 g .. 4 g + 3: the items of a fragment
  const unsigned N = (unsigned)p.N;
  const unsigned n_begin = (unsigned)ch * (unsigned)p.chunk;  // < N < 2^31
  const unsigned n_end = N - n_begin < (unsigned)p.chunk ? N : n_begin + (unsigned)p.chunk;
  const int ntiles = (int)((n_end - n_begin + IT - 1) / IT);  // >= 1

  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const int qrow = qt * QT + wave * 16 + ql;
  const bool qv = qrow < p.B;
  bf16x8 bq[NKF];  // the query's K-fragments, resident for the whole chunk
#pragma unroll
  for (int kf = 0; kf < NKF; ++kf) {
    const u32x4 v = qv ? *reinterpret_cast<const u32x4*>(p.q + ((long)qrow * D + kf * 32 + g * 8)) : zero4;
    bq[kf] = __builtin_bit_cast(bf16x8, v);
  }

  u32x4 xr[CPT];
  float br = 0.f;
  auto load_tile = [&](int t) {
    const unsigned n0 = n_begin + (unsigned)t * IT;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int c = tid + i * NT;
      const unsigned n = n0 + (unsigned)(c / RC);
      xr[i] = n < N ? *reinterpret_cast<const u32x4*>(p.items + ((long)n * D + (c % RC) * 8)) : zero4;
    }
    if (tid < IT) {
      const unsigned n = n0 + (unsigned)tid;
      br = (p.bias != nullptr && n < N) ? p.bias[n] : 0.f;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int c = tid + i * NT;
      const int row = c / RC, cc = c % RC;
      *reinterpret_cast<u32x4*>(&stage[buf][row * D + ((cc ^ (row & SW)) << 3)]) = xr[i];
    }
    if (tid < IT) sbias[buf][tid] = br;
  };

  // selection state of query ql, replicated in its 4 lanes
  unsigned long long* const wcand = cand + wave * 16 * CST;  // the wave's 16 buffers
  unsigned long long* const myc = wcand + ql * CST;
  unsigned long long thr = 0;  // key of the k-th best so far; 0: fewer than k yet
  float thr_f = qv ? -__builtin_inff() : __builtin_inff();  // its score; +inf switches a padding query off
  int count = 0;

  auto prune = [&]() {
    for (int j = count + g; j < CAP; j += 4) myc[j] = 0;
    wave_lds_fence();
    unsigned long long* const sc = wcand + (lane >> 2) * CST;  // sort: 4 lanes per query
    const int sub = lane & 3;
    for (int kk = 2; kk <= CAP; kk <<= 1) {
      for (int j = kk >> 1; j > 0; j >>= 1) {
        for (int t = sub; t < CAP / 2; t += 4) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // pair t: bit j clear, partner i | j
          const int l = i | j;
          const unsigned long long a = sc[i], b = sc[l];
          const bool desc = (i & kk) == 0;
          if (desc ? a < b : a > b) {
            sc[i] = b;
            sc[l] = a;
          }
        }
        wave_lds_fence();
      }
    }
    count = count < p.k ? count : p.k;  // keys k .. CAP - 1 are dropped: later appends overwrite them
    thr = myc[p.k - 1];
    if (qv) thr_f = thr != 0 ? image_score((uint32_t)(thr >> 32)) : -__builtin_inff();
  };

  load_tile(0);
  store_tile(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) load_tile(t + 1);
    const bf16* st = stage[t & 1];
    f32x4 acc[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) {
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int row = f * 16 + ql;
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(st + row * D + (((kf * 4 + g) ^ (row & SW)) << 3));
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bq[kf], acc[f], 0, 0, 0);
      }
    }
    const unsigned n0 = n_begin + (unsigned)t * IT;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const f32x4 s = acc[f] + *reinterpret_cast<const f32x4*>(&sbias[t & 1][f * 16 + g * 4]);
      const float m = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
      if (__ballot(!(m < thr_f)) == 0) continue;  // wave-uniform: nothing here reaches a threshold
      const unsigned nb = n0 + (unsigned)(f * 16 + g * 4);
      unsigned long long key[4];
      int c = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned n = nb + r;
        const unsigned long long kr = ((unsigned long long)score_image(s[r]) << 32) | (uint32_t)~n;
        const bool pass = qv && n < N && kr > thr;
        key[r] = pass ? kr : 0;
        c += pass ? 1 : 0;
      }
      const int c0 = __shfl(c, ql, 64), c1 = __shfl(c, ql + 16, 64), c2 = __shfl(c, ql + 32, 64),
                c3 = __shfl(c, ql + 48, 64);
      int pos = count + (g > 0 ? c0 : 0) + (g > 1 ? c1 : 0) + (g > 2 ? c2 : 0);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (key[r] != 0) myc[pos++] = key[r];  // count <= CAP - 16 before the fragment: in bounds
      count += c0 + c1 + c2 + c3;
      if (__ballot(count + 16 > CAP) != 0) prune();
    }
    if (t + 1 < ntiles) store_tile((t + 1) & 1);
    __syncthreads();
  }

  prune();
  const int oq = qt * QT + wave * 16 + (lane >> 2);
  if (oq < p.B) {
    unsigned long long* dst = p.scratch + ((long)oq * p.chunks + ch) * p.kpad;
    const unsigned long long* src = wcand + (lane >> 2) * CST;
    for (int j = lane & 3; j < p.kpad; j += 4) dst[j] = src[j];
  }
}

FTM_DEVICE unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w > v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(MERGE_THREADS) void retrieve_merge_kernel(const unsigned long long* scratch, float* values,
                                                                      int* indices, int chunks, int kpad, int k) {
  __shared__ unsigned long long best[128];  // the merged keys, best first (k <= 128)
  __shared__ unsigned long long wmax[2][MERGE_THREADS / 64];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const unsigned long long* base = scratch + (long)b * chunks * kpad;
  unsigned long long head[MERGE_LISTS];
  int pos[MERGE_LISTS];
#pragma unroll
  for (int j = 0; j < MERGE_LISTS; ++j) {
    const int list = tid + j * MERGE_THREADS;
    head[j] = list < chunks ? base[(long)list * kpad] : 0;
    pos[j] = 0;
  }
  int t = 0;
  for (; t < k; ++t) {
    unsigned long long m = head[0];
#pragma unroll
    for (int j = 1; j < MERGE_LISTS; ++j) m = head[j] > m ? head[j] : m;
    m = wave_max_u64(m);
    if ((tid & 63) == 0) wmax[t & 1][tid >> 6] = m;
    __syncthreads();  // one barrier a round: round t + 2 rewrites this half only after the barrier of t + 1
    unsigned long long w = wmax[t & 1][0];
#pragma unroll
    for (int i = 1; i < MERGE_THREADS / 64; ++i) w = wmax[t & 1][i] > w ? wmax[t & 1][i] : w;
    if (w == 0) break;  // every list is used up (the same w in every thread)
#pragma unroll
    for (int j = 0; j < MERGE_LISTS; ++j) {
      if (head[j] == w) {  // keys are unique: exactly one list of one thread wins
        best[t] = w;
        ++pos[j];
        head[j] = pos[j] < kpad ? base[(long)(tid + j * MERGE_THREADS) * kpad + pos[j]] : 0;
      }
    }
  }
  const int total = t;  // k whenever N >= k
  __syncthreads();
  if (tid < k) {
    const unsigned long long key = tid < total ? best[tid] : 0;
    values[(long)b * k + tid] = key != 0 ? image_score((uint32_t)(key >> 32)) : -__builtin_inff();
    indices[(long)b * k + tid] = key != 0 ? (int)~(uint32_t)key : -1;
  }
}

template <int CAP>
void launch_partial(const RetrieveParams& p, int nkf, hipStream_t s) {
  constexpr int NT = CAP == 256 ? 128 : 256;
  const dim3 grid((unsigned)(p.qtiles * p.chunks)), block(NT);
  switch (nkf) {
    case 1: hipLaunchKernelGGL((retrieve_partial_kernel<1, CAP>), grid, block, 0, s, p); break;
    case 2: hipLaunchKernelGGL((retrieve_partial_kernel<2, CAP>), grid, block, 0, s, p); break;
    case 3: hipLaunchKernelGGL((retrieve_partial_kernel<3, CAP>), grid, block, 0, s, p); break;
    case 4: hipLaunchKernelGGL((retrieve_partial_kernel<4, CAP>), grid, block, 0, s, p); break;
    case 5: hipLaunchKernelGGL((retrieve_partial_kernel<5, CAP>), grid, block, 0, s, p); break;
    case 6: hipLaunchKernelGGL((retrieve_partial_kernel<6, CAP>), grid, block, 0, s, p); break;
    case 7: hipLaunchKernelGGL((retrieve_partial_kernel<7, CAP>), grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL((retrieve_partial_kernel<8, CAP>), grid, block, 0, s, p); break;
  }
}

}  // namespace

// part: 0 = both launches, 1 = retrieve_partial only, 2 = retrieve_merge only (measurement: the
// merge then reads what an earlier partial launch left in scratch).  scratch_elems is the size of
// the scratch in 8-byte keys, checked against B * chunks * kpad.
void retrieve_topk(uintptr_t q, uintptr_t items, uintptr_t bias, int B, long N, int D, int k, long chunk,
                   uintptr_t scratch, long scratch_elems, uintptr_t values, uintptr_t indices, int part,
                   uintptr_t stream) {
  if (B < 1) throw std::invalid_argument("retrieve_topk: empty batch");
  if (D % 32 || D < 32 || D > 256) throw std::invalid_argument("retrieve_topk: D must be a multiple of 32 in 32..256");
  if (k < 1 || k > 128) throw std::invalid_argument("retrieve_topk: k must be 1..128");
  if (N < k || N >= (1L << 31)) throw std::invalid_argument("retrieve_topk: N must be k..2^31 - 1");
  if (chunk < IT || chunk % IT || chunk >= (1L << 31))
    throw std::invalid_argument("retrieve_topk: chunk must be a positive multiple of " + std::to_string(IT));
  const long chunks = (N + chunk - 1) / chunk;
  if (chunks > MAX_CHUNKS) throw std::invalid_argument("retrieve_topk: more than " + std::to_string(MAX_CHUNKS) + " chunks");
  if (part < 0 || part > 2) throw std::invalid_argument("retrieve_topk: part must be 0, 1 or 2");
  if (!q || !items || !scratch || !values || !indices) throw std::invalid_argument("retrieve_topk: null pointer");
  if (q % 16 || items % 16 || bias % 4 || scratch % 8 || values % 4 || indices % 4)
    throw std::invalid_argument("retrieve_topk: misaligned pointer");
  int kpad = 1;
  while (kpad < k) kpad <<= 1;
  if (scratch_elems < (long)B * chunks * kpad) throw std::invalid_argument("retrieve_topk: scratch too small");
  const int qt = k > 64 ? 32 : 64;
  const long qtiles = ((long)B + qt - 1) / qt;
  if (qtiles * chunks >= (1L << 31)) throw std::invalid_argument("retrieve_topk: more than 2^31 workgroups");
  RetrieveParams p;
  p.q = reinterpret_cast<const bf16*>(q);
  p.items = reinterpret_cast<const bf16*>(items);
  p.bias = reinterpret_cast<const float*>(bias);
  p.scratch = reinterpret_cast<unsigned long long*>(scratch);
  p.B = B, p.N = (int)N, p.k = k, p.kpad = kpad;
  p.chunk = (int)chunk, p.chunks = (int)chunks, p.qtiles = (int)qtiles;
  auto s = reinterpret_cast<hipStream_t>(stream);
  if (part != 2) {
    if (k <= 16) launch_partial<64>(p, D / 32, s);
    else if (k <= 64) launch_partial<128>(p, D / 32, s);
    else launch_partial<256>(p, D / 32, s);
    FTM_CHECK_LAUNCH();
  }
  if (part != 1) {
    hipLaunchKernelGGL(retrieve_merge_kernel, dim3((unsigned)B), dim3(MERGE_THREADS), 0, s, p.scratch,
                       reinterpret_cast<float*>(values), reinterpret_cast<int*>(indices), p.chunks, kpad, k);
    FTM_CHECK_LAUNCH();
  }
}

void register_retrieve(pybind11::module_& m) {
  m.def("retrieve_topk", &retrieve_topk);
  m.attr("retrieve_item_tile") = IT;
  m.attr("retrieve_max_chunks") = MAX_CHUNKS;
}
