// Ranking: embedding gather + pairwise dot interaction (DLRM), one launch, and a plain embedding
// lookup.  ops/kernels.py:dot_interact / embed_rows hold the host definitions.
//
// dot_interact   per record b: gather M <= 64 vectors of D bf16 elements into T [M, D], form
//   Z = T T^T in fp32, and write one bf16 row of Wout = roundup(Wlog, 8) columns:
//   [a copy of the activation vector] + the entries of Z a lookup table selects, each rounded
//   once, + zeros up to Wout.  [B, M, D], [B, M, M] and the flattened gather never reach HBM.
//
//   table [rows, D] bf16     every field's table, one under the other
//   ids   [B, F] int32       read through a row pitch
//   meta  [3, M] int64       per vector m: first table row of its field, its id column (-1: the
//                            activation vector), its field's vocabulary size V
//   dense [B, D] bf16        the activation vector, read through a row pitch (at most one m)
//   lut   [Mpad * Mpad] int16, Mpad = 32 or 64: Z[i][j] -> output column or -1.  Z is symmetric:
//                            the host maps a pair above the diagonal to its mirror below it, so
//                            only blocks at or below the diagonal are computed.
//   out   [B, Wout] bf16     written at a row pitch (a concat slot)
//
//   An id outside [0, V), or a row past the table, is a predicated zero load: the vector is
//   zero, no address is formed from it.  So are vectors >= M.
//
//   interact_kernel<NSMAX, G>: a workgroup is 4 waves, one wave owns one record at a time and
//   strides over records.  G = 1 (M <= 32) or 2 row groups of 32 vectors; NSMAX is the MFMA step
//   count D / 16 rounded up to 4 (4, 8, 12, 16: D <= 64, 128, 192, 256), so only the last three
//   steps of an instantiation carry a run-time guard.
//   * operands   v_mfma_f32_32x32x16_bf16 with the rows of T on both M and N.  Lane l holds
//                vector (l & 31) and k-group (l >> 5) in the A layout and in the B layout alike,
//                so for T T^T both fragments are the same registers: a lane loads its share of
//                one vector once, from global memory straight into VGPRs, no LDS stage.  Both
//                operands share any permutation of K, so lane half h = l >> 5 takes the
//                contiguous columns [h D/2, (h+1) D/2) of its vector (at D = 128 one 128-byte
//                line per lane, as 16-byte loads) and step s consumes its elements [8s, 8s+8).
//   * blocks     G = 2 keeps three accumulators, Z00, Z10 and Z11; Z01 is never computed.
//   * prefetch   the next record's ids and then, when NSMAX * G <= 8, its rows are requested
//                before the current record's MFMAs and epilogue: the chain id -> row is two
//                dependent HBM latencies.  Above that a second register set of 32 to 128 VGPRs
//                would cost a wave per SIMD or more, so those instantiations prefetch the ids
//                only and rely on the other waves (a choice by register count, not yet timed).
//   * epilogue   the LUT sits in LDS, loaded once per workgroup.  In a 32x32 accumulator lane l
//                holds column (l & 31) and rows 8 i + 4 (l >> 5) + j as element 4 i + j.  A lane
//                looks each of its elements up and writes hits as bf16 into the wave's LDS row,
//                which starts as zeros (the tail, and any column no pair selects); the copy of
//                the activation vector comes from memory through D / 8 lanes, whatever meta
//                says; the wave stores the row as whole 16-byte chunks: any triangle, any
//                order, no scattered 2-byte global stores.
//
//   Static LDS: LUT 2 Mpad^2 + 4 rows of WMAX bf16 (WMAX = 32 * 33 / 2 + 256 = 784, or
//   64 * 65 / 2 + 256 = 2336): 8,320 B (G = 1), 26,880 B (G = 2).
//
// embed_rows   out[r, :] = table[base + ids[r]] as bf16, one thread per 8-element vector,
//   16-byte loads and stores, an id outside [0, V) gives zeros; out has a row pitch.
//
// Every offset into the table, the ids, the activation and the output is 64-bit.
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace {

constexpr int WAVES = 4;

struct InteractParams {
  const bf16* table;
  const int* ids;
  const long* meta;  // [3, M]
  const short* lut;  // [Mpad * Mpad]
  const bf16* dense;
  bf16* out;
  long rows, ids_pitch, dense_pitch, out_pitch;
  int B, F, M, D, wlog, copy_dense;
};

FTM_DEVICE void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

template <int NSMAX, int G>
__global__ __launch_bounds__(WAVES * 64) void interact_kernel(const InteractParams p) {
  constexpr int MPAD = 32 * G;
  constexpr int WMAX = MPAD * (MPAD + 1) / 2 + 256;
  constexpr bool PREFETCH_ROWS = NSMAX * G <= 8;
  static_assert(WMAX % 8 == 0 && (MPAD * MPAD) % 8 == 0, "16-byte chunks of the row and the LUT");
  __shared__ __attribute__((aligned(16))) short slut[MPAD * MPAD];
  __shared__ __attribute__((aligned(16))) bf16 srow[WAVES][WMAX];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 31;  // vector within a row group; accumulator column
  const int h = lane >> 5;  // k-group: which half of the vector this lane holds
  const int ns = p.D >> 4;  // MFMA steps
  const int half_off = h * (p.D >> 1);
  const int wout = (p.wlog + 7) & ~7;

  for (int i = tid; i < MPAD * MPAD / 8; i += WAVES * 64)
    reinterpret_cast<u32x4*>(slut)[i] = reinterpret_cast<const u32x4*>(p.lut)[i];
  __syncthreads();

  // this lane's vector per row group: 0 = none (zero), 1 = a table row by id, 2 = the activation vector
  int kind[G], col[G];
  long base[G], vocab[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int m = g * 32 + r;
    kind[g] = 0, col[g] = 0, base[g] = 0, vocab[g] = 0;
    if (m < p.M) {
      const long c = p.meta[p.M + m];
      if (c < 0) {
        kind[g] = p.dense != nullptr ? 2 : 0;
      } else if (c < p.F) {
        kind[g] = 1, col[g] = (int)c, base[g] = p.meta[m], vocab[g] = p.meta[2 * p.M + m];
      }
    }
  }

  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  auto load_ids = [&](long rec, int (&id)[G]) {
#pragma unroll
    for (int g = 0; g < G; ++g) id[g] = kind[g] == 1 ? p.ids[rec * p.ids_pitch + col[g]] : 0;
  };
  auto load_rows = [&](long rec, const int (&id)[G], bf16x8 (&x)[G][NSMAX]) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const bf16* src = nullptr;
      if (kind[g] == 2) {
        src = p.dense + rec * p.dense_pitch + half_off;
      } else if (kind[g] == 1) {
        const long row = base[g] + id[g];
        if (id[g] >= 0 && id[g] < vocab[g] && row >= 0 && row < p.rows) src = p.table + row * p.D + half_off;
      }
#pragma unroll
      for (int s = 0; s < NSMAX; ++s) x[g][s] = __builtin_bit_cast(bf16x8, zero4);
      if (src != nullptr) {  // one lane predicate for the whole vector; the step bound is wave-uniform
#pragma unroll
        for (int s = 0; s < NSMAX; ++s) {
          if (s < NSMAX - 3 || s < ns) x[g][s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(src + 8 * s));
        }
      }
    }
  };

  bf16* const myrow = srow[wave];
  // one 32x32 block of Z: look every element up, write the hits
  auto scatter = [&](const f32x16& z, int row0, int col0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = slut[(row0 + 8 * i + 4 * h + j) * MPAD + col0 + r];
        if ((unsigned)t < (unsigned)p.wlog) myrow[t] = f2bf(z[4 * i + j]);
      }
    }
  };

  const long stride = (long)gridDim.x * WAVES;
  long rec = (long)blockIdx.x * WAVES + wave;
  int id[G];
  bf16x8 x[G][NSMAX];
  if (rec < p.B) {
    load_ids(rec, id);
    load_rows(rec, id, x);
  }
  while (rec < p.B) {
    const long nrec = rec + stride;
    int nid[G];
    bf16x8 nx[G][NSMAX];
    if (nrec < p.B) {
      load_ids(nrec, nid);
      if constexpr (PREFETCH_ROWS) load_rows(nrec, nid, nx);
    }

    // the concat's first operand, straight from memory (the line a lane of the MFMA operand has just asked for)
    u32x4 dcopy = zero4;
    if (p.copy_dense && lane < (p.D >> 3)) dcopy = *reinterpret_cast<const u32x4*>(p.dense + rec * p.dense_pitch + 8 * lane);

    f32x16 z00, z10, z11;
#pragma unroll
    for (int e = 0; e < 16; ++e) z00[e] = 0.f, z10[e] = 0.f, z11[e] = 0.f;
#pragma unroll
    for (int s = 0; s < NSMAX; ++s) {
      if (s < NSMAX - 3 || s < ns) {  // NSMAX - 4 < ns <= NSMAX: only the last three steps are in question
        z00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[0][s], x[0][s], z00, 0, 0, 0);
        if constexpr (G == 2) {
          z10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[1][s], x[0][s], z10, 0, 0, 0);
          z11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[1][s], x[1][s], z11, 0, 0, 0);
        }
      }
    }

    // the row starts as zeros (a column no pair selects, and the tail), then the hits, then the copy: a wave's
    // LDS operations complete in order
    for (int c = lane; c < (wout >> 3); c += 64) *reinterpret_cast<u32x4*>(myrow + 8 * c) = zero4;
    scatter(z00, 0, 0);
    if constexpr (G == 2) {
      scatter(z10, 32, 0);
      scatter(z11, 32, 32);
    }
    if (p.copy_dense && lane < (p.D >> 3)) *reinterpret_cast<u32x4*>(myrow + 8 * lane) = dcopy;
    wave_lds_fence();
    bf16* const dst = p.out + rec * p.out_pitch;
    for (int c = lane; c < (wout >> 3); c += 64)
      *reinterpret_cast<u32x4*>(dst + 8 * c) = *reinterpret_cast<const u32x4*>(myrow + 8 * c);
    wave_lds_fence();  // the next record's hits come after these reads

    if (nrec < p.B) {
      if constexpr (PREFETCH_ROWS) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
          for (int s = 0; s < NSMAX; ++s) x[g][s] = nx[g][s];
        }
      } else {
        load_rows(nrec, nid, x);
      }
    }
    rec = nrec;
  }
}

__global__ __launch_bounds__(256) void embed_rows_kernel(const bf16* table, const int* ids, long base, long vocab,
                                                         long rows, long R, int D, bf16* out, long out_pitch) {
  const int vpr = D >> 3;  // 8-element vectors per row
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= R * vpr) return;
  const long rr = i / vpr;
  const int c = (int)(i % vpr) * 8;
  const long id = ids[rr];
  const long row = base + id;
  u32x4 v = {0u, 0u, 0u, 0u};
  if (id >= 0 && id < vocab && row >= 0 && row < rows) v = *reinterpret_cast<const u32x4*>(table + row * D + c);
  *reinterpret_cast<u32x4*>(out + rr * out_pitch + c) = v;
}

template <int G>
void launch_interact(const InteractParams& p, int workgroups, hipStream_t s) {
  const dim3 grid((unsigned)workgroups), block(WAVES * 64);
  if (p.D <= 64) hipLaunchKernelGGL((interact_kernel<4, G>), grid, block, 0, s, p);
  else if (p.D <= 128) hipLaunchKernelGGL((interact_kernel<8, G>), grid, block, 0, s, p);
  else if (p.D <= 192) hipLaunchKernelGGL((interact_kernel<12, G>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((interact_kernel<16, G>), grid, block, 0, s, p);
}

}  // namespace

// Pitches are in elements.  ``lut`` holds (M <= 32 ? 32 : 64)^2 entries, ``meta`` 3 M.  ``workgroups``
// is the grid: a wave takes records wave, wave + 4 workgroups, ...
void dot_interact(uintptr_t table, long rows, uintptr_t ids, long ids_pitch, int F, uintptr_t meta, uintptr_t lut,
                  uintptr_t dense, long dense_pitch, int copy_dense, int B, int M, int D, int wlog, uintptr_t out,
                  long out_pitch, int workgroups, uintptr_t stream) {
  if (B < 1) throw std::invalid_argument("dot_interact: empty batch");
  if (workgroups < 1 || workgroups > 65536) throw std::invalid_argument("dot_interact: workgroups must be 1..65536");
  if (M < 1 || M > 64) throw std::invalid_argument("dot_interact: M must be 1..64");
  if (D % 16 || D < 16 || D > 256) throw std::invalid_argument("dot_interact: D must be a multiple of 16 in 16..256");
  const int mpad = M <= 32 ? 32 : 64;
  const int wout = (wlog + 7) & ~7;
  if (wlog < 1 || wout > mpad * (mpad + 1) / 2 + 256) throw std::invalid_argument("dot_interact: output width outside the kernel's row buffer");
  if (copy_dense && (!dense || wlog < D)) throw std::invalid_argument("dot_interact: an activation copy needs the activation and Wlog >= D");
  if (!table || !ids || !meta || !lut || !out) throw std::invalid_argument("dot_interact: null pointer");
  if (rows < 0 || F < 1 || ids_pitch < F) throw std::invalid_argument("dot_interact: bad table rows or id pitch");
  if (table % 16 || ids % 4 || meta % 8 || lut % 16 || dense % 16 || out % 16 || dense_pitch % 8 || out_pitch % 8)
    throw std::invalid_argument("dot_interact: misaligned pointer or pitch");
  if (out_pitch < wout || (dense && dense_pitch < D)) throw std::invalid_argument("dot_interact: pitch below the row width");
  InteractParams p;
  p.table = reinterpret_cast<const bf16*>(table);
  p.ids = reinterpret_cast<const int*>(ids);
  p.meta = reinterpret_cast<const long*>(meta);
  p.lut = reinterpret_cast<const short*>(lut);
  p.dense = reinterpret_cast<const bf16*>(dense);
  p.out = reinterpret_cast<bf16*>(out);
  p.rows = rows, p.ids_pitch = ids_pitch, p.dense_pitch = dense_pitch, p.out_pitch = out_pitch;
  p.B = B, p.F = F, p.M = M, p.D = D, p.wlog = wlog, p.copy_dense = copy_dense;
  auto s = reinterpret_cast<hipStream_t>(stream);
  if (M <= 32) launch_interact<1>(p, workgroups, s);
  else launch_interact<2>(p, workgroups, s);
  FTM_CHECK_LAUNCH();
}

void embed_rows(uintptr_t table, long rows, uintptr_t ids, long base, long vocab, long R, int D, uintptr_t out,
                long out_pitch, uintptr_t stream) {
  if (R < 1) throw std::invalid_argument("embed_rows: no rows");
  if (D % 8 || D < 8) throw std::invalid_argument("embed_rows: D must be a positive multiple of 8");
  if (!table || !ids || !out) throw std::invalid_argument("embed_rows: null pointer");
  if (table % 16 || ids % 4 || out % 16 || out_pitch % 8 || out_pitch < D)
    throw std::invalid_argument("embed_rows: misaligned pointer or pitch");
  const long blocks = (R * (D / 8) + 255) / 256;
  if (blocks >= (1L << 31)) throw std::invalid_argument("embed_rows: more than 2^31 workgroups");
  hipLaunchKernelGGL(embed_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const bf16*>(table), reinterpret_cast<const int*>(ids), base, vocab, rows, R, D,
                     reinterpret_cast<bf16*>(out), out_pitch);
  FTM_CHECK_LAUNCH();
}

void register_interact(pybind11::module_& m) {
  m.def("dot_interact", &dot_interact);
  m.def("embed_rows", &embed_rows);
}
