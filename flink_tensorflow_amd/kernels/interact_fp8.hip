// Ranking on 8-bit embedding tables: dot_interact and embed_rows (interact.hip) for tables stored
// as OCP e4m3 codes with one power-of-two exponent per row.  ops/kernels.py:quantize_table_fp8
// holds the format, dot_interact / embed_rows (table_exp=...) the host definitions.
//
//   codes [rows, D] uint8    e4m3fn bytes (0x7F / 0xFF never stored)
//   exps  [rows]    int8     value[r, d] = e4m3(codes[r, d]) * 2^exps[r], -32 <= exps[r] <= 31
//
//   Every value has 4 significant bits and a magnitude in [2^-41, 448 * 2^31]: exact in bf16.  So
//   a lane widens its codes to the very bf16 operands interact.hip would have loaded from the
//   dequantised table, the MFMAs see the same registers, and the output has the same bits.
//
// dot_interact_fp8   the contract of dot_interact (meta, lut, dense, copy_dense, pitches, zero
//   vectors for ids outside [0, V), 64-bit offsets), a row being D + 1 bytes instead of 2 D.
//
//   interact_fp8_kernel<NSMAX, G, PREFETCH_ROWS>: 4 waves, a wave owns one record at a time; lane
//   l holds vector (l & 31) of a row group and k-group h = l >> 5, as in interact.hip.
//   * loads      a lane's share of a vector is the D / 2 contiguous bytes at h D / 2 and step s
//                consumes its bytes [8 s, 8 s + 8): the columns interact.hip gives step s.  That
//                is what the equal bits rest on: fp32 rounds once per MFMA, so another split of
//                the columns over the steps, free as far as the sum goes, would round
//                differently.  With q = D / 32 the share is q 16-byte loads (two steps each) and,
//                when D % 32 == 16, an 8-byte tail (step 2 q); in that case half 1 starts 8 bytes
//                off a 16-byte boundary, so the loads are declared 8-byte aligned (global loads
//                take that; still one global_load_dwordx4 each).  The exponent byte's address
//                depends on the id alone: its load is issued ahead of the row loads.
//   * operands   stay packed, two VGPRs a step (interact.hip: four).  Right before its MFMA a
//                step is widened: 4 v_cvt_pk_f32_fp8, 8 v_mul_f32 by 2^k (exact), 4 v_perm_b32
//                that keep the high halves (exact: 4 significant bits).  The fused gfx950
//                conversions with a scale operand (v_cvt_scalef32_pk_bf16_fp8) were not tried.
//   * activation the one vector that is bf16 in memory.  It does not go through the lane's
//                operand registers (a bf16 set in every lane for the sake of two): D / 8 lanes
//                load the record's vector once, for the copy into the output row as well, the
//                wave keeps it in LDS and the two lanes that own it read each step from there.
//                The next record's vector is requested with the next record's ids.
//   * prefetch   the next record's ids and activation vector are always requested before the
//                current record's MFMAs; its exponents and rows too wherever the second packed
//                set leaves four waves a SIMD or costs none (the table; a choice by the compiled
//                register counts, not yet timed).  interact.hip prefetches rows in <4, 1>, <8, 1>
//                and <4, 2> only.
//   * epilogue   as in interact.hip: LUT in LDS, hits into the wave's LDS row, 16-byte row stores.
//
//   Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): VGPRs + AGPRs -> waves per
//   SIMD; scratch is 0 bytes in all sixteen.  The last column is interact.hip's VGPRs -> waves.
//     <NSMAX, G>   row prefetch on    off               chosen   interact.hip
//     < 4, 1>       62 + 16 -> 6       62 + 16 -> 6     on        72 -> 5
//     < 8, 1>       82 + 16 -> 4       70 + 16 -> 5     on       104 -> 4
//     <12, 1>       96 + 16 -> 4       78 + 16 -> 5     on        94 -> 4
//     <16, 1>      108 + 16 -> 4       86 + 16 -> 4     on       110 -> 4
//     < 4, 2>      126 + 48 -> 2      110 + 48 -> 3     off      152 -> 2
//     < 8, 2>      160 + 48 -> 2      126 + 48 -> 2     on       152 -> 2
//     <12, 2>      192 + 48 -> 2      142 + 48 -> 2     on       184 -> 2
//     <16, 2>      224 + 48 -> 1      158 + 48 -> 2     off      216 -> 1
//
//   Static LDS: interact.hip's (LUT + 4 output rows) + 4 activation vectors of 256 bf16:
//   10,368 B (G = 1), 28,928 B (G = 2).
//
// embed_rows_fp8   out[r, :] = bf16(value[base + ids[r]]), D % 16 == 0: one thread per 16 codes,
//   one 16-byte load, two 16-byte stores; an id outside [0, V) gives zeros; out has a row pitch.
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace {

constexpr int WAVES = 4;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef u32x4 u32x4_a8 __attribute__((aligned(8)));  // a 16-byte load from an 8-byte boundary

struct InteractFp8Params {
  const uint8_t* codes;
  const int8_t* exps;
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

// 2^k for -32 <= k <= 31
FTM_DEVICE float exp_scale(int k) { return __builtin_bit_cast(float, (uint32_t)(127 + k) << 23); }

// the high halves of two floats as two bf16 (no rounding: the caller's values have 4 significant bits)
FTM_DEVICE uint32_t high_halves(float lo, float hi) {
  return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, hi), __builtin_bit_cast(uint32_t, lo), 0x07060302u);
}

// 8 e4m3 codes (memory order) times ``sc`` = 2^k as 8 bf16
FTM_DEVICE bf16x8 widen8(u32x2 c, float sc) {
  u32x4 w;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], false);
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], true);
    w[2 * i] = high_halves(a[0] * sc, a[1] * sc);
    w[2 * i + 1] = high_halves(b[0] * sc, b[1] * sc);
  }
  return __builtin_bit_cast(bf16x8, w);
}

template <int NSMAX, int G, bool PREFETCH_ROWS>
__global__ __launch_bounds__(WAVES * 64) void interact_fp8_kernel(const InteractFp8Params p) {
  constexpr int MPAD = 32 * G;
  constexpr int WMAX = MPAD * (MPAD + 1) / 2 + 256;
  constexpr int NC = NSMAX / 2;  // 16-byte loads of a lane at the instantiation's largest D
  static_assert(WMAX % 8 == 0 && (MPAD * MPAD) % 8 == 0, "16-byte chunks of the row and the LUT");
  __shared__ __attribute__((aligned(16))) short slut[MPAD * MPAD];
  __shared__ __attribute__((aligned(16))) bf16 srow[WAVES][WMAX];
  __shared__ __attribute__((aligned(16))) bf16 sden[WAVES][256];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 31;  // vector within a row group; accumulator column
  const int h = lane >> 5;  // k-group: which half of the vector this lane holds
  const int ns = p.D >> 4;  // MFMA steps; NSMAX - 4 < ns <= NSMAX
  const int nfull = p.D >> 5;  // 16-byte loads of this lane; NC - 2 <= nfull <= NC
  const bool tail = (p.D & 16) != 0;
  const int half_off = h * (p.D >> 1);  // bytes of codes, elements of the activation vector
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
  const u32x2 zero2 = {0u, 0u};
  auto load_ids = [&](long rec, int (&id)[G]) {
#pragma unroll
    for (int g = 0; g < G; ++g) id[g] = kind[g] == 1 ? p.ids[rec * p.ids_pitch + col[g]] : 0;
  };
  // the activation vector of a record, 8 elements a lane: the concat's first operand and the MFMA operand of its lanes
  auto load_dense = [&](long rec) {
    u32x4 v = zero4;
    if (p.dense != nullptr && lane < (p.D >> 3)) v = *reinterpret_cast<const u32x4*>(p.dense + rec * p.dense_pitch + 8 * lane);
    return v;
  };
  auto load_rows = [&](const int (&id)[G], u32x2 (&x)[G][NSMAX], int (&k)[G]) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const uint8_t* src = nullptr;
      k[g] = 0;
      if (kind[g] == 1) {
        const long row = base[g] + id[g];
        if (id[g] >= 0 && id[g] < vocab[g] && row >= 0 && row < p.rows) {
          k[g] = p.exps[row];  // first: it is as far away as the row
          src = p.codes + row * p.D + half_off;
        }
      }
#pragma unroll
      for (int s = 0; s < NSMAX; ++s) x[g][s] = zero2;
      if (src != nullptr) {  // one lane predicate for the whole vector; the bounds below are wave-uniform
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (c < NC - 2 || c < nfull) {
            const u32x4 v = *reinterpret_cast<const u32x4_a8*>(src + 16 * c);
            x[g][2 * c] = u32x2{v[0], v[1]};
            x[g][2 * c + 1] = u32x2{v[2], v[3]};
          } else if (c == nfull && tail) {
            x[g][2 * c] = *reinterpret_cast<const u32x2*>(src + 16 * c);
          }
        }
      }
    }
  };

  bf16* const myrow = srow[wave];
  bf16* const myden = sden[wave];
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
  int id[G], k[G];
  u32x2 x[G][NSMAX];
  u32x4 dvec = zero4;
  if (rec < p.B) {
    load_ids(rec, id);
    dvec = load_dense(rec);
    load_rows(id, x, k);
  }
  while (rec < p.B) {
    const long nrec = rec + stride;
    int nid[G], nk[G];
    u32x2 nx[G][NSMAX];
    u32x4 ndvec = zero4;
    if (nrec < p.B) {
      load_ids(nrec, nid);
      ndvec = load_dense(nrec);
      if constexpr (PREFETCH_ROWS) load_rows(nid, nx, nk);
    }

    if (p.dense != nullptr) {
      if (lane < (p.D >> 3)) *reinterpret_cast<u32x4*>(myden + 8 * lane) = dvec;
      wave_lds_fence();
    }

    float sc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) sc[g] = exp_scale(k[g]);
    f32x16 z00, z10, z11;
#pragma unroll
    for (int e = 0; e < 16; ++e) z00[e] = 0.f, z10[e] = 0.f, z11[e] = 0.f;
#pragma unroll
    for (int s = 0; s < NSMAX; ++s) {
      if (s < NSMAX - 3 || s < ns) {  // only the last three steps are in question
        bf16x8 a[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          a[g] = widen8(x[g][s], sc[g]);
          // the activation vector's lanes: this step's columns, as the loads above split them.  half_off is 8
          // elements off a 16-byte boundary when D % 32 == 16: two 8-byte LDS reads
          if (kind[g] == 2) {
            const u32x2* d = reinterpret_cast<const u32x2*>(myden + half_off + 8 * s);
            a[g] = __builtin_bit_cast(bf16x8, u32x4{d[0][0], d[0][1], d[1][0], d[1][1]});
          }
        }
        z00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], a[0], z00, 0, 0, 0);
        if constexpr (G == 2) {
          z10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], a[0], z10, 0, 0, 0);
          z11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], a[1], z11, 0, 0, 0);
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
    if (p.copy_dense && lane < (p.D >> 3)) *reinterpret_cast<u32x4*>(myrow + 8 * lane) = dvec;
    wave_lds_fence();
    bf16* const dst = p.out + rec * p.out_pitch;
    for (int c = lane; c < (wout >> 3); c += 64)
      *reinterpret_cast<u32x4*>(dst + 8 * c) = *reinterpret_cast<const u32x4*>(myrow + 8 * c);
    wave_lds_fence();  // the next record's hits and activation vector come after these reads

    if (nrec < p.B) {
      if constexpr (PREFETCH_ROWS) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          k[g] = nk[g];
#pragma unroll
          for (int s = 0; s < NSMAX; ++s) x[g][s] = nx[g][s];
        }
      } else {
        load_rows(nid, x, k);
      }
      dvec = ndvec;
    }
    rec = nrec;
  }
}

__global__ __launch_bounds__(256) void embed_rows_fp8_kernel(const uint8_t* codes, const int8_t* exps, const int* ids,
                                                             long base, long vocab, long rows, long R, int D, bf16* out,
                                                             long out_pitch) {
  const int vpr = D >> 4;  // 16-code vectors per row
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= R * vpr) return;
  const long rr = i / vpr;
  const int c = (int)(i % vpr) * 16;
  const long id = ids[rr];
  const long row = base + id;
  u32x4 v = {0u, 0u, 0u, 0u};
  int k = 0;
  if (id >= 0 && id < vocab && row >= 0 && row < rows) {
    k = exps[row];
    v = *reinterpret_cast<const u32x4*>(codes + row * D + c);
  }
  const float sc = exp_scale(k);
  bf16* const dst = out + rr * out_pitch + c;
  *reinterpret_cast<bf16x8*>(dst) = widen8(u32x2{v[0], v[1]}, sc);
  *reinterpret_cast<bf16x8*>(dst + 8) = widen8(u32x2{v[2], v[3]}, sc);
}

template <int NSMAX, int G, bool PREFETCH_ROWS>
void launch_one(const InteractFp8Params& p, int workgroups, hipStream_t s) {
  hipLaunchKernelGGL((interact_fp8_kernel<NSMAX, G, PREFETCH_ROWS>), dim3((unsigned)workgroups), dim3(WAVES * 64), 0, s, p);
}

}  // namespace

// Pitches are in elements.  ``lut`` holds (M <= 32 ? 32 : 64)^2 entries, ``meta`` 3 M, ``exps`` ``rows``
// bytes.  ``workgroups`` is the grid: a wave takes records wave, wave + 4 workgroups, ...
void dot_interact_fp8(uintptr_t codes, uintptr_t exps, long rows, uintptr_t ids, long ids_pitch, int F, uintptr_t meta,
                      uintptr_t lut, uintptr_t dense, long dense_pitch, int copy_dense, int B, int M, int D, int wlog,
                      uintptr_t out, long out_pitch, int workgroups, uintptr_t stream) {
  if (B < 1) throw std::invalid_argument("dot_interact_fp8: empty batch");
  if (workgroups < 1 || workgroups > 65536) throw std::invalid_argument("dot_interact_fp8: workgroups must be 1..65536");
  if (M < 1 || M > 64) throw std::invalid_argument("dot_interact_fp8: M must be 1..64");
  if (D % 16 || D < 16 || D > 256) throw std::invalid_argument("dot_interact_fp8: D must be a multiple of 16 in 16..256");
  const int mpad = M <= 32 ? 32 : 64;
  const int wout = (wlog + 7) & ~7;
  if (wlog < 1 || wout > mpad * (mpad + 1) / 2 + 256) throw std::invalid_argument("dot_interact_fp8: output width outside the kernel's row buffer");
  if (copy_dense && (!dense || wlog < D)) throw std::invalid_argument("dot_interact_fp8: an activation copy needs the activation and Wlog >= D");
  if (!codes || !exps || !ids || !meta || !lut || !out) throw std::invalid_argument("dot_interact_fp8: null pointer");
  if (rows < 0 || F < 1 || ids_pitch < F) throw std::invalid_argument("dot_interact_fp8: bad table rows or id pitch");
  if (codes % 16 || ids % 4 || meta % 8 || lut % 16 || dense % 16 || out % 16 || dense_pitch % 8 || out_pitch % 8)
    throw std::invalid_argument("dot_interact_fp8: misaligned pointer or pitch");
  if (out_pitch < wout || (dense && dense_pitch < D)) throw std::invalid_argument("dot_interact_fp8: pitch below the row width");
  InteractFp8Params p;
  p.codes = reinterpret_cast<const uint8_t*>(codes);
  p.exps = reinterpret_cast<const int8_t*>(exps);
  p.ids = reinterpret_cast<const int*>(ids);
  p.meta = reinterpret_cast<const long*>(meta);
  p.lut = reinterpret_cast<const short*>(lut);
  p.dense = reinterpret_cast<const bf16*>(dense);
  p.out = reinterpret_cast<bf16*>(out);
  p.rows = rows, p.ids_pitch = ids_pitch, p.dense_pitch = dense_pitch, p.out_pitch = out_pitch;
  p.B = B, p.F = F, p.M = M, p.D = D, p.wlog = wlog, p.copy_dense = copy_dense;
  auto s = reinterpret_cast<hipStream_t>(stream);
  const int nsmax = (D + 63) / 64 * 4;
  // the row prefetch per instantiation: the register table in the header
  if (M <= 32) {
    if (nsmax == 4) launch_one<4, 1, true>(p, workgroups, s);
    else if (nsmax == 8) launch_one<8, 1, true>(p, workgroups, s);
    else if (nsmax == 12) launch_one<12, 1, true>(p, workgroups, s);
    else launch_one<16, 1, true>(p, workgroups, s);
  } else {
    if (nsmax == 4) launch_one<4, 2, false>(p, workgroups, s);
    else if (nsmax == 8) launch_one<8, 2, true>(p, workgroups, s);
    else if (nsmax == 12) launch_one<12, 2, true>(p, workgroups, s);
    else launch_one<16, 2, false>(p, workgroups, s);
  }
  FTM_CHECK_LAUNCH();
}

void embed_rows_fp8(uintptr_t codes, uintptr_t exps, long rows, uintptr_t ids, long base, long vocab, long R, int D,
                    uintptr_t out, long out_pitch, uintptr_t stream) {
  if (R < 1) throw std::invalid_argument("embed_rows_fp8: no rows");
  if (D % 16 || D < 16) throw std::invalid_argument("embed_rows_fp8: D must be a positive multiple of 16");
  if (!codes || !exps || !ids || !out) throw std::invalid_argument("embed_rows_fp8: null pointer");
  if (rows < 0 || codes % 16 || ids % 4 || out % 16 || out_pitch % 8 || out_pitch < D)
    throw std::invalid_argument("embed_rows_fp8: misaligned pointer or pitch");
  const long blocks = (R * (D / 16) + 255) / 256;
  if (blocks >= (1L << 31)) throw std::invalid_argument("embed_rows_fp8: more than 2^31 workgroups");
  hipLaunchKernelGGL(embed_rows_fp8_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const uint8_t*>(codes), reinterpret_cast<const int8_t*>(exps),
                     reinterpret_cast<const int*>(ids), base, vocab, rows, R, D, reinterpret_cast<bf16*>(out), out_pitch);
  FTM_CHECK_LAUNCH();
}

void register_interact_fp8(pybind11::module_& m) {
  m.def("dot_interact_fp8", &dot_interact_fp8);
  m.def("embed_rows_fp8", &embed_rows_fp8);
}
