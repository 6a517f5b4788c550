// Detection head: SSD box decoding and per-class greedy non-maximum suppression
// (TF CombinedNonMaxSuppression; graph/ops_nn.py:combined_nms_host is the definition).  Sort,
// IoU and a data-dependent greedy walk: nothing here is MFMA-shaped.  Two launches per batch,
// both deterministic (no atomics; nothing depends on how workgroups are scheduled).
//
//   nms_per_class   one workgroup of 256 threads per (image, class), image-major on grid.x.
//     1. keys    every box n < N gets the 64-bit key (order-preserving uint32 image of its
//                fp32 score) << 32 | ~n; score <= threshold, a NaN score and the tail up to the
//                padded size NP (a power of two >= 64) get key 0.  -0.0 counts as 0.0.  Keys are
//                unique, so a descending sort visits equal scores lower index first.  Scores
//                are read in place from [B, N, ld] at column class_offset + class (bf16 or fp32).
//     2. sort    bitonic, descending, NP keys in LDS, a compare-exchange pair per thread and step.
//     3. select  wave 0 walks the sorted keys 64 at a time.  Each lane loads (or decodes) its
//                candidate's box and tests it against every box already kept (LDS, <= max_per_class
//                of them); the chunk is then resolved in order with a __ballot mask: the lowest
//                live lane is kept and broadcast, later lanes drop out where iou > threshold.
//                Stops at max_per_class kept or at the first key 0.
//     out        count[b, c], and kept[b, c, k] = score image << 32 | (0xffff - c) << 16 |
//                (0xffff - n): the merge order (score desc, class asc, index asc) as one integer.
//   nms_merge       one workgroup per image: the top T of the <= C * max_per_class kept keys.
//     Every class list is already sorted, so this is a T-round tournament, not a sort: thread c
//     holds the head of class c's list (its next 16 keys staged in LDS), a round takes the
//     largest head of the workgroup (wave shuffles, one barrier) and the one class that owns it
//     moves on.  Cost grows with T, not with C * max_per_class (which can be 65536 keys, 512 KiB,
//     more than LDS holds): a bitonic sort of the kept keys in 4096-key passes took 504 us for
//     9000 keys on an MI355X, more than the per-class kernel; a rank-by-count select would cost
//     C binary searches per key.  Then thread t < T gathers box t, clips it if asked and writes
//     the four outputs; rows past valid = min(kept, T) are zero.
//
// Boxes come in one of four forms (box_mode), loaded by load_box() in both kernels, so that
// the merge needs no decoded copy: 0 = fp32 [B, N, 4], 1 = bf16 [B, N, 4], 2 / 3 = fused decode of
// bf16 / fp32 encodings [B, N, 4] = (ty, tx, th, tw) with an fp32 anchor table [N, 4] = (yc, xc, h, w)
// and four reciprocal scale factors, in fp32, every operation rounded, in this order
// (ops_nn.py:decode_boxes_yxhw is the host mirror):
//     cy = (ty * s0) * ha + yca            cx = (tx * s1) * wa + xca
//     h  = expf(th * s2) * ha              w  = expf(tw * s3) * wa
//     box = (cy - 0.5 h, cx - 0.5 w, cy + 0.5 h, cx + 0.5 w)
//
// IoU, as the reference: corners canonicalised by min / max, area = (y2 - y1) * (x2 - x1),
// inter = max(0, min(y2) - max(y1)) * max(0, min(x2) - max(x1)), iou = inter / ((area_a +
// area_b) - inter) with the correctly rounded fp32 division (hipcc's default), 0 when either
// area is <= 0.  The build has -ffp-contract=fast, which also overrides a contract(off) pragma
// (and __fmul_rn / __fadd_rn are plain operators to the compiler), and an FMA would skip a
// rounding that the reference makes.  Every product that the reference rounds before a sum or a
// difference goes through rnd(), an empty asm the optimiser cannot see through: the decode, the
// areas and the IoU then have no contraction left in the ISA but the exact 0.5 * h.
//
// Every index into scores / boxes is 64-bit.
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace {

constexpr int NMS_THREADS = 256;
constexpr int NMS_MAX_N = 4096;    // per-class keys: 4096 * 8 B = 32 KiB of LDS
constexpr int NMS_MAX_KEEP = 256;  // kept boxes + areas: 256 * 20 B = 5 KiB of LDS
constexpr int NMS_MAX_C = 256;     // merge: one class per thread
constexpr int NMS_WINDOW = 16;     // merge: keys staged per class, 16 * 256 * 8 B = 32 KiB of LDS
constexpr int NMS_MAX_T = 1024;    // merge: the merged keys, 8 KiB of LDS

struct NmsParams {
  const void* boxes;     // box_mode 0: fp32, 1: bf16, 2: bf16 encodings, 3: fp32 encodings
  const float* anchors;  // box_mode 2, 3
  float s0, s1, s2, s3;  // box_mode 2, 3
  const void* scores;
  int scores_f32;
  int box_mode;
  int B, N, C, NP;
  int ld, coff;  // scores row pitch and first class column
  int max_keep, T;
  float iou_thr, score_thr;
  int clip;
  unsigned long long* kept;  // [B, C, max_keep]
  int* count;                // [B, C]
};

struct Box {
  float y1, x1, y2, x2;
};

FTM_DEVICE uint32_t score_image(float s) {
  const uint32_t u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
FTM_DEVICE float image_score(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the value as rounded to fp32: a contraction barrier (see the header)
FTM_DEVICE float rnd(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

FTM_DEVICE Box load_box(const NmsParams& p, int b, int n) {
  const long at = ((long)b * p.N + n) * 4;
  Box r;  // the four stored numbers: corners, or (ty, tx, th, tw)
  if (p.box_mode == 0 || p.box_mode == 3) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.boxes) + at);
    r.y1 = v[0], r.x1 = v[1], r.y2 = v[2], r.x2 = v[3];
  } else {
    const bf16x4 e = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16*>(p.boxes) + at);
    r.y1 = bf2f(e[0]), r.x1 = bf2f(e[1]), r.y2 = bf2f(e[2]), r.x2 = bf2f(e[3]);
  }
  if (p.box_mode < 2) return r;
  const f32x4 a = *reinterpret_cast<const f32x4*>(p.anchors + (long)n * 4);
  const float cy = rnd(rnd(r.y1 * p.s0) * a[2]) + a[0];
  const float cx = rnd(rnd(r.x1 * p.s1) * a[3]) + a[1];
  const float h = rnd(expf(rnd(r.y2 * p.s2)) * a[2]);
  const float w = rnd(expf(rnd(r.x2 * p.s3)) * a[3]);
  const float hh = 0.5f * h;  // exact: fusing it into the corners changes nothing
  const float hw = 0.5f * w;
  r.y1 = cy - hh, r.x1 = cx - hw, r.y2 = cy + hh, r.x2 = cx + hw;
  return r;
}

FTM_DEVICE Box canonical(const Box& v) {
  Box r;
  r.y1 = fminf(v.y1, v.y2), r.y2 = fmaxf(v.y1, v.y2);
  r.x1 = fminf(v.x1, v.x2), r.x2 = fmaxf(v.x1, v.x2);
  return r;
}

FTM_DEVICE float box_area(const Box& c) {
  return rnd((c.y2 - c.y1) * (c.x2 - c.x1));
}

// a, b canonical
FTM_DEVICE float iou(const Box& a, float area_a, const Box& b, float area_b) {
  if (!(area_a > 0.f) || !(area_b > 0.f)) return 0.f;
  const float iy = fmaxf(0.f, fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1));
  const float ix = fmaxf(0.f, fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1));
  const float inter = rnd(iy * ix);
  if (!(inter > 0.f)) return 0.f;  // 0 / union: most pairs, and no wave then pays for the division
  const float uni = (area_a + area_b) - inter;
  return inter / uni;
}

// descending bitonic sort of n (a power of two) keys in LDS, by all NMS_THREADS threads
FTM_DEVICE void bitonic_desc(unsigned long long* keys, int n) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < n / 2; t += NMS_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // pair t: bit j clear, partner i | j
        const int l = i | j;
        const unsigned long long a = keys[i], b = keys[l];
        const bool desc = (i & k) == 0;
        if (desc ? a < b : a > b) {
          keys[i] = b;
          keys[l] = a;
        }
      }
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(NMS_THREADS) void nms_per_class_kernel(const NmsParams p) {
  // dynamic LDS, sized by the launch: NP keys, then max_keep kept boxes and their areas
  extern __shared__ __attribute__((aligned(16))) unsigned char nms_lds[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(nms_lds);
  float* kbox = reinterpret_cast<float*>(nms_lds + (size_t)p.NP * 8);
  float* karea = kbox + 4 * p.max_keep;
  const int c = blockIdx.x % p.C, b = blockIdx.x / p.C;
  const long srow = (long)b * p.N;
  for (int n = threadIdx.x; n < p.NP; n += NMS_THREADS) {
    unsigned long long key = 0;
    if (n < p.N) {
      const long at = (srow + n) * p.ld + p.coff + c;
      float s = p.scores_f32 ? reinterpret_cast<const float*>(p.scores)[at]
                             : bf2f(reinterpret_cast<const bf16*>(p.scores)[at]);
      s = s + 0.f;  // -0.0 -> 0.0
      if (s > p.score_thr) key = ((unsigned long long)score_image(s) << 32) | (uint32_t)~(uint32_t)n;
    }
    keys[n] = key;
  }
  bitonic_desc(keys, p.NP);
  if (threadIdx.x >= 64) return;  // the walk is one wave; no barrier follows

  const int lane = threadIdx.x;
  const long obase = ((long)b * p.C + c) * p.max_keep;
  const unsigned long long cls_bits = (unsigned long long)(0xffffu - (unsigned)c) << 16;
  int nkept = 0;
  for (int base = 0; base < p.NP && nkept < p.max_keep; base += 64) {
    const unsigned long long key = keys[base + lane];
    bool live = key != 0;
    const bool last = __ballot(!live) != 0;  // sorted: a key 0 ends the candidates
    const int n = live ? (int)~(uint32_t)key : 0;
    const Box cb = canonical(load_box(p, b, n));
    const float ca = box_area(cb);
    for (int k = 0; k < nkept; ++k) {
      Box kb;
      kb.y1 = kbox[4 * k], kb.x1 = kbox[4 * k + 1], kb.y2 = kbox[4 * k + 2], kb.x2 = kbox[4 * k + 3];
      if (iou(cb, ca, kb, karea[k]) > p.iou_thr) live = false;
    }
    unsigned long long mask = __ballot(live);
    while (mask != 0 && nkept < p.max_keep) {
      const int j = __builtin_ctzll(mask);
      Box kb;
      kb.y1 = __shfl(cb.y1, j, 64), kb.x1 = __shfl(cb.x1, j, 64);
      kb.y2 = __shfl(cb.y2, j, 64), kb.x2 = __shfl(cb.x2, j, 64);
      const float ka = __shfl(ca, j, 64);
      if (lane == j) {
        kbox[4 * nkept] = cb.y1, kbox[4 * nkept + 1] = cb.x1, kbox[4 * nkept + 2] = cb.y2, kbox[4 * nkept + 3] = cb.x2;
        karea[nkept] = ca;
        p.kept[obase + nkept] = (key & 0xffffffff00000000ull) | cls_bits | (0xffffu - (unsigned)n);
        live = false;
      }
      if (live && lane > j && iou(cb, ca, kb, ka) > p.iou_thr) live = false;
      ++nkept;
      mask = __ballot(live);  // only lanes above j can still be live
    }
    __threadfence_block();  // the next chunk reads the kept boxes this one wrote (same wave)
    if (last) break;
  }
  if (lane == 0) p.count[(long)b * p.C + c] = nkept;
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

__global__ __launch_bounds__(NMS_THREADS) void nms_merge_kernel(const NmsParams p, float* out_boxes, float* out_scores,
                                                               float* out_classes, int* out_valid) {
  __shared__ unsigned long long win[NMS_WINDOW * NMS_THREADS];  // win[k * 256 + class]: its next keys
  __shared__ unsigned long long buf[NMS_MAX_T];                 // the merged keys, best first
  __shared__ unsigned long long wmax[2][NMS_THREADS / 64];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  // thread = class (C <= 256): a cursor into that class's kept list, which is sorted; only its
  // first T keys can reach the top T
  const long base = ((long)b * p.C + tid) * p.max_keep;
  int cnt = tid < p.C ? p.count[(long)b * p.C + tid] : 0;
  cnt = cnt < p.T ? cnt : p.T;
  int pos = 0, wbase = 0;
  for (int k = 0; k < NMS_WINDOW; ++k) win[k * NMS_THREADS + tid] = k < cnt ? p.kept[base + k] : 0;
  unsigned long long head = win[tid];
  int t = 0;
  for (; t < p.T; ++t) {
    const unsigned long long m = wave_max_u64(head);
    if ((tid & 63) == 0) wmax[t & 1][tid >> 6] = m;
    __syncthreads();  // one barrier a round: round t + 2 rewrites this half only after the barrier of t + 1
    unsigned long long g = wmax[t & 1][0];
#pragma unroll
    for (int w = 1; w < NMS_THREADS / 64; ++w) g = wmax[t & 1][w] > g ? wmax[t & 1][w] : g;
    if (g == 0) break;  // every list is used up (the same g in every thread)
    if (head == g) {    // keys are unique: exactly one class wins
      buf[t] = g;
      ++pos;
      if (pos >= cnt) {
        head = 0;
      } else {
        if (pos - wbase == NMS_WINDOW) {  // window used up: the class's next keys
          wbase = pos;
          for (int k = 0; k < NMS_WINDOW; ++k) win[k * NMS_THREADS + tid] = pos + k < cnt ? p.kept[base + pos + k] : 0;
        }
        head = win[(pos - wbase) * NMS_THREADS + tid];
      }
    }
  }
  const int total = t;  // min(kept keys, T)
  __syncthreads();
  for (int t = tid; t < p.T; t += NMS_THREADS) {
    const unsigned long long key = t < total ? buf[t] : 0;
    Box r;
    r.y1 = r.x1 = r.y2 = r.x2 = 0.f;
    float score = 0.f, cls = 0.f;
    if (key != 0) {
      const int n = 0xffff - (int)(key & 0xffffu);
      cls = (float)(0xffff - (int)((key >> 16) & 0xffffu));
      score = image_score((uint32_t)(key >> 32));
      r = load_box(p, b, n);
      if (p.clip) {
        r.y1 = fminf(fmaxf(r.y1, 0.f), 1.f), r.x1 = fminf(fmaxf(r.x1, 0.f), 1.f);
        r.y2 = fminf(fmaxf(r.y2, 0.f), 1.f), r.x2 = fminf(fmaxf(r.x2, 0.f), 1.f);
      }
    }
    const long o = (long)b * p.T + t;
    f32x4 v;
    v[0] = r.y1, v[1] = r.x1, v[2] = r.y2, v[3] = r.x2;
    *reinterpret_cast<f32x4*>(out_boxes + o * 4) = v;
    out_scores[o] = score;
    out_classes[o] = cls;
  }
  if (tid == 0) out_valid[b] = total;
}

}  // namespace

// LDS: nms_per_class takes NP * 8 B of keys + max_keep * 20 B of kept boxes and areas as dynamic
// LDS, at most 32 KiB + 5 KiB (under 64 KiB: no function attribute to set) and 18 KiB for an SSD
// (N = 1917, 100 kept), so that eight workgroups share a CU's 160 KiB; nms_merge has 32 KiB of
// staged keys + 8 KiB of merged keys, static.  The limits below are those sizes; the kept keys
// carry class and box index in 16 bits each.
// box_mode: 0 fp32 boxes, 1 bf16 boxes, 2 / 3 bf16 / fp32 encodings + anchors + scales.  scratch_kept holds
// B * C * max_keep 8-byte keys, scratch_count B * C ints.
void combined_nms(uintptr_t boxes, int box_mode, uintptr_t anchors, float s0, float s1, float s2, float s3,
                  uintptr_t scores, bool scores_f32, int B, int N, int C, int ld, int coff, int max_keep, int T,
                  float iou_thr, float score_thr, bool clip, uintptr_t scratch_kept, uintptr_t scratch_count,
                  uintptr_t out_boxes, uintptr_t out_scores, uintptr_t out_classes, uintptr_t out_valid,
                  uintptr_t stream) {
  if (B < 1 || N < 1 || C < 1 || max_keep < 1 || T < 1) throw std::invalid_argument("combined_nms: empty problem");
  if ((long)B * C >= (1L << 31)) throw std::invalid_argument("combined_nms: more than 2^31 (image, class) pairs");
  if (N > NMS_MAX_N) throw std::invalid_argument("combined_nms: N exceeds 4096");
  if (C > NMS_MAX_C) throw std::invalid_argument("combined_nms: C exceeds 256");
  if (max_keep > NMS_MAX_KEEP) throw std::invalid_argument("combined_nms: max_per_class exceeds 256");
  if (T > NMS_MAX_T) throw std::invalid_argument("combined_nms: max_total exceeds 1024");
  if (box_mode < 0 || box_mode > 3) throw std::invalid_argument("combined_nms: box_mode must be 0..3");
  if (coff < 0 || coff + C > ld) throw std::invalid_argument("combined_nms: class columns exceed the scores row");
  if (boxes % (box_mode % 3 == 0 ? 16 : 8) || (box_mode >= 2 && (anchors == 0 || anchors % 16)) || out_boxes % 16 ||
      scratch_kept % 8 || scratch_count % 4)
    throw std::invalid_argument("combined_nms: misaligned pointer");
  int NP = 64;
  while (NP < N) NP <<= 1;
  NmsParams p;
  p.boxes = reinterpret_cast<const void*>(boxes);
  p.anchors = reinterpret_cast<const float*>(anchors);
  p.s0 = s0, p.s1 = s1, p.s2 = s2, p.s3 = s3;
  p.scores = reinterpret_cast<const void*>(scores);
  p.scores_f32 = scores_f32 ? 1 : 0;
  p.box_mode = box_mode;
  p.B = B, p.N = N, p.C = C, p.NP = NP;
  p.ld = ld, p.coff = coff;
  p.max_keep = max_keep, p.T = T;
  p.iou_thr = iou_thr, p.score_thr = score_thr;
  p.clip = clip ? 1 : 0;
  p.kept = reinterpret_cast<unsigned long long*>(scratch_kept);
  p.count = reinterpret_cast<int*>(scratch_count);
  auto s = reinterpret_cast<hipStream_t>(stream);
  const size_t lds = (size_t)NP * 8 + (size_t)max_keep * 20;
  hipLaunchKernelGGL(nms_per_class_kernel, dim3((unsigned)(B * C)), dim3(NMS_THREADS), lds, s, p);
  FTM_CHECK_LAUNCH();
  hipLaunchKernelGGL(nms_merge_kernel, dim3(B), dim3(NMS_THREADS), 0, s, p, reinterpret_cast<float*>(out_boxes),
                     reinterpret_cast<float*>(out_scores), reinterpret_cast<float*>(out_classes),
                     reinterpret_cast<int*>(out_valid));
  FTM_CHECK_LAUNCH();
}

void register_detection(pybind11::module_& m) { m.def("combined_nms", &combined_nms); }
