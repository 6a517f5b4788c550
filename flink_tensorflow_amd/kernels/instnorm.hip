// Instance normalisation of bf16 NHWC activations (style-transfer / CycleGAN generators):
//
//   y[n, p, c] = act((x[n, p, c] - m[n, c]) * a[n, c] + beta[c]),   a = gamma[c] / sqrt(v[n, c] + eps)
//
// m and v are the mean and the biased variance over the P = H * W pixels of one image and channel.
// x is bf16, every operation is fp32, the one rounding to bf16 is at the store.  The result is
// written once, at channel offset y_coff of a pixel of pitch ldy (a concat slot).
//
// Three launches on one stream, all with 16-byte loads and stores and 64-bit offsets:
//
//   in_stats_kernel     grid (chunks, N, groups).  A workgroup owns one pixel chunk of one image
//       and one group of up to 256 channel vectors (8 channels each).  Its 256 threads are laid
//       out as R rows of L lanes, L = vectors of the group, R = 256 / L; lane l of row r reads the
//       vector l of the pixels r, r + R, .. (IN_PT = 8 of them, held in registers; pixels past P
//       are predicated off, never clamped), takes their mean, then the sum of squared distances
//       from that mean, and the rows are merged pairwise in LDS with Chan's update
//       (mean, M2, count).  The chunk's (mean, M2) per channel goes to the scratch.
//   in_finalize_kernel  grid (C / 32, N).  32 channels x 8 slices: slice j merges the chunks
//       j, j + 8, .. in that order, the 8 slices are merged pairwise in LDS; (m, a) per (image,
//       channel) goes to the scratch.
//   in_apply_kernel     the grid and the thread layout of in_stats_kernel; re-reads x (normally from
//       the Infinity Cache), one fma per element, the activation, one rounding, one store.
//
// Nothing is accumulated with atomics and every merge order is a function of (H * W, C) alone, so
// two launches give identical bits and an image's result does not depend on its batch.  The
// statistics are centred at every level: no E[x^2] - E[x]^2.
//
// Paths by shape: C <= 2048 runs one channel group (grid.z == 1), C > 2048 several (the last
// group may be narrower); H * W <= R * 8 is a single chunk (the finalize kernel then merges
// nothing); more than 8 chunks make a finalize slice merge sequentially before the pairwise
// tree.  R is no power of two when C / 8 does not divide 256 (C = 24, 40): the pairwise tree
// skips the partners that do not exist.
//
// Scratch (fp32): partials [N, chunks, C, 2] followed by the statistics [N, C, 2].
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace {

constexpr int IN_THREADS = 256;
constexpr int IN_PT = 8;        // pixels a thread holds in registers
constexpr int IN_FC = 32;       // channels per finalize workgroup
constexpr int IN_FS = IN_THREADS / IN_FC;  // chunk slices per finalize workgroup

struct InParams {
  int N, C, ldy, y_coff, chunks;
  long P;        // pixels per image
  float eps;
};

// thread geometry of a workgroup: R rows of L lanes (channel vectors), first vector cv0.  Every
// group has the geometry of the first, so a chunk is the same pixels in all of them; the last
// group of C > 2048 may have fewer than L vectors (its other lanes idle).
struct InGroup {
  int L, R, cv0, nv;
};

FTM_DEVICE InGroup in_group(int C, int z) {
  const int cv = C / 8;
  InGroup g;
  g.cv0 = z * IN_THREADS;
  g.L = cv < IN_THREADS ? cv : IN_THREADS;
  g.R = IN_THREADS / g.L;
  g.nv = cv - g.cv0 < g.L ? cv - g.cv0 : g.L;
  return g;
}

FTM_DEVICE void unpack8f(const bf16x8 v, float (&f)[8]) {
  const u32x4 u = __builtin_bit_cast(u32x4, v);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __builtin_bit_cast(float, u[i] << 16);
    f[2 * i + 1] = __builtin_bit_cast(float, u[i] & 0xffff0000u);
  }
}

// Chan's parallel update of (count, mean, M2): b merged into a.  na + nb > 0.
FTM_DEVICE void chan_merge(float& na, float& ma, float& qa, float nb, float mb, float qb) {
#pragma clang fp contract(off)
  const float n = na + nb;
  const float d = mb - ma;
  const float f = nb / n;
  ma = ma + d * f;
  qa = qa + qb + d * d * (na * f);
  na = n;
}

__global__ __launch_bounds__(IN_THREADS) void in_stats_kernel(const bf16* __restrict__ x, float* __restrict__ part,
                                                              const InParams q) {
  __shared__ float s_mean[8][IN_THREADS];
  __shared__ float s_m2[8][IN_THREADS];
  __shared__ float s_cnt[IN_THREADS];
  const InGroup g = in_group(q.C, blockIdx.z);
  const int t = threadIdx.x;
  const int n = blockIdx.y, chunk = blockIdx.x;
  const int row = t / g.L, lane = t - row * g.L;
  const bool live = row < g.R && lane < g.nv;
  const long p0 = (long)chunk * (g.R * IN_PT);
  float cnt = 0.f, mean[8], m2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) mean[e] = m2[e] = 0.f;
  if (live) {
    const bf16* xp = x + (size_t)n * q.P * q.C + (size_t)(g.cv0 + lane) * 8;
    float v[IN_PT][8];
#pragma unroll
    for (int k = 0; k < IN_PT; ++k) {
      const long p = p0 + row + (long)k * g.R;
      if (p < q.P) {
        unpack8f(*reinterpret_cast<const bf16x8*>(xp + (size_t)p * q.C), v[k]);
        cnt += 1.f;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[k][e] = 0.f;
      }
    }
    if (cnt > 0.f) {
      const float inv = 1.f / cnt;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < IN_PT; ++k) s += v[k][e];
        mean[e] = s * inv;
      }
#pragma unroll
      for (int k = 0; k < IN_PT; ++k) {
        if (p0 + row + (long)k * g.R < q.P) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float d = v[k][e] - mean[e];
            m2[e] += d * d;
          }
        }
      }
    }
  }
  s_cnt[t] = cnt;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    s_mean[e][t] = mean[e];
    s_m2[e][t] = m2[e];
  }
  __syncthreads();
  // pairwise merge of the rows: row r takes row r + s, s = the powers of two below R, downwards
  int s0 = 1;
  while (s0 < g.R) s0 <<= 1;
  for (int s = s0 >> 1; s > 0; s >>= 1) {
    if (live && row < s && row + s < g.R) {
      const int o = t + s * g.L;
      const float nb = s_cnt[o];
      if (nb > 0.f) {
        float na = s_cnt[t];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float a_n = na, a_m = s_mean[e][t], a_q = s_m2[e][t];
          chan_merge(a_n, a_m, a_q, nb, s_mean[e][o], s_m2[e][o]);
          s_mean[e][t] = a_m;
          s_m2[e][t] = a_q;
        }
        s_cnt[t] = na + nb;
      }
    }
    __syncthreads();
  }
  if (live && row == 0) {
    float* o = part + (((size_t)n * q.chunks + chunk) * q.C + (size_t)(g.cv0 + lane) * 8) * 2;
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      f32x4 w;
      w[0] = s_mean[e][t];
      w[1] = s_m2[e][t];
      w[2] = s_mean[e + 1][t];
      w[3] = s_m2[e + 1][t];
      *reinterpret_cast<f32x4*>(o + e * 2) = w;
    }
  }
}

__global__ __launch_bounds__(IN_THREADS) void in_finalize_kernel(const float* __restrict__ part,
                                                                 const float* __restrict__ gamma,
                                                                 float* __restrict__ stats, const InParams q,
                                                                 const int chunk_px) {
  __shared__ float s_n[IN_THREADS], s_m[IN_THREADS], s_q[IN_THREADS];
  const int t = threadIdx.x;
  const int cl = t % IN_FC, slice = t / IN_FC;
  const int c = blockIdx.x * IN_FC + cl;
  const int n = blockIdx.y;
  float cn = 0.f, cm = 0.f, cq = 0.f;
  if (c < q.C) {
    for (int k = slice; k < q.chunks; k += IN_FS) {
      const long left = q.P - (long)k * chunk_px;
      const float nb = (float)(left < chunk_px ? left : (long)chunk_px);
      const float* p = part + (((size_t)n * q.chunks + k) * q.C + c) * 2;
      if (cn == 0.f) {
        cn = nb;
        cm = p[0];
        cq = p[1];
      } else {
        chan_merge(cn, cm, cq, nb, p[0], p[1]);
      }
    }
  }
  s_n[t] = cn;
  s_m[t] = cm;
  s_q[t] = cq;
  __syncthreads();
  for (int s = IN_FS / 2; s > 0; s >>= 1) {
    if (slice < s) {
      const int o = t + s * IN_FC;
      if (s_n[o] > 0.f) {
        float a_n = s_n[t], a_m = s_m[t], a_q = s_q[t];
        chan_merge(a_n, a_m, a_q, s_n[o], s_m[o], s_q[o]);
        s_n[t] = a_n;
        s_m[t] = a_m;
        s_q[t] = a_q;
      }
    }
    __syncthreads();
  }
  if (slice == 0 && c < q.C) {
    const float var = s_q[t] / (float)q.P;
    float* o = stats + ((size_t)n * q.C + c) * 2;
    o[0] = s_m[t];
    o[1] = gamma[c] / sqrtf(var + q.eps);
  }
}

template <int ACT>
__global__ __launch_bounds__(IN_THREADS) void in_apply_kernel(const bf16* __restrict__ x,
                                                              const float* __restrict__ stats,
                                                              const float* __restrict__ beta, bf16* __restrict__ y,
                                                              const InParams q) {
  const InGroup g = in_group(q.C, blockIdx.z);
  const int t = threadIdx.x;
  const int n = blockIdx.y;
  const int row = t / g.L, lane = t - row * g.L;
  if (row >= g.R || lane >= g.nv) return;
  const int c0 = (g.cv0 + lane) * 8;
  float m[8], a[8], b[8];
  {
    const float* sp = stats + ((size_t)n * q.C + c0) * 2;
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(sp + e * 2);
      m[e] = w[0];
      a[e] = w[1];
      m[e + 1] = w[2];
      a[e + 1] = w[3];
    }
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + c0), b1 = *reinterpret_cast<const f32x4*>(beta + c0 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      b[e] = b0[e];
      b[e + 4] = b1[e];
    }
  }
  const long p0 = (long)blockIdx.x * (g.R * IN_PT);
  const bf16* xp = x + (size_t)n * q.P * q.C + c0;
  bf16* yp = y + (size_t)n * q.P * q.ldy + q.y_coff + c0;
#pragma unroll
  for (int k = 0; k < IN_PT; ++k) {
    const long p = p0 + row + (long)k * g.R;
    if (p < q.P) {
      float v[8];
      unpack8f(*reinterpret_cast<const bf16x8*>(xp + (size_t)p * q.C), v);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(apply_act<ACT>(__builtin_fmaf(v[e] - m[e], a[e], b[e])));
      *reinterpret_cast<bf16x8*>(yp + (size_t)p * q.ldy) = o;
    }
  }
}

// pixels of one chunk: rows x IN_PT
long in_chunk_px(int C) {
  const int cv = C / 8;
  const int L = cv < IN_THREADS ? cv : IN_THREADS;
  return (long)(IN_THREADS / L) * IN_PT;
}

}  // namespace

// fp32 elements of scratch instance_norm_nhwc_bf16 needs for x [N, H, W, C] (ops/kernels.py:
// instance_norm_scratch_numel is the same formula)
static long instance_norm_scratch_floats(int N, int H, int W, int C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) throw std::invalid_argument("instance_norm: bad shape");
  const long P = (long)H * W, cp = in_chunk_px(C);
  const long chunks = (P + cp - 1) / cp;
  return (long)N * chunks * C * 2 + (long)N * C * 2;
}

void instance_norm_nhwc_bf16(uintptr_t x, uintptr_t gamma, uintptr_t beta, uintptr_t y, uintptr_t scratch,
                             long scratch_floats, int N, int H, int W, int C, int ldy, int y_coff, float eps, int act,
                             uintptr_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) throw std::invalid_argument("instance_norm: empty problem");
  if (C % 8 || ldy % 8 || y_coff % 8) throw std::invalid_argument("instance_norm: C, ldy, y_coff must be multiples of 8");
  if (y_coff < 0 || y_coff + C > ldy) throw std::invalid_argument("instance_norm: channel slot exceeds the row");
  if (x % 16 || y % 16 || gamma % 16 || beta % 16 || scratch % 16)
    throw std::invalid_argument("instance_norm: pointers must be 16-byte aligned");
  if (act != ACT_NONE && act != ACT_RELU && act != ACT_RELU6)
    throw std::invalid_argument("instance_norm: activation must be none, relu or relu6");
  if (scratch_floats < instance_norm_scratch_floats(N, H, W, C))
    throw std::invalid_argument("instance_norm: scratch too small");
  const long P = (long)H * W, cp = in_chunk_px(C);
  const long chunks = (P + cp - 1) / cp;
  const int groups = (C / 8 + IN_THREADS - 1) / IN_THREADS;
  if (chunks > 0x7fffffffL || N > 65535 || groups > 65535) throw std::invalid_argument("instance_norm: grid too large");
  const InParams q{N, C, ldy, y_coff, (int)chunks, P, eps};
  auto s = reinterpret_cast<hipStream_t>(stream);
  float* part = reinterpret_cast<float*>(scratch);
  float* stats = part + (size_t)N * chunks * C * 2;
  const dim3 grid((unsigned)chunks, N, groups), block(IN_THREADS);
  hipLaunchKernelGGL(in_stats_kernel, grid, block, 0, s, reinterpret_cast<const bf16*>(x), part, q);
  hipLaunchKernelGGL(in_finalize_kernel, dim3((C + IN_FC - 1) / IN_FC, N), block, 0, s, part,
                     reinterpret_cast<const float*>(gamma), stats, q, (int)cp);
  auto X = reinterpret_cast<const bf16*>(x);
  auto B = reinterpret_cast<const float*>(beta);
  auto Y = reinterpret_cast<bf16*>(y);
  if (act == ACT_RELU) hipLaunchKernelGGL(in_apply_kernel<ACT_RELU>, grid, block, 0, s, X, stats, B, Y, q);
  else if (act == ACT_RELU6) hipLaunchKernelGGL(in_apply_kernel<ACT_RELU6>, grid, block, 0, s, X, stats, B, Y, q);
  else hipLaunchKernelGGL(in_apply_kernel<ACT_NONE>, grid, block, 0, s, X, stats, B, Y, q);
  FTM_CHECK_LAUNCH();
}

void register_instnorm(pybind11::module_& m) {
  m.def("instance_norm_nhwc_bf16", &instance_norm_nhwc_bf16);
}
