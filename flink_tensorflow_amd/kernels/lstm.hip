// LSTM recurrence (TF BlockLSTM, gate order i, ci, f, o): one launch walks all steps of one
// layer.  The input projection xproj = x . w[:I] + b (forget bias folded in) is a GEMM of its
// own; this kernel computes, for t = 0 .. steps-1,
//
//   [i, ci, f, o] = xproj[t] + h_{t-1} . Wh                      (MFMA, fp32 accumulate)
//   i = sig(i + c wci)   f = sig(f + c wcf)   ci = tanh(ci)      (peephole terms optional)
//   c = ci i + c f ;  clip ;  o = sig(o + c wco) ;  h = tanh(c) o
//
// Sequences are independent: a workgroup owns 16 of them (the N of v_mfma_f32_16x16x32_bf16)
// for the whole sequence and never talks to another workgroup.  The weights are the A operand
// with gate units on M: a wave's four accumulators of a 16-unit group hold i, ci, f, o of
// the same (unit, sequence) pairs (C/D map: column = lane & 15 = sequence, row =
// 4 (lane >> 4) + reg = unit), so the pointwise part needs no exchange between lanes.
//
//   xproj   bf16, element strides (xs_t, xs_b), last axis 4H contiguous
//   wpk     bf16 [H/16][4 gates][KS][64 lanes][8]: the A fragments as each lane loads them
//           (lstm_pack_weights); KS = ceil(H / 32), rows j >= H are zero
//   h0      bf16 [B, H];  c0 fp32 or bf16 [B, H];  wci / wcf / wco fp32 [H] or null
//   h_out   bf16, strides (hs_t, hs_b): [T, .., H]; last_only: [B, ..H] = h_{steps-1}
//   cs_out  bf16 (optional), strides (cs_t, cs_b);  c_last fp32 [B, H] (optional)
//
// c stays in fp32 registers for the whole sequence; h_t is rounded to bf16 once, stored, and
// written to a double-buffered LDS tile [16][KS * 32 + 8] that is the B operand of step t + 1
// (columns >= H stay zero: with H % 32 == 16 the last K step's upper half multiplies zero
// weights by zero).  One workgroup barrier per step (lds_barrier).  Rows of a partial last tile
// take zero initial state (predicated loads), read the projection rows of the last real
// sequence (in bounds, see load_x) and are never stored.
//
//   RES   H <= 128: H / 16 waves, wave v owns units [16v, 16v + 16); its 4 x KS weight
//         fragments (64 VGPRs at H = 128) are loaded once and stay in registers.
//   !RES  128 < H <= 512: 8 waves, wave v owns groups v, v + 8, ... (NG of them at most);
//         the fragments are re-read (L2) every step.
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace {

struct LstmParams {
  const bf16* xproj;
  const bf16* wpk;
  const bf16* h0;
  const void* c0;
  const float* wci;
  const float* wcf;
  const float* wco;
  bf16* h_out;
  bf16* cs_out;
  float* c_last;
  long xs_t, xs_b, hs_t, hs_b, cs_t, cs_b;
  int T, B, H, steps, last_only, c0_bf16;
  float clip;
};

FTM_DEVICE f32x4 widen4(const bf16x4 v) { return f32x4{bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3])}; }
FTM_DEVICE bf16x4 narrow4(const f32x4 v) { return bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])}; }

// The per-step barrier: the h tile is LDS only, so the waves wait for their LDS operations and
// meet; global loads and stores (the prefetched projection rows, h_out) stay in flight across it,
// which the fence of __syncthreads() would drain every step.
FTM_DEVICE void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

template <int KSR, int NG, bool RES>
__global__ __launch_bounds__(512) void lstm_seq_kernel(const LstmParams p) {
  extern __shared__ __attribute__((aligned(16))) bf16 lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int col = lane & 15, quad = lane >> 4;
  const int H = p.H, ngroups = H >> 4;
  const int KS = RES ? KSR : (H + 31) >> 5;
  const int pitch = KS * 32 + 8;  // elements; +16 B keeps the 16 rows of a ds_read_b128 on distinct banks
  const long b = (long)blockIdx.x * 16 + col;
  const bool valid = b < p.B;
  const bool peep = p.wci != nullptr;

  // both h tiles start as zeros: the K padding and the rows of a partial tile stay zero
  for (int i = threadIdx.x; i < 2 * 16 * pitch / 8; i += blockDim.x) reinterpret_cast<u32x4*>(lds)[i] = u32x4{0, 0, 0, 0};
  __syncthreads();

  bool own[NG];
  int u0[NG];  // first of this lane's four units in group n
  f32x4 c[NG], pw[NG][3];
  bf16x4 hlast[NG], xp[NG][4];
#pragma unroll
  for (int n = 0; n < NG; ++n) {
    const int g = wave + n * nwaves;
    own[n] = g < ngroups;  // wave-uniform
    u0[n] = g * 16 + quad * 4;
    c[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    hlast[n] = bf16x4{};
#pragma unroll
    for (int k = 0; k < 3; ++k) pw[n][k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!own[n]) continue;
    if (RES && peep) {  // the streamed form re-reads them per step: its registers go to the accumulators
      pw[n][0] = *reinterpret_cast<const f32x4*>(p.wci + u0[n]);
      pw[n][1] = *reinterpret_cast<const f32x4*>(p.wcf + u0[n]);
      pw[n][2] = *reinterpret_cast<const f32x4*>(p.wco + u0[n]);
    }
    if (valid) {
      const long off = b * H + u0[n];
      if (p.c0_bf16) c[n] = widen4(*reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16*>(p.c0) + off));
      else c[n] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.c0) + off);
      *reinterpret_cast<bf16x4*>(lds + col * pitch + u0[n]) = *reinterpret_cast<const bf16x4*>(p.h0 + off);
    }
  }

  // resident form: the wave's 4 x KS weight fragments, loaded once
  bf16x8 wreg[RES ? 4 : 1][RES ? KSR : 1];
  if constexpr (RES) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int ks = 0; ks < KSR; ++ks)
        wreg[g][ks] = *reinterpret_cast<const bf16x8*>(p.wpk + (((long)wave * 4 + g) * KSR + ks) * 512 + lane * 8);
  }

  // The projection rows are loaded without a branch (the compiler waits for every load in flight
  // at the first use behind a branch that may have skipped one): the dead rows of a partial tile
  // read the last real row again, in bounds, and nothing of theirs is ever stored.
  const long bx = valid ? b : (long)p.B - 1;
  auto load_x = [&](int n, int t) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      xp[n][g] = bf16x4{};
      if (RES || own[n]) xp[n][g] = *reinterpret_cast<const bf16x4*>(p.xproj + t * p.xs_t + bx * p.xs_b + g * H + u0[n]);
    }
  };
  if (p.steps > 0) {
#pragma unroll
    for (int n = 0; n < NG; ++n) load_x(n, 0);
  }
  __syncthreads();

  for (int t = 0; t < p.steps; ++t) {
    const bf16* hcur = lds + (t & 1) * 16 * pitch + col * pitch + quad * 8;  // this lane's B fragments
    bf16* hnext = lds + ((t & 1) ^ 1) * 16 * pitch + col * pitch;
    // a wave finishes one 16-unit group (MFMAs, then the pointwise part) before the next
#pragma unroll
    for (int n = 0; n < NG; ++n) {
      if (!RES && !own[n]) continue;  // the resident form has one wave per group
      f32x4 acc[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = widen4(xp[n][g]);
      // the next step's projection rows: the address does not depend on the recurrence (the last
      // step re-reads its own rows, so that no branch stands between the load and its wait)
      load_x(n, t + 1 < p.steps ? t + 1 : t);

      if constexpr (RES) {
#pragma unroll
        for (int ks = 0; ks < KSR; ++ks) {
          const bf16x8 hb = *reinterpret_cast<const bf16x8*>(hcur + ks * 32);
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wreg[g][ks], hb, acc[g], 0, 0, 0);
        }
      } else {
        const bf16* wg = p.wpk + (long)(wave + n * nwaves) * 4 * KS * 512 + lane * 8;
#pragma unroll 2
        for (int ks = 0; ks < KS; ++ks) {
          const bf16x8 hb = *reinterpret_cast<const bf16x8*>(hcur + ks * 32);
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const bf16x8 wa = *reinterpret_cast<const bf16x8*>(wg + ((long)g * KS + ks) * 512);
            acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, hb, acc[g], 0, 0, 0);
          }
        }
        if (peep) {
          pw[n][0] = *reinterpret_cast<const f32x4*>(p.wci + u0[n]);
          pw[n][1] = *reinterpret_cast<const f32x4*>(p.wcf + u0[n]);
          pw[n][2] = *reinterpret_cast<const f32x4*>(p.wco + u0[n]);
        }
      }

      f32x4 hv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float cp = c[n][r];
        const float gi = apply_act<ACT_SIGMOID>(acc[0][r] + cp * pw[n][0][r]);
        const float gc = apply_act<ACT_TANH>(acc[1][r]);
        const float gf = apply_act<ACT_SIGMOID>(acc[2][r] + cp * pw[n][1][r]);
        float cn = gc * gi + cp * gf;
        if (p.clip > 0.f) cn = fminf(fmaxf(cn, -p.clip), p.clip);
        const float go = apply_act<ACT_SIGMOID>(acc[3][r] + cn * pw[n][2][r]);
        hv[r] = apply_act<ACT_TANH>(cn) * go;
        c[n][r] = cn;
      }
      const bf16x4 hb4 = narrow4(hv);
      hlast[n] = hb4;
      *reinterpret_cast<bf16x4*>(hnext + u0[n]) = valid ? hb4 : bf16x4{};
      if (valid) {
        if (!p.last_only) *reinterpret_cast<bf16x4*>(p.h_out + t * p.hs_t + b * p.hs_b + u0[n]) = hb4;
        if (p.cs_out) *reinterpret_cast<bf16x4*>(p.cs_out + t * p.cs_t + b * p.cs_b + u0[n]) = narrow4(c[n]);
      }
    }
    lds_barrier();
  }

#pragma unroll
  for (int n = 0; n < NG; ++n) {
    if (!own[n] || !valid) continue;
    for (int t = p.steps; t < p.T; ++t) {  // steps past the sequence length are zero
      if (!p.last_only) *reinterpret_cast<bf16x4*>(p.h_out + t * p.hs_t + b * p.hs_b + u0[n]) = bf16x4{};
      if (p.cs_out) *reinterpret_cast<bf16x4*>(p.cs_out + t * p.cs_t + b * p.cs_b + u0[n]) = bf16x4{};
    }
    if (p.last_only) *reinterpret_cast<bf16x4*>(p.h_out + b * p.hs_b + u0[n]) = hlast[n];
    if (p.c_last) *reinterpret_cast<f32x4*>(p.c_last + b * H + u0[n]) = c[n];
  }
}

template <int KSR, int NG, bool RES>
void launch(const LstmParams& p, hipStream_t s) {
  const int KS = (p.H + 31) / 32;
  const dim3 grid((p.B + 15) / 16), block(RES ? p.H / 16 * 64 : 512);
  const size_t shmem = (size_t)2 * 16 * (KS * 32 + 8) * sizeof(bf16);
  hipLaunchKernelGGL((lstm_seq_kernel<KSR, NG, RES>), grid, block, shmem, s, p);
}

}  // namespace

// Strides are in elements.  hs_t is ignored with last_only; cs_out and c_last may be 0.
void lstm_seq_bf16(uintptr_t xproj, uintptr_t wpk, uintptr_t h0, uintptr_t c0, int c0_bf16, uintptr_t wci, uintptr_t wcf,
                   uintptr_t wco, uintptr_t h_out, uintptr_t cs_out, uintptr_t c_last, int T, int B, int H, int steps,
                   long xs_t, long xs_b, long hs_t, long hs_b, long cs_t, long cs_b, int last_only, float clip,
                   uintptr_t stream) {
  if (T < 1 || B < 1) throw std::invalid_argument("lstm: empty problem");
  if (H < 16 || H > 512 || H % 16) throw std::invalid_argument("lstm: H must be a multiple of 16 in 16..512");
  if (steps < 0 || steps > T) throw std::invalid_argument("lstm: steps must be in 0..T");
  if (!xproj || !wpk || !h0 || !c0 || !h_out) throw std::invalid_argument("lstm: null operand");
  if (xproj % 16 || wpk % 16 || h0 % 16 || c0 % 16 || h_out % 16 || cs_out % 16 || c_last % 16 || wci % 16 || wcf % 16 ||
      wco % 16)
    throw std::invalid_argument("lstm: pointers must be 16-byte aligned");
  if (xs_t % 8 || xs_b % 8 || hs_t % 8 || hs_b % 8 || cs_t % 8 || cs_b % 8)
    throw std::invalid_argument("lstm: strides must be multiples of 8 elements");
  if (xs_b < 4L * H || hs_b < H || (cs_out && cs_b < H)) throw std::invalid_argument("lstm: row stride shorter than the row");
  if ((wci != 0) != (wcf != 0) || (wci != 0) != (wco != 0))
    throw std::invalid_argument("lstm: the three peephole vectors come together");
  LstmParams p;
  p.xproj = reinterpret_cast<const bf16*>(xproj);
  p.wpk = reinterpret_cast<const bf16*>(wpk);
  p.h0 = reinterpret_cast<const bf16*>(h0);
  p.c0 = reinterpret_cast<const void*>(c0);
  p.wci = reinterpret_cast<const float*>(wci);
  p.wcf = reinterpret_cast<const float*>(wcf);
  p.wco = reinterpret_cast<const float*>(wco);
  p.h_out = reinterpret_cast<bf16*>(h_out);
  p.cs_out = reinterpret_cast<bf16*>(cs_out);
  p.c_last = reinterpret_cast<float*>(c_last);
  p.xs_t = xs_t, p.xs_b = xs_b, p.hs_t = hs_t, p.hs_b = hs_b, p.cs_t = cs_t, p.cs_b = cs_b;
  p.T = T, p.B = B, p.H = H, p.steps = steps, p.last_only = last_only, p.c0_bf16 = c0_bf16;
  p.clip = clip;
  auto s = reinterpret_cast<hipStream_t>(stream);
  if (H <= 128) {
    switch ((H + 31) / 32) {
      case 1: launch<1, 1, true>(p, s); break;
      case 2: launch<2, 1, true>(p, s); break;
      case 3: launch<3, 1, true>(p, s); break;
      default: launch<4, 1, true>(p, s); break;
    }
  } else {
    const int ng = (H / 16 + 7) / 8;  // groups per wave of the 8-wave streamed form
    if (ng == 2) launch<0, 2, false>(p, s);
    else if (ng == 3) launch<0, 3, false>(p, s);
    else launch<0, 4, false>(p, s);
  }
  FTM_CHECK_LAUNCH();
}

void register_lstm(pybind11::module_& m) { m.def("lstm_seq_bf16", &lstm_seq_bf16); }
