"""The fp8 inference kernels of ``kernels/fp8.hip``, bit for bit.

The data are integers that are exact in e4m3 (or in bf16 for the bf16 inputs), the scales are
powers of two that differ per channel and the biases are multiples of 1/4.  Every product and
every partial sum is then exact in fp32 in any order, ``acc * scale + bias`` is exact whether
or not the compiler fuses it, and the only inexact steps are the kernels' roundings.  The
float64 mirrors below round where the ``.hip`` file rounds:

``igemm_fp8_kernel`` / ``conv_lite_fp8_body`` (non-multi)
    ``v = act(acc * scale[c] + bias[c])``; fp8 output ``e4m3_rne(clamp(v * out_q, +-448))``
    (one rounding), bf16 output ``bf16_rne(v)``.  A bf16 input is quantised on load,
    ``e4m3_rne(clamp(x * in_q))``, before the sum (``quant16``).
``conv_lite_fp8_body`` multi epilogue
    ``v = max(acc * scale[c] + bias[c], lo[c])`` -> ``bf16_rne`` into the LDS tile -> per segment
    either stored as bf16 or ``e4m3_rne(clamp(float(bf16) * q))``: two roundings, here only.
``pool_fp8_kernel<MAX>`` / ``maxpool3_fp8_kernel``
    the max of the decoded bytes (padding never enters), ``fp32(max * rq)``, clamp, e4m3.
``pool_fp8_kernel<avg>``
    ``sc = fp32(rq / fp32(cnt))``, ``fp32(sum * sc)``, clamp, e4m3 (cnt = in-bounds pixels).
``avgpool_epi_kernel`` / ``avgpool3_epi_kernel``
    ``inv = fp32(1 / fp32(cnt))``, ``v = act(fp32(fma(sum, inv, bias)))``, then
    ``e4m3_rne(clamp(fp32(v * out_q)))`` or ``bf16_rne(v)``.
``gap_fp8_kernel``
    ``inv = fp32(s / fp32(HW))``, ``bf16_rne(fp32(sum * inv))``.
``quantize_kernel`` / ``dequantize_kernel``
    ``e4m3_rne(clamp(fp32(x * q)))`` and ``bf16_rne(fp32(e4m3 * s))``.

The GPU tests write into buffers wider (and longer) than the slot, pre-filled with a non-zero
sentinel, and compare with equality: fp8 bytes after mapping both zero encodings (0x00, 0x80)
to one value, bf16 with ``torch.equal``.  A mismatch names M tile, N tile, pixel and channel.

The non-GPU tests check the mirrors alone: that torch's e4m3 cast is round-to-nearest-even,
that each mirror equals the ``Q.*`` host path of ``ops/fp8.py`` where both are defined, that
the data make saturation, subnormals, ReLU and quantise-on-load observable, and that each
deliberately wrong variant (``FAULTS``) changes the output of every case it applies to."""
import collections
import functools
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from flink_tensorflow_amd.ops import fp8 as Q

BF, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
E4M3 = torch.float8_e4m3fn
EXACT = 2 ** 24         # integers below this are exact in fp32
SENT8 = 0x5A            # fp8 sentinel byte (e4m3 208.0)
SENT16 = -77.0          # bf16 sentinel, exact in bf16
GUARD = 8               # sentinel pixel rows behind every output
BK = 128                # K bytes per K-tile of every fp8 GEMM tile
FAULTS = ("drop_chunk", "stale_stage", "stale_rows", "tap_swap", "no_dilation", "scale_shift4", "round_via_bf16",
          "round_direct", "seg_shift16", "pad_counted", "pad_wins_max")


# ------------------------------------------------------------------------ rounding helpers
def _f32(v):
    """float64 -> fp32 (RNE) -> float64: one fp32 rounding of an exactly known value."""
    return v.float().double()


def _e4m3(v):
    """float64 -> e4m3 bytes as ``pack4`` does: fp32, clamp to +-448, round to nearest even."""
    return v.float().clamp(-448.0, 448.0).to(E4M3).view(U8)


def _dec(b):
    return b.contiguous().view(E4M3).double()


def _bf(v):
    """bf16 RNE of values that are exact in fp32 (float64 -> fp32 then changes nothing)."""
    return v.float().to(BF).double()


def _canon(b):
    """fp8 bytes with both zero encodings mapped to 0x00."""
    return torch.where(b == 0x80, torch.zeros_like(b), b)


def _is_sub(b):
    m = b & 0x7F
    return (m >= 1) & (m <= 7)


def _is_neg(b):
    return ((b & 0x80) != 0) & ((b & 0x7F) != 0)


class _Trace:
    """What a mirror saw: an upper bound of every intermediate magnitude (partial sums included),
    in units of the data's least significant bit, and the shares the observability test reads."""

    def __init__(self):
        self.peak, self.stats = 0.0, {}

    def see(self, bound, unit=1.0):
        self.peak = max(self.peak, float(bound.max()) / unit)

    def exact(self, v, what):
        assert torch.equal(_f32(v), v), f"{what} is not exact in fp32"
        return v

    def note(self, **kw):
        self.stats.update(kw)

    def close(self):
        assert self.peak < EXACT, f"intermediate magnitude {self.peak} is not exact in fp32"
        return self


# -------------------------------------------------------------------------- conv / GEMM mirror
Geom = collections.namedtuple("Geom", "N H W Cin Cout k stride pad dil", defaults=((1, 1), (0, 0, 0, 0), (1, 1)))


def _out_hw(g):
    (kh, kw), (sh, sw), (pt, pb, pl, pr), (dh, dw) = g.k, g.stride, g.pad, g.dil
    return (g.H + pt + pb - ((kh - 1) * dh + 1)) // sh + 1, (g.W + pl + pr - ((kw - 1) * dw + 1)) // sw + 1


def _pixels(g):
    ho, wo = _out_hw(g)
    return g.N * ho * wo


def _im2col(x, g, fault=None):
    """[M, KH * KW * Cin] in the kernels' K order (kh, kw, ci); zeros in the padding."""
    (KH, KW), (sh, sw), (pt, _, pl, _), (dh, dw) = g.k, g.stride, g.pad, g.dil
    Ho, Wo = _out_hw(g)
    if fault == "no_dilation":
        dh = dw = 1
    oh, ow = torch.arange(Ho) * sh - pt, torch.arange(Wo) * sw - pl
    cols = []
    for kh in range(KH):
        for kw in range(KW):
            a, b = (kw, kh) if fault == "tap_swap" else (kh, kw)
            hi, wi = oh + a * dh, ow + b * dw
            ok = ((hi >= 0) & (hi < g.H))[:, None] & ((wi >= 0) & (wi < g.W))[None, :]
            t = x[:, hi.clamp(0, g.H - 1)][:, :, wi.clamp(0, g.W - 1)]
            cols.append(t * ok[None, :, :, None])
    return torch.cat(cols, -1).reshape(g.N * Ho * Wo, KH * KW * g.Cin)


def _acc(tr, x, w, g, bm, fault, unit):
    """The exact accumulation ``im2col(x) . w^T``.  Faults: one 16-byte chunk of the last K-tile
    zero; K-tile kt computed from the activations of K-tile kt - 1; the rows of the last,
    partial M tile taken from the tile before it; (kh, kw) exchanged; dilation ignored."""
    A = _im2col(x, g, fault)
    M, K = A.shape
    nk = -(-K // BK)
    if fault == "drop_chunk":
        A = A.clone()
        A[:, (nk - 1) * BK:(nk - 1) * BK + 16] = 0
    if fault == "stale_stage":
        B = A.clone()
        for kt in range(1, nk):
            wd = min(BK, K - kt * BK)
            B[:, kt * BK:kt * BK + wd] = A[:, (kt - 1) * BK:(kt - 1) * BK + wd]
        A = B
    if fault == "stale_rows":
        m0 = (M - 1) // bm * bm
        B = A.clone()
        B[m0:] = A[m0 - bm:M - bm]
        A = B
    w2 = w.reshape(g.Cout, K)
    tr.see(A.abs() @ w2.abs().t(), unit)
    return A @ w2.t()


def ref_conv(x, w, scale, bias, g, act, out_q, in_q=None, bm=128, fault=None):
    """``igemm_fp8_kernel`` and the non-multi ``conv_lite_fp8_body``.  x [N, H, W, Cin] (decoded
    e4m3 values, or bf16 values with ``in_q``), w [Cout, KH, KW, Cin], ``out_q`` None = bf16
    output.  Returns (e4m3 bytes or bf16 values as float64 [M, Cout], trace)."""
    tr, unit = _Trace(), 1.0
    if in_q is not None:
        xs = x * in_q
        xq = _dec(_e4m3(xs))
        tr.note(in_changed=(xq != xs).double().mean().item(), in_saturated=(xs.abs() > 448).double().mean().item())
        x, unit = xq, min(1.0, in_q)   # integers times a power of two: the quantised values keep that lsb
    acc = _acc(tr, x, w, g, bm, fault, unit)
    if fault == "scale_shift4":
        scale, bias = scale.roll(-4), bias.roll(-4)
    v = tr.exact(acc * scale + bias, "acc * scale + bias")
    if act == "relu":
        v = torch.relu(v)
    if out_q is None:
        return _bf(v), tr.close()
    t = tr.exact(v * out_q, "v * out_q")
    if fault == "round_via_bf16":
        t = _bf(v) * out_q
    return _e4m3(t), tr.close()


def ref_multi(x, w, scale, bias, lo, segs, g, fault=None):
    """The multi-destination epilogue: ``bf16(max(acc * s + b, lo))`` staged, then per segment
    ``(c0, c1, q)`` kept as bf16 (q None) or ``e4m3(clamp(bf16 * q))``.  Faults: the fp8
    segments skip the bf16 staging; the boundary between segments 0 and 1 moved up by 16
    channels (those channels take segment 0's scale).  Returns ([per-segment output], trace)."""
    tr = _Trace()
    acc = _acc(tr, x, w, g, 128, fault, 1.0)
    if fault == "scale_shift4":
        scale, bias = scale.roll(-4), bias.roll(-4)
    v = tr.exact(torch.maximum(acc * scale + bias, lo), "max(acc * scale + bias, lo)")
    staged = _bf(v)
    qv = torch.ones(g.Cout, dtype=F64)
    for i, (c0, c1, q) in enumerate(segs):
        if fault == "seg_shift16" and i == 1:
            c0 += 16
        qv[c0:c1] = 1.0 if q is None else q
    bytes_ = _e4m3(tr.exact((v if fault == "round_direct" else staged) * qv, "bf16 * q"))
    return [staged[:, c0:c1] if q is None else bytes_[:, c0:c1] for c0, c1, q in segs], tr.close()


# --------------------------------------------------------------------------------- conv data
# Activations: integers in [0, 8] (exact in e4m3).  bf16 inputs: integers in [0, 24] with 1 % at
# 1024, quantised on load with in_q = 1/2: halves above 8 are no e4m3 values (the quantisation
# changes them, ties to even) and 512 saturates at 448.  Weights: integers in [-4, 4].
# scale[c] = 2^(T[c % 7] - log2(sigma) - log2(out_q)) with sigma the standard deviation of the
# K-deep sum, so that channel c's fp8 output has standard deviation 2^T[c % 7]: 2^-7 lands in the
# e4m3 subnormals (below 2^-6, steps of 2^-9), 2^8 and 2^10 saturate at +-448.  The period of 7
# makes scale[c + 4] and scale[c + 16] differ from scale[c] everywhere.  Biases are multiples of
# 1/4 in [-8, 8], zero on the two smallest channel classes (a bias would lift them out of the
# subnormals).  Worst case |x| . |w| = 8320 * 8 * 4 < 2^19; each mirror asserts its own bound.
TARGETS = (-7, -4, -1, 2, 5, 8, 10)
IN_Q = 0.5
OUT_Q = 0.125


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _chan_scales(gen, x_eff, w, cout, k, q):
    sigma = math.sqrt(k * float((x_eff ** 2).mean()) * float((w ** 2).mean()))
    base = -round(math.log2(sigma)) - round(math.log2(q))
    t = torch.tensor([TARGETS[c % 7] for c in range(cout)])
    scale = torch.pow(torch.tensor(2.0, dtype=F64), (t + base).double())
    bias = _ints(gen, (cout,), -32, 32) / 4 * (t > -4)
    return scale, bias


def conv_data(g, in_bf16, q=OUT_Q):
    gen = _gen("conv", tuple(g), in_bf16)
    shape = (g.N, g.H, g.W, g.Cin)
    if in_bf16:
        x = _ints(gen, shape, 0, 24)
        x = torch.where(torch.rand(shape, generator=gen) < 0.01, torch.full_like(x, 1024.0), x)
        x_eff = _dec(_e4m3(x * IN_Q))
    else:
        x = x_eff = _ints(gen, shape, 0, 8)
    w = _ints(gen, (g.Cout, *g.k, g.Cin), -4, 4)
    scale, bias = _chan_scales(gen, x_eff, w, g.Cout, g.k[0] * g.k[1] * g.Cin, q)
    return dict(x=x, w=w, scale=scale, bias=bias)


def _gemm(M, K, N):
    return Geom(M, 1, 1, K, N, (1, 1))


# igemm_fp8_kernel.  M = 286 is a partial last M tile at both tile heights (128, 256), Cout 144
# a tail at both tile widths (128, 64), K = 432 four K-tiles with the last 48 wide.
# name -> (geometry, act, channel offset, buffer width)
IGEMM = {
    "3x3-c48-144": (Geom(2, 11, 13, 48, 144, (3, 3), (1, 1), (1, 1, 1, 1)), "relu", 32, 208),
    "3x3-s2-c16-32": (Geom(2, 11, 13, 16, 32, (3, 3), (2, 2), (0, 1, 0, 1)), None, 16, 64),
    "3x3-dil2-c32-64": (Geom(2, 11, 13, 32, 64, (3, 3), (1, 1), (2, 2, 2, 2), (2, 2)), "relu", 0, 80),
    "1x7-c48-96": (Geom(2, 11, 13, 48, 96, (1, 7), (1, 1), (0, 0, 3, 3)), None, 16, 128),
    "pw-c160-80": (Geom(3, 7, 7, 160, 80, (1, 1)), "relu", 48, 128),
}
GEMMS = {"gemm-5x64x64": (_gemm(5, 64, 64), None), "gemm-300x272x96": (_gemm(300, 272, 96), "relu")}
TILES = {0: (128, 128), 1: (256, 64), 2: (128, 64)}


def _lite_bn(cout):
    """``lite_fp8_bn`` (checked against the library by tests/test_fp8.py)."""
    return min((192, 160, 128, 96, 64), key=lambda bn: (-(-cout // bn) * (128 + bn), -bn))


# conv_lite_fp8 (cfg 11).  name -> (geometry, act, channel offset, buffer width)
LITE = {
    "bn64-1x1-k64": (Geom(2, 11, 13, 64, 64, (1, 1)), "relu", 0, 80),                       # one stage, K 64
    "bn64-3x3-c32": (Geom(2, 11, 13, 32, 64, (3, 3), (1, 1), (1, 1, 1, 1)), None, 16, 96),    # 3 K-tiles
    "bn96-1x7-c48": (Geom(2, 11, 13, 48, 96, (1, 7), (1, 1), (0, 0, 3, 3)), "relu", 32, 128),
    "bn96-tail80-7x1-c80": (Geom(1, 7, 7, 80, 80, (7, 1), (1, 1), (3, 3, 0, 0)), None, 0, 96),   # M 49
    "bn128-1x1-k128": (Geom(3, 7, 7, 128, 128, (1, 1)), "relu", 0, 144),                     # one stage, K 128
    "bn160x2-3x3-c16": (Geom(2, 11, 13, 16, 320, (3, 3), (1, 1), (1, 1, 1, 1)), None, 16, 352),  # 8 taps per K-tile
    "bn160x3-tail-dil2-c192": (Geom(2, 11, 13, 192, 448, (3, 3), (1, 1), (2, 2, 2, 2), (2, 2)), "relu", 0, 464),
    "bn192-s2-c288": (Geom(2, 11, 13, 288, 384, (3, 3), (2, 2), (0, 1, 0, 1)), None, 32, 448),
    "bn64-c1040-74ktiles": (Geom(1, 7, 7, 1040, 64, (3, 3), (1, 1), (1, 1, 1, 1)), "relu", 16, 96),
}
LITE_BN = {"bn64-1x1-k64": 64, "bn64-3x3-c32": 64, "bn96-1x7-c48": 96, "bn96-tail80-7x1-c80": 96,
           "bn128-1x1-k128": 128, "bn160x2-3x3-c16": 160, "bn160x3-tail-dil2-c192": 160, "bn192-s2-c288": 192,
           "bn64-c1040-74ktiles": 64}


@functools.lru_cache(maxsize=None)
def conv_case(family, name, in_bf16, out_fp8):
    g, act = {"igemm": IGEMM, "gemm": GEMMS, "lite": LITE}[family][name][:2]
    d = conv_data(g, in_bf16)
    y, tr = ref_conv(**d, g=g, act=act, out_q=OUT_Q if out_fp8 else None, in_q=IN_Q if in_bf16 else None)
    return d, y, tr


# conv2d_nhwc_fp8_multi, 1x1, M = 286.  Segments (channels, q or None for bf16, offset, width).
# Four fp8 segments of different power-of-two scales and a bf16 one.  "inner": every boundary
# strictly inside the one 160-wide channel tile; "edge": total Cout 320 on the 160 tile, the first
# boundary on the tile edge.  The last segment has no activation (lo = -inf).
MULTI_LAYOUTS = {
    "inner": [(48, 0.25, 32, 128), (32, 2.0, 0, 32), (16, 0.5, 16, 48), (32, None, 0, 32), (32, 1.0, 0, 32)],
    "edge": [(160, 0.5, 0, 160), (64, 4.0, 16, 128), (32, 0.25, 0, 32), (48, None, 16, 80), (16, 1.0, 0, 16)],
}


def _multi_geom(C, layout):
    return Geom(2, 13, 11, C, sum(s[0] for s in MULTI_LAYOUTS[layout]), (1, 1))


def _multi_segs(layout):
    segs, c = [], 0
    for n, q, _, _ in MULTI_LAYOUTS[layout]:
        segs.append((c, c + n, q))
        c += n
    return segs


@functools.lru_cache(maxsize=None)
def multi_case(C, layout):
    g = _multi_geom(C, layout)
    d = conv_data(g, False, q=1.0)
    segs = _multi_segs(layout)
    lo = torch.zeros(g.Cout, dtype=F64)
    lo[segs[-1][0]:] = float("-inf")
    d["lo"] = lo
    ys, tr = ref_multi(**d, segs=segs, g=g)
    return d, segs, ys, tr


# ------------------------------------------------------------------------------ pool mirrors
def _windows(x, k, s, pad, fill):
    """[N, Ho, Wo, C, kh * kw] windows of NHWC ``x`` padded with ``fill``, and the in-bounds count."""
    pt, pb, pl, pr = pad
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb), value=fill)
    win = xp.unfold(2, k[0], s[0]).unfold(3, k[1], s[1]).flatten(-2).permute(0, 2, 3, 1, 4)
    ones = F.pad(torch.ones(1, 1, x.shape[1], x.shape[2], dtype=F64), (pl, pr, pt, pb))
    cnt = ones.unfold(2, k[0], s[0]).unfold(3, k[1], s[1]).flatten(-2).sum(-1)[0, 0]
    return win, cnt[None, :, :, None]


def _r32(v):
    return torch.tensor(v, dtype=F32)


def ref_pool(x, k, s, pad, mode, rq, fault=None):
    """``pool_fp8_kernel`` and ``maxpool3_fp8_kernel``.  x: decoded e4m3 values [N, H, W, C]."""
    tr = _Trace()
    if mode == "max":
        win, _ = _windows(x, k, s, pad, 0.0 if fault == "pad_wins_max" else float("-inf"))
        return _e4m3(_f32(win.amax(-1) * _r32(rq).double())), tr.close()
    win, cnt = _windows(x, k, s, pad, 0.0)
    tr.see(win.abs().sum(-1), 1.0)
    if fault == "pad_counted":
        cnt = torch.full_like(cnt, k[0] * k[1])
    sc = (_r32(rq) / cnt.float()).double()          # fp32 division, correctly rounded
    return _e4m3(_f32(win.sum(-1) * sc)), tr.close()  # |sum| < 2^12, sc 24 bits: exact in float64


def ref_avgpool_epi(x, bias, k, s, pad, act, out_q, fault=None):
    """``avgpool_epi_kernel`` / ``avgpool3_epi_kernel``.  x: bf16-exact integers [N, H, W, C]."""
    tr = _Trace()
    win, cnt = _windows(x, k, s, pad, 0.0)
    tr.see(win.abs().sum(-1), 1.0)
    if fault == "pad_counted":
        cnt = torch.full_like(cnt, k[0] * k[1])
    inv = (1.0 / cnt.float()).double()
    v = _f32(win.sum(-1) * inv + bias)   # fma: the product (< 2^19, multiples of 2^-28) plus a multiple of 1/4
    if act == "relu":                    # fits float64, so this is one fp32 rounding
        v = torch.relu(v)
    if out_q is None:
        return _bf(v), tr.close()
    return _e4m3(_f32(v * out_q)), tr.close()


def ref_gap(x, s):
    """``gap_fp8_kernel``.  x: decoded e4m3 integers [N, HW, C]."""
    tr = _Trace()
    tr.see(x.abs().sum(1), 1.0)
    inv = (_r32(s) / _r32(float(x.shape[1]))).double()
    return _bf(_f32(x.sum(1) * inv)), tr.close()


# -------------------------------------------------------------------------------- pool data
# m * 2^j with m an integer in [lo, 8] and j in [0, 5]: integers of at most four significant
# bits, |v| <= 256, exact in e4m3; a 9-pixel sum stays below 2^12.
def pool_data(key, shape, lo=-8):
    gen = _gen("pool", key, shape)
    v = _ints(gen, shape, lo, 8) * torch.pow(torch.tensor(2.0, dtype=F64), _ints(gen, shape, 0, 5))
    assert torch.equal(_dec(_e4m3(v)), v)
    return v


# pool_fp8_kernel: (shape, kernel, stride, pad, rq, offset, width).  Stride-1 rows take two outputs
# per thread (odd Wo: the second one of the last pair is unused).  3x3 / stride 2 max goes to
# maxpool3_fp8_kernel, so the generic max kernel's strided case is 2x2.
POOL = {
    "3x3-s1-same-c48": ((2, 9, 9, 48), (3, 3), (1, 1), (1, 1, 1, 1), 0.5, 16, 80),
    "3x3-s1-valid-c16": ((2, 9, 9, 16), (3, 3), (1, 1), (0, 0, 0, 0), 2.0, 0, 32),
    "2x2-s2-asym-c48": ((2, 9, 9, 48), (2, 2), (2, 2), (0, 1, 0, 1), 2.0 ** -10, 32, 96),
    "2x2-s1-asym-c16": ((2, 6, 7, 16), (2, 2), (1, 1), (0, 1, 0, 1), 1.0, 16, 48),
}
POOL_AVG_ONLY = {
    "3x3-s2-same-c48": ((2, 9, 9, 48), (3, 3), (2, 2), (1, 1, 1, 1), 8.0, 0, 64),
    "3x3-s1-same-c16-rq0.7": ((2, 9, 9, 16), (3, 3), (1, 1), (1, 1, 1, 1), 0.7, 16, 48),
    "3x3-s2-asym-c16-rq0.7": ((1, 8, 10, 16), (3, 3), (2, 2), (0, 1, 0, 1), 0.7, 0, 32),
}
# maxpool3_fp8_kernel<2> (stride (2, 2)) and <1> (stride (2, 1)); mostly negative inputs
MAXPOOL3 = {
    "s2-valid-c64": ((2, 15, 15, 64), (3, 3), (2, 2), (0, 0, 0, 0), 1.0, 0, 80),
    "s2-same-c48": ((3, 9, 13, 48), (3, 3), (2, 2), (1, 1, 1, 1), 0.5, 32, 96),
    "s2-asym-c16": ((1, 8, 10, 16), (3, 3), (2, 2), (0, 1, 0, 1), 2.0, 16, 48),
    "s21-same-c48": ((2, 11, 7, 48), (3, 3), (2, 1), (1, 1, 1, 1), 2.0 ** -10, 0, 64),
    "s21-asym-c16": ((1, 9, 9, 16), (3, 3), (2, 1), (0, 1, 0, 1), 2.0, 16, 48),
    "s21-valid-c16": ((2, 9, 8, 16), (3, 3), (2, 1), (0, 0, 0, 0), 0.25, 0, 32),
}


def _pool_cases(mode):
    if mode == "max":
        return {**{("pool", n): c for n, c in POOL.items()}, **{("maxpool3", n): c for n, c in MAXPOOL3.items()}}
    return {("pool", n): c for n, c in {**POOL, **POOL_AVG_ONLY}.items()}


@functools.lru_cache(maxsize=None)
def pool_case(mode, family, name):
    shape, k, s, pad, rq, _, _ = _pool_cases(mode)[(family, name)]
    x = pool_data((family, name), shape)
    if family == "maxpool3":   # mostly negative (four of five positives negated): all-negative windows at the padding
        x = torch.where(torch.rand(shape, generator=_gen("neg", name)) < 0.8, -x.abs(), x)
    y, tr = ref_pool(x, k, s, pad, mode, rq)
    return x, y, tr


# avgpool_bias_act: bf16 integers m * 2^(c % 13) (m in [-8, 8]): channel c's average spans
# 2^(c % 13), so with out_q = 2^-4 the small channels reach the e4m3 subnormals and the large ones
# saturate; bias[c] = (k / 4) * 2^(c % 13).  H = W = 5 with a padded 3x3 window has the counts 4, 6
# and 9.  name -> (kernel, stride, pad): avgpool3_epi_kernel, avgpool_epi_kernel<.., 2> (row stride
# 2 keeps the 3x3 window off the unrolled kernel; 2x2 has the counts 1, 2, 4), and <.., 1>.
AVGPOOL = {
    "avgpool3-3x3-s1": ((3, 3), (1, 1), (1, 1, 1, 1)),
    "generic2-3x3-s21": ((3, 3), (2, 1), (1, 1, 1, 1)),
    "generic2-2x2-s1": ((2, 2), (1, 1), (0, 1, 0, 1)),
    "generic1-3x3-s2": ((3, 3), (2, 2), (1, 1, 1, 1)),
}
AVG_SHAPE, AVG_Q = (2, 5, 5, 32), 2.0 ** -4


@functools.lru_cache(maxsize=None)
def avgpool_case(name, act, out_fp8):
    k, s, pad = AVGPOOL[name]
    gen = _gen("avgpool", name)
    oct_ = torch.pow(torch.tensor(2.0, dtype=F64), (torch.arange(AVG_SHAPE[3]) % 13).double())
    x = _ints(gen, AVG_SHAPE, -8, 8) * oct_
    bias = _ints(gen, (AVG_SHAPE[3],), -8, 8) / 4 * oct_
    assert torch.equal(_bf(x), x)
    y, tr = ref_avgpool_epi(x, bias, k, s, pad, act, AVG_Q if out_fp8 else None)
    return x, bias, y, tr


GAP = {"hw25-c64": (2, 25, 64, 0.5), "hw64-c64": (2, 64, 64, 0.37), "hw25-c4112": (2, 25, 4112, 0.37)}


@functools.lru_cache(maxsize=None)
def gap_case(name):
    N, HW, C, s = GAP[name]
    x = pool_data(("gap", name), (N, HW, C))
    y, tr = ref_gap(x, s)
    return x, y, tr


# ------------------------------------------------------------ non-GPU: the mirrors alone
def test_torch_e4m3_cast_rounds_to_nearest_even():
    """``_e4m3`` rests on torch's fp32 -> float8_e4m3fn cast: against a search over the 127
    positive e4m3 values, on every midpoint and its two fp32 neighbours, subnormals included."""
    vals = torch.arange(0, 127, dtype=torch.int16).to(U8).view(E4M3).double()   # 0 .. 448, ascending
    mid = (vals[:-1] + vals[1:]) / 2
    probe = torch.cat([vals, mid, _f32(mid * (1 + 2.0 ** -23)), _f32(mid * (1 - 2.0 ** -23)),
                       torch.tensor([449.0, 1e4, 2.0 ** -11, 2.0 ** -12], dtype=F64)])
    probe = torch.cat([probe, -probe])
    a = probe.abs().clamp(max=448.0)
    hi = torch.searchsorted(vals, a).clamp(max=126)
    lo = (hi - 1).clamp(min=0)
    dl, dh = a - vals[lo], vals[hi] - a
    pick = torch.where(dl < dh, lo, torch.where(dh < dl, hi, torch.where(lo % 2 == 0, lo, hi)))
    want = pick.to(U8) | ((probe < 0).to(U8) << 7)
    assert torch.equal(_canon(_e4m3(probe)), _canon(want))


def _host_conv(d, g, act, out_fp8, in_bf16):
    x = d["x"].float() if in_bf16 else _e4m3(d["x"])
    xs = 1.0 / IN_Q if in_bf16 else 1.0
    y = Q.conv2d_nhwc_fp8(x, xs, _e4m3(d["w"]).reshape(g.Cout, -1), g.k, (d["scale"] / xs).float(), d["bias"].float(),
                          g.stride, g.pad, g.dil, act, out_scale=1.0 / OUT_Q if out_fp8 else None)
    return y.reshape(-1, g.Cout)


def test_conv_mirror_equals_the_host_path():
    """``Q.conv2d_nhwc_fp8`` on host tensors sums the same exact values in fp32 and quantises at
    the same points (its bf16 output stays fp32: rounded to bf16 here)."""
    for family, cases in (("igemm", IGEMM), ("gemm", GEMMS), ("lite", LITE)):
        for name, (g, act, *_) in cases.items():
            for in_bf16 in ((False, True) if family != "lite" else (False,)):
                for out_fp8 in (True, False):
                    d, y, _ = conv_case(family, name, in_bf16, out_fp8)
                    h = _host_conv(d, g, act, out_fp8, in_bf16)
                    if out_fp8:
                        assert torch.equal(_canon(h), _canon(y)), (name, in_bf16)
                    else:
                        assert torch.equal(_bf(h.double()), y), (name, in_bf16)


def test_multi_mirror_equals_the_host_path():
    for C in (96, 192):
        for layout in MULTI_LAYOUTS:
            d, segs, ys, _ = multi_case(C, layout)
            g = _multi_geom(C, layout)
            outs = [torch.zeros((g.N, g.H, g.W, c1 - c0), dtype=F32 if q is None else U8) for c0, c1, q in segs]
            Q.conv2d_nhwc_fp8_multi(_e4m3(d["x"]), 1.0, _e4m3(d["w"]).reshape(g.Cout, -1), (1, 1), d["scale"].float(),
                                    d["bias"].float(), d["lo"].float(),
                                    [(o, c0, c1, 0, None if q is None else 1.0 / q) for o, (c0, c1, q) in zip(outs, segs)])
            for o, y, (c0, c1, q) in zip(outs, ys, segs):
                o = o.reshape(-1, c1 - c0)
                assert torch.equal(o.double(), y) if q is None else torch.equal(_canon(o), _canon(y)), (C, layout, c0)


def test_pool_mirrors_equal_the_host_paths():
    """Max pools everywhere.  The host average pools divide first (``(sum / cnt) * rq``,
    ``sum / cnt + bias``, ``mean * s``) where the kernels multiply by a rounded reciprocal, so
    they are the same function only where the count and the scale are powers of two."""
    for (family, name), (shape, k, s, pad, rq, _, _) in _pool_cases("max").items():
        x, y, _ = pool_case("max", family, name)
        assert torch.equal(_canon(Q.pool2d_nhwc_fp8(_e4m3(x), k, s, pad, "max", rq)), _canon(y)), name
    for name in ("2x2-s2-asym-c48", "2x2-s1-asym-c16"):
        shape, k, s, pad, rq, _, _ = POOL[name]
        x, y, _ = pool_case("avg", "pool", name)
        assert torch.equal(_canon(Q.pool2d_nhwc_fp8(_e4m3(x), k, s, pad, "avg", rq)), _canon(y)), name
    k, s, pad = AVGPOOL["generic2-2x2-s1"]
    for act in (None, "relu"):
        x, bias, y, _ = avgpool_case("generic2-2x2-s1", act, True)
        assert torch.equal(_canon(Q.avgpool_bias_act(x.float(), k, s, pad, bias.float(), act, 1.0 / AVG_Q)), _canon(y))
        x, bias, y, _ = avgpool_case("generic2-2x2-s1", act, False)
        assert torch.equal(_bf(Q.avgpool_bias_act(x.float(), k, s, pad, bias.float(), act).double()), y)
    x = pool_data(("gap", "host"), (2, 64, 64))
    assert torch.equal(_bf(Q.global_avgpool_fp8(_e4m3(x).reshape(2, 8, 8, 64), 0.5).double()), ref_gap(x, 0.5)[0])


def _conv_family_cases():
    for family, cases in (("igemm", IGEMM), ("gemm", GEMMS), ("lite", LITE)):
        for name, (g, act, *_) in cases.items():
            for in_bf16 in ((False, True) if family != "lite" else (False,)):
                yield family, name, g, act, in_bf16


def test_conv_data_make_every_rounding_observable():
    """Per case: some fp8 outputs saturate at +448, some are e4m3 subnormals, ReLU zeroes some
    and keeps some, no-act cases keep negatives (-448 among them); the quantisation on load
    changes some bf16 inputs and saturates some; every intermediate is exact in fp32."""
    for family, name, g, act, in_bf16 in _conv_family_cases():
        d, y, tr = conv_case(family, name, in_bf16, True)
        yb, trb = conv_case(family, name, in_bf16, False)[1:]
        print(family, name, in_bf16, "peak", tr.peak, tr.stats, "sat", (y == 0x7E).double().mean().item(), "sub",
              _is_sub(y).double().mean().item())
        assert tr.peak < EXACT and trb.peak < EXACT
        assert (y == 0x7E).any() and _is_sub(y).any(), (name, in_bf16)
        if act == "relu":
            zero = ((y & 0x7F) == 0).double().mean().item()
            assert 0.1 < zero < 0.9 and not _is_neg(y).any() and not (yb < 0).any(), (name, zero)
        else:
            assert _is_neg(y).any() and (y == 0xFE).any() and (yb < 0).any(), name
        assert (yb != _f32(yb)).sum() == 0 and (yb.abs() > 256).any()   # bf16 values, some beyond 8 bits
        if in_bf16:
            assert tr.stats["in_changed"] > 0.05 and tr.stats["in_saturated"] > 0.001, tr.stats


def test_multi_and_pool_data_make_every_rounding_observable():
    for C in (96, 192):
        for layout in MULTI_LAYOUTS:
            d, segs, ys, tr = multi_case(C, layout)
            fp8 = torch.cat([y for y, (_, _, q) in zip(ys, segs) if q is not None], 1)
            assert (fp8 == 0x7E).any() and _is_sub(fp8).any() and tr.peak < EXACT
            relu = torch.cat(ys[:3], 1)
            zero = ((relu & 0x7F) == 0).double().mean().item()
            assert 0.1 < zero < 0.9 and not _is_neg(relu).any(), zero
            assert _is_neg(ys[4]).any() and (ys[3] > 256).any()      # no-act segment; bf16 segment beyond 8 bits
    for mode in ("max", "avg"):
        ys = [pool_case(mode, *key)[1] for key in _pool_cases(mode)]
        for fam in ("pool", "maxpool3") if mode == "max" else ("pool",):
            y = torch.cat([v.reshape(-1) for v, key in zip(ys, _pool_cases(mode)) if key[0] == fam])
            assert (y == 0x7E).any() and _is_sub(y).any() and _is_neg(y).any(), (mode, fam)
    for out_fp8 in (True, False):
        for act in (None, "relu"):
            y = torch.cat([avgpool_case(n, act, out_fp8)[2].reshape(-1) for n in AVGPOOL])
            if out_fp8:
                assert (y == 0x7E).any() and _is_sub(y).any()
                assert _is_neg(y).any() if act is None else ((y & 0x7F) == 0).any() and not _is_neg(y).any()
            else:
                assert (y < 0).any() if act is None else ((y == 0).any() and not (y < 0).any())
    for name in AVGPOOL:   # the counts the issue asks for
        k, s, pad = AVGPOOL[name]
        cnt = set(_windows(torch.zeros(AVG_SHAPE, dtype=F64), k, s, pad, 0.0)[1].reshape(-1).tolist())
        assert cnt == ({1.0, 2.0, 4.0} if k == (2, 2) else {4.0, 6.0, 9.0}), (name, cnt)


def _differs(a, b):
    if a.dtype == U8:
        a, b = _canon(a), _canon(b)
    return a.shape == b.shape and not torch.equal(a, b)


def _conv_fault_applies(fault, g, out_fp8, bm):
    K, M = g.k[0] * g.k[1] * g.Cin, _pixels(g)
    return {"drop_chunk": True, "stale_stage": K > BK, "stale_rows": M > bm and M % bm != 0,
            "tap_swap": g.k != (1, 1), "no_dilation": g.dil != (1, 1), "scale_shift4": True,
            "round_via_bf16": out_fp8}.get(fault, False)


@pytest.mark.parametrize("fault", FAULTS)
def test_wrong_variants_differ_from_the_mirrors(fault):
    """Each fault changes at least one output byte of every case it applies to."""
    applied = 0
    for family, name, g, act, in_bf16 in _conv_family_cases():
        for out_fp8 in (True, False):
            for bm in (128,) if family == "lite" else (128, 256):
                if not _conv_fault_applies(fault, g, out_fp8, bm):
                    continue
                d, y, _ = conv_case(family, name, in_bf16, out_fp8)
                w = ref_conv(**d, g=g, act=act, out_q=OUT_Q if out_fp8 else None, in_q=IN_Q if in_bf16 else None,
                             bm=bm, fault=fault)[0]
                assert _differs(w, y), (fault, family, name, in_bf16, out_fp8, bm)
                applied += 1
    for C in (96, 192):
        for layout in MULTI_LAYOUTS:
            g = _multi_geom(C, layout)
            if fault not in ("round_direct", "seg_shift16") and not (
                    fault != "round_via_bf16" and _conv_fault_applies(fault, g, True, 128)):
                continue
            d, segs, ys, _ = multi_case(C, layout)
            ws = ref_multi(**d, segs=segs, g=g, fault=fault)[0]
            hit = [_differs(w, y) for w, y in zip(ws, ys)]
            if fault == "seg_shift16":
                assert hit[1], (C, layout)          # the moved channels belong to segment 1
            elif fault == "round_direct":
                assert hit == [q is not None for _, _, q in segs], (C, layout, hit)
            else:
                assert all(hit), (fault, C, layout, hit)
            applied += 1
    if fault in ("pad_counted", "pad_wins_max"):
        mode = "avg" if fault == "pad_counted" else "max"
        for key, (shape, k, s, pad, rq, _, _) in _pool_cases(mode).items():
            if pad == (0, 0, 0, 0):
                continue
            x, y, _ = pool_case(mode, *key)
            assert _differs(ref_pool(x, k, s, pad, mode, rq, fault=fault)[0], y), (fault, key)
            applied += 1
    if fault == "pad_counted":
        for name, (k, s, pad) in AVGPOOL.items():
            for act in (None, "relu"):
                for out_fp8 in (True, False):
                    x, bias, y, _ = avgpool_case(name, act, out_fp8)
                    w = ref_avgpool_epi(x, bias, k, s, pad, act, AVG_Q if out_fp8 else None, fault=fault)[0]
                    assert _differs(w, y), (name, act, out_fp8)
    assert applied, fault


def test_pool2d_nhwc_fp8_rejects_a_slot_past_the_row_end():
    """``pool2d_nhwc_fp8`` throws before any launch when the channel slot does not fit the output
    row or the problem is empty (host argument checks: no GPU), and so does the wrapper."""
    from flink_tensorflow_amd import _ext

    hip = _ext.hip(required=False)
    if hip is None:
        pytest.skip("HIP kernel library not built")
    x = torch.zeros((1, 4, 4, 32), dtype=U8)
    y = torch.zeros((1, 2, 2, 48), dtype=U8)

    def call(N=1, Ho=2, Wo=2, C=32, ldy=48, off=16, kh=2, sh=2):
        hip.pool2d_nhwc_fp8(x.data_ptr(), y.data_ptr(), N, 4, 4, C, Ho, Wo, kh, 2, sh, 2, 0, 0, ldy, off, 1, 1.0, 0)

    for kw in (dict(off=32), dict(ldy=32, off=16), dict(N=0), dict(Ho=0), dict(Wo=0), dict(kh=0), dict(sh=0),
               dict(off=-16)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):
        Q.pool2d_nhwc_fp8(x, (2, 2), (2, 2), out=y, out_channel_offset=32)
    with pytest.raises(ValueError):
        Q.pool2d_nhwc_fp8(x, (2, 2), (2, 2), out=torch.zeros((1, 3, 2, 48), dtype=U8), out_channel_offset=0)
    assert Q.pool2d_nhwc_fp8(x, (2, 2), (2, 2), out=y, out_channel_offset=16) is y


# ------------------------------------------------------------------------------ GPU helpers
DEV = torch.device("cuda", 0)


def _guarded(M, width, fp8):
    """Output of ``M + GUARD`` pixel rows of ``width`` channels, all sentinel."""
    if fp8:
        return torch.full((M + GUARD, width), SENT8, dtype=U8, device=DEV)
    return torch.full((M + GUARD, width), SENT16, dtype=BF, device=DEV)


def _assert_slot(what, buf, want, off, tile, out_shape):
    """``buf[:M, off:off + C]`` equals ``want`` (fp8 bytes after the +-0 mapping, bf16 by value:
    ``torch.equal``) and every other element of ``buf`` still holds the sentinel.  A mismatch
    names the (M tile, N tile) of ``tile`` = (BM, BN), pixel (n, oh, ow) and channel."""
    fp8 = buf.dtype == U8
    M, C = want.shape
    got_all = buf.cpu()
    got = got_all[:M, off:off + C]
    got, ref = (_canon(got), _canon(want)) if fp8 else (got, want.to(BF))
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        _, Ho, Wo = out_shape
        lines = []
        for m, c in bad[:12].tolist():
            n, r = divmod(m, Ho * Wo)
            g, e = (f"0x{got[m, c].item():02x}", f"0x{ref[m, c].item():02x}") if fp8 else (got[m, c].item(), ref[m, c].item())
            lines.append(f"  M tile {m // tile[0]}, N tile {c // tile[1]}, pixel (n {n}, oh {r // Wo}, ow {r % Wo}) = row "
                         f"{m % tile[0]} of the tile, channel {c}: got {g}, expected {e}")
        raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} values differ (tile {tile[0]} x {tile[1]}); "
                             "first:\n" + "\n".join(lines))
    outside = torch.ones(got_all.shape, dtype=torch.bool)
    outside[:M, off:off + C] = False
    sent = SENT8 if fp8 else SENT16
    assert (got_all[outside] == sent).all(), (f"{what}: {(got_all[outside] != sent).sum().item()} values written "
                                               f"outside rows [0, {M}) x channels [{off}, {off + C})")


def _conv_inputs(d, g, in_bf16):
    x = d["x"].to(BF).to(DEV) if in_bf16 else _e4m3(d["x"]).to(DEV)
    return (x, 1.0 / IN_Q if in_bf16 else 1.0, _e4m3(d["w"]).reshape(g.Cout, -1).to(DEV),
            d["scale"].float().to(DEV), d["bias"].float().to(DEV))


def _run_conv(family, name, in_bf16, out_fp8, cfg, tile):
    g, act, off, width = {"igemm": IGEMM, "lite": LITE}[family][name]
    d, want, _ = conv_case(family, name, in_bf16, out_fp8)
    Ho, Wo = _out_hw(g)
    M = g.N * Ho * Wo
    buf = _guarded(M, width, out_fp8)
    x, xs, wq, scale, bias = _conv_inputs(d, g, in_bf16)
    Q.conv2d_nhwc_fp8(x, xs, wq, g.k, scale, bias, g.stride, g.pad, g.dil, act, out_scale=1.0 / OUT_Q if out_fp8 else None,
                      out=buf[:M].view(g.N, Ho, Wo, width), out_channel_offset=off, cfg=cfg, chan_scale=scale)
    torch.cuda.synchronize()
    _assert_slot(f"{family} {name} cfg {cfg} in {'bf16' if in_bf16 else 'fp8'}", buf, want, off, tile, (g.N, Ho, Wo))


def _io_id(v):
    return {True: "fp8", False: "bf16"}[v]


# --------------------------------------------------------------------- GPU: bit-exact cases
@pytest.mark.gpu
def test_mfma_f8f6f4_sums_integer_products_exactly():
    """The premise of everything below, at the smallest size: one 128 x 64 tile, one K-tile
    (K = 128), fp8 in, bf16 out with scale 1 and no bias, values small enough that bf16 holds
    the sum: the output is the integer sum itself."""
    gen = _gen("premise")
    x, w = _ints(gen, (64, 128), 0, 2), _ints(gen, (64, 128), -1, 1)
    want = x @ w.t()
    assert want.abs().max() <= 256 and (want != 0).any()
    buf = _guarded(64, 64, False)
    Q.gemm_fp8(_e4m3(x).to(DEV), 1.0, _e4m3(w).to(DEV), torch.ones(64, device=DEV), out=buf[:64], cfg=2)
    torch.cuda.synchronize()
    _assert_slot("128 x 64 tile, K 128", buf, want, 0, TILES[2], (64, 1, 1))


# cfg x input type x output type; 256 x 64 (cfg 1) with bf16 staging is reachable but never
# chosen (it spills), so one case covers it
def _tile_io(cases, bf16_on_cfg1):
    return [pytest.param(n, cfg, in_bf16, out_fp8, id=f"{n}-cfg{cfg}-in-{_io_id(not in_bf16)}-out-{_io_id(out_fp8)}")
            for n in cases for cfg in (0, 1, 2) for in_bf16 in (False, True) for out_fp8 in (True, False)
            if not (cfg == 1 and in_bf16) or (n, out_fp8) == bf16_on_cfg1]


@pytest.mark.gpu
@pytest.mark.parametrize("name,cfg,in_bf16,out_fp8", _tile_io(IGEMM, ("3x3-c48-144", True)))
def test_igemm_fp8_bit_exact(name, cfg, in_bf16, out_fp8):
    _run_conv("igemm", name, in_bf16, out_fp8, cfg, TILES[cfg])


@pytest.mark.gpu
@pytest.mark.parametrize("name,cfg,in_bf16,out_fp8", _tile_io(GEMMS, None))
def test_gemm_fp8_bit_exact(name, cfg, in_bf16, out_fp8):
    g, act = GEMMS[name]
    d, want, _ = conv_case("gemm", name, in_bf16, out_fp8)
    buf = _guarded(g.N, g.Cout, out_fp8)
    x, xs, wq, scale, bias = _conv_inputs(d, g, in_bf16)
    Q.gemm_fp8(x.reshape(g.N, g.Cin), xs, wq, scale, bias, act, out_scale=1.0 / OUT_Q if out_fp8 else None,
               out=buf[:g.N], cfg=cfg, chan_scale=scale)
    torch.cuda.synchronize()
    _assert_slot(f"gemm {name} cfg {cfg}", buf, want, 0, TILES[cfg], (g.N, 1, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("out_fp8", [True, False], ids=lambda v: "out-" + _io_id(v))
@pytest.mark.parametrize("name", list(LITE))
def test_conv_lite_fp8_bit_exact(name, out_fp8):
    assert _lite_bn(LITE[name][0].Cout) == LITE_BN[name]
    _run_conv("lite", name, False, out_fp8, 11, (128, LITE_BN[name]))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(MULTI_LAYOUTS))
@pytest.mark.parametrize("C", [96, 192], ids=["c96-one-stage", "c192-two-stages"])
def test_conv_fp8_multi_bit_exact(C, layout):
    g = _multi_geom(C, layout)
    d, segs, wants, _ = multi_case(C, layout)
    M = g.N * g.H * g.W
    bufs = [_guarded(M, width, q is not None) for _, q, _, width in MULTI_LAYOUTS[layout]]
    x, xs, wq, scale, bias = _conv_inputs(d, g, False)
    Q.conv2d_nhwc_fp8_multi(x, xs, wq, (1, 1), scale, bias, d["lo"].float().to(DEV),
                            [(b[:M].view(g.N, g.H, g.W, -1), c0, c1, off, None if q is None else 1.0 / q)
                             for b, (c0, c1, q), (_, _, off, _) in zip(bufs, segs, MULTI_LAYOUTS[layout])],
                            chan_scale=scale)
    torch.cuda.synchronize()
    bn = _lite_bn(g.Cout)
    for i, (b, want, (c0, _, _), (_, _, off, _)) in enumerate(zip(bufs, wants, segs, MULTI_LAYOUTS[layout])):
        try:
            _assert_slot(f"multi C {C} {layout} segment {i}", b, want, off, (128, bn), (g.N, g.H, g.W))
        except AssertionError as e:   # channels above are the segment's own: name the GEMM channel too
            raise AssertionError(f"{e}\n  (segment {i} starts at GEMM channel {c0}, channel tile {bn})") from None


def _run_pool(mode, family, name):
    shape, k, s, pad, rq, off, width = _pool_cases(mode)[(family, name)]
    x, want, _ = pool_case(mode, family, name)
    N, Ho, Wo, C = want.shape
    buf = _guarded(N * Ho * Wo, width, True)
    Q.pool2d_nhwc_fp8(_e4m3(x).to(DEV), k, s, pad, mode, rq, out=buf[:N * Ho * Wo].view(N, Ho, Wo, width),
                      out_channel_offset=off)
    torch.cuda.synchronize()
    _assert_slot(f"{family} {mode} {name}", buf, want.reshape(-1, C), off, (N * Ho * Wo, C), (N, Ho, Wo))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POOL))
def test_pool_fp8_max_bit_exact(name):
    _run_pool("max", "pool", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POOL) + list(POOL_AVG_ONLY))
def test_pool_fp8_avg_bit_exact(name):
    _run_pool("avg", "pool", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MAXPOOL3))
def test_maxpool3_fp8_bit_exact(name):
    _run_pool("max", "maxpool3", name)


@pytest.mark.gpu
@pytest.mark.parametrize("out_fp8", [True, False], ids=lambda v: "out-" + _io_id(v))
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("name", list(AVGPOOL))
def test_avgpool_bias_act_bit_exact(name, act, out_fp8):
    k, s, pad = AVGPOOL[name]
    x, bias, want, _ = avgpool_case(name, act, out_fp8)
    N, Ho, Wo, C = want.shape
    M, off, width = N * Ho * Wo, 16, 64
    buf = _guarded(M, width, out_fp8)
    Q.avgpool_bias_act(x.to(BF).to(DEV), k, s, pad, bias.float().to(DEV), act, 1.0 / AVG_Q if out_fp8 else None,
                       out=buf[:M].view(N, Ho, Wo, width), out_channel_offset=off)
    torch.cuda.synchronize()
    _assert_slot(f"avgpool {name} {act}", buf, want.reshape(-1, C), off, (M, C), (N, Ho, Wo))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GAP))
def test_gap_fp8_bit_exact(name):
    N, HW, C, s = GAP[name]
    x, want, _ = gap_case(name)
    buf = _guarded(N, C, False)
    Q.global_avgpool_fp8(_e4m3(x).to(DEV).reshape(N, HW, 1, C), s, out=buf[:N])
    torch.cuda.synchronize()
    _assert_slot(f"gap {name}", buf, want, 0, (N, C), (N, 1, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("q", [1.0, 0.5, 2.0 ** -7, 3.0])
def test_quantize_every_bf16_bit_pattern(q):
    """All 65 536 bf16 bit patterns but the NaNs (infinities saturate on both sides), padded
    with zeros to a multiple of 16."""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[((bits & 0x7F80) != 0x7F80) | ((bits & 0x7F) == 0)]
    bits = torch.cat([bits, torch.zeros(-bits.numel() % 16, dtype=torch.int32)])
    x = bits.to(torch.int16).view(BF)
    scale = 1.0 / q
    q32 = _r32(1.0 / scale).double()                    # what the wrapper hands to the kernel
    want = _e4m3(_f32(x.double() * q32))                # 8 x 24 significant bits: exact in float64
    buf = _guarded(1, x.numel(), True)
    Q.quantize(x.to(DEV), scale, out=buf[0])
    torch.cuda.synchronize()
    got = _canon(buf[0].cpu())
    bad = (got != _canon(want)).nonzero().reshape(-1)
    assert bad.numel() == 0, (f"q {q}: {bad.numel()} patterns differ; first (bf16 bits, got, expected) "
                              f"{[(hex(bits[i].item()), hex(got[i].item()), hex(want[i].item())) for i in bad[:12]]}")
    assert (buf[1:] == SENT8).all()


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1.0, 0.5, 0.0123])
def test_dequantize_every_e4m3_byte(s):
    """All 256 bytes but the two NaN encodings (0x7F, 0xFF), padded to 256."""
    b = torch.arange(256, dtype=torch.int16).to(U8)
    b = torch.cat([b[(b & 0x7F) != 0x7F], torch.zeros(2, dtype=U8)])
    want = _bf(_f32(_dec(b) * _r32(s).double()))
    buf = _guarded(1, 256, False)
    Q.dequantize(b.to(DEV), s, out=buf[0])
    torch.cuda.synchronize()
    got = buf[0].cpu()
    assert torch.equal(got, want.to(BF)), [(hex(b[i].item()), got[i].item(), want[i].item())
                                           for i in (got != want.to(BF)).nonzero().reshape(-1)[:12]]
    assert (buf[1:] == SENT16).all()
