"""``conv_lite`` of ``kernels/conv_pp.hip`` (the 128x128 four-wave implicit-GEMM convolution, one
and two sources), bit for bit: the (channel chunk, filter column, filter row) K walk, padding by
descriptor range, strides, dilation, the dual-source switch, both epilogues and the host-side
argument checks.  Method and helpers are those of ``tests/test_igemm_exact.py``.

The operands are integers that are exact in bf16 (the bias is fp32 half-integers): x in [-8, 8],
w in [-4, 4], bias halves in [-600, 600] with both signs, residual integers in [-256, 256]; without
a bias x in [-24, 24] and w in [-8, 8], so that the sums alone pass 256, where bf16 starts to round.
Each reference asserts ``sum |x||w| + |b| + |r| < 2^23`` per output: fp32 accumulation is then exact
in any order and the only inexact steps are the kernel's ``f2bf`` roundings (round to nearest even).
The float64 reference is written from the ``.hip`` file and rounds where it rounds:

without residual
    ``y = bf16(act(acc + bias))``.
with residual
    ``a = bf16(acc + bias)`` into the LDS tile, then ``y = bf16(act(float(a) + r))``: two roundings,
    the first before the residual add.  ``ConvPP._reference`` rounds once.
dual
    one accumulator over ``[K of source 0 | K of source 1]``; source 1 is pointwise and read at
    ``(oh * sh1, ow * sw1)``.

The reference has two inputs: an im2col matrix ``X [M, K]``, built from the definition (a loop over
the filter taps on a zero-padded float64 image with strided and dilated slices, K in (kh, kw, ci)
order, bottom and right padding as implied by ``(OH, OW)``), and the weight matrix ``W [Cout, K]``.
It is anchored against ``torch.nn.functional.conv2d`` in float64 and against ``ConvPP._reference``.

The GPU tests compare bf16 bit patterns (``view(torch.int16)``).  No -0 can arise: the accumulators
start from +0 and sums of integers give +0 under round-to-nearest, the data hold no -0 and ReLU is
``x > 0 ? x : 0``.  A mismatch is reported with (pixel, channel, tile index, K-tile count) of the
first few elements.

Guards of every GPU case: the output goes through ``out=`` into a buffer pre-filled with the
sentinel 2^100, row stride ``ldy = Cout + 40``, a channel offset from (16, 0, 8, 24) in turn and 128
guard rows (one more tile) after the last pixel; everything outside the written window must still
hold the sentinel and nothing inside may.  Every operand (x, w, bias, residual, second source) is a
view between NaN bands.  Bias and residual are plain global loads, so a read past either end of
them shows as NaN.  x, the second source and w (with ``ldw``) go through buffer descriptors sized
exactly: a read past their end returns zero and one before their start cannot be formed, so the NaN
bands see nothing of those reads; the value comparison covers them.  Cases with a residual run a
second time through the raw entry (``_hip().conv_pp``) with ``ldr = Cout + 24`` and NaN in the pad
columns.

Paths that no test reached before: dual mode with a non-pointwise (3x3, padded) source 0, which
the lowering does not emit but the kernel and ``ConvPP`` accept (``nk0`` comes from ``KH * KW * C``);
``ldr != Cout``; the XCD tile remap with a tile count that is no multiple of 8 (12 and 9 tiles).

The wrong variants (``FAULTS``), each of which must differ from the truth on every case it applies
to: ``drop_tap``; ``wrap_row`` (a tap outside [0, W) reads the adjacent pixel in memory instead of
zero); ``pad_swap``; ``dil_swap``; ``stride_swap``; ``walk_swap`` (taps walked in (kw, kh) order against
(kh, kw) weights); ``chunk_next_tap`` (C = 128: the second 64-channel chunk from the next tap);
``stale_stage`` (K-tile ``t >= 1`` uses the X rows of tile ``t - 1``); ``image_straddle`` (``m -> (n, oh,
ow)`` with the tile's first image for all 128 rows); ``dual_switch`` (source 1 starts one K-tile
early); ``shortcut_stride1``; ``round_once``; ``res_ld`` (residual rows ``Cout`` apart where ``ldr`` is
wider); ``swap_frag`` (two 16-channel fragments swapped).

The non-GPU tests check the reference alone: the exactness bound, that the data make every
rounding and ReLU observable, the anchors, the wrong variants and the coverage of the case list."""
import collections
import functools
import itertools
import zlib

import pytest
import torch

from flink_tensorflow_amd.ops import kernels as K
from test_igemm_exact import EXACT, GAP, SENT, COFFS   # the conventions of that file, not copies of them

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
BT = 128                 # tile edge; also the guard rows after the last pixel
RPAD = 24                # raw entry: ldr - Cout
FAULTS = ("drop_tap", "wrap_row", "pad_swap", "dil_swap", "stride_swap", "walk_swap", "chunk_next_tap", "stale_stage",
          "image_straddle", "dual_switch", "shortcut_stride1", "round_once", "res_ld", "swap_frag")

# src: shape (N, H, W, C), k (KH, KW), st (sh, sw), pad (ph, pw) top / left, dil (dh, dw)
_Src = collections.namedtuple("_Src", "shape k st pad dil")
_Case = collections.namedtuple("_Case", "name geom srcs Cout ohw act bias res coff")
_SEQ = itertools.count()


def _s(shape, k=(1, 1), st=(1, 1), pad=(0, 0), dil=(1, 1)):
    return _Src(shape, k, st, pad, dil)


# name -> (sources, Cout, (OH, OW))
GEOMS = {
    # one K-tile (prologue only), Cout = 8, M = 70: one tile with a tail
    "1x1-m70-n8": ([_s((2, 5, 7, 64))], 8, (5, 7)),
    # two M-tiles whose 128 rows straddle image boundaries (M = 147), N tail, nk = 9
    "3x3-m147-n136": ([_s((3, 7, 7, 64), (3, 3), pad=(1, 1))], 136, (7, 7)),
    # cpt = 2 chunk walk, nk = 18, stride 2 on even extents: the last taps read the bottom / right
    # padding that only the output size implies
    "3x3s2-c128-even": ([_s((2, 8, 6, 128), (3, 3), (2, 2))], 72, (4, 3)),
    "3x3-s21-p10": ([_s((1, 10, 9, 64), (3, 3), (2, 1), (1, 0))], 72, (5, 7)),
    "1x7-p03": ([_s((1, 9, 9, 64), (1, 7), pad=(0, 3))], 72, (9, 9)),
    "7x1-p30": ([_s((1, 9, 9, 64), (7, 1), pad=(3, 0))], 72, (9, 9)),
    # most taps outside the image
    "5x5-d22-p44": ([_s((1, 9, 9, 64), (5, 5), pad=(4, 4), dil=(2, 2))], 72, (9, 9)),
    "3x3-d12-p12": ([_s((1, 9, 9, 64), (3, 3), pad=(1, 2), dil=(1, 2))], 40, (9, 9)),
    # the tile remap with r != 0: 4 x 3 = 12 tiles and 3 x 3 = 9 tiles
    "1x1-12tiles": ([_s((3, 13, 13, 64))], 264, (13, 13)),
    "1x1-9tiles": ([_s((2, 13, 13, 64))], 264, (13, 13)),
    # dual, minimal: nk0 = 1 plus one source-1 tile
    "dual-min": ([_s((2, 7, 7, 64)), _s((2, 14, 14, 64), st=(2, 2))], 72, (7, 7)),
    "dual-odd-c128": ([_s((2, 7, 7, 128)), _s((2, 13, 13, 128), st=(2, 2))], 136, (7, 7)),
    "dual-s23": ([_s((1, 7, 5, 64)), _s((1, 13, 14, 64), st=(2, 3))], 72, (7, 5)),
    # a 3x3 padded source 0 (nk0 = 9) and two source-1 tiles
    "dual-3x3": ([_s((2, 7, 7, 64), (3, 3), pad=(1, 1)), _s((2, 14, 14, 128), st=(2, 2))], 136, (7, 7)),
}
# every geometry sees bias, residual and act both ways; the two sets alternate, so that all eight
# combinations occur in the single and in the dual mode
_COMBOS = (((True, True, "relu"), (False, False, None), (True, False, None), (False, True, "relu")),
           ((False, False, "relu"), (True, True, None), (False, True, None), (True, False, "relu")))


def _cases():
    out, count = [], {1: 0, 2: 0}
    for geom, (srcs, Cout, ohw) in GEOMS.items():
        for bias, res, act in _COMBOS[count[len(srcs)] % 2]:
            coff = COFFS[next(_SEQ) % 4]
            name = f"{geom}-{act or 'none'}{'' if bias else '-nobias'}{'-res' if res else ''}-off{coff}"
            out.append(_Case(name, geom, tuple(srcs), Cout, ohw, act, bias, res, coff))
        count[len(srcs)] += 1
    return out


ALL_CASES = _cases()


def _ids(cases):
    return [c.name for c in cases]


def _geom(c):
    """(N, OH, OW, M, K, nk0)."""
    N, (OH, OW) = c.srcs[0].shape[0], c.ohw
    ks = [s.k[0] * s.k[1] * s.shape[3] for s in c.srcs]
    return N, OH, OW, N * OH * OW, sum(ks), ks[0] // 64


# ------------------------------------------------------------------------------------ data
def _bf(v):
    return v.to(BF).to(F64)


def _act(v, act):
    return torch.relu(v) if act == "relu" else v


def _gen(c, salt):
    g = torch.Generator().manual_seed(zlib.crc32(f"{c.name}/{salt}".encode()))
    N, OH, OW, M, Kd, nk0 = _geom(c)

    def ints(lo, hi, shape):
        return torch.randint(lo, hi + 1, shape, generator=g).to(F64)

    rx, rw = (8, 4) if c.bias else (24, 8)
    d = dict(xs=[ints(-rx, rx, s.shape) for s in c.srcs], w=ints(-rw, rw, (c.Cout, Kd)), bias=None, res=None)
    if c.bias:   # halves in [-600, 600], signs alternating along a random permutation: both occur
        sign = torch.ones(c.Cout, dtype=F64)
        sign[torch.randperm(c.Cout, generator=g)[::2]] = -1
        d["bias"] = sign * ints(1, 1200, (c.Cout,)) / 2
    if c.res:
        d["res"] = ints(-256, 256, (M, c.Cout))
    return d


@functools.lru_cache(maxsize=None)
def _data(c):
    """The case's operands as float64 (exact in bf16 / fp32, no -0).  The seed is the first of 64
    for which the conditions of ``test_data_make_the_properties_observable`` hold; that test asserts
    them (they are conditions on the data and the reference, the kernel has no part in them)."""
    for salt in range(64):
        d = _gen(c, salt)
        if not _unobservable(c, _reference(c, d=d).shares):
            break
    return d


# -------------------------------------------------------------------------------- reference
def _im2col(s, x, ohw):
    """``X [M, KH KW C]`` of one source from the definition: row m = output pixel (n, oh, ow), column
    k = (kh, kw, ci); the zero-padded image sliced per filter tap."""
    (N, H, W, C), (KH, KW), (sh, sw), (ph, pw), (dh, dw) = s
    OH, OW = ohw
    # the canvas: top / left padding, the image, and zeros as far as the last tap of the last pixel reaches
    Hp = max(ph + H, (KH - 1) * dh + (OH - 1) * sh + 1)
    Wp = max(pw + W, (KW - 1) * dw + (OW - 1) * sw + 1)
    xp = torch.zeros(N, Hp, Wp, C, dtype=F64)
    xp[:, ph:ph + H, pw:pw + W] = x
    cols = [xp[:, kh * dh:kh * dh + (OH - 1) * sh + 1:sh, kw * dw:kw * dw + (OW - 1) * sw + 1:sw].reshape(-1, C)
            for kh in range(KH) for kw in range(KW)]
    return torch.cat(cols, 1)


def _gather(s, x, ohw, fault=None):
    """The same matrix by address, as the kernel forms it: pixel (n, oh, ow) and tap (kh, kw) read
    ``x[n, oh sh - ph + kh dh, ow sw - pw + kw dw]`` if that lies inside the image, else zero.  The
    geometric wrong variants change the address or the test."""
    (N, H, W, C), (KH, KW), (sh, sw), (ph, pw), (dh, dw) = s
    OH, OW = ohw
    if fault == "pad_swap":
        ph, pw = pw, ph
    if fault == "dil_swap":
        dh, dw = dw, dh
    if fault == "stride_swap":
        sh, sw = sw, sh
    M = N * OH * OW
    m = torch.arange(M)
    n, oh, ow = m // (OH * OW), m // OW % OH, m % OW
    if fault == "image_straddle":   # the tile's first image for all its rows; oh runs on past OH
        n = (m // BT * BT) // (OH * OW)
        rem = m - n * (OH * OW)
        oh, ow = rem // OW, rem % OW
    flat = torch.cat([x.reshape(-1, C), torch.zeros(1, C, dtype=F64)])   # the last row: what a refused tap reads
    taps = [(kh, kw) for kh in range(KH) for kw in range(KW)]
    if fault == "walk_swap":
        taps = [(kh, kw) for kw in range(KW) for kh in range(KH)]
    cols = []
    for kh, kw in taps:
        ih, iw = oh * sh - ph + kh * dh, ow * sw - pw + kw * dw
        ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
        pix = (n * H + ih) * W + iw
        if fault == "wrap_row":     # the column test missing: the neighbouring pixel in memory
            ok = (ih >= 0) & (ih < H) & (pix >= 0) & (pix < N * H * W)
        t = flat[torch.where(ok, pix, torch.full_like(pix, N * H * W))]
        if fault == "drop_tap" and (kh, kw) == (KH // 2, KW // 2):
            t = torch.zeros_like(t)
        cols.append(t)
    if fault == "chunk_next_tap":   # channels [64, 128) of every tap from the next tap (zeros after the last)
        cols = [torch.cat([t[:, :64], (cols[i + 1] if i + 1 < len(cols) else torch.zeros_like(t))[:, 64:]], 1)
                for i, t in enumerate(cols)]
    return torch.cat(cols, 1)


def _wraps(s, ohw):
    """Some tap lies outside [0, W) at a row inside the image (``wrap_row`` then reads a pixel)."""
    (N, H, W, C), (KH, KW), (sh, sw), (ph, pw), (dh, dw) = s
    rows = any(0 <= oh * sh - ph + kh * dh < H for oh in range(ohw[0]) for kh in range(KH))
    return rows and any(not 0 <= ow * sw - pw + kw * dw < W for ow in range(ohw[1]) for kw in range(KW))


def _straddles(c):
    N, OH, OW, M, Kd, nk0 = _geom(c)
    return any(m0 // (OH * OW) != min(m0 + BT - 1, M - 1) // (OH * OW) for m0 in range(0, M, BT))


_GEO_FAULTS = ("drop_tap", "wrap_row", "pad_swap", "dil_swap", "stride_swap", "walk_swap", "chunk_next_tap",
               "image_straddle")
_Ref = collections.namedtuple("_Ref", "out exact peak shares")


def _matrix(c, d, fault=None):
    """``X [M, K]`` over both sources."""
    N, OH, OW, M, Kd, nk0 = _geom(c)
    s0 = c.srcs[0]
    X = _gather(s0, d["xs"][0], c.ohw, fault) if fault in _GEO_FAULTS else _im2col(s0, d["xs"][0], c.ohw)
    if len(c.srcs) == 2:
        s1, x1 = c.srcs[1], d["xs"][1]
        if fault == "shortcut_stride1":
            s1 = s1._replace(st=(1, 1))
        X1 = _gather(s1, x1, c.ohw, "image_straddle" if fault == "image_straddle" else None)
        X = torch.cat([X, X1], 1)
        if fault == "dual_switch":  # K-tiles from nk0 - 1 on walk source 1's memory from the pixel's first channel
            C1 = s1.shape[3]
            flat = torch.cat([x1.reshape(-1), torch.zeros(Kd, dtype=F64)])
            m = torch.arange(M)
            base = ((m // (OH * OW) * s1.shape[1] + m // OW % OH * s1.st[0]) * s1.shape[2] + m % OW * s1.st[1]) * C1
            k = torch.arange(Kd - 64 * (nk0 - 1))
            X = torch.cat([X[:, :64 * (nk0 - 1)], flat[(base[:, None] + k[None, :]).clamp(max=flat.numel() - 1)]], 1)
    if fault == "stale_stage":
        X = torch.cat([X[:, :64], X[:, :-64]], 1)
    return X


def _reference(c, fault=None, d=None):
    """float64 mirror of the kernel -> ``_Ref``: ``out [M, Cout]`` holding the bf16 values, ``exact`` =
    ``act(acc + bias + res)`` unrounded (what ``ConvPP._reference`` computes), ``peak`` = the largest
    ``sum |x||w| + |b| + |r|``, ``shares`` = what each rounding / activation did."""
    d = _data(c) if d is None else d
    N, OH, OW, M, Kd, nk0 = _geom(c)
    X, W = _matrix(c, d, fault), d["w"]
    acc = X @ W.t()
    if fault == "swap_frag":
        n = torch.arange(c.Cout)
        acc = acc[:, torch.where((n // 32 + 1) * 32 <= c.Cout, n ^ 16, n)]     # complete 32-channel groups only
    bias = torch.zeros(c.Cout, dtype=F64) if d["bias"] is None else d["bias"]
    v = acc + bias
    r = d["res"]
    Xt = X if fault is None else _matrix(c, d)
    peak = float((Xt.abs() @ W.abs().t() + bias.abs() + (0 if r is None else r.abs())).max())
    sh = {}
    if r is None:
        exact = _act(v, c.act)
        out = _bf(exact)
        sh["round"] = (out != exact).double().mean().item()
    else:
        if fault == "res_ld":   # rows taken Cout apart in the [M, Cout + RPAD] buffer (zeros in its pad)
            flat = torch.cat([r, torch.zeros(M, RPAD, dtype=F64)], 1).reshape(-1)
            r = flat[torch.arange(M)[:, None] * c.Cout + torch.arange(c.Cout)[None, :]]
        exact = _act(v + r, c.act)
        a = _bf(v)
        pre = _act(a + r, c.act)
        out = _bf(exact) if fault == "round_once" else _bf(pre)
        sh["round_a"] = (a != v).double().mean().item()
        sh["round"] = (_bf(pre) != pre).double().mean().item()
        sh["double"] = (_bf(pre) != _bf(exact)).double().mean().item()
    if c.act == "relu":
        sh["zeros"], sh["pos"] = (out == 0).double().mean().item(), (out > 0).double().mean().item()
    return _Ref(out, exact, peak, sh)


def _unobservable(c, s):
    bad = []
    if c.act == "relu" and min(s["zeros"], s["pos"]) < 0.05:
        bad.append("relu")
    if s["round"] == 0:
        bad.append("round")
    if c.res and (s["round_a"] == 0 or s["double"] == 0):
        bad.append("double rounding")
    return bad


@functools.lru_cache(maxsize=None)
def _ref(c):
    r = _reference(c)
    assert r.peak < EXACT, f"{c.name}: sum |x||w| + |b| + |r| = {r.peak} is not exact in fp32"
    return r


def _applies(fault, c):
    N, OH, OW, M, Kd, nk0 = _geom(c)
    s0, dual = c.srcs[0], len(c.srcs) == 2
    taps = s0.k[0] * s0.k[1]
    return {"drop_tap": taps > 1,
            "wrap_row": _wraps(s0, c.ohw),
            "pad_swap": s0.pad[0] != s0.pad[1],
            "dil_swap": s0.dil[0] != s0.dil[1],
            "stride_swap": s0.st[0] != s0.st[1],
            "walk_swap": s0.k[0] > 1 and s0.k[1] > 1,
            "chunk_next_tap": s0.shape[3] == 128 and taps > 1,
            "stale_stage": Kd > 64,
            "image_straddle": _straddles(c),
            "dual_switch": dual,
            "shortcut_stride1": dual and c.srcs[1].st != (1, 1),
            "round_once": c.res,
            "res_ld": c.res and M > 1,
            "swap_frag": c.Cout >= 32}[fault]


# ---------------------------------------------------------------------------- running a case
def _band(v, dtype, dev, ld=None):
    """``v`` on ``dev`` as a view between NaN bands (one leading-dimension row before and after, 8
    elements around a vector: the view stays 16-byte aligned); a matrix with ``ld`` has its rows
    ``ld`` apart with NaN in the pad columns.  -> (view, the whole buffer, which owns the memory)."""
    if v.dim() == 1:
        big = torch.full((v.numel() + 16,), float("nan"), dtype=dtype)
        big[8:-8] = v.to(dtype)
        big = big.to(dev)
        return big[8:-8], big
    shape = (v.shape[0] + 2, *v.shape[1:]) if ld is None else (v.shape[0] + 2, ld)
    big = torch.full(shape, float("nan"), dtype=dtype)
    big[1:-1, ..., :v.shape[-1]] = v.to(dtype)
    big = big.to(dev)
    return big[1:-1, ..., :v.shape[-1]], big


def _launch(c, dev, raw):
    """One launch into a fresh sentinel buffer -> the whole buffer on the host, [M + 128, ldy]."""
    d = _data(c)
    N, OH, OW, M, Kd, nk0 = _geom(c)
    ldy = c.Cout + GAP
    xs, _xs = zip(*(_band(x, BF, dev) for x in d["xs"]))
    w, _w = _band(d["w"], BF, dev)
    b, _b = (None, None) if d["bias"] is None else _band(d["bias"], F32, dev)
    r, _r = (None, None) if d["res"] is None else _band(d["res"], BF, dev, c.Cout + RPAD if raw else None)
    big = torch.full((M + BT, ldy), SENT, dtype=BF, device=dev)
    if raw:
        srcs = [(x.data_ptr(), N, s.shape[1], s.shape[2], s.shape[3], *s.k, *s.st, *s.pad, *s.dil)
                for x, s in zip(xs, c.srcs)]
        K._hip().conv_pp(srcs, w.data_ptr(), K._ptr(b), K._ptr(r), big.data_ptr(), N, OH, OW, c.Cout, ldy, c.coff,
                         c.Cout + RPAD, K.act_code(c.act), K._stream())
    else:
        cp = K.ConvPP([tuple(s) for s in c.srcs], c.Cout, c.ohw, dev)
        cp(list(xs), w, b, None if r is None else r.reshape(N, OH, OW, c.Cout), c.act,
           out=big[:M].view(N, OH, OW, ldy), out_channel_offset=c.coff)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return big.cpu()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check_window(buf, c, want, what):
    """Pixels < M, channels [coff, coff + Cout) of ``buf`` hold ``want`` bit for bit and no sentinel;
    everything else still holds the sentinel."""
    N, OH, OW, M, Kd, nk0 = _geom(c)
    Cout, coff = c.Cout, c.coff
    win = buf[:M, coff:coff + Cout]
    if not torch.equal(_bits(win), _bits(want)):
        bad = (_bits(win) != _bits(want)).nonzero()
        tn = -(-Cout // BT)
        lines = [f"  pixel m = {m} (n, oh, ow) = ({m // (OH * OW)}, {m // OW % OH}, {m % OW})  channel {ch}  "
                 f"tile {m // BT * tn + ch // BT} = ({m // BT}, {ch // BT}) of {-(-M // BT)} x {tn}  "
                 f"K-tiles {Kd // 64} ({nk0} of source 0): got {win[m, ch].item()!r}, want {want[m, ch].item()!r}"
                 for m, ch in bad[:8].tolist()]
        pytest.fail(f"{what}: {len(bad)} of {win.numel()} elements differ\n" + "\n".join(lines))
    assert not bool((win == SENT).any()), f"{what}: sentinel left inside the output"
    rest = buf.clone()
    rest[:M, coff:coff + Cout] = SENT
    if not bool((rest == SENT).all()):
        m, ch = (rest != SENT).nonzero()[0].tolist()
        pytest.fail(f"{what}: written outside the output window at pixel {m} (M = {M}), channel {ch} "
                    f"(window [{coff}, {coff + Cout}))")


# --------------------------------------------------------------------------------- CPU tests
_PER_GEOM = [next(c for c in ALL_CASES if c.geom == g) for g in GEOMS]


@pytest.mark.parametrize("c", _PER_GEOM, ids=_ids(_PER_GEOM))
def test_conv_reference_equals_torch_conv2d_float64(c):
    """The im2col matrix from slices, the same by address, and ``conv2d`` (bottom / right padding
    as the output size implies) give one accumulator."""
    d = _data(c)
    N, OH, OW, M, Kd, nk0 = _geom(c)
    X = _matrix(c, d)
    ref, k0 = 0, 0
    for s, x in zip(c.srcs, d["xs"]):
        (_, H, W, C), (KH, KW), (sh, sw), (ph, pw), (dh, dw) = s
        assert torch.equal(_gather(s, x, c.ohw), _im2col(s, x, c.ohw))
        wk = d["w"][:, k0:k0 + KH * KW * C].reshape(c.Cout, KH, KW, C).permute(0, 3, 1, 2)
        k0 += KH * KW * C
        pb = max(0, (OH - 1) * sh + (KH - 1) * dh + 1 - H - ph)
        pr = max(0, (OW - 1) * sw + (KW - 1) * dw + 1 - W - pw)
        xn = torch.nn.functional.pad(x.permute(0, 3, 1, 2), (pw, pr, ph, pb))
        ref = ref + torch.nn.functional.conv2d(xn, wk, stride=(sh, sw), dilation=(dh, dw))[:, :, :OH, :OW]
    ref = ref.permute(0, 2, 3, 1).reshape(M, c.Cout)
    assert X.shape == (M, Kd) and k0 == Kd and torch.equal(X @ d["w"].t(), ref)


@pytest.mark.parametrize("c", ALL_CASES, ids=_ids(ALL_CASES))
def test_reference_equals_host_path_where_it_does_not_round(c):
    """``ConvPP`` on host tensors computes in fp32 (exact here); into an fp32 ``out`` it rounds nowhere."""
    d = _data(c)
    N, OH, OW, M, Kd, nk0 = _geom(c)
    f = lambda v: None if v is None else v.to(F32)   # noqa: E731
    cp = K.ConvPP([tuple(s) for s in c.srcs], c.Cout, c.ohw, "cpu")
    out = torch.full((N, OH, OW, c.Cout), SENT, dtype=F32)
    res = None if d["res"] is None else f(d["res"]).reshape(N, OH, OW, c.Cout)
    cp([f(x) for x in d["xs"]], f(d["w"]), f(d["bias"]), res, c.act, out=out)
    assert torch.equal(out.reshape(M, c.Cout).to(F64), _ref(c).exact)


def test_host_path_into_a_strided_bf16_out_rounds_once():
    """The host path writes ``out=`` windows like the kernel but rounds once: with a residual it
    equals the ``round_once`` variant, not the reference."""
    for c in (next(c for c in ALL_CASES if c.res and len(c.srcs) == 1 and c.srcs[0].k == (3, 3)),
              next(c for c in ALL_CASES if c.res and len(c.srcs) == 2), next(c for c in ALL_CASES if not c.res)):
        want = (_reference(c, "round_once") if c.res else _ref(c)).out.to(BF)
        _check_window(_launch(c, torch.device("cpu"), raw=False), c, want, c.name)


@pytest.mark.parametrize("c", ALL_CASES, ids=_ids(ALL_CASES))
def test_data_make_the_properties_observable(c):
    """Conditions on the data (not measurements): the bound; ReLU zeroes >= 5 % and passes >= 5 %;
    each rounding changes some value; with a residual the first rounding changes the final result
    of some element (else ``round_once`` could not be told apart)."""
    r = _ref(c)
    print(f"{c.name}: peak {r.peak:.0f} " + " ".join(f"{k} {v:.3f}" for k, v in r.shares.items()))
    assert r.peak < EXACT
    assert _unobservable(c, r.shares) == []
    assert torch.equal(r.out.to(BF).to(F64), r.out) and torch.equal(r.exact.to(F32).to(F64), r.exact)
    d = _data(c)
    for v in (*d["xs"], d["w"], d["res"]):
        assert v is None or (torch.equal(v.to(BF).to(F64), v) and not bool((v.signbit() & (v == 0)).any()))
    b = d["bias"]
    assert b is None or (bool((b < 0).any()) and bool((b > 0).any()) and torch.equal(b * 2, (b * 2).round()))


@pytest.mark.parametrize("fault", FAULTS)
def test_wrong_variants_differ(fault):
    hit = 0
    for c in ALL_CASES:
        if _applies(fault, c):
            assert not torch.equal(_reference(c, fault).out, _ref(c).out), f"{fault} goes unnoticed on {c.name}"
            hit += 1
    assert hit >= 1, f"{fault} applies to no case"


def test_case_list_covers_every_path():
    G = {g: _geom(next(c for c in ALL_CASES if c.geom == g)) for g in GEOMS}     # (N, OH, OW, M, K, nk0)
    S = {g: v[0] for g, v in GEOMS.items()}
    cout = {g: v[1] for g, v in GEOMS.items()}
    tiles = {g: -(-G[g][3] // BT) * -(-cout[g] // BT) for g in GEOMS}
    single = [g for g in GEOMS if len(S[g]) == 1]
    dual = [g for g in GEOMS if len(S[g]) == 2]
    assert any(G[g][4] == 64 and cout[g] == 8 and G[g][3] < BT for g in single)                 # prologue only
    assert any(tiles[g] == 4 and G[g][3] % BT and cout[g] % BT and G[g][4] // 64 % 2 == 1
               and _straddles(next(c for c in ALL_CASES if c.geom == g)) for g in single)
    assert any(S[g][0].shape[3] == 128 and S[g][0].st == (2, 2) and S[g][0].pad == (0, 0) and G[g][4] // 64 % 2 == 0
               and S[g][0].shape[1] % 2 == 0 and S[g][0].shape[2] % 2 == 0
               and (G[g][1] - 1) * 2 + 3 > S[g][0].shape[1] and (G[g][2] - 1) * 2 + 3 > S[g][0].shape[2] for g in single)
    assert any(S[g][0].st[0] != S[g][0].st[1] and S[g][0].pad[0] != S[g][0].pad[1] for g in single)
    assert {S[g][0].k for g in single} >= {(1, 7), (7, 1), (5, 5), (3, 3), (1, 1)}
    assert any(S[g][0].dil == (2, 2) and S[g][0].k == (5, 5) for g in single)
    assert any(S[g][0].dil[0] != S[g][0].dil[1] for g in single)
    assert {tiles[g] for g in single} >= {9, 12} and max(tiles.values()) <= 12 and max(v[4] for v in G.values()) <= 1600
    assert any(G[g][5] == 1 and G[g][4] == 128 for g in dual)                                   # minimal dual
    assert any(S[g][1].shape[1] % 2 == 1 and S[g][1].st == (2, 2) and S[g][1].shape[3] == 128 for g in dual)
    assert any(S[g][1].st[0] != S[g][1].st[1] for g in dual)
    assert any(S[g][0].k == (3, 3) and S[g][0].pad == (1, 1) for g in dual)
    every = set(itertools.product((True, False), (True, False), (None, "relu")))
    for n in (1, 2):
        assert {(c.bias, c.res, c.act) for c in ALL_CASES if len(c.srcs) == n} == every
    for g in GEOMS:
        mine = [c for c in ALL_CASES if c.geom == g]
        assert {c.bias for c in mine} == {c.res for c in mine} == {True, False} and {c.act for c in mine} == {None, "relu"}
    assert sum(c.coff != 0 for c in ALL_CASES) * 2 >= len(ALL_CASES)


# --------------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("c", ALL_CASES, ids=_ids(ALL_CASES))
def test_conv_lite_gpu(c):
    dev = torch.device("cuda", 0)
    want = _ref(c).out.to(BF)
    N, OH, OW, M, Kd, nk0 = _geom(c)
    what = f"{c.name} ({-(-M // BT)} x {-(-c.Cout // BT)} tiles, {Kd // 64} K-tiles)"
    _check_window(_launch(c, dev, raw=False), c, want, what + " ConvPP")
    if c.res:
        _check_window(_launch(c, dev, raw=True), c, want, what + f" raw entry, ldr = Cout + {RPAD}")


# ----------------------------------------------------------------- host-side argument checks
_RAW_ARGS = ("srcs", "w", "bias", "res", "y", "N", "OH", "OW", "Cout", "ldy", "y_coff", "ldr", "act", "stream")
_SRC_ARGS = ("x", "N", "H", "W", "C", "KH", "KW", "sh", "sw", "ph", "pw", "dh", "dw")
# every ``need(...)`` of ``conv_pp`` and its activation check: the arguments changed from the good
# dual launch (a 3x3 padded source 0 and a stride-2 shortcut).  s0 / s1 = changes of a source's
# tuple; "+n" = that pointer moved by n bytes; "res" = the residual pointer is passed.
BAD_RAW = {
    "no-source": dict(srcs=0), "three-sources": dict(srcs=3), "short-tuple": dict(srcs="short"),
    "batch-s0": dict(s0=dict(N=2)), "batch-s1": dict(s1=dict(N=2)),
    "C%64-s0": dict(s0=dict(C=72)), "C%64-s1": dict(s1=dict(C=32)),
    "x+2-s0": dict(s0=dict(x="+2")), "x+8-s1": dict(s1=dict(x="+8")),
    "input-2GiB": dict(s0=dict(H=4096, W=4096)),
    "H-16384": dict(s0=dict(H=16384)), "W-16384": dict(s0=dict(W=16384)), "ph-1024": dict(s0=dict(ph=1024)),
    "pw-1024": dict(s0=dict(pw=1024)),
    "field-h": dict(s0=dict(dh=512)), "field-w": dict(s0=dict(dw=512)),
    "second-3x1": dict(s1=dict(KH=3)), "second-1x3": dict(s1=dict(KW=3)), "second-ph": dict(s1=dict(ph=1)),
    "second-pw": dict(s1=dict(pw=1)), "second-short-H": dict(s1=dict(H=6)), "second-short-W": dict(s1=dict(W=6)),
    "Cout%8": dict(Cout=12), "ldy%8": dict(ldy=44), "y_coff%8": dict(y_coff=4), "ldr%8": dict(res="res", ldr=12),
    "w+2": dict(w="+2"), "y+2": dict(y="+2"), "bias+4": dict(bias="+4"), "res+2": dict(res="res+2"),
    "weights-2GiB": dict(Cout=1 << 21, ldy=(1 << 21) + 8),
    "act-relu6": dict(act=K.ACT_RELU6), "act-gelu": dict(act=K.ACT_GELU), "act-drelu": dict(act=K.ACT_DRELU),
}
_RAW_REASON = {"source": "one or two sources", "tuple": "source tuple", "batch": "batch", "C%64": "multiple of 64",
               "x+": "x alignment", "input-2GiB": "input larger", "-16384": "spatial size", "-1024": "spatial size",
               "field": "receptive field", "second-short": "smaller than the output grid", "second": "must be 1x1",
               "ldr": "ldr alignment", "%8": "multiples of 8", "+": "alignment", "weights": "weights larger",
               "act": "unsupported activation"}


@functools.lru_cache(maxsize=None)
def _arg_env():
    """Buffers far larger than the 1 x 4 x 4 problem needs, y filled with the sentinel."""
    dev = torch.device("cuda", 0)
    env = {k: torch.zeros(1 << 17, dtype=BF, device=dev) for k in ("x0", "x1", "w", "res")}
    env["bias"] = torch.zeros(1 << 12, dtype=F32, device=dev)
    env["y"] = torch.full((1 << 16,), SENT, dtype=BF, device=dev)
    return env


def _raw_call(changes):
    ptr = {k: t.data_ptr() for k, t in _arg_env().items()}
    s = [dict(x=ptr["x0"], N=1, H=4, W=4, C=64, KH=3, KW=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1),
         dict(x=ptr["x1"], N=1, H=7, W=7, C=64, KH=1, KW=1, sh=2, sw=2, ph=0, pw=0, dh=1, dw=1)]
    a = dict(w=ptr["w"], bias=ptr["bias"], res=0, y=ptr["y"], N=1, OH=4, OW=4, Cout=8, ldy=16, y_coff=8, ldr=8,
             act=K.ACT_RELU, stream=K._stream())
    for k, v in changes.items():
        if k in ("s0", "s1"):
            for kk, vv in v.items():
                s[int(k[1])][kk] = s[int(k[1])][kk] + int(vv) if isinstance(vv, str) else vv
        elif isinstance(v, str) and k != "srcs":
            name, _, off = v.partition("+")
            a[k] = ptr[name or k] + int(off or 0)
        elif k != "srcs":
            a[k] = v
    tup = [tuple(t[k] for k in _SRC_ARGS) for t in s]
    a["srcs"] = {None: tup, 0: [], 3: tup + tup[1:], "short": [tup[0][:12], tup[1]]}[changes.get("srcs")]
    K._hip().conv_pp(*[a[k] for k in _RAW_ARGS])


def _bad_launches(dev):
    """(good plan and call arguments of ``ConvPP``, [(what, plan overrides, call overrides)]) for every
    refusal of the wrapper."""
    z = lambda *s, dtype=BF, device=dev: torch.zeros(s, dtype=dtype, device=device)   # noqa: E731
    cpu = torch.device("cpu")
    s0, s1 = ((1, 4, 4, 64), (3, 3), (1, 1), (1, 1), (1, 1)), ((1, 7, 7, 64), (1, 1), (2, 2), (0, 0), (1, 1))
    plan = dict(srcs=[s0, s1], Cout=8, out_hw=(4, 4), device=dev)
    call = dict(xs=[z(1, 4, 4, 64), z(1, 7, 7, 64)], w=z(8, 640), bias=z(8, dtype=F32), residual=z(1, 4, 4, 8), act="relu",
                out=z(1, 4, 4, 24), out_channel_offset=8)
    s1_ = lambda **kw: [s0, tuple(kw.get(k, v) for k, v in zip(("shape", "k", "st", "pad", "dil"), s1))]   # noqa: E731
    bad = [("tile argument", dict(tile=0), {}), ("splits argument", dict(splits=2), {}),
           ("C % 64", dict(srcs=[((1, 4, 4, 72), *s0[1:]), s1]), {}), ("batches differ", dict(srcs=s1_(shape=(2, 7, 7, 64))), {}),
           ("Cout % 8", dict(Cout=12), {}), ("second 3x3", dict(srcs=s1_(k=(3, 3))), {}),
           ("second padded", dict(srcs=s1_(pad=(1, 1))), {}), ("second short H", dict(srcs=s1_(shape=(1, 6, 7, 64))), {}),
           ("second short W", dict(srcs=s1_(shape=(1, 7, 6, 64))), {}),
           ("source count", {}, dict(xs=[z(1, 4, 4, 64)])), ("input shape", {}, dict(xs=[z(1, 4, 4, 64), z(1, 7, 8, 64)])),
           ("a larger batch than planned", {}, dict(xs=[z(2, 4, 4, 64), z(2, 7, 7, 64)], out=z(2, 4, 4, 24),
                                                   residual=z(2, 4, 4, 8))),
           ("out pixels", {}, dict(out=z(1, 4, 5, 24))), ("window past the row", {}, dict(out_channel_offset=24)),
           ("weight shape", {}, dict(w=z(8, 576))), ("unknown activation", {}, dict(act="swish"))]
    if dev.type == "cuda":
        bad += [("x dtype", {}, dict(xs=[z(1, 4, 4, 64, dtype=F32), z(1, 7, 7, 64)])),
                ("x1 device", {}, dict(xs=[z(1, 4, 4, 64), z(1, 7, 7, 64, device=cpu)])),
                ("x not contiguous", {}, dict(xs=[z(1, 4, 4, 128)[..., ::2], z(1, 7, 7, 64)])),
                ("w dtype", {}, dict(w=z(8, 640, dtype=F32))), ("w device", {}, dict(w=z(8, 640, device=cpu))),
                ("out dtype", {}, dict(out=z(1, 4, 4, 24, dtype=F32))), ("out not contiguous", {}, dict(out=z(1, 4, 4, 48)[..., ::2])),
                ("bias dtype", {}, dict(bias=z(8))), ("bias device", {}, dict(bias=z(8, dtype=F32, device=cpu))),
                ("residual dtype", {}, dict(residual=z(1, 4, 4, 8, dtype=F32))),
                ("residual device", {}, dict(residual=z(1, 4, 4, 8, device=cpu))),
                ("residual size", {}, dict(residual=z(1, 4, 4, 16))), ("ldy % 8", {}, dict(out=z(1, 4, 4, 28))),
                ("w not contiguous", {}, dict(w=z(8, 1280)[:, ::2])), ("bias not contiguous", {}, dict(bias=z(16, dtype=F32)[::2])),
                ("residual not contiguous", {}, dict(residual=z(1, 4, 4, 16)[..., ::2])),
                ("offset % 8", {}, dict(out_channel_offset=4)), ("relu6", {}, dict(act="relu6")), ("gelu", {}, dict(act="gelu"))]
    return plan, call, bad


def _assert_wrapper_refusals(dev):
    plan, call, bad = _bad_launches(dev)
    call["out"].fill_(SENT)
    for what, p, a in bad:
        with pytest.raises((ValueError, TypeError)):
            K.ConvPP(**{**plan, **p})(**{**call, **a})
            pytest.fail(f"not refused: {what}")
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert bool((call["out"] == SENT).all()), "a refused launch wrote the output"
    K.ConvPP(**plan)(**call)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert bool((call["out"][..., 8:16] == 0).all()) and bool((call["out"][..., :8] == SENT).all())


def test_wrapper_refusals_that_need_no_gpu():
    _assert_wrapper_refusals(torch.device("cpu"))


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch_gpu():
    """Every ``need(...)`` of ``conv_pp`` and every ``ValueError`` / ``TypeError`` of ``ConvPP`` is raised by
    a launch that differs from an accepted one in that respect alone; nothing is written."""
    y = _arg_env()["y"]
    _raw_call({})
    _raw_call(dict(res="res"))
    torch.cuda.synchronize()
    got = y.cpu()
    y.fill_(SENT)
    assert bool((got[:16 * 16].reshape(16, 16)[:, 8:] == 0).all()) and bool((got[16 * 16:] == SENT).all())
    for what, changes in BAD_RAW.items():
        reason = next(msg for key, msg in _RAW_REASON.items() if key in what)
        with pytest.raises(ValueError, match=reason):
            _raw_call(changes)
            pytest.fail(f"not refused: {what}")
    torch.cuda.synchronize()
    assert bool((y == SENT).all()), "a refused raw launch wrote the output"
    _assert_wrapper_refusals(torch.device("cuda", 0))
