"""Video models: the interpreter ops ``Conv3D`` / ``MaxPool3D`` / ``AvgPool3D``, the kernels of
``kernels/conv3d.hip``, their weight packing and launchers, the lowering and the C3D model.

The definition (``graph/ops_nn.py:conv3d_tf``) has two independent anchors: ``torch``'s ``conv3d``
on an explicitly padded NCDHW copy, and a float64 mirror written here from the formula, one
filter tap and one output plane at a time: ``y[n, od, oh, ow, co] += x[n, od sd + kd - pf, oh sh +
kh - pt, ow sw + kw - pl, ci] w[kd, kh, kw, ci, co]`` wherever the input index is inside ``x`` on
all three axes.  On integer data all three agree exactly.  ``pool3d_tf`` has a mirror of its own.

The mirror has three deliberately wrong variants: out-of-range taps clamped to the edge instead
of dropped, SAME's extra pad in front instead of behind, and the taps walked in (kh, kd, kw)
order against weights laid out in (kd, kh, kw) order.  Each differs from the truth exactly on the
geometries where it can: some tap outside the input, an odd total pad on some axis, ``KD > 1`` and
``KH > 1``.

Exact data.  x, w are small integers and the bias halves, sized per activation (sparse for ReLU6,
so that the sums stay near [0, 6]); the mirror asserts ``sum |x| |w| + |b| < 2^22`` per output, so
fp32 accumulation is exact in any order and the only rounding is the kernel's final ``f2bf``.  The
largest case, 7x7x7 over 72 channels, is bounded by 24,696 x 32, about 7.9e5.  Kernel outputs are
compared on their bf16 bit patterns.

Device tests put x, the packed weights and the bias between NaN bands and write a channel slice
of a wider buffer filled with the sentinel 2^100, itself between bands, as ``tests/test_deconv.py``
does.

Plans.  Outputs within 0.05 of the fp32 interpreter relative to its maximum
(``tests/test_deconv.py:_check_logits``)."""
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from flink_tensorflow_amd.graph.builder import GraphBuilder
from flink_tensorflow_amd.graph.compiler import CompiledFunction, CompileError
from flink_tensorflow_amd.graph.graph import Graph
from flink_tensorflow_amd.graph.ops_nn import conv3d_tf, pool3d_tf, same_pads
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.ops import kernels as K

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 2.0 ** 100
ACTS = ("none", "relu", "relu6")

# (N, D, H, W, Cin, Cout)
SHAPES = ((1, 3, 5, 7, 8, 8), (2, 4, 6, 5, 72, 136), (3, 3, 9, 9, 16, 64))
# name -> ((KD, KH, KW), (sd, sh, sw), padding)
GEOMS = {
    "3x3x3s1-same": ((3, 3, 3), (1, 1, 1), "SAME"),
    "3x3x3s1-valid": ((3, 3, 3), (1, 1, 1), "VALID"),
    "3x3x3s2-same": ((3, 3, 3), (2, 2, 2), "SAME"),       # asymmetric pads on the even extents
    "1x3x3s122-same": ((1, 3, 3), (1, 2, 2), "SAME"),
    "3x1x1s211-same": ((3, 1, 1), (2, 1, 1), "SAME"),
    "2x2x2s2-valid": ((2, 2, 2), (2, 2, 2), "VALID"),
    "1x1x1s1": ((1, 1, 1), (1, 1, 1), "VALID"),
    "5x3x2s121-same": ((5, 3, 2), (1, 2, 1), "SAME"),
    "7x7x7s2-same": ((7, 7, 7), (2, 2, 2), "SAME"),       # most taps outside the input
}
CASES = [(s, g) for g in GEOMS for s in SHAPES]


def _case_id(c):
    (N, D, H, W, Ci, Co), g = c
    return f"{g}-{N}x{D}x{H}x{W}x{Ci}x{Co}"


def _geo(geom, ext, front=False):
    """(k, s, pads (front, back, top, bottom, left, right), (Do, Ho, Wo)); ``front``: SAME's extra
    pad in front (the wrong variant)."""
    k, s, padding = GEOMS[geom]
    pads, out = [], []
    for i in range(3):
        lo, hi = same_pads(ext[i], k[i], s[i]) if padding == "SAME" else (0, 0)
        pads += [hi, lo] if front else [lo, hi]
        out.append(-(-ext[i] // s[i]) if padding == "SAME" else (ext[i] - k[i]) // s[i] + 1)
    return k, s, tuple(pads), tuple(out)


def _has_outside_tap(geom, ext):
    """Some (output index, tap) pair of the definition lands outside the input."""
    k, s, pads, out = _geo(geom, ext)
    return any(not 0 <= o * s[a] + t - pads[2 * a] < ext[a] for a in range(3) for o in range(out[a]) for t in range(k[a]))


def _has_odd_pad(geom, ext):
    pads = _geo(geom, ext)[2]
    return any(pads[2 * a] != pads[2 * a + 1] for a in range(3))


# =================================================================================== the mirror
def _axis_taps(O, I, t, s, p, clamp):
    """(output indices, input indices) of filter tap t along one axis"""
    oi = []
    for o in range(O):
        i = o * s + t - p
        if 0 <= i < I:
            oi.append((o, i))
        elif clamp:
            oi.append((o, min(max(i, 0), I - 1)))
    if not oi:
        return None
    return tuple(torch.tensor(v) for v in zip(*oi))


def _mirror_pre(x, w, geom, clamp=False, front=False, swapped=False):
    """float64 ``conv3d(x, w)`` from the definition, one filter tap and one output plane at a
    time.  ``clamp`` / ``front`` / ``swapped``: the deliberately wrong variants."""
    N, D, H, W, Cin = x.shape
    k, s, pads, out = _geo(geom, (D, H, W), front)
    Cout = w.shape[4]
    y = torch.zeros((N, *out, Cout), dtype=F64)
    order = [(a, b, c) for a in range(k[0]) for b in range(k[1]) for c in range(k[2])]
    wrong = [(a, b, c) for b in range(k[1]) for a in range(k[0]) for c in range(k[2])]
    for t, (kd, kh, kw) in enumerate(order):
        wt = w[wrong[t]] if swapped else w[kd, kh, kw]           # [Cin, Cout]
        ax = [_axis_taps(out[a], (D, H, W)[a], (kd, kh, kw)[a], s[a], pads[2 * a], clamp) for a in range(3)]
        if any(v is None for v in ax):
            continue
        (od, idd), (oh, ih), (ow, iw) = ax
        for j in range(len(od)):                                 # one output plane at a time
            y[:, od[j], oh[:, None], ow[None, :]] += x[:, idd[j], ih[:, None], iw[None, :]] @ wt
    return y


def _act(v, act):
    if act == "relu":
        return torch.relu(v)
    if act == "relu6":
        return torch.clamp(v, 0, 6)
    return v


def _mean_taps(shape, geom):
    """Mean number of in-image taps per output pixel."""
    ext = shape[1:4]
    k, s, pads, out = _geo(geom, ext)
    m = 1.0
    for a in range(3):
        inside = sum(0 <= o * s[a] + t - pads[2 * a] < ext[a] for o in range(out[a]) for t in range(k[a]))
        m *= inside / out[a]
    return m


@functools.lru_cache(maxsize=None)
def _data(shape, geom, small, bias):
    """(x, w [KD, KH, KW, Cin, Cout], bias or None) as float64 integers / half-integers.  ``small``
    (ReLU6): x in {0, 1} with a density that puts the sums around [0, 6], w in [-1, 2], bias halves
    spread over [-6, 8.5]; otherwise x in [-8, 8], w in [-4, 4], bias halves in [-600, 600] with
    alternating signs."""
    N, D, H, W, Cin, Cout = shape
    k = GEOMS[geom][0]
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, geom, small, bias)).encode()))
    if small:
        kmax = Cin * _mean_taps(shape, geom)
        dens = min(1.0, (4.0 if bias else 10.0) / kmax)
        x = (torch.rand((N, D, H, W, Cin), generator=g) < dens).to(F64)
        w = torch.randint(-1, 3, (*k, Cin, Cout), generator=g).to(F64)
        b = ((torch.arange(Cout) % 8) * 2 - 6 + torch.randint(0, 2, (Cout,), generator=g) / 2).to(F64) if bias else None
    else:
        x = torch.randint(-8, 9, (N, D, H, W, Cin), generator=g).to(F64)
        w = torch.randint(-4, 5, (*k, Cin, Cout), generator=g).to(F64)
        b = torch.randint(1, 1201, (Cout,), generator=g).to(F64) / 2 if bias else None
        if bias:
            b[1::2] *= -1        # both signs whatever the draw: few channels must not all clip at 0
    return x, w, b


@functools.lru_cache(maxsize=None)
def _pre(shape, geom, small, bias):
    """The mirror's ``conv3d + bias`` in float64; asserts that fp32 accumulation is exact."""
    x, w, b = _data(shape, geom, small, bias)
    bound = _mirror_pre(x.abs(), w.abs(), geom) + (b.abs() if b is not None else 0)
    assert bound.max() < 2 ** 22
    y = _mirror_pre(x, w, geom)
    return y + b if b is not None else y


def _ref(shape, geom, act, bias):
    """(float64 result, its single bf16 rounding)"""
    y = _act(_pre(shape, geom, act == "relu6", bias), act)
    return y, y.to(F32).to(BF)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _pool_mirror(x, k, s, pads, mode):
    """3-D pooling from the definition: per output element the window elements inside ``x``; the
    average sums in float64 and divides in fp32."""
    N, D, H, W, C = x.shape
    out = tuple((e + pads[2 * a] + pads[2 * a + 1] - k[a]) // s[a] + 1 for a, e in enumerate((D, H, W)))
    y = torch.zeros((N, *out, C), dtype=F32 if mode == "avg" else x.dtype)
    for od in range(out[0]):
        d0, d1 = max(od * s[0] - pads[0], 0), min(od * s[0] - pads[0] + k[0], D)
        for oh in range(out[1]):
            h0, h1 = max(oh * s[1] - pads[2], 0), min(oh * s[1] - pads[2] + k[1], H)
            for ow in range(out[2]):
                w0, w1 = max(ow * s[2] - pads[4], 0), min(ow * s[2] - pads[4] + k[2], W)
                win = x[:, d0:d1, h0:h1, w0:w1].reshape(N, -1, C)
                if mode == "max":
                    y[:, od, oh, ow] = win.max(1).values
                else:
                    y[:, od, oh, ow] = win.to(F64).sum(1).to(F32) / torch.tensor(float(win.shape[1]), dtype=F32)
    return y


# name -> (ksize, strides, padding, (D, H, W) or None for the default extents)
POOLS = {
    "1x2x2s122-valid": ((1, 2, 2), (1, 2, 2), "VALID", None),
    "2x2x2s2-valid": ((2, 2, 2), (2, 2, 2), "VALID", None),
    "2x2x2s2-same-odd": ((2, 2, 2), (2, 2, 2), "SAME", None),
    "3x3x3s2-same": ((3, 3, 3), (2, 2, 2), "SAME", None),
    "3x3x3s1-same": ((3, 3, 3), (1, 1, 1), "SAME", None),
    "2x7x7s1-valid": ((2, 7, 7), (1, 1, 1), "VALID", (2, 7, 7)),
}
POOL_EXT = (3, 5, 7)      # odd on every axis
POOL_N = 2


def _pool_geo(name):
    k, s, padding, ext = POOLS[name]
    ext = ext or POOL_EXT
    pads = tuple(p for a in range(3) for p in (same_pads(ext[a], k[a], s[a]) if padding == "SAME" else (0, 0)))
    return k, s, padding, ext, pads, (1 if ext != POOL_EXT else POOL_N)


def _pool_data(name, C, mode):
    """Integers: [-100, -1] for max (a zero leaking in from padding would win), [-100, 100] for avg."""
    ext, n = _pool_geo(name)[3], _pool_geo(name)[5]
    g = torch.Generator().manual_seed(zlib.crc32(repr((name, C, mode)).encode()))
    return torch.randint(-100, 0 if mode == "max" else 101, (n, *ext, C), generator=g).to(F32)


# =================================================================================== CPU: the definition
ANCHOR_SHAPE = (2, 4, 5, 7, 8, 16)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_definition_has_two_anchors(geom):
    x, w, _ = _data(ANCHOR_SHAPE, geom, False, False)
    N, D, H, W, Cin, Cout = ANCHOR_SHAPE
    k, s, pads, out = _geo(geom, (D, H, W))
    y = conv3d_tf(x, w, s, GEOMS[geom][2])
    assert y.dtype == F64 and y.shape == (N, *out, Cout)
    # anchor 1: torch's conv3d on an explicitly padded NCDHW copy
    xn = F.pad(x.permute(0, 4, 1, 2, 3), (pads[4], pads[5], pads[2], pads[3], pads[0], pads[1]))
    t = F.conv3d(xn, w.permute(4, 3, 0, 1, 2), stride=s).permute(0, 2, 3, 4, 1)
    assert torch.equal(y, t)
    # anchor 2: the mirror
    m = _mirror_pre(x, w, geom)
    assert torch.equal(y, m)
    # the wrong variants are caught wherever they can differ
    outside = _has_outside_tap(geom, (D, H, W))
    if GEOMS[geom][2] == "VALID":
        assert not outside
    if geom in ("3x3x3s1-same", "7x7x7s2-same", "5x3x2s121-same"):
        assert outside
    assert torch.equal(_mirror_pre(x, w, geom, clamp=True), m) != outside
    assert torch.equal(_mirror_pre(x, w, geom, front=True), m) != _has_odd_pad(geom, (D, H, W))
    assert torch.equal(_mirror_pre(x, w, geom, swapped=True), m) != (k[0] > 1 and k[1] > 1)
    # float32 inputs stay float32
    assert conv3d_tf(x.float(), w.float(), s, GEOMS[geom][2]).dtype == F32


def test_wrong_mirrors_have_ground_on_the_cases():
    """Each wrong variant has geometries among the test cases on which it can differ."""
    for shape in SHAPES:
        ext = shape[1:4]
        assert any(_has_outside_tap(g, ext) for g in GEOMS) and any(_has_odd_pad(g, ext) for g in GEOMS)
        assert _has_odd_pad("3x3x3s2-same", ext) == any(e % 2 == 0 for e in ext)


@pytest.mark.parametrize("name", list(POOLS))
def test_pool_definition(name):
    k, s, padding, ext, pads, _ = _pool_geo(name)
    for mode in ("max", "avg"):
        x = _pool_data(name, 8, mode)
        y = pool3d_tf(x.double(), k, s, padding, mode)
        m = _pool_mirror(x, k, s, pads, mode)
        assert y.shape == m.shape
        if mode == "max":
            assert torch.equal(y, m.double())
        else:
            torch.testing.assert_close(y, m.double(), rtol=1e-6, atol=1e-6)
        if all(pads[2 * a] == pads[2 * a + 1] for a in range(3)):       # symmetric pads: torch's own pools
            xn = x.double().permute(0, 4, 1, 2, 3)
            p = (pads[0], pads[2], pads[4])
            if all(2 * p[a] <= k[a] for a in range(3)):
                t = F.max_pool3d(xn, k, s, p) if mode == "max" else F.avg_pool3d(xn, k, s, p, count_include_pad=False)
                torch.testing.assert_close(y, t.permute(0, 2, 3, 4, 1), rtol=1e-12, atol=1e-12)


def test_definition_rejections():
    x, w = torch.zeros((1, 4, 4, 4, 8)), torch.zeros((3, 3, 3, 8, 8))
    conv3d_tf(x, w, (1, 1, 1), "SAME")
    with pytest.raises(ValueError, match="channels"):
        conv3d_tf(torch.zeros((1, 4, 4, 4, 16)), w, (1, 1, 1), "SAME")
    with pytest.raises(ValueError, match="empty"):
        conv3d_tf(torch.zeros((1, 2, 4, 4, 8)), w, (1, 1, 1), "VALID")
    gb = GraphBuilder()
    xin = gb.placeholder("x", "FLOAT", [None, 4, 4, 4, 8])
    gb.op("Conv3D", [xin, gb.constant("w", w.numpy())], name="bad", strides=[2, 1, 1, 1, 1], padding=b"SAME",
          data_format=b"NDHWC", dilations=[1, 1, 1, 1, 1])
    with pytest.raises(Exception, match="batch and channel"):
        Session(gb.build()).run(["bad:0"], {"x:0": x})
    with pytest.raises(ValueError, match="empty"):
        pool3d_tf(torch.zeros((1, 1, 4, 4, 8)), (2, 2, 2), (2, 2, 2), "VALID", "max")


def test_interpreter_op_and_builder():
    """NDHWC and NCDHW (by permuting), the pools, a 5-D inference batch norm, the builder's nodes."""
    x, w, _ = _data(ANCHOR_SHAPE, "3x3x3s2-same", False, False)
    ref = conv3d_tf(x.float(), w.float(), (2, 2, 2), "SAME")
    gb = GraphBuilder()
    xin = gb.placeholder("x", "FLOAT", [None, 4, 5, 7, 8])
    wc = gb.constant("w", w.float().numpy())
    y = gb.conv3d(xin, wc, (2, 2, 2), "SAME", name="c")
    xt = gb.transpose(xin, [0, 4, 1, 2, 3], name="ncdhw")
    gb.op("Conv3D", [xt, wc], name="cc", strides=[1, 1, 2, 2, 2], padding=b"SAME", data_format=b"NCDHW",
          dilations=[1, 1, 1, 1, 1])
    mp = gb.max_pool3d(xin, (2, 2, 2), (2, 2, 2), "SAME", name="mp")
    ap = gb.avg_pool3d(xin, (3, 3, 3), (1, 1, 1), "SAME", name="ap")
    rng = np.random.default_rng(0)
    vec = [gb.constant(n, rng.uniform(0.5, 1.5, 16).astype(np.float32)) for n in ("g", "b", "m", "v")]
    gb.fused_batch_norm(y, *vec, name="bn")
    g = gb.build()
    assert y == "c:0" and g["c"].op == "Conv3D" and g["mp"].op == "MaxPool3D" and g["ap"].op == "AvgPool3D"
    assert list(g["c"].attr("strides")) == [1, 2, 2, 2, 1] and list(g["mp"].attr("ksize")) == [1, 2, 2, 2, 1]
    a, c, p, q, bn = Session(g).run(["c:0", "cc:0", mp, ap, "bn:0"], {"x:0": x.float()})
    assert torch.equal(a, ref) and torch.equal(c.permute(0, 2, 3, 4, 1), ref)
    assert torch.equal(p, pool3d_tf(x.float(), (2, 2, 2), (2, 2, 2), "SAME", "max"))
    assert torch.equal(q, pool3d_tf(x.float(), (3, 3, 3), (1, 1, 1), "SAME", "avg"))
    consts = Session(g).run(["g:0", "b:0", "m:0", "v:0"], {})    # the 5-D inference batch norm, per channel
    inv = torch.rsqrt(consts[3] + 1e-3) * consts[0]
    torch.testing.assert_close(bn, ref * inv + (consts[1] - consts[2] * inv))


@pytest.mark.parametrize("geom", list(GEOMS))
def test_exact_data_covers_every_outcome(geom):
    for shape in SHAPES:
        for bias in (False, True):
            pre = _pre(shape, geom, False, bias)
            assert (pre <= 0).double().mean() >= 0.05 and (pre > 0).double().mean() >= 0.05, (shape, bias)
            if bias:   # the rounding to bf16 is observable
                y, yb = _ref(shape, geom, "none", True)
                assert (yb.double() != y).any(), shape
            p6 = _pre(shape, geom, True, bias)
            shares = [(p6 <= 0).double().mean(), ((p6 > 0) & (p6 < 6)).double().mean(), (p6 >= 6).double().mean()]
            assert min(shares) >= 0.05, (shape, bias, shares)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_wrong_mirrors_differ_on_the_cases(case):
    shape, geom = case
    x, w, _ = _data(shape, geom, False, False)
    ext, k = shape[1:4], GEOMS[geom][0]
    m = _pre(shape, geom, False, False)
    assert torch.equal(_mirror_pre(x, w, geom, clamp=True), m) != _has_outside_tap(geom, ext)
    assert torch.equal(_mirror_pre(x, w, geom, front=True), m) != _has_odd_pad(geom, ext)
    assert torch.equal(_mirror_pre(x, w, geom, swapped=True), m) != (k[0] > 1 and k[1] > 1)


# =================================================================================== CPU: packing, launchers
@pytest.mark.parametrize("geom", list(GEOMS))
def test_pack_weights(geom):
    shape = SHAPES[1]
    _, w, _ = _data(shape, geom, False, False)
    k = GEOMS[geom][0]
    Cin, Cout = w.shape[3:]
    wp = K.conv3d_pack_weights(w)
    assert wp.shape == (Cout, k[0] * k[1] * k[2] * Cin) and wp.dtype == w.dtype and wp.is_contiguous()
    assert torch.equal(K.conv3d_unpack_weights(wp, k, Cin), w)
    # row co: the taps' Cin-vectors of output channel co, back to back in (kd, kh, kw) order
    row = torch.cat([w[a, b, c, :, 5] for a in range(k[0]) for b in range(k[1]) for c in range(k[2])])
    assert torch.equal(wp[5], row)


def test_eligible_is_pure_and_matches_the_launchers():
    ok = K.conv3d_eligible
    assert ok(8, 8, (1, 1, 1), (1, 1, 1)) and ok(264, 136, (7, 7, 7), (4, 4, 4)) and ok(16, 24, (5, 3, 2), (1, 2, 1))
    assert not ok(12, 8, (3, 3, 3), (1, 1, 1)) and not ok(8, 12, (3, 3, 3), (1, 1, 1)) and not ok(0, 8, (3, 3, 3), (1, 1, 1))
    assert not ok(8, 8, (8, 3, 3), (1, 1, 1)) and not ok(8, 8, (3, 3, 0), (1, 1, 1)) and not ok(8, 8, (3, 3), (1, 1, 1))
    assert not ok(8, 8, (3, 3, 3), (5, 1, 1)) and not ok(8, 8, (3, 3, 3), (1, 0, 1))
    assert not ok(8, 8, (3, 3, 3), (1, 1, 1), (1, 2, 1)) and ok(8, 8, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    for Cin, Cout, k, st in ((12, 8, (3, 3, 3), (1, 1, 1)), (8, 12, (3, 3, 3), (1, 1, 1)), (8, 8, (8, 3, 3), (1, 1, 1)),
                             (8, 8, (3, 3, 3), (5, 1, 1)), (8, 8, (3, 3, 3), (2, 2, 2)), (16, 8, (7, 1, 2), (4, 1, 3))):
        x = torch.zeros((1, 9, 9, 9, Cin))
        wp = torch.zeros((Cout, k[0] * k[1] * k[2] * Cin))
        if K.conv3d_eligible(Cin, Cout, k, st):
            K.conv3d_ndhwc(x, wp, None, k, st)
        else:
            with pytest.raises(ValueError):
                K.conv3d_ndhwc(x, wp, None, k, st)
    pk = K.pool3d_eligible
    assert pk(8, (1, 1, 1), (1, 1, 1)) and pk(24, (8, 8, 8), (8, 8, 8)) and pk(16, (2, 7, 7), (1, 1, 1))
    assert not pk(12, (2, 2, 2), (2, 2, 2)) and not pk(8, (9, 2, 2), (2, 2, 2)) and not pk(8, (2, 2, 2), (2, 9, 2))
    assert not pk(8, (2, 2), (2, 2, 2)) and not pk(8, (2, 0, 2), (2, 2, 2)) and not pk(0, (2, 2, 2), (2, 2, 2))
    for C, k, st in ((12, (2, 2, 2), (2, 2, 2)), (8, (9, 2, 2), (2, 2, 2)), (8, (2, 2, 2), (2, 9, 2)), (8, (2, 2, 2), (2, 2, 2))):
        x = torch.zeros((1, 9, 9, 9, C))
        if K.pool3d_eligible(C, k, st):
            K.pool3d_ndhwc(x, k, st)
        else:
            with pytest.raises(ValueError):
                K.pool3d_ndhwc(x, k, st)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_host_path_equals_the_interpreter(case):
    shape, geom = case
    N, D, H, W, Cin, Cout = shape
    k, s, pads, out = _geo(geom, (D, H, W))
    for act in ACTS:
        for bias in (False, True):
            x, w, b = _data(shape, geom, act == "relu6", bias)
            ref = conv3d_tf(x.float(), w.float(), s, GEOMS[geom][2])
            ref = _act(ref + b.float() if bias else ref, act)
            wp = K.conv3d_pack_weights(w.float())
            bf = b.float() if bias else None
            y = K.conv3d_ndhwc(x.float(), wp, bf, k, s, pads, act)
            assert y.dtype == F32 and torch.equal(y, ref)
            assert torch.equal(y.double(), _ref(shape, geom, act, bias)[0])
    wide = torch.full((N, *out, Cout + 24), 7.0)
    assert K.conv3d_ndhwc(x.float(), wp, bf, k, s, pads, act, out=wide, out_channel_offset=16) is wide
    assert torch.equal(wide[..., 16:16 + Cout], ref)
    assert (wide[..., :16] == 7).all() and (wide[..., 16 + Cout:] == 7).all()


@pytest.mark.parametrize("name", list(POOLS))
def test_pool_host_path_equals_the_interpreter(name):
    k, s, padding, ext, pads, _ = _pool_geo(name)
    for mode in ("max", "avg"):
        x = _pool_data(name, 24, mode)
        ref = pool3d_tf(x, k, s, padding, mode)
        y = K.pool3d_ndhwc(x, k, s, pads, mode)
        assert y.dtype == F32 and y.shape == ref.shape
        torch.testing.assert_close(y, ref, rtol=1e-6, atol=1e-6)
        assert torch.equal(y, _pool_mirror(x, k, s, pads, mode))
        wide = torch.full((*ref.shape[:4], 24 + 24), 7.0)
        assert K.pool3d_ndhwc(x, k, s, pads, mode, out=wide, out_channel_offset=16) is wide
        assert torch.equal(wide[..., 16:40], y) and (wide[..., :16] == 7).all() and (wide[..., 40:] == 7).all()


def _bad_launches(dev):
    """(description, kwargs overriding a good launch) for every refusal of the conv launcher."""
    N, D, H, W, Cin, Cout = 1, 3, 4, 5, 16, 24
    dt = BF if dev.type == "cuda" else F32
    z = lambda *s, dtype=dt, device=dev: torch.zeros(s, dtype=dtype, device=device)   # noqa: E731
    good = dict(x=z(N, D, H, W, Cin), w_packed=z(Cout, 8 * Cin), bias=z(Cout, dtype=F32), kernel=(2, 2, 2),
                stride=(1, 2, 1), pad=(1, 0, 0, 0, 0, 1), act="relu", out=z(N, 3, 2, 5, 40), out_channel_offset=8)
    bad = [("x rank", dict(x=z(D, H, W, Cin))), ("weights length", dict(w_packed=z(Cout, 8 * Cin + 8))),
           ("weights rank", dict(w_packed=z(Cout * 8 * Cin))), ("Cin % 8", dict(x=z(N, D, H, W, 12), w_packed=z(Cout, 8 * 12))),
           ("Cout % 8", dict(w_packed=z(12, 8 * Cin), bias=z(12, dtype=F32), out=None)),
           ("filter above 7", dict(kernel=(8, 1, 1), pad=(0, 0, 0, 0, 0, 0), x=z(N, 9, H, W, Cin), out=None)),
           ("filter rank", dict(kernel=(2, 4))), ("stride above 4", dict(stride=(5, 2, 1))),
           ("stride 0", dict(stride=(0, 2, 1))), ("pad above the filter", dict(pad=(2, 0, 0, 0, 0, 1), out=None)),
           ("negative pad", dict(pad=(1, 0, -1, 0, 0, 1))), ("pad rank", dict(pad=(1, 0, 0, 1))),
           ("empty output", dict(x=z(N, D, 1, W, Cin), pad=(1, 0, 0, 0, 0, 1), out=None)),
           ("out too small", dict(out=z(N, 3, 2, 4, 40))), ("out batch", dict(out=z(2, 3, 2, 5, 40))),
           ("out rank", dict(out=z(3, 2, 5, 40))), ("slot past the row", dict(out_channel_offset=24)),
           ("negative offset", dict(out_channel_offset=-8)), ("bias length", dict(bias=z(16, dtype=F32))),
           ("activation", dict(act="sigmoid")), ("tile", dict(cfg=7))]
    if dev.type == "cuda":
        cpu = torch.device("cpu")
        bad += [("pitch % 8", dict(out=z(N, 3, 2, 5, 44))), ("offset % 8", dict(out_channel_offset=4)),
                ("x dtype", dict(x=z(N, D, H, W, Cin, dtype=F32))), ("w dtype", dict(w_packed=z(Cout, 8 * Cin, dtype=F32))),
                ("out dtype", dict(out=z(N, 3, 2, 5, 40, dtype=F32))), ("bias dtype", dict(bias=z(Cout))),
                ("w device", dict(w_packed=z(Cout, 8 * Cin, device=cpu))), ("bias device", dict(bias=z(Cout, dtype=F32, device=cpu))),
                ("out device", dict(out=z(N, 3, 2, 5, 40, device=cpu))),
                ("x not contiguous", dict(x=z(N, D, H, W, 2 * Cin)[..., ::2]))]
    return good, bad


def _bad_pools(dev):
    N, D, H, W, C = 1, 3, 4, 5, 16
    dt = BF if dev.type == "cuda" else F32
    z = lambda *s, dtype=dt, device=dev: torch.zeros(s, dtype=dtype, device=device)   # noqa: E731
    good = dict(x=z(N, D, H, W, C), ksize=(2, 2, 2), stride=(1, 2, 1), pad=(1, 0, 0, 0, 0, 1), mode="avg",
                out=z(N, 3, 2, 5, 40), out_channel_offset=8)
    bad = [("x rank", dict(x=z(D, H, W, C))), ("C % 8", dict(x=z(N, D, H, W, 12), out=None)),
           ("window above 8", dict(ksize=(9, 2, 2), x=z(N, 9, H, W, C), out=None)), ("window rank", dict(ksize=(2, 2))),
           ("stride above 8", dict(stride=(9, 2, 1))), ("stride 0", dict(stride=(1, 0, 1))),
           ("pad above the window", dict(pad=(2, 0, 0, 0, 0, 1), out=None)), ("negative pad", dict(pad=(1, 0, 0, -1, 0, 1))),
           ("a window outside", dict(pad=(1, 0, 0, 0, 0, 4), out=None)), ("empty output", dict(x=z(N, D, 1, W, C), out=None)),
           ("out too small", dict(out=z(N, 3, 2, 4, 40))), ("out rank", dict(out=z(3, 2, 5, 40))),
           ("slot past the row", dict(out_channel_offset=32)), ("mode", dict(mode="sum"))]
    if dev.type == "cuda":
        bad += [("pitch % 8", dict(out=z(N, 3, 2, 5, 44))), ("offset % 8", dict(out_channel_offset=4)),
                ("x dtype", dict(x=z(N, D, H, W, C, dtype=F32))), ("out dtype", dict(out=z(N, 3, 2, 5, 40, dtype=F32))),
                ("out device", dict(out=z(N, 3, 2, 5, 40, device=torch.device("cpu"))))]
    return good, bad


def _assert_refusals(dev):
    for fn, (good, bad) in ((K.conv3d_ndhwc, _bad_launches(dev)), (K.pool3d_ndhwc, _bad_pools(dev))):
        fn(**good)
        for what, over in bad:
            with pytest.raises((ValueError, TypeError)):
                fn(**{**good, **over})
                pytest.fail(f"not refused: {what}")


def test_launchers_reject_bad_arguments_host():
    _assert_refusals(torch.device("cpu"))


# =================================================================================== CPU: lowering
def _check_logits(got, ref):
    err = (got.float().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 0.05, err


class _G:
    """A small graph on a float feed ``x`` [2, 4, 5, 6, Cin]."""

    def __init__(self, cin=16, seed=0):
        self.gb = GraphBuilder()
        self.rng = np.random.default_rng(seed)
        self.cin = cin
        self.x = self.gb.placeholder("x", "FLOAT", [None, 4, 5, 6, cin])
        self.feeds = {"x:0": torch.from_numpy(self.rng.standard_normal((2, 4, 5, 6, cin)).astype(np.float32))}
        self.dtypes = {"x:0": "FLOAT"}

    def w(self, k, cout, cin=None, name="w"):
        cin = cin or self.cin
        fan = cin * k[0] * k[1] * k[2]
        return self.gb.constant(name, (self.rng.standard_normal((*k, cin, cout)) * np.sqrt(2.0 / fan)).astype(np.float32))

    def vec(self, n, name, lo=-0.5, hi=0.5):
        return self.gb.constant(name, self.rng.uniform(lo, hi, n).astype(np.float32))

    def feed(self, name, shape):
        self.feeds[f"{name}:0"] = torch.from_numpy(self.rng.standard_normal(shape).astype(np.float32))
        self.dtypes[f"{name}:0"] = "FLOAT"
        return self.gb.placeholder(name, "FLOAT", [None, *shape[1:]])

    def compile(self, fetches, device="cpu", strict=True):
        specs = {k: (tuple(v.shape), self.dtypes[k]) for k, v in self.feeds.items()}
        return CompiledFunction(self.gb.build(), specs, list(fetches), device, strict=strict)

    def reference(self, fetches):
        return Session(self.gb.build()).run(list(fetches), self.feeds)


def _g_chain():
    g = _G()
    y = g.gb.conv3d(g.x, g.w((3, 3, 3), 24), (1, 1, 1), "SAME", name="c")
    g.gb.relu(g.gb.bias_add(y, g.vec(24, "b"), name="bias"), name="y")
    return g, ["y:0"]


def _g_bn():
    g = _G()
    y = g.gb.conv3d(g.x, g.w((3, 3, 3), 24), (2, 2, 2), "SAME", name="c")
    y = g.gb.fused_batch_norm(y, g.vec(24, "gamma", 0.8, 1.2), g.vec(24, "beta"), g.vec(24, "mean"),
                              g.vec(24, "var", 0.8, 1.2), name="bn")
    g.gb.relu6(y, name="y")
    return g, ["y:0"]


def _g_sigmoid():
    g = _G()
    y = g.gb.conv3d(g.x, g.w((2, 3, 2), 8), (1, 1, 1), "VALID", name="c")
    g.gb.sigmoid(g.gb.bias_add(y, g.vec(8, "b"), name="bias"), name="y")
    return g, ["y:0"]


def _g_r2plus1d():
    """A (2+1)D block: a 1x3x3 spatial conv, then a 3x1x1 temporal conv with a depth stride."""
    g = _G()
    y = g.gb.conv3d(g.x, g.w((1, 3, 3), 24, name="ws"), (1, 1, 1), "SAME", name="spatial")
    y = g.gb.relu(g.gb.bias_add(y, g.vec(24, "bs"), name="bias_s"), name="relu_s")
    y = g.gb.conv3d(y, g.w((3, 1, 1), 16, cin=24, name="wt"), (2, 1, 1), "SAME", name="temporal")
    g.gb.relu(g.gb.bias_add(y, g.vec(16, "bt"), name="bias_t"), name="y")
    return g, ["y:0"]


def _g_cout3():
    g = _G()
    y = g.gb.conv3d(g.x, g.w((3, 3, 3), 3), (1, 1, 1), "SAME", name="c")
    g.gb.bias_add(y, g.vec(3, "b"), name="y")
    return g, ["y:0"]


def _g_padded_input():
    """A conv reading the 3-of-8-channel output of another one, in place."""
    g = _G()
    y = g.gb.conv3d(g.x, g.w((3, 3, 3), 3), (1, 1, 1), "SAME", name="c")
    y = g.gb.relu(g.gb.bias_add(y, g.vec(3, "b"), name="bias"), name="mid")
    g.gb.conv3d(y, g.w((3, 3, 3), 8, cin=3, name="w2"), (1, 1, 1), "SAME", name="y")
    return g, ["y:0"]


def _g_u8():
    g = _G()
    gb = g.gb
    clips = gb.placeholder("clips", "UINT8", [None, 4, 5, 6, 3])
    del g.feeds["x:0"]
    g.feeds["clips:0"] = torch.randint(0, 256, (2, 4, 5, 6, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    g.dtypes["clips:0"] = "UINT8"
    x = gb.mul(gb.cast(clips, "FLOAT", name="Cast"), gb.constant("scale", np.float32(1 / 255)), name="scaled")
    y = gb.conv3d(x, g.w((3, 3, 3), 16, cin=3), (1, 1, 1), "SAME", name="c")
    gb.relu(gb.bias_add(y, g.vec(16, "b"), name="bias"), name="y")
    return g, ["y:0"]


def _g_concat():
    """An I3D-style module: a conv branch and a pooled branch written into one buffer."""
    g = _G()
    a = g.gb.conv3d(g.x, g.w((3, 3, 3), 8, name="wa"), (1, 1, 1), "SAME", name="conv_a")
    a = g.gb.relu(g.gb.bias_add(a, g.vec(8, "ba"), name="bias_a"), name="relu_a")
    b = g.gb.max_pool3d(g.x, (3, 3, 3), (1, 1, 1), "SAME", name="pool_b")
    # a 1x1x1 branch would route to 2-D; read only by the concat it stays a conv3d step and writes its slice
    p = g.gb.relu(g.gb.conv3d(g.x, g.w((1, 1, 1), 8, name="wp"), (1, 1, 1), "SAME", name="conv_p"), name="relu_p")
    c = g.gb.concat([a, b, p], 4, name="cat")
    g.gb.conv3d(c, g.w((1, 1, 1), 16, cin=32, name="wc"), (1, 1, 1), "SAME", name="y")
    return g, ["y:0"]


def _g_mean():
    g = _G()
    y = g.gb.relu(g.gb.conv3d(g.x, g.w((3, 3, 3), 24), (1, 1, 1), "SAME", name="c"), name="r")
    g.gb.mean(y, [1, 2, 3], name="gap")
    g.gb.mean(y, [1, 2, 3], keep_dims=True, name="gap_keep")
    return g, ["gap:0", "gap_keep:0"]


def _g_flatten():
    g = _G()
    y = g.gb.relu(g.gb.conv3d(g.x, g.w((3, 3, 3), 8), (2, 2, 2), "SAME", name="c"), name="r")
    y = g.gb.avg_pool3d(y, (2, 2, 2), (2, 2, 2), "SAME", name="pool")
    f = g.gb.reshape(y, [-1, 1 * 2 * 2 * 8], name="flat")
    wm = g.gb.constant("wm", (g.rng.standard_normal((32, 10)) * 0.3).astype(np.float32))
    g.gb.bias_add(g.gb.matmul(f, wm, name="mm"), g.vec(10, "bm"), name="y")
    return g, ["y:0"]


LOWERED = {"chain": _g_chain, "bn": _g_bn, "sigmoid": _g_sigmoid, "r2plus1d": _g_r2plus1d, "cout3": _g_cout3,
           "padded_input": _g_padded_input, "u8": _g_u8, "concat": _g_concat, "mean": _g_mean, "flatten": _g_flatten}


def _check_lowered(name, plan, g, fetches, dev="cpu"):
    s = plan.summary()
    kinds = s["kinds"]
    steps = {st.name: st for st in plan.steps}
    assert s["glue_ops"] == []
    if name in ("chain", "bn"):
        assert kinds.get("conv3d") == 1 and "elementwise" not in kinds and "conv" not in kinds
        assert steps["c"].meta["impl"] == "conv3d"
        mid = "bias:0" if name == "chain" else "bn:0"
        assert {"y"} <= plan._fused and plan._val_of("y:0") is plan._val_of(mid)         # the chain is one value
        assert ({"bias"} if name == "chain" else {"bn"}) <= plan._fused
    elif name == "sigmoid":
        assert kinds.get("conv3d") == 1 and kinds.get("elementwise") == 1 and "bias" in plan._fused
        assert "y" not in plan._fused
    elif name == "r2plus1d":
        assert "conv3d" not in kinds and kinds.get("conv") == 2 and "copy" not in kinds
        assert {"spatial", "temporal"} <= set(steps) and {"bias_s", "relu_s", "bias_t", "y"} <= plan._fused
        assert tuple(plan._val_of("y:0").shape) == (2, 2, 5, 6, 16)
    elif name == "cout3":
        v = plan._val_of("y:0")
        assert kinds.get("conv3d") == 1 and tuple(v.shape) == (2, 4, 5, 6, 3) and v.phys_c == 8
    elif name == "padded_input":
        assert kinds.get("conv3d") == 2 and plan._val_of("mid:0").phys_c == 8
        assert not [n for n in steps if n.endswith("/pad_cin")]          # read in place
    elif name == "u8":
        assert kinds.get("conv3d") == 1 and "elementwise" not in kinds
        assert "Cast" not in steps and "scaled" not in steps and "scaled" in plan._fused
        assert [n for n in steps if n.endswith("/pad_cin")] == ["c/pad_cin"] and len(plan.steps) == 2
        assert plan._val_of("clips:0").dtype == torch.uint8 and plan._input_bufs["clips:0"].dtype == torch.uint8
    elif name == "concat":
        assert kinds.get("conv3d") == 2 and kinds.get("pool3d") == 1 and kinds.get("conv") == 1 and "concat" not in kinds
        cat = plan._val_of("cat:0")
        assert plan._val_of("relu_a:0").concat_slot == (cat, 0) and plan._val_of("pool_b:0").concat_slot == (cat, 8)
        assert plan._val_of("relu_p:0").concat_slot == (cat, 24) and steps["y"].kind == "conv"
    elif name == "mean":
        assert kinds.get("gap") == 2 and kinds.get("conv3d") == 1
        assert tuple(plan._val_of("gap:0").shape) == (2, 24) and tuple(plan._val_of("gap_keep:0").shape) == (2, 1, 1, 1, 24)
    elif name == "flatten":
        assert kinds.get("conv3d") == 1 and kinds.get("pool3d") == 1 and kinds.get("gemm") == 1
    got = plan({k: v.to(dev) for k, v in g.feeds.items()})
    for a, r in zip(got, g.reference(fetches)):
        assert a.shape == r.shape
        _check_logits(a, r)
    if name == "cout3":
        assert (plan._val_of("y:0").buf[..., 3:] == 0).all()             # zero padding columns
    return got


@pytest.mark.parametrize("name", list(LOWERED))
def test_lowered_graphs_host(name):
    g, fetches = LOWERED[name]()
    _check_lowered(name, g.compile(fetches), g, fetches)


def test_second_reader_of_the_uint8_prefix_leaves_it_alone():
    g, fetches = _g_u8()
    g.gb.mean(g.gb.identity("scaled:0", name="tap"), [1, 2, 3], name="other")
    with pytest.raises(CompileError):
        g.compile(fetches + ["other:0"])
    plan = g.compile(fetches + ["other:0"], strict=False)
    assert "Cast" in plan.summary()["glue_ops"]
    for a, r in zip(plan(g.feeds), g.reference(fetches + ["other:0"])):
        _check_logits(a, r)


def _glue_graph(case):
    """(graph holder, fetch, op name) of one op the lowering leaves to glue."""
    g = _G(cin=12 if case == "pool_c12" else 16)
    gb = g.gb
    attrs = dict(strides=[1, 1, 1, 1, 1], padding=b"SAME", data_format=b"NDHWC", dilations=[1, 1, 1, 1, 1])
    op = "Conv3D"
    if case == "fed_filter":
        gb.op("Conv3D", [g.x, g.feed("wf", (3, 3, 3, 16, 8))], name="y", **attrs)
    elif case == "ncdhw":
        xt = g.feed("xc", (2, 16, 4, 5, 6))
        del g.feeds["x:0"]
        gb.op("Conv3D", [xt, g.w((3, 3, 3), 8)], name="y", **{**attrs, "data_format": b"NCDHW"})
    elif case == "dilations":
        gb.op("Conv3D", [g.x, g.w((3, 3, 3), 8)], name="y", **{**attrs, "dilations": [1, 1, 2, 2, 1]})
    elif case == "filter9":
        gb.op("Conv3D", [g.x, g.w((3, 9, 3), 8)], name="y", **attrs)
    elif case == "stride5":
        gb.op("Conv3D", [g.x, g.w((3, 3, 3), 8)], name="y", **{**attrs, "strides": [1, 1, 5, 1, 1]})
    elif case == "pool_c12":
        op = "MaxPool3D"
        gb.max_pool3d(g.x, (2, 2, 2), (2, 2, 2), "SAME", name="y")
    elif case == "pool_window9":
        op = "AvgPool3D"
        gb.avg_pool3d(g.x, (2, 9, 2), (1, 1, 1), "SAME", name="y")
    return g, ["y:0"], op


GLUE = ("fed_filter", "ncdhw", "dilations", "filter9", "stride5", "pool_c12", "pool_window9")


@pytest.mark.parametrize("case", GLUE)
def test_what_stays_glue(case):
    g, fetches, op = _glue_graph(case)
    with pytest.raises(CompileError, match=op):
        g.compile(fetches)
    plan = g.compile(fetches, strict=False)
    s = plan.summary()
    assert op in s["glue_ops"] and "conv3d" not in s["kinds"] and "pool3d" not in s["kinds"]
    got, = plan(g.feeds)
    ref, = g.reference(fetches)
    assert got.shape == ref.shape
    _check_logits(got, ref)


# =================================================================================== C3D
C3D = dict(base=8, fc=32, frames=4, image_hw=(16, 16), num_classes=11, top_k=5, seed=0)
C3D_KINDS = {"glue": 1, "conv3d": 8, "pool3d": 5, "gemm": 3, "softmax_topk": 1}
C3D_FETCHES = ["logits:0", "top_k:0", "top_k:1"]


def _clips(n, seed):
    return torch.randint(0, 256, (n, 4, 16, 16, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def c3d():
    """The graph, three clips and the fp32 interpreter's (logits, top-k probabilities, indices): once."""
    from flink_tensorflow_amd.models.zoo import c3d_graph_def

    g = Graph.from_graph_def(c3d_graph_def(**C3D))
    clips = _clips(3, seed=11)
    ref = Session(g).run(C3D_FETCHES, {"clips:0": clips})
    return g, clips, ref


def _c3d_plan(g, clips, dev="cpu"):
    return CompiledFunction(g, {"clips:0": (tuple(clips.shape), "UINT8")}, C3D_FETCHES, dev, strict=True)


def _check_top1(labels, probs, ref):
    """Top-1 labels agree with the interpreter wherever its top-2 probabilities are at least 0.02
    apart, and the top probability is within 0.02 of its."""
    must = (ref[1][:, 0] - ref[1][:, 1]) >= 0.02
    assert must.any()
    assert torch.equal(torch.as_tensor(labels)[must].long(), ref[2][:, 0][must].long())
    assert (torch.as_tensor(probs).float() - ref[1][:, 0]).abs().max() < 0.02


def _check_c3d_plan(plan, clips, ref, dev="cpu"):
    s = plan.summary()
    assert s["glue_ops"] == [] and "elementwise" not in s["kinds"] and s["kinds"] == C3D_KINDS
    assert [st.name for st in plan.steps if st.kind == "glue"] == ["conv1/Conv3D/pad_cin"]
    assert all(st.meta["impl"] == "conv3d" for st in plan.steps if st.kind == "conv3d")
    assert plan._input_bufs["clips:0"].dtype == torch.uint8
    logits, vals, idxs = plan({"clips:0": clips.to(dev)})
    assert logits.shape == (3, 11) and vals.shape == (3, 5) and idxs.shape == (3, 5)
    _check_logits(logits, ref[0])
    _check_top1(idxs[:, 0].cpu(), vals[:, 0].cpu(), ref)
    return idxs.cpu()


def test_c3d_plan_host(c3d):
    g, clips, ref = c3d
    assert ref[0].shape == (3, 11) and ref[2].shape == (3, 5)
    _check_c3d_plan(_c3d_plan(g, clips), clips, ref)


def test_default_c3d_lowers_without_glue():
    """The default 16 x 112 x 112 C3D (a narrow head, to keep the constants small): strict, no glue op."""
    from flink_tensorflow_amd.models.zoo import c3d_graph_def
    from flink_tensorflow_amd.models.zoo.c3d import c3d_layer_shapes

    layers = c3d_layer_shapes()
    assert [l["out"] for l in layers if l["kind"] == "pool"] == [(16, 56, 56, 64), (8, 28, 28, 128), (4, 14, 14, 256),
                                                                 (2, 7, 7, 512), (1, 4, 4, 512)]
    g = Graph.from_graph_def(c3d_graph_def(fc=64))
    plan = CompiledFunction(g, {"clips:0": ((1, 16, 112, 112, 3), "UINT8")}, ["top_k:1"], "cpu", strict=True)
    assert plan.summary()["kinds"] == C3D_KINDS and plan.summary()["glue_ops"] == []


def test_video_classifier_on_the_host(c3d):
    from flink_tensorflow_amd.models.zoo import VideoClassifierModel

    g, clips, ref = c3d
    m = VideoClassifierModel(buckets=(3,), device="cpu", **C3D)
    m.open()
    try:
        res = m.classify(list(clips.numpy()))
        (batched, tags, _), = m.submit(list(clips.numpy()), np.zeros(3), [5, 6, 7])
        with pytest.raises(ValueError):
            m.classify([clips[0].numpy()[:2]])
    finally:
        m.close()
    assert len(res) == 3 and all(len(r) == 5 for r in res)
    assert [[lab for _, lab in r] for r in res] == [[f"class_{i}" for i in row] for row in ref[2].tolist()]   # host: the interpreter
    assert np.allclose([[p for p, _ in r] for r in res], ref[1].numpy())
    assert tags == [5, 6, 7] and batched == res


def test_c3d_saved_model_compiles_strict(tmp_path, c3d):
    from flink_tensorflow_amd.models import PredictMethod, SavedModelModel
    from flink_tensorflow_amd.models.zoo import export_c3d_saved_model

    _, clips, ref = c3d
    d = export_c3d_saved_model(str(tmp_path / "c3d"), **C3D)
    m = SavedModelModel(d, device="cpu")
    m.open()
    try:
        interp = m.function("serving_default", PredictMethod(), compile=False)
        fn = m.function("serving_default", PredictMethod(), compile=True, batch_buckets=None)
        a, b = interp.apply({"clips": clips.numpy()}), fn.apply({"clips": clips.numpy()})
        s = fn.plan_summary()
    finally:
        m.close()
    assert s is not None and s["glue_ops"] == [] and s["kinds"]["conv3d"] == 8 and s["kinds"]["pool3d"] == 5
    assert torch.equal(torch.as_tensor(a["scores"]).float(), ref[1])       # the variables restore the weights
    _check_top1(torch.as_tensor(b["classes"])[:, 0], torch.as_tensor(b["scores"])[:, 0], ref)


# =================================================================================== GPU: the kernels
def _banded(t, fill, dev, band=4096):
    """``t`` as a view into a larger allocation filled with ``fill`` -> (view, whole buffer)."""
    n = t.numel()
    buf = torch.full((band + n + band,), fill, dtype=t.dtype, device=dev)
    v = buf[band:band + n].view(t.shape)
    v.copy_(t)
    return v, buf


def _bands_intact(buf, n, fill, band=4096):
    h = buf.cpu()
    lo, hi = h[:band], h[band + n:]
    if fill != fill:
        return bool(torch.isnan(lo).all() and torch.isnan(hi).all())
    return bool((lo == fill).all() and (hi == fill).all())


def _launch(shape, geom, act, bias, cfg, dev, **kw):
    k, s, pads, _ = _geo(geom, shape[1:4])
    x, w, b = _data(shape, geom, act == "relu6", bias)
    wp = K.conv3d_pack_weights(w).to(BF)
    assert torch.equal(wp.double(), K.conv3d_pack_weights(w))     # exact in bf16
    return K.conv3d_ndhwc(x.to(BF).to(dev), wp.to(dev), b.float().to(dev) if bias else None, k, s, pads, act, cfg=cfg, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_kernel_bit_exact(case):
    shape, geom = case
    dev = torch.device("cuda", 0)
    for act in ACTS:
        for bias in (False, True):
            want = _bits(_ref(shape, geom, act, bias)[1])
            for cfg in (-1, *K.CONV3D_TILES.values()):
                y = _launch(shape, geom, act, bias, cfg, dev)
                assert y.dtype == BF and torch.equal(_bits(y.cpu()), want), (act, bias, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POOLS))
def test_pool_kernel_bit_exact(name):
    dev = torch.device("cuda", 0)
    k, s, padding, ext, pads, _ = _pool_geo(name)
    for C in (8, 24):
        for mode in ("max", "avg"):
            x = _pool_data(name, C, mode)
            assert torch.equal(x.to(BF).float(), x)
            want = _bits(_pool_mirror(x, k, s, pads, mode).to(BF))
            y = K.pool3d_ndhwc(x.to(BF).to(dev), k, s, pads, mode)
            assert y.dtype == BF and torch.equal(_bits(y.cpu()), want), (C, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", list(GEOMS))
def test_kernel_guard_bands(geom):
    shape = SHAPES[1]
    N, D, H, W, Cin, Cout = shape
    k, s, pads, out = _geo(geom, (D, H, W))
    dev = torch.device("cuda", 0)
    nan = float("nan")
    x, w, b = _data(shape, geom, False, True)
    want = _bits(_ref(shape, geom, "relu", True)[1])
    xv, xbuf = _banded(x.to(BF), nan, dev)
    wv, wbuf = _banded(K.conv3d_pack_weights(w).to(BF), nan, dev)
    bv, bbuf = _banded(b.float(), nan, dev)
    coff, ldo = 16, 16 + Cout + 24
    for cfg in K.CONV3D_TILES.values():
        ov, obuf = _banded(torch.full((N, *out, ldo), SENT, dtype=BF), SENT, dev)
        y = K.conv3d_ndhwc(xv, wv, bv, k, s, pads, "relu", out=ov, out_channel_offset=coff, cfg=cfg)
        assert y is ov and _bands_intact(obuf, ov.numel(), SENT), "stray store"
        o = ov.cpu()
        assert torch.equal(_bits(o[..., coff:coff + Cout]), want)
        assert (o[..., :coff] == SENT).all() and (o[..., coff + Cout:] == SENT).all()   # outside the slice: untouched
    for buf, v in ((xbuf, xv), (wbuf, wv), (bbuf, bv)):
        assert _bands_intact(buf, v.numel(), nan)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POOLS))
def test_pool_kernel_guard_bands(name):
    dev = torch.device("cuda", 0)
    k, s, padding, ext, pads, _ = _pool_geo(name)
    C, coff = 24, 16
    ldo = coff + C + 24
    for mode in ("max", "avg"):
        x = _pool_data(name, C, mode)
        ref = _pool_mirror(x, k, s, pads, mode).to(BF)
        xv, xbuf = _banded(x.to(BF), float("nan"), dev)
        ov, obuf = _banded(torch.full((*ref.shape[:4], ldo), SENT, dtype=BF), SENT, dev)
        y = K.pool3d_ndhwc(xv, k, s, pads, mode, out=ov, out_channel_offset=coff)
        assert y is ov and _bands_intact(obuf, ov.numel(), SENT), "stray store"
        o = ov.cpu()
        assert torch.equal(_bits(o[..., coff:coff + C]), _bits(ref))
        assert (o[..., :coff] == SENT).all() and (o[..., coff + C:] == SENT).all()
        assert _bands_intact(xbuf, xv.numel(), float("nan"))


@pytest.mark.gpu
def test_offsets_past_2_31():
    """Two launches whose element offsets need 64 bits; only the tail rows are filled and checked,
    against a row-wise matmul: a 1x1x1 conv has one tap and its rows do not interact."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    Cin, Cout = 8, 8
    w = torch.randint(-4, 5, (1, 1, 1, Cin, Cout), generator=g).to(F64)
    b = torch.randint(-1200, 1201, (Cout,), generator=g).to(F64) / 2
    wp = K.conv3d_pack_weights(w).to(BF).to(dev)
    # 1. an output of more than 2^31 elements: pitch 520 over 16 x 512 x 512 pixels
    D, H, W, ldo, coff = 16, 512, 512, 520, 504
    assert D * H * W * ldo > 2 ** 31
    xt = torch.randint(-8, 9, (8, W, Cin), generator=g).to(F64)           # the last 8 rows of the last plane
    x = torch.zeros((1, D, H, W, Cin), dtype=BF, device=dev)
    x[0, -1, -8:] = xt.to(BF).to(dev)
    out = torch.empty((1, D, H, W, ldo), dtype=BF, device=dev)
    out[0, -1, -8:].fill_(SENT)
    K.conv3d_ndhwc(x, wp, b.float().to(dev), (1, 1, 1), (1, 1, 1), (0,) * 6, "none", out=out, out_channel_offset=coff)
    tail = out[0, -1, -8:].cpu()
    ref = xt @ w[0, 0, 0] + b
    assert torch.equal(_bits(tail[..., coff:coff + Cout]), _bits(ref.to(F32).to(BF)))
    assert (tail[..., :coff] == SENT).all() and (tail[..., coff + Cout:] == SENT).all()
    del out, x
    torch.cuda.empty_cache()
    # 2. an input of more than 2^31 elements, read at stride (1, 4, 4)
    D, H, W = 4, 8192, 8200
    assert D * H * W * Cin > 2 ** 31
    x = torch.empty((1, D, H, W, Cin), dtype=BF, device=dev)
    xt = torch.randint(-8, 9, (8, W, Cin), generator=g).to(F64)           # input rows 8184 .. 8191 of the last plane
    x[0, -1, -8:] = xt.to(BF).to(dev)
    y = K.conv3d_ndhwc(x, wp, b.float().to(dev), (1, 1, 1), (1, 4, 4), (0,) * 6, "none")
    assert y.shape == (1, 4, 2048, 2050, Cout)
    ref = xt[::4, ::4] @ w[0, 0, 0] + b                                  # output rows 2046, 2047
    assert torch.equal(_bits(y[0, -1, -2:].cpu()), _bits(ref.to(F32).to(BF)))
    del x, y
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_launchers_reject_bad_arguments():
    _assert_refusals(torch.device("cuda", 0))


# =================================================================================== GPU: the plans
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LOWERED))
def test_lowered_graphs_gpu(name):
    dev = torch.device("cuda", 0)
    g, fetches = LOWERED[name]()
    plan = g.compile(fetches, dev)
    assert plan.summary()["hip_graph"]
    got = _check_lowered(name, plan, g, fetches, dev)
    again = plan({k: v.to(dev) for k, v in g.feeds.items()})
    for a, b in zip(got, again):
        assert torch.equal(a, b)                               # a second replay is bit-identical


@pytest.mark.gpu
def test_glue_op_is_captured_gpu():
    """A 3-D conv the lowering leaves to glue (a 9-tall filter) still runs in a captured plan."""
    dev = torch.device("cuda", 0)
    g, fetches, _ = _glue_graph("filter9")
    plan = g.compile(fetches, dev, strict=False)
    s = plan.summary()
    assert s["hip_graph"] and s["glue_ops"] == ["Conv3D"]
    got, = plan({k: v.to(dev) for k, v in g.feeds.items()})
    _check_logits(got, g.reference(fetches)[0])


@pytest.mark.gpu
def test_c3d_plan_and_model_gpu(c3d):
    from flink_tensorflow_amd.models.zoo import VideoClassifierModel

    g, clips, ref = c3d
    dev = torch.device("cuda", 0)
    plan = _c3d_plan(g, clips, dev)
    assert plan.summary()["hip_graph"]
    idxs = _check_c3d_plan(plan, clips, ref, dev)
    again = plan({"clips:0": clips.to(dev)})
    assert torch.equal(again[2].cpu(), idxs)            # a second replay is bit-identical
    m = VideoClassifierModel(buckets=(3,), lanes=1, **C3D)
    m.open()
    try:
        s = m.plan_summary()
        assert s["glue_ops"] == [] and s["kinds"]["conv3d"] == 8
        res = m.classify(list(clips.numpy()))
        done = []
        for i in range(3):   # one record per batch: results come back in submission order
            done += m.submit([clips[i].numpy()], np.zeros(1), [i])
        done += m.drain()
    finally:
        m.close()
    labels = [[f"class_{i}" for i in row] for row in idxs.tolist()]
    assert [[lab for _, lab in r] for r in res] == labels      # the model is the plan
    assert [t for _, tags, _ in done for t in tags] == [0, 1, 2]
    batched = [r for rs, _, _ in done for r in rs]
    top1 = torch.tensor([int(r[0][1].split("_")[1]) for r in batched])
    _check_top1(top1, torch.tensor([r[0][0] for r in batched]), ref)
