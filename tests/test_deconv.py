"""Transposed convolution: the interpreter op ``Conv2DBackpropInput``, the kernel of
``kernels/deconv.hip``, its weight packing and launcher, the lowering and the U-Net model.

The definition (``graph/ops_nn.py:conv2d_transpose_tf``) has two independent anchors: the gradient
of the existing ``conv2d_tf`` with respect to its input (``out_backprop`` as the cotangent), and a
float64 mirror written here from the formula, tap by tap:
``y[n, oy, ox, co] += x[n, iy, ix, ci] w[ky, kx, co, ci]`` wherever ``oy + pt - ky == iy * sh`` and
``0 <= iy < Hi`` (likewise in x).  On integer data all three agree exactly.

The mirror has two deliberately wrong variants: out-of-range taps clamped to the edge instead of
dropped, and the filter taken unflipped (``w[KH-1-ky, KW-1-kx]``).  The clamped one differs from
the truth exactly for the geometries in which some tap falls outside the input (none for
``k <= s``); the unflipped one whenever ``KH * KW > 1``.

Exact data.  x, w are small integers and the bias halves, sized per activation (sparse for ReLU6,
so that the sums stay near [0, 6]); the mirror asserts ``sum |x| |w| + |b| < 2^22`` per output, so
fp32 accumulation is exact in any order and the only rounding is the kernel's final ``f2bf``.
Kernel outputs are compared on their bf16 bit patterns.  Per activation every outcome (zero,
interior, clipped at 6) covers at least 5 % of the outputs, and on the bias cases the rounding
to bf16 is observable.

Device tests put x, the packed weights and the bias between NaN bands and write a channel slice
of a wider buffer filled with the sentinel 2^100, itself between bands, as ``tests/test_dwconv.py``
does.

Plans.  ``logits`` within 0.05 of the fp32 interpreter relative to its maximum and labels
agreeing wherever the interpreter's top-2 margin is at least 0.1 of the largest logit, at most
half of the pixels excused: the rules of ``tests/test_segmentation.py``."""
import functools
import zlib

import numpy as np
import pytest
import torch

from flink_tensorflow_amd.graph.builder import GraphBuilder
from flink_tensorflow_amd.graph.compiler import CompiledFunction, CompileError
from flink_tensorflow_amd.graph.graph import Graph
from flink_tensorflow_amd.graph.ops_nn import conv2d_tf, conv2d_transpose_tf, same_pads
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.ops import kernels as K

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 2.0 ** 100
ACTS = ("none", "relu", "relu6")

# (N, Hi, Wi, Cin, Cout)
SHAPES = ((1, 3, 5, 8, 8), (2, 5, 7, 40, 24), (3, 4, 3, 72, 136), (1, 9, 6, 264, 8), (2, 17, 3, 16, 72))
# name -> (KH, KW, (sh, sw), padding, (Ho, Wo) of (Hi, Wi))
GEOMS = {
    "2x2s2-same": (2, 2, (2, 2), "SAME", lambda h, w: (2 * h, 2 * w)),
    "2x2s2-valid": (2, 2, (2, 2), "VALID", lambda h, w: (2 * h, 2 * w)),
    "3x3s2-same": (3, 3, (2, 2), "SAME", lambda h, w: (2 * h, 2 * w)),
    "3x3s2-same-odd": (3, 3, (2, 2), "SAME", lambda h, w: (2 * h - 1, 2 * w - 1)),       # unequal phases
    "3x3s2-valid-extra": (3, 3, (2, 2), "VALID", lambda h, w: (2 * h + 2, 2 * w + 2)),   # a row no tap reaches
    "4x4s2-same": (4, 4, (2, 2), "SAME", lambda h, w: (2 * h, 2 * w)),
    "5x5s3-same": (5, 5, (3, 3), "SAME", lambda h, w: (3 * h - 2, 3 * w - 2)),
    "1x1s2-valid": (1, 1, (2, 2), "VALID", lambda h, w: (2 * h, 2 * w)),                 # phases without taps
    "2x2s3-valid": (2, 2, (3, 3), "VALID", lambda h, w: (3 * h, 3 * w)),                 # phases without taps
    "4x4s4": (4, 4, (4, 4), "VALID", lambda h, w: (4 * h, 4 * w)),
    "3x2s21": (3, 2, (2, 1), "SAME", lambda h, w: (2 * h, w)),
    "3x3s1": (3, 3, (1, 1), "SAME", lambda h, w: (h, w)),
}
CASES = [(s, g) for g in GEOMS for s in SHAPES]


def _case_id(c):
    (N, H, W, Ci, Co), g = c
    return f"{g}-{N}x{H}x{W}x{Ci}x{Co}"


def _geo(geom, Hi, Wi):
    """(KH, KW, sh, sw, pt, pl, Ho, Wo)"""
    KH, KW, (sh, sw), padding, fn = GEOMS[geom]
    Ho, Wo = fn(Hi, Wi)
    pt = same_pads(Ho, KH, sh)[0] if padding == "SAME" else 0
    pl = same_pads(Wo, KW, sw)[0] if padding == "SAME" else 0
    return KH, KW, sh, sw, pt, pl, Ho, Wo


def _has_outside_tap(geom, Hi, Wi):
    """Some (output row, tap) pair of the definition lands outside the input."""
    KH, KW, sh, sw, pt, pl, Ho, Wo = _geo(geom, Hi, Wi)

    def axis(O, I, Kk, s, p):
        return any((o + p - k) % s == 0 and not 0 <= (o + p - k) // s < I for o in range(O) for k in range(Kk))

    return axis(Ho, Hi, KH, sh, pt) or axis(Wo, Wi, KW, sw, pl)


# =================================================================================== the mirror
def _mirror_pre(x, w, geom, clamp=False, unflipped=False):
    """float64 ``deconv(x, w)`` from the definition, one filter tap and one output row / column
    at a time.  ``clamp`` / ``unflipped``: the deliberately wrong variants."""
    N, Hi, Wi, Cin = x.shape
    KH, KW, sh, sw, pt, pl, Ho, Wo = _geo(geom, Hi, Wi)
    Cout = w.shape[2]
    y = torch.zeros((N, Ho, Wo, Cout), dtype=F64)

    def taps(O, I, k, s, p):
        """(output index, input index) pairs of filter tap k along one axis"""
        out = []
        for o in range(O):
            if (o + p - k) % s:
                continue
            i = (o + p - k) // s
            if 0 <= i < I:
                out.append((o, i))
            elif clamp:
                out.append((o, min(max(i, 0), I - 1)))
        return out

    for ky in range(KH):
        rows = taps(Ho, Hi, ky, sh, pt)
        for kx in range(KW):
            cols = taps(Wo, Wi, kx, sw, pl)
            if not rows or not cols:
                continue
            wt = w[KH - 1 - ky, KW - 1 - kx] if unflipped else w[ky, kx]   # [Cout, Cin]
            oy, iy = (torch.tensor(v) for v in zip(*rows))
            ox, ix = (torch.tensor(v) for v in zip(*cols))
            y[:, oy[:, None], ox[None, :]] += x[:, iy[:, None], ix[None, :]] @ wt.t()
    return y


def _act(v, act):
    if act == "relu":
        return torch.relu(v)
    if act == "relu6":
        return torch.clamp(v, 0, 6)
    return v


def _max_taps(geom):
    KH, KW, (sh, sw), _, _ = GEOMS[geom]
    return -(-KH // sh) * -(-KW // sw)


@functools.lru_cache(maxsize=None)
def _data(shape, geom, small, bias):
    """(x, w [KH, KW, Cout, Cin], bias or None) as float64 integers / half-integers.  ``small``
    (ReLU6): x in {0, 1} with a density that puts the largest phase's sums around [0, 6], w in
    [-1, 2], bias halves spread over [-6, 8.5]; otherwise x in [-8, 8], w in [-4, 4], bias halves in
    [-600, 600] with alternating signs."""
    N, Hi, Wi, Cin, Cout = shape
    KH, KW = GEOMS[geom][:2]
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, geom, small, bias)).encode()))
    if small:
        kmax = Cin * _max_taps(geom)
        dens = min(1.0, (4.0 if bias else 10.0) / kmax)
        x = (torch.rand((N, Hi, Wi, Cin), generator=g) < dens).to(F64)
        w = torch.randint(-1, 3, (KH, KW, Cout, Cin), generator=g).to(F64)
        # a spread from -6 to 8.5 across the channels (few channels must not all land on one outcome)
        b = ((torch.arange(Cout) % 8) * 2 - 6 + torch.randint(0, 2, (Cout,), generator=g) / 2).to(F64) if bias else None
    else:
        x = torch.randint(-8, 9, (N, Hi, Wi, Cin), generator=g).to(F64)
        w = torch.randint(-4, 5, (KH, KW, Cout, Cin), generator=g).to(F64)
        b = torch.randint(1, 1201, (Cout,), generator=g).to(F64) / 2 if bias else None
        if bias:
            b[1::2] *= -1        # both signs whatever the draw: few channels must not all clip at 0
    return x, w, b


@functools.lru_cache(maxsize=None)
def _pre(shape, geom, small, bias):
    """The mirror's ``deconv + bias`` in float64; asserts that fp32 accumulation is exact."""
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


# =================================================================================== CPU: the definition
ANCHOR_SHAPE = (2, 5, 7, 8, 16)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_definition_has_two_anchors(geom):
    x, w, _ = _data(ANCHOR_SHAPE, geom, False, False)
    N, Hi, Wi, Cin, Cout = ANCHOR_SHAPE
    KH, KW, (sh, sw), padding, _ = GEOMS[geom]
    Ho, Wo = _geo(geom, Hi, Wi)[6:]
    y = conv2d_transpose_tf(x, w, (Ho, Wo), (sh, sw), padding)
    assert y.dtype == F64 and y.shape == (N, Ho, Wo, Cout)
    # anchor 1: the gradient of the forward conv (filter [KH, KW, in = Cout, out = Cin])
    inp = torch.zeros((N, Ho, Wo, Cout), dtype=F64, requires_grad=True)
    fwd = conv2d_tf(inp, w, (sh, sw), padding)
    assert fwd.shape == x.shape
    grad, = torch.autograd.grad(fwd, inp, x)
    assert torch.equal(y, grad)
    # anchor 2: the mirror
    m = _mirror_pre(x, w, geom)
    assert torch.equal(y, m)
    # the wrong variants are caught
    outside = _has_outside_tap(geom, Hi, Wi)
    if KH <= sh and KW <= sw:
        assert not outside            # k <= s: every tap of every output row is inside
    if geom in ("3x3s2-same", "3x3s2-valid-extra", "4x4s2-same", "3x3s1"):
        assert outside                # the border rows of these read past the input
    assert torch.equal(_mirror_pre(x, w, geom, clamp=True), m) != outside
    assert torch.equal(_mirror_pre(x, w, geom, unflipped=True), m) == (KH * KW == 1)
    # float32 inputs stay float32
    assert conv2d_transpose_tf(x.float(), w.float(), (Ho, Wo), (sh, sw), padding).dtype == F32


def test_definition_rejects_inconsistent_sizes():
    x, w = torch.zeros((1, 4, 4, 8)), torch.zeros((3, 3, 8, 8))
    conv2d_transpose_tf(x, w, (8, 8), (2, 2), "SAME")
    conv2d_transpose_tf(x, w, (7, 7), (2, 2), "SAME")
    for hw, pad in (((9, 9), "SAME"), ((6, 8), "SAME"), ((8, 8), "VALID"), ((0, 8), "SAME")):
        with pytest.raises(ValueError):
            conv2d_transpose_tf(x, w, hw, (2, 2), pad)
    with pytest.raises(ValueError):
        conv2d_transpose_tf(torch.zeros((1, 4, 4, 16)), w, (8, 8), (2, 2), "SAME")


def test_interpreter_op_and_builder():
    """4-vector and 2-vector ``input_sizes``, NCHW by permuting, the builder's node."""
    x, w, _ = _data(ANCHOR_SHAPE, "3x3s2-same-odd", False, False)
    ref = conv2d_transpose_tf(x.float(), w.float(), (9, 13), (2, 2), "SAME")
    gb = GraphBuilder()
    xin = gb.placeholder("x", "FLOAT", [None, 5, 7, 8])
    y2 = gb.conv2d_transpose(xin, gb.constant("w", w.float().numpy()), (9, 13), (2, 2), "SAME", name="up")
    s4 = gb.constant("sizes4", np.asarray([2, 9, 13, 16], dtype=np.int32))
    gb.op("Conv2DBackpropInput", [s4, "w:0", xin], name="up4", strides=[1, 2, 2, 1], padding=b"SAME",
          data_format=b"NHWC")
    xt = gb.transpose(xin, [0, 3, 1, 2], name="nchw")
    s4c = gb.constant("sizes4c", np.asarray([2, 16, 9, 13], dtype=np.int32))
    gb.op("Conv2DBackpropInput", [s4c, "w:0", xt], name="upc", strides=[1, 1, 2, 2], padding=b"SAME",
          data_format=b"NCHW")
    g = gb.build()
    assert y2 == "up:0" and g["up"].op == "Conv2DBackpropInput"
    assert [s for s, _ in g["up"].inputs] == ["up/input_sizes", "w", "x"]
    a, b, c = Session(g).run(["up:0", "up4:0", "upc:0"], {"x:0": x.float()})
    assert torch.equal(a, ref) and torch.equal(b, ref) and torch.equal(c.permute(0, 2, 3, 1), ref)
    gb.op("Conv2DBackpropInput", [gb.constant("bad", np.asarray([12, 13], dtype=np.int32)), "w:0", xin], name="upbad",
          strides=[1, 2, 2, 1], padding=b"SAME", data_format=b"NHWC")
    with pytest.raises(Exception, match="does not give"):
        Session(gb.build()).run(["upbad:0"], {"x:0": x.float()})


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


# =================================================================================== CPU: packing, launcher
@pytest.mark.parametrize("geom", list(GEOMS))
def test_pack_weights(geom):
    shape = SHAPES[1]
    _, w, _ = _data(shape, geom, False, False)
    KH, KW, sh, sw, pt, pl, _, _ = _geo(geom, shape[1], shape[2])
    Cout, Cin = w.shape[2:]
    phases = K.deconv_phases((KH, KW), (sh, sw), (pt, pl), Cin, Cout)
    assert [(p["py"], p["px"]) for p in phases] == [(py, px) for py in range(sh) for px in range(sw)]
    seen = [(ky, kx) for p in phases for ky, kx, _, _ in p["taps"]]
    assert sorted(seen) == [(ky, kx) for ky in range(KH) for kx in range(KW)]    # each tap in exactly one phase
    off = 0
    for p in phases:
        assert p["offset"] == off and p["k"] == len(p["taps"]) * Cin
        for ky, kx, dy, dx in p["taps"]:
            assert (p["py"] + pt - ky) == dy * sh and (p["px"] + pl - kx) == dx * sw
        off += p["k"] * Cout
    empty = [p for p in phases if not p["taps"]]
    assert all(p["k"] == 0 for p in empty) and bool(empty) == (KH < sh or KW < sw)
    wp = K.deconv_pack_weights(w, (sh, sw), (pt, 0, pl, 0))
    assert wp.shape == (KH * KW * Cout * Cin,) and wp.dtype == w.dtype
    assert torch.equal(K.deconv_unpack_weights(wp, (KH, KW), (sh, sw), (pt, pl), Cin, Cout), w)
    # the first row of the first non-empty phase: its taps' Cin-vectors of output channel 0, back to back
    p0 = next(p for p in phases if p["taps"])
    row = torch.cat([w[ky, kx, 0] for ky, kx, _, _ in p0["taps"]])
    assert torch.equal(wp[p0["offset"]:p0["offset"] + p0["k"]], row)


def test_eligible_is_pure_and_matches_the_launcher():
    ok = lambda *a: K.deconv_eligible(*a)   # noqa: E731
    assert ok(8, 8, 1, 1, (1, 1)) and ok(264, 136, 8, 8, (4, 4)) and ok(16, 24, 3, 2, (2, 1))
    assert not ok(12, 8, 2, 2, (2, 2)) and not ok(8, 12, 2, 2, (2, 2)) and not ok(0, 8, 2, 2, (2, 2))
    assert not ok(8, 8, 9, 2, (2, 2)) and not ok(8, 8, 2, 9, (2, 2)) and not ok(8, 8, 0, 2, (2, 2))
    assert not ok(8, 8, 2, 2, (5, 2)) and not ok(8, 8, 2, 2, (2, 0))
    # the launcher refuses what it rejects, on the host too
    for Cin, Cout, KH, KW, st in ((12, 8, 2, 2, (2, 2)), (8, 12, 2, 2, (2, 2)), (8, 8, 9, 2, (2, 2)),
                                  (8, 8, 2, 2, (5, 2)), (8, 8, 2, 2, (2, 2))):
        x = torch.zeros((1, 3, 3, Cin))
        wp = torch.zeros(KH * KW * Cout * Cin)
        if K.deconv_eligible(Cin, Cout, KH, KW, st):
            K.deconv2d_nhwc(x, wp, None, (3 * st[0], 3 * st[1]), (KH, KW), st)
        else:
            with pytest.raises(ValueError):
                K.deconv2d_nhwc(x, wp, None, (3 * st[0], 3 * st[1]), (KH, KW), st)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_host_path_equals_the_interpreter(geom):
    shape = SHAPES[1]
    N, Hi, Wi, Cin, Cout = shape
    KH, KW, sh, sw, pt, pl, Ho, Wo = _geo(geom, Hi, Wi)
    for act in ACTS:
        for bias in (False, True):
            x, w, b = _data(shape, geom, act == "relu6", bias)
            ref = conv2d_transpose_tf(x.float(), w.float(), (Ho, Wo), (sh, sw), GEOMS[geom][3])
            ref = _act(ref + b.float() if bias else ref, act)
            wp = K.deconv_pack_weights(w.float(), (sh, sw), (pt, pl))
            bf = b.float() if bias else None
            y = K.deconv2d_nhwc(x.float(), wp, bf, (Ho, Wo), (KH, KW), (sh, sw), (pt, 0, pl, 0), act)
            assert y.dtype == F32 and torch.equal(y, ref)
            assert torch.equal(y.double(), _ref(shape, geom, act, bias)[0])
            wide = torch.full((N, Ho, Wo, Cout + 24), 7.0)
            assert K.deconv2d_nhwc(x.float(), wp, bf, (Ho, Wo), (KH, KW), (sh, sw), (pt, 0, pl, 0), act, out=wide,
                                   out_channel_offset=16) is wide
            assert torch.equal(wide[..., 16:16 + Cout], ref)
            assert (wide[..., :16] == 7).all() and (wide[..., 16 + Cout:] == 7).all()


def _bad_launches(dev):
    """(description, kwargs overriding a good launch) for every refusal of the launcher."""
    N, Hi, Wi, Cin, Cout = 1, 3, 4, 16, 24
    dt = BF if dev.type == "cuda" else F32
    good = dict(x=torch.zeros((N, Hi, Wi, Cin), dtype=dt, device=dev),
                w_packed=torch.zeros(4 * Cin * Cout, dtype=dt, device=dev),
                bias=torch.zeros(Cout, dtype=F32, device=dev), out_hw=(6, 8), kernel=(2, 2), stride=(2, 2),
                pad=(0, 0, 0, 0), act="relu", out=torch.zeros((N, 6, 8, 40), dtype=dt, device=dev), out_channel_offset=8)
    z = lambda *s, dtype=dt, device=dev: torch.zeros(s, dtype=dtype, device=device)   # noqa: E731
    bad = [("x rank", dict(x=z(3, 4, Cin))), ("weights length", dict(w_packed=z(4 * Cin * Cout + 8))),
           ("weights rank", dict(w_packed=z(4, Cin * Cout))), ("Cin % 8", dict(x=z(N, Hi, Wi, 12), w_packed=z(4 * 12 * 24))),
           ("Cout % 8", dict(w_packed=z(4 * Cin * 12), bias=z(12, dtype=F32), out=None)),
           ("filter above 8", dict(kernel=(9, 1), w_packed=z(9 * Cin * Cout))), ("stride above 4", dict(stride=(5, 2))),
           ("stride 0", dict(stride=(0, 2))), ("pad above the filter", dict(pad=(2, 0, 0, 0))),
           ("negative pad", dict(pad=(0, 0, -1, 0))), ("empty output", dict(out_hw=(0, 8), out=None)),
           ("out too small", dict(out=z(N, 6, 7, 40))), ("out batch", dict(out=z(2, 6, 8, 40))),
           ("out rank", dict(out=z(6, 8, 40))), ("slot past the row", dict(out_channel_offset=24)),
           ("negative offset", dict(out_channel_offset=-8)), ("bias length", dict(bias=z(16, dtype=F32))),
           ("activation", dict(act="sigmoid")), ("tile", dict(cfg=7))]
    if dev.type == "cuda":
        cpu = torch.device("cpu")
        bad += [("pitch % 8", dict(out=z(N, 6, 8, 44))), ("offset % 8", dict(out_channel_offset=4)),
                ("x dtype", dict(x=z(N, Hi, Wi, Cin, dtype=F32))), ("w dtype", dict(w_packed=z(4 * Cin * Cout, dtype=F32))),
                ("out dtype", dict(out=z(N, 6, 8, 40, dtype=F32))), ("bias dtype", dict(bias=z(Cout))),
                ("w device", dict(w_packed=z(4 * Cin * Cout, device=cpu))), ("bias device", dict(bias=z(Cout, dtype=F32, device=cpu))),
                ("out device", dict(out=z(N, 6, 8, 40, device=cpu))),
                ("x not contiguous", dict(x=z(N, Hi, Wi, 2 * Cin)[..., ::2]))]
    return good, bad


def _assert_refusals(dev):
    good, bad = _bad_launches(dev)
    K.deconv2d_nhwc(**good)
    for what, over in bad:
        with pytest.raises((ValueError, TypeError)):
            K.deconv2d_nhwc(**{**good, **over})
            pytest.fail(f"not refused: {what}")


def test_launcher_rejects_bad_arguments_host():
    _assert_refusals(torch.device("cpu"))


# =================================================================================== CPU: lowering
def _imgs(n, hw, seed):
    return torch.randint(0, 256, (n, hw, hw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _margin(y):
    t = torch.topk(y, 2, -1).values
    return t[..., 0] - t[..., 1]


def _check_logits(got, ref):
    err = (got.float().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 0.05, err


def _check_labels(got, ref_up, ref_logits, cap=0.5):
    """``got`` agrees with the ArgMax of the interpreter's logits ``ref_up`` wherever their top-2
    margin is at least 0.1 max|logits|; at most ``cap`` of the pixels are excused."""
    must = _margin(ref_up) >= 0.1 * ref_logits.abs().max()
    assert (~must).double().mean() <= cap
    bad = (got.cpu().long() != torch.argmax(ref_up, -1)) & must
    assert got.shape == must.shape and not bad.any(), f"{int(bad.sum())} wrong labels"


class _G:
    """A small graph on a float feed ``x`` [2, 5, 6, Cin] (``r``: a second feed for the residual)."""

    def __init__(self, cin=16, seed=0):
        self.gb = GraphBuilder()
        self.rng = np.random.default_rng(seed)
        self.cin = cin
        self.x = self.gb.placeholder("x", "FLOAT", [None, 5, 6, cin])
        self.feeds = {"x:0": torch.from_numpy(self.rng.standard_normal((2, 5, 6, cin)).astype(np.float32))}

    def w(self, kh, kw, cout, cin=None, name="w"):
        cin = cin or self.cin
        return self.gb.constant(name, (self.rng.standard_normal((kh, kw, cout, cin)) * np.sqrt(2.0 / (cin * kh * kw / 2)))
                                .astype(np.float32))

    def vec(self, n, name, lo=-0.5, hi=0.5):
        return self.gb.constant(name, self.rng.uniform(lo, hi, n).astype(np.float32))

    def feed(self, name, shape):
        self.feeds[f"{name}:0"] = torch.from_numpy(self.rng.standard_normal(shape).astype(np.float32))
        return self.gb.placeholder(name, "FLOAT", [None, *shape[1:]])

    def compile(self, fetches, device="cpu", strict=True):
        specs = {k: (tuple(v.shape), "FLOAT") for k, v in self.feeds.items()}
        return CompiledFunction(self.gb.build(), specs, list(fetches), device, strict=strict)

    def reference(self, fetches):
        return Session(self.gb.build()).run(list(fetches), self.feeds)


def _g_chain():
    g = _G()
    y = g.gb.conv2d_transpose(g.x, g.w(2, 2, 24), (10, 12), (2, 2), "SAME", name="up")
    g.gb.relu(g.gb.bias_add(y, g.vec(24, "b"), name="bias"), name="y")
    return g, ["y:0"]


def _g_bn():
    g = _G()
    y = g.gb.conv2d_transpose(g.x, g.w(3, 3, 24), (9, 11), (2, 2), "SAME", name="up")
    y = g.gb.fused_batch_norm(y, g.vec(24, "gamma", 0.8, 1.2), g.vec(24, "beta"), g.vec(24, "mean"),
                              g.vec(24, "var", 0.8, 1.2), name="bn")
    g.gb.relu6(y, name="y")
    return g, ["y:0"]


def _g_sigmoid():
    g = _G()
    y = g.gb.conv2d_transpose(g.x, g.w(4, 4, 8), (10, 12), (2, 2), "SAME", name="up")
    g.gb.sigmoid(g.gb.bias_add(y, g.vec(8, "b"), name="bias"), name="y")
    return g, ["y:0"]


def _g_residual():
    g = _G()
    r = g.feed("r", (2, 10, 12, 16))
    y = g.gb.conv2d_transpose(g.x, g.w(2, 2, 16), (10, 12), (2, 2), "VALID", name="up")
    g.gb.relu(g.gb.add(g.gb.bias_add(y, g.vec(16, "b"), name="bias"), r, name="sum"), name="y")
    return g, ["y:0"]


def _g_stride1():
    g = _G()
    y = g.gb.conv2d_transpose(g.x, g.w(3, 3, 24), (5, 6), (1, 1), "SAME", name="up")
    g.gb.relu(g.gb.bias_add(y, g.vec(24, "b"), name="bias"), name="y")
    y2 = g.gb.conv2d_transpose(g.x, g.w(3, 2, 8, name="w2"), (7, 7), (1, 1), "VALID", name="up_valid")
    g.gb.bias_add(y2, g.vec(8, "b2"), name="y2")
    return g, ["y:0", "y2:0"]


def _g_cout3():
    g = _G()
    y = g.gb.conv2d_transpose(g.x, g.w(4, 4, 3), (10, 12), (2, 2), "SAME", name="up")
    g.gb.bias_add(y, g.vec(3, "b"), name="y")
    return g, ["y:0"]


def _g_padded_input():
    """An up-conv reading the 3-of-8-channel output of another one, in place."""
    g = _G()
    y = g.gb.conv2d_transpose(g.x, g.w(2, 2, 3), (10, 12), (2, 2), "SAME", name="up")
    y = g.gb.relu(g.gb.bias_add(y, g.vec(3, "b"), name="bias"), name="mid")
    g.gb.conv2d_transpose(y, g.w(3, 3, 8, cin=3, name="w2"), (20, 24), (2, 2), "SAME", name="y")
    return g, ["y:0"]


def _g_concat():
    g = _G()
    a = g.gb.conv2d_transpose(g.x, g.w(2, 2, 8, name="wa"), (10, 12), (2, 2), "SAME", name="up_a")
    a = g.gb.relu(g.gb.bias_add(a, g.vec(8, "ba"), name="bias_a"), name="relu_a")
    b = g.gb.conv2d_transpose(g.x, g.w(3, 3, 24, name="wb"), (10, 12), (2, 2), "SAME", name="up_b")
    c = g.gb.concat([a, b], 3, name="cat")
    wc = g.gb.constant("wc", (g.rng.standard_normal((1, 1, 32, 16)) * 0.25).astype(np.float32))
    g.gb.conv2d(c, wc, (1, 1), "SAME", name="y")
    return g, ["y:0"]


LOWERED = {"chain": _g_chain, "bn": _g_bn, "sigmoid": _g_sigmoid, "residual": _g_residual, "stride1": _g_stride1,
           "cout3": _g_cout3, "padded_input": _g_padded_input, "concat": _g_concat}


def _check_lowered(name, plan, g, fetches, dev="cpu"):
    s = plan.summary()
    kinds = s["kinds"]
    steps = {st.name: st for st in plan.steps}
    assert s["glue_ops"] == []
    if name in ("chain", "bn"):
        assert kinds.get("deconv") == 1 and "elementwise" not in kinds and "conv" not in kinds
        assert steps["up"].meta == {"phases": 4, "impl": "deconv"}
        mid = "bias:0" if name == "chain" else "bn:0"
        assert {"y"} <= plan._fused and plan._val_of("y:0") is plan._val_of(mid)         # the chain is one value
        assert ({"bias"} if name == "chain" else {"bn"}) <= plan._fused
    elif name == "sigmoid":
        assert kinds.get("deconv") == 1 and kinds.get("elementwise") == 1 and "bias" in plan._fused
        assert "y" not in plan._fused
    elif name == "residual":
        assert kinds.get("deconv") == 1 and kinds.get("elementwise", 0) >= 1 and "bias" in plan._fused
        assert "sum" not in plan._fused and "sum" in steps
    elif name == "stride1":
        assert "deconv" not in kinds and kinds.get("conv") == 2 and {"up", "up_valid"} <= set(steps)
    elif name == "cout3":
        v = plan._val_of("y:0")
        assert kinds.get("deconv") == 1 and tuple(v.shape) == (2, 10, 12, 3) and v.phys_c == 8
    elif name == "padded_input":
        assert kinds.get("deconv") == 2 and plan._val_of("mid:0").phys_c == 8
        assert not [n for n in steps if n.endswith("/pad_cin")]          # read in place
    elif name == "concat":
        assert kinds.get("deconv") == 2 and "concat" not in kinds
        cat = plan._val_of("cat:0")
        assert plan._val_of("relu_a:0").concat_slot == (cat, 0) and plan._val_of("up_b:0").concat_slot == (cat, 8)
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


def _glue_graph(case):
    """(graph holder, fetch) of one op the lowering leaves to glue."""
    g = _G(cin=12 if case == "cin12" else 16)
    gb = g.gb
    attrs = dict(strides=[1, 2, 2, 1], padding=b"SAME", data_format=b"NHWC", dilations=[1, 1, 1, 1])
    sizes = gb.constant("sizes", np.asarray([10, 12], dtype=np.int32))
    if case == "fed_filter":
        gb.op("Conv2DBackpropInput", [sizes, g.feed("wf", (2, 2, 8, 16)), g.x], name="y", **attrs)
        g.feeds["wf:0"] = g.feeds["wf:0"][:2]
    elif case == "dilations":
        s = gb.constant("sizes_d", np.asarray([9, 10], dtype=np.int32))
        gb.op("Conv2DBackpropInput", [s, g.w(3, 3, 8), g.x], name="y", **{**attrs, "strides": [1, 1, 1, 1],
                                                                           "padding": b"VALID", "dilations": [1, 2, 2, 1]})
    elif case == "explicit":
        gb.op("Conv2DBackpropInput", [sizes, g.w(4, 4, 8), g.x], name="y",
              **{**attrs, "padding": b"EXPLICIT", "explicit_paddings": [0, 0, 1, 1, 1, 1, 0, 0]})
    elif case == "nchw":
        xt = g.feed("xc", (2, 16, 5, 6))
        del g.feeds["x:0"]
        s = gb.constant("sizes_c", np.asarray([2, 8, 10, 12], dtype=np.int32))
        gb.op("Conv2DBackpropInput", [s, g.w(2, 2, 8), xt], name="y", **{**attrs, "strides": [1, 1, 2, 2],
                                                                         "data_format": b"NCHW"})
    elif case == "cin12":
        gb.op("Conv2DBackpropInput", [sizes, g.w(2, 2, 8), g.x], name="y", **attrs)
    elif case == "filter9":
        gb.op("Conv2DBackpropInput", [sizes, g.w(9, 9, 8), g.x], name="y", **attrs)
    elif case == "stride5":
        s = gb.constant("sizes_5", np.asarray([25, 30], dtype=np.int32))
        gb.op("Conv2DBackpropInput", [s, g.w(5, 5, 8), g.x], name="y", **{**attrs, "strides": [1, 5, 5, 1]})
    return g, ["y:0"]


GLUE = ("fed_filter", "dilations", "explicit", "nchw", "cin12", "filter9", "stride5")


@pytest.mark.parametrize("case", GLUE)
def test_what_stays_glue(case):
    g, fetches = _glue_graph(case)
    with pytest.raises(CompileError, match="Conv2DBackpropInput"):
        g.compile(fetches)
    plan = g.compile(fetches, strict=False)
    assert "Conv2DBackpropInput" in plan.summary()["glue_ops"] and "deconv" not in plan.summary()["kinds"]
    got, = plan(g.feeds)
    ref, = g.reference(fetches)
    assert got.shape == ref.shape
    _check_logits(got, ref)


def test_fed_input_sizes_stays_glue():
    """A computed ``input_sizes`` (Keras's ``Shape → StridedSlice → Pack``; here a fed vector) is
    refused under ``strict``.  It has no non-strict plan either: the glue path sizes its outputs
    by a dry run on zeros, and zero sizes are no output shape."""
    g = _G()
    s = g.gb.placeholder("sizes", "INT32", [2])
    g.gb.op("Conv2DBackpropInput", [s, g.w(2, 2, 8), g.x], name="y", strides=[1, 2, 2, 1], padding=b"SAME",
            data_format=b"NHWC", dilations=[1, 1, 1, 1])
    specs = {"x:0": ((2, 5, 6, 16), "FLOAT"), "sizes:0": ((2,), "INT32")}
    with pytest.raises(CompileError, match="Conv2DBackpropInput"):
        CompiledFunction(g.gb.build(), specs, ["y:0"], "cpu", strict=True)
    ref, = Session(g.gb.build()).run(["y:0"], {**g.feeds, "sizes:0": torch.tensor([10, 12], dtype=torch.int32)})
    assert ref.shape == (2, 10, 12, 8)      # the interpreter runs it


# =================================================================================== U-Net
UNET = dict(base=8, depth=2, num_classes=5, image_hw=(40, 40), crop_hw=(32, 32), seed=0)
UNET_KINDS = {"deconv": 2, "concat": 2, "pool": 2, "resize_argmax": 1, "conv": 4 * 2 + 3, "preprocess": 1}


@pytest.fixture(scope="module")
def unet():
    """The graph, three images and the fp32 interpreter's (logits, label_map): once."""
    from flink_tensorflow_amd.models.zoo import unet_graph_def

    g = Graph.from_graph_def(unet_graph_def(**UNET))
    imgs = _imgs(3, 40, seed=11)
    ref = Session(g).run(["logits:0", "label_map:0"], {"images:0": imgs})
    # the interpreter's own excused share and class count, before any plan runs
    assert (_margin(ref[0]) < 0.1 * ref[0].abs().max()).double().mean() <= 0.5
    assert len(torch.unique(ref[1])) > 1
    return g, imgs, ref


def _check_unet_plan(plan, imgs, ref, dev="cpu"):
    s = plan.summary()
    assert s["glue_ops"] == [] and "glue" not in s["kinds"] and "elementwise" not in s["kinds"]
    assert s["kinds"] == UNET_KINDS
    assert all(st.meta == {"phases": 4, "impl": "deconv"} for st in plan.steps if st.kind == "deconv")
    logits, labels = plan({"images:0": imgs.to(dev)})
    assert logits.shape == (3, 32, 32, 5) and labels.shape == (3, 32, 32) and labels.dtype == torch.uint8
    _check_logits(logits, ref[0])
    _check_labels(labels, ref[0], ref[0])
    return labels.cpu()


def _unet_plan(g, imgs, dev="cpu"):
    return CompiledFunction(g, {"images:0": (tuple(imgs.shape), "UINT8")}, ["logits:0", "label_map:0"], dev, strict=True)


def test_unet_plan_host(unet):
    g, imgs, ref = unet
    assert ref[0].shape == (3, 32, 32, 5) and ref[1].shape == (3, 32, 32) and ref[1].dtype == torch.uint8
    _check_unet_plan(_unet_plan(g, imgs), imgs, ref)


def test_unet_model_segments_on_the_host(unet):
    from flink_tensorflow_amd.models.zoo import UNetModel

    g, imgs, ref = unet
    plan_maps = _unet_plan(g, imgs)({"images:0": imgs})[1]
    m = UNetModel(buckets=(3,), device="cpu", **UNET)
    m.open()
    try:
        maps = m.segment(list(imgs.numpy()))
        (res, tags, _), = m.submit(list(imgs.numpy()), np.zeros(3), [5, 6, 7])
    finally:
        m.close()
    assert len(maps) == 3 and all(a.shape == (32, 32) and a.dtype == np.uint8 for a in maps)
    must = (_margin(ref[0]) >= 0.1 * ref[0].abs().max()).numpy()
    assert np.array_equal(np.stack(maps), ref[1].numpy())                # host: the interpreter
    assert np.array_equal(np.stack(maps)[must], plan_maps.numpy()[must])
    assert tags == [5, 6, 7] and np.array_equal(np.stack(res), np.stack(maps))


def test_unet_saved_model_compiles_strict(tmp_path, unet):
    from flink_tensorflow_amd.models import PredictMethod, SavedModelModel
    from flink_tensorflow_amd.models.zoo import export_unet_saved_model

    _, imgs, ref = unet
    d = export_unet_saved_model(str(tmp_path / "unet"), **UNET)
    m = SavedModelModel(d, device="cpu")
    m.open()
    try:
        interp = m.function("serving_default", PredictMethod(), compile=False)
        fn = m.function("serving_default", PredictMethod(), compile=True, batch_buckets=None)
        a, b = interp.apply({"images": imgs.numpy()}), fn.apply({"images": imgs.numpy()})
        s = fn.plan_summary()
    finally:
        m.close()
    assert s is not None and s["glue_ops"] == [] and s["kinds"]["deconv"] == 2
    assert torch.equal(torch.as_tensor(a["logits"]).float(), ref[0])       # the variables restore the weights
    _check_logits(torch.as_tensor(b["logits"]), ref[0])
    _check_labels(torch.as_tensor(b["label_map"]), ref[0], ref[0])


# =================================================================================== GPU: the kernel
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
    N, Hi, Wi, Cin, Cout = shape
    KH, KW, sh, sw, pt, pl, Ho, Wo = _geo(geom, Hi, Wi)
    x, w, b = _data(shape, geom, act == "relu6", bias)
    wp = K.deconv_pack_weights(w, (sh, sw), (pt, pl)).to(BF)
    assert torch.equal(wp.double(), K.deconv_pack_weights(w, (sh, sw), (pt, pl)))     # exact in bf16
    return K.deconv2d_nhwc(x.to(BF).to(dev), wp.to(dev), b.float().to(dev) if bias else None, (Ho, Wo), (KH, KW),
                           (sh, sw), (pt, 0, pl, 0), act, cfg=cfg, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_kernel_bit_exact(case):
    shape, geom = case
    dev = torch.device("cuda", 0)
    for act in ACTS:
        for bias in (False, True):
            want = _bits(_ref(shape, geom, act, bias)[1])
            for cfg in (-1, *K.DECONV_TILES.values()):
                y = _launch(shape, geom, act, bias, cfg, dev)
                assert y.dtype == BF and torch.equal(_bits(y.cpu()), want), (act, bias, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", list(GEOMS))
def test_kernel_guard_bands(geom):
    shape = SHAPES[1]
    N, Hi, Wi, Cin, Cout = shape
    KH, KW, sh, sw, pt, pl, Ho, Wo = _geo(geom, Hi, Wi)
    dev = torch.device("cuda", 0)
    nan = float("nan")
    x, w, b = _data(shape, geom, False, True)
    want = _bits(_ref(shape, geom, "relu", True)[1])
    xv, xbuf = _banded(x.to(BF), nan, dev)
    wv, wbuf = _banded(K.deconv_pack_weights(w, (sh, sw), (pt, pl)).to(BF), nan, dev)
    bv, bbuf = _banded(b.float(), nan, dev)
    coff, ldo = 16, 16 + Cout + 24
    for cfg in K.DECONV_TILES.values():
        ov, obuf = _banded(torch.full((N, Ho, Wo, ldo), SENT, dtype=BF), SENT, dev)
        y = K.deconv2d_nhwc(xv, wv, bv, (Ho, Wo), (KH, KW), (sh, sw), (pt, 0, pl, 0), "relu", out=ov,
                            out_channel_offset=coff, cfg=cfg)
        assert y is ov and _bands_intact(obuf, ov.numel(), SENT), "stray store"
        o = ov.cpu()
        assert torch.equal(_bits(o[..., coff:coff + Cout]), want)
        assert (o[..., :coff] == SENT).all() and (o[..., coff + Cout:] == SENT).all()   # outside the slice: untouched
    for buf, v in ((xbuf, xv), (wbuf, wv), (bbuf, bv)):
        assert _bands_intact(buf, v.numel(), nan)


@pytest.mark.gpu
def test_offsets_past_2_31():
    """One launch into a buffer of more than 2^31 elements (4x4/4 VALID, Cin = 8): the last
    output rows, whose element offsets need 64 bits, against the mirror."""
    dev = torch.device("cuda", 0)
    N, Hi, Wi, Cin, Cout = 1, 512, 512, 8, 8
    ldo, coff = 520, 504
    Ho, Wo = 4 * Hi, 4 * Wi
    assert Ho * Wo * ldo > 2 ** 31
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-8, 9, (N, Hi, Wi, Cin), generator=g).to(F64)
    w = torch.randint(-4, 5, (4, 4, Cout, Cin), generator=g).to(F64)
    b = torch.randint(-1200, 1201, (Cout,), generator=g).to(F64) / 2
    out = torch.empty((N, Ho, Wo, ldo), dtype=BF, device=dev)
    out[:, -8:].fill_(SENT)
    wp = K.deconv_pack_weights(w, (4, 4), (0, 0)).to(BF).to(dev)
    K.deconv2d_nhwc(x.to(BF).to(dev), wp, b.float().to(dev), (Ho, Wo), (4, 4), (4, 4), (0, 0, 0, 0), "none", out=out,
                    out_channel_offset=coff)
    tail = out[:, -8:].cpu()     # the last two input rows' outputs
    ref = _mirror_pre_rows(x[:, -2:], w) + b
    assert torch.equal(_bits(tail[..., coff:coff + Cout]), _bits(ref.to(F32).to(BF)))
    assert (tail[..., :coff] == SENT).all() and (tail[..., coff + Cout:] == SENT).all()
    del out
    torch.cuda.empty_cache()


def _mirror_pre_rows(x, w):
    """4x4/4 VALID of a few input rows: with k == s every output pixel has one tap and rows do
    not interact, so the last rows can be mirrored alone."""
    N, Hi, Wi, Cin = x.shape
    y = torch.zeros((N, 4 * Hi, 4 * Wi, w.shape[2]), dtype=F64)
    for ky in range(4):
        for kx in range(4):
            y[:, ky::4, kx::4] = x @ w[ky, kx].t()
    return y


@pytest.mark.gpu
def test_launcher_rejects_bad_arguments():
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
    """A transposed conv the lowering leaves to glue (a 9x9 filter) still runs in a captured
    plan: its ``input_sizes`` stays on the host, where the interpreter op reads it."""
    dev = torch.device("cuda", 0)
    g, fetches = _glue_graph("filter9")
    plan = g.compile(fetches, dev, strict=False)
    s = plan.summary()
    assert s["hip_graph"] and s["glue_ops"] == ["Conv2DBackpropInput"]
    got, = plan({k: v.to(dev) for k, v in g.feeds.items()})
    _check_logits(got, g.reference(fetches)[0])


@pytest.mark.gpu
def test_unet_plan_and_model_gpu(unet):
    from flink_tensorflow_amd.models.zoo import UNetModel

    g, imgs, ref = unet
    dev = torch.device("cuda", 0)
    plan = _unet_plan(g, imgs, dev)
    assert plan.summary()["hip_graph"]
    labels = _check_unet_plan(plan, imgs, ref, dev)
    again = plan({"images:0": imgs.to(dev)})
    assert torch.equal(again[1].cpu(), labels)            # a second replay is bit-identical
    m = UNetModel(buckets=(3,), lanes=1, **UNET)
    m.open()
    try:
        s = m.plan_summary()
        assert s["glue_ops"] == [] and s["kinds"]["deconv"] == 2
        maps = m.segment(list(imgs.numpy()))
        done = []
        for i in range(3):   # one record per batch: results come back in submission order
            done += m.submit([imgs[i].numpy()], np.zeros(1), [i])
        done += m.drain()
    finally:
        m.close()
    assert all(a.shape == (32, 32) and a.dtype == np.uint8 for a in maps)
    assert np.array_equal(np.stack(maps), labels.numpy())
    assert [t for _, tags, _ in done for t in tags] == [0, 1, 2]
    batched = np.stack([r for res, _, _ in done for r in res])
    must = (_margin(ref[0]) >= 0.1 * ref[0].abs().max()).numpy()
    assert batched.shape == (3, 32, 32) and batched.dtype == np.uint8
    assert np.array_equal(batched[must], labels.numpy()[must])
