"""Generator networks: the ``MirrorPad`` op, the instance-norm kernel (``kernels/instnorm.hip``),
the pad and image-output kernels (``kernels/pad.hip``), their launchers, the lowering
(``graph/generator_lowering.py``) and the style-transfer zoo model.

**Instance norm: the mirror.**  float64 from the definition: ``m`` the mean, ``v`` the biased variance
over ``H W`` of one image and channel, ``y = act((x - m) / sqrt(v + eps) * gamma + beta)``, rounded to
bf16 once.  ``x`` is given as bf16.

**Data**, seeded from the case: ``x ~ N(0, 1)`` rounded to bf16, ``gamma ~ U(0.5, 1.5)``, ``beta ~
0.5 N(0, 1)``, ``eps = 1e-5``.  The *offset* data set is ``x ~ 64 + N(0, 1)``: on it the naive
``E[x^2] - E[x]^2`` in fp32 loses the variance's low bits, on zero-mean data it does not.

**The tolerance** is measured, not chosen (``_host_error``), by the method of ``test_lstm.py``: over
every GPU case the launcher's fp32 host path differs from the mirror by at most ``E`` in at most a
share ``P`` of the elements.  ``E`` is in bf16 ulps at the mirror's value, the spacing taken at
``max(|y|, 2^-12)``: a smaller ``y`` is a difference of terms of order 1 whose fp32 error (about
2^-23 of them) does not shrink with it, and a ReLU's zero has no spacing at all.  The GPU tests allow ``A = max(4 E, 1 ulp)``
and a differing share of ``max(10 P, 1 %)``: the device's division and square root may be an fp32 ulp
off, which only moves more values across a bf16 rounding boundary.  Measured on the CPU:

    E = 1 ulp, P = 0.005 % of the elements of a case
    A = 4 ulp, allowed differing share 1 %

``test_instnorm_tolerance_cannot_hide_a_fault`` asserts that mirrors with one deliberate fault each
exceed ``4 A``, or the share cap, in a stated share of the elements.

**Cases** ``(N, H, W, C)`` of the GPU tests and the path of the kernel's decomposition each covers
(256 threads = R rows of L = C / 8 lanes, a chunk = 8 R pixels):

    (1, 1, 1, 8)        one pixel: every row but one is empty; the result is act(beta)
    (2, 7, 9, 24)       L = 3, R = 85: no power of two, rows partly filled, one chunk
    (3, 16, 16, 8)      L = 1, R = 256: the deepest row tree, one chunk
    (2, 67, 61, 16)     4 chunks with a short last one; also on the offset data
    (2, 33, 31, 40)     L = 5, R = 51, 3 chunks
    (1, 33, 32, 128)    9 chunks: a finalize slice merges two chunks before the slice tree
    (1, 3, 3, 2056)     C > 2048: two channel groups, the second one vector wide; R = 1, 2 chunks
"""
import functools
import zlib

import numpy as np
import pytest
import torch

from flink_tensorflow_amd.graph.builder import GraphBuilder
from flink_tensorflow_amd.graph.compiler import CompiledFunction, CompileError
from flink_tensorflow_amd.graph.graph import Graph
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.ops import kernels as K

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 2.0 ** 100          # output sentinel: exact in bf16 and fp32, far above any result
NAN = float("nan")
EPS = 1e-5

# ((N, H, W, C), offset data set)
IN_CASES = (((1, 1, 1, 8), False), ((2, 7, 9, 24), False), ((3, 16, 16, 8), False), ((2, 67, 61, 16), False),
            ((2, 67, 61, 16), True), ((2, 33, 31, 40), False), ((1, 33, 32, 128), False), ((1, 3, 3, 2056), False))
IN_ACTS = ("none", "relu", "relu6")


def _in_id(c):
    return "x".join(map(str, c[0])) + ("-offset" if c[1] else "")


@functools.lru_cache(maxsize=None)
def _in_data(shape, offset=False, scale=1.0, mean=64.0):
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, offset)).encode()))
    x = torch.randn(shape, generator=g, dtype=F64) * scale + (mean if offset else 0.0)
    C = shape[-1]
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).to(F32)
    beta = (torch.randn(C, generator=g, dtype=F64) * 0.5).to(F32)
    return x.to(BF), gamma, beta


def _act64(y, act):
    if act == "relu":
        return y.clamp_min(0)
    if act == "relu6":
        return y.clamp(0, 6)
    return y


def _in_mirror(x, gamma, beta, act="none", fault=None, eps=EPS):
    """The float64 mirror, rounded to bf16 once; ``fault`` plants one deliberate error."""
    xd, g, b = x.to(F64), gamma.to(F64), beta.to(F64)
    dims = (1,) if fault == "h_only" else (1, 2)
    m = xd.mean(dims, keepdim=True)
    v = ((xd - m) ** 2).mean(dims, keepdim=True)
    if fault == "unbiased":
        n = x.shape[1] * x.shape[2]
        v = v * n / (n - 1)
    if fault == "naive_fp32":
        xf = x.to(F32)
        mf = xf.mean((1, 2), keepdim=True)
        v = ((xf * xf).mean((1, 2), keepdim=True) - mf * mf).clamp_min(0).to(F64)
    if fault == "next_image":
        m, v = m.roll(1, 0), v.roll(1, 0)
    if fault == "next_channel":
        m, v = m.roll(1, 3), v.roll(1, 3)
    if fault == "swap_affine":
        g, b = b, g
    return _act64((xd - m) / torch.sqrt(v + eps) * g + b, act).to(BF)


def _ulps(got, ref):
    """``|got - ref|`` in bf16 ulps at the mirror's value (the spacing at ``max(|ref|, 2^-12)``)."""
    r = ref.to(F64).abs().clamp_min(2.0 ** -12)
    ulp = torch.exp2(torch.floor(torch.log2(r)) - 7)
    return (got.to(F64) - ref.to(F64)).abs() / ulp


def _in_diff(got, ref):
    u = _ulps(got, ref)
    return float(u.max()), float((u > 0).double().mean())


@functools.lru_cache(maxsize=None)
def _in_ref(case, act):
    return _in_mirror(*_in_data(*case), act)


@functools.lru_cache(maxsize=None)
def _host_error():
    """(E in bf16 ulps, P): the fp32 host path against the mirror over every GPU case."""
    e = p = 0.0
    for case in IN_CASES:
        x, gamma, beta = _in_data(*case)
        for act in IN_ACTS:
            a, pa = _in_diff(K.instance_norm(x, gamma, beta, EPS, act), _in_ref(case, act))
            e, p = max(e, a), max(p, pa)
    return e, p


def _bounds():
    """(A in bf16 ulps, allowed differing share): 4 E floored at 1 ulp, 10 P floored at 1 %."""
    e, p = _host_error()
    return max(4 * e, 1.0), max(10 * p, 0.01)


# =================================================================================== CPU: the ops
def _mirror_index(i, lo, size, mode):
    """The index formula of ``MirrorPad``: the source of output index ``i``."""
    r = i - lo
    if 0 <= r < size:
        return r
    if mode == "REFLECT":
        return -r if r < 0 else 2 * (size - 1) - r
    return -r - 1 if r < 0 else 2 * size - 1 - r


def _loop_mirror_pad(x, pads, mode):
    """MirrorPad by plain loops over the output, any rank."""
    x = np.asarray(x)
    out = np.empty([s + lo + hi for s, (lo, hi) in zip(x.shape, pads)], dtype=x.dtype)
    for idx in np.ndindex(*out.shape):
        out[idx] = x[tuple(_mirror_index(i, lo, s, mode) for i, (lo, _), s in zip(idx, pads, x.shape))]
    return out


def _run_mirror_pad(x, pads, mode):
    gb = GraphBuilder()
    p = gb.placeholder("x", "FLOAT", list(x.shape))
    gb.mirror_pad(p, pads, mode, name="y")
    return Session(gb.build()).run(["y:0"], {"x:0": torch.as_tensor(x)})[0]


@pytest.mark.parametrize("mode", ["REFLECT", "SYMMETRIC"])
def test_mirror_pad_nhwc_against_the_loop_mirror(mode):
    x = np.random.default_rng(1).standard_normal((2, 4, 5, 3)).astype(np.float32)
    pads = ((0, 0), (2, 1), (3, 0), (0, 0))
    got = _run_mirror_pad(x, pads, mode)
    assert tuple(got.shape) == (2, 7, 8, 3)
    assert np.array_equal(np.asarray(got), _loop_mirror_pad(x, pads, mode))


def test_mirror_pad_analytic_anchor():
    a, b, c = 1.0, 2.0, 3.0
    x = np.asarray([a, b, c], dtype=np.float32)
    assert _run_mirror_pad(x, ((2, 2),), "REFLECT").tolist() == [c, b, a, b, c, b, a]
    assert _run_mirror_pad(x, ((2, 2),), "SYMMETRIC").tolist() == [b, a, a, b, c, c, b]


def test_mirror_pad_bounds():
    x = np.zeros((2, 3), dtype=np.float32)
    assert tuple(_run_mirror_pad(x, ((1, 1), (2, 2)), "REFLECT").shape) == (4, 7)      # dim - 1 is allowed
    assert tuple(_run_mirror_pad(x, ((2, 2), (3, 3)), "SYMMETRIC").shape) == (6, 9)    # dim is allowed
    with pytest.raises(ValueError, match="axis 1"):
        _run_mirror_pad(x, ((0, 0), (3, 0)), "REFLECT")
    with pytest.raises(ValueError, match="axis 0"):
        _run_mirror_pad(x, ((0, 3), (0, 0)), "SYMMETRIC")


@pytest.mark.parametrize("mode", ["REFLECT", "SYMMETRIC"])
def test_mirror_pad_rank_2_and_rank_5(mode):
    rng = np.random.default_rng(2)
    for shape, pads in (((3, 4), ((2, 1), (0, 3))), ((2, 3, 2, 4, 3), ((1, 0), (2, 2), (0, 1), (3, 0), (1, 2)))):
        x = rng.standard_normal(shape).astype(np.float32)
        assert np.array_equal(np.asarray(_run_mirror_pad(x, pads, mode)), _loop_mirror_pad(x, pads, mode))


def test_pad_and_padv2_keep_their_behaviour():
    x = np.arange(12, dtype=np.float32).reshape(1, 2, 2, 3)
    pads = [[0, 0], [1, 0], [0, 2], [0, 0]]
    for value in (0, 1.5):
        gb = GraphBuilder()
        gb.pad(gb.placeholder("x", "FLOAT", [1, 2, 2, 3]), pads, value, name="y")
        g = gb.build()
        assert g["y"].op == ("Pad" if value == 0 else "PadV2")
        got, = Session(g).run(["y:0"], {"x:0": torch.as_tensor(x)})
        assert np.array_equal(np.asarray(got), np.pad(x, pads, constant_values=value))


def test_builder_instance_norm_is_the_float64_formula():
    shape = (2, 5, 7, 16)
    x, gamma, beta = _in_data(shape)
    gb = GraphBuilder()
    p = gb.placeholder("x", "FLOAT", list(shape))
    y = gb.instance_norm(p, gb.constant("gamma", gamma.numpy()), gb.constant("beta", beta.numpy()), EPS, name="IN")
    g = gb.build()
    ops = [n.op for n in g.nodes.values() if n.name.startswith("IN/")]
    assert sorted(o for o in ops if o != "Const") == sorted(
        ["Mean", "StopGradient", "SquaredDifference", "Mean", "Add", "Rsqrt", "Mul", "Mul", "Mul", "Sub", "Add"])
    got, = Session(g).run([y], {"x:0": x.float()})
    xd = x.to(F64)
    m = xd.mean((1, 2), keepdim=True)
    v = ((xd - m) ** 2).mean((1, 2), keepdim=True)
    want = (xd - m) / torch.sqrt(v + EPS) * gamma.to(F64) + beta.to(F64)
    assert float((torch.as_tensor(got).to(F64) - want).abs().max()) <= 1e-5
    assert GraphBuilder().tanh("x:0").startswith("Tanh") and GraphBuilder().clip_by_value("x:0", 0, 1) == "clip_by_value:0"


# =================================================================================== CPU: the launchers
@pytest.mark.parametrize("case", IN_CASES, ids=_in_id)
def test_instnorm_host_path_is_the_mirror(case):
    """The fp32 host path against the float64 mirror: at most one bf16 ulp apart, in well under
    1 % of the elements."""
    x, gamma, beta = _in_data(*case)
    for act in IN_ACTS:
        got = K.instance_norm(x, gamma, beta, EPS, act)
        assert got.dtype == BF and got.shape == x.shape
        e, p = _in_diff(got, _in_ref(case, act))
        assert e <= 1.0 and p < 0.01, (act, e, p)
    if case[0][1:3] == (1, 1):
        assert torch.equal(K.instance_norm(x, gamma, beta, EPS, "relu"), beta.clamp_min(0).to(BF).expand(x.shape))


def test_instnorm_measured_tolerance():
    e, p = _host_error()
    a, share = _bounds()
    print(f"E = {e:g} bf16 ulp, P = {p:.5f}; A = {a:g} ulp, allowed differing share = {share:.4f}")
    assert 0 < e <= 1.0 and a == 4.0 and p <= 0.002 and share <= 0.02


def test_instnorm_tolerance_cannot_hide_a_fault():
    """Mirrors with one deliberate fault against the true mirror: the share of elements beyond
    ``4 A`` and the differing share, of which one must exceed its stated floor or the share cap.
    Seen at (2, 33, 31, 40): the neighbouring image's statistics 30 % beyond 4 A, the neighbouring
    channel's 30 %, statistics over H only 70 %, gamma / beta swapped 90 %.  At (2, 7, 9, 24) the
    unbiased variance moves 86 % of the elements (by a few ulps: it is caught by the share cap, not
    by 4 A).  On the offset data at (2, 67, 61, 16) the naive fp32 variance moves 2.9 %, each by one
    ulp: the share cap again."""
    a, cap = _bounds()

    def shares(case, fault, act="none"):
        x, gamma, beta = _in_data(*case)
        u = _ulps(_in_mirror(x, gamma, beta, act, fault), _in_ref(case, act))
        far, any_ = float((u > 4 * a).double().mean()), float((u > 0).double().mean())
        print(f"{_in_id(case)} {fault}: {far:.3f} beyond {4 * a:g} ulp, {any_:.4f} differ (cap {cap:.4f})")
        return far, any_

    for fault in ("next_image", "next_channel", "h_only", "swap_affine"):
        far, _ = shares(((2, 33, 31, 40), False), fault)
        assert far >= 0.10, (fault, far)
    _, moved = shares(((2, 7, 9, 24), False), "unbiased")
    assert moved >= 0.20 and moved > cap
    _, moved = shares(((2, 67, 61, 16), True), "naive_fp32")
    assert moved >= 0.02 and moved > cap
    # the centred fp32 host path on the same data: every element equals the mirror
    case = ((2, 67, 61, 16), True)
    assert _in_diff(K.instance_norm(*_in_data(*case), EPS), _in_ref(case, "none")) == (0.0, 0.0)


def test_instnorm_host_path_writes_a_channel_slice():
    shape = (2, 7, 9, 24)
    x, gamma, beta = _in_data(shape)
    wide = torch.full((2, 7, 9, 48), SENT, dtype=BF)
    K.instance_norm(x, gamma, beta, EPS, "relu", out=wide, out_channel_offset=16)
    assert torch.equal(wide[..., 16:40], K.instance_norm(x, gamma, beta, EPS, "relu"))
    assert (wide[..., :16] == SENT).all() and (wide[..., 40:] == SENT).all()
    assert K.instance_norm_scratch_numel(2, 67, 61, 16) == 2 * 4 * 16 * 2 + 2 * 16 * 2
    assert K.instance_norm_eligible(1, 1, 8) and not K.instance_norm_eligible(4, 4, 12) \
        and not K.instance_norm_eligible(0, 4, 8)


def test_launchers_reject_malformed_calls():
    x, gamma, beta = _in_data((2, 7, 9, 24))
    with pytest.raises(ValueError):
        K.instance_norm(x[..., :12].contiguous(), gamma[:12], beta[:12])       # C % 8
    with pytest.raises(ValueError):
        K.instance_norm(x, gamma[:8], beta)
    with pytest.raises(ValueError):
        K.instance_norm(x, gamma, beta, act="tanh")
    with pytest.raises(TypeError):
        K.instance_norm(x.float(), gamma, beta)
    with pytest.raises(TypeError):
        K.instance_norm(x, gamma.to(BF), beta)
    with pytest.raises(ValueError):
        K.instance_norm(x, gamma, beta, out=torch.empty((2, 7, 9, 32), dtype=BF), out_channel_offset=16)
    with pytest.raises(ValueError):
        K.instance_norm(x[0], gamma, beta)
    with pytest.raises(ValueError):
        K.instance_norm_scratch_numel(1, 4, 4, 12)
    with pytest.raises(ValueError):
        K.pad_nhwc(x, (1, 1, 1, 1), "edge")
    with pytest.raises(ValueError):
        K.pad_nhwc(x, (7, 0, 0, 0), "reflect")        # at most H - 1
    with pytest.raises(ValueError):
        K.pad_nhwc(x, (0, 0, 0, 10), "symmetric")     # at most W
    with pytest.raises(ValueError):
        K.pad_nhwc(x, (1, 1, 1), "constant")
    with pytest.raises(ValueError):
        K.pad_nhwc(x, (-1, 0, 0, 0), "constant")
    with pytest.raises(TypeError):
        K.pad_nhwc(x.float(), (1, 1, 1, 1), "constant")
    with pytest.raises(ValueError):
        K.pad_nhwc(x, (1, 1, 1, 1), "constant", out=torch.empty((2, 9, 10, 24), dtype=BF))
    with pytest.raises(ValueError):
        K.pad_nhwc(x, (0, 0, 0, 0), "constant", channels=25)
    with pytest.raises(ValueError):
        K.image_out(x, 2)
    with pytest.raises(ValueError):
        K.image_out(x, 3, act="relu")
    with pytest.raises(ValueError):
        K.image_out(x, 3, dtype=torch.uint8)                       # no clamp
    with pytest.raises(ValueError):
        K.image_out(x, 3, clamp=(0.0, 256.0), dtype=torch.uint8)   # outside [0, 255]
    with pytest.raises(ValueError):
        K.image_out(x, 3, clamp=(2.0, 1.0))
    with pytest.raises(TypeError):
        K.image_out(x, 3, dtype=torch.int32)
    with pytest.raises(TypeError):
        K.image_out(x.float(), 3)
    with pytest.raises(ValueError):
        K.image_out(x, 3, out=torch.empty((2, 7, 9, 4)))


# ---- pad_nhwc: index mirrors
PAD_SHAPES = ((2, 5, 6, 8), (1, 9, 4, 24))
PAD_MODES = ("constant", "reflect", "symmetric")


def _pad_cases():
    """(shape, pads (top, bottom, left, right), mode): the two pad sets on both shapes in every
    mode, and per shape the extreme pads of each mirror mode (H - 1 / W - 1 reflect, H / W symmetric)."""
    out = [(s, p, m) for s in PAD_SHAPES for p in ((3, 3, 3, 3), (2, 1, 0, 3)) for m in PAD_MODES]
    for s in PAD_SHAPES:
        out.append((s, (s[1] - 1, s[1] - 1, s[2] - 1, s[2] - 1), "reflect"))
        out.append((s, (s[1], s[1], s[2], s[2]), "symmetric"))
    return out


def _pad_id(c):
    return "x".join(map(str, c[0])) + "-" + "_".join(map(str, c[1])) + "-" + c[2]


def _pad_mirror(x, pads, mode, value=0.0, channels=None):
    """``pad_nhwc`` by loops over the output pixels, from the index formula."""
    N, H, W, C = x.shape
    pt, pb, pl, pr = pads
    fill = torch.zeros(C, dtype=x.dtype)
    fill[:C if channels is None else channels] = torch.tensor(value).to(x.dtype)
    out = torch.empty((N, H + pt + pb, W + pl + pr, C), dtype=x.dtype)
    for i in range(out.shape[1]):
        for j in range(out.shape[2]):
            if mode == "constant":
                inside = 0 <= i - pt < H and 0 <= j - pl < W
                out[:, i, j] = x[:, i - pt, j - pl] if inside else fill
            else:
                out[:, i, j] = x[:, _mirror_index(i, pt, H, mode.upper()), _mirror_index(j, pl, W, mode.upper())]
    return out


@functools.lru_cache(maxsize=None)
def _pad_data(shape):
    g = torch.Generator().manual_seed(zlib.crc32(repr(("pad", shape)).encode()))
    return torch.randn(shape, generator=g).to(BF)


@pytest.mark.parametrize("case", _pad_cases(), ids=_pad_id)
def test_pad_host_path_is_the_index_mirror(case):
    shape, pads, mode = case
    x = _pad_data(shape)
    assert torch.equal(K.pad_nhwc(x, pads, mode, value=1.5), _pad_mirror(x, pads, mode, 1.5))
    if mode != "constant":   # and the interpreter's MirrorPad is the same function
        tf_pads = ((0, 0), pads[:2], pads[2:], (0, 0))
        assert torch.equal(torch.as_tensor(_run_mirror_pad(x.float().numpy(), tf_pads, mode.upper())).to(BF),
                           K.pad_nhwc(x, pads, mode))


def test_pad_host_path_padded_channels_and_slot():
    x = _pad_data((2, 5, 6, 8)).clone()
    x[..., 3:] = 0                              # 3 logical channels over 8 physical ones
    got = K.pad_nhwc(x, (1, 2, 3, 0), "constant", value=2.0, channels=3)
    assert torch.equal(got, _pad_mirror(x, (1, 2, 3, 0), "constant", 2.0, channels=3))
    assert (got[..., 3:] == 0).all() and (got[:, 0, :, :3] == 2.0).all()
    wide = torch.full((2, 8, 9, 24), SENT, dtype=BF)
    K.pad_nhwc(x, (1, 2, 3, 0), "symmetric", out=wide, out_channel_offset=8)
    assert torch.equal(wide[..., 8:16], _pad_mirror(x, (1, 2, 3, 0), "symmetric"))
    assert (wide[..., :8] == SENT).all() and (wide[..., 16:] == SENT).all()


# ---- image_out: float64 mirrors that round where the kernel rounds
IMG_SHAPES = ((2, 5, 7), (1, 3, 3), (3, 8, 8))     # (N, H, W): 70 and 9 pixels (tails of 2 and 1), 192 (none)
IMG_CASES = [(s, cl, act, dt) for s in IMG_SHAPES for cl in (1, 3, 4) for act in (None, "tanh", "sigmoid")
             for dt in (torch.uint8, F32)]


def _img_id(c):
    return "x".join(map(str, c[0])) + f"-c{c[1]}-{c[2] or 'none'}-{str(c[3]).split('.')[-1]}"


def _img_params(act):
    """(scale, offset, clamp): a grid on which the fp32 arithmetic of ``act = None`` is exact, the
    pixel range of the activation otherwise."""
    return {None: (0.5, 64.0, (0.0, 255.0)), "tanh": (127.5, 127.5, (0.0, 255.0)), "sigmoid": (255.0, 0.0, (0.0, 255.0))}[act]


@functools.lru_cache(maxsize=None)
def _img_data(shape, act):
    """bf16 ``[N, H, W, 8]``: integers in [-256, 256] for ``act = None`` (x / 2 + 64 is then exact in
    fp32 and crosses both clamp ends), ``2 N(0, 1)`` otherwise; the padding channels hold NaN, which
    the kernel must not let through."""
    g = torch.Generator().manual_seed(zlib.crc32(repr(("img", shape, act)).encode()))
    if act is None:
        x = torch.randint(-256, 257, (*shape, 8), generator=g).to(BF)
    else:
        x = (torch.randn((*shape, 8), generator=g) * 2).to(BF)
    return x


def _img_mirror(x, cl, act, scale, offset, clamp, dtype):
    """float64, rounded to fp32 after the activation, the product and the sum; uint8 truncates."""
    v = x[..., :cl].to(F64)
    v = torch.tanh(v) if act == "tanh" else torch.sigmoid(v) if act == "sigmoid" else v
    v = v.to(F32).to(F64) * float(np.float32(scale))
    v = v.to(F32).to(F64) + float(np.float32(offset))
    v = v.to(F32)
    if clamp is not None:
        v = v.clamp(*clamp)
    return v.to(torch.int32).to(torch.uint8) if dtype == torch.uint8 else v


def _img_input(shape, cl, act):
    x = _img_data(shape, act).clone()
    x[..., cl:] = NAN
    return x


@functools.lru_cache(maxsize=None)
def _img_host_error():
    """E: the largest difference of the fp32 host path from the mirror over the fp32 tanh / sigmoid cases."""
    e = 0.0
    for shape, cl, act, dt in IMG_CASES:
        if act is not None and dt == F32:
            x = _img_input(shape, cl, act)
            got = K.image_out(x, cl, act, *_img_params(act), dtype=dt)
            e = max(e, float((got.to(F64) - _img_mirror(x, cl, act, *_img_params(act), dt).to(F64)).abs().max()))
    return e


def _img_atol():
    """``max(4 E, one fp32 ulp of the largest pixel value)`` = ``max(4 E, 2^-16)``."""
    return max(4 * _img_host_error(), 2.0 ** -16)


def _check_image(got, x, case):
    shape, cl, act, dt = case
    ref = _img_mirror(x, cl, act, *_img_params(act), dt)
    assert got.dtype == dt and tuple(got.shape) == (*shape, cl)
    if act is None:
        assert torch.equal(got, ref)
    elif dt == torch.uint8:
        assert int((got.int() - ref.int()).abs().max()) <= 1
    else:
        assert torch.isfinite(got).all() and float((got.to(F64) - ref.to(F64)).abs().max()) <= _img_atol()


@pytest.mark.parametrize("case", IMG_CASES, ids=_img_id)
def test_image_out_host_path_is_the_mirror(case):
    shape, cl, act, dt = case
    x = _img_input(shape, cl, act)
    _check_image(K.image_out(x, cl, act, *_img_params(act), dtype=dt), x, case)


def test_image_out_measured_tolerance():
    e = _img_host_error()
    print(f"E = {e:g} (fp32 host path vs the mirror, tanh / sigmoid pixels); allowed {_img_atol():g}")
    assert e <= 2.0 ** -14 and _img_atol() <= 2.0 ** -12
    # without a clamp the fp32 image is the affine map itself
    x = _img_input((1, 3, 3), 3, None)
    assert torch.equal(K.image_out(x, 3, None, 0.5, 64.0), x[..., :3].float() * 0.5 + 64.0)


# =================================================================================== the lowering
class _G:
    """A small graph: a fed fp32 activation ``x`` and helpers that add constants."""

    def __init__(self, shape=(2, 9, 7, 16), seed=0):
        self.gb = GraphBuilder()
        self.rng = np.random.default_rng(seed)
        self.shape = shape
        self.x = self.gb.placeholder("x", "FLOAT", list(shape))
        self.feeds = {"x:0": torch.from_numpy(self.rng.standard_normal(shape).astype(np.float32))}
        self.specs = {"x:0": (tuple(shape), "FLOAT")}

    def const(self, name, *shape, scale=1.0, shift=0.0):
        return self.gb.constant(name, (self.rng.standard_normal(shape) * scale + shift).astype(np.float32))

    def norm(self, x, c, name, shaped=False):
        g = self.const(f"{name}/gamma", *((1, 1, 1, c) if shaped else (c,)), scale=0.2, shift=1.0)
        b = self.const(f"{name}/beta", *((1, 1, 1, c) if shaped else (c,)), scale=0.3)
        return self.gb.instance_norm(x, g, b, EPS, name=name)

    def conv(self, x, k, cin, cout, name, padding="SAME", bias=False):
        y = self.gb.conv2d(x, self.const(f"{name}/w", k, k, cin, cout, scale=(2.0 / (k * k * cin)) ** 0.5), (1, 1), padding,
                           name=name)
        return self.gb.bias_add(y, self.const(f"{name}/b", cout, scale=0.1), name=f"{name}/BiasAdd") if bias else y

    def compile(self, fetches, dev="cpu", strict=True):
        return CompiledFunction(self.gb.build(), self.specs, fetches, dev, strict=strict)

    def reference(self, fetches):
        return Session(self.gb.build()).run(fetches, self.feeds)

    def check(self, fetches, dev, want, absent=(), atol=0.06):
        """Strict plan on ``dev``: no glue op, the kinds of ``want``, none of ``absent``; the results
        against the fp32 interpreter (bf16 activations: ``atol`` on values of order 1)."""
        plan = self.compile(fetches, dev)
        s = plan.summary()
        assert s["glue_ops"] == [] and s["hip_graph"] == (dev != "cpu")
        assert {k: s["kinds"].get(k, 0) for k in want} == want and not set(absent) & set(s["kinds"]), s["kinds"]
        outs = plan({k: v.to(dev) for k, v in self.feeds.items()})
        for o, r in zip(outs, self.reference(fetches)):
            r = torch.as_tensor(r)
            assert tuple(o.shape) == tuple(r.shape)
            assert float((o.cpu().double() - r.double()).abs().max()) <= atol, s["kinds"]
        return plan, outs


def _image_graph(with_cast, hw=(12, 12)):
    """uint8 images → preprocess → MirrorPad(2) → 5x5 VALID conv to 8 → instance norm + Relu → 3x3
    conv to 3 + bias → Tanh → Mul → Add → ClipByValue [→ Cast]."""
    g = _G((2, 4, 4, 8))
    gb = g.gb
    img = gb.placeholder("images", "UINT8", [None, *hw, 3])
    g.feeds = {"images:0": torch.from_numpy(g.rng.integers(0, 256, (2, *hw, 3), dtype=np.uint8))}
    g.specs = {"images:0": ((2, *hw, 3), "UINT8")}
    x = gb.div(gb.sub(gb.cast(img, "FLOAT", name="Cast"), gb.constant("mean", np.float32(127.5)), name="Sub"),
               gb.constant("std", np.float32(127.5)), name="normalized")
    x = gb.mirror_pad(x, [[0, 0], [2, 2], [2, 2], [0, 0]], "SYMMETRIC", name="mp")
    x = g.conv(x, 5, 3, 8, "c1", "VALID")
    x = gb.relu(g.norm(x, 8, "in1"), name="relu1")
    x = g.conv(x, 3, 8, 3, "rgb", "SAME", bias=True)
    y = gb.tanh(x, name="Tanh")
    y = gb.mul(y, gb.constant("scale", np.float32(127.5)), name="Mul")
    y = gb.add(y, gb.constant("offset", np.float32(127.5)), name="Add")
    y = gb.clip_by_value(y, 0.0, 255.0, name="pixels")
    if with_cast:
        gb.cast(y, "UINT8", name="bytes")
    return g


def _check_lowerings(dev):
    # a lone instance norm, without and with the ReLU, [C] and [1, 1, 1, C] parameters
    g = _G()
    g.norm(g.x, 16, "in0")
    g.check(["in0/instancenorm/add_1:0"], dev, {"instnorm": 1}, ("elementwise", "gap"))
    g = _G()
    g.gb.relu(g.norm(g.x, 16, "in0", shaped=True), name="y")
    plan, _ = g.check(["y:0"], dev, {"instnorm": 1}, ("elementwise", "gap"))
    assert [s.meta["act"] for s in plan.steps if s.kind == "instnorm"] == [K.ACT_RELU]
    # Relu6; a fetched norm keeps its Relu a step of its own
    g = _G()
    g.gb.relu6(g.norm(g.x, 16, "in0"), name="y")
    plan, _ = g.check(["y:0"], dev, {"instnorm": 1}, ("elementwise",))
    assert [s.meta["act"] for s in plan.steps if s.kind == "instnorm"] == [K.ACT_RELU6]
    g = _G()
    g.gb.relu(g.norm(g.x, 16, "in0"), name="y")
    g.check(["in0/instancenorm/add_1:0", "y:0"], dev, {"instnorm": 1, "elementwise": 1})
    # two norms into a concat: the slices are written in place, no copy step
    g = _G()
    a = g.gb.relu(g.norm(g.x, 16, "in_a"), name="ra")
    b = g.norm(g.conv(g.x, 1, 16, 8, "cb"), 8, "in_b")
    g.gb.concat([a, b], 3, name="cat")
    plan, (cat,) = g.check(["cat:0"], dev, {"instnorm": 2, "conv": 1}, ("concat", "elementwise"))
    assert tuple(cat.shape) == (2, 9, 7, 24)
    # the norm's input is a concat operand too: it keeps a buffer of its own (the kernel reads a
    # pitch of C), so the concat is a copy step; the norm itself may still write its slice
    g = _G()
    a = g.conv(g.x, 1, 16, 8, "ca")
    g.gb.concat([a, g.norm(a, 8, "in_a")], 3, name="cat")
    _, (cat,) = g.check(["cat:0"], dev, {"conv": 1, "instnorm": 1, "concat": 1})
    assert tuple(cat.shape) == (2, 9, 7, 16)
    g = _G()
    n1 = g.norm(g.x, 16, "in1")
    g.gb.concat([n1, g.gb.relu(g.norm(n1, 16, "in2"), name="r2")], 3, name="cat")
    _, (cat,) = g.check(["cat:0"], dev, {"instnorm": 2, "concat": 1}, ("elementwise",))
    assert tuple(cat.shape) == (2, 9, 7, 32)
    # a residual Add behind the norm stays an elementwise step
    g = _G()
    g.gb.add(g.x, g.norm(g.conv(g.x, 3, 16, 16, "c"), 16, "in0"), name="y")
    g.check(["y:0"], dev, {"conv": 1, "instnorm": 1, "elementwise": 1})
    # a constant Pad (TF-slim's conv2d_same) and a PadV2, into a concat
    g = _G()
    p0 = g.gb.pad(g.x, [[0, 0], [1, 0], [2, 1], [0, 0]], name="p0")
    p1 = g.gb.pad(g.x, [[0, 0], [0, 1], [0, 3], [0, 0]], value=-1.5, name="p1")
    g.gb.concat([p0, p1], 3, name="cat")
    plan, _ = g.check(["cat:0"], dev, {"pad": 2}, ("concat",), atol=0.02)
    assert sorted(g.gb.build()[n].op for n in ("p0", "p1")) == ["Pad", "PadV2"]
    # MirrorPad over the preprocess output, the output stage without and with the Cast
    for with_cast in (False, True):
        g = _image_graph(with_cast)
        fetch = "bytes:0" if with_cast else "pixels:0"
        plan, (img,) = g.check([fetch], dev, {"preprocess": 1, "pad": 1, "conv": 2, "instnorm": 1, "image_out": 1},
                               ("elementwise", "glue"), atol=6.0)      # pixel counts: bf16 convs under a slope of 127.5
        assert img.dtype == (torch.uint8 if with_cast else F32) and tuple(img.shape) == (2, 12, 12, 3)
        step = [s for s in plan.steps if s.kind == "image_out"][0]
        assert step.meta["act"] == "tanh" and step.meta["dtype"] == str(img.dtype)
        assert [s.meta["mode"] for s in plan.steps if s.kind == "pad"] == ["symmetric"]
    # a BERT-style last-axis layer_norm next to an instance norm keeps its layernorm step
    from flink_tensorflow_amd.models.zoo.bert_graph import layer_norm

    g = _G()
    y = g.gb.reshape(g.norm(g.x, 16, "in0"), [-1, 16], name="rows")
    layer_norm(g.gb, y, g.const("ln/gamma", 16, scale=0.2, shift=1.0), g.const("ln/beta", 16, scale=0.3), 1e-12, "ln")
    g.check(["ln/batchnorm/add_1:0"], dev, {"instnorm": 1, "layernorm": 1}, ("elementwise",))


def test_lowerings_host():
    _check_lowerings("cpu")


@pytest.mark.gpu
def test_lowerings_gpu():
    _check_lowerings("cuda")


def _refusal_graph(kind):
    """-> (graph, fetch, an op that must stay glue)."""
    g = _G()
    gb = g.gb
    if kind == "other_axes":        # moments over H only
        x, gamma, beta = g.x, g.const("gamma", 16, shift=1.0, scale=0.2), g.const("beta", 16, scale=0.3)
        ax = gb.constant("ax", np.asarray([1], np.int32))
        mean = gb.op("Mean", [x, ax], name="mean", keep_dims=True)
        sq = gb.op("SquaredDifference", [x, gb.op("StopGradient", [mean], name="sg")], name="sq")
        var = gb.op("Mean", [sq, gb.constant("ax2", np.asarray([1], np.int32))], name="var", keep_dims=True)
        inv = gb.mul(gb.op("Rsqrt", [gb.add(var, gb.constant("eps", np.float32(EPS)), name="ve")], name="rs"), gamma,
                     name="inv")
        gb.add(gb.mul(x, inv, name="m1"), gb.sub(beta, gb.mul(mean, inv, name="m2"), name="sh"), name="y")
        return g, "y:0", "SquaredDifference"
    if kind == "padded_input":      # 12 channels over a 16-channel buffer
        y = g.conv(g.x, 1, 16, 12, "c")
        gb.identity(g.norm(y, 12, "in0"), name="y")
        return g, "y:0", "SquaredDifference"
    if kind == "fed_gamma":
        gamma = gb.placeholder("gamma", "FLOAT", [16])
        g.feeds["gamma:0"] = torch.from_numpy(g.rng.uniform(0.5, 1.5, 16).astype(np.float32))
        g.specs["gamma:0"] = ((16,), "FLOAT")
        gb.identity(gb.instance_norm(g.x, gamma, g.const("beta", 16, scale=0.3), EPS, name="in0"), name="y")
        return g, "y:0", "SquaredDifference"
    if kind == "handwritten":       # (x - mu) / sqrt(var + eps) * gamma + beta
        ax = gb.constant("ax", np.asarray([1, 2], np.int32))
        mu = gb.op("Mean", [g.x, ax], name="mu", keep_dims=True)
        d = gb.sub(g.x, mu, name="d")
        var = gb.op("Mean", [gb.mul(d, d, name="dd"), ax], name="var", keep_dims=True)
        sd = gb.op("Sqrt", [gb.add(var, gb.constant("eps", np.float32(EPS)), name="ve")], name="sd")
        y = gb.op("RealDiv", [d, sd], name="n")
        gb.add(gb.mul(y, g.const("gamma", 16, shift=1.0, scale=0.2), name="sc"), g.const("beta", 16, scale=0.3), name="y")
        return g, "y:0", "Sqrt"
    if kind == "group_norm":        # reshape to [N, H, W, G, C / G], moments over (1, 2, 4)
        x5 = gb.reshape(g.x, [2, 9, 7, 4, 4], name="x5")
        ax = gb.constant("ax", np.asarray([1, 2, 4], np.int32))
        mean = gb.op("Mean", [x5, ax], name="mean", keep_dims=True)
        sq = gb.op("SquaredDifference", [x5, gb.op("StopGradient", [mean], name="sg")], name="sq")
        var = gb.op("Mean", [sq, gb.constant("ax2", np.asarray([1, 2, 4], np.int32))], name="var", keep_dims=True)
        inv = gb.mul(gb.op("Rsqrt", [gb.add(var, gb.constant("eps", np.float32(EPS)), name="ve")], name="rs"),
                     g.const("gamma", 1, 1, 1, 4, 4, shift=1.0, scale=0.2), name="inv")
        y5 = gb.add(gb.mul(x5, inv, name="m1"), gb.sub(g.const("beta", 1, 1, 1, 4, 4, scale=0.3),
                                                       gb.mul(mean, inv, name="m2"), name="sh"), name="y5")
        gb.reshape(y5, [2, 9, 7, 16], name="y")
        return g, "y:0", "Mean"
    if kind == "pad_channels":
        gb.mirror_pad(g.x, [[0, 0], [1, 1], [1, 1], [0, 8]], "REFLECT", name="y")
        return g, "y:0", "MirrorPad"
    if kind == "pad_batch":
        gb.pad(g.x, [[1, 0], [1, 1], [1, 1], [0, 0]], name="y")
        return g, "y:0", "Pad"
    if kind == "fed_paddings":
        p = gb.placeholder("p", "INT32", [4, 2])
        # captured glue sizes its buffers by a dry run on zeros (as before this change), so zero
        # paddings are the only ones such a plan can be fed
        g.feeds["p:0"] = torch.zeros((4, 2), dtype=torch.int32)
        g.specs["p:0"] = ((4, 2), "INT32")
        gb.op("MirrorPad", [g.x, p], name="y", mode=b"REFLECT")
        return g, "y:0", "MirrorPad"
    raise AssertionError(kind)


REFUSALS = ("other_axes", "padded_input", "fed_gamma", "handwritten", "group_norm", "pad_channels", "pad_batch",
            "fed_paddings")


@pytest.mark.parametrize("kind", REFUSALS)
def test_lowering_refusals(kind):
    """What stays glue: a ``CompileError`` under ``strict``, the op in ``glue_ops`` otherwise, no step
    of the new kinds, and the non-strict plan still the interpreter's function (bf16 values)."""
    g, fetch, op = _refusal_graph(kind)
    with pytest.raises(CompileError, match="no CDNA4 lowering"):
        g.compile([fetch], strict=True)
    plan = g.compile([fetch], strict=False)
    s = plan.summary()
    assert op in s["glue_ops"] and not {"instnorm", "pad", "image_out"} & set(s["kinds"]), s
    got, = plan(g.feeds)
    ref, = g.reference([fetch])
    assert tuple(got.shape) == tuple(ref.shape)
    assert float((got.double() - torch.as_tensor(ref).double()).abs().max()) <= 0.1


# on the GPU a non-strict plan is captured, and a captured interpreter op cannot read a device tensor
# into Python: the reductions of a glue norm (their axes) and fed paddings cannot run there, before
# this change as after it.  The pads with constant paddings can: they stay on the host.
GPU_GLUE_RUNS = ("pad_channels", "pad_batch")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", REFUSALS)
def test_lowering_refusals_gpu(kind):
    """The same refusals on the GPU: ``CompileError`` under ``strict``; for the glue pads the captured
    non-strict plan against the interpreter."""
    g, fetch, op = _refusal_graph(kind)
    with pytest.raises(CompileError, match="no CDNA4 lowering"):
        g.compile([fetch], "cuda", strict=True)
    if kind not in GPU_GLUE_RUNS:
        return
    plan = g.compile([fetch], "cuda", strict=False)
    s = plan.summary()
    assert s["hip_graph"] and op in s["glue_ops"] and not {"instnorm", "pad", "image_out"} & set(s["kinds"]), s
    got, = plan({k: v.to("cuda") for k, v in g.feeds.items()})
    ref, = g.reference([fetch])
    assert tuple(got.shape) == tuple(ref.shape)
    assert float((got.cpu().double() - torch.as_tensor(ref).double()).abs().max()) <= 0.1


def test_image_out_pattern_edges():
    """What the output stage does not absorb: a ``Cast`` behind a clamp outside ``[0, 255]`` and a
    link with a second reader; a bare ``Tanh`` stays in the conv's epilogue as before."""
    def stage(lo, hi, second_reader=False, bare=False):
        g = _G()
        y = g.gb.tanh(g.conv(g.x, 3, 16, 3, "rgb", bias=True), name="Tanh")
        if bare:
            return g, ["Tanh:0"]
        m = g.gb.mul(y, g.gb.constant("s", np.float32(100.0)), name="Mul")
        c = g.gb.clip_by_value(m, lo, hi, name="clip")
        g.gb.cast(c, "UINT8" if not second_reader else "INT32", name="out")
        return g, ["out:0"] + (["Mul:0"] if second_reader else [])

    g, f = stage(-300.0, 300.0)
    s = g.compile(f, strict=False).summary()
    assert s["kinds"].get("image_out") == 1 and "Cast" in s["glue_ops"]      # the clamp is absorbed, the Cast is not
    g, f = stage(0.0, 255.0, second_reader=True)
    plan = g.compile(f, strict=False)
    s = plan.summary()
    assert s["kinds"].get("image_out") == 1 and "ClipByValue" in s["glue_ops"]  # the chain ends at the fetched Mul
    out, mul = plan(g.feeds)
    ref = g.reference(f)
    assert mul.dtype == F32 and float((mul.double() - torch.as_tensor(ref[1]).double()).abs().max()) <= 2.0  # of 100
    g, f = stage(0, 0, bare=True)
    plan = g.compile(f, strict=True)
    assert plan.summary()["kinds"].get("image_out") is None and "conv" in plan.summary()["kinds"]


# =================================================================================== the model
ST = dict(base=8, blocks=1, image_hw=(32, 32))
ST_KINDS = {"preprocess": 1, "pad": 4, "conv": 6, "instnorm": 7, "elementwise": 1, "deconv": 2, "image_out": 1}
PLAN_ATOL = 2 * 6     # uint8 counts, host plan vs fp32 interpreter on these images: twice the measured error


def _imgs(n, hw=32, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, hw, hw, 3), dtype=np.uint8))


@pytest.fixture(scope="module")
def st():
    """The small generator, four images, the fp32 interpreter's image and the host plan's: once."""
    from flink_tensorflow_amd.models.zoo import style_transfer_graph_def

    g = Graph.from_graph_def(style_transfer_graph_def(**ST))
    imgs = _imgs(4, seed=11)
    ref, = Session(g).run(["stylized:0"], {"images:0": imgs})
    plan = CompiledFunction(g, {"images:0": (tuple(imgs.shape), "UINT8")}, ["stylized:0"], "cpu", strict=True)
    host, = plan({"images:0": imgs})
    return g, imgs, torch.as_tensor(ref), host.clone(), plan.summary()


def _counts(a, b):
    return int((torch.as_tensor(a).int() - torch.as_tensor(b).int()).abs().max())


def test_style_transfer_compiles_strict_to_the_stated_kinds(st):
    from flink_tensorflow_amd.models.zoo.style_transfer import expected_step_kinds

    _, _, _, _, s = st
    assert s["glue_ops"] == [] and s["kinds"] == ST_KINDS == expected_step_kinds(1)
    assert expected_step_kinds() == {"preprocess": 1, "pad": 12, "conv": 14, "instnorm": 15, "elementwise": 5,
                                     "deconv": 2, "image_out": 1}


def test_style_transfer_host_plan_against_the_interpreter(st):
    """Seen: at most 6 counts between the bf16 host plan and the fp32 interpreter (half the pixels
    differ by a count or more: bf16 activations under ``127.5 tanh``); asserted: twice that."""
    _, imgs, ref, host, _ = st
    assert ref.dtype == torch.uint8 and tuple(ref.shape) == (4, 32, 32, 3) and host.dtype == torch.uint8
    assert len(torch.unique(ref)) > 100                 # an image, not a flat field
    worst = _counts(host, ref)
    print(f"host plan vs interpreter: {worst} counts (allowed {PLAN_ATOL})")
    assert worst <= PLAN_ATOL


def test_style_transfer_symmetric_pads_compile_too():
    from flink_tensorflow_amd.models.zoo import style_transfer_graph_def

    g = Graph.from_graph_def(style_transfer_graph_def(pad_mode="SYMMETRIC", **ST))
    plan = CompiledFunction(g, {"images:0": ((1, 32, 32, 3), "UINT8")}, ["stylized:0"], "cpu", strict=True)
    assert plan.summary()["kinds"] == ST_KINDS
    assert {s.meta["mode"] for s in plan.steps if s.kind == "pad"} == {"symmetric"}
    with pytest.raises(ValueError):
        style_transfer_graph_def(base=12)


def test_style_transfer_model_behind_map_with_model_batched(st):
    from flink_tensorflow_amd.models.zoo import StyleTransferModel
    from flink_tensorflow_amd.runtime import StreamExecutionEnvironment

    _, imgs, ref, _, _ = st
    m = StyleTransferModel(buckets=(4,), device="cpu", **ST)
    m.open()
    try:
        out = m.stylize(list(imgs.numpy()))
        (sub, tags, _), = m.submit(list(imgs.numpy()), np.zeros(4), [3, 4, 5, 6])
    finally:
        m.close()
    assert len(out) == 4 and all(a.shape == (32, 32, 3) and a.dtype == np.uint8 for a in out)
    assert np.array_equal(np.stack(out), ref.numpy()) and tags == [3, 4, 5, 6]     # host: the interpreter
    assert np.array_equal(np.stack(sub), np.stack(out))
    env = StreamExecutionEnvironment.get_execution_environment()
    got = env.from_collection(list(imgs.numpy())).map_with_model_batched(
        StyleTransferModel(buckets=(4,), device="cpu", **ST), None, max_batch=2, max_delay_ms=1).execute_and_collect()
    assert sorted(a.tobytes() for a in got) == sorted(a.tobytes() for a in out)


def test_style_transfer_saved_model_round_trip(tmp_path, st):
    from flink_tensorflow_amd.models import PredictMethod, SavedModelModel
    from flink_tensorflow_amd.models.zoo import export_style_transfer_saved_model

    _, imgs, ref, host, _ = st
    d = export_style_transfer_saved_model(str(tmp_path / "style"), **ST)
    m = SavedModelModel(d, device="cpu")
    m.open()
    try:
        interp = m.function("serving_default", PredictMethod(), compile=False)
        fn = m.function("serving_default", PredictMethod(), compile=True, batch_buckets=None)
        a, b = interp.apply({"images": imgs.numpy()}), fn.apply({"images": imgs.numpy()})
        s = fn.plan_summary()
    finally:
        m.close()
    assert s is not None and s["glue_ops"] == [] and s["kinds"] == ST_KINDS
    assert torch.equal(torch.as_tensor(a["stylized"]), ref)          # the variables restore the weights
    assert torch.equal(torch.as_tensor(b["stylized"]), host)


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


def _in_gpu(case, act, dev, slot=None):
    """The kernel with every operand between NaN bands and the output (a channel slice of a wider
    tensor with ``slot = (pitch, offset)``) between sentinel bands -> the result on the host."""
    shape = case[0]
    x, gamma, beta = _in_data(*case)
    ops = {"x": _banded(x, NAN, dev), "gamma": _banded(gamma, NAN, dev), "beta": _banded(beta, NAN, dev)}
    C = shape[-1]
    pitch, off = slot or (C, 0)
    out, obuf = _banded(torch.full((*shape[:3], pitch), SENT, dtype=BF), SENT, dev)
    scratch, sbuf = _banded(torch.zeros(K.instance_norm_scratch_numel(*shape), dtype=F32), SENT, dev)
    K.instance_norm(ops["x"][0], ops["gamma"][0], ops["beta"][0], EPS, act, out=out, out_channel_offset=off, scratch=scratch)
    torch.cuda.synchronize()
    for k, (v, buf) in ops.items():
        assert _bands_intact(buf, v.numel(), NAN), f"{k}: a guard band was written"
    assert _bands_intact(obuf, out.numel(), SENT) and _bands_intact(sbuf, scratch.numel(), SENT)
    o = out.cpu()
    assert (o[..., :off] == SENT).all() and (o[..., off + C:] == SENT).all(), "the slot's neighbours were written"
    return o[..., off:off + C]


@pytest.mark.gpu
@pytest.mark.parametrize("act", IN_ACTS)
@pytest.mark.parametrize("case", IN_CASES, ids=_in_id)
def test_instnorm_kernel_matches_the_mirror(case, act):
    """Every case (the paths they cover: the module docstring) and activation, between guard bands,
    into a plain buffer and into a channel slice of a wider one."""
    a, share = _bounds()
    dev = torch.device("cuda", 0)
    C = case[0][-1]
    for slot in (None, (C + 24, 16)):
        got = _in_gpu(case, act, dev, slot)
        assert torch.isfinite(got.float()).all()
        e, p = _in_diff(got, _in_ref(case, act))
        print(f"{_in_id(case)} {act} slot={slot}: {e:g} ulp (allowed {a:g}), differing share {p:.5f} (allowed {share:.4f})")
        assert e <= a and p <= share, (e, p)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in IN_CASES if c[0][0] > 1], ids=_in_id)
def test_instnorm_kernel_is_deterministic_and_images_are_independent(case):
    dev = torch.device("cuda", 0)
    x, gamma, beta = (t.to(dev) for t in _in_data(*case))
    a = K.instance_norm(x, gamma, beta, EPS, "relu")
    b = K.instance_norm(x, gamma, beta, EPS, "relu")
    assert torch.equal(a, b)                                     # two launches: identical bits
    for n in range(x.shape[0]):                                  # image n alone: the same bits
        assert torch.equal(K.instance_norm(x[n:n + 1].contiguous(), gamma, beta, EPS, "relu")[0], a[n])


@pytest.mark.gpu
@pytest.mark.parametrize("case", _pad_cases(), ids=_pad_id)
def test_pad_kernel_is_the_index_mirror(case):
    shape, pads, mode = case
    dev = torch.device("cuda", 0)
    x = _pad_data(shape)
    ref = _pad_mirror(x, pads, mode, 1.5)
    xd, xbuf = _banded(x, NAN, dev)
    for pitch, off in ((shape[3], 0), (shape[3] + 16, 8)):      # a plain buffer, a concat slot
        out, obuf = _banded(torch.full((*ref.shape[:3], pitch), SENT, dtype=BF), SENT, dev)
        K.pad_nhwc(xd, pads, mode, 1.5, out=out, out_channel_offset=off)
        torch.cuda.synchronize()
        assert _bands_intact(xbuf, x.numel(), NAN) and _bands_intact(obuf, out.numel(), SENT)
        o = out.cpu()
        assert torch.equal(o[..., off:off + shape[3]], ref)
        assert (o[..., :off] == SENT).all() and (o[..., off + shape[3]:] == SENT).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", PAD_MODES)
def test_pad_kernel_channel_padded_input(mode):
    """3 logical channels over 8 physical ones: physical vectors are copied (a mirror of zero is
    zero), a constant fill writes the value to the logical channels only."""
    dev = torch.device("cuda", 0)
    x = _pad_data((2, 5, 6, 8)).clone()
    x[..., 3:] = 0
    pads = (1, 2, 3, 0)
    got = K.pad_nhwc(x.to(dev), pads, mode, 2.0, channels=3).cpu()
    assert torch.equal(got, _pad_mirror(x, pads, mode, 2.0, channels=3)) and (got[..., 3:] == 0).all()
    assert torch.equal(got, K.pad_nhwc(x, pads, mode, 2.0, channels=3))


@pytest.mark.gpu
@pytest.mark.parametrize("case", IMG_CASES, ids=_img_id)
def test_image_out_kernel_matches_the_mirror(case):
    """Exact on the grid data; tanh / sigmoid: uint8 within one count, fp32 within the measured
    tolerance.  NaN guard bands and NaN padding channels in, untouched bytes behind the image."""
    shape, cl, act, dt = case
    dev = torch.device("cuda", 0)
    x = _img_input(shape, cl, act)
    xd, xbuf = _banded(x, NAN, dev)
    fill = 77 if dt == torch.uint8 else SENT
    out, obuf = _banded(torch.full((*shape, cl), fill, dtype=dt), fill, dev)
    K.image_out(xd, cl, act, *_img_params(act), out=out)
    torch.cuda.synchronize()
    assert _bands_intact(xbuf, x.numel(), NAN) and _bands_intact(obuf, out.numel(), fill)
    _check_image(out.cpu(), x, case)


# =================================================================================== GPU: the model
@pytest.mark.gpu
def test_style_transfer_plan_and_model_gpu(st):
    from flink_tensorflow_amd.models.zoo import StyleTransferModel

    g, imgs, ref, host, _ = st
    dev = torch.device("cuda", 0)
    plan = CompiledFunction(g, {"images:0": (tuple(imgs.shape), "UINT8")}, ["stylized:0"], dev, strict=True)
    s = plan.summary()
    assert s["hip_graph"] and s["glue_ops"] == [] and s["kinds"] == ST_KINDS
    out, = plan({"images:0": imgs.to(dev)})
    out = out.cpu().clone()
    worst = _counts(out, host)
    print(f"captured plan vs host plan: {worst} counts (allowed {PLAN_ATOL})")
    assert out.dtype == torch.uint8 and tuple(out.shape) == (4, 32, 32, 3) and worst <= PLAN_ATOL
    again, = plan({"images:0": imgs.to(dev)})
    assert torch.equal(again.cpu(), out)                   # a second replay is bit-identical
    m = StyleTransferModel(buckets=(4,), lanes=1, **ST)
    m.open()
    try:
        assert m.plan_summary()["kinds"] == ST_KINDS
        pics = m.stylize(list(imgs.numpy()))
        done = []
        for i in range(4):   # one record per batch: results come back in submission order
            done += m.submit([imgs[i].numpy()], np.zeros(1), [i])
        done += m.drain()
    finally:
        m.close()
    assert len(pics) == 4 and all(a.shape == (32, 32, 3) and a.dtype == np.uint8 for a in pics)
    assert np.array_equal(np.stack(pics), out.numpy())
    assert [t for _, tags, _ in done for t in tags] == [0, 1, 2, 3]
    batched = np.stack([r for res, _, _ in done for r in res])
    assert batched.shape == (4, 32, 32, 3) and batched.dtype == np.uint8 and _counts(batched, out) <= PLAN_ATOL
