"""Depthwise conv: the kernel of ``kernels/dwconv.hip`` bit for bit, its lowering, MobileNet-V1.

The kernel tests follow ``test_igemm_exact.py``: operands are integers exact in bf16 (the bias is
fp32 half-integers), every partial sum stays far below 2^23, so fp32 accumulation is exact in any
order and the only inexact step is the kernel's single ``f2bf`` (round to nearest even).  The
float64 mirror is built from the definition (a loop over the taps on a zero-padded image with
strided, dilated slices) and rounds once, after bias and activation.  Data per activation:

none / relu   x in [-8, 8], w in [-4, 4], bias = halves in [-600, 600]: sums pass 256, where bf16
              starts to round; without a bias x in [-24, 24], w in [-8, 8].
relu6         "low" data: x, w in [-1, 1] and bias = halves in [-3, 9]; without a bias x, w in
              [-3, 3] up to 9 taps and [-2, 2] above (a tap's product then has variance 16 or 4:
              one tap in the image already reaches 6, and 49 taps still leave sums inside (0, 6)).

The comparison is on the bit patterns.  No -0 can occur: sums start from +0, ``x + (-x)`` is +0
under round-to-nearest, ReLU is ``x > 0 ? x : 0`` and ReLU6 ``min(max(x, 0), 6)``.

The non-GPU tests check the lowering against the interpreter, the host path of the launcher, and
the mirror itself: that the data put outputs on every clamp and inside, and that a mirror with
clamp-to-edge padding differs, so a border bug shows."""
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from flink_tensorflow_amd.graph.builder import GraphBuilder
from flink_tensorflow_amd.graph.compiler import CompiledFunction, CompileError
from flink_tensorflow_amd.graph.graph import Graph
from flink_tensorflow_amd.graph.ops_nn import conv2d_tf, same_pads
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.ops import kernels as K

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 2.0 ** 100        # output sentinel: exact in bf16, far above any result
ACTS = (None, "relu", "relu6")

SHAPES = ((1, 9, 11, 8), (3, 9, 11, 24), (2, 8, 10, 72), (2, 2, 3, 32), (1, 17, 5, 520))
# name -> (KH, KW, stride, dilation, padding)
GEOM_3X3 = {"3x3s1-same": (3, 3, (1, 1), (1, 1), "SAME"), "3x3s2-same": (3, 3, (2, 2), (1, 1), "SAME"),
            "3x3s1-valid": (3, 3, (1, 1), (1, 1), "VALID")}
GEOM_GENERIC = {"5x5s1": (5, 5, (1, 1), (1, 1), "SAME"), "7x7s2": (7, 7, (2, 2), (1, 1), "SAME"),
                "3x3d2": (3, 3, (1, 1), (2, 2), "SAME"), "3x3s12": (3, 3, (1, 2), (1, 1), "SAME"),
                "1x1": (1, 1, (1, 1), (1, 1), "SAME")}
GEOMS = {**GEOM_3X3, **GEOM_GENERIC}
CASES = [(s, g) for g in GEOMS for s in SHAPES]


def _case_id(c):
    (N, H, W, C), g = c
    return f"{g}-{N}x{H}x{W}x{C}"


def _pads(H, W, geom):
    KH, KW, (sh, sw), (dh, dw), padding = GEOMS[geom]
    if padding == "VALID":
        return (0, 0, 0, 0)
    return (*same_pads(H, KH, sh, dh), *same_pads(W, KW, sw, dw))


def _out_hw(H, W, geom):
    KH, KW, (sh, sw), (dh, dw), _ = GEOMS[geom]
    pt, pb, pl, pr = _pads(H, W, geom)
    return (H + pt + pb - ((KH - 1) * dh + 1)) // sh + 1, (W + pl + pr - ((KW - 1) * dw + 1)) // sw + 1


@functools.lru_cache(maxsize=None)
def _data(shape, geom, act, bias):
    """(x [N,H,W,C], w [KH*KW, C], bias [C] or None) as float64 integers / half-integers."""
    KH, KW = GEOMS[geom][:2]
    N, H, W, C = shape
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, geom, act, bias)).encode()))
    if act == "relu6":
        xr, wr = (1, 1) if bias else ((3, 3) if KH * KW <= 9 else (2, 2))
        br = (-6, 18)            # halves in [-3, 9]
    else:
        xr, wr = (8, 4) if bias else (24, 8)
        br = (-1200, 1200)       # halves in [-600, 600]
    x = torch.randint(-xr, xr + 1, shape, generator=g).to(F64)
    w = torch.randint(-wr, wr + 1, (KH * KW, C), generator=g).to(F64)
    b = torch.randint(br[0], br[1] + 1, (C,), generator=g).to(F64) / 2 if bias else None
    return x, w, b


def _act(v, act):
    if act == "relu":
        return torch.relu(v)
    if act == "relu6":
        return torch.clamp(v, 0, 6)
    return v


def _mirror(x, w, b, geom, act, edge=False):
    """float64 definition; one bf16 rounding at the end.  ``edge``: the deliberately wrong
    variant that pads by repeating the border pixel instead of zeros."""
    KH, KW, (sh, sw), (dh, dw), _ = GEOMS[geom]
    N, H, W, C = x.shape
    pt, pb, pl, pr = _pads(H, W, geom)
    Ho, Wo = _out_hw(H, W, geom)
    xn = x.permute(0, 3, 1, 2)
    if edge:
        # replicate needs pad < size: pad one pixel at a time
        xp = xn
        for _ in range(max(pt, pb, pl, pr)):
            cur = [min(1, max(0, p)) for p in (pl, pr, pt, pb)]
            xp = F.pad(xp, cur, mode="replicate")
            pl, pr, pt, pb = (p - c for p, c in zip((pl, pr, pt, pb), cur))
    else:
        xp = F.pad(xn, (pl, pr, pt, pb))
    xp = xp.permute(0, 2, 3, 1)
    acc = torch.zeros((N, Ho, Wo, C), dtype=F64)
    for kh in range(KH):
        for kw in range(KW):
            y0, x0 = kh * dh, kw * dw
            acc += xp[:, y0:y0 + (Ho - 1) * sh + 1:sh, x0:x0 + (Wo - 1) * sw + 1:sw, :] * w[kh * KW + kw]
    if b is not None:
        acc = acc + b
    assert acc.abs().max() < 2 ** 22            # fp32 accumulation is exact in any order
    return _act(acc, act).to(F32).to(BF)


def _bits(t):
    return t.contiguous().view(torch.int16)


# =================================================================================== the mirror
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_mirror_is_the_definition_and_the_data_show_bugs(case):
    shape, geom = case
    KH, KW, stride, dil, padding = GEOMS[geom]
    Ho, Wo = _out_hw(*shape[1:3], geom)
    if Ho < 1 or Wo < 1:
        assert padding == "VALID"
        return
    for act in ACTS:
        for bias in (True, False):
            x, w, b = _data(shape, geom, act, bias)
            y = _mirror(x, w, b, geom, act).to(F64)
            ref = conv2d_tf(x, w.reshape(KH, KW, 1, -1), stride, padding, dil, groups=shape[3])
            ref = _act(ref + b if bias else ref, act).to(F32).to(BF).to(F64)
            assert torch.equal(y, ref)
            n = y.numel()
            if act == "relu":
                assert (y == 0).sum() >= 0.05 * n and (y > 0).sum() >= 0.05 * n
            if act == "relu6":
                assert (y == 0).sum() >= 0.05 * n and (y == 6).sum() >= 0.05 * n
                assert ((y > 0) & (y < 6)).sum() >= 0.05 * n
            if any(_pads(*shape[1:3], geom)):
                assert not torch.equal(_mirror(x, w, b, geom, act, edge=True).to(F64), y)


def test_rounding_is_observable():
    x, w, b = _data(SHAPES[1], "3x3s1-same", None, True)
    y = _mirror(x, w, b, "3x3s1-same", None).to(F64)
    exact = conv2d_tf(x, w.reshape(3, 3, 1, -1), (1, 1), "SAME", (1, 1), groups=24) + b
    assert (y != exact).float().mean() > 0.05


# =================================================================================== host launcher
@pytest.mark.parametrize("hw,k,stride,dil", [((8, 10), 3, (1, 1), (1, 1)), ((9, 11), 3, (1, 1), (1, 1)),
                                              ((8, 10), 3, (2, 2), (1, 1)), ((9, 11), 3, (2, 2), (1, 1)),
                                              ((9, 11), 3, (1, 1), (2, 2)), ((8, 9), 5, (2, 1), (1, 1))])
def test_host_path_matches_the_interpreter(hw, k, stride, dil):
    torch.manual_seed(3)
    H, W = hw
    C = 24
    x = torch.randn(2, H, W, C)
    w = torch.randn(k, k, C, 1)
    b = torch.randn(C)
    pads = (*same_pads(H, k, stride[0], dil[0]), *same_pads(W, k, stride[1], dil[1]))
    ref = torch.clamp(conv2d_tf(x, w.reshape(k, k, 1, C), stride, "SAME", dil, groups=C) + b, 0, 6)
    y = K.dwconv2d_nhwc(x, w.reshape(k * k, C), b, stride, pads, dil, "relu6")
    assert y.shape == ref.shape and torch.allclose(y, ref, atol=1e-5)
    # into a concat slot: the neighbours keep their values
    out = torch.full((*ref.shape[:3], C + 16), 7.0)
    K.dwconv2d_nhwc(x, w.reshape(k * k, C), b, stride, pads, dil, "relu6", out=out, out_channel_offset=8)
    assert torch.allclose(out[..., 8:8 + C], ref, atol=1e-5)
    assert (out[..., :8] == 7).all() and (out[..., 8 + C:] == 7).all()


def test_eligibility_is_pure():
    assert K.dwconv_eligible(32, 3, 3, (1, 1), (1, 1)) and K.dwconv_eligible(520, 7, 7, (2, 2), (1, 1))
    assert not K.dwconv_eligible(12, 3, 3, (1, 1), (1, 1)) and not K.dwconv_eligible(32, 9, 9, (1, 1), (1, 1))
    assert K.dwconv_impl(3, 3, (2, 2), (1, 1)) == "dwconv3x3"
    assert K.dwconv_impl(3, 3, (1, 2), (1, 1)) == K.dwconv_impl(5, 5, (1, 1), (1, 1)) == "dwconv_generic"
    assert K.dwconv_impl(3, 3, (1, 1), (2, 2)) == "dwconv_generic"
    with pytest.raises(ValueError):
        K.dwconv2d_nhwc(torch.zeros(1, 2, 3, 8), torch.zeros(9, 8))  # VALID 3x3 on 2x3: no output


# =================================================================================== lowering
def _bn(gb, rng, y, c, name):
    with gb.name_scope(name):
        g = rng.uniform(0.8, 1.2, c).astype(np.float32)
        b = (rng.standard_normal(c) * 0.05).astype(np.float32)
        m = (rng.standard_normal(c) * 0.05).astype(np.float32)
        v = rng.uniform(0.8, 1.2, c).astype(np.float32)
        return gb.fused_batch_norm(y, gb.constant("gamma", g), gb.constant("beta", b), gb.constant("mean", m),
                                   gb.constant("var", v), name="BatchNorm")


def _front(gb, hw):
    images = gb.placeholder("images", "UINT8", [None, hw, hw, 3])
    x = gb.cast(images, "FLOAT", name="Cast")
    x = gb.sub(x, gb.constant("mean", np.asarray([120.0, 115.0, 100.0], dtype=np.float32)), name="Sub")
    return gb.div(x, gb.constant("std", np.asarray([58.0, 57.0, 57.5], dtype=np.float32)), name="normalized")


def _head(gb, rng, x, c, classes=16):
    x = gb.mean(x, [1, 2], name="avg_pool")
    w = gb.constant("fc/weights", (rng.standard_normal((c, classes)) / np.sqrt(c)).astype(np.float32))
    logits = gb.bias_add(gb.matmul(x, w, name="fc/MatMul"), gb.constant("fc/b", np.zeros(classes, np.float32)),
                         name="logits")
    gb.top_k(gb.softmax(logits, name="probs"), 3, name="top_k")


def _conv_w(rng, kh, cin, cout):
    return (rng.standard_normal((kh, kh, cin, cout)) * np.sqrt(2.0 / (kh * kh * cin))).astype(np.float32)


def _dw_w(rng, k, c, mult=1):
    return (rng.standard_normal((k, k, c, mult)) * np.sqrt(2.0 / (k * k))).astype(np.float32)


def _small_graph(depthwise=True):
    """preprocess, 3x3/s2 stem, dw 3x3, pw 1x1, dw 3x3/s2, pw 1x1, GAP, MatMul, softmax + top-k;
    every conv followed by BN + Relu6."""
    gb, rng = GraphBuilder(), np.random.default_rng(5)
    x = _front(gb, 24)
    x = gb.relu6(_bn(gb, rng, gb.conv2d(x, gb.constant("stem/w", _conv_w(rng, 3, 3, 16)), (2, 2), name="stem"), 16,
                     "stem_bn"), name="stem_relu6")
    cin = 16
    for i, (cout, s) in enumerate(((32, 1), (64, 2))):
        if depthwise:
            y = gb.depthwise_conv2d(x, gb.constant(f"dw{i}/w", _dw_w(rng, 3, cin)), (s, s), name=f"dw{i}")
            x = gb.relu6(_bn(gb, rng, y, cin, f"dw{i}_bn"), name=f"dw{i}_relu6")
        y = gb.conv2d(x, gb.constant(f"pw{i}/w", _conv_w(rng, 1, cin, cout)), name=f"pw{i}")
        x = gb.relu6(_bn(gb, rng, y, cout, f"pw{i}_bn"), name=f"pw{i}_relu6")
        cin = cout
    _head(gb, rng, x, cin)
    return gb.build()


def _agree(logits, idx, ref_logits, ref_idx):
    """The rule of ``test_compiler._check_plan``."""
    err = (logits.float().cpu() - ref_logits).abs().max().item() / ref_logits.abs().max().item()
    assert err < 0.05, err
    top2 = torch.topk(torch.softmax(ref_logits, -1), 2, -1).values
    ok = (idx[:, 0].cpu() == ref_idx[:, 0]) | ((top2[:, 0] - top2[:, 1]) < 0.02)
    assert ok.all()


def _compile(graph, imgs, device="cpu", strict=True):
    return CompiledFunction(graph, {"images:0": (tuple(imgs.shape), "UINT8")}, ["logits:0", "top_k:1"], device,
                            strict=strict)


def test_small_graph_compiles_strict():
    imgs = torch.randint(0, 256, (2, 24, 24, 3), dtype=torch.uint8)
    s = _compile(_small_graph(False), imgs).summary()
    assert s["glue_ops"] == [] and s["kinds"] == {"preprocess": 1, "conv": 3, "gap": 1, "gemm": 1, "softmax_topk": 1}
    g = _small_graph()
    plan = _compile(g, imgs)
    s = plan.summary()
    assert s["glue_ops"] == []
    assert s["kinds"]["dwconv"] == 2 and s["kinds"]["conv"] == 3
    assert "elementwise" not in s["kinds"] and "glue" not in s["kinds"]     # BN and Relu6 are absorbed
    assert [st.meta["impl"] for st in plan.steps if st.kind == "dwconv"] == ["dwconv3x3", "dwconv3x3"]
    _agree(*plan({"images:0": imgs}), *Session(g).run(["logits:0", "top_k:1"], {"images:0": imgs}))


def _one_dw_graph(c=16, mult=1, k=3, explicit=False, residual=False, act="Relu", stride=1, dil=1):
    gb, rng = GraphBuilder(), np.random.default_rng(9)
    x = _front(gb, 12)
    x = gb.relu(gb.conv2d(x, gb.constant("stem/w", _conv_w(rng, 3, 3, c)), name="stem"), name="stem_relu")
    if explicit:
        y = gb.op("DepthwiseConv2dNative", [x, gb.constant("dw/w", _dw_w(rng, k, c, mult))], name="dw",
                  strides=[1, 1, 1, 1], padding=b"EXPLICIT", data_format=b"NHWC", dilations=[1, 1, 1, 1],
                  explicit_paddings=[0, 0, 1, 1, 1, 1, 0, 0])
    else:
        y = gb.depthwise_conv2d(x, gb.constant("dw/w", _dw_w(rng, k, c, mult)), (stride, stride), name="dw",
                                dilations=(dil, dil))
    y = _bn(gb, rng, y, c * mult, "dw_bn")
    if residual:
        y = gb.add(y, x, name="res_add")
    y = gb.op(act, [y], name="dw_act")
    _head(gb, rng, y, c * mult)
    return gb.build()


def test_residual_add_stays_its_own_step():
    g = _one_dw_graph(residual=True)
    imgs = torch.randint(0, 256, (2, 12, 12, 3), dtype=torch.uint8)
    plan = _compile(g, imgs)
    s = plan.summary()
    assert s["glue_ops"] == [] and s["kinds"]["dwconv"] == 1
    names = [st.name for st in plan.steps if st.kind == "elementwise"]
    assert names == ["res_add", "dw_act"]
    _agree(*plan({"images:0": imgs}), *Session(g).run(["logits:0", "top_k:1"], {"images:0": imgs}))


@pytest.mark.parametrize("act", ["Sigmoid", "Tanh"])
def test_sigmoid_and_tanh_end_the_chain(act):
    g = _one_dw_graph(act=act)
    imgs = torch.randint(0, 256, (2, 12, 12, 3), dtype=torch.uint8)
    plan = _compile(g, imgs)
    assert plan.summary()["kinds"]["dwconv"] == 1
    assert [st.name for st in plan.steps if st.kind == "elementwise"] == ["dw_act"]
    _agree(*plan({"images:0": imgs}), *Session(g).run(["logits:0", "top_k:1"], {"images:0": imgs}))


@pytest.mark.parametrize("geom", [dict(k=5), dict(k=7, stride=2), dict(dil=2)], ids=["5x5", "7x7s2", "3x3d2"])
def test_generic_geometries_lower(geom):
    g = _one_dw_graph(act="Relu6", **geom)
    imgs = torch.randint(0, 256, (2, 12, 12, 3), dtype=torch.uint8)
    plan = _compile(g, imgs)
    assert [st.meta["impl"] for st in plan.steps if st.kind == "dwconv"] == ["dwconv_generic"]
    _agree(*plan({"images:0": imgs}), *Session(g).run(["logits:0", "top_k:1"], {"images:0": imgs}))


@pytest.mark.parametrize("kw", [dict(mult=2), dict(c=12), dict(explicit=True)], ids=["mult2", "c12", "explicit"])
def test_ineligible_layers_stay_glue(kw):
    g = _one_dw_graph(**kw)
    imgs = torch.randint(0, 256, (2, 12, 12, 3), dtype=torch.uint8)
    with pytest.raises(CompileError, match="no CDNA4 lowering"):
        _compile(g, imgs)
    plan = _compile(g, imgs, strict=False)
    s = plan.summary()
    assert "DepthwiseConv2dNative" in s["glue_ops"] and "dwconv" not in s["kinds"]
    _agree(*plan({"images:0": imgs}), *Session(g).run(["logits:0", "top_k:1"], {"images:0": imgs}))


# =================================================================================== MobileNet-V1
MB = dict(alpha=0.25, image_hw=(72, 72), out_hw=(64, 64), num_classes=64)


@pytest.fixture(scope="module")
def mobilenet():
    """The graph, three images and the fp32 interpreter's (logits, top-k indices): computed once."""
    from flink_tensorflow_amd.models.zoo import mobilenet_v1_graph_def

    g = Graph.from_graph_def(mobilenet_v1_graph_def(**MB))
    imgs = torch.randint(0, 256, (3, 72, 72, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(11))
    ref = Session(g).run(["logits:0", "top_k:1"], {"images:0": imgs})
    return g, imgs, ref


def test_mobilenet_plan_host(mobilenet):
    g, imgs, ref = mobilenet
    plan = _compile(g, imgs[:2])
    s = plan.summary()
    assert s["glue_ops"] == [] and s["kinds"]["dwconv"] == 13 and s["kinds"]["conv"] == 14
    assert "elementwise" not in s["kinds"]
    _agree(*plan({"images:0": imgs[:2]}), ref[0][:2], ref[1][:2])


def test_mobilenet_model_labels_on_the_host(mobilenet):
    from flink_tensorflow_amd.models.zoo import MobileNetV1Model

    _, imgs, ref = mobilenet
    m = MobileNetV1Model(buckets=(4,), top_k=3, device="cpu", **MB)
    m.open()
    try:
        out = m.label(list(imgs.numpy()))
    finally:
        m.close()
    assert len(out) == 3 and all(len(r) == 3 for r in out)
    assert [r[0][1] for r in out] == [f"class_{int(i)}" for i in ref[1][:, 0]]
    assert all(0 < p <= 1 for r in out for p, _ in r)


# =================================================================================== GPU: the kernel
def _tiles(geom):
    return (0, *K.DWCONV_TILES.values(), K.DWCONV_GENERIC) if geom in GEOM_3X3 else (0,)


def _report(y, ref, what):
    bad = (_bits(y) != _bits(ref)).nonzero()
    lines = [f"{what}: {len(bad)} of {ref.numel()} differ"]
    for n, h, w_, c in bad[:5].tolist():
        lines.append(f"  [n={n} y={h} x={w_} c={c}] got {float(y[n, h, w_, c])} want {float(ref[n, h, w_, c])}")
    return "\n".join(lines)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_kernel_bit_exact(case):
    shape, geom = case
    KH, KW, stride, dil, _ = GEOMS[geom]
    N, H, W, C = shape
    Ho, Wo = _out_hw(H, W, geom)
    dev = torch.device("cuda", 0)
    if Ho < 1 or Wo < 1:     # 3x3 VALID on 2x3: the launcher refuses an empty output
        with pytest.raises(ValueError):
            K.dwconv2d_nhwc(torch.zeros(shape, dtype=BF, device=dev), torch.zeros(9, C, dtype=BF, device=dev))
        return
    pads = _pads(H, W, geom)
    for act in ACTS:
        for bias in (True, False):
            x, w, b = _data(shape, geom, act, bias)
            ref = _mirror(x, w, b, geom, act)
            xd, wd = x.to(BF).to(dev), w.to(BF).to(dev)
            bd = b.to(F32).to(dev) if bias else None
            for tile in _tiles(geom):
                what = f"{_case_id(case)} act={act} bias={bias} tile={tile}"
                y = K.dwconv2d_nhwc(xd, wd, bd, stride, pads, dil, act, kernel=(KH, KW), tile=tile)
                assert y.shape == ref.shape and y.dtype == BF
                assert torch.equal(_bits(y.cpu()), _bits(ref)), _report(y.cpu(), ref, what)
                # a concat slot: row pitch C + 16, offset 8, the neighbours keep the sentinel
                out = torch.full((N, Ho, Wo, C + 16), SENT, dtype=BF, device=dev)
                K.dwconv2d_nhwc(xd, wd, bd, stride, pads, dil, act, out=out, out_channel_offset=8, kernel=(KH, KW),
                                tile=tile)
                o = out.cpu()
                assert torch.equal(_bits(o[..., 8:8 + C]), _bits(ref)), _report(o[..., 8:8 + C], ref, what + " slot")
                assert (o[..., :8] == SENT).all() and (o[..., 8 + C:] == SENT).all(), what + ": neighbours written"


def _banded(t, fill, dev, band=4096):
    """``t`` as a view into a larger allocation filled with ``fill`` -> (view, whole buffer)."""
    n = t.numel()
    assert n % 8 == 0 or t.dtype == F32
    buf = torch.full((band + n + band,), fill, dtype=t.dtype, device=dev)
    v = buf[band:band + n].view(t.shape)
    v.copy_(t)
    return v, buf


GUARD_CASES = [(s, g) for s in (SHAPES[1], SHAPES[3], SHAPES[4]) for g in ("3x3s1-same", "3x3s2-same", "5x5s1", "3x3d2")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", GUARD_CASES, ids=_case_id)
def test_kernel_guard_bands(case):
    """x, w and bias between NaN bands, the output between sentinel bands: a read of a neighbour
    hidden behind a zero multiply turns the result NaN, a stray store breaks a band."""
    shape, geom = case
    KH, KW, stride, dil, _ = GEOMS[geom]
    N, H, W, C = shape
    Ho, Wo = _out_hw(H, W, geom)
    pads = _pads(H, W, geom)
    dev = torch.device("cuda", 0)
    band = 4096
    x, w, b = _data(shape, geom, "relu", True)
    ref = _mirror(x, w, b, geom, "relu")
    xv, xbuf = _banded(x.to(BF), float("nan"), dev)
    wv, wbuf = _banded(w.to(BF), float("nan"), dev)
    bv, bbuf = _banded(b.to(F32), float("nan"), dev)
    for tile in _tiles(geom):
        obuf = torch.full((band + ref.numel() + band,), SENT, dtype=BF, device=dev)
        ov = obuf[band:band + ref.numel()].view(ref.shape)
        K.dwconv2d_nhwc(xv, wv, bv, stride, pads, dil, "relu", out=ov, kernel=(KH, KW), tile=tile)
        y = ov.cpu()
        assert torch.isfinite(y.float()).all(), f"tile {tile}: a NaN neighbour was read"
        assert torch.equal(_bits(y), _bits(ref)), _report(y, ref, f"{_case_id(case)} tile={tile}")
        o = obuf.cpu()
        assert (o[:band] == SENT).all() and (o[band + ref.numel():] == SENT).all(), f"tile {tile}: stray store"
    for buf, t in ((xbuf, x), (wbuf, w), (bbuf, b)):
        h = buf.cpu()
        assert torch.isnan(h[:band]).all() and torch.isnan(h[band + t.numel():]).all()
        assert torch.equal(h[band:band + t.numel()].double().view(t.shape), t)


@pytest.mark.gpu
def test_launcher_rejects_bad_arguments():
    dev = torch.device("cuda", 0)
    x = torch.zeros((1, 4, 4, 16), dtype=BF, device=dev)
    w = torch.zeros((9, 16), dtype=BF, device=dev)
    with pytest.raises(ValueError):
        K.dwconv2d_nhwc(x, w, act="sigmoid", pad=(1, 1, 1, 1))
    with pytest.raises(ValueError):     # offset not a multiple of 8
        K.dwconv2d_nhwc(x, w, pad=(1, 1, 1, 1), out=torch.zeros((1, 4, 4, 32), dtype=BF, device=dev),
                        out_channel_offset=4)
    with pytest.raises(ValueError):     # slot past the row
        K.dwconv2d_nhwc(x, w, pad=(1, 1, 1, 1), out=torch.zeros((1, 4, 4, 24), dtype=BF, device=dev),
                        out_channel_offset=16)
    with pytest.raises(TypeError):
        K.dwconv2d_nhwc(x, w.float(), pad=(1, 1, 1, 1))


# =================================================================================== GPU: the plan
@pytest.mark.gpu
def test_mobilenet_plan_gpu(mobilenet):
    g, imgs, ref = mobilenet
    dev = torch.device("cuda", 0)
    plan = _compile(g, imgs, dev)
    s = plan.summary()
    assert s["glue_ops"] == [] and s["kinds"]["dwconv"] == 13 and s["hip_graph"]
    a = plan({"images:0": imgs.to(dev)})
    _agree(a[0], a[1], *ref)
    a0 = a[0].clone()
    b = plan({"images:0": imgs.to(dev)})
    assert torch.equal(a0, b[0])


@pytest.mark.gpu
def test_mobilenet_model_gpu(mobilenet):
    from flink_tensorflow_amd.models.zoo import MobileNetV1Model

    _, imgs, ref = mobilenet
    m = MobileNetV1Model(buckets=(4,), lanes=1, top_k=3, **MB)
    m.open()
    try:
        assert m.plan_summary()["kinds"]["dwconv"] == 13
        out = m.label(list(imgs.numpy()))
    finally:
        m.close()
    top2 = torch.topk(torch.softmax(ref[0], -1), 2, -1).values
    for r, i, t in zip(out, ref[1][:, 0].tolist(), top2):
        assert r[0][1] == f"class_{i}" or (t[0] - t[1]) < 0.02
