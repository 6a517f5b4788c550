"""Semantic segmentation: the kernels of ``kernels/resize.hip``, their lowerings, convs whose
output channels are no multiple of 8, and DeepLab-v3.

The mirror is float64 and built from the definition in ``graph/ops_nn.py:resize_bilinear_tf``:
coordinates in fp32 exactly as there (an fp32 scale, ``y * scale`` or ``(y + 0.5) * scale - 0.5``,
``floor``, clamps, a weight clipped to [0, 1]), then float64 lerps.

Exact cases.  x is integers in [-64, 64] and the geometries give lerp weights that are multiples
of 1/16 with exact fp32 coordinates, so every intermediate is a multiple of 1/256 below 2^7:
exact in fp32 in any operation order, with or without FMA contraction.  The only rounding is
the kernel's final ``f2bf``; outputs are compared on the bf16 bit patterns, labels index for
index (lowest index wins a tie).  For the ArgMax the logits have ``C`` channels in rows of pitch
``ceil8(C)``; the padding columns hold +inf (host) or 2^100 (device), so a kernel that lets
padding compete picks a wrong index.

General cases (non-dyadic scales, x = 4 * normal rounded to bf16).  Resize: every output within
``0.5 ulp_bf16(ref) + 2^-20 max|x|`` of the mirror: the one bf16 rounding, plus 16 fp32 ulps of the
largest operand for contraction and coordinate rounding, 2^12 times tighter than a bf16 step.
ArgMax: indices match wherever the mirror's top-1 minus top-2 margin exceeds ``2^-18 max|x|``; at
most 2 % of the pixels of the general cases may be excused (bf16 data has exact ties: the share
is 0.13 %), and the mirror's own excused share is asserted first.

Device tests put every operand between NaN guard bands and every output between sentinel bands
(2^100 for bf16, a byte / integer pattern no label equals for label maps), as
``tests/test_dwconv.py`` does.

DeepLab.  ``logits`` within 0.05 of the fp32 interpreter relative to its maximum (the rule of
``test_compiler._check_plan``).  Interpolation is a convex combination, so a per-logit error
``e`` can flip a label only where the top-2 margin of the upsampled logits is below ``2 e``:
labels must agree wherever the interpreter's margin is at least ``0.1 max|logits|``; at most half
of the pixels may be excused, which is asserted on the interpreter before any plan runs."""
import functools
import zlib

import numpy as np
import pytest
import torch

from flink_tensorflow_amd.graph.builder import GraphBuilder
from flink_tensorflow_amd.graph.compiler import CompiledFunction, CompileError
from flink_tensorflow_amd.graph.graph import Graph
from flink_tensorflow_amd.graph.ops_nn import resize_bilinear_tf
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.ops import kernels as K

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 2.0 ** 100                       # bf16 sentinel: exact, far above any result
LABEL_SENT = {torch.uint8: 0xA5, torch.int32: -7, torch.int64: -7}
LABEL_DTYPES = tuple(LABEL_SENT)

# name -> (H, W, Ho, Wo, align_corners, half_pixel_centers, the weights are not all 0)
EXACT = {"ac-3x3-9x9": (3, 3, 9, 9, True, False, True), "ac-2x3-17x33": (2, 3, 17, 33, True, False, True),
         "legacy-3x5-6x20": (3, 5, 6, 20, False, False, True), "hpc-3x5-6x10": (3, 5, 6, 10, False, True, True),
         "hpc-8x6-4x3": (8, 6, 4, 3, False, True, True), "bcast-1x1-5x6": (1, 1, 5, 6, True, False, False),
         "identity-7x5": (7, 5, 7, 5, False, False, False),
         # more than one 16 x 64 output tile per axis, odd sizes
         "ac-5x9-33x129": (5, 9, 33, 129, True, False, True)}
# weights of 1/2 only: results are multiples of 1/4 below 2^6, which bf16 holds: nothing rounds
EXACT_IN_BF16 = ("hpc-8x6-4x3",)
MODES = {"legacy": (False, False), "ac": (True, False), "hpc": (False, True)}
GENERAL = {f"{m}-{h}x{w}-{ho}x{wo}": (h, w, ho, wo, *MODES[m], True)
           for (h, w, ho, wo) in ((5, 7, 13, 11), (9, 6, 4, 5), (3, 3, 10, 7)) for m in MODES}
BATCHES = (1, 3)
RESIZE_C = (8, 24, 72)
ARGMAX_C = (1, 5, 21, 24, 151)


def _ceil8(c):
    return -(-c // 8) * 8


# =================================================================================== the mirror
def _coords(i, o, align, half):
    """(low index, high index, float64 weight) per output index: fp32 arithmetic as in
    ``resize_bilinear_tf``."""
    scale = (i - 1) / (o - 1) if align and o > 1 else i / o
    s = torch.arange(o, dtype=F32)
    f = (s + 0.5) * scale - 0.5 if half else s * scale
    assert f.dtype == F32
    i0 = torch.clamp(torch.floor(f), min=0).long()
    i1 = torch.clamp(i0 + 1, max=i - 1)
    w = (f - i0.float()) if half else (f - torch.floor(f))
    return i0, i1, w.clamp(0, 1).double()


def _mirror(x, oh, ow, align, half, flip_align=False, nearest_row=False):
    """float64 bilinear resize of x [N,H,W,C] (float64).  ``flip_align`` / ``nearest_row``: the
    deliberately wrong variants (the other scale rule; the high row replaced by the low one)."""
    if flip_align:
        align = not align
    y0, y1, wy = _coords(x.shape[1], oh, align, half)
    x0, x1, wx = _coords(x.shape[2], ow, align, half)
    if nearest_row:
        y1 = y0
    wx = wx[None, None, :, None]
    wy = wy[None, :, None, None]
    top = x[:, y0][:, :, x0] * (1 - wx) + x[:, y0][:, :, x1] * wx
    bot = x[:, y1][:, :, x0] * (1 - wx) + x[:, y1][:, :, x1] * wx
    return top * (1 - wy) + bot * wy


def _first_argmax(y):
    """Lowest index of the largest value along the last axis."""
    C = y.shape[-1]
    return torch.where(y == y.amax(-1, keepdim=True), torch.arange(C), C).amin(-1)


def _margin(y):
    """top-1 minus top-2 along the last axis (inf for a single channel)."""
    if y.shape[-1] == 1:
        return torch.full(y.shape[:-1], float("inf"), dtype=y.dtype)
    t = torch.topk(y, 2, -1).values
    return t[..., 0] - t[..., 1]


@functools.lru_cache(maxsize=None)
def _exact_x(name, N, C):
    H, W = EXACT[name][:2]
    g = torch.Generator().manual_seed(zlib.crc32(repr((name, N, C)).encode()))
    return torch.randint(-64, 65, (N, H, W, C), generator=g).to(F64)


@functools.lru_cache(maxsize=None)
def _general_x(name, N, C):
    H, W = GENERAL[name][:2]
    g = torch.Generator().manual_seed(zlib.crc32(repr((name, N, C)).encode()))
    return (torch.randn((N, H, W, C), generator=g) * 4).to(BF).to(F64)


@functools.lru_cache(maxsize=None)
def _exact_ref(name, N, C):
    """(float64 mirror, its single bf16 rounding) of an exact case."""
    _, _, Ho, Wo, align, half, _ = EXACT[name]
    y = _mirror(_exact_x(name, N, C), Ho, Wo, align, half)
    assert y.abs().max() <= 64 and torch.equal(y * 256, torch.round(y * 256))  # multiples of 1/256 below 2^7
    return y, y.to(F32).to(BF)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ulp_bf16(ref):
    """Spacing of bf16 at ``ref`` (8 significant bits)."""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


def _padded_logits(x, fill):
    """x [N,H,W,C] float64 -> bf16 rows of pitch ceil8(C), the padding columns = ``fill``."""
    C = x.shape[-1]
    p = torch.full((*x.shape[:3], _ceil8(C)), fill, dtype=BF)
    p[..., :C] = x.to(BF)
    return p


@pytest.mark.parametrize("name", list(EXACT))
def test_mirror_is_the_definition_and_the_data_show_bugs(name):
    _, _, Ho, Wo, align, half, lerps = EXACT[name]
    rounded = ties = pixels = 0
    for N in BATCHES:
        for C in RESIZE_C + ARGMAX_C:
            x = _exact_x(name, N, C)
            y, yb = _exact_ref(name, N, C)
            # the interpreter (fp32) equals the float64 mirror exactly on these cases
            assert torch.equal(resize_bilinear_tf(x.float(), Ho, Wo, align, half).double(), y)
            rounded += int((yb.double() != y).sum())
            if C > 1:
                ties += int((_margin(y) == 0).sum())
                pixels += y[..., 0].numel()
            if lerps:  # a coordinate bug shows: the wrong mirrors differ
                assert not torch.equal(_mirror(x, Ho, Wo, align, half, flip_align=True), y)
                assert not torch.equal(_mirror(x, Ho, Wo, align, half, nearest_row=True), y)
    if lerps and name not in EXACT_IN_BF16:
        assert rounded > 0          # the final f2bf is exercised
    assert ties > 0, (ties, pixels)  # lowest-index tie-breaking is exercised


@pytest.mark.parametrize("name", list(GENERAL))
def test_general_mirror_agrees_with_the_interpreter(name):
    _, _, Ho, Wo, align, half, _ = GENERAL[name]
    x = _general_x(name, 3, 24)
    y = _mirror(x, Ho, Wo, align, half)
    ref = resize_bilinear_tf(x.float(), Ho, Wo, align, half).double()
    assert (ref - y).abs().max() <= 2.0 ** -23.5 * x.abs().max() * 4  # a few fp32 roundings of max|x|


def _check_resize_general(got, name, N, C):
    _, _, Ho, Wo, align, half, _ = GENERAL[name]
    x = _general_x(name, N, C)
    ref = _mirror(x, Ho, Wo, align, half)
    tol = 0.5 * _ulp_bf16(ref) + 2.0 ** -20 * x.abs().max()
    err = (got.double() - ref).abs()
    assert got.shape == ref.shape and (err <= tol).all(), f"{name} N={N} C={C}: worst {float((err / tol).max())} x tol"


@functools.lru_cache(maxsize=None)
def _general_must(name, N, C):
    """(mirror, the pixels whose label is binding: margin above 2^-18 max|x|) of a general case."""
    _, _, Ho, Wo, align, half, _ = GENERAL[name]
    x = _general_x(name, N, C)
    ref = _mirror(x, Ho, Wo, align, half)
    return ref, _margin(ref) > 2.0 ** -18 * x.abs().max()


@functools.lru_cache(maxsize=None)
def _general_excused_share():
    """Share of the general cases' pixels the margin rule excuses (bf16 data has exact ties)."""
    must = [_general_must(name, N, C)[1] for name in GENERAL for N in BATCHES for C in ARGMAX_C]
    return float(sum(int((~m).sum()) for m in must)) / sum(m.numel() for m in must)


def _check_argmax_general(got, name, N, C):
    assert _general_excused_share() <= 0.02          # the mirror's own excused share first
    ref, must = _general_must(name, N, C)
    assert got.shape == must.shape
    bad = (got.long() != _first_argmax(ref)) & must
    assert not bad.any(), f"{name} N={N} C={C}: {int(bad.sum())} wrong labels"


# =================================================================================== host launchers
@pytest.mark.parametrize("name", list(EXACT))
def test_host_paths_exact(name):
    _, _, Ho, Wo, align, half, _ = EXACT[name]
    for N in BATCHES:
        for C in RESIZE_C:
            y = K.resize_bilinear_nhwc(_exact_x(name, N, C).to(BF), (Ho, Wo), align, half)
            assert y.dtype == BF and torch.equal(_bits(y), _bits(_exact_ref(name, N, C)[1]))
        for C in ARGMAX_C:
            want = _first_argmax(_exact_ref(name, N, C)[0])
            p = _padded_logits(_exact_x(name, N, C), float("inf"))
            for dt in LABEL_DTYPES:
                lab = K.resize_argmax_nhwc(p, (Ho, Wo), align, half, channels=C, out_dtype=dt)
                assert lab.dtype == dt and torch.equal(lab.long(), want)


@pytest.mark.parametrize("name", list(GENERAL))
def test_host_paths_general(name):
    _, _, Ho, Wo, align, half, _ = GENERAL[name]
    for C in (8, 24):
        _check_resize_general(K.resize_bilinear_nhwc(_general_x(name, 3, C).to(BF), (Ho, Wo), align, half), name, 3, C)
    for C in (5, 21):
        p = _padded_logits(_general_x(name, 3, C), float("inf"))
        _check_argmax_general(K.resize_argmax_nhwc(p, (Ho, Wo), align, half, channels=C), name, 3, C)


def test_host_concat_slot_and_identity_argmax():
    x = _exact_x("ac-3x3-9x9", 3, 24).to(BF)
    out = torch.full((3, 9, 9, 40), 7.0, dtype=BF)
    K.resize_bilinear_nhwc(x, (9, 9), True, out=out, out_channel_offset=8)
    assert torch.equal(_bits(out[..., 8:32]), _bits(_exact_ref("ac-3x3-9x9", 3, 24)[1]))
    assert (out[..., :8] == 7).all() and (out[..., 32:] == 7).all()
    logits = _exact_x("identity-7x5", 3, 21)
    lab = K.resize_argmax_nhwc(_padded_logits(logits, float("inf")), channels=21, out_dtype=torch.uint8)
    assert torch.equal(lab.long(), _first_argmax(logits))


def _bad_launches(dev):
    """(exception, call) pairs every launcher path must refuse."""
    x = torch.zeros((1, 4, 4, 16), dtype=BF, device=dev)
    z = lambda *s, dt=BF: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    return [
        (ValueError, lambda: K.resize_bilinear_nhwc(z(1, 4, 4, 12), (8, 8))),                    # pitch % 8
        (ValueError, lambda: K.resize_bilinear_nhwc(x, (8, 8), channels=12)),                    # C % 8
        (ValueError, lambda: K.resize_bilinear_nhwc(x, (0, 8))),                                 # empty output
        (ValueError, lambda: K.resize_bilinear_nhwc(x, (8, 8), out=z(1, 8, 8, 32), out_channel_offset=4)),
        (ValueError, lambda: K.resize_bilinear_nhwc(x, (8, 8), out=z(1, 8, 8, 24), out_channel_offset=16)),
        (ValueError, lambda: K.resize_bilinear_nhwc(x, (8, 8), out=z(1, 8, 8, 20))),             # out pitch % 8
        (ValueError, lambda: K.resize_bilinear_nhwc(x, (8, 8), out=z(1, 8, 9, 16))),             # wrong out shape
        (ValueError, lambda: K.resize_argmax_nhwc(z(1, 4, 4, 21))),                              # pitch % 8
        (ValueError, lambda: K.resize_argmax_nhwc(z(1, 2, 2, 304), channels=300)),               # C > 256
        (ValueError, lambda: K.resize_argmax_nhwc(x, channels=0)),
        (ValueError, lambda: K.resize_argmax_nhwc(x, channels=17)),                              # C > pitch
        (ValueError, lambda: K.resize_argmax_nhwc(x, (0, 3))),                                   # empty output
        (ValueError, lambda: K.resize_argmax_nhwc(x, (8, 8), out=z(1, 8, 7, dt=torch.int32))),   # wrong out shape
        (TypeError, lambda: K.resize_argmax_nhwc(x, out_dtype=torch.int16)),
        (TypeError, lambda: K.resize_argmax_nhwc(x, out=z(1, 4, 4, dt=torch.float32))),
    ]


def test_launchers_reject_bad_arguments_on_the_host():
    for exc, call in _bad_launches(torch.device("cpu")):
        with pytest.raises(exc):
            call()


# =================================================================================== lowering
def _conv_w(rng, k, cin, cout):
    return (rng.standard_normal((k, k, cin, cout)) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32)


def _front(gb, hw=16):
    images = gb.placeholder("images", "UINT8", [None, hw, hw, 3])
    x = gb.cast(images, "FLOAT", name="Cast")
    x = gb.sub(x, gb.constant("mean", np.asarray([120.0, 115.0, 100.0], dtype=np.float32)), name="Sub")
    x = gb.div(x, gb.constant("std", np.asarray([58.0, 57.0, 57.5], dtype=np.float32)), name="normalized")
    rng = np.random.default_rng(7)
    y = gb.conv2d(x, gb.constant("stem/w", _conv_w(rng, 3, 3, 8)), (2, 2), name="stem")
    return rng, gb.relu(y, name="stem_relu")


def _seg_graph(classes=5, axis=3, fed_size=False):
    """stem(3->8, /2) -> [conv(8->24, /2) -> ResizeBilinear x2 | conv3x3(8->16)] -> ConcatV2 ->
    conv(->classes) + BiasAdd -> ResizeBilinear(align_corners) -> ArgMax -> Cast(UINT8)."""
    gb = GraphBuilder()
    rng, x = _front(gb)
    a = gb.relu(gb.conv2d(x, gb.constant("a/w", _conv_w(rng, 1, 8, 24)), (2, 2), name="a"), name="a_relu")
    a = gb.resize_bilinear(a, gb.constant("a_size", np.asarray([8, 8], dtype=np.int32)), name="a_up")
    b = gb.relu(gb.conv2d(x, gb.constant("b/w", _conv_w(rng, 3, 8, 16)), name="b"), name="b_relu")
    x = gb.concat([a, b], 3, name="concat")
    y = gb.conv2d(x, gb.constant("cls/w", _conv_w(rng, 1, 40, classes) * 3), name="cls")
    b = gb.constant("cls/b", (rng.standard_normal(classes) * 0.1).astype(np.float32))
    logits = gb.bias_add(y, b, name="logits")
    size = gb.placeholder("size", "INT32", [2]) if fed_size else \
        gb.constant("up_size", np.asarray([15, 13], dtype=np.int32))
    up = gb.resize_bilinear(logits, size, name="upsampled", align_corners=True)
    labels = gb.argmax(up, axis, output_type="INT32", name="labels")
    gb.cast(labels, "UINT8", name="label_map")
    return gb.build()


def _imgs(n=2, hw=16, seed=3):
    return torch.randint(0, 256, (n, hw, hw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _compile(graph, imgs, fetches, device="cpu", strict=True, extra=None):
    feeds = {"images:0": (tuple(imgs.shape), "UINT8"), **(extra or {})}
    return CompiledFunction(graph, feeds, list(fetches), device, strict=strict)


def _check_logits(got, ref):
    err = (got.float().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 0.05, err


def _check_labels(got, ref_up, ref_logits, cap=0.5):
    """``got`` agrees with the ArgMax of the interpreter's upsampled logits ``ref_up`` wherever
    their top-2 margin is at least 0.1 max|logits|; at most ``cap`` of the pixels are excused."""
    must = _margin(ref_up) >= 0.1 * ref_logits.abs().max()
    assert (~must).double().mean() <= cap
    bad = (got.cpu().long() != torch.argmax(ref_up, -1)) & must
    assert got.shape == must.shape and not bad.any(), f"{int(bad.sum())} wrong labels"


def test_segmentation_head_compiles_strict():
    g, imgs = _seg_graph(), _imgs()
    ref_logits, ref_up = Session(g).run(["logits:0", "upsampled:0"], {"images:0": imgs})
    plan = _compile(g, imgs, ["logits:0", "label_map:0"])
    s = plan.summary()
    assert s["glue_ops"] == [] and s["kinds"]["resize"] == 1 and s["kinds"]["resize_argmax"] == 1
    assert "elementwise" not in s["kinds"] and "concat" not in s["kinds"]  # the resize writes its concat slot
    cls = [st for st in plan.steps if st.name == "cls"]
    assert len(cls) == 1 and cls[0].kind == "conv"
    assert cls[0].outputs[0].shape[-1] == 5 and cls[0].outputs[0].phys_c == 8
    am = [st for st in plan.steps if st.kind == "resize_argmax"][0]
    assert am.meta["fused_resize"] and am.outputs[0].dtype == torch.uint8     # the Cast became the store type
    logits, labels = plan({"images:0": imgs})
    assert logits.shape == ref_logits.shape and labels.shape == (2, 15, 13) and labels.dtype == torch.uint8
    _check_logits(logits, ref_logits)
    _check_labels(labels, ref_up, ref_logits)


def test_fetched_resize_stays_its_own_step():
    g, imgs = _seg_graph(), _imgs()
    ref_logits, ref_up = Session(g).run(["logits:0", "upsampled:0"], {"images:0": imgs})
    plan = _compile(g, imgs, ["upsampled:0", "labels:0"])
    s = plan.summary()
    assert s["glue_ops"] == [] and s["kinds"]["resize"] == 2 and s["kinds"]["resize_argmax"] == 1
    am = [st for st in plan.steps if st.kind == "resize_argmax"][0]
    assert not am.meta["fused_resize"] and am.outputs[0].dtype == torch.int32  # labels is fetched: no Cast absorbed
    up, labels = plan({"images:0": imgs})
    assert up.shape == ref_up.shape == (2, 15, 13, 5)
    assert (up.float() - ref_up).abs().max() / ref_logits.abs().max() < 0.05
    _check_labels(labels, ref_up, ref_logits)


@pytest.mark.parametrize("kw,op", [(dict(axis=1), "ArgMax"), (dict(classes=300), "ArgMax")], ids=["axis1", "c300"])
def test_ineligible_argmax_stays_glue(kw, op):
    g, imgs = _seg_graph(**kw), _imgs()
    with pytest.raises(CompileError, match="no CDNA4 lowering"):
        _compile(g, imgs, ["labels:0"])
    plan = _compile(g, imgs, ["labels:0"], strict=False)
    s = plan.summary()
    assert op in s["glue_ops"] and "resize_argmax" not in s["kinds"]
    ref_logits, ref_up = Session(g).run(["logits:0", "upsampled:0"], {"images:0": imgs})
    got = plan({"images:0": imgs})[0]
    axis = kw.get("axis", 3)
    ref = torch.argmax(ref_up, axis)
    t = torch.topk(ref_up, 2, axis).values
    must = (t.select(axis, 0) - t.select(axis, 1)) >= 0.1 * ref_logits.abs().max()
    assert got.shape == ref.shape and not ((got.cpu().long() != ref) & must).any()


def test_fed_size_is_left_to_the_glue_fallback(monkeypatch):
    """A size that is not a constant is not lowered: strict mode refuses the op, non-strict mode
    hands it to the glue fallback.  (That fallback infers shapes from a dry run on zeros, so a
    zero size stops it with a division by zero, as it did before the lowering existed.)"""
    g, imgs = _seg_graph(fed_size=True), _imgs()
    extra = {"size:0": ((2,), "INT32")}
    with pytest.raises(CompileError, match="ResizeBilinear"):
        _compile(g, imgs, ["label_map:0"], extra=extra)
    seen, orig = [], CompiledFunction._lower_glue

    def spy(self, node):
        seen.append(node.name)
        return orig(self, node)

    monkeypatch.setattr(CompiledFunction, "_lower_glue", spy)
    try:
        plan = _compile(g, imgs, ["label_map:0"], strict=False, extra=extra)
        assert "resize" not in [st.kind for st in plan.steps if st.name == "upsampled"]
    except ZeroDivisionError:
        pass
    assert "upsampled" in seen


def test_fed_fp32_activation_is_resized():
    """A fed fp32 NHWC tensor goes through the bf16 cast, then the resize kernel."""
    gb = GraphBuilder()
    x = gb.placeholder("feat", "FLOAT", [None, 4, 5, 8])
    gb.resize_bilinear(x, gb.constant("size", np.asarray([7, 9], dtype=np.int32)), name="up", half_pixel_centers=True)
    g = gb.build()
    feat = torch.randn((2, 4, 5, 8), generator=torch.Generator().manual_seed(2))
    plan = CompiledFunction(g, {"feat:0": ((2, 4, 5, 8), "FLOAT")}, ["up:0"], "cpu", strict=True)
    assert plan.summary()["glue_ops"] == [] and plan.summary()["kinds"]["resize"] == 1
    got = plan({"feat:0": feat})[0]
    ref = resize_bilinear_tf(feat, 7, 9, False, True)
    # the input and the output are each rounded to bf16 once: 2^-8 relative, twice
    assert got.shape == ref.shape and (got.float() - ref).abs().max() <= 2.0 ** -7 * feat.abs().max()


def _narrow_graph(pool=False):
    gb = GraphBuilder()
    rng, x = _front(gb)
    y = gb.relu(gb.conv2d(x, gb.constant("n/w", _conv_w(rng, 3, 8, 12)), name="narrow"), name="narrow_relu")
    if pool:
        gb.max_pool(y, (2, 2), (2, 2), name="pooled")
    return gb.build()


def test_padded_conv_output_reads_its_logical_columns():
    g, imgs = _narrow_graph(), _imgs()
    plan = _compile(g, imgs, ["narrow_relu:0"])
    st = [s for s in plan.steps if s.name == "narrow"][0]
    assert st.kind == "conv" and st.outputs[0].phys_c == 16 and st.outputs[0].buf.shape[-1] == 16
    got = plan({"images:0": imgs})[0]
    ref = Session(g).run(["narrow_relu:0"], {"images:0": imgs})[0]
    assert got.shape == ref.shape == (2, 8, 8, 12)
    _check_logits(got, ref)
    assert (st.outputs[0].buf[..., 12:] == 0).all()  # zero filters, zero bias


def test_glue_consumer_of_a_padded_conv_sees_the_logical_columns():
    g, imgs = _narrow_graph(pool=True), _imgs()
    with pytest.raises(CompileError, match="MaxPool"):
        _compile(g, imgs, ["pooled:0"])
    plan = _compile(g, imgs, ["pooled:0"], strict=False)
    assert plan.summary()["glue_ops"] == ["MaxPool"]
    got = plan({"images:0": imgs})[0]
    ref = Session(g).run(["pooled:0"], {"images:0": imgs})[0]
    assert got.shape == ref.shape == (2, 4, 4, 12)
    _check_logits(got, ref)


# =================================================================================== DeepLab-v3
DL = dict(alpha=0.25, num_classes=21, image_hw=(72, 72), crop_hw=(65, 65), output_stride=16)
DL_KINDS = {"preprocess": 1, "dwconv": 13, "conv": 21, "gap": 1, "resize": 1, "resize_argmax": 1}


@pytest.fixture(scope="module")
def deeplab():
    """The graph, three images and the fp32 interpreter's (logits, upsampled, label_map): once."""
    from flink_tensorflow_amd.models.zoo import deeplab_v3_graph_def

    g = Graph.from_graph_def(deeplab_v3_graph_def(**DL))
    imgs = _imgs(3, 72, seed=11)
    ref = Session(g).run(["logits:0", "upsampled:0", "label_map:0"], {"images:0": imgs})
    # the interpreter's own excused share, before any plan runs
    assert (_margin(ref[1]) < 0.1 * ref[0].abs().max()).double().mean() <= 0.5
    return g, imgs, ref


def _check_deeplab_plan(plan, imgs, ref, dev="cpu"):
    s = plan.summary()
    assert s["glue_ops"] == [] and "elementwise" not in s["kinds"] and "glue" not in s["kinds"]
    assert s["kinds"] == DL_KINDS
    assert [st.meta["impl"] for st in plan.steps if st.kind == "dwconv"].count("dwconv_generic") == 1  # the dilated one
    logits, labels = plan({"images:0": imgs.to(dev)})
    assert logits.shape == (3, 5, 5, 21) and labels.shape == (3, 65, 65) and labels.dtype == torch.uint8
    _check_logits(logits, ref[0])
    _check_labels(labels, ref[1], ref[0])
    return labels.cpu()


def test_deeplab_plan_host(deeplab):
    g, imgs, ref = deeplab
    assert ref[0].shape == (3, 5, 5, 21) and ref[2].shape == (3, 65, 65) and ref[2].dtype == torch.uint8
    assert len(torch.unique(ref[2])) > 1   # not one class everywhere
    _check_deeplab_plan(_compile(g, imgs, ["logits:0", "label_map:0"]), imgs, ref)


def test_deeplab_fp8_plan_host(deeplab):
    """In an fp8 plan the resize steps run bf16.  The ASPP concat then has fp8 and bf16 inputs and
    must not be stride-written (one buffer, one format): it is joined by a bf16 copy.  Logits:
    the cosine rule of ``test_fp8``.  Labels: interpolation is a convex combination, so with a
    largest logit error ``e`` they must agree wherever the interpreter's margin exceeds ``2 e``."""
    g, imgs, ref = deeplab
    plan = CompiledFunction(g, {"images:0": (tuple(imgs.shape), "UINT8")}, ["logits:0", "label_map:0"], "cpu",
                            strict=True, precision="fp8")
    s = plan.summary()
    assert s["glue_ops"] == [] and s["fp8_layers"] > 0
    assert s["kinds"]["resize"] == 1 and s["kinds"]["resize_argmax"] == 1 and s["kinds"]["concat"] == 1
    logits, labels = plan({"images:0": imgs})
    assert torch.nn.functional.cosine_similarity(logits.float().flatten(), ref[0].flatten(), dim=0) > 0.99
    e = (logits.float() - ref[0]).abs().max()
    must = _margin(ref[1]) > 2 * e
    assert must.any() and not ((labels.long() != ref[2].long()) & must).any()


def test_deeplab_model_segments_on_the_host(deeplab):
    from flink_tensorflow_amd.models.zoo import DeepLabV3Model

    _, imgs, ref = deeplab
    m = DeepLabV3Model(buckets=(3,), device="cpu", **DL)
    m.open()
    try:
        maps = m.segment(list(imgs.numpy()))
        (res, tags, _), = m.submit(list(imgs.numpy()), np.zeros(3), [5, 6, 7])
    finally:
        m.close()
    assert len(maps) == 3 and all(a.shape == (65, 65) and a.dtype == np.uint8 for a in maps)
    assert np.array_equal(np.stack(maps), ref[2].numpy())  # host: the interpreter
    assert tags == [5, 6, 7] and np.array_equal(np.stack(res), ref[2].numpy())


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
    if isinstance(fill, float) and fill != fill:
        return bool(torch.isnan(lo).all() and torch.isnan(hi).all())
    return bool((lo == fill).all() and (hi == fill).all())


def _gpu_resize(x, Ho, Wo, align, half, dev):
    """The kernel on x (float64 -> bf16) between NaN bands, writing between sentinel bands, twice."""
    xv, xbuf = _banded(x.to(BF), float("nan"), dev)
    N, _, _, C = x.shape
    n = N * Ho * Wo * C
    outs = []
    for _ in range(2):
        ov, obuf = _banded(torch.full((N, Ho, Wo, C), SENT, dtype=BF), SENT, dev)
        y = K.resize_bilinear_nhwc(xv, (Ho, Wo), align, half, out=ov)
        assert y is ov and _bands_intact(obuf, n, SENT), "stray store"
        outs.append(ov.cpu())
    assert _bands_intact(xbuf, x.numel(), float("nan")) and torch.equal(xv.cpu().double(), x)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two runs differ"
    return outs[0]


def _gpu_argmax(x, C, Ho, Wo, align, half, dt, path, dev):
    """The kernel on logits x (float64, C channels, pitch ceil8(C), padding 2^100) between NaN
    bands, the label map between sentinel bands, twice."""
    pv, pbuf = _banded(_padded_logits(x, SENT), float("nan"), dev)
    N = x.shape[0]
    n = N * Ho * Wo
    outs = []
    for _ in range(2):
        ov, obuf = _banded(torch.full((N, Ho, Wo), LABEL_SENT[dt], dtype=dt), LABEL_SENT[dt], dev)
        K.resize_argmax_nhwc(pv, (Ho, Wo), align, half, channels=C, out=ov, path=path)
        assert _bands_intact(obuf, n, LABEL_SENT[dt]), "stray store"
        outs.append(ov.cpu())
    assert _bands_intact(pbuf, pv.numel(), float("nan"))
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    return outs[0]


def _paths(H, W, Ho, Wo):
    """The launcher's choice, the simple kernel, and the staged kernel where it applies."""
    up = Ho >= H and Wo >= W
    return (0, K.RESIZE_ARGMAX_PATHS["simple"]) + ((K.RESIZE_ARGMAX_PATHS["staged"],) if up else ())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EXACT))
def test_resize_kernel_bit_exact(name):
    H, W, Ho, Wo, align, half, _ = EXACT[name]
    dev = torch.device("cuda", 0)
    for N in BATCHES:
        for C in RESIZE_C:
            ref = _exact_ref(name, N, C)[1]
            y = _gpu_resize(_exact_x(name, N, C), Ho, Wo, align, half, dev)
            bad = (_bits(y) != _bits(ref)).nonzero()
            assert len(bad) == 0, f"{name} N={N} C={C}: {len(bad)} differ, first {bad[:3].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EXACT))
def test_argmax_kernel_index_exact(name):
    H, W, Ho, Wo, align, half, _ = EXACT[name]
    dev = torch.device("cuda", 0)
    for N in BATCHES:
        for C in ARGMAX_C:
            want = _first_argmax(_exact_ref(name, N, C)[0])
            for dt in LABEL_DTYPES:
                for path in _paths(H, W, Ho, Wo):
                    got = _gpu_argmax(_exact_x(name, N, C), C, Ho, Wo, align, half, dt, path, dev)
                    bad = (got.long() != want).nonzero()
                    assert len(bad) == 0, f"{name} N={N} C={C} {dt} path={path}: {len(bad)} differ, {bad[:3].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GENERAL))
def test_kernels_general_geometries(name):
    H, W, Ho, Wo, align, half, _ = GENERAL[name]
    dev = torch.device("cuda", 0)
    for N in BATCHES:
        for C in RESIZE_C:
            _check_resize_general(_gpu_resize(_general_x(name, N, C), Ho, Wo, align, half, dev), name, N, C)
        for C in ARGMAX_C:
            for path in _paths(H, W, Ho, Wo):
                got = _gpu_argmax(_general_x(name, N, C), C, Ho, Wo, align, half, torch.uint8, path, dev)
                _check_argmax_general(got, name, N, C)


@pytest.mark.gpu
def test_resize_kernel_concat_slot_and_padded_source():
    dev = torch.device("cuda", 0)
    name = "ac-3x3-9x9"
    ref = _exact_ref(name, 3, 24)[1]
    xv, xbuf = _banded(_exact_x(name, 3, 24).to(BF), float("nan"), dev)
    ov, obuf = _banded(torch.full((3, 9, 9, 40), SENT, dtype=BF), SENT, dev)
    K.resize_bilinear_nhwc(xv, (9, 9), True, out=ov, out_channel_offset=8)
    o = ov.cpu()
    assert torch.equal(_bits(o[..., 8:32]), _bits(ref))
    assert (o[..., :8] == SENT).all() and (o[..., 32:] == SENT).all(), "neighbours written"
    assert _bands_intact(obuf, ov.numel(), SENT) and _bands_intact(xbuf, xv.numel(), float("nan"))
    # a source of pitch 40 read at its first 24 channels
    src = torch.full((3, 3, 3, 40), float("nan"), dtype=BF)
    src[..., :24] = _exact_x(name, 3, 24).to(BF)
    y = K.resize_bilinear_nhwc(src.to(dev), (9, 9), True, channels=24)
    assert y.shape == (3, 9, 9, 24) and torch.equal(_bits(y.cpu()), _bits(ref))


@pytest.mark.gpu
def test_argmax_window_that_does_not_fit_takes_the_simple_kernel():
    """Identity over 20 x 70 x 151: the 16 x 67-pixel window of a tile is past the LDS budget."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-64, 65, (1, 20, 70, 151), generator=g).to(F64)
    want = _first_argmax(x)
    p = _padded_logits(x, SENT).to(dev)
    assert torch.equal(K.resize_argmax_nhwc(p, channels=151, out_dtype=torch.uint8).cpu().long(), want)
    with pytest.raises(ValueError):
        K.resize_argmax_nhwc(p, channels=151, path=K.RESIZE_ARGMAX_PATHS["staged"])
    # the same shape at 21 channels fits: staged, several tiles per axis, identical labels
    x = x[..., :21].contiguous()
    p = _padded_logits(x, SENT).to(dev)
    for path in (0, 1, -1):
        assert torch.equal(K.resize_argmax_nhwc(p, channels=21, out_dtype=torch.uint8, path=path).cpu().long(),
                           _first_argmax(x))


@pytest.mark.gpu
def test_element_offsets_past_2_31():
    """16385 x 16385 pixels of 8 channels are 2^31 + 262k elements: offsets must be 64-bit.  The
    broadcast writes that many, the identity ArgMax reads that many; both are checked on the device."""
    dev = torch.device("cuda", 0)
    S = 16385
    v = torch.arange(-3, 5, dtype=F32).to(BF).to(dev)
    big = K.resize_bilinear_nhwc(v.view(1, 1, 1, 8), (S, S), True)
    assert big.numel() > 2 ** 31 and bool((big.view(-1, 8) == v).all())
    # channel (pixel index mod 8) holds the only 1 of its pixel
    want = (torch.arange(S * S, device=dev) % 8).to(torch.uint8)
    big.zero_()
    big.view(-1, 8).scatter_(1, want.long().view(-1, 1), 1.0)
    for path in (K.RESIZE_ARGMAX_PATHS["staged"], K.RESIZE_ARGMAX_PATHS["simple"]):
        lab = K.resize_argmax_nhwc(big, out_dtype=torch.uint8, path=path)
        assert bool((lab.view(-1) == want).all()), path
        del lab
    del big, want
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_launchers_reject_bad_arguments_on_the_device():
    dev = torch.device("cuda", 0)
    for exc, call in _bad_launches(dev):
        with pytest.raises(exc):
            call()
    x = torch.zeros((1, 4, 4, 16), dtype=BF, device=dev)
    with pytest.raises(TypeError):
        K.resize_bilinear_nhwc(x.float(), (8, 8))
    with pytest.raises(TypeError):
        K.resize_argmax_nhwc(x.float())
    with pytest.raises(ValueError):
        K.resize_argmax_nhwc(x, path=2)


# =================================================================================== GPU: the plans
@pytest.mark.gpu
def test_segmentation_head_plan_gpu():
    g, imgs = _seg_graph(), _imgs()
    dev = torch.device("cuda", 0)
    ref_logits, ref_up = Session(g).run(["logits:0", "upsampled:0"], {"images:0": imgs})
    plan = _compile(g, imgs, ["logits:0", "label_map:0"], dev)
    s = plan.summary()
    assert s["glue_ops"] == [] and s["kinds"]["resize"] == 1 and s["kinds"]["resize_argmax"] == 1
    logits, labels = plan({"images:0": imgs.to(dev)})
    _check_logits(logits, ref_logits)
    _check_labels(labels, ref_up, ref_logits)
    # the unfused pair gives the same kind of answer from the padded buffer
    plan2 = _compile(g, imgs, ["upsampled:0", "labels:0"], dev)
    up, labels2 = plan2({"images:0": imgs.to(dev)})
    assert (up.float().cpu() - ref_up).abs().max() / ref_logits.abs().max() < 0.05
    _check_labels(labels2, ref_up, ref_logits)


@pytest.mark.gpu
def test_padded_conv_output_gpu():
    g, imgs = _narrow_graph(), _imgs()
    dev = torch.device("cuda", 0)
    plan = _compile(g, imgs, ["narrow_relu:0"], dev)
    got = plan({"images:0": imgs.to(dev)})[0]
    ref = Session(g).run(["narrow_relu:0"], {"images:0": imgs})[0]
    assert got.shape == ref.shape
    _check_logits(got, ref)


@pytest.mark.gpu
def test_deeplab_plan_and_model_gpu(deeplab):
    from flink_tensorflow_amd.models.zoo import DeepLabV3Model

    g, imgs, ref = deeplab
    dev = torch.device("cuda", 0)
    plan = _compile(g, imgs, ["logits:0", "label_map:0"], dev)
    assert plan.summary()["hip_graph"]
    labels = _check_deeplab_plan(plan, imgs, ref, dev)
    again = plan({"images:0": imgs.to(dev)})
    assert torch.equal(again[1].cpu(), labels)            # a second replay is bit-identical
    m = DeepLabV3Model(buckets=(3,), lanes=1, **DL)
    m.open()
    try:
        s = m.plan_summary()
        assert s["glue_ops"] == [] and s["kinds"]["resize_argmax"] == 1
        maps = m.segment(list(imgs.numpy()))
        done = []
        for i in range(3):   # one record per batch: results come back in submission order
            done += m.submit([imgs[i].numpy()], np.zeros(1), [i])
        done += m.drain()
    finally:
        m.close()
    assert all(a.shape == (65, 65) and a.dtype == np.uint8 for a in maps)
    assert np.array_equal(np.stack(maps), labels.numpy())
    assert [t for _, tags, _ in done for t in tags] == [0, 1, 2]
    batched = np.stack([r for res, _, _ in done for r in res])
    must = (_margin(ref[1]) >= 0.1 * ref[0].abs().max()).numpy()
    assert batched.shape == (3, 65, 65) and batched.dtype == np.uint8
    assert np.array_equal(batched[must], labels.numpy()[must])
