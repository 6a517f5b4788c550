"""Object detection: the NMS interpreter ops, ``kernels/detection.hip`` (box decode + per-class
greedy NMS + top-T merge), their lowering and SSD-MobileNet-V1.

**The mirror** (``_mirror``) is an independent float64 brute-force implementation of the
definition in ``graph/ops_nn.py``, written with plain loops over images, classes, candidates
and kept boxes; it calls nothing of the package.  It rounds where the kernel rounds (the fp32
box decode in the documented order) and takes every IoU in float64.  Greedy selection
cascades, so no mismatch can be excused: instead the mirror asserts, on the inputs of every
case and before anything is compared, that

* every IoU it evaluates differs from ``iou_threshold`` by more than 2^-20 (fp32 IoU of
  in-range boxes carries a few ulps, about 2^-22) - or, in the cases that are about it, equals
  it exactly,
* every score differs from ``score_threshold``,
* the keys (-score, class, index) it sorts by are pairwise different, so the pinned order is
  strict.

Exact cases put boxes on the 1/64 grid (areas, intersections and unions are small integers
over 4096, exact in fp32 and bf16) and scores on the bf16 grid k/256 (with many ties): the
kernel must then agree bit for bit.  The fused-decode cases compare boxes within ``2^-20 *
max(|centre|, size)`` of the mirror's: 16 fp32 ulps for ``expf`` plus four roundings, the
margin rule of ``tests/test_segmentation.py``.
"""
import functools

import numpy as np
import pytest
import torch

from flink_tensorflow_amd.graph.builder import GraphBuilder
from flink_tensorflow_amd.graph.compiler import CompiledFunction, CompileError
from flink_tensorflow_amd.graph.graph import Graph
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.ops import kernels as K

BF = torch.bfloat16
SENT = 2.0 ** 100
EPS = 2.0 ** -20


# =================================================================================== the mirror
def _decode32(enc, anchors, inv_scales):
    """The documented fp32 decode, one rounding per operation (numpy float32 arithmetic)."""
    e, a, s = (np.asarray(v, dtype=np.float32) for v in (enc, anchors, inv_scales))
    cy = (e[..., 0] * s[0]) * a[:, 2] + a[:, 0]
    cx = (e[..., 1] * s[1]) * a[:, 3] + a[:, 1]
    h = np.exp(e[..., 2] * s[2]) * a[:, 2]
    w = np.exp(e[..., 3] * s[3]) * a[:, 3]
    hh, hw = np.float32(0.5) * h, np.float32(0.5) * w
    out = np.stack([cy - hh, cx - hw, cy + hh, cx + hw], axis=-1)
    assert out.dtype == np.float32
    return out


def _iou64(a, b):
    ay1, ay2, ax1, ax2 = min(a[0], a[2]), max(a[0], a[2]), min(a[1], a[3]), max(a[1], a[3])
    by1, by2, bx1, bx2 = min(b[0], b[2]), max(b[0], b[2]), min(b[1], b[3]), max(b[1], b[3])
    area_a, area_b = (ay2 - ay1) * (ax2 - ax1), (by2 - by1) * (bx2 - bx1)
    if area_a <= 0 or area_b <= 0:
        return 0.0
    inter = max(0.0, min(ay2, by2) - max(ay1, by1)) * max(0.0, min(ax2, bx2) - max(ax1, bx1))
    return inter / (area_a + area_b - inter)


def _mirror(boxes, scores, mpc, T, iou_thr, score_thr, pad=False, clip=True, equal_ok=False):
    """float64 brute force.  ``boxes`` [B, N, q, 4], ``scores`` [B, N, C].  Returns (boxes,
    scores, classes, valid, indices) as float64 / int arrays; asserts its own margins."""
    bx, sc = np.asarray(boxes, dtype=np.float64), np.asarray(scores, dtype=np.float64)
    B, N, C = sc.shape
    q = bx.shape[2]
    iou_thr, score_thr = float(np.float32(iou_thr)), float(np.float32(score_thr))
    if pad:
        T = min(T, mpc * C)
    ob, os_, oc = np.zeros((B, T, 4)), np.zeros((B, T)), np.zeros((B, T))
    ov, oi = np.zeros((B,), dtype=np.int64), np.full((B, T), -1, dtype=np.int64)
    for b in range(B):
        merged = []
        for c in range(C):
            col = sc[b, :, c].tolist()
            assert all(s != score_thr for s in col), "a score sits on the threshold"
            cand = sorted((-s, i) for i, s in enumerate(col) if s > score_thr)   # NaN > x is False
            cb = bx[b, :, c if q > 1 else 0].tolist()
            kept = []
            for _, i in cand:
                if len(kept) >= min(mpc, N):
                    break
                ok = True
                for k in kept:
                    v = _iou64(cb[i], cb[k])
                    assert abs(v - iou_thr) > EPS or (equal_ok and v == iou_thr), f"IoU {v} too close to {iou_thr}"
                    if v > iou_thr:
                        ok = False
                        break
                if ok:
                    kept.append(i)
            merged += [(-col[i], c, i) for i in kept]
        assert len(set(merged)) == len(merged)
        merged.sort()
        merged = merged[:T]
        ov[b] = len(merged)
        for t, (ns, c, i) in enumerate(merged):
            ob[b, t], os_[b, t], oc[b, t], oi[b, t] = bx[b, i, c if q > 1 else 0], -ns, c, i
    if clip:
        ob = np.clip(ob, 0.0, 1.0)
    return ob, os_, oc, ov, oi


# =================================================================================== data
def _grid_boxes(rng, B, N, q=1, lo=-64, hi=128, smax=24):
    """Corners on the 1/64 grid inside [lo/64, (hi + smax)/64): exact in bf16 (|k| < 256).  A tenth
    have swapped corners and a twentieth no area."""
    y1, x1 = rng.integers(lo, hi, (B, N, q)), rng.integers(lo, hi, (B, N, q))
    h, w = rng.integers(1, smax + 1, (B, N, q)), rng.integers(1, smax + 1, (B, N, q))
    h = np.where(rng.random((B, N, q)) < 0.05, 0, h)
    bx = np.stack([y1, x1, y1 + h, x1 + w], axis=-1).astype(np.float64)
    swap = rng.random((B, N, q)) < 0.1
    bx[swap] = bx[swap][:, [2, 3, 0, 1]]
    return bx / 64.0


def _grid_scores(rng, B, N, C, nan_share=0.02):
    """Scores k/256 (bf16-exact, N > 256 forces ties), a few NaN, some negative."""
    sc = rng.integers(-16, 256, (B, N, C)).astype(np.float64) / 256.0
    sc[rng.random((B, N, C)) < nan_share] = np.nan
    return sc


# (B, C, N, max_per_class, max_total, pad_per_class, clip_boxes, box dtype): every B, C, N,
# max_per_class and T of the envelope's corner list at least once, N at the launcher's limit
EXACT = {
    "b1-c1-n1": (1, 1, 1, 1, 1, False, True, "bf16"),
    "b3-c3-n63": (3, 3, 63, 5, 100, False, True, "f32"),
    "b1-c3-n64": (1, 3, 64, 100, 1, False, False, "bf16"),
    "b3-c1-n65": (3, 1, 65, 5, 100, True, True, "bf16"),
    "b1-c3-n300": (1, 3, 300, 100, 100, False, False, "f32"),
    "b3-c3-n300-t1": (3, 3, 300, 5, 1, False, True, "bf16"),
    "b1-c90-n64-k1": (1, 90, 64, 1, 100, True, True, "f32"),
    "b1-c90-n1917": (1, 90, 1917, 100, 100, False, True, "bf16"),
    "b3-c3-n1917": (3, 3, 1917, 100, 100, False, False, "f32"),
    "b1-c1-n4096": (1, 1, K.NMS_MAX_BOXES, 100, 100, False, True, "bf16"),
    "b1-c3-n4096-k5": (1, 3, K.NMS_MAX_BOXES, 5, 1, False, True, "f32"),
}
IOU_THR, SCORE_THR = 0.37, 0.3   # neither is a k/256 score; 0.37 is no ratio of small integers


@functools.lru_cache(maxsize=None)
def _exact_case(name):
    """Inputs (float64) and the mirror's answer for an exact case: computed once, never changed."""
    B, C, N, mpc, T, pad, clip, _ = EXACT[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    bx, sc = _grid_boxes(rng, B, N), _grid_scores(rng, B, N, C)
    return bx, sc, _mirror(bx, sc, mpc, T, IOU_THR, SCORE_THR, pad, clip)


def _same(got, want, boxes_exact=True, tol=None):
    gb, gs, gc, gv = (torch.as_tensor(t).cpu() for t in got)
    wb, ws, wc, wv = want[:4]
    assert gb.dtype == gs.dtype == gc.dtype == torch.float32 and gv.dtype == torch.int32
    assert gv.tolist() == wv.tolist(), (gv.tolist(), wv.tolist())
    assert torch.equal(gc, torch.from_numpy(wc).float()), "classes differ"
    assert torch.equal(gs, torch.from_numpy(ws).float()), "scores differ"      # also the zero rows past valid
    if boxes_exact:
        assert torch.equal(gb, torch.from_numpy(wb).float()), "boxes differ"
    else:
        assert gb.shape == wb.shape and bool(((gb.double() - torch.from_numpy(wb)).abs() <= torch.from_numpy(tol)).all())
    for b, n in enumerate(wv.tolist()):
        assert not gb[b, n:].any() and not gs[b, n:].any() and not gc[b, n:].any(), "rows past valid are not zero"


# =================================================================================== interpreter ops (CPU)
def _nms_graph(B, N, C, q, mpc, T, iou, thr, pad, clip):
    gb = GraphBuilder()
    boxes = gb.placeholder("boxes", "FLOAT", [B, N, q, 4])
    scores = gb.placeholder("scores", "FLOAT", [B, N, C])
    gb.combined_nms(boxes, scores, mpc, T, iou, thr, pad_per_class=pad, clip_boxes=clip, name="nms")
    return gb.build()


def _run_op(bx, sc, mpc, T, iou, thr, pad=False, clip=True):
    B, N, C = sc.shape
    g = _nms_graph(B, N, C, bx.shape[2], mpc, T, iou, thr, pad, clip)
    return Session(g).run(["nms:0", "nms:1", "nms:2", "nms:3"],
                          {"boxes:0": torch.from_numpy(bx).float(), "scores:0": torch.from_numpy(sc).float()})


@pytest.mark.parametrize("q_is_c", [False, True], ids=["q1", "qC"])
@pytest.mark.parametrize("pad", [False, True], ids=["nopad", "pad"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
def test_combined_nms_op_matches_the_mirror(q_is_c, pad, clip):
    B, N, C, mpc, T = 2, 150, 4, 7, 40          # pad: T = min(40, 28); boxes reach outside [0, 1]
    rng = np.random.default_rng(5 + 4 * q_is_c + 2 * pad + clip)
    bx, sc = _grid_boxes(rng, B, N, C if q_is_c else 1), _grid_scores(rng, B, N, C)
    want = _mirror(bx, sc, mpc, T, IOU_THR, SCORE_THR, pad, clip)
    assert want[0].shape[1] == (28 if pad else 40) and want[3].min() > 0
    assert (bx.min() < 0 and bx.max() > 1) and (clip or want[0].max() > 1)
    _same(_run_op(bx, sc, mpc, T, IOU_THR, SCORE_THR, pad, clip), want)


def test_combined_nms_op_edge_cases():
    rng = np.random.default_rng(11)
    bx, sc = _grid_boxes(rng, 2, 40), _grid_scores(rng, 2, 40, 3)
    # a threshold above every score: nothing is valid, every row is zero
    want = _mirror(bx, sc, 5, 10, IOU_THR, 1.5)
    assert want[3].tolist() == [0, 0]
    _same(_run_op(bx, sc, 5, 10, IOU_THR, 1.5), want)
    # max_per_class > N, and T larger / smaller than the number kept
    for mpc, T in ((1000, 1000), (1000, 3)):
        want = _mirror(bx, sc, mpc, T, IOU_THR, SCORE_THR)
        assert (want[3] < 1000).all() and (T == 3 or (want[3] > 3).all())
        _same(_run_op(bx, sc, mpc, T, IOU_THR, SCORE_THR), want)
    # zero-area boxes are never suppressed and never suppress; swapped corners count as the same box
    bx = np.asarray([[[[0, 0, 0.5, 0.5]], [[0.5, 0.5, 0, 0]], [[0.25, 0.25, 0.25, 0.75]], [[0.25, 0.25, 0.25, 0.75]]]])
    sc = np.asarray([[[0.9], [0.8], [0.7], [0.6]]])
    want = _mirror(bx, sc, 4, 4, 0.5, 0.0)
    assert want[4].tolist() == [[0, 2, 3, -1]]
    _same(_run_op(bx, sc, 4, 4, 0.5, 0.0), want)


def test_ties_follow_the_pinned_order():
    """bf16-grid scores with only four values: box index orders a class, class then index the merge."""
    rng = np.random.default_rng(3)
    bx = _grid_boxes(rng, 1, 60, smax=6)
    sc = rng.integers(1, 5, (1, 60, 3)).astype(np.float64) / 4.0
    want = _mirror(bx, sc, 60, 180, IOU_THR, 0.0)
    got = _run_op(bx, sc, 60, 180, IOU_THR, 0.0)
    _same(got, want)
    n = int(want[3][0])
    order = list(zip((-want[1][0, :n]).tolist(), want[2][0, :n].tolist(), want[4][0, :n].tolist()))
    assert order == sorted(order) and n > 100 and len({o[0] for o in order}) <= 4


def _equality_case():
    """IoU exactly 1/2 on the 1/64 grid: [0, 32] x [0, 32] and [0, 32] x [0, 16] over 64.  The second
    box is not suppressed at threshold 0.5 (the test is ``>``), but is at 1/2 - 2^-13."""
    bx = np.asarray([[[[0, 0, 32, 32]], [[0, 0, 32, 16]], [[40, 40, 60, 60]]]]) / 64.0
    sc = np.asarray([[[0.75], [0.5], [0.25]]])
    assert _iou64(bx[0, 0, 0], bx[0, 1, 0]) == 0.5
    return bx, sc


def test_iou_equal_to_the_threshold_does_not_suppress():
    bx, sc = _equality_case()
    want = _mirror(bx, sc, 3, 3, 0.5, 0.0, equal_ok=True)
    assert want[4].tolist() == [[0, 1, 2]]
    _same(_run_op(bx, sc, 3, 3, 0.5, 0.0), want)
    below = 0.5 - 2.0 ** -13
    want = _mirror(bx, sc, 3, 3, below, 0.0)
    assert want[4].tolist() == [[0, 2, -1]]
    _same(_run_op(bx, sc, 3, 3, below, 0.0), want)


def _single_graph(op, N, mpc, iou, thr=None, sigma=None, **attrs):
    gb = GraphBuilder()
    ins = [gb.placeholder("boxes", "FLOAT", [N, 4]), gb.placeholder("scores", "FLOAT", [N]),
           gb.constant("max_output_size", np.asarray(mpc, dtype=np.int32)),
           gb.constant("iou_threshold", np.asarray(iou, dtype=np.float32))]
    if thr is not None:
        ins.append(gb.constant("score_threshold", np.asarray(thr, dtype=np.float32)))
    if sigma is not None:
        ins.append(gb.constant("soft_nms_sigma", np.asarray(sigma, dtype=np.float32)))
    gb.op(op, ins, name="nms", **attrs)
    return gb.build()


def test_single_class_nms_ops():
    rng = np.random.default_rng(21)
    bx, sc = _grid_boxes(rng, 1, 80, lo=0, hi=48), _grid_scores(rng, 1, 80, 1, nan_share=0.0)
    feeds = {"boxes:0": torch.from_numpy(bx[0, :, 0]).float(), "scores:0": torch.from_numpy(sc[0, :, 0]).float()}
    want = _mirror(bx, sc, 60, 60, IOU_THR, SCORE_THR, clip=False)
    n = int(want[3][0])
    idx = want[4][0, :n].tolist()
    assert 3 < n < 60
    v3, = Session(_single_graph("NonMaxSuppressionV3", 80, 60, IOU_THR, SCORE_THR)).run(["nms:0"], feeds)
    assert v3.dtype == torch.int32 and v3.tolist() == idx
    all_in = _mirror(bx, sc, 60, 60, IOU_THR, -1.0, clip=False)       # V2 has no score threshold
    v2, = Session(_single_graph("NonMaxSuppressionV2", 80, 60, IOU_THR)).run(["nms:0"], feeds)
    assert v2.tolist() == all_in[4][0, :int(all_in[3][0])].tolist() and v2.tolist() != idx
    v4 = Session(_single_graph("NonMaxSuppressionV4", 80, 60, IOU_THR, SCORE_THR, pad_to_max_output_size=True)).run(
        ["nms:0", "nms:1"], feeds)
    assert v4[0].tolist() == idx + [0] * (60 - n) and int(v4[1]) == n and v4[1].dtype == torch.int32
    v4u = Session(_single_graph("NonMaxSuppressionV4", 80, 60, IOU_THR, SCORE_THR)).run(["nms:0", "nms:1"], feeds)
    assert v4u[0].tolist() == idx and int(v4u[1]) == n
    v5 = Session(_single_graph("NonMaxSuppressionV5", 80, 60, IOU_THR, SCORE_THR, 0.0)).run(["nms:0", "nms:1", "nms:2"], feeds)
    assert v5[0].tolist() == idx and int(v5[2]) == n
    assert torch.equal(v5[1], torch.from_numpy(want[1][0, :n]).float())
    with pytest.raises(NotImplementedError, match="soft_nms_sigma"):
        Session(_single_graph("NonMaxSuppressionV5", 80, 60, IOU_THR, SCORE_THR, 0.5)).run(["nms:0"], feeds)


# =================================================================================== launcher, host path
@pytest.mark.parametrize("name", list(EXACT))
def test_host_path_exact(name):
    B, C, N, mpc, T, pad, clip, dt = EXACT[name]
    bx, sc, want = _exact_case(name)
    dtype = BF if dt == "bf16" else torch.float32
    got = K.combined_nms(torch.from_numpy(bx).to(dtype), torch.from_numpy(sc).to(BF), mpc, T, IOU_THR, SCORE_THR, pad, clip)
    _same(got, want)


def _pitched_scores(sc, ld, off, fill):
    B, N, C = sc.shape
    wide = np.full((B, N, ld), fill, dtype=np.float64)
    wide[..., off:off + C] = sc
    return wide


def test_host_path_pitch_and_offset():
    bx, sc, want = _exact_case("b3-c3-n63")
    wide = torch.from_numpy(_pitched_scores(sc, 8, 1, SENT)).to(BF)
    got = K.combined_nms(torch.from_numpy(bx).float(), wide, 5, 100, IOU_THR, SCORE_THR, num_classes=3, class_offset=1)
    _same(got, want)


def _decode_case(exact, B=2, N=300, C=3, seed=31):
    """Encodings, anchors, reciprocal scales, scores.  ``exact``: th = tw = 0 and everything
    dyadic, so the decode is exact; else encodings = normal rounded to bf16."""
    rng = np.random.default_rng(seed)
    a = np.stack([rng.integers(0, 65, N), rng.integers(0, 65, N), 8 * rng.integers(1, 4, N), 8 * rng.integers(1, 4, N)],
                 axis=1) / 64.0
    if exact:
        enc = np.concatenate([rng.integers(-4, 5, (B, N, 2)), np.zeros((B, N, 2))], axis=-1).astype(np.float64)
        inv = np.asarray([0.125, 0.125, 0.25, 0.25])
    else:
        enc = torch.from_numpy(rng.standard_normal((B, N, 4))).to(BF).double().numpy()
        inv = (np.float32(1) / np.asarray([10, 10, 5, 5], dtype=np.float32)).astype(np.float64)
    return enc, a, inv, _grid_scores(rng, B, N, C)


def _decode_tol(enc, a, inv, idx):
    """2^-20 * max(|centre|, size) per selected box (rows past valid: 0)."""
    box = _decode32(enc, a, inv).astype(np.float64)
    cy, cx = (box[..., 0] + box[..., 2]) / 2, (box[..., 1] + box[..., 3]) / 2
    mag = np.maximum(np.maximum(np.abs(cy), np.abs(cx)), np.maximum(box[..., 2] - box[..., 0], box[..., 3] - box[..., 1]))
    tol = np.zeros(idx.shape + (4,))
    for b in range(idx.shape[0]):
        for t, i in enumerate(idx[b].tolist()):
            if i >= 0:
                tol[b, t] = EPS * mag[b, i]
    return tol


@pytest.mark.parametrize("exact", [True, False], ids=["dyadic", "normal"])
def test_host_path_fused_decode(exact):
    enc, a, inv, sc = _decode_case(exact)
    boxes = _decode32(enc, a, inv)[:, :, None]
    want = _mirror(boxes, sc, 20, 50, IOU_THR, SCORE_THR, clip=False)
    got = K.combined_nms(torch.from_numpy(enc).to(BF), torch.from_numpy(sc).to(BF), 20, 50, IOU_THR, SCORE_THR,
                         clip_boxes=False, anchors=torch.from_numpy(a).float(), box_scales=inv.tolist())
    _same(got, want, boxes_exact=exact, tol=_decode_tol(enc, a, inv, want[4]))


def _past_the_limits(dev):
    def call(N=8, C=2, mpc=4, T=4, **kw):
        bx = torch.zeros((1, N, 1, 4), dtype=torch.float32, device=dev)
        sc = torch.zeros((1, N, C), dtype=BF, device=dev)
        return lambda: K.combined_nms(bx, sc, mpc, T, 0.5, 0.0, **kw)

    return [call(N=K.NMS_MAX_BOXES + 1), call(C=K.NMS_MAX_CLASSES + 1), call(N=512, mpc=K.NMS_MAX_PER_CLASS + 1),
            call(T=K.NMS_MAX_TOTAL + 1)]


def test_eligibility_and_bad_arguments_on_the_host():
    assert K.nms_eligible(K.NMS_MAX_BOXES, K.NMS_MAX_CLASSES, K.NMS_MAX_PER_CLASS, K.NMS_MAX_TOTAL)
    assert not K.nms_eligible(K.NMS_MAX_BOXES + 1, 1, 1, 1) and not K.nms_eligible(8, K.NMS_MAX_CLASSES + 1, 1, 1)
    assert not K.nms_eligible(8, 1, K.NMS_MAX_PER_CLASS + 1, 1) and not K.nms_eligible(8, 1, 1, K.NMS_MAX_TOTAL + 1)
    assert not K.nms_eligible(8, 2, 1, 1, q=2)
    assert K.nms_scratch_numel(3, 5, 7) == 3 * 5 * 7 + 8
    bx, sc = torch.zeros((1, 8, 1, 4)), torch.zeros((1, 8, 2))
    for kw in (dict(class_offset=2), dict(num_classes=3), dict(anchors=torch.zeros((8, 4))),
               dict(anchors=torch.zeros((7, 4)), box_scales=[1, 1, 1, 1])):
        with pytest.raises(ValueError):
            K.combined_nms(bx, sc, 4, 4, 0.5, 0.0, **kw)
    with pytest.raises(ValueError):
        K.combined_nms(torch.zeros((1, 9, 1, 4)), sc, 4, 4, 0.5, 0.0)
    with pytest.raises(ValueError):
        K.combined_nms(bx, sc, 0, 4, 0.5, 0.0)


# =================================================================================== lowering
HEAD = dict(B=2, N=300, C=3, mpc=20, T=50)


def _head_graph(N=HEAD["N"], C=HEAD["C"], q1=True, fed_total=False, mpc=HEAD["mpc"], T=HEAD["T"], anchors=None, inv=None,
                B=HEAD["B"]):
    """encodings, scores [B, N, C + 1] -> drop column 0 -> decode_boxes -> CombinedNonMaxSuppression
    (``q1``), or per-class boxes fed directly (not ``q1``)."""
    gb = GraphBuilder()
    scores = gb.last_axis_slice(gb.placeholder("scores", "FLOAT", [B, N, C + 1]), 1, C + 1, name="class_scores")
    if q1:
        enc = gb.placeholder("encodings", "FLOAT", [B, N, 4])
        boxes = gb.decode_boxes(enc, anchors, tuple(1.0 / inv), name="decode")
    else:
        boxes = gb.placeholder("boxes", "FLOAT", [B, N, C, 4])
    total = gb.placeholder("total", "INT32", []) if fed_total else T
    gb.combined_nms(boxes, scores, mpc, total, IOU_THR, SCORE_THR, clip_boxes=False, name="nms")
    return gb.build()


NMS_OUT = ["nms:0", "nms:1", "nms:2", "nms:3"]


@functools.lru_cache(maxsize=None)
def _head_case():
    enc, a, inv, sc = _decode_case(True, HEAD["B"], HEAD["N"], HEAD["C"] + 1, seed=41)
    boxes = _decode32(enc, a, inv)[:, :, None]
    assert np.array_equal(boxes, torch.from_numpy(boxes).to(BF).float().numpy())    # exact in bf16 too
    want = _mirror(boxes, sc[..., 1:], HEAD["mpc"], HEAD["T"], IOU_THR, SCORE_THR, clip=False)
    assert (want[3] == HEAD["T"]).all()
    return enc, a, inv, sc, boxes, want


def _head_feeds(dev="cpu"):
    enc, _, _, sc, _, _ = _head_case()
    return {"encodings:0": torch.from_numpy(enc).float().to(dev), "scores:0": torch.from_numpy(sc).float().to(dev)}


def _head_spec():
    return {"encodings:0": ((HEAD["B"], HEAD["N"], 4), "FLOAT"), "scores:0": ((HEAD["B"], HEAD["N"], HEAD["C"] + 1), "FLOAT")}


def _check_head_lowering(dev):
    _, a, inv, _, boxes, want = _head_case()
    g = _head_graph(anchors=a, inv=inv)
    _same(Session(g).run(NMS_OUT, _head_feeds()), want)               # the interpreter, decode op by op
    plan = CompiledFunction(g, _head_spec(), NMS_OUT, dev, strict=True)
    assert [s.kind for s in plan.steps] == ["nms"] and plan.summary()["kinds"] == {"nms": 1}
    assert plan.steps[0].meta["fused_decode"] and plan.steps[0].meta["class_offset"] == 1
    assert plan.steps[0].meta["pitch"] == HEAD["C"] + 1
    _same(plan(_head_feeds(dev)), want)
    # the boxes fetched as well: decode op by op (Exp and the [N, 2] broadcasts are glue), NMS on decoded boxes
    with pytest.raises(CompileError):
        CompiledFunction(g, _head_spec(), NMS_OUT + ["decode/boxes:0"], dev, strict=True)
    plan = CompiledFunction(g, _head_spec(), NMS_OUT + ["decode/boxes:0"], dev, strict=False)
    nms = [s for s in plan.steps if s.kind == "nms"]
    assert len(nms) == 1 and not nms[0].meta["fused_decode"] and "Exp" in plan.summary()["glue_ops"]
    assert "CombinedNonMaxSuppression" not in plan.summary()["glue_ops"]
    outs = plan(_head_feeds(dev))
    _same(outs[:4], want)
    assert torch.equal(outs[4].float().cpu(), torch.from_numpy(boxes).float())


def test_head_lowers_to_one_nms_step():
    _check_head_lowering("cpu")


def test_what_stays_glue():
    _, a, inv, sc, boxes, _ = _head_case()
    B, N, C = HEAD["B"], HEAD["N"], HEAD["C"]
    # per-class boxes
    g = _head_graph(q1=False)
    spec = {"boxes:0": ((B, N, C, 4), "FLOAT"), "scores:0": ((B, N, C + 1), "FLOAT")}
    with pytest.raises(CompileError, match="CombinedNonMaxSuppression"):
        CompiledFunction(g, spec, NMS_OUT, "cpu", strict=True)
    plan = CompiledFunction(g, spec, NMS_OUT, "cpu", strict=False)
    assert plan.summary()["glue_ops"] == ["CombinedNonMaxSuppression"] and "nms" not in plan.summary()["kinds"]
    rng = np.random.default_rng(9)
    pc = _grid_boxes(rng, B, N, C, lo=0, hi=64)
    feeds = {"boxes:0": torch.from_numpy(pc).float(), "scores:0": torch.from_numpy(sc).float()}
    _same(plan(feeds)[:4], _mirror(pc, sc[..., 1:], HEAD["mpc"], HEAD["T"], IOU_THR, SCORE_THR, clip=False))
    # a fed max_total_size
    g = _head_graph(anchors=a, inv=inv, fed_total=True)
    with pytest.raises(CompileError, match="CombinedNonMaxSuppression"):
        CompiledFunction(g, {**_head_spec(), "total:0": ((), "INT32")}, NMS_OUT, "cpu", strict=True)
    # N one past the limit: the decode is materialised for the glue op
    n = K.NMS_MAX_BOXES + 1
    enc, a2, inv2, sc2 = _decode_case(True, 1, n, 2, seed=43)
    g = _head_graph(N=n, C=1, B=1, mpc=3, T=5, anchors=a2, inv=inv2)
    spec = {"encodings:0": ((1, n, 4), "FLOAT"), "scores:0": ((1, n, 2), "FLOAT")}
    with pytest.raises(CompileError, match="CombinedNonMaxSuppression"):
        CompiledFunction(g, spec, NMS_OUT, "cpu", strict=True)
    plan = CompiledFunction(g, spec, NMS_OUT, "cpu", strict=False)
    assert plan.summary()["glue_ops"] == ["CombinedNonMaxSuppression"]
    want = _mirror(_decode32(enc, a2, inv2)[:, :, None], sc2[..., 1:], 3, 5, IOU_THR, SCORE_THR, clip=False)
    _same(plan({"encodings:0": torch.from_numpy(enc).float(), "scores:0": torch.from_numpy(sc2).float()}), want)


def test_unpadded_nms_is_refused_by_every_plan():
    g = _single_graph("NonMaxSuppressionV3", 16, 4, 0.5, 0.0)
    spec = {"boxes:0": ((16, 4), "FLOAT"), "scores:0": ((16,), "FLOAT")}
    for strict in (True, False):
        with pytest.raises(CompileError, match="data-dependent"):
            CompiledFunction(g, spec, ["nms:0"], "cpu", strict=strict)
    g = _single_graph("NonMaxSuppressionV4", 16, 4, 0.5, 0.0, pad_to_max_output_size=True)
    plan = CompiledFunction(g, spec, ["nms:0", "nms:1"], "cpu", strict=False)       # a static shape: glue
    assert plan.summary()["glue_ops"] == ["NonMaxSuppressionV4"]


def _reshape_graph():
    """stem -> conv(8 -> 12 channels: stored 16 wide) + BiasAdd -> Reshape [B, 8 * 8 * 3, 4]: an SSD box head."""
    gb = GraphBuilder()
    images = gb.placeholder("images", "UINT8", [None, 16, 16, 3])
    x = gb.cast(images, "FLOAT", name="Cast")
    x = gb.sub(x, gb.constant("mean", np.asarray([120.0, 115.0, 100.0], dtype=np.float32)), name="Sub")
    x = gb.div(x, gb.constant("std", np.asarray([58.0, 57.0, 57.5], dtype=np.float32)), name="normalized")
    rng = np.random.default_rng(7)

    def w(k, cin, cout):
        return (rng.standard_normal((k, k, cin, cout)) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32)

    x = gb.relu(gb.conv2d(x, gb.constant("stem/w", w(3, 3, 8)), (2, 2), name="stem"), name="stem_relu")
    y = gb.bias_add(gb.conv2d(x, gb.constant("head/w", w(1, 8, 12)), name="head"),
                    gb.constant("head/b", rng.standard_normal(12).astype(np.float32)), name="head_bias")
    gb.reshape(y, [-1, 8 * 8 * 3, 4], name="encodings")
    return gb.build()


def _imgs(n, hw, seed):
    return torch.randint(0, 256, (n, hw, hw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _check_reshape_lowering(dev):
    g, imgs = _reshape_graph(), _imgs(2, 16, 3)
    plan = CompiledFunction(g, {"images:0": ((2, 16, 16, 3), "UINT8")}, ["encodings:0"], dev, strict=True)
    head = [s for s in plan.steps if s.name == "head"][0]
    assert head.outputs[0].phys_c == 16 and [s.kind for s in plan.steps if s.name == "encodings"] == ["copy"]
    got = plan({"images:0": imgs.to(dev)})[0].float().cpu()
    ref = Session(g).run(["encodings:0"], {"images:0": imgs})[0]
    assert got.shape == ref.shape == (2, 192, 4)
    assert (got - ref).abs().max() / ref.abs().max() < 0.05


def test_reshape_of_a_padded_conv_output_compiles_strict():
    _check_reshape_lowering("cpu")


# =================================================================================== SSD-MobileNet-V1
SSD = dict(alpha=0.25, image_hw=(96, 96), num_classes=5)
SSD_FETCH = ["detection_boxes:0", "detection_scores:0", "detection_classes:0", "num_detections:0", "box_encodings:0",
             "class_scores:0"]


@pytest.fixture(scope="module")
def ssd():
    """The graph, two images and the fp32 interpreter's fetches: once."""
    from flink_tensorflow_amd.models.zoo import ssd_mobilenet_v1_graph_def

    g = Graph.from_graph_def(ssd_mobilenet_v1_graph_def(**SSD))
    imgs = _imgs(2, 96, seed=13)
    return g, imgs, Session(g).run(SSD_FETCH, {"images:0": imgs})


def _ssd_postprocess_reference(enc, sc):
    """The detections the plan must produce given the heads it computed: the mirror on them
    (it asserts its margins), checked against the interpreter's decode + NMS ops on the same."""
    from flink_tensorflow_amd.models.zoo.ssd import BOX_CODER_SCALES, ssd_anchors, ssd_feature_grids

    a, _ = ssd_anchors(ssd_feature_grids(SSD["image_hw"]))
    inv = (np.float32(1) / np.asarray(BOX_CODER_SCALES, dtype=np.float32)).astype(np.float64)
    enc, sc = enc.double().numpy(), sc.double().numpy()
    want = _mirror(_decode32(enc, a, inv)[:, :, None], sc, 100, 100, 0.6, 1e-8)
    B, N, C = sc.shape
    gb = GraphBuilder()
    boxes = gb.decode_boxes(gb.placeholder("enc", "FLOAT", [B, N, 4]), a, BOX_CODER_SCALES)
    gb.combined_nms(boxes, gb.placeholder("sc", "FLOAT", [B, N, C]), 100, 100, 0.6, 1e-8, name="nms")
    tol = _decode_tol(enc, a, inv, want[4])
    _same(Session(gb.build()).run(NMS_OUT, {"enc:0": torch.from_numpy(enc).float(), "sc:0": torch.from_numpy(sc).float()}),
          want, boxes_exact=False, tol=tol)
    return want, tol


def _check_ssd_plan(plan, imgs, ref, dev):
    s = plan.summary()
    assert s["glue_ops"] == [] and "glue" not in s["kinds"]
    assert s["kinds"]["dwconv"] == 13 and s["kinds"]["nms"] == 1
    nms = [st for st in plan.steps if st.kind == "nms"][0]
    assert nms.meta["fused_decode"]
    outs = plan({"images:0": imgs.to(dev)})
    enc, sc = outs[4].float().cpu(), outs[5].float().cpu()
    N = ref[4].shape[1]
    assert enc.shape == ref[4].shape == (2, N, 4) and sc.shape == ref[5].shape == (2, N, 5) and 100 < N < 1000
    for got, want in ((enc, ref[4]), (sc, ref[5])):
        assert (got - want).abs().max() / want.abs().max() < 0.05
    want, tol = _ssd_postprocess_reference(enc, sc)
    assert want[3].min() > 10
    _same(outs[:4], want, boxes_exact=False, tol=tol)
    return outs


def test_ssd_plan_host(ssd):
    g, imgs, ref = ssd
    assert ref[0].shape == (2, 100, 4) and ref[3].dtype == torch.int32 and len(torch.unique(ref[2])) > 1
    plan = CompiledFunction(g, {"images:0": ((2, 96, 96, 3), "UINT8")}, SSD_FETCH, "cpu", strict=True)
    _check_ssd_plan(plan, imgs, ref, "cpu")
    # without the heads fetched the score slice is absorbed: no copy step for it
    plan = CompiledFunction(g, {"images:0": ((2, 96, 96, 3), "UINT8")}, SSD_FETCH[:4], "cpu", strict=True)
    assert "class_scores" not in [st.name for st in plan.steps]
    assert [st for st in plan.steps if st.kind == "nms"][0].meta["class_offset"] == 1


def test_ssd_model_rejects_buckets_that_cannot_compile():
    from flink_tensorflow_amd.models.zoo import SSDMobileNetModel
    from flink_tensorflow_amd.models.zoo.ssd import ssd_batch_ok

    assert ssd_batch_ok(8, (300, 300), 90) and not ssd_batch_ok(4, (300, 300), 90) and ssd_batch_ok(1, (96, 96), 5)
    with pytest.raises(ValueError, match="multiple of 8"):
        SSDMobileNetModel(buckets=(2, 8), device="cpu")          # 2 * 1917 * 91 is no multiple of 8
    SSDMobileNetModel(buckets=(8, 32), device="cpu")


def _as_lists(boxes, scores, classes, valid):
    return [[(float(scores[b, i]), f"class_{int(classes[b, i])}", tuple(float(v) for v in boxes[b, i]))
             for i in range(int(valid[b]))] for b in range(len(valid))]


def test_ssd_model_detects_on_the_host(ssd):
    from flink_tensorflow_amd.models.zoo import SSDMobileNetModel

    _, imgs, ref = ssd
    m = SSDMobileNetModel(buckets=(2,), device="cpu", **SSD)
    m.open()
    try:
        dets = m.detect(list(imgs.numpy()))
        (res, tags, _), = m.submit(list(imgs.numpy()), np.zeros(2), [5, 6])
    finally:
        m.close()
    assert dets == _as_lists(*ref[:4]) and res == dets and tags == [5, 6]      # host: the interpreter
    assert all(0 < len(d) <= 100 for d in dets)
    for d in dets:
        assert [s for s, _, _ in d] == sorted((s for s, _, _ in d), reverse=True)
        assert all(lab in {f"class_{c}" for c in range(5)} and len(box) == 4 for _, lab, box in d)


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
    if isinstance(fill, float) and fill != fill:
        return bool(torch.isnan(lo).all() and torch.isnan(hi).all())
    return bool((lo == fill).all() and (hi == fill).all())


def _gpu_nms(boxes, scores, mpc, T, iou, thr, pad, clip, dev, C=None, off=0, anchors=None, scales=None):
    """The kernel between guard bands: NaN around every operand, sentinels around every output
    and the scratch; twice, and both runs must agree bit for bit."""
    nan = float("nan")
    ops = [_banded(boxes, nan, dev), _banded(scores, nan, dev)]
    av = None
    if anchors is not None:
        ops.append(_banded(anchors, nan, dev))
        av = ops[2][0]
    B, N, ld = scores.shape
    C = ld - off if C is None else C
    Tout = min(T, mpc * C) if pad else T
    runs = []
    for _ in range(2):
        outs = [_banded(torch.full(s, SENT if d == torch.float32 else -7, dtype=d), SENT if d == torch.float32 else -7, dev)
                for s, d in (((B, Tout, 4), torch.float32), ((B, Tout), torch.float32), ((B, Tout), torch.float32),
                             ((B,), torch.int32))]
        scr = _banded(torch.full((K.nms_scratch_numel(B, C, min(mpc, N)),), -7, dtype=torch.int64), -7, dev)
        got = K.combined_nms(ops[0][0], ops[1][0], mpc, T, iou, thr, pad, clip, anchors=av, box_scales=scales,
                             num_classes=C, class_offset=off, out=tuple(o[0] for o in outs), scratch=scr[0])
        torch.cuda.synchronize()
        assert all(g is o[0] for g, o in zip(got, outs))
        for v, buf in outs + [scr]:
            assert _bands_intact(buf, v.numel(), SENT if v.dtype == torch.float32 else -7), "stray store"
        runs.append([v.cpu() for v, _ in outs])
    for (v, buf), src in zip(ops, (boxes, scores, anchors)):
        assert _bands_intact(buf, v.numel(), nan) and torch.equal(v.cpu().view(torch.uint8), src.contiguous().view(torch.uint8))
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*runs)), "two runs differ"
    return runs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EXACT))
def test_kernel_bit_exact(name):
    B, C, N, mpc, T, pad, clip, dt = EXACT[name]
    bx, sc, want = _exact_case(name)
    dev = torch.device("cuda", 0)
    boxes = torch.from_numpy(bx).to(BF if dt == "bf16" else torch.float32)
    _same(_gpu_nms(boxes, torch.from_numpy(sc).to(BF), mpc, T, IOU_THR, SCORE_THR, pad, clip, dev), want)


@pytest.mark.gpu
def test_kernel_pitch_offset_fp32_scores_and_equality():
    dev = torch.device("cuda", 0)
    # a padded scores row: +2^100 in the background column and in the padding; neither may compete
    bx, sc, want = _exact_case("b3-c3-n63")
    wide = torch.from_numpy(_pitched_scores(sc, 8, 1, SENT))
    for dt in (BF, torch.float32):
        _same(_gpu_nms(torch.from_numpy(bx).float(), wide.to(dt), 5, 100, IOU_THR, SCORE_THR, False, True, dev, C=3, off=1),
              want)
    # IoU exactly at the threshold does not suppress; a threshold 2^-13 lower does
    bx, sc = _equality_case()
    below = 0.5 - 2.0 ** -13
    for thr, kw in ((0.5, dict(equal_ok=True)), (below, {})):
        want = _mirror(bx, sc, 3, 3, thr, 0.0, **kw)
        for dt in (BF, torch.float32):
            _same(_gpu_nms(torch.from_numpy(bx).to(dt), torch.from_numpy(sc).to(BF), 3, 3, thr, 0.0, False, True, dev), want)
    # nothing passes the score threshold
    bx, sc, _ = _exact_case("b1-c3-n300")
    want = _mirror(bx, sc, 5, 10, IOU_THR, 1.5)
    _same(_gpu_nms(torch.from_numpy(bx).float(), torch.from_numpy(sc).to(BF), 5, 10, IOU_THR, 1.5, False, True, dev), want)


@pytest.mark.gpu
def test_kernel_merge_of_many_kept_keys():
    """T = 1000 of about 9000 kept keys (C * max_per_class = 90 * 100): classes win more rounds of the
    merge than their staged window of 16 keys holds."""
    rng = np.random.default_rng(77)
    bx, sc = _grid_boxes(rng, 1, 1917, lo=-64, hi=190, smax=3), _grid_scores(rng, 1, 1917, 90)
    want = _mirror(bx, sc, 100, 1000, IOU_THR, SCORE_THR)
    assert want[3].tolist() == [1000]
    dev = torch.device("cuda", 0)
    _same(_gpu_nms(torch.from_numpy(bx).to(BF), torch.from_numpy(sc).to(BF), 100, 1000, IOU_THR, SCORE_THR, False, True, dev),
          want)


@pytest.mark.gpu
def test_kernel_at_the_envelope_corners():
    """C, max_per_class and T at the launcher's limits: one class per merge thread, 256 kept boxes in
    LDS, 1024 merge rounds.  (N at its limit is in ``EXACT``.)"""
    dev = torch.device("cuda", 0)
    C, mpc, T = K.NMS_MAX_CLASSES, K.NMS_MAX_PER_CLASS, K.NMS_MAX_TOTAL
    rng = np.random.default_rng(55)
    bx, sc = _grid_boxes(rng, 1, 300), _grid_scores(rng, 1, 300, C)
    want = _mirror(bx, sc, mpc, T, IOU_THR, 0.9)               # about 30 candidates a class
    assert want[3].tolist() == [T] and len(set(want[2][0].tolist())) > 200
    _same(_gpu_nms(torch.from_numpy(bx).to(BF), torch.from_numpy(sc).to(BF), mpc, T, IOU_THR, 0.9, False, True, dev), want)
    bx, sc = _grid_boxes(rng, 1, 4096, lo=-120, hi=120, smax=4), _grid_scores(rng, 1, 4096, 1)
    want = _mirror(bx, sc, mpc, T, IOU_THR, SCORE_THR)         # one class keeps all 256
    assert want[3].tolist() == [mpc]
    _same(_gpu_nms(torch.from_numpy(bx).float(), torch.from_numpy(sc).to(BF), mpc, T, IOU_THR, SCORE_THR, False, True, dev),
          want)


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False], ids=["dyadic", "normal"])
@pytest.mark.parametrize("enc_dtype", [BF, torch.float32], ids=["bf16", "f32"])
def test_kernel_fused_decode(exact, enc_dtype):
    enc, a, inv, sc = _decode_case(exact)
    want = _mirror(_decode32(enc, a, inv)[:, :, None], sc, 20, 50, IOU_THR, SCORE_THR, clip=False)
    dev = torch.device("cuda", 0)
    got = _gpu_nms(torch.from_numpy(enc).to(enc_dtype), torch.from_numpy(sc).to(BF), 20, 50, IOU_THR, SCORE_THR, False, False,
                   dev, anchors=torch.from_numpy(a).float(), scales=inv.tolist())
    _same(got, want, boxes_exact=exact, tol=_decode_tol(enc, a, inv, want[4]))


@pytest.mark.gpu
def test_one_step_past_each_limit_raises_on_the_host():
    dev = torch.device("cuda", 0)
    for call in _past_the_limits(dev):
        with pytest.raises(ValueError, match="envelope"):
            call()
    bx = torch.zeros((1, 8, 1, 4), dtype=torch.float32, device=dev)
    with pytest.raises(TypeError):
        K.combined_nms(bx, torch.zeros((1, 8, 2), dtype=torch.float16, device=dev), 4, 4, 0.5, 0.0)
    with pytest.raises(ValueError, match="scratch"):
        K.combined_nms(bx, torch.zeros((1, 8, 2), dtype=BF, device=dev), 4, 4, 0.5, 0.0,
                       scratch=torch.zeros(3, dtype=torch.int64, device=dev))


# =================================================================================== GPU: the plans
@pytest.mark.gpu
def test_head_lowering_gpu():
    _check_head_lowering(torch.device("cuda", 0))


@pytest.mark.gpu
def test_glue_forms_are_refused_by_gpu_plans():
    """The forms that stay glue in a host plan run the interpreter's host routine, which a GPU
    plan cannot capture (and should not run per batch): on a GPU they raise ``CompileError`` in
    non-strict mode too, which is what ``ModelFunction`` catches to fall back to the interpreter."""
    dev = torch.device("cuda", 0)
    _, a, inv, _, _, _ = _head_case()
    B, N, C = HEAD["B"], HEAD["N"], HEAD["C"]
    n = K.NMS_MAX_BOXES + 1
    _, a2, inv2, _ = _decode_case(True, 1, n, 2, seed=43)
    single = {"boxes:0": ((16, 4), "FLOAT"), "scores:0": ((16,), "FLOAT")}
    cases = {
        "q=C": (_head_graph(q1=False), {"boxes:0": ((B, N, C, 4), "FLOAT"), "scores:0": ((B, N, C + 1), "FLOAT")}, NMS_OUT),
        "fed total": (_head_graph(anchors=a, inv=inv, fed_total=True), {**_head_spec(), "total:0": ((), "INT32")}, NMS_OUT),
        "N over": (_head_graph(N=n, C=1, B=1, mpc=3, T=5, anchors=a2, inv=inv2),
                   {"encodings:0": ((1, n, 4), "FLOAT"), "scores:0": ((1, n, 2), "FLOAT")}, NMS_OUT),
        "padded V4": (_single_graph("NonMaxSuppressionV4", 16, 4, 0.5, 0.0, pad_to_max_output_size=True), single,
                      ["nms:0", "nms:1"]),
        "padded V5": (_single_graph("NonMaxSuppressionV5", 16, 4, 0.5, 0.0, 0.0, pad_to_max_output_size=True), single,
                      ["nms:0", "nms:1", "nms:2"]),
        "unpadded V3": (_single_graph("NonMaxSuppressionV3", 16, 4, 0.5, 0.0), single, ["nms:0"]),
    }
    for name, (g, spec, fetches) in cases.items():
        for strict in (True, False):
            with pytest.raises(CompileError):
                CompiledFunction(g, spec, fetches, dev, strict=strict)
                pytest.fail(f"{name} (strict={strict}) compiled on the GPU")


@pytest.mark.gpu
def test_kernel_takes_more_images_than_a_grid_axis():
    """B = 65536 images of one box and one class: (image, class) pairs ride on grid.x."""
    dev = torch.device("cuda", 0)
    B = 65536
    rng = np.random.default_rng(5)
    sc = torch.from_numpy(rng.integers(0, 256, (B, 1, 1)) / 256.0)
    bx = torch.from_numpy(rng.integers(0, 64, (B, 1, 1, 4)) / 64.0)
    got = [t.cpu() for t in K.combined_nms(bx.float().to(dev), sc.to(BF).to(dev), 1, 1, IOU_THR, SCORE_THR)]
    keep = sc[:, 0, 0] > SCORE_THR
    assert torch.equal(got[3], keep.to(torch.int32)) and not got[2].any()
    assert torch.equal(got[1][:, 0], torch.where(keep, sc[:, 0, 0], 0.0).float())
    assert torch.equal(got[0][:, 0], torch.where(keep[:, None], bx[:, 0, 0], 0.0).float())


@pytest.mark.gpu
def test_reshape_of_a_padded_conv_output_gpu():
    _check_reshape_lowering(torch.device("cuda", 0))


@pytest.mark.gpu
def test_ssd_plan_and_model_gpu(ssd):
    from flink_tensorflow_amd.models.zoo import SSDMobileNetModel

    g, imgs, ref = ssd
    dev = torch.device("cuda", 0)
    plan = CompiledFunction(g, {"images:0": ((2, 96, 96, 3), "UINT8")}, SSD_FETCH, dev, strict=True)
    assert plan.summary()["hip_graph"]
    outs = _check_ssd_plan(plan, imgs, ref, dev)
    again = plan({"images:0": imgs.to(dev)})
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(again, outs))      # a second replay is bit-identical
    m = SSDMobileNetModel(buckets=(2,), lanes=1, **SSD)
    m.open()
    try:
        s = m.plan_summary()
        assert s["glue_ops"] == [] and s["kinds"]["nms"] == 1 and s["kinds"]["dwconv"] == 13
        dets = m.detect(list(imgs.numpy()))
        done = m.submit(list(imgs.numpy()), np.zeros(2), [0, 1])   # the same batch: the same bits
        done += m.drain()
    finally:
        m.close()
    assert dets == _as_lists(*(o.cpu() for o in outs[:4]))
    assert [t for _, tags, _ in done for t in tags] == [0, 1]
    assert [r for res, _, _ in done for r in res] == dets
