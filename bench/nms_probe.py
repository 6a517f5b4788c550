"""Box decode + NMS (``kernels/detection.hip``) on the head of an SSD-MobileNet-V1 at B=32,
N=1917, C=90, T=100, the whole SSD plan, and what serving an SSD took before the kernel existed.

Candidates are alternated round by round in one process (device events around ``--reps``
launches, ``--rounds`` rounds after a warm-up of every candidate; the median and the min..max
spread of the rounds are printed).

``step``: the ``nms`` step, both launches (``nms_per_class`` + ``nms_merge``), on scores
``sigmoid(4 * normal)`` in rows of 91 with the background column skipped in place, encodings
``normal`` in bf16 and the SSD anchor table:

* ``fused``         bf16 encodings decoded inside the kernel;
* ``decoded:f32``   fp32 corner boxes decoded beforehand (decode not timed);
* ``decoded:bf16``  the same boxes rounded to bf16;
* ``fused:thr0.3``  ``fused`` with ``score_threshold`` 0.3 instead of the SSD default 1e-8: fewer
  candidates to sort past and walk.

``--plan``: the hipGraph replay of the strict SSD plan, the device time of every step of one
eager run (``plan.profile()``) summed by kind, and the share of the ``nms`` step in it.

``--host``: today's alternative for the same batch: the plan that fetches ``box_encodings`` and
``class_scores`` instead, their device-to-host copy, and the host routine of ``K.combined_nms``
(fp32 decode + numpy NMS, per image and class in Python) on them; host clock, ``--host-rounds``
times.

    python bench/nms_probe.py --reps 1000 --rounds 7 --plan --host
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from flink_tensorflow_amd.graph.ops_nn import decode_boxes_yxhw  # noqa: E402
from flink_tensorflow_amd.ops import kernels as K  # noqa: E402

BF = torch.bfloat16


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def alternate(fns, reps, rounds):
    for fn in fns.values():  # warm up every candidate
        fn()
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, reps))
    return t


def line(shape, name, ts, **extra):
    med = statistics.median(ts)
    print(json.dumps({"shape": shape, "impl": name, "us": round(med, 1), "min": round(min(ts), 1),
                      "max": round(max(ts), 1), **extra}), flush=True)


def step(B, N_hw, C, mpc, T, iou, dev, reps, rounds):
    from flink_tensorflow_amd.models.zoo.ssd import BOX_CODER_SCALES, ssd_anchors, ssd_feature_grids

    anchors = torch.from_numpy(ssd_anchors(ssd_feature_grids(N_hw))[0]).to(dev)
    N = anchors.shape[0]
    g = torch.Generator(device=dev).manual_seed(0)
    enc = torch.randn((B, N, 4), device=dev, generator=g).to(BF)
    scores = torch.sigmoid(4 * torch.randn((B, N, C + 1), device=dev, generator=g)).to(BF)
    inv = [float(np.float32(1) / np.float32(s)) for s in BOX_CODER_SCALES]
    boxes32 = decode_boxes_yxhw(enc, anchors, torch.tensor(inv, device=dev)).contiguous()
    boxes16 = boxes32.to(BF)
    outs = {k: (torch.empty((B, T, 4), dtype=torch.float32, device=dev), torch.empty((B, T), dtype=torch.float32, device=dev),
                torch.empty((B, T), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
            for k in ("fused", "decoded:f32", "decoded:bf16", "fused:thr0.3")}
    scratch = torch.empty(K.nms_scratch_numel(B, C, mpc), dtype=torch.int64, device=dev)

    def run(key, bx, thr=1e-8, **kw):
        return lambda: K.combined_nms(bx, scores, mpc, T, iou, thr, num_classes=C, class_offset=1, out=outs[key],
                                      scratch=scratch, **kw)

    fns = {"fused": run("fused", enc, anchors=anchors, box_scales=inv), "decoded:f32": run("decoded:f32", boxes32),
           "decoded:bf16": run("decoded:bf16", boxes16),
           "fused:thr0.3": run("fused:thr0.3", enc, 0.3, anchors=anchors, box_scales=inv)}
    t = alternate(fns, reps, rounds)
    shape = f"nms_b{B}_n{N}_c{C}_k{mpc}_t{T}"
    for k, ts in t.items():
        line(shape, k, ts, valid_mean=round(float(outs[k][3].float().mean()), 1))
    same = all(torch.equal(a, b) for a, b in zip(outs["fused"][1:], outs["decoded:f32"][1:]))
    dbox = float((outs["fused"][0] - outs["decoded:f32"][0]).abs().max())
    print(json.dumps({"shape": shape, "fused_equals_decoded_f32": same, "max_abs_box_diff": dbox,
                      "candidates_per_class": round(float((scores[..., 1:].float() > 1e-8).sum() / (B * C)), 1),
                      "candidates_per_class_thr0.3": round(float((scores[..., 1:].float() > 0.3).sum() / (B * C)), 1)}),
          flush=True)


def plans(B, hw, C, alpha, dev, reps, rounds, host, host_rounds):
    from flink_tensorflow_amd.graph.compiler import CompiledFunction
    from flink_tensorflow_amd.graph.graph import Graph
    from flink_tensorflow_amd.models.zoo.ssd import ssd_mobilenet_v1_graph_def

    g = Graph.from_graph_def(ssd_mobilenet_v1_graph_def(num_classes=C, image_hw=hw, alpha=alpha))
    feeds = {"images:0": ((B, hw[0], hw[1], 3), "UINT8")}
    imgs = torch.randint(0, 256, (B, hw[0], hw[1], 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    det = ["detection_boxes:0", "detection_scores:0", "detection_classes:0", "num_detections:0"]
    strict = CompiledFunction(g, feeds, det, dev, strict=True)
    strict.input_buffer("images:0").copy_(imgs)
    assert strict.summary()["hip_graph"]
    name = f"ssd_mobilenet_v1_{alpha}_{hw[0]}_c{C}_b{B}"
    print(json.dumps({"plan": name, "hip_graph": True, "kinds": strict.summary()["kinds"]}), flush=True)
    fns = {"detections": strict.replay}
    heads = None
    if host:
        heads = CompiledFunction(g, feeds, ["box_encodings:0", "class_scores:0"], dev, strict=True)
        heads.input_buffer("images:0").copy_(imgs)
        fns["heads_only"] = heads.replay
    t = alternate(fns, reps, rounds)
    for k, ts in t.items():
        line(name, "replay:" + k, ts)
    by_kind: dict = {}
    for _ in range(3):  # the third eager run: every launch warm
        md = strict.profile()
    for ns in md.step_stats.dev_stats[0].node_stats:
        by_kind[ns.timeline_label] = by_kind.get(ns.timeline_label, 0) + ns.op_end_rel_micros
    total = sum(by_kind.values())
    print(json.dumps({"plan": name, "profile_us_by_kind": by_kind, "profile_total_us": total,
                      "nms_share": round(by_kind.get("nms", 0) / max(total, 1), 4)}), flush=True)
    if not host:
        return
    from flink_tensorflow_amd.models.zoo.ssd import BOX_CODER_SCALES, ssd_anchors, ssd_feature_grids

    anchors = torch.from_numpy(ssd_anchors(ssd_feature_grids(hw))[0])
    inv = [float(np.float32(1) / np.float32(s)) for s in BOX_CODER_SCALES]
    strict.replay()
    torch.cuda.synchronize()
    want = [o.cpu() for o in strict.output_tensors()]
    d2h, post = [], []
    for _ in range(host_rounds):
        heads.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc, sc = (o.cpu() for o in heads.output_tensors())
        t1 = time.perf_counter()
        got = K.combined_nms(enc, sc, 100, 100, 0.6, 1e-8, anchors=anchors, box_scales=inv)
        t2 = time.perf_counter()
        d2h.append((t1 - t0) * 1e6)
        post.append((t2 - t1) * 1e6)
    line(name, "host:d2h_heads", d2h, bytes=enc.numel() * enc.element_size() + sc.numel() * sc.element_size())
    line(name, "host:decode+nms", post)
    print(json.dumps({"plan": name, "host_equals_device": {
        "valid": torch.equal(got[3], want[3]), "classes": torch.equal(got[2], want[2]), "scores": torch.equal(got[1], want[1]),
        "max_abs_box_diff": float((got[0] - want[0]).abs().max())}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000, help="launches per timed window (0.3 s for the step)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--classes", type=int, default=90)
    ap.add_argument("--size", type=int, default=300)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--plan", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-rounds", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nms_probe measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    hw = (a.size, a.size)
    if not a.no_step:
        step(a.batch, hw, a.classes, 100, 100, 0.6, dev, a.reps, a.rounds)
    if a.plan or a.host:
        plans(a.batch, hw, a.classes, a.alpha, dev, a.reps, a.rounds, a.host, a.host_rounds)


if __name__ == "__main__":
    main()
