"""Bilinear resize and fused resize + ArgMax (``kernels/resize.hip``) against what a plan ran
before they existed, on the shapes of a DeepLab-v3 head at B=32, and the whole DeepLab-v3 plan.

Candidates are alternated round by round in one process (device events around ``--reps``
launches, ``--rounds`` rounds after a warm-up of every candidate; the median and the min..max
spread of the rounds are printed).

``head``: logits 33x33x21 in rows of 24 -> a 513x513 uint8 label map, ``align_corners``:

* ``fused``           ``K.resize_argmax_nhwc``, the launcher's choice (the LDS-staged kernel);
  ``fused:simple``    the same with the global-memory kernel pinned;
* ``resize+argmax``   ``K.resize_bilinear_nhwc`` of the padded 24 channels, then
                      ``K.resize_argmax_nhwc`` with identity geometry: what the plan runs when the
                      upsampled logits are fetched;
* ``glue``            the steps a plan without the lowerings runs: the interpreter's
                      ``ResizeBilinear``, ``ArgMax`` and ``Cast`` as captured glue ops (fp32 torch
                      ops on the bf16 buffer, each result copied into its plan buffer).

``aspp_bcast``: the image-pooling broadcast 1x1x256 -> 33x33 into a 1280-channel concat row;
``up2x``: 65x65x256 -> 129x129.  Both ``resize`` against the interpreter's op as glue.

``gbps`` is the ideal traffic (input + output, from the shapes; for ``resize+argmax`` the
upsampled tensor written and read once more) over the time; ``roof`` its share of the 6.29 TB/s
copy rate measured on the MI355X.

``--plan`` times the hipGraph replay of the strict DeepLab-v3 plan against a non-strict plan in
which ``ResizeBilinear``, ``ArgMax`` and convs whose output channels are no multiple of 8 are
forced to glue by a monkey-patch local to this script (the plan before these lowerings).  That
plan cannot be captured: the interpreter's ``ResizeBilinear`` reads its size operand on the
host, which a stream capture refuses.  It is compiled with ``use_graph=False`` and its eager
replay is timed, launch overhead included, as a user of that plan would run it.

    python bench/resize_probe.py --reps 10 --rounds 7 --plan
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from flink_tensorflow_amd.graph.ops_nn import resize_bilinear_tf  # noqa: E402
from flink_tensorflow_amd.ops import kernels as K  # noqa: E402

COPY_ROOF = 6.29e12  # B/s, MI355X_MICROARCH measured copy rate
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


def line(shape, name, ts, nbytes=None):
    med = statistics.median(ts)
    rec = {"shape": shape, "impl": name, "us": round(med, 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}
    if nbytes is not None:
        rec["gbps"] = round(nbytes / med / 1e3, 1)
        rec["roof"] = round(nbytes / (med * 1e-6) / COPY_ROOF, 4)
    print(json.dumps(rec), flush=True)


def head(B, dev, g, reps, rounds, hw=33, out=513, C=21):
    pitch = -(-C // 8) * 8
    x = torch.zeros((B, hw, hw, pitch), dtype=BF, device=dev)
    x[..., :C] = (torch.randn((B, hw, hw, C), device=dev, generator=g) * 4).to(BF)
    lab, lab2, lab_g = (torch.empty((B, out, out), dtype=torch.uint8, device=dev) for _ in range(3))
    up = torch.empty((B, out, out, pitch), dtype=BF, device=dev)
    up_g = torch.empty((B, out, out, C), dtype=BF, device=dev)
    idx_g = torch.empty((B, out, out), dtype=torch.int32, device=dev)

    def fused(path=0):
        K.resize_argmax_nhwc(x, (out, out), True, channels=C, out=lab, path=path)

    def two_step():
        K.resize_bilinear_nhwc(x, (out, out), True, out=up)
        K.resize_argmax_nhwc(up, channels=C, out=lab2)

    def glue():
        up_g.copy_(resize_bilinear_tf(x[..., :C].float(), out, out, True))
        idx_g.copy_(torch.argmax(up_g.float(), dim=3).to(torch.int32))
        lab_g.copy_(idx_g.to(torch.uint8))

    fns = {"fused": fused, "fused:simple": lambda: fused(K.RESIZE_ARGMAX_PATHS["simple"]), "resize+argmax": two_step,
           "glue": glue}
    t = alternate(fns, reps, rounds)
    n_in, n_out, n_up = x.numel() * 2, lab.numel(), up.numel() * 2
    shape = f"head_b{B}_{hw}x{hw}x{C}_to_{out}"
    for k, ts in t.items():
        line(shape, k, ts, {"resize+argmax": n_in + 2 * n_up + n_out, "glue": None}.get(k, n_in + n_out))
    fused()
    two_step()
    glue()
    torch.cuda.synchronize()
    print(json.dumps({"shape": shape, "fused_equals_resize+argmax": round(float((lab == lab2).float().mean()), 6),
                      "fused_equals_glue": round(float((lab == lab_g).float().mean()), 6)}), flush=True)


def resize_case(shape, B, hw, out, C, ldy, dev, g, reps, rounds):
    x = (torch.randn((B, hw, hw, C), device=dev, generator=g) * 4).to(BF)
    y = torch.zeros((B, out, out, ldy), dtype=BF, device=dev)
    y_g = torch.empty((B, out, out, C), dtype=BF, device=dev)

    def resize():
        K.resize_bilinear_nhwc(x, (out, out), True, out=y, out_channel_offset=0)

    def glue():
        y_g.copy_(resize_bilinear_tf(x.float(), out, out, True))

    t = alternate({"resize": resize, "glue": glue}, reps, rounds)
    nbytes = x.numel() * 2 + y_g.numel() * 2
    line(shape, "resize", t["resize"], nbytes)
    line(shape, "glue", t["glue"])
    torch.cuda.synchronize()
    err = (y[..., :C].float() - y_g.float()).abs().max().item()
    print(json.dumps({"shape": shape, "max_abs_diff_vs_glue": round(err, 4)}), flush=True)


def plan_times(B, reps, rounds, dev, alpha, crop):
    from flink_tensorflow_amd.graph.compiler import CompiledFunction
    from flink_tensorflow_amd.graph.graph import Graph
    from flink_tensorflow_amd.models.zoo.deeplab import deeplab_v3_graph_def

    g = Graph.from_graph_def(deeplab_v3_graph_def(alpha=alpha, image_hw=(crop, crop), crop_hw=(crop, crop)))
    feeds = {"images:0": ((B, crop, crop, 3), "UINT8")}
    imgs = torch.randint(0, 256, (B, crop, crop, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    strict = CompiledFunction(g, feeds, ["label_map:0"], dev, strict=True)
    saved = {n: getattr(CompiledFunction, n) for n in ("_lower_resize", "_lower_argmax", "_conv_geometry")}

    def geometry(self, node, x, wv):  # as before the padded-Cout lowering
        if wv.is_const and wv.const.shape[-1] % 8:
            return None
        return saved["_conv_geometry"](self, node, x, wv)

    CompiledFunction._lower_resize = lambda self, node: self._lower_glue(node)   # this script only
    CompiledFunction._lower_argmax = lambda self, node: self._lower_glue(node)
    CompiledFunction._conv_geometry = geometry
    try:
        glue = CompiledFunction(g, feeds, ["label_map:0"], dev, strict=False, use_graph=False)
    finally:
        for n, f in saved.items():
            setattr(CompiledFunction, n, f)
    for p in (strict, glue):
        p.input_buffer("images:0").copy_(imgs)
    assert strict.summary()["hip_graph"]
    print(json.dumps({"plan": "strict", "hip_graph": True, "kinds": strict.summary()["kinds"]}), flush=True)
    print(json.dumps({"plan": "head_as_glue", "hip_graph": False, "kinds": glue.summary()["kinds"],
                      "glue_ops": glue.summary()["glue_ops"]}), flush=True)
    t = alternate({"strict": strict.replay, "head_as_glue": glue.replay}, reps, rounds)
    a, b = strict.output_tensors()[0].cpu(), glue.output_tensors()[0].cpu()
    for k, ts in t.items():
        line(f"deeplab_v3_{alpha}_{crop}_b{B}", k, ts)
    print(json.dumps({"plan": "label_agreement", "frac": round(float((a == b).float().mean()), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="head,aspp_bcast,up2x")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--plan", action="store_true")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--crop", type=int, default=513)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resize_probe measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    for name in [n for n in a.shapes.split(",") if n]:
        if name == "head":
            head(a.batch, dev, g, a.reps, a.rounds)
        elif name == "aspp_bcast":
            resize_case(f"aspp_bcast_b{a.batch}_1x1x256_to_33", a.batch, 1, 33, 256, 1280, dev, g, a.reps, a.rounds)
        elif name == "up2x":
            resize_case(f"up2x_b{a.batch}_65x65x256_to_129", a.batch, 65, 129, 256, 256, dev, g, a.reps, a.rounds)
        else:
            raise SystemExit(f"unknown shape {name!r}")
        torch.cuda.empty_cache()
    if a.plan:
        plan_times(a.batch, a.reps, a.rounds, dev, a.alpha, a.crop)


if __name__ == "__main__":
    main()
