"""Transposed conv (``kernels/deconv.hip``) against what a plan could run before it existed, on
the four distinct up-conv layers of the default U-Net at B=32 (2x2/2), on a 4x4/2 and a 3x3/2
layer of the same sizes, and on the whole U-Net plan.

Per layer, alternated round by round in one process (device events around ``--reps`` launches,
``--rounds`` rounds after a warm-up of every candidate; the median and the min..max spread of
the rounds are printed):

* ``deconv``        the launcher's choice; ``deconv:128x128 / 256x64`` pin a tile;
* ``stuffed``       what the tree could do without the kernel: the input copied at stride ``s``
                    into a buffer zeroed once (the holes stay zero), then ``K.conv2d_nhwc`` with
                    the spatially flipped filter over it: ``s * s`` times the MACs and input
                    traffic, plus the stuffing pass;
* ``torch_bf16``    ``torch.nn.functional.conv_transpose2d`` on bf16 channels-last tensors;
* ``glue``          the interpreter's ``Conv2DBackpropInput`` + ``BiasAdd`` as captured glue ops
                    (fp32 torch ops on the bf16 buffers, the result copied back to bf16).

``ideal_bytes`` is the ideal traffic (input + output + weights + bias, from the shapes), ``gbps`` that over the time,
``roof`` its share of the 6.29 TB/s copy rate measured on the MI355X, ``tflops`` the useful MACs
(``2 * N * Ho * Wo * Cout * Cin * KH * KW / (s * s)``) over the time.

``--plan`` times the hipGraph replay of the strict U-Net plan against a non-strict plan whose
transposed convs are forced to glue by a monkey-patch local to this script.

    python bench/deconv_probe.py --reps 20 --rounds 7 --plan
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from flink_tensorflow_amd.graph.ops_nn import conv2d_transpose_tf, same_pads  # noqa: E402
from flink_tensorflow_amd.ops import kernels as K  # noqa: E402

COPY_ROOF = 6.29e12  # B/s, MI355X_MICROARCH measured copy rate
SIZES = {"16x1024": (16, 1024, 512), "32x512": (32, 512, 256), "64x256": (64, 256, 128), "128x128": (128, 128, 64)}
LAYERS = {f"{k}k{s}": (*v, k) for k in (2, 4, 3) for s, v in SIZES.items()}  # name: (Hi = Wi, Cin, Cout, KH = KW)


def ideal_bytes(B, Hi, Cin, Cout, k):
    return 2 * B * Hi * Hi * Cin + 2 * B * 4 * Hi * Hi * Cout + 2 * k * k * Cin * Cout + 4 * Cout


def useful_flops(B, Hi, Cin, Cout, k):
    return 2 * B * 4 * Hi * Hi * Cout * Cin * k * k / 4


def candidates(B, Hi, Cin, Cout, k, dev, g, which):
    s, Ho = 2, 2 * Hi
    pt = same_pads(Ho, k, s)[0]
    x = torch.randn((B, Hi, Hi, Cin), device=dev, generator=g).to(torch.bfloat16)
    w = torch.randn((k, k, Cout, Cin), device=dev, generator=g) * (2.0 / (Cin * k * k / 4)) ** 0.5
    bias = torch.randn(Cout, device=dev, generator=g) * 0.1
    wp = K.deconv_pack_weights(w, (s, s), (pt, pt)).to(torch.bfloat16)
    y = torch.empty((B, Ho, Ho, Cout), dtype=torch.bfloat16, device=dev)
    y_ref = torch.empty_like(y)
    fns = {}
    for name in which:
        if name.startswith("deconv"):
            cfg = K.DECONV_TILES[name.split(":")[1]] if ":" in name else -1

            def fn(cfg=cfg):
                K.deconv2d_nhwc(x, wp, bias, (Ho, Ho), (k, k), (s, s), (pt, 0, pt, 0), None, out=y, cfg=cfg)
        elif name == "stuffed":
            Hs = (Hi - 1) * s + 1
            stuffed = torch.zeros((B, Hs, Hs, Cin), dtype=torch.bfloat16, device=dev)
            w_ohwi = w.flip(0, 1).permute(2, 0, 1, 3).contiguous().to(torch.bfloat16)
            lo = k - 1 - pt
            pads = (lo, Ho - Hs + k - 1 - lo, lo, Ho - Hs + k - 1 - lo)
            y_s = torch.empty_like(y)

            def fn(stuffed=stuffed, w_ohwi=w_ohwi, pads=pads, y_s=y_s):
                stuffed[:, ::s, ::s].copy_(x)
                K.conv2d_nhwc(x=stuffed, w_ohwi=w_ohwi, bias=bias, stride=(1, 1), pad=pads, out=y_s)
            fns["_stuffed_out"] = y_s
        elif name == "torch_bf16":
            xc = x.permute(0, 3, 1, 2)  # NCHW view of the NHWC buffer (channels-last)
            wt = w.permute(3, 2, 0, 1).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            b16 = bias.to(torch.bfloat16)

            def fn(xc=xc, wt=wt, b16=b16):
                F.conv_transpose2d(xc, wt, b16, stride=(s, s))[:, :, pt:pt + Ho, pt:pt + Ho]
        elif name == "glue":
            def fn():
                t = conv2d_transpose_tf(x.float(), w, (Ho, Ho), (s, s), "SAME")
                y_ref.copy_(t + bias)
        else:
            raise SystemExit(f"unknown candidate {name!r}")
        fns[name] = fn
    return fns, (y, y_ref)


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


def line(layer, name, ts, nbytes=None, flops=None):
    med = statistics.median(ts)
    rec = {"layer": layer, "impl": name, "us": round(med, 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}
    if nbytes is not None:
        rec["ideal_bytes"] = nbytes
        rec["gbps"] = round(nbytes / med / 1e3, 1)
        rec["roof"] = round(nbytes / (med * 1e-6) / COPY_ROOF, 3)
    if flops is not None:
        rec["tflops"] = round(flops / (med * 1e-6) / 1e12, 1)
    print(json.dumps(rec), flush=True)


def plan_times(B, reps, rounds, dev):
    from flink_tensorflow_amd.graph.compiler import CompiledFunction
    from flink_tensorflow_amd.graph.graph import Graph
    from flink_tensorflow_amd.models.zoo.unet import unet_graph_def

    g = Graph.from_graph_def(unet_graph_def(image_hw=(256, 256), crop_hw=(256, 256)))
    feeds = {"images:0": ((B, 256, 256, 3), "UINT8")}
    imgs = torch.randint(0, 256, (B, 256, 256, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    strict = CompiledFunction(g, feeds, ["label_map:0"], dev, strict=True)
    lower = CompiledFunction._lower_deconv
    CompiledFunction._lower_deconv = lambda self, node: self._lower_glue(node, host_consts=(0,))  # this script only
    try:
        glue = CompiledFunction(g, feeds, ["label_map:0"], dev, strict=False)
    finally:
        CompiledFunction._lower_deconv = lower
    for p in (strict, glue):
        p.input_buffer("images:0").copy_(imgs)
        assert p.summary()["hip_graph"]
    print(json.dumps({"plan": "strict", "kinds": strict.summary()["kinds"]}), flush=True)
    print(json.dumps({"plan": "deconv_as_glue", "kinds": glue.summary()["kinds"], "glue_ops": glue.summary()["glue_ops"]}),
          flush=True)
    t = alternate({"strict": strict.replay, "deconv_as_glue": glue.replay}, reps, rounds)
    a, b = strict.output_tensors()[0].cpu(), glue.output_tensors()[0].cpu()
    for k, ts in t.items():
        line(f"unet_b{B}", k, ts)
    print(json.dumps({"plan": "label_agreement", "frac": round(float((a == b).float().mean()), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default=",".join(LAYERS))
    ap.add_argument("--impls", default="deconv,deconv:128x128,deconv:256x64,stuffed,torch_bf16,glue")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--plan", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deconv_probe measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    for name in [n for n in a.layers.split(",") if n]:
        Hi, Cin, Cout, k = LAYERS[name]
        fns, (y, y_ref) = candidates(a.batch, Hi, Cin, Cout, k, dev, g, a.impls.split(","))
        y_s = fns.pop("_stuffed_out", None)
        t = alternate(fns, a.reps, a.rounds)
        nbytes, flops = ideal_bytes(a.batch, Hi, Cin, Cout, k), useful_flops(a.batch, Hi, Cin, Cout, k)
        for kk, ts in t.items():
            line(name, kk, ts, nbytes if kk.startswith("deconv") else None, flops)
        # same layer, same inputs: the new kernel against the candidates that keep their output
        fns["deconv"]() if "deconv" in fns else None
        for other, buf in (("glue", y_ref), ("stuffed", y_s)):
            if "deconv" in fns and other in fns:
                fns[other]()
                torch.cuda.synchronize()
                err = (y.float() - buf.float()).abs().max().item()
                print(json.dumps({"layer": name, f"max_abs_diff_vs_{other}": round(err, 4)}), flush=True)
        del fns, y, y_ref, y_s
        torch.cuda.empty_cache()
    if a.plan:
        plan_times(a.batch, a.reps, a.rounds, dev)


if __name__ == "__main__":
    main()
