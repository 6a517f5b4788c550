"""Depthwise conv (``kernels/dwconv.hip``) against what a plan ran before it existed, on the
nine distinct depthwise layers of MobileNet-V1 at B=256, and the whole MobileNet-V1 plan.

Per layer, alternated round by round in one process (device events around ``--reps`` launches,
``--rounds`` rounds after a warm-up of every candidate; the median and the min..max spread of
the rounds are printed):

* ``dwconv``        the launcher's choice; ``dwconv:1x4 / 2x2 / generic`` pin a kernel;
* ``glue``          the steps a plan without the lowering runs for the layer: the interpreter's
                    ``DepthwiseConv2dNative`` and ``FusedBatchNormV3`` as captured glue ops (fp32
                    torch ops on the bf16 buffers, results copied back to bf16) and the
                    standalone Relu6 elementwise kernel;
* ``torch_bf16``    the same three ops on bf16 tensors, no fp32 round trip;
* ``pool3x3``       ``K.pool2d_nhwc`` (max, 3x3, the layer's stride): the in-tree kernel with
                    the same access pattern.

``gbps`` is the ideal traffic (input + output + weights + bias, from the shapes) over the time;
``roof`` its share of the 6.29 TB/s copy rate measured on the MI355X.

``--plan`` times the hipGraph replay of the strict MobileNet-V1 plan against a non-strict plan
whose depthwise layers are forced to glue by a monkey-patch local to this script.

    python bench/dwconv_probe.py --reps 20 --rounds 7 --plan
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from flink_tensorflow_amd.graph.ops_nn import conv2d_tf, fused_batch_norm_inference, same_pads  # noqa: E402
from flink_tensorflow_amd.ops import kernels as K  # noqa: E402

COPY_ROOF = 6.29e12  # B/s, MI355X_MICROARCH measured copy rate
LAYERS = {  # name: (H = W, C, stride)
    "112x32s1": (112, 32, 1), "112x64s2": (112, 64, 2), "56x128s1": (56, 128, 1), "56x128s2": (56, 128, 2),
    "28x256s1": (28, 256, 1), "28x256s2": (28, 256, 2), "14x512s1": (14, 512, 1), "14x512s2": (14, 512, 2),
    "7x1024s1": (7, 1024, 1),
}
PINS = {**K.DWCONV_TILES, "generic": K.DWCONV_GENERIC}


def ideal_bytes(B, H, C, s):
    Ho = -(-H // s)
    return 2 * B * H * H * C + 2 * B * Ho * Ho * C + 2 * 9 * C + 4 * C


def candidates(B, H, C, s, dev, g, which):
    pads = (*same_pads(H, 3, s), *same_pads(H, 3, s))
    Ho = -(-H // s)
    x = torch.randn((B, H, H, C), device=dev, generator=g).to(torch.bfloat16)
    w = torch.randn((3, 3, C, 1), device=dev, generator=g) * 0.3
    gamma, beta, mean = (torch.randn(C, device=dev, generator=g) * 0.1 + o for o in (1.0, 0.0, 0.0))
    var = torch.rand(C, device=dev, generator=g) + 0.5
    sc = gamma * torch.rsqrt(var + 1e-3)
    w_fold = (w[..., 0] * sc).reshape(9, C).to(torch.bfloat16).contiguous()
    b_fold = (beta - mean * sc).float().contiguous()
    y = torch.empty((B, Ho, Ho, C), dtype=torch.bfloat16, device=dev)
    t1, t2, t3 = (torch.empty_like(y) for _ in range(3))
    w_g = w.reshape(3, 3, 1, C)
    w_g16 = w_g.to(torch.bfloat16)
    p16 = [t.to(torch.bfloat16) for t in (gamma, beta, mean, var)]
    fns = {}
    for name in which:
        if name.startswith("dwconv"):
            tile = PINS[name.split(":")[1]] if ":" in name else 0

            def fn(tile=tile):
                K.dwconv2d_nhwc(x, w_fold, b_fold, (s, s), pads, (1, 1), K.ACT_RELU6, out=y, tile=tile)
        elif name == "glue":
            def fn():
                t1.copy_(conv2d_tf(x.float(), w_g, (s, s), "SAME", (1, 1), groups=C))
                t2.copy_(fused_batch_norm_inference(t1.float(), gamma, beta, mean, var, 1e-3))
                K.binary(t2, 0.0, "add", act=K.ACT_RELU6, out=t3)
        elif name == "torch_bf16":
            def fn():
                a = conv2d_tf(x, w_g16, (s, s), "SAME", (1, 1), groups=C)
                torch.clamp(fused_batch_norm_inference(a, *p16, 1e-3), 0, 6, out=t3)
        elif name == "pool3x3":
            def fn():
                K.pool2d_nhwc(x, (3, 3), (s, s), pads, "max", out=t1)
        else:
            raise SystemExit(f"unknown candidate {name!r}")
        fns[name] = fn
    return fns, (y, t3)


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


def line(layer, name, ts, nbytes=None):
    med = statistics.median(ts)
    rec = {"layer": layer, "impl": name, "us": round(med, 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}
    if nbytes is not None:
        rec["gbps"] = round(nbytes / med / 1e3, 1)
        rec["roof"] = round(nbytes / (med * 1e-6) / COPY_ROOF, 3)
    print(json.dumps(rec), flush=True)


def plan_times(B, reps, rounds, dev, alpha):
    from flink_tensorflow_amd.graph.compiler import CompiledFunction
    from flink_tensorflow_amd.graph.graph import Graph
    from flink_tensorflow_amd.models.zoo.mobilenet import mobilenet_v1_graph_def

    g = Graph.from_graph_def(mobilenet_v1_graph_def(alpha=alpha, image_hw=(256, 256)))
    feeds = {"images:0": ((B, 256, 256, 3), "UINT8")}
    imgs = torch.randint(0, 256, (B, 256, 256, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    strict = CompiledFunction(g, feeds, ["top_k:0", "top_k:1"], dev, strict=True)
    lower = CompiledFunction._lower_dwconv
    CompiledFunction._lower_dwconv = lambda self, node: self._lower_glue(node)  # this script only
    try:
        glue = CompiledFunction(g, feeds, ["top_k:0", "top_k:1"], dev, strict=False)
    finally:
        CompiledFunction._lower_dwconv = lower
    for p in (strict, glue):
        p.input_buffer("images:0").copy_(imgs)
        assert p.summary()["hip_graph"]
    print(json.dumps({"plan": "strict", "kinds": strict.summary()["kinds"]}), flush=True)
    print(json.dumps({"plan": "dw_as_glue", "kinds": glue.summary()["kinds"], "glue_ops": glue.summary()["glue_ops"]}),
          flush=True)
    t = alternate({"strict": strict.replay, "dw_as_glue": glue.replay}, reps, rounds)
    a, b = strict.output_tensors()[1][:, 0].cpu(), glue.output_tensors()[1][:, 0].cpu()
    for k, ts in t.items():
        line(f"mobilenet_v1_{alpha}_b{B}", k, ts)
    print(json.dumps({"plan": "top1_agreement", "frac": round(float((a == b).float().mean()), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default=",".join(LAYERS))
    ap.add_argument("--impls", default="dwconv,dwconv:1x4,dwconv:2x2,dwconv:generic,pool3x3,torch_bf16,glue")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--plan", action="store_true")
    ap.add_argument("--alpha", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dwconv_probe measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    for name in [n for n in a.layers.split(",") if n]:
        H, C, s = LAYERS[name]
        fns, (y, y_ref) = candidates(a.batch, H, C, s, dev, g, a.impls.split(","))
        t = alternate(fns, a.reps, a.rounds)
        nbytes = ideal_bytes(a.batch, H, C, s)
        for k, ts in t.items():
            line(name, k, ts, nbytes if k.startswith("dwconv") or k == "pool3x3" else None)
        if "dwconv" in fns and ("glue" in fns or "torch_bf16" in fns):
            # same layer, same inputs: the new kernel against the ops it replaces
            fns["dwconv"]()
            fns["glue" if "glue" in fns else "torch_bf16"]()
            torch.cuda.synchronize()
            err = (y.float() - y_ref.float()).abs().max().item()
            print(json.dumps({"layer": name, "max_abs_diff_vs_glue": round(err, 4)}), flush=True)
        del fns, y, y_ref
        torch.cuda.empty_cache()
    if a.plan:
        plan_times(a.batch, a.reps, a.rounds, dev, a.alpha)


if __name__ == "__main__":
    main()
