"""The generator kernels (``kernels/instnorm.hip``, ``kernels/pad.hip``) on the layers of the default
style-transfer model (``models/zoo/style_transfer.py``: base 32, 5 blocks, 256x256) at B = 8 and 32,
against PyTorch on the same buffers, and the whole plan against the same graph without the new
lowerings.

Per layer, alternated round by round in one process (device events around ``--reps`` launches,
``--rounds`` rounds after a warm-up of every candidate; the median and the min..max spread of the
rounds are printed):

* ``instnorm``   ``K.instance_norm`` (three launches: partials, finalize, normalise) with the
                 layer's activation, against ``torch``: ``F.instance_norm`` (+ ``relu_``) on the
                 bf16 channels-last view of the same NHWC buffer;
* ``pad``        ``K.pad_nhwc`` in reflect mode, against ``torch``: ``F.pad(mode="reflect")`` on the
                 channels-last view;
* ``image_out``  ``K.image_out`` (tanh, 127.5, 127.5, clamp, uint8), against ``torch``: the five
                 elementwise ops on the three logical channels.

``ideal_bytes`` counts one read and one write for ``pad`` and ``image_out`` (the physical 8-channel
pixels of the padded RGB buffers included) and two reads and one write for ``instnorm``; ``gbps``
is that over the time, ``roof`` its share of the 6.29 TB/s copy rate measured on the MI355X.

``--plan`` times the hipGraph replay of the strict plan against a non-strict plan of the same
graph whose instance norms, pads and output stage are forced to glue by monkey-patches local to
this script (the captured-glue plan a compiler without ``generator_lowering.py`` would build).

    python bench/generator_probe.py --reps 20 --rounds 7 --plan
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from flink_tensorflow_amd.ops import kernels as K  # noqa: E402

COPY_ROOF = 6.29e12  # B/s, MI355X_MICROARCH measured copy rate
# name: (kind, H = W, physical C, logical C, pad or activation, how often the default model runs it)
LAYERS = {
    "pad3_rgb_256": ("pad", 256, 8, 3, 3, 1),
    "pad1_64x128": ("pad", 64, 128, 128, 1, 10),
    "pad3_256x32": ("pad", 256, 32, 32, 3, 1),
    "in_256x32_relu": ("instnorm", 256, 32, 32, "relu", 2),
    "in_128x64_relu": ("instnorm", 128, 64, 64, "relu", 2),
    "in_64x128_relu": ("instnorm", 64, 128, 128, "relu", 6),
    "in_64x128": ("instnorm", 64, 128, 128, None, 5),
    "image_out_256": ("image_out", 256, 8, 3, "tanh", 1),
}


def candidates(kind, B, hw, C, Cl, arg, dev, g):
    x = torch.randn((B, hw, hw, C), device=dev, generator=g).to(torch.bfloat16)
    if Cl != C:
        x[..., Cl:] = 0
    xc = x.permute(0, 3, 1, 2)  # NCHW view of the NHWC buffer (channels-last)
    if kind == "instnorm":
        gamma = torch.rand(C, device=dev, generator=g) + 0.5
        beta = torch.randn(C, device=dev, generator=g) * 0.5
        g16, b16 = gamma.to(torch.bfloat16), beta.to(torch.bfloat16)
        y = torch.empty_like(x)
        scratch = torch.empty(K.instance_norm_scratch_numel(B, hw, hw, C), dtype=torch.float32, device=dev)

        def ours():
            K.instance_norm(x, gamma, beta, 1e-5, arg, out=y, scratch=scratch)

        def ref():
            t = F.instance_norm(xc, weight=g16, bias=b16, eps=1e-5)
            if arg == "relu":
                t.relu_()

        return {"instnorm": ours, "torch": ref}, 3 * x.numel() * 2
    if kind == "pad":
        p = arg
        y = torch.empty((B, hw + 2 * p, hw + 2 * p, C), dtype=torch.bfloat16, device=dev)

        def ours():
            K.pad_nhwc(x, (p, p, p, p), "reflect", out=y, channels=Cl)

        def ref():
            F.pad(xc, (p, p, p, p), mode="reflect")

        return {"pad": ours, "torch": ref}, (x.numel() + y.numel()) * 2
    out = torch.empty((B, hw, hw, Cl), dtype=torch.uint8, device=dev)

    def ours():
        K.image_out(x, Cl, arg, 127.5, 127.5, (0.0, 255.0), out=out)

    def ref():
        x[..., :Cl].float().tanh_().mul_(127.5).add_(127.5).clamp_(0.0, 255.0).to(torch.uint8)

    return {"image_out": ours, "torch": ref}, x.numel() * 2 + out.numel()


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


def line(layer, name, ts, nbytes=None, **extra):
    med = statistics.median(ts)
    rec = {"layer": layer, "impl": name, "us": round(med, 1), "min": round(min(ts), 1), "max": round(max(ts), 1), **extra}
    if nbytes is not None:
        rec["ideal_bytes"] = nbytes
        rec["gbps"] = round(nbytes / med / 1e3, 1)
        rec["roof"] = round(nbytes / (med * 1e-6) / COPY_ROOF, 3)
    print(json.dumps(rec), flush=True)


def plan_times(B, reps, rounds, dev):
    from flink_tensorflow_amd.graph.compiler import CompiledFunction
    from flink_tensorflow_amd.graph.graph import Graph
    from flink_tensorflow_amd.models.zoo.style_transfer import style_transfer_graph_def

    g = Graph.from_graph_def(style_transfer_graph_def())
    feeds = {"images:0": ((B, 256, 256, 3), "UINT8")}
    imgs = torch.randint(0, 256, (B, 256, 256, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    strict = CompiledFunction(g, feeds, ["stylized:0"], dev, strict=True)
    # (the last conv still leaves its Tanh alone: the implicit-GEMM kernel has no tanh epilogue for it on
    # the device, so the Tanh is a glue op of the comparison plan like the rest of the output stage)
    saved = {k: getattr(CompiledFunction, k) for k in ("_lower_instnorm_group", "_lower_pad", "_lower_image_out")}
    CompiledFunction._lower_instnorm_group = lambda self, grp: False           # this script only
    CompiledFunction._lower_pad = lambda self, node: self._lower_glue(node, host_consts=(1, 2))
    CompiledFunction._lower_image_out = lambda self, node: False
    try:
        glue = CompiledFunction(g, feeds, ["stylized:0"], dev, strict=False)
    finally:
        for k, v in saved.items():
            setattr(CompiledFunction, k, v)
    for p in (strict, glue):
        p.input_buffer("images:0").copy_(imgs)
        assert p.summary()["hip_graph"]
    print(json.dumps({"plan": "strict", "kinds": strict.summary()["kinds"]}), flush=True)
    print(json.dumps({"plan": "generator_ops_as_glue", "kinds": glue.summary()["kinds"],
                      "glue_ops": glue.summary()["glue_ops"]}), flush=True)
    t = alternate({"strict": strict.replay, "generator_ops_as_glue": glue.replay}, reps, rounds)
    a, b = strict.output_tensors()[0].cpu().int(), glue.output_tensors()[0].cpu().int()
    for k, ts in t.items():
        line(f"style_transfer_b{B}", k, ts)
    print(json.dumps({"plan": "pixel_agreement", "max_counts": int((a - b).abs().max()),
                      "frac_equal": round(float((a == b).float().mean()), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default=",".join(LAYERS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--plan", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("generator_probe measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    batches = [int(b) for b in a.batches.split(",") if b]
    for B in batches:
        for name in [n for n in a.layers.split(",") if n]:
            kind, hw, C, Cl, arg, count = LAYERS[name]
            fns, nbytes = candidates(kind, B, hw, C, Cl, arg, dev, g)
            for k, ts in alternate(fns, a.reps, a.rounds).items():
                line(name, k, ts, nbytes if k != "torch" else None, batch=B, per_model=count)
            del fns
            torch.cuda.empty_cache()
    if a.plan:
        for B in batches:
            plan_times(B, a.reps, a.rounds, dev)


if __name__ == "__main__":
    main()
