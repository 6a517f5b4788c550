"""3-D conv and 3-D pooling (``kernels/conv3d.hip``) against what PyTorch-ROCm gives a user, on
the eight conv layers and five pools of the default C3D (16 x 112 x 112 clips) at B = 4 and 16,
on a ``KD = 1`` layer against the existing 2-D path, and on the whole C3D plan.

Per layer, alternated round by round in one process (device events around ``--reps`` launches,
``--rounds`` rounds after a warm-up of every candidate; the median and the min..max spread of
the rounds are printed):

* ``conv3d``        ``K.conv3d_ndhwc`` with bias + ReLU fused, the launcher's tile; conv1 reads
                    the 8-channel padded input the plan gives it;
* ``pool3d``        ``K.pool3d_ndhwc``;
* ``torch_bf16``    ``torch.nn.functional.conv3d`` (with bias, no ReLU) / ``max_pool3d`` on bf16
                    ``channels_last_3d`` tensors of the same shapes (conv1: 3 channels).

``tflops`` is the useful MACs (``2 * M * Cout * Cin * 27``, conv1 with ``Cin = 3``) over the time;
for a pool ``ideal_bytes`` is input + output, ``gbps`` that over the time and ``roof`` its share
of the 6.29 TB/s copy rate measured on the MI355X.

``--fold`` is the roof check of the kernel's K walk: a ``1x3x3`` layer run through
``K.conv3d_ndhwc`` and through ``K.conv2d_nhwc`` on the ``[N * D, H, W, C]`` view: the same GEMM.

``--plan`` times the hipGraph replay of the strict C3D plan.

    python bench/conv3d_probe.py --reps 10 --rounds 5 --fold --plan
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from flink_tensorflow_amd.models.zoo.c3d import c3d_layer_shapes  # noqa: E402
from flink_tensorflow_amd.ops import kernels as K  # noqa: E402

COPY_ROOF = 6.29e12  # B/s, MI355X_MICROARCH measured copy rate


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


def conv_layer(B, layer, dev, g, impls):
    (D, H, W, Cin), Cout = layer["in"], layer["out"][3]
    cin_phys = -(-Cin // 8) * 8
    x = torch.randn((B, D, H, W, cin_phys), device=dev, generator=g).to(torch.bfloat16)
    x[..., Cin:] = 0
    w = torch.randn((3, 3, 3, cin_phys, Cout), device=dev, generator=g) * (2.0 / (27 * Cin)) ** 0.5
    w[:, :, :, Cin:] = 0
    bias = torch.randn(Cout, device=dev, generator=g) * 0.1
    wp = K.conv3d_pack_weights(w).to(torch.bfloat16)
    y = torch.empty((B, D, H, W, Cout), dtype=torch.bfloat16, device=dev)
    fns, keep = {}, {}
    if "conv3d" in impls:
        fns["conv3d"] = lambda: K.conv3d_ndhwc(x, wp, bias, (3, 3, 3), (1, 1, 1), (1,) * 6, "relu", out=y)
    if "torch_bf16" in impls:
        xc = x[..., :Cin].permute(0, 4, 1, 2, 3).contiguous(memory_format=torch.channels_last_3d)
        wt = w[:, :, :, :Cin].permute(4, 3, 0, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last_3d)
        b16 = bias.to(torch.bfloat16)

        def fn():
            keep["t"] = F.conv3d(xc, wt, b16, padding=1)
        fns["torch_bf16"] = fn
    t = alternate(fns, *impls["_timing"])
    flops = 2 * B * D * H * W * Cout * Cin * 27
    for k, ts in t.items():
        line(f"{layer['name']}_b{B}", k, ts, None, flops)
    if len(fns) == 2:  # same layer, same inputs
        torch.cuda.synchronize()
        ref = torch.relu(keep["t"].float()).permute(0, 2, 3, 4, 1)
        err = (y.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)
        print(json.dumps({"layer": f"{layer['name']}_b{B}", "max_rel_diff_vs_torch": round(err, 4)}), flush=True)


def pool_layer(B, layer, dev, g, impls):
    (D, H, W, C), win, padding = layer["in"], layer["window"], layer["padding"]
    x = torch.randn((B, D, H, W, C), device=dev, generator=g).to(torch.bfloat16)
    out = layer["out"][:3]
    pads = tuple(p for a in range(3) for p in ((0, out[a] * win[a] - (D, H, W)[a]) if padding == "SAME" else (0, 0)))
    y = torch.empty((B, *out, C), dtype=torch.bfloat16, device=dev)
    fns = {}
    if "pool3d" in impls:
        fns["pool3d"] = lambda: K.pool3d_ndhwc(x, win, win, pads, "max", out=y)
    if "torch_bf16" in impls:
        xc = x.permute(0, 4, 1, 2, 3)  # NCDHW view of the NDHWC buffer (channels_last_3d)
        fns["torch_bf16"] = lambda: F.max_pool3d(xc, win, win, ceil_mode=padding == "SAME")
    t = alternate(fns, *impls["_timing"])
    nbytes = 2 * x.numel() + 2 * y.numel()
    for k, ts in t.items():
        line(f"{layer['name']}_b{B}", k, ts, nbytes)


def fold_check(B, dev, g, reps, rounds):
    """The same GEMM two ways: a 1x3x3 conv of [B, 8, 28, 28, 128] -> 128 through the 3-D kernel
    and through the 2-D implicit GEMM on the [B * 8, 28, 28, 128] view."""
    D, H, W, C = 8, 28, 28, 128
    x = torch.randn((B, D, H, W, C), device=dev, generator=g).to(torch.bfloat16)
    w = torch.randn((1, 3, 3, C, C), device=dev, generator=g) * (2.0 / (9 * C)) ** 0.5
    bias = torch.randn(C, device=dev, generator=g) * 0.1
    wp = K.conv3d_pack_weights(w).to(torch.bfloat16)
    w_ohwi = w[0].permute(3, 0, 1, 2).contiguous().to(torch.bfloat16)
    y3 = torch.empty((B, D, H, W, C), dtype=torch.bfloat16, device=dev)
    y2 = torch.empty((B * D, H, W, C), dtype=torch.bfloat16, device=dev)
    fns = {"conv3d": lambda: K.conv3d_ndhwc(x, wp, bias, (1, 3, 3), (1, 1, 1), (0, 0, 1, 1, 1, 1), "relu", out=y3),
           "conv2d_folded": lambda: K.conv2d_nhwc(x.view(B * D, H, W, C), w_ohwi, bias, None, (1, 1), (1, 1, 1, 1), (1, 1),
                                                  "relu", out=y2)}
    t = alternate(fns, reps, rounds)
    flops = 2 * B * D * H * W * C * C * 9
    for k, ts in t.items():
        line(f"fold_1x3x3_b{B}", k, ts, None, flops)
    torch.cuda.synchronize()
    print(json.dumps({"layer": f"fold_1x3x3_b{B}", "bit_equal": bool(torch.equal(y3.view(-1), y2.view(-1)))}), flush=True)


def plan_times(B, reps, rounds, dev):
    from flink_tensorflow_amd.graph.compiler import CompiledFunction
    from flink_tensorflow_amd.graph.graph import Graph
    from flink_tensorflow_amd.models.zoo.c3d import c3d_graph_def

    g = Graph.from_graph_def(c3d_graph_def())
    plan = CompiledFunction(g, {"clips:0": ((B, 16, 112, 112, 3), "UINT8")}, ["top_k:0", "top_k:1"], dev, strict=True)
    clips = torch.randint(0, 256, (B, 16, 112, 112, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    plan.input_buffer("clips:0").copy_(clips)
    assert plan.summary()["hip_graph"] and plan.summary()["glue_ops"] == []
    print(json.dumps({"plan": f"c3d_b{B}", "kinds": plan.summary()["kinds"]}), flush=True)
    line(f"c3d_b{B}", "strict_plan_replay", alternate({"replay": plan.replay}, reps, rounds)["replay"])
    del plan
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impls", default="conv3d,pool3d,torch_bf16")
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--layers", default="")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fold", action="store_true")
    ap.add_argument("--plan", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv3d_probe measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    impls = {k: True for k in a.impls.split(",") if k}
    impls["_timing"] = (a.reps, a.rounds)
    want = set(n for n in a.layers.split(",") if n)
    for B in (int(b) for b in a.batches.split(",") if b):
        for layer in c3d_layer_shapes():
            if want and layer["name"] not in want:
                continue
            (conv_layer if layer["kind"] == "conv" else pool_layer)(B, layer, dev, g, impls)
            torch.cuda.empty_cache()
        if a.fold:
            fold_check(B, dev, g, a.reps, a.rounds)
        if a.plan:
            plan_times(B, a.reps, a.rounds, dev)


if __name__ == "__main__":
    main()
