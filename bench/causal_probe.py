"""Causal attention (``kernels/attention_causal.hip``): the ``causal_attention`` step against the
full-square kernel and torch SDPA, and the next-item model's strict plan.

Candidates are alternated round by round in one process (device events around ``reps`` launches,
``--rounds`` rounds after a warm-up of every candidate; the median and the min..max spread of the
rounds are printed; ``reps`` is sized so that a window holds about ``--window-ms`` of device work).
Per ``S`` with ``H`` heads of 64 and ``B = tokens // S`` (``randn`` bf16 QKV, no padding):

* ``causal``       ``K.attention(..., causal=True)``;
* ``full``         ``K.attention`` without ``causal`` on the same buffers: the whole S x S square;
* ``sdpa_causal``  ``torch`` ``scaled_dot_product_attention(is_causal=True)`` on the same data as
  ``[B, H, S, 64]`` views of the QKV buffer.

The summary line of a shape holds the ratios of the medians with their ranges over the rounds, the
MFMA work of the causal walk (``2 * 2 * 64 * 64 * 64`` flops per visited 64 x 64 tile and head)
over the median time, and the largest difference between ``causal`` and fp32 ``torch`` attention.

``--model``: the default next-item model's strict plan per call at B = 32 and 256.

    python bench/causal_probe.py --rounds 5 --model
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from retrieval_probe import alternate, line  # noqa: E402  (the script's directory is on the path)
from flink_tensorflow_amd.ops import kernels as K  # noqa: E402

BF = torch.bfloat16


def step(S, H, tokens, dev, window_us, rounds):
    B = max(1, tokens // S)
    g = torch.Generator(device=dev).manual_seed(S)
    qkv = torch.randn((B * S, 3 * H * 64), device=dev, generator=g).to(BF)
    ids = torch.ones(B * S, dtype=torch.int32, device=dev)
    out = torch.empty((B * S, H * 64), dtype=BF, device=dev)
    q, k, v = qkv.view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)  # [B, H, S, 64] views, as SDPA takes them
    sdpa = torch.nn.functional.scaled_dot_product_attention
    fns = {"causal": lambda: K.attention(qkv, ids, B, S, H, out=out, causal=True),
           "full": lambda: K.attention(qkv, ids, B, S, H, out=out),
           "sdpa_causal": lambda: sdpa(q, k, v, is_causal=True)}
    t, reps = alternate(fns, window_us, rounds)
    shape = f"attn_s{S}_h{H}_b{B}"
    for name, ts in t.items():
        line(shape, name, ts, reps=reps[name])
    med = statistics.median(t["causal"])
    nq = -(-S // 64)
    flops = B * H * (nq * (nq + 1) // 2) * 2 * 2 * 64 ** 3
    summary = {"shape": shape, "tokens": B * S, "causal_tflops_visited_tiles": round(flops / med / 1e6, 1)}
    for other in ("full", "sdpa_causal"):
        r = [o / c for o, c in zip(t[other], t["causal"])]
        summary[f"{other}_over_causal"] = round(statistics.median(t[other]) / med, 2)
        summary[f"{other}_over_causal_range"] = [round(min(r), 2), round(max(r), 2)]
    fns["causal"]()
    nb = min(B, max(1, 4096 // S))  # fp32 reference on the first sequences
    ref = sdpa(q[:nb].float(), k[:nb].float(), v[:nb].float(), is_causal=True).permute(0, 2, 1, 3).reshape(nb * S, H * 64)
    summary["max_abs_diff_fp32"] = float((out[:nb * S].float() - ref).abs().max())
    print(json.dumps(summary), flush=True)


def model(dev, window_us, rounds):
    from flink_tensorflow_amd.graph.compiler import CompiledFunction
    from flink_tensorflow_amd.graph.graph import Graph
    from flink_tensorflow_amd.models.zoo.next_item import NextItemConfig, next_item_graph_def

    cfg, S = NextItemConfig(), 64
    g = Graph.from_graph_def(next_item_graph_def(cfg, S, 10))
    for B in (32, 256):
        plan = CompiledFunction(g, {"item_ids:0": ((B, S), "INT32")}, ["top_k:0", "top_k:1"], dev, strict=True)
        ids = torch.randint(1, cfg.num_items, (B, S), generator=torch.Generator().manual_seed(0), dtype=torch.int32)
        for b in range(B):
            ids[b, :(b * 7) % S] = 0  # sessions of mixed length, left-padded
        plan.input_buffer("item_ids:0").copy_(ids)
        name = f"next_item_h{cfg.hidden}_l{cfg.layers}_s{S}_n{cfg.num_items}_k10_b{B}"
        print(json.dumps({"plan": name, "hip_graph": plan.summary()["hip_graph"], "kinds": plan.summary()["kinds"]}),
              flush=True)
        t, reps = alternate({"replay": plan.replay}, window_us, rounds)
        line(name, "replay", t["replay"], reps=reps["replay"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="device work per timed window")
    ap.add_argument("--seqs", type=int, nargs="+", default=[64, 128, 256, 512, 1024, 2048])
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("causal_probe measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    if not a.no_step:
        for S in a.seqs:
            step(S, a.heads, a.tokens, dev, a.window_ms * 1e3, a.rounds)
    if a.model:
        model(dev, a.window_ms * 1e3, a.rounds)


if __name__ == "__main__":
    main()
