"""Padding-free causal attention (``kernels/attention_causal_packed.hip``): the packed step against
the padded ``causal_attention`` step on the same tokens, and the next-item model's packed plan
against its padded plan.

Candidates are alternated round by round in one process (``retrieval_probe.alternate``: device
events around ``reps`` launches, ``--rounds`` rounds after a warm-up of every candidate; the median
and the min..max spread of the rounds are printed).  Per ``S`` with ``H`` heads of 64 and
``B = tokens // S`` sessions, for two length profiles — ``uniform``: lengths uniform in [1, S];
``short``: 80 % of the sessions uniform in [1, S / 4], the rest uniform in [1, S]:

* ``padded``       ``K.attention(..., causal=True)`` on the left-padded ``[B * S]`` rows;
* ``packed``       ``K.packed_causal_attention`` on the same tokens packed into the next multiple of 64
  rows (the QKV values of a token are the same in both layouts);
* ``packed_rows``  the bookkeeping kernel the packed plan runs once per batch.

The summary line holds ``padded / packed`` with its range over the rounds, the share of real tokens,
and the largest difference between the two outputs on the real tokens.

``--model``: the default next-item model at B = 32 and 256, S = 64, sessions of mixed length: the
padded strict plan against the packed plan of the capacity the batch selects, per replay.

    python bench/packed_causal_probe.py --rounds 5 --model
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


def lengths(profile, B, S, g):
    full = torch.randint(1, S + 1, (B,), generator=g)
    if profile == "uniform":
        return full
    short = torch.randint(1, max(1, S // 4) + 1, (B,), generator=g)
    return torch.where(torch.rand(B, generator=g) < 0.8, short, full)


def step(S, H, tokens, profile, dev, window_us, rounds):
    B = max(1, tokens // S)
    g = torch.Generator().manual_seed(S)
    lens = lengths(profile, B, S, g)
    keep = torch.arange(S)[None, :] >= (S - lens)[:, None]  # left-padded
    ids = keep.to(torch.int32).reshape(-1).to(dev)
    qkv = torch.randn((B * S, 3 * H * 64), generator=g).to(BF).to(dev)
    n = int(lens.sum())
    T = -(-n // 64) * 64
    pq = torch.zeros((T, 3 * H * 64), dtype=BF, device=dev)
    pq[:n] = qkv[keep.reshape(-1).to(dev)]
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    cu = cu.to(dev)
    start, last = torch.empty(T, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    K.packed_rows(cu, B, T, start, last)
    out = torch.empty((B * S, H * 64), dtype=BF, device=dev)
    pout = torch.zeros((T, H * 64), dtype=BF, device=dev)
    fns = {"padded": lambda: K.attention(qkv, ids, B, S, H, out=out, causal=True),
           "packed": lambda: K.packed_causal_attention(pq, cu, start, B, H, out=pout),
           "packed_rows": lambda: K.packed_rows(cu, B, T, start, last)}
    t, reps = alternate(fns, window_us, rounds)
    shape = f"attn_s{S}_h{H}_b{B}_{profile}"
    for name, ts in t.items():
        line(shape, name, ts, reps=reps[name])
    r = [a / b for a, b in zip(t["padded"], t["packed"])]
    fns["padded"]()
    fns["packed"]()
    diff = float((out[keep.reshape(-1).to(dev)].float() - pout[:n].float()).abs().max())
    print(json.dumps({"shape": shape, "real_tokens": n, "share_of_padded_rows": round(n / (B * S), 3), "capacity": T,
                      "padded_over_packed": round(statistics.median(t["padded"]) / statistics.median(t["packed"]), 2),
                      "padded_over_packed_range": [round(min(r), 2), round(max(r), 2)],
                      "max_abs_diff_padded_vs_packed": diff}), flush=True)


def model(dev, window_us, rounds):
    from flink_tensorflow_amd.models.zoo.next_item import NextItemConfig, NextItemModel

    cfg, S = NextItemConfig(), 64
    models = {pack: NextItemModel(cfg, seq_len=S, buckets=(32, 256), device=str(dev), lanes=1, pack_tokens=pack)
              for pack in (False, True)}
    for m in models.values():
        m.open()
    try:
        for B in (32, 256):
            ids = torch.randint(1, cfg.num_items, (B, S), generator=torch.Generator().manual_seed(0), dtype=torch.int32)
            for b in range(B):
                ids[b, :(b * 7) % S] = 0  # sessions of mixed length, left-padded (causal_probe's batch)
            padded, packed = models[False]._plans[B], models[True]._plans[B].select(ids)
            for p in (padded, packed):
                p.input_buffer("item_ids:0").copy_(ids)
            name = f"next_item_h{cfg.hidden}_l{cfg.layers}_s{S}_n{cfg.num_items}_k10_b{B}"
            s = models[True]._plans[B].summary()
            print(json.dumps({"plan": name, "hip_graph": s["hip_graph"], "packed_kinds": s["kinds"],
                              "real_tokens": int((ids != 0).sum()), "padded_rows": B * S,
                              "capacity": packed.token_cap, "capacities": s["token_capacities"]}), flush=True)
            t, reps = alternate({"padded_replay": padded.replay, "packed_replay": packed.replay}, window_us, rounds)
            for impl, ts in t.items():
                line(name, impl, ts, reps=reps[impl])
            r = [a / b for a, b in zip(t["padded_replay"], t["packed_replay"])]
            padded.replay()
            packed.replay()
            diff = float((padded.output_tensors()[0].float() - packed.output_tensors()[0].float()).abs().max())
            print(json.dumps({"plan": name, "padded_over_packed": round(
                statistics.median(t["padded_replay"]) / statistics.median(t["packed_replay"]), 2),
                "padded_over_packed_range": [round(min(r), 2), round(max(r), 2)],
                "max_abs_diff_top_scores": diff}), flush=True)
    finally:
        for m in models.values():
            m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="device work per timed window")
    ap.add_argument("--seqs", type=int, nargs="+", default=[64, 128, 512])
    ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=262144)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("packed_causal_probe measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    if not a.no_step:
        for S in a.seqs:
            for profile in ("uniform", "short"):
                step(S, a.heads, a.tokens, profile, dev, a.window_ms * 1e3, a.rounds)
    if a.model:
        model(dev, a.window_ms * 1e3, a.rounds)


if __name__ == "__main__":
    main()
