"""Sliding-window causal attention (``kernels/attention_window.hip``): the ``window_attention`` step
against the ``causal_attention`` step on the same buffers.

Candidates are alternated round by round in one process as in ``causal_probe.py`` (device events
around ``reps`` launches, ``--rounds`` rounds after a warm-up of every candidate; the median and the
min..max spread of the rounds are printed; ``reps`` is sized so that a window holds about
``--window-ms`` of device work).  Per ``(S, W)`` with ``H`` heads of ``Dh`` and ``B`` sequences
(``randn`` bf16 QKV, no padding):

* ``window``  ``K.attention(..., causal=True, window=W)``;
* ``causal``  ``K.attention(..., causal=True)`` (``S <= 2048`` only).

The summary line holds the ratio of the medians with its range over the rounds, the ratio the key
walks alone predict, ``(W / KB + 2) / (S / (2 KB) + 1)`` (steps of a windowed query block over the mean
steps of a causal one, KB = 64 keys; 32 at ``Dh`` = 128), and the largest difference between
``window`` and fp32 ``torch`` attention under the band mask on the first sequence.

    python bench/window_attention_probe.py --rounds 5
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


def step(B, H, Dh, S, W, dev, window_us, rounds):
    g = torch.Generator(device=dev).manual_seed(S + W)
    qkv = torch.randn((B * S, 3 * H * Dh), device=dev, generator=g).to(BF)
    ids = torch.ones(B * S, dtype=torch.int32, device=dev)
    out = torch.empty((B * S, H * Dh), dtype=BF, device=dev)
    fns = {"window": lambda: K.attention(qkv, ids, B, S, H, out=out, causal=True, window=W)}
    if S <= K.CAUSAL_ATTENTION_MAX_SEQ:
        fns["causal"] = lambda: K.attention(qkv, ids, B, S, H, out=out, causal=True)
    t, reps = alternate(fns, window_us, rounds)
    shape = f"attn_b{B}_h{H}_d{Dh}_s{S}_w{W}"
    for name, ts in t.items():
        line(shape, name, ts, reps=reps[name])
    kb = 32 if Dh == 128 else 64
    summary = {"shape": shape, "window_us": round(statistics.median(t["window"]), 1)}
    if "causal" in t:
        r = [w / c for w, c in zip(t["window"], t["causal"])]
        summary["window_over_causal"] = round(statistics.median(t["window"]) / statistics.median(t["causal"]), 3)
        summary["window_over_causal_range"] = [round(min(r), 3), round(max(r), 3)]
        summary["step_count_ratio"] = round((W / kb + 2) / (S / (2 * kb) + 1), 3)
    fns["window"]()
    q, k, v = qkv[:S].float().view(S, 3, H, Dh).permute(1, 2, 0, 3)  # the first sequence in fp32
    d = torch.arange(S, device=dev)[:, None] - torch.arange(S, device=dev)[None, :]
    s = ((q @ k.transpose(-1, -2)) / Dh ** 0.5).masked_fill(~((d >= 0) & (d < W)), float("-inf"))
    ref = (torch.softmax(s, -1) @ v).permute(1, 0, 2).reshape(S, H * Dh)
    summary["max_abs_diff_fp32"] = float((out[:S].float() - ref).abs().max())
    print(json.dumps(summary), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="device work per timed window")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--head-dim", type=int, default=64)
    ap.add_argument("--cases", type=int, nargs="+", default=[2048, 128, 2048, 512, 8192, 128],
                    help="S W pairs")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_attention_probe measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    for S, W in zip(a.cases[::2], a.cases[1::2]):
        step(a.batch, a.heads, a.head_dim, S, W, dev, a.window_ms * 1e3, a.rounds)


if __name__ == "__main__":
    main()
