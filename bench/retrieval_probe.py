"""Retrieval (``kernels/retrieve.hip``): the fused score GEMM + top-k against the path it replaces,
and the two-tower model end to end.

Candidates are alternated round by round in one process (device events around ``reps`` launches,
``--rounds`` rounds after a warm-up of every candidate; the median and the min..max spread of the
rounds are printed).  ``reps`` is sized per shape so that a window holds about ``--window-ms`` of
device work.  Per shape ``N x D x k x B`` (items and queries ``normal`` in bf16, bias uniform):

* ``retrieve``          both launches of the ``retrieve`` step (``K.retrieve_topk``, default chunk);
* ``retrieve:partial``  the scan alone;  ``retrieve:merge``  the merge alone;
* ``gemm_pp+topk``      what a GPU plan ran before: ``K.gemm_pp`` writing the bf16 ``[B, N]`` score
  matrix (bias in its epilogue) and ``torch.topk`` on it, on the same tensors.

The summary line of a shape holds the ratio of the medians with the ratio's range over the
rounds, the roof (reading the ``N * D * 2`` bytes of items once at the measured 6.29 TB/s copy
rate), the step's share of it, and a check of the step against fp32 ``torch`` scores (fraction of
equal indices, largest value difference; skipped above 2^28 scores).

``--model``: the strict plan of the default two-tower model at B = 32 and 256 against the plan of
the same graph with ``scores`` fetched as well, which keeps the ``gemm`` + glue ``TopKV2`` path.

    python bench/retrieval_probe.py --rounds 5 --model
"""
import argparse
import itertools
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from flink_tensorflow_amd.ops import kernels as K  # noqa: E402

BF = torch.bfloat16
COPY_BYTES_PER_US = 6.29e6  # measured device copy rate, 6.29 TB/s


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def alternate(fns, window_us, rounds):
    reps = {}
    for k, fn in fns.items():  # warm up every candidate; size its window from a first timing
        fn()
        fn()
        torch.cuda.synchronize()
        reps[k] = max(3, min(2000, int(window_us / max(timed(fn, 3), 1.0))))
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, reps[k]))
    return t, reps


def line(shape, name, ts, **extra):
    print(json.dumps({"shape": shape, "impl": name, "us": round(statistics.median(ts), 1), "min": round(min(ts), 1),
                      "max": round(max(ts), 1), **extra}), flush=True)


def step(N, D, k, B, dev, window_us, rounds):
    g = torch.Generator(device=dev).manual_seed(0)
    items = torch.randn((N, D), device=dev, generator=g).to(BF)
    q = torch.randn((B, D), device=dev, generator=g).to(BF)
    bias = torch.rand((N,), device=dev, generator=g) - 0.5
    chunk = K.retrieve_chunk(B, N, D, k)
    out = (torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int32, device=dev))
    scratch = torch.empty(K.retrieve_scratch_numel(B, N, k, chunk), dtype=torch.int64, device=dev)
    scores = torch.empty((B, N), dtype=BF, device=dev)

    def retrieve(part=0):
        return lambda: K.retrieve_topk(q, items, k, bias, chunk=chunk, out=out, scratch=scratch, part=part)

    def old():
        K.gemm_pp(q, items, bias, out=scores, splits=1)
        torch.topk(scores, k, dim=-1)

    fns = {"retrieve": retrieve(), "retrieve:partial": retrieve(1), "retrieve:merge": retrieve(2), "gemm_pp+topk": old}
    t, reps = alternate(fns, window_us, rounds)
    shape = f"retrieve_n{N}_d{D}_k{k}_b{B}"
    for name, ts in t.items():
        line(shape, name, ts, reps=reps[name])
    ratios = [o / r for o, r in zip(t["gemm_pp+topk"], t["retrieve"])]
    roof = N * D * 2 / COPY_BYTES_PER_US
    med = statistics.median(t["retrieve"])
    summary = {"shape": shape, "chunk": chunk, "chunks": -(-N // chunk), "query_tiles": -(-B // (32 if k > 64 else 64)),
               "old_over_new": round(statistics.median(t["gemm_pp+topk"]) / med, 2),
               "old_over_new_range": [round(min(ratios), 2), round(max(ratios), 2)],
               "roof_us": round(roof, 1), "share_of_roof": round(roof / med, 3),
               "partial_share_of_roof": round(roof / statistics.median(t["retrieve:partial"]), 3),
               "score_matrix_bytes": B * N * 2, "item_bytes": N * D * 2}
    if B * N <= 2 ** 28:
        fns["retrieve"]()
        ref = torch.topk(q.float() @ items.float().t() + bias, k, dim=-1)
        summary["indices_equal_fp32"] = round(float((ref.indices == out[1]).float().mean()), 5)
        summary["values_max_abs_diff_fp32"] = float((ref.values - out[0]).abs().max())
    print(json.dumps(summary), flush=True)


def model(dev, window_us, rounds):
    from flink_tensorflow_amd.graph.compiler import CompiledFunction
    from flink_tensorflow_amd.graph.graph import Graph
    from flink_tensorflow_amd.models.zoo.two_tower import two_tower_graph_def

    g = Graph.from_graph_def(two_tower_graph_def())
    for B in (32, 256):
        feeds = {"features:0": ((B, 64), "FLOAT")}
        x = torch.randn((B, 64), generator=torch.Generator().manual_seed(0))
        name = f"two_tower_f64_h256x128_d64_n100000_k10_b{B}"
        strict = CompiledFunction(g, feeds, ["top_k:0", "top_k:1"], dev, strict=True)
        strict.input_buffer("features:0").copy_(x)
        fns = {"replay:retrieve": strict.replay}
        print(json.dumps({"plan": name, "hip_graph": strict.summary()["hip_graph"], "kinds": strict.summary()["kinds"]}),
              flush=True)
        try:  # the same graph with the scores fetched too: gemm + glue TopKV2, as before the step existed
            glue = CompiledFunction(g, feeds, ["top_k:0", "top_k:1", "scores:0"], dev)
            glue.input_buffer("features:0").copy_(x)
            fns["replay:gemm+glue_topk"] = glue.replay
            print(json.dumps({"plan": name + "_glue", "hip_graph": glue.summary()["hip_graph"],
                              "kinds": glue.summary()["kinds"], "glue_ops": glue.summary()["glue_ops"]}), flush=True)
        except Exception as e:  # noqa: BLE001 - reported, not hidden
            print(json.dumps({"plan": name + "_glue", "captured": False, "error": f"{type(e).__name__}: {e}"[:300]}),
                  flush=True)
        t, reps = alternate(fns, window_us, rounds)
        for k, ts in t.items():
            line(name, k, ts, reps=reps[k])
        if len(t) == 2:
            r = [o / n for o, n in zip(t["replay:gemm+glue_topk"], t["replay:retrieve"])]
            print(json.dumps({"plan": name, "old_over_new": round(statistics.median(r), 2),
                              "old_over_new_range": [round(min(r), 2), round(max(r), 2)]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="device work per timed window")
    ap.add_argument("--items", type=int, nargs="+", default=[100_000, 1_000_000, 4_000_000])
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_probe measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    if not a.no_step:
        for N, D, k, B in itertools.product(a.items, a.dims, a.ks, a.batches):
            step(N, D, k, B, dev, a.window_ms * 1e3, a.rounds)
    if a.model:
        model(dev, a.window_ms * 1e3, a.rounds)


if __name__ == "__main__":
    main()
