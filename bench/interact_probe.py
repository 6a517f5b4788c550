"""Ranking (``kernels/interact.hip``): the fused embedding gather + dot interaction against the same
result op by op in torch, and the DLRM plan end to end.

Candidates are alternated round by round in one process (device events around ``reps`` launches,
``--rounds`` rounds after a warm-up of every candidate; the median and the min..max spread of the
rounds are printed).  Per shape ``B x F x D`` with ``F`` tables of ``--rows`` rows, uniform and
Zipf(1.05) ids:

* ``interact``  ``K.dot_interact``: the activation vector + ``F`` lookups, the strict lower triangle
  behind a copy of the activation vector (``Wlog = D + (F + 1) F / 2``);
* ``torch``     ``F.embedding`` + ``torch.cat`` + ``torch.bmm`` + ``index_select`` + ``torch.cat`` on the
  same bf16 tensors.

The summary line holds the ratio of the medians, the roof ``B (F D 2 + D 2 + Wout 2 + 4 F)`` bytes at
the measured 6.29 TB/s copy rate, the step's share of it and the largest difference between both results.

``--model``: the strict plan of the default DLRM (tables of ``--model-rows`` rows) at B = 256 and
2048 against the plan of the same graph with the packed vectors fetched as well, which keeps the
lookups as ``embed`` steps and the rest as glue.

``--wide``: B = 32768 at ``F x D`` = 26 x 256, 48 x 128 and 48 x 256 (the other kernel instantiations).

``--tables fp8``: the same shapes with 8-bit tables (``kernels/interact_fp8.hip``) against the bf16 step on tables of
the same values and the same ids, each with its share of its own roof (a row is ``D + 1`` bytes instead of ``2 D``)
and whether both outputs have the same bits.

    python bench/interact_probe.py --rounds 5 --wide --model
    python bench/interact_probe.py --rounds 5 --wide --tables fp8
"""
import argparse
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
    return t


def line(shape, name, ts, **extra):
    print(json.dumps({"shape": shape, "impl": name, "us": round(statistics.median(ts), 1), "min": round(min(ts), 1),
                      "max": round(max(ts), 1), **extra}), flush=True)


def step(table, B, F, D, rows, dist, dev, window_us, rounds):
    g = torch.Generator(device=dev).manual_seed(B + D)
    if dist == "zipf":
        u = torch.rand((B, F), device=dev, generator=g).double()
        # P(id >= n) = (n + 1)^-0.05: a Zipf law of exponent 1.05
        ids = ((1.0 - u) ** (-1.0 / 0.05) - 1.0).clamp(0, rows - 1).to(torch.int32)
    else:
        ids = torch.randint(0, rows, (B, F), device=dev, generator=g, dtype=torch.int32)
    dense = torch.randn((B, D), device=dev, generator=g).to(BF)
    M = F + 1
    pairs = [(i, j) for i in range(M) for j in range(i)]
    wlog = D + len(pairs)
    wout = -(-wlog // 8) * 8
    meta = torch.tensor([(0, -1, 0)] + [(f * rows, f, rows) for f in range(F)], dtype=torch.int64).t().contiguous().to(dev)
    lut = K.dot_interact_lut(M, pairs, D).to(dev)
    out = torch.empty((B, wout), dtype=BF, device=dev)
    bases = (torch.arange(F, device=dev, dtype=torch.int64) * rows)[None, :]
    sel = torch.tensor([i * M + j for i, j in pairs], device=dev)

    def fused():
        K.dot_interact(table, ids, meta, lut, wlog, dense, True, out=out)

    def eager():
        T = torch.cat([dense[:, None, :], torch.nn.functional.embedding(ids.long() + bases, table)], 1)
        Z = torch.bmm(T, T.transpose(1, 2)).reshape(B, M * M)
        return torch.cat([dense, Z.index_select(1, sel)], 1)

    fused()
    diff = float((out[:, :wlog].float() - eager().float()).abs().max())  # summation orders differ: not bit-equal
    shape = f"B{B}xF{F}xD{D}:{dist}"
    t = alternate({"interact": fused, "torch": eager}, window_us, rounds)
    roof = B * (F * D * 2 + D * 2 + wout * 2 + 4 * F) / COPY_BYTES_PER_US
    for name, ts in t.items():
        line(shape, name, ts)
    mi, mt = statistics.median(t["interact"]), statistics.median(t["torch"])
    print(json.dumps({"shape": shape, "speedup": round(mt / mi, 2), "roof_us": round(roof, 2), "share_of_roof": round(roof / mi, 3),
                      "max_abs_diff": diff}), flush=True)


def fp8_tables(F, rows, D, dev):
    """Random 8-bit tables built on the device (finite codes, row exponents in -8..-4) and the bf16 table they stand
    for, one field at a time: ``(codes, exps, bf16 table)``."""
    g = torch.Generator(device=dev).manual_seed(F + D)
    finite = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
    value = K.dequantize_table_fp8(finite[:, None].expand(254, 16).contiguous(), torch.zeros(254, dtype=torch.int8))[:, 0].to(dev)
    codes = torch.empty((F * rows, D), dtype=torch.uint8, device=dev)
    exps = torch.randint(-8, -3, (F * rows,), device=dev, generator=g, dtype=torch.int8)
    table = torch.empty((F * rows, D), dtype=BF, device=dev)
    for f in range(F):
        s = slice(f * rows, (f + 1) * rows)
        pick = torch.randint(0, 254, (rows, D), device=dev, generator=g)
        codes[s] = finite.to(dev)[pick]
        table[s] = value[pick] * torch.exp2(exps[s].float()).to(BF)[:, None]  # a power of two: exact
        del pick
    return codes, exps, table


def step_fp8(tables, B, F, D, rows, dist, dev, window_us, rounds):
    """``--tables fp8``: the 8-bit step against the bf16 step (interact.hip, unchanged) on the dequantised table and
    the same ids, alternated; each one's share of its own read-the-rows-once roof."""
    codes, exps, table = tables
    g = torch.Generator(device=dev).manual_seed(B + D)
    if dist == "zipf":
        u = torch.rand((B, F), device=dev, generator=g).double()
        ids = ((1.0 - u) ** (-1.0 / 0.05) - 1.0).clamp(0, rows - 1).to(torch.int32)
    else:
        ids = torch.randint(0, rows, (B, F), device=dev, generator=g, dtype=torch.int32)
    dense = torch.randn((B, D), device=dev, generator=g).to(BF)
    M = F + 1
    pairs = [(i, j) for i in range(M) for j in range(i)]
    wlog = D + len(pairs)
    wout = -(-wlog // 8) * 8
    meta = torch.tensor([(0, -1, 0)] + [(f * rows, f, rows) for f in range(F)], dtype=torch.int64).t().contiguous().to(dev)
    lut = K.dot_interact_lut(M, pairs, D).to(dev)
    outs = {k: torch.empty((B, wout), dtype=BF, device=dev) for k in ("interact", "interact_fp8")}
    fns = {"interact": lambda: K.dot_interact(table, ids, meta, lut, wlog, dense, True, out=outs["interact"]),
           "interact_fp8": lambda: K.dot_interact(codes, ids, meta, lut, wlog, dense, True, out=outs["interact_fp8"], table_exp=exps)}
    shape = f"B{B}xF{F}xD{D}:{dist}"
    t = alternate(fns, window_us, rounds)
    same = torch.equal(outs["interact"].view(torch.int16), outs["interact_fp8"].view(torch.int16))
    rest = D * 2 + wout * 2 + 4 * F
    roofs = {"interact": B * (F * D * 2 + rest) / COPY_BYTES_PER_US, "interact_fp8": B * (F * (D + 1) + rest) / COPY_BYTES_PER_US}
    for name, ts in t.items():
        line(shape, name, ts, roof_us=round(roofs[name], 2), share_of_roof=round(roofs[name] / statistics.median(ts), 3))
    print(json.dumps({"shape": shape, "fp8_over_bf16_time": round(statistics.median(t["interact_fp8"]) / statistics.median(t["interact"]), 3),
                      "same_bits": same}), flush=True)


def model(rows, dev, window_us, rounds):
    from flink_tensorflow_amd.graph.compiler import CompiledFunction
    from flink_tensorflow_amd.models.core import GraphDefGraphLoader
    from flink_tensorflow_amd.models.zoo import dlrm_graph_def

    g = GraphDefGraphLoader(dlrm_graph_def(vocab_sizes=(rows,) * 26)).load()
    for B in (256, 2048):
        feeds = {"dense:0": ((B, 16), "FLOAT"), "ids:0": ((B, 26), "INT32")}
        fed = {"dense:0": torch.randn((B, 16), device=dev),
               "ids:0": torch.randint(0, rows, (B, 26), device=dev, dtype=torch.int32)}
        plans = {"strict": CompiledFunction(g, feeds, ["probability:0"], dev, strict=True)}
        try:
            plans["separate"] = CompiledFunction(g, feeds, ["probability:0", "interaction/stack:0"], dev)
        except Exception as e:  # the glue path may not capture
            print(json.dumps({"shape": f"dlrm:B{B}", "impl": "separate", "error": str(e)[:200]}), flush=True)
        for name, p in plans.items():
            print(json.dumps({"shape": f"dlrm:B{B}", "impl": name, "kinds": p.summary()["kinds"], "glue_ops": p.summary()["glue_ops"],
                              "hip_graph": p.summary()["hip_graph"]}), flush=True)
        t = alternate({n: (lambda p=p: p(fed)) for n, p in plans.items()}, window_us, rounds)
        for name, ts in t.items():
            line(f"dlrm:B{B}", name, ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--model-rows", type=int, default=10_000)
    ap.add_argument("--tables", choices=["bf16", "fp8"], default="bf16")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    F = 26
    if a.tables == "fp8":  # the same shapes, 8-bit tables against bf16 tables of the same values
        for F, D, Bs, dists in [(26, 64, (256, 2048, 32768), ("uniform", "zipf")), (26, 128, (256, 2048, 32768), ("uniform", "zipf"))] + \
                ([(26, 80, (32768,), ("uniform",)), (26, 256, (32768,), ("uniform",)), (48, 128, (32768,), ("uniform",)), (48, 256, (32768,), ("uniform",))] if a.wide else []):
            tables = fp8_tables(F, a.rows, D, dev)
            for B in Bs:
                for dist in dists:
                    step_fp8(tables, B, F, D, a.rows, dist, dev, a.window_ms * 1e3, a.rounds)
            del tables
        return
    for D in (64, 128):
        table = torch.empty((F * a.rows, D), dtype=BF, device=dev).normal_()
        for B in (256, 2048, 32768):
            for dist in ("uniform", "zipf"):
                step(table, B, F, D, a.rows, dist, dev, a.window_ms * 1e3, a.rounds)
        del table
    if a.wide:  # the instantiations beyond the Criteo shape: D = 256, and two row groups (M = 49)
        for F, D in ((26, 256), (48, 128), (48, 256)):
            table = torch.empty((F * a.rows, D), dtype=BF, device=dev).normal_()
            step(table, 32768, F, D, a.rows, "uniform", dev, a.window_ms * 1e3, a.rounds)
            del table
    if a.model:
        model(a.model_rows, dev, a.window_ms * 1e3, a.rounds)


if __name__ == "__main__":
    main()
