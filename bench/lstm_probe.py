"""The LSTM recurrence (``kernels/lstm.hip``) at B=256, T=128, the strict plan of the two-layer
zoo classifier, and what running the same model took before the kernel existed.

Candidates are alternated round by round in one process (device events around ``--reps``
launches, ``--rounds`` rounds after a warm-up of every candidate; the median and the min..max
spread of the rounds are printed).

``step``: the ``lstm`` step alone on ``xproj ~ 2 normal``, ``Wh ~ normal / sqrt(H)`` in bf16, zero
initial state, for ``H`` in 64, 128 (resident weights) and 256 (streamed weights):

* ``all``    every ``h_t`` stored, time-major;
* ``last``   only ``h_{T-1}`` stored (what a classifier's last layer does);
* ``bm``     batch-major ``xproj`` and ``h_out`` through strides.

``--plan``: the hipGraph replay of the strict plan of ``lstm_classifier_graph_def`` at I=64,
H=128, two layers, and the device time of every step of one eager run (``plan.profile()``) summed
by kind.

``--unrolled``: the same model written as an unrolled cell of primitive ops (per step two
``MatMul``, last-axis slices, ``Sigmoid``, ``Tanh``, ``Mul``, ``Add``) on time-major input, compiled
non-strict on the same tree and replayed as one hipGraph: ``T x (2 gemm + ~14 elementwise / copy
steps)`` per layer.

``--interpreter``: ``Session.run`` of the classifier graph on the device (the ``BlockLSTM``
interpreter op: one PyTorch op per gate and step); host clock around a synchronised run.

    python bench/lstm_probe.py --reps 200 --rounds 7 --plan --unrolled --interpreter
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from flink_tensorflow_amd.ops import kernels as K  # noqa: E402

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


def line(shape, name, ts, **extra):
    med = statistics.median(ts)
    print(json.dumps({"shape": shape, "impl": name, "us": round(med, 1), "min": round(min(ts), 1),
                      "max": round(max(ts), 1), **extra}), flush=True)


def step(B, T, H, dev, reps, rounds):
    g = torch.Generator(device=dev).manual_seed(H)
    xproj = (2 * torch.randn((T, B, 4 * H), device=dev, generator=g)).to(BF)
    x_bm = xproj.transpose(0, 1).contiguous()
    wh = (torch.randn((H, 4 * H), device=dev, generator=g) / H ** 0.5).to(BF)
    wpk = K.lstm_pack_weights(wh, H)
    h0, c0 = torch.zeros((B, H), dtype=BF, device=dev), torch.zeros((B, H), dtype=torch.float32, device=dev)
    h_all, h_bm = torch.empty((T, B, H), dtype=BF, device=dev), torch.empty((B, T, H), dtype=BF, device=dev)
    h_last = torch.empty((B, H), dtype=BF, device=dev)
    fns = {"all": lambda: K.lstm_seq(xproj, wpk, h0, c0, h_out=h_all),
           "last": lambda: K.lstm_seq(xproj, wpk, h0, c0, h_out=h_last, last_only=True),
           "bm": lambda: K.lstm_seq(x_bm.transpose(0, 1), wpk, h0, c0, h_out=h_bm.transpose(0, 1))}
    t = alternate(fns, reps, rounds)
    shape = f"lstm_b{B}_t{T}_h{H}"
    for k, ts in t.items():
        line(shape, k, ts, impl_kernel=K.lstm_impl(H), us_per_step=round(statistics.median(ts) / T, 3),
             workgroups=-(-B // 16))
    same = torch.equal(h_all[T - 1], h_last) and torch.equal(h_bm.transpose(0, 1), h_all)
    print(json.dumps({"shape": shape, "layouts_agree_bit_for_bit": same}), flush=True)


def unrolled_graph_def(T, B, I, H, layers, classes, seed=0):
    """The classifier's arithmetic from primitive ops on time-major ``sequences_tm [T, B, I]``
    (same seeded weights as ``lstm_classifier_graph_def``; forget bias folded into the bias)."""
    from flink_tensorflow_amd.graph.builder import GraphBuilder

    rng = np.random.default_rng(seed)
    gb = GraphBuilder()
    x = gb.placeholder("sequences_tm", "FLOAT", [T, B, I])
    zeros = gb.constant("zero_state", np.zeros((B, H), dtype=np.float32))
    xs = [gb.strided_slice(x, [t], [0], name=f"x{t}", end_mask=1, shrink_axis_mask=1) for t in range(T)]
    cin = I
    for layer in range(layers):
        with gb.name_scope(f"lstm_{layer}"):
            lim = float(np.sqrt(6.0 / (cin + 5 * H)))  # as lstm_classifier_graph_def draws it
            w = rng.uniform(-lim, lim, (cin + H, 4 * H)).astype(np.float32)
            b = np.zeros((4 * H,), dtype=np.float32)
            b[2 * H:3 * H] += 1.0
            wx, wh, bias = gb.constant("wx", w[:cin]), gb.constant("wh", w[cin:]), gb.constant("bias", b)
            c = h = zeros
            hs = []
            for t in range(T):
                with gb.name_scope(f"t{t}"):
                    g = gb.add(gb.bias_add(gb.matmul(xs[t], wx, name="xw"), bias, name="xwb"),
                               gb.matmul(h, wh, name="hw"), name="gates")
                    gi, gc, gf, go = (gb.last_axis_slice(g, k * H, (k + 1) * H, rank=2, name=n)
                                      for k, n in enumerate(("gi", "gc", "gf", "go")))
                    i, f, ci = gb.sigmoid(gi, name="i"), gb.sigmoid(gf, name="f"), gb.op("Tanh", [gc], name="ci")
                    c = gb.add(gb.mul(ci, i, name="ci_i"), gb.mul(c, f, name="c_f"), name="c")
                    c = gb.op("Minimum", [gb.op("Maximum", [c, gb.constant("lo", np.float32(-3.0))], name="max"),
                                          gb.constant("hi", np.float32(3.0))], name="c_clip")
                    h = gb.mul(gb.op("Tanh", [c], name="co"), gb.sigmoid(go, name="o"), name="h")
                    hs.append(h)
            xs, cin = hs, H
    lim = float(np.sqrt(6.0 / (H + classes)))
    wo = gb.constant("dense/kernel", rng.uniform(-lim, lim, (H, classes)).astype(np.float32))
    bo = gb.constant("dense/bias", rng.uniform(-0.1, 0.1, (classes,)).astype(np.float32))
    probs = gb.softmax(gb.bias_add(gb.matmul(xs[-1], wo, name="dense/MatMul"), bo, name="logits"), name="probs")
    gb.top_k(probs, min(3, classes), name="top_k")
    return gb.build_graph_def()


def plans(B, T, I, H, layers, classes, dev, reps, rounds, unrolled, interpreter, interp_rounds):
    from flink_tensorflow_amd.graph.compiler import CompiledFunction
    from flink_tensorflow_amd.graph.graph import Graph
    from flink_tensorflow_amd.graph.session import Session
    from flink_tensorflow_amd.models.zoo.lstm import lstm_classifier_graph_def

    g = Graph.from_graph_def(lstm_classifier_graph_def(T, I, H, layers, classes, batch=B))
    x = 1.5 * torch.randn((B, T, I), generator=torch.Generator().manual_seed(0))
    strict = CompiledFunction(g, {"sequences:0": ((B, T, I), "FLOAT")}, ["probs:0", "top_k:1"], dev, strict=True)
    strict.input_buffer("sequences:0").copy_(x)
    name = f"lstm_classifier_l{layers}_i{I}_h{H}_t{T}_b{B}"
    s = strict.summary()
    assert s["hip_graph"] and s["glue_ops"] == []
    print(json.dumps({"plan": name, "hip_graph": True, "steps": s["steps"], "kinds": s["kinds"]}), flush=True)
    fns = {"strict": strict.replay}
    loose = None
    if unrolled:
        t0 = time.perf_counter()
        gu = Graph.from_graph_def(unrolled_graph_def(T, B, I, H, layers, classes))
        loose = CompiledFunction(gu, {"sequences_tm:0": ((T, B, I), "FLOAT")}, ["probs:0", "top_k:1"], dev)
        loose.input_buffer("sequences_tm:0").copy_(x.transpose(0, 1))
        su = loose.summary()
        print(json.dumps({"plan": name + "_unrolled", "hip_graph": su["hip_graph"], "steps": su["steps"],
                          "kinds": su["kinds"], "glue_ops": su["glue_ops"],
                          "compile_s": round(time.perf_counter() - t0, 1)}), flush=True)
        fns["unrolled"] = loose.replay
    t = alternate(fns, reps, rounds)
    for k, ts in t.items():
        line(name, "replay:" + k, ts)
    if loose is not None:
        torch.cuda.synchronize()
        a, b = strict.output_tensors()[0].float(), loose.output_tensors()[0].float()
        print(json.dumps({"plan": name, "max_abs_prob_diff_strict_vs_unrolled": float((a - b).abs().max())}), flush=True)
    by_kind: dict = {}
    for _ in range(3):  # the third eager run: every launch warm
        md = strict.profile()
    for ns in md.step_stats.dev_stats[0].node_stats:
        by_kind[ns.timeline_label] = by_kind.get(ns.timeline_label, 0) + ns.op_end_rel_micros
    print(json.dumps({"plan": name, "profile_us_by_kind": by_kind, "profile_total_us": sum(by_kind.values())}), flush=True)
    if interpreter:
        sess = Session(g, device=dev)
        xd = x.to(dev)
        ts = []
        for r in range(interp_rounds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = sess.run(["probs:0"], {"sequences:0": xd})
            torch.cuda.synchronize()
            if r:  # the first run warms up
                ts.append((time.perf_counter() - t0) * 1e6)
        line(name, "interpreter:session_run", ts,
             max_abs_prob_diff_vs_strict=float((torch.as_tensor(out[0]).float() - strict.output_tensors()[0].float()).abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="launches per timed window")
    ap.add_argument("--plan-reps", type=int, default=20, help="replays per timed window of a plan")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--plan", action="store_true")
    ap.add_argument("--unrolled", action="store_true")
    ap.add_argument("--interpreter", action="store_true")
    ap.add_argument("--interpreter-rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lstm_probe measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    if not a.no_step:
        for H in (64, 128, 256):
            step(a.batch, a.steps, H, dev, a.reps, a.rounds)
    if a.plan or a.unrolled or a.interpreter:
        plans(a.batch, a.steps, a.features, a.hidden, 2, 10, dev, a.plan_reps, a.rounds, a.unrolled, a.interpreter,
              a.interpreter_rounds)


if __name__ == "__main__":
    main()
