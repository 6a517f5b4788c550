"""The audio front end (``kernels/audio.hip``) at B=256 one-second clips, the strict plan of the
zoo keyword spotter, and the same model fed fingerprints computed on the host.

Candidates are alternated round by round in one process (device events around ``--reps``
launches, ``--rounds`` rounds after a warm-up of every candidate; the median and the min..max
spread of the rounds are printed).

``step``: the ``mfcc`` step alone in the workload's configuration (16 kHz, window 480, stride
160, 40 mel channels, 40 coefficients: 98 frames per clip) on noise plus a tone:

* ``i16_pad8``   int16 ``[B, S]`` in, the conv's padded bf16 input out (what the plan runs);
* ``f32_pad8``   fp32 ``[B, S]`` in, the same output;
* ``f32_f32``    fp32 ``[S, B]`` in, fp32 ``[B, F, D]`` out;
* ``spectrogram``  the squared spectrogram alone, fp32 ``[B, F, 257]``.

``--plan``: the hipGraph replay of the strict plan of ``speech_commands_graph_def`` (int16 feed)
and the device time of every step of one eager run (``plan.profile()``), with the first conv's
share of the total.

``--host-frontend``: the same graph compiled from its ``fingerprint`` tensor on (fed fp32 ``[B,
98, 40, 1]``), the fp32 host front end that has to produce that feed (the launcher's host path,
wall clock, torch's thread pool as configured) and the host-to-device copies of both feeds from
pinned memory.

    python bench/audio_probe.py --reps 100 --rounds 7 --plan --host-frontend
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from flink_tensorflow_amd.ops import kernels as K  # noqa: E402

BF = torch.bfloat16
S, RATE, WINDOW, STRIDE, C, D = 16000, 16000, 480, 160, 40, 40


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


def clips(B, seed=0):
    """``[B, S]`` fp32 in [-1, 1): noise of amplitude 0.25 plus one tone per clip."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(S, dtype=torch.float64) / RATE
    f = 200 + 2800 * torch.rand((B, 1), generator=g, dtype=torch.float64)
    x = 0.25 * torch.randn((B, S), generator=g, dtype=torch.float64) + 0.4 * torch.sin(2 * torch.pi * f * t)
    return x.clamp(-1, 32767 / 32768).float()


def step(B, dev, reps, rounds):
    x = clips(B)
    pcm = (x * 32768).round().clamp(-32768, 32767).to(torch.int16).to(dev)
    xf, xs = x.to(dev), x.t().contiguous().to(dev)
    tb = K.mfcc_tables(WINDOW, RATE, 20.0, 4000.0, C, D, device=dev)
    F_ = K.audio_frames(S, WINDOW, STRIDE)
    pad = torch.empty((B, F_, D, 8), dtype=BF, device=dev)
    out32 = torch.empty((B, F_, D), dtype=torch.float32, device=dev)
    spec = torch.empty((B, F_, tb["fft"] // 2 + 1), dtype=torch.float32, device=dev)
    fns = {"i16_pad8": lambda: K.audio_mfcc(pcm.t(), tb, STRIDE, 1 / 32768, out=pad, pad8=True),
           "f32_pad8": lambda: K.audio_mfcc(xf.t(), tb, STRIDE, out=pad, pad8=True),
           "f32_f32": lambda: K.audio_mfcc(xs, tb, STRIDE, out=out32),
           "spectrogram": lambda: K.audio_spectrogram(xf.t(), tb, STRIDE, True, out=spec)}
    t = alternate(fns, reps, rounds)
    shape = f"mfcc_b{B}_s{S}_w{WINDOW}_st{STRIDE}_c{C}_d{D}"
    wgs = B * -(-F_ // K.AUDIO_FRAMES_PER_WG)
    for k, ts in t.items():
        med = statistics.median(ts)
        line(shape, k, ts, frames=B * F_, ns_per_frame=round(med * 1e3 / (B * F_), 1), workgroups=wgs)
    K.audio_mfcc(pcm.t(), tb, STRIDE, 1 / 32768, out=pad, pad8=True)
    a = pad[..., 0].clone()
    K.audio_mfcc(pcm.float().mul(1 / 32768).t(), tb, STRIDE, out=out32)
    print(json.dumps({"shape": shape, "forms_agree_bit_for_bit": bool(torch.equal(a, out32.to(BF)))}), flush=True)


def plans(B, dev, reps, rounds, host_frontend):
    from flink_tensorflow_amd.graph.compiler import CompiledFunction
    from flink_tensorflow_amd.graph.graph import Graph
    from flink_tensorflow_amd.models.zoo.speech import speech_commands_graph_def

    g = Graph.from_graph_def(speech_commands_graph_def(pcm="int16"))
    x = clips(B, seed=1)
    pcm = (x * 32768).round().clamp(-32768, 32767).to(torch.int16)
    fetches = ["probs:0", "top_k:1"]
    strict = CompiledFunction(g, {"clips:0": ((B, S), "INT16")}, fetches, dev, strict=True)
    strict.input_buffer("clips:0").copy_(pcm)
    name = f"speech_commands_b{B}"
    s = strict.summary()
    assert s["hip_graph"] and s["glue_ops"] == []
    print(json.dumps({"plan": name, "hip_graph": True, "steps": s["steps"], "kinds": s["kinds"],
                      "impls": [st.meta.get("impl") for st in strict.steps]}), flush=True)
    fns = {"strict": strict.replay}
    fed = None
    if host_frontend:
        F_ = K.audio_frames(S, WINDOW, STRIDE)
        fed = CompiledFunction(g, {"fingerprint:0": ((B, F_, D, 1), "FLOAT")}, fetches, dev, strict=True)
        tb = K.mfcc_tables(WINDOW, RATE, 20.0, 4000.0, C, D)
        xs = (pcm.float() * (1 / 32768)).t()
        ts = []
        for r in range(4):
            t0 = time.perf_counter()
            fp = K.audio_mfcc(xs, tb, STRIDE)
            if r:  # the first run warms up
                ts.append((time.perf_counter() - t0) * 1e6)
        fed.input_buffer("fingerprint:0").copy_(fp.reshape(B, F_, D, 1))
        sf = fed.summary()
        print(json.dumps({"plan": name + "_fed_fingerprint", "hip_graph": sf["hip_graph"], "steps": sf["steps"],
                          "kinds": sf["kinds"]}), flush=True)
        line(name, "host_frontend:fp32_torch_rfft", ts, threads=torch.get_num_threads())
        fns["fed_fingerprint"] = fed.replay
        pin_fp, pin_pcm = fp.reshape(B, F_, D, 1).contiguous().pin_memory(), pcm.pin_memory()
        copies = {"h2d:fingerprint_fp32": lambda: fed.input_buffer("fingerprint:0").copy_(pin_fp, non_blocking=True),
                  "h2d:pcm_int16": lambda: strict.input_buffer("clips:0").copy_(pin_pcm, non_blocking=True)}
        for k, ts in alternate(copies, reps, rounds).items():
            line(name, k, ts, bytes=(pin_fp if "finger" in k else pin_pcm).numel() * (4 if "finger" in k else 2))
    for k, ts in alternate(fns, reps, rounds).items():
        line(name, "replay:" + k, ts)
    if fed is not None:
        torch.cuda.synchronize()
        a, b = strict.output_tensors()[0].float(), fed.output_tensors()[0].float()
        print(json.dumps({"plan": name, "max_abs_prob_diff_strict_vs_fed": float((a - b).abs().max())}), flush=True)
    for _ in range(3):  # the third eager run: every launch warm
        md = strict.profile()
    per_step = {ns.node_name: ns.op_end_rel_micros for ns in md.step_stats.dev_stats[0].node_stats}
    total = sum(per_step.values())
    print(json.dumps({"plan": name, "profile_us_by_step": per_step, "profile_total_us": total,
                      "first_conv_share": round(per_step.get("conv1/Conv2D", 0) / max(total, 1), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100, help="launches per timed window")
    ap.add_argument("--plan-reps", type=int, default=20, help="replays per timed window of a plan")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--plan", action="store_true")
    ap.add_argument("--host-frontend", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("audio_probe measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    if not a.no_step:
        step(a.batch, dev, a.reps, a.rounds)
    if a.plan or a.host_frontend:
        plans(a.batch, dev, a.plan_reps, a.rounds, a.host_frontend)


if __name__ == "__main__":
    main()
