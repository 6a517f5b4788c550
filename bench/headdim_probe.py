"""Attention at head dims 32 / 64 / 128 and equal total width ``H * Dh`` (default 768): the encoder
step (``K.attention``) and the causal step (``causal=True``) per width against each other and
against torch SDPA on the same tensors.

At equal ``H * Dh`` the three widths move the same bytes and run the same MFMA work (``S = Q K^T``
and ``O = P V`` are ``2 * S * S * H * Dh`` flops each), so the 64-wide kernel is the yardstick of the
other two.  Candidates are alternated round by round in one process (``retrieval_probe.alternate``:
device events around ``reps`` launches, ``--rounds`` rounds after a warm-up of every candidate); the
median and the min..max spread of the rounds are printed, and per shape one summary line with each
width's time over the 64-wide kernel's (ratio of medians and its range over the rounds) and the
SDPA time over ours.  ``randn`` bf16 QKV, no padding, ``B = tokens // S``.

``--resources`` first compiles the two kernel files with ``-Rpass-analysis=kernel-resource-usage``
(the project's flags) and prints registers, scratch, LDS and occupancy of every attention kernel.

    python bench/headdim_probe.py --rounds 5 --resources
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from retrieval_probe import alternate, line  # noqa: E402  (the script's directory is on the path)
from flink_tensorflow_amd import _build  # noqa: E402
from flink_tensorflow_amd.ops import kernels as K  # noqa: E402

BF = torch.bfloat16


def resources():
    hipcc = os.environ.get("HIPCC", f"{_build.ROCM}/bin/hipcc")
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("attention.hip", "attention_causal.hip"):
            cmd = [hipcc, *_build.hip_flags(), *_build.HIP_FILE_FLAGS.get(name, []), *_build._pybind_includes(),
                   "-Rpass-analysis=kernel-resource-usage", "-c", str(_build.KERNELS / name), "-o", f"{tmp}/o.o"]
            err = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, check=True).stderr
            cur = None
            for ln in err.splitlines():
                m = re.search(r"remark: Function Name: (\S+)", ln)
                if m:
                    k = re.search(r"\d+([a-z_]+_kernel)((?:ILi\d+E(?:Li\d+E)*E)?)", m.group(1))  # name<ints>, mangled
                    args = re.findall(r"Li(\d+)E", k.group(2)) if k else []
                    cur = {"kernel": (k.group(1) + (f"<{', '.join(args)}>" if args else "")) if k else m.group(1)}
                    continue
                m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", ln)
                if m and cur is not None and m.group(1) in keys:
                    cur[keys[m.group(1)]] = int(m.group(2))
                    if m.group(1).startswith("LDS") and "attention" in cur["kernel"]:
                        print(json.dumps({"resources": cur}), flush=True)


def step(S, causal, width, tokens, dev, window_us, rounds):
    B = max(1, tokens // S)
    sdpa = torch.nn.functional.scaled_dot_product_attention
    ids = torch.ones(B * S, dtype=torch.int32, device=dev)
    fns, outs, views = {}, {}, {}
    for D in K.ATTENTION_HEAD_DIMS:
        H = width // D
        qkv = torch.randn((B * S, 3 * H * D), device=dev, generator=torch.Generator(device=dev).manual_seed(S)).to(BF)
        outs[D] = torch.empty((B * S, H * D), dtype=BF, device=dev)
        views[D] = qkv.view(B, S, 3, H, D).permute(2, 0, 3, 1, 4)  # [B, H, S, D] views, as SDPA takes them
        fns[f"d{D}"] = lambda qkv=qkv, H=H, D=D: K.attention(qkv, ids, B, S, H, out=outs[D], causal=causal)
        fns[f"sdpa_d{D}"] = lambda D=D: sdpa(*views[D], is_causal=causal)
    t, reps = alternate(fns, window_us, rounds)
    shape = f"{'causal' if causal else 'encoder'}_s{S}_w{width}_b{B}"
    for name, ts in t.items():
        line(shape, name, ts, reps=reps[name])
    summary = {"shape": shape, "tokens": B * S}
    for D in K.ATTENTION_HEAD_DIMS:
        for name, num, den in ((f"d{D}_over_d64", f"d{D}", "d64"), (f"sdpa_over_d{D}", f"sdpa_d{D}", f"d{D}")):
            if num != den:
                r = [a / b for a, b in zip(t[num], t[den])]
                summary[name] = [round(statistics.median(t[num]) / statistics.median(t[den]), 3),
                                 round(min(r), 3), round(max(r), 3)]
        fns[f"d{D}"]()
        nb = min(B, max(1, 4096 // S))  # fp32 reference on the first sequences
        ref = sdpa(*(x[:nb].float() for x in views[D]), is_causal=causal).permute(0, 2, 1, 3).reshape(nb * S, -1)
        summary[f"d{D}_max_abs_diff_fp32"] = round(float((outs[D][:nb * S].float() - ref).abs().max()), 5)
    print(json.dumps(summary), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0, help="device work per timed window")
    ap.add_argument("--seqs", type=int, nargs="+", default=[64, 128, 512])
    ap.add_argument("--width", type=int, default=768, help="H * Dh, a multiple of 128")
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("headdim_probe measures on the GPU; none found")
    if a.resources:
        resources()
    dev = torch.device("cuda", 0)
    for causal in (False, True):
        for S in a.seqs:
            step(S, causal, a.width, a.tokens, dev, a.window_ms * 1e3, a.rounds)


if __name__ == "__main__":
    main()
