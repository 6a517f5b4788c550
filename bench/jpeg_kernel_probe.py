#!/usr/bin/env python3
"""The device half of the JPEG decode on its own: ``jpeg_idct_rgb`` over one micro-batch of
coefficient rows (B images of hw x hw, 4:2:0, quality 90, entropy-decoded on the host
first), and the preprocess kernel that reads its output (``preprocess_s2d_rows``), timed
with events and laid out for a kernel trace of this process.  Prints one JSON line with the
kernel's time against the bytes it must move (coefficients + headers in, RGB out).

    python bench/jpeg_kernel_probe.py [--batch 256] [--hw 256] [--iters 50]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bench"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hw", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()

    import numpy as np
    import torch
    from jpeg_e2e import make_jpegs

    from flink_tensorflow_amd import _ext
    from flink_tensorflow_amd.ops import kernels as K

    nat = _ext.native()
    B, hw = a.batch, a.hw
    with tempfile.TemporaryDirectory(prefix="ftm-jpeg-") as d:
        make_jpegs(d, 64, hw)
        files = [open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))]
    blobs = (files * (B // len(files) + 1))[:B]
    stride, hbytes = nat.jpeg_coeff_layout(hw, hw, 420)
    coef = torch.empty((B, stride), dtype=torch.uint8).pin_memory()
    hdrs = torch.empty((B, hbytes), dtype=torch.uint8).pin_memory()
    st = nat.jpeg_entropy_into(coef.data_ptr(), coef.numel(), hdrs.data_ptr(), hdrs.numel(), blobs, stride, hw, hw, 16)
    assert not any(st), st
    ref = np.empty((B, hw, hw, 3), np.uint8)
    nat.jpeg_decode_into(ref.ctypes.data, ref.nbytes, blobs, hw * hw * 3, hw, hw, 16)

    dev = torch.device("cuda", 0)
    dcoef, dhdr = coef.to(dev), hdrs.to(dev)
    out = torch.empty((B, hw, hw, 3), dtype=torch.uint8, device=dev)
    pre = K.preprocess_images(out, out_hw=(hw, hw), s2d=True)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters * 1e3  # us

    idct_us = timed(lambda: K.jpeg_idct_rgb(dcoef, dhdr, out, B, hw, hw))
    pre_us = timed(lambda: K.preprocess_images(out, out_hw=(hw, hw), s2d=True, out=pre))
    got = out.cpu().numpy()
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    used = int(hdrs.view(torch.int32).view(B, -1)[0, 2:17].view(3, 5)[:, 2:4].prod(1).sum()) * 128  # bw * bh * 64 * 2
    moved = B * (used + hbytes + hw * hw * 3)
    print(json.dumps({
        "bench": "jpeg_kernel_probe", "batch": B, "hw": hw, "iters": a.iters,
        "jpeg_idct_rgb_us": round(idct_us, 1), "preprocess_s2d_rows_us": round(pre_us, 1),
        "coef_bytes_per_image": used, "header_bytes_per_image": hbytes, "rgb_bytes_per_image": hw * hw * 3,
        "bytes_moved": moved, "achieved_GBps": round(moved / idct_us / 1e3, 1),
        "max_abs_diff_vs_host_RGB": [int(d[..., c].max()) for c in range(3)]}), flush=True)


if __name__ == "__main__":
    main()
