"""The device half of the JPEG decode (``kernels/jpeg.hip`` ``jpeg_idct_rgb``: dequantise,
IDCT, upsample, colour-convert the host's entropy-decoded coefficient rows) against the
existing host decoder ``jpeg_decode_into``, with the derived bounds of
``test_jpeg_coeffs.py`` (grayscale and R / B bit-identical, G within one count and identical
where the host converts colour in scalar code), and the runner's ``jpeg_decode="device"``."""
import functools

import numpy as np
import pytest

from test_jpeg_coeffs import CASES, _img, _jpeg, blobs_for, check_bounds, entropy, host_decode

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


def device_decode(blobs, h, w, max_sampling=444):
    """All of ``blobs`` in ONE launch -> ([n, h, w, 3] uint8 with the sentinel where the
    kernel did not write, statuses)."""
    import torch

    from flink_tensorflow_amd.ops import kernels as K

    coef, hdr, st, _ = entropy(blobs, h, w, max_sampling)
    dev = torch.device("cuda", 0)
    # the output sits inside a larger buffer: the bytes around it must come back untouched
    n, row = len(blobs), h * w * 3
    buf = torch.full((4096 + n * row + 4096,), SENTINEL, dtype=torch.uint8, device=dev)
    out = buf[4096:4096 + n * row].view(n, h, w, 3)
    K.jpeg_idct_rgb(torch.from_numpy(coef).to(dev), torch.from_numpy(hdr).to(dev), out, n, h, w)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:4096] == SENTINEL).all() and (host[-4096:] == SENTINEL).all(), "wrote outside the rows"
    return host[4096:-4096].reshape(n, h, w, 3), st


def _size_classes():
    """The issue's shapes grouped by image size, every group decoded in one launch so that
    a wrong per-image offset shows; plus multi-tile sizes (several 128 x 32 tiles each way,
    an odd width so that rows start at every byte alignment) with the samplings mixed."""
    groups = {}
    for name, h, w, gray, kw in CASES:
        groups.setdefault((h, w), []).append((name, gray, kw))
    groups[(70, 299)] = [("420", False, dict(quality=90, subsampling=2)), ("gray", True, dict(quality=90)),
                         ("422", False, dict(quality=75, subsampling=1)),
                         ("444", False, dict(quality=95, subsampling=0))]
    groups[(256, 256)] = [("420", False, dict(quality=90, subsampling=2))]
    return groups


GROUPS = _size_classes()


@functools.lru_cache(maxsize=None)
def _group(hw):
    h, w = hw
    blobs, gray = [], []
    for _, g, kw in GROUPS[hw]:
        b = blobs_for(h, w, g, **kw)
        blobs += b
        gray += [g] * len(b)
    ref, st = host_decode(blobs, h, w)
    assert st == [0] * len(blobs)
    ref.setflags(write=False)
    return blobs, gray, ref


@pytest.mark.parametrize("hw", list(GROUPS), ids=[f"{h}x{w}" for h, w in GROUPS])
def test_kernel_matches_host_decoder(hw):
    h, w = hw
    blobs, gray, ref = _group(hw)
    got, st = device_decode(blobs, h, w)
    assert st == [0] * len(blobs)
    for i, g in enumerate(gray):
        check_bounds(got[i:i + 1], ref[i:i + 1], w, g)
        if w < 16:  # the host is scalar everywhere: all three channels exact
            assert np.array_equal(got[i], ref[i])


def test_kernel_skips_images_with_a_status():
    """Five images, image 2 declined by the entropy decoder: its row keeps the sentinel, the
    other four are decoded (exact: W < 16 puts the host on its scalar colour path)."""
    h, w = 33, 15
    blobs = [_jpeg(_img(h, w, s), quality=90, subsampling=2) for s in range(5)]
    blobs[2] = _jpeg(_img(h, w, 2), quality=90, progressive=True)
    got, st = device_decode(blobs, h, w, 420)
    assert st == [0, 0, 2, 0, 0]
    assert (got[2] == SENTINEL).all()
    keep = [0, 1, 3, 4]
    ref, _ = host_decode([blobs[i] for i in keep], h, w)
    assert np.array_equal(got[keep], ref)


def _runner_records():
    """Twelve 64 x 64 records: mostly 4:2:0, one gray, one 4:4:4 (too many samples for the
    slot's rows: host decoder), one progressive (Pillow)."""
    blobs = [_jpeg(_img(64, 64, s), quality=90) for s in range(12)]
    blobs[3] = _jpeg(_img(64, 64, 3)[..., 0], quality=90)
    blobs[7] = _jpeg(_img(64, 64, 7), quality=90, subsampling=0)
    blobs[10] = _jpeg(_img(64, 64, 10), quality=90, progressive=True)
    return blobs, {7, 10}, {3}


@functools.lru_cache(maxsize=None)
def _host_mode_labels():
    """Top-1 labels of the runner records in the default host mode."""
    return _run_model("host", True)[0]


def _run_model(mode, async_decode):
    import torch

    from flink_tensorflow_amd.models.zoo.image_classifier import ResNet50Model

    blobs, _, _ = _runner_records()
    m = ResNet50Model(image_hw=(64, 64), buckets=(8,), depth_layers=26, lanes=1, jpeg_decode=mode)
    m.open()
    try:
        r = m._runner
        assert r.jpeg_decode == mode
        r.async_decode = async_decode
        r.stage_chunk = 4  # a 6-record batch is two pieces
        labels, staged, done = [], [], []
        for lo in range(0, len(blobs), 6):  # 6-record batches (bucket 8: padded)
            chunk = [(f"f{i}.jpg", b) for i, b in enumerate(blobs[lo:lo + 6], lo)]
            done += m.submit(chunk, np.zeros(6), list(range(lo, lo + 6)))
        done += m.drain()
        torch.cuda.synchronize()
        for res, _, _ in done:
            labels += [x[0][1] for x in res]
        assert len(r.slots[8]) >= 2  # batch k was staged in ring slot k, still untouched
        for slot in r.slots[8][:2]:
            staged.append(slot.dev_in[:6].cpu().numpy())
            assert (slot.dev_in[6:] == 0).all()  # padding rows
        coef_bufs = [s.pinned_coef is not None for s in r.slots[8]]
        return labels, np.concatenate(staged), r.decode_fallbacks, coef_bufs
    finally:
        m.close()


@pytest.mark.parametrize("async_decode", [True, False])
def test_runner_decodes_on_the_device(async_decode):
    from flink_tensorflow_amd.graph.ops_io import decode_jpegs

    blobs, declined, gray = _runner_records()
    labels, staged, fallbacks, coef_bufs = _run_model("device", async_decode)
    ref = decode_jpegs(blobs, 64, 64)
    for i in range(len(blobs)):
        if i in declined:
            assert np.array_equal(staged[i], ref[i]), f"declined record {i} is not the host decoder's row"
        else:
            check_bounds(staged[i:i + 1], ref[i:i + 1], 64, i in gray)
    assert fallbacks == 2
    assert any(coef_bufs)
    assert len(labels) == len(blobs) and labels == _host_mode_labels()


def test_host_mode_allocates_no_coefficient_buffers():
    labels, staged, fallbacks, coef_bufs = _run_model("host", False)
    assert not any(coef_bufs)
    assert fallbacks == 1  # the progressive file, as before
    from flink_tensorflow_amd.graph.ops_io import decode_jpegs

    assert np.array_equal(staged, decode_jpegs(_runner_records()[0], 64, 64))
