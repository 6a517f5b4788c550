"""The split JPEG decode on the host: ``jpeg_entropy_into`` (Huffman only -> quantised
coefficient rows + headers) followed by ``jpeg_coeffs_to_rgb`` (the scalar back half that
the device kernel mirrors) against the existing ``jpeg_decode_into``.

The bounds are derived from the arithmetic, not tuned: the IDCT performs the host decoder's
operations one for one (grayscale bit-identical), the upsampling is integer on both sides,
and the 16.16 colour formula agrees with the host's Q15 AVX2 path on R and B for every
(Y, Cb, Cr) and on G within one count; where the host takes its scalar colour loop
(``x >= 16 * (W // 16)``) G is identical too."""
import io

import numpy as np
import pytest

from flink_tensorflow_amd import _ext

K_SLOT = 5  # "the host decoder takes it, this row does not"


def _img(h, w, seed, noise=False):
    from PIL import Image

    rng = np.random.default_rng(seed)
    if noise:  # every coefficient large: the IDCT and colour clamps fire
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    low = rng.integers(0, 256, (max(2, h // 16), max(2, w // 16), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(low).resize((w, h), Image.BICUBIC), np.float32)
    return np.clip(a + rng.normal(0, 12, a.shape), 0, 255).astype(np.uint8)


def _jpeg(a, **kw):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def blobs_for(h, w, gray=False, **kw):
    """Three seeded images and one of pure noise at quality 100, all with ``kw``."""
    pick = (lambda a: a[..., 0]) if gray else (lambda a: a)
    out = [_jpeg(pick(_img(h, w, s)), **kw) for s in range(3)]
    out.append(_jpeg(pick(_img(h, w, 9, noise=True)), **{**kw, "quality": 100}))
    return out


# (name, H, W, gray, Pillow options): the shapes of the issue
CASES = [
    ("gray-8x8", 8, 8, True, dict(quality=90)),                                  # single block
    ("gray-23x17", 17, 23, True, dict(quality=90)),                              # ragged edges
    ("444-13x15", 15, 13, False, dict(quality=90, subsampling=0)),               # host fully scalar: all exact
    ("420-15x33", 33, 15, False, dict(quality=90, subsampling=2)),               # W < 16, vertical filter across MCU rows
    ("420-40x48", 48, 40, False, dict(quality=90, subsampling=2)),               # horizontal filter across an MCU boundary
    ("422-40x24", 24, 40, False, dict(quality=90, subsampling=1)),
    ("420-restart", 48, 40, False, dict(quality=90, subsampling=2, restart_marker_blocks=3)),
    ("420-q50", 48, 40, False, dict(quality=50, subsampling=2)),
    ("420-q100", 48, 40, False, dict(quality=100, subsampling=2)),
]


def host_decode(blobs, h, w, threads=4):
    out = np.zeros((len(blobs), h, w, 3), np.uint8)
    st = _ext.native().jpeg_decode_into(out.ctypes.data, out.nbytes, list(blobs), h * w * 3, h, w, threads)
    return out, st


def _aligned(shape_rows, row_bytes, guard=0, fill=0):
    """``[rows, row_bytes]`` uint8 view at a 64-byte aligned address, followed by ``guard`` bytes."""
    raw = np.full(shape_rows * row_bytes + guard + 64, fill, np.uint8)
    off = (-raw.ctypes.data) % 64
    flat = raw[off:off + shape_rows * row_bytes + guard]
    return flat[:shape_rows * row_bytes].reshape(shape_rows, row_bytes), flat[shape_rows * row_bytes:]


def entropy(blobs, h, w, max_sampling=444, threads=4, start=False, fill=0, guard=0):
    """(coefficient rows, headers, statuses, guard bytes) of ``jpeg_entropy_into`` / ``_start``."""
    nat = _ext.native()
    stride, hbytes = nat.jpeg_coeff_layout(h, w, max_sampling)
    coef, g = _aligned(len(blobs), stride, guard, fill)
    hdr, _ = _aligned(len(blobs), hbytes)
    args = (coef.ctypes.data, coef.size, hdr.ctypes.data, hdr.size, list(blobs), stride, h, w, threads)
    st = nat.jpeg_entropy_start(*args).wait() if start else nat.jpeg_entropy_into(*args)
    return coef, hdr, st, g


def split_decode(blobs, h, w, max_sampling=444, sentinel=7):
    nat = _ext.native()
    coef, hdr, st, _ = entropy(blobs, h, w, max_sampling)
    out = np.full((len(blobs), h, w, 3), sentinel, np.uint8)
    st2 = nat.jpeg_coeffs_to_rgb(coef.ctypes.data, coef.size, hdr.ctypes.data, hdr.size, out.ctypes.data, out.nbytes,
                                 len(blobs), coef.shape[1], h * w * 3, h, w, 4)
    assert st2 == st
    return out, st


def check_bounds(got, ref, w, gray):
    """The derived bounds of ``got`` (split decode) against ``ref`` (``jpeg_decode_into``)."""
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    print("max |diff| R G B:", d[..., 0].max(), d[..., 1].max(), d[..., 2].max())
    if gray:
        assert np.array_equal(got, ref)
        return
    assert d[..., 0].max() == 0 and d[..., 2].max() == 0, "R / B differ: an operation-order bug"
    assert d[..., 1].max() <= 1, "G more than one count off the host's Q15 path"
    x0 = 16 * (w // 16)  # from here on the host converts colour in its scalar 16.16 loop
    assert d[:, :, x0:, 1].max(initial=0) == 0


@pytest.mark.parametrize("name,h,w,gray,kw", CASES, ids=[c[0] for c in CASES])
def test_split_decode_matches_host_decoder(name, h, w, gray, kw):
    blobs = blobs_for(h, w, gray, **kw)
    if "restart" in name:
        assert blobs[0].count(b"\xff\xd0") >= 1
    ref, st0 = host_decode(blobs, h, w)
    got, st = split_decode(blobs, h, w)
    assert st0 == st == [0] * len(blobs)
    check_bounds(got, ref, w, gray)
    if w < 16 and not gray:  # the host is scalar everywhere: all three channels exact
        assert np.array_equal(got, ref)


def test_noise_image_fires_the_clamps():
    """The quality-100 noise image really reaches 0 and 255, so the clamps are covered."""
    ref, _ = host_decode(blobs_for(48, 40, subsampling=2, quality=90)[3:], 48, 40)
    assert ref.min() == 0 and ref.max() == 255


def test_statuses_and_declined_rows_stay_in_bounds():
    a = _img(64, 64, 1)
    prog = _jpeg(a, quality=90, progressive=True)
    other = _jpeg(_img(32, 64, 2), quality=90)
    ok420 = _jpeg(a, quality=90, subsampling=2)
    full = _jpeg(a, quality=90, subsampling=0)  # 4:4:4: 3 samples per pixel, the row holds 1.5
    blobs = [prog, other, b"not a jpeg at all", ok420, full]
    coef, hdr, st, guard = entropy(blobs, 64, 64, max_sampling=420, fill=0xA5, guard=4096)
    assert st == [2, 4, 1, 0, K_SLOT]
    assert hdr.view(np.int32)[:, 0].tolist() == st  # the header carries the status to the device
    assert (guard == 0xA5).all(), "a declined image wrote past the coefficient rows"
    assert (coef[4] == 0xA5).all(), "the declined 4:4:4 image touched its row"
    assert (coef[:3] == 0xA5).all()
    # the same file in a row sized for it is taken, and the 4:2:2 capacity sits in between
    assert entropy([full], 64, 64, max_sampling=444)[2] == [0]
    assert entropy([full], 64, 64, max_sampling=422)[2] == [K_SLOT]
    assert entropy([_jpeg(a, quality=90, subsampling=1)], 64, 64, max_sampling=422)[2] == [0]
    # declined rows are left alone by the back half
    out, st2 = split_decode(blobs, 64, 64, max_sampling=420, sentinel=0x3C)
    assert st2 == st and (out[[0, 1, 2, 4]] == 0x3C).all()
    ref, _ = host_decode([ok420], 64, 64)
    check_bounds(out[3:4], ref, 64, False)


@pytest.mark.parametrize("h,w,sub,ms", [(48, 40, 2, 420), (33, 15, 2, 420), (24, 40, 1, 422), (15, 13, 0, 444),
                                        (17, 23, None, 420)])
def test_coeff_layout_agrees_with_the_bytes_written(h, w, sub, ms):
    """The row stride holds every block the decoder writes, the header names exactly those
    blocks, and nothing outside them is written."""
    nat = _ext.native()
    stride, hbytes = nat.jpeg_coeff_layout(h, w, ms)
    assert stride % 16 == 0 and hbytes == 512
    a = _img(h, w, 9, noise=True)
    blob = _jpeg(a[..., 0] if sub is None else a, quality=100, **({} if sub is None else {"subsampling": sub}))
    rows = []
    for fill in (0x00, 0xFF):
        coef, hdr, st, guard = entropy([blob], h, w, ms, fill=fill, guard=256)
        assert st == [0] and (guard == fill).all()
        rows.append(coef[0].copy())
    written = rows[0] == rows[1]  # bytes that do not depend on what the row held before
    hd = hdr[0].view(np.int32)
    ncomp = int(hd[1])
    assert ncomp == (1 if sub is None else 3)
    comps = hd[2:2 + 5 * ncomp].reshape(ncomp, 5)  # h, v, bw, bh, offset
    end = 0
    for ch, cv, bw, bh, off in comps.tolist():
        assert off == end  # planes follow one another
        end = off + bw * bh * 64
    hm, vm = comps[0, 0], comps[0, 1]
    assert (comps[:, 2] == -(-w // (8 * hm)) * comps[:, 0]).all() and (comps[:, 3] == -(-h // (8 * vm)) * comps[:, 1]).all()
    assert end * 2 <= stride
    assert written[:end * 2].all(), "every block is written in full"
    assert not written[end * 2:].any(), "bytes past the last plane were written"
    qt = hdr[0, 8 + 60:8 + 60 + 384].view(np.uint16).reshape(3, 64)
    assert (qt[:ncomp] == 1).all()  # quality 100: Pillow writes all-ones tables


def test_background_job_and_thread_count_give_identical_rows():
    blobs = [_jpeg(_img(64, 80, s), quality=85) for s in range(24)]
    blobs[5] = _jpeg(_img(64, 80, 5), quality=85, progressive=True)
    c1, h1, s1, _ = entropy(blobs, 64, 80, 420, threads=1)
    c16, h16, s16, _ = entropy(blobs, 64, 80, 420, threads=16)
    cb, hb, sb, _ = entropy(blobs, 64, 80, 420, threads=4, start=True)
    assert s1 == s16 == sb and s1[5] == 2 and sum(s1) == 2
    ok = [i for i in range(len(blobs)) if i != 5]
    assert np.array_equal(c1[ok], c16[ok]) and np.array_equal(h1, h16)
    assert np.array_equal(c1[ok], cb[ok]) and np.array_equal(h1, hb)


def test_cpu_launcher_runs_the_host_back_half():
    """``K.jpeg_idct_rgb`` on host tensors is the CPU implementation of the device path."""
    import torch

    from flink_tensorflow_amd.ops import kernels as K

    blobs = blobs_for(48, 40, subsampling=2, quality=90)
    coef, hdr, st, _ = entropy(blobs, 48, 40, 420)
    out = torch.zeros((4, 48, 40, 3), dtype=torch.uint8)
    K.jpeg_idct_rgb(torch.from_numpy(coef), torch.from_numpy(hdr), out, 4, 48, 40)
    ref, _ = host_decode(blobs, 48, 40)
    check_bounds(out.numpy(), ref, 40, False)


def test_engine_config_and_models_take_jpeg_decode():
    from flink_tensorflow_amd.config import EngineConfig
    from flink_tensorflow_amd.models.zoo.image_classifier import InceptionV3Model, ResNet50Model

    assert EngineConfig().jpeg_decode == "host"
    assert EngineConfig.from_env(environ={"FT_JPEG_DECODE": "device"}).jpeg_decode == "device"
    with pytest.raises(ValueError):
        EngineConfig().update({"jpeg_decode": "gpu"})
    assert ResNet50Model(image_hw=(64, 64), jpeg_decode="device").jpeg_decode == "device"
    assert InceptionV3Model().jpeg_decode is None  # the engine's default applies at open()
