"""The stage-1 tail and chain kernels next to another stream's kernel, bit for bit.

``tests/test_persistent_kernels.py`` runs every tail and chain variant alone on the device.
In the two-lane plan they run beside the sibling lane's kernels, and that is the one
condition under which the chain kernel has raced before: a co-resident workgroup of another
stream delayed the LDS queue, and a wave read the y1 staging tile before a sibling wave's
write had landed (the comment at the top of the tile loop in ``bottleneck_chain.hip``).

Each case here takes the exact-integer data and float64 reference of
``test_persistent_kernels`` (7 tiles of 64 pixels, the last partial; the decimated case 3),
runs the kernel once on an idle device, then 16 times back to back on one stream into 16
separate sentinel-filled buffers while a second stream loops a ``conv_lite`` 3x3 convolution
of (8, 64, 64, 64) -> 128 channels (256 workgroups of 64 KiB LDS: enough to sit on every CU
beside a tail).  The second stream starts first and is fed until the first stream has
drained.  Every one of the 16 results must equal the idle result and the reference exactly,
guard rows included.  With 3 workgroups every workgroup walks 2 to 3 tiles (the loop's back
edge); with the device's CU count every workgroup runs one.

This is a screen, not a proof: whether a conv workgroup lands on a tail's CU in the window
that matters is up to the dispatcher, and a pass does not show that no interleaving fails."""
import functools

import pytest
import torch

from flink_tensorflow_amd.ops import kernels as K
from test_persistent_kernels import (BF, DEV, TAIL_VARIANTS, _assert_bits, _dec_rows, _g, _grid, _grid_id, _guarded,
                                     _pixels, chain_case, tail_case)

RUNS = 16        # launches on stream A
LEAD = 32        # sibling convs queued on stream B before A's first launch
MAX_FEED = 4096  # bound of the loop that feeds B until A has drained
M7 = 6 * 64 + 37


@functools.lru_cache(maxsize=None)
def _sibling_conv():
    """The sibling lane's stand-in: one planned 3x3 conv and its operands, launched on the
    current stream by the returned function."""
    plan = K.ConvPP([((8, 64, 64, 64), (3, 3), (1, 1), (1, 1), (1, 1))], 128, (64, 64), DEV)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 64, 64, 64, generator=g).to(DEV, BF)
    w = (torch.randn(128, plan.K, generator=g) * 0.05).to(DEV, BF)
    out = torch.empty(8, 64, 64, 128, dtype=BF, device=DEV)
    return lambda: plan([x], w, None, None, "relu", out=out)


def _beside_sibling(launch, make_bufs, check):
    """``launch(bufs)`` enqueues the kernel under test on the current stream; ``check(bufs, what)``
    compares one run's buffers with the reference and the guard rows with the sentinel."""
    conv = _sibling_conv()
    idle = make_bufs()
    launch(idle)
    torch.cuda.synchronize()
    check(idle, "idle")
    runs = [make_bufs() for _ in range(RUNS)]
    sa, sb = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    drained = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(sb):  # B first
        for _ in range(LEAD):
            conv()
    for bufs in runs:
        with torch.cuda.stream(sa):
            launch(bufs)
        with torch.cuda.stream(sb):
            conv()
    with torch.cuda.stream(sa):
        drained.record()
    fed = 0
    with torch.cuda.stream(sb):  # B is fed until A's last launch has run
        while not drained.query() and fed < MAX_FEED:
            conv()
            fed += 1
    torch.cuda.synchronize()
    for i, bufs in enumerate(runs):
        check(bufs, f"run {i} beside the sibling stream")
        for got, want in zip(bufs, idle):
            assert torch.equal(got, want), f"run {i} beside the sibling stream differs from the idle run"


@pytest.mark.gpu
@pytest.mark.parametrize("num_cu", [3, None], ids=_grid_id)
@pytest.mark.parametrize("variant", ["cn128-res", "cn64-res", "cn64-dual"])
def test_tail_beside_a_sibling_stream(monkeypatch, variant, num_cu):
    num_cu = _grid(monkeypatch, num_cu)
    cn, dual, tp = TAIL_VARIANTS[variant]
    M = M7
    d, (y3, y1, _) = tail_case(variant, M)
    x2, second = _g(d["x2"]), _g(d["second"])
    w3, b3, w1, b1 = _g(d["w3"]), _g(d["b3"], torch.float32), _g(d["w1"]), _g(d["b1"], torch.float32)
    wgs = min(-(-M // tp), num_cu)

    def launch(bufs):
        K.bottleneck_tail(x2, None if dual else second, w3, b3, w1, b1, y3=bufs[0][:M], y1=bufs[1][:M],
                          xs=second if dual else None)

    def check(bufs, what):
        _assert_bits(f"tail {variant} y3, {what}", bufs[0], y3, tp, wgs)
        _assert_bits(f"tail {variant} y1, {what}", bufs[1], y1, tp, wgs)

    _beside_sibling(launch, lambda: (_guarded(M, 256, tp), _guarded(M, cn, tp)), check)


@pytest.mark.gpu
@pytest.mark.parametrize("num_cu", [3, None], ids=_grid_id)
@pytest.mark.parametrize("J,cn,store,dec", [(1, 64, False, None), (2, 64, True, None), (3, 128, True, (2, 6, 16))],
                         ids=["J1-cn64-nostore", "J2-cn64-store", "J3-cn128-dec2x6x16"])
def test_chain_beside_a_sibling_stream(monkeypatch, J, cn, store, dec, num_cu):
    num_cu = _grid(monkeypatch, num_cu)
    M = _pixels(dec) if dec else M7
    d, (y3, y1, _) = chain_case(J, cn, M, dec)
    lead = dec if dec else (M,)
    lead3 = (dec[0], dec[1] // 2, dec[2] // 2) if dec else (M,)
    links = [(_g(x).reshape(*lead, 64), None if xs is None else _g(xs).reshape(*lead, 64), _g(w), _g(b, torch.float32))
             for x, xs, w, b in d["links"]]
    w1, b1 = _g(d["w1"]), _g(d["b1"], torch.float32)
    wgs = min(-(-M // 64), num_cu)
    rows3 = y3.shape[0]

    def launch(bufs):
        K.bottleneck_chain(links, w1, b1, y1=bufs[1][:M].view(*lead, cn),
                           y3=bufs[0][:rows3].view(*lead3, 256) if store else None, y3_decimated=dec is not None,
                           store_y3=store)

    def check(bufs, what):
        if store:
            _assert_bits(f"chain J{J} cn{cn} y3, {what}", bufs[0], y3, 64, wgs, _dec_rows(dec) if dec else None)
        else:  # nothing may touch the y3 buffer
            _assert_bits(f"chain J{J} cn{cn} y3 (not stored), {what}", bufs[0], y3[:0], 64, wgs)
        _assert_bits(f"chain J{J} cn{cn} y1, {what}", bufs[1], y1, 64, wgs)

    _beside_sibling(launch, lambda: (_guarded(rows3 if store else 0, 256, 64), _guarded(M, cn, 64)), check)
