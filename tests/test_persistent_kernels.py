"""The persistent kernels' multi-tile loops, bit for bit.

``conv3x3c64``, ``bottleneck_tail``, ``bottleneck_chain`` and ``pw_res`` launch
``min(tiles, num_cu)`` workgroups that loop over tiles with a one-tile-ahead prefetch.  The
grid size is an argument (``ops.kernels._NUM_CU``), so a handful of workgroups can be made
to walk every tile of a few hundred pixels: the loop's back edge (double-buffered stages,
deferred stores, the ``more`` / ``!more`` exits) runs at test sizes.

The data are integers that are exact in bf16.  Every product and every partial sum is then
an integer below 2^24, fp32 accumulation is exact in any order, and the only inexact steps
are the kernels' bf16 roundings (``f2bf``, round to nearest even), which are deterministic.
The float64 references below round where the ``.hip`` files round, so kernel and reference
must agree exactly: the GPU tests assert ``torch.equal`` on bf16 tensors (a value
comparison; integer sums that start from +0 never produce -0, so it is a bit comparison
here) and report tile, owning workgroup, pixel and channel of the first mismatches.

The non-GPU tests check the references alone: that the data make each rounding and each
ReLU observable, that deliberately wrong variants of each reference differ from it on these
data, and that each reference equals the ``K.*`` host path where nothing rounds."""
import functools

import pytest
import torch

from flink_tensorflow_amd.ops import kernels as K

BF = torch.bfloat16
F64 = torch.float64
EXACT = 2 ** 24      # integers below this are exact in fp32
SENTINEL = -77.0     # exact in bf16
FAULTS = ("round_late", "drop_chunk", "stale_tile", "swap_frag")


# ------------------------------------------------------------------------------ references
def _bf(v):
    """bf16 round-to-nearest-even of float64 integers below 2^24 (float64 -> fp32 is exact)."""
    return v.to(BF).to(F64)


class _Trace:
    """What a reference saw: the share of values each rounding changed, the share each ReLU
    zeroed, and an upper bound of every intermediate magnitude (partial sums included)."""

    def __init__(self):
        self.rounded, self.zeros, self.peak = {}, {}, 0.0

    def see(self, bound):
        self.peak = max(self.peak, float(bound.max()))

    def round(self, name, v):
        r = _bf(v)
        self.rounded[name] = (r != v).double().mean().item()
        return r

    def relu(self, name, v):
        r = torch.relu(v)
        self.zeros[name] = (r == 0).double().mean().item()
        return r

    def close(self):
        assert self.peak < EXACT, f"intermediate magnitude {self.peak} is not exact in fp32"
        return self


_SWAP = torch.cat([torch.arange(16, 32), torch.arange(0, 16)])


def _acc(tr, x, w, extra, tp, fault):
    """``x [M, K] . w [N, K]^T`` in float64, ``extra`` = what is added before the next rounding
    (for the magnitude bound only).  ``fault`` builds the wrong variants of the discrimination
    test: one 8-element K chunk dropped, the source rows of every tile but the first read one
    tile early (a stale prefetch stage), two 16-channel accumulator fragments swapped."""
    if fault == "drop_chunk":
        x = x.clone()
        x[:, 8:16] = 0
    if fault == "stale_tile":
        rows = torch.arange(x.shape[0])
        rows[tp:] -= tp
        x = x[rows]
    tr.see(x.abs() @ w.abs().t() + extra)
    a = x @ w.t()
    if fault == "swap_frag":
        a = a.clone()
        a[:, :32] = a[:, _SWAP]
    return a


def _decimate(y, dec):
    if dec is None:
        return y
    N, H, W = dec
    return y.reshape(N, H, W, -1)[:, ::2, ::2].reshape(N * (H // 2) * (W // 2), -1)


def ref_tail(x2, second, w3, b3, w1, b1, dual, tp, dec=None, fault=None):
    """bottleneck.hip.  Phase 1: ``a = bf16(acc + b3)`` into the Y tile (acc over ``[x2 | xs]``
    for dual).  Pass: ``y3 = bf16(relu(a + res))`` (dual: residual registers are zero), stored
    (decimated: even (h, w) only, compact) and written back into Y.  Phase 2:
    ``y1 = bf16(relu(y3 . W1^T + b1))``.  Returns ``(y3 as stored, y1, trace)``."""
    tr = _Trace()
    xin = torch.cat([x2, second], 1) if dual else x2
    res = torch.zeros(1, dtype=F64) if dual else second
    acc = _acc(tr, xin, w3, b3.abs() + res.abs().max(), tp, fault) + b3
    if fault == "round_late":
        y3 = tr.round("y3", tr.relu("y3", acc + res))
    else:
        y3 = tr.round("y3", tr.relu("y3", tr.round("a", acc) + res))
    y1 = tr.round("y1", tr.relu("y1", _acc(tr, y3, w1, b1.abs(), tp, None) + b1))
    return _decimate(y3, dec), y1, tr.close()


def ref_chain(links, w1, b1, tp=64, dec=None, fault=None):
    """bottleneck_chain.hip.  Per link (``finish``): ``v = bf16(acc + b)``; first link
    ``y = bf16(relu(v))`` with acc over ``[x | xs]``, later links ``y = bf16(relu(v + y))`` with
    the previous link's y as residual.  The last y goes to the Y tile and, if stored, to y3
    (decimated or not).  Phase 2: ``y1 = bf16(relu(y . W1^T + b1))``.  Returns (y3, y1, trace)."""
    tr = _Trace()
    y = None
    for j, (x, xs, w, b) in enumerate(links):
        xin = x if xs is None else torch.cat([x, xs], 1)
        prev = torch.zeros(1, dtype=F64) if y is None else y
        acc = _acc(tr, xin, w, b.abs() + prev.abs().max(), tp, fault) + b
        if fault == "round_late" and j:
            y = tr.round(f"y3_{j}", tr.relu(f"y3_{j}", acc + prev))
        else:
            y = tr.round(f"y3_{j}", tr.relu(f"y3_{j}", tr.round(f"a_{j}", acc) + prev))
    y1 = tr.round("y1", tr.relu("y1", _acc(tr, y, w1, b1.abs(), tp, None) + b1))
    return _decimate(y, dec), y1, tr.close()


def _conv_tiles(N, H, W):
    """conv3x3c64.hip ``tile_of``: 8 x 32 output tiles, the last row / column tile pulled
    back inside the image (it overlaps its neighbour)."""
    return [(n, min(i * 8, H - 8), min(j * 32, W - 32))
            for n in range(N) for i in range(-(-H // 8)) for j in range(-(-W // 32))]


def ref_conv(x, w, b, act, fault=None):
    """conv3x3c64.hip: ``y = bf16(act(conv + b))``, 3x3 / stride 1 / pad 1, one rounding in
    the epilogue.  x [N, H, W, 64], w [64, 3, 3, 64] (OHWI).  There is no residual, so
    ``round_late`` has no counterpart; ``stale_tile`` gives every tile but the first the
    output of the tile before it (what a stale patch stage computes).  Returns (y, trace)."""
    tr = _Trace()
    if fault == "drop_chunk":
        x = x.clone()
        x[..., 8:16] = 0
    conv = lambda xx, ww: torch.nn.functional.conv2d(xx.permute(0, 3, 1, 2), ww.permute(0, 3, 1, 2),
                                                     padding=1).permute(0, 2, 3, 1)
    tr.see(conv(x.abs(), w.abs()) + b.abs())
    y = conv(x, w) + b
    if fault == "swap_frag":
        y = y.clone()
        y[..., :32] = y[..., _SWAP]
    if fault == "stale_tile":
        tiles, stale = _conv_tiles(*x.shape[:3]), y.clone()
        for (n, y0, x0), (pn, py, px) in zip(tiles[1:], tiles[:-1]):
            stale[n, y0:y0 + 8, x0:x0 + 32] = y[pn, py:py + 8, px:px + 32]
        y = stale
    if act == "relu":
        y = tr.relu("y", y)
    return tr.round("y", y), tr.close()


def ref_pw_res(x, w, b, res, tp, fault=None):
    """pw_res.hip.  The epilogue first writes ``a = bf16(acc + bias)`` into the LDS output
    tile, then reads it back in coalesced chunks and stores ``y = bf16(relu(a + res))``: two
    roundings, the first before the residual add.  Returns (y, trace)."""
    tr = _Trace()
    acc = _acc(tr, x, w, b.abs() + res.abs().max(), tp, fault) + b
    if fault == "round_late":
        return tr.round("y", tr.relu("y", acc + res)), tr.close()
    return tr.round("y", tr.relu("y", tr.round("a", acc) + res)), tr.close()


# ------------------------------------------------------------------------------------ data
# Integer ranges.  A K-deep sum of products of uniform integers in [-rx, rx] and [-rw, rw] has
# a standard deviation of sqrt(K (rx (rx + 1) / 3) (rw (rw + 1) / 3)); bf16 holds 8 significant
# bits, so a rounding changes a value only beyond +-256.  Activations in [-8, 8] with weights in
# [-4, 4] over K = 128 give sigma = 143 (|v| > 256 for ~7 %, about half of those odd); over
# K = 64 that is sigma = 101 and under 1 % rounded, so the 64-deep GEMMs take weights in
# [-6, 6] (sigma = 147).  The 256-deep reduce over y3 (hundreds) takes weights in [-2, 2];
# the 3x3 conv (K = 576) takes [-4, 4] (sigma = 304).  Worst case 576 * 8 * 4 and
# 256 * ~1500 * 2 stay far below 2^24; each reference asserts its own bound.
# ``small``: magnitudes at which no rounding changes anything (host-path comparison).
def _ints(g, shape, r, keep=1.0):
    t = torch.randint(-r, r + 1, shape, generator=g).to(F64)
    if keep < 1.0:
        t = t * (torch.rand(shape, generator=g) < keep)
    return t


TAIL_VARIANTS = {"cn64-res": (64, False, 128), "cn64-dual": (64, True, 64), "cn128-res": (128, False, 64)}


def tail_data(variant, M, small=False):
    cn, dual, _ = TAIL_VARIANTS[variant]
    g = torch.Generator().manual_seed(1000 + cn + dual + M)
    if small:
        return dict(x2=_ints(g, (M, 64), 1), second=_ints(g, (M, 64 if dual else 256), 1),
                    w3=_ints(g, (256, 128 if dual else 64), 1, 0.5), b3=_ints(g, (256,), 2),
                    w1=_ints(g, (cn, 256), 1, 0.1), b1=_ints(g, (cn,), 2))
    return dict(x2=_ints(g, (M, 64), 8), second=_ints(g, (M, 64), 8) if dual else _ints(g, (M, 256), 40),
                w3=_ints(g, (256, 128), 4) if dual else _ints(g, (256, 64), 6), b3=_ints(g, (256,), 33),
                w1=_ints(g, (cn, 256), 2), b1=_ints(g, (cn,), 33))


def chain_data(J, cn, M, small=False):
    g = torch.Generator().manual_seed(2000 + 10 * J + cn + M)
    rx, rw0, rw, rb, r1, k0, k1 = (1, 1, 1, 2, 1, 0.5, 0.1) if small else (8, 4, 6, 33, 2, 1.0, 1.0)
    links = [(_ints(g, (M, 64), rx), _ints(g, (M, 64), rx) if j == 0 else None,
              _ints(g, (256, 128), rw0, k0) if j == 0 else _ints(g, (256, 64), rw, k0), _ints(g, (256,), rb))
             for j in range(J)]
    return dict(links=links, w1=_ints(g, (cn, 256), r1, k1), b1=_ints(g, (cn,), rb))


def conv_data(shape, small=False):
    N, H, W = shape
    g = torch.Generator().manual_seed(3000 + N * H * W)
    rx, rw, rb, keep = (1, 1, 2, 0.5) if small else (8, 4, 33, 1.0)
    return dict(x=_ints(g, (N, H, W, 64), rx), w=_ints(g, (64, 3, 3, 64), rw, keep), b=_ints(g, (64,), rb))


PW_VARIANTS = {"k128-n128": (128, 128, 0, 128), "k256-n256": (256, 256, 0, 64), "k256-n128-tp128": (256, 128, 128, 128)}


def pw_data(variant, M, small=False):
    K_, N, _, _ = PW_VARIANTS[variant]
    g = torch.Generator().manual_seed(4000 + K_ + N + M)
    rx, rw, rb, rr, keep = (1, 1, 2, 2, 0.5) if small else (8, 4, 33, 40, 1.0)
    return dict(x=_ints(g, (M, K_), rx), w=_ints(g, (N, K_), rw, keep), b=_ints(g, (N,), rb), res=_ints(g, (M, N), rr))


# Shapes.  Pixel-matrix kernels: 6 full tiles and a partial one (37 rows), and the partial tile
# alone.  Decimated y3: the production row width (448 px: a partial TP = 128 tile); W no multiple
# of 16 with image rows that straddle tiles and a partial tile; the existing small case.
DEC_SHAPES = [(1, 8, 56), (3, 6, 22), (2, 6, 10)]
CONV_SHAPES = [(3, 13, 37), (1, 8, 32)]   # 12 tiles, edge tiles overlapping both ways; one tile


@functools.lru_cache(maxsize=None)
def tail_case(variant, M, dec=None):
    cn, dual, tp = TAIL_VARIANTS[variant]
    d = tail_data(variant, M)
    return d, ref_tail(**d, dual=dual, tp=tp, dec=dec)


@functools.lru_cache(maxsize=None)
def chain_case(J, cn, M, dec=None):
    d = chain_data(J, cn, M)
    return d, ref_chain(**d, dec=dec)


@functools.lru_cache(maxsize=None)
def conv_case(shape, act):
    d = conv_data(shape)
    return d, ref_conv(**d, act=act)


@functools.lru_cache(maxsize=None)
def pw_case(variant, M):
    d = pw_data(variant, M)
    return d, ref_pw_res(**d, tp=PW_VARIANTS[variant][3])


def _pixels(shape):
    return shape[0] * shape[1] * shape[2]


# ------------------------------------------------------------ non-GPU: the references alone
# Rounding points excused from the 1 % condition, with the reason: relu(bf16 value) is a bf16
# value, so the second rounding of a link without residual changes nothing by construction.
EXCUSED = {"tail cn64-dual": ("y3",), "chain": ("y3_0",)}

REFERENCES = (
    [(f"tail {v}", lambda v=v: tail_case(v, 6 * TAIL_VARIANTS[v][2] + 37)[1][-1]) for v in TAIL_VARIANTS]
    + [(f"chain J{J} cn{cn}", lambda J=J, cn=cn: chain_case(J, cn, 6 * 64 + 37)[1][-1])
       for J in (1, 2, 3) for cn in (64, 128)]
    + [(f"chain J3 cn128 dec {s}", lambda s=s: chain_case(3, 128, _pixels(s), s)[1][-1]) for s in DEC_SHAPES]
    + [(f"conv {s} {act}", lambda s=s, act=act: conv_case(s, act)[1][-1]) for s in CONV_SHAPES for act in (None, "relu")]
    + [(f"pw_res {v}", lambda v=v: pw_case(v, 20 * PW_VARIANTS[v][3] + 37)[1][-1]) for v in PW_VARIANTS])


@pytest.mark.parametrize("name,trace", REFERENCES, ids=[n for n, _ in REFERENCES])
def test_reference_data_make_roundings_and_relus_observable(name, trace):
    """Every rounding changes at least 1 % of its values (the order of rounding is then
    observable), every ReLU zeroes 10 to 90 %, every intermediate is exact in fp32."""
    tr = trace()
    print(name, "rounded", tr.rounded, "zeroed", tr.zeros, "peak", tr.peak)
    assert tr.peak < EXACT
    excused = EXCUSED.get(name, EXCUSED["chain"] if name.startswith("chain") else ())
    for point, share in tr.rounded.items():
        if point in excused:
            assert share == 0.0, (point, share)
        else:
            assert share >= 0.01, f"{name}: rounding {point} changes only {share:.4f} of the values"
    for point, share in tr.zeros.items():
        assert 0.10 <= share <= 0.90, f"{name}: relu {point} zeroes {share:.4f} of the values"


def _differs(a, b):
    return a.shape == b.shape and not torch.equal(a, b)


@pytest.mark.parametrize("fault", FAULTS)
def test_wrong_variants_differ_from_the_reference(fault):
    """The data can catch what the GPU tests are for: rounding after the residual add, a
    dropped 8-element K chunk, a tile computed from the previous tile's rows, two swapped
    16-channel fragments — each changes every output of every reference it applies to
    (``round_late`` needs a residual: not the dual tail, the one-link chain or the conv)."""
    for v, (cn, dual, tp) in TAIL_VARIANTS.items():
        if fault == "round_late" and dual:
            continue
        for M, dec in [(6 * tp + 37, None)] + ([(_pixels(s), s) for s in DEC_SHAPES[:2]] if not dual else []):
            d, (y3, y1, _) = tail_case(v, M, dec)
            w3, w1, _ = ref_tail(**d, dual=dual, tp=tp, dec=dec, fault=fault)
            assert _differs(w3, y3) and _differs(w1, y1), (v, M, dec)
    for J in (1, 2, 3):
        if fault == "round_late" and J == 1:
            continue
        for cn in (64, 128):
            d, (y3, y1, _) = chain_case(J, cn, 6 * 64 + 37)
            w3, w1, _ = ref_chain(**d, fault=fault)
            assert _differs(w3, y3) and _differs(w1, y1), (J, cn)
    if fault != "round_late":
        for act in (None, "relu"):
            d, (y, _) = conv_case(CONV_SHAPES[0], act)
            assert _differs(ref_conv(**d, act=act, fault=fault)[0], y), act
    for v, (_, _, _, tp) in PW_VARIANTS.items():
        d, (y, _) = pw_case(v, 20 * tp + 37)
        assert _differs(ref_pw_res(**d, tp=tp, fault=fault)[0], y), v


def _f32(d):
    return {k: v.float() if torch.is_tensor(v) else v for k, v in d.items()}


def test_references_equal_the_host_paths_where_nothing_rounds():
    """All values <= 256: the bf16 roundings are the identity, and the fp32 host paths of
    ``ops.kernels`` (which skip them) compute the same integers as the references."""
    def small(tr):
        assert tr.peak <= 256 and not any(tr.rounded.values()), (tr.peak, tr.rounded)

    for v, (cn, dual, tp) in TAIL_VARIANTS.items():
        for shape in ((2, 8, 20), (2, 6, 10)):
            dec = shape if not dual and shape[1] == 6 else None
            d = tail_data(v, _pixels(shape), small=True)
            y3, y1, tr = ref_tail(**d, dual=dual, tp=tp, dec=dec)
            small(tr)
            f = _f32(d)
            x2, second = f["x2"].reshape(*shape, 64), f["second"].reshape(*shape, -1)
            h3, h1 = K.bottleneck_tail(x2, None if dual else second, f["w3"], f["b3"], f["w1"], f["b1"],
                                       xs=second if dual else None, y3_decimated=dec is not None)
            assert torch.equal(h3.reshape(-1, 256).double(), y3) and torch.equal(h1.reshape(-1, cn).double(), y1)
    for J in (1, 2, 3):
        for cn, shape, dec in ((64, (2, 8, 20), False), (128, (2, 6, 10), True)):
            d = chain_data(J, cn, _pixels(shape), small=True)
            y3, y1, tr = ref_chain(**d, dec=shape if dec else None)
            small(tr)
            links = [(x.float().reshape(*shape, 64), None if xs is None else xs.float().reshape(*shape, 64), w.float(),
                      b.float()) for x, xs, w, b in d["links"]]
            h3, h1 = K.bottleneck_chain(links, d["w1"].float(), d["b1"].float(), y3_decimated=dec)
            assert torch.equal(h3.reshape(-1, 256).double(), y3) and torch.equal(h1.reshape(-1, cn).double(), y1)
            assert K.bottleneck_chain(links, d["w1"].float(), d["b1"].float(), store_y3=False)[0] is None
    for act in (None, "relu"):
        d = conv_data((2, 13, 37), small=True)
        y, tr = ref_conv(**d, act=act)
        small(tr)
        f = _f32(d)
        assert torch.equal(K.conv3x3_c64(f["x"], f["w"], f["b"], act).double(), y)
    for v, (K_, N, tp_arg, tp) in PW_VARIANTS.items():
        d = pw_data(v, 300, small=True)
        y, tr = ref_pw_res(**d, tp=tp)
        small(tr)
        f = _f32(d)
        assert torch.equal(K.pw_res(f["x"], f["w"], f["b"], f["res"], tp=tp_arg).double(), y)


# ------------------------------------------------------------------------------ GPU helpers
DEV = torch.device("cuda", 0)
# Forced grids.  With 7 tiles (6 full + the partial one, tile 6):
#   1        one workgroup runs all 7 tiles; the partial tile is its last
#   3        workgroup 0 runs tiles 0, 3, 6 (three tiles, the partial one as a later tile),
#            workgroups 1 and 2 run two each
#   5        workgroups 0 and 1 run two tiles (1: tile 1, then the partial tile 6), workgroups
#            2 to 4 run exactly one tile and leave by the ``!more`` exit at once
#   default  one tile per workgroup: the partial tile is a workgroup's first tile
# and with M = 37 the partial tile is the first and only tile at every grid.  The decimated
# shapes have 7, 7 and 2 tiles at TP = 64 and 4, 4 and 1 at TP = 128 (grid 3: workgroup 0 runs
# tile 0 and the partial tile 3).
GRIDS = [1, 3, 5, None]


def _grid_id(n):
    return "cu-default" if n is None else f"cu{n}"


def _shape_id(s):
    return "x".join(map(str, s))


def _grid(monkeypatch, num_cu):
    if num_cu is not None:
        monkeypatch.setitem(K._NUM_CU, DEV.index, num_cu)
    return K._NUM_CU[DEV.index]


def _g(t, dtype=BF):
    return None if t is None else t.to(DEV, dtype)


def _guarded(rows, width, guard):
    """Output buffer with ``guard`` rows beyond ``rows``, all pre-filled with the sentinel."""
    return torch.full((rows + guard, width), SENTINEL, dtype=BF, device=DEV)


def _assert_bits(what, buf, want, tp, workgroups, src_rows=None):
    """Rows < M of ``buf`` equal ``want`` exactly; the guard rows beyond still hold the
    sentinel.  A mismatch names tile, owning workgroup, pixel within the tile and channel."""
    M = want.shape[0]
    got, want = buf[:M].cpu(), want.to(BF)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        lines = []
        for r, c in bad[:12].tolist():
            p = r if src_rows is None else int(src_rows[r])
            tile, px = divmod(p, tp)
            lines.append(f"  row {r} (pixel {p}) = tile {tile} (workgroup {tile % workgroups}) pixel {px}, channel {c}:"
                         f" got {got[r, c].item()}, want {want[r, c].item()}")
        raise AssertionError(f"{what}: {bad.shape[0]} of {want.numel()} values differ ({workgroups} workgroups, tile of"
                             f" {tp} pixels); first:\n" + "\n".join(lines))
    guard = buf[M:]
    assert (guard == SENTINEL).all(), f"{what}: {(guard != SENTINEL).sum().item()} values written past row {M}"


def _dec_rows(dec):
    """Source pixel of each row of a decimated y3."""
    N, H, W = dec
    return torch.arange(N * H * W).reshape(N, H, W)[:, ::2, ::2].reshape(-1)


def _run_tail(variant, M, dec, num_cu):
    cn, dual, tp = TAIL_VARIANTS[variant]
    d, (y3, y1, _) = tail_case(variant, M, dec)
    lead = dec if dec else (M,)
    lead3 = (dec[0], dec[1] // 2, dec[2] // 2) if dec else (M,)
    b3, b1 = _guarded(y3.shape[0], 256, tp), _guarded(M, cn, tp)
    second = _g(d["second"]).reshape(*lead, -1)
    K.bottleneck_tail(_g(d["x2"]).reshape(*lead, 64), None if dual else second, _g(d["w3"]), _g(d["b3"], torch.float32),
                      _g(d["w1"]), _g(d["b1"], torch.float32), y3=b3[:y3.shape[0]].view(*lead3, 256),
                      y1=b1[:M].view(*lead, cn), xs=second if dual else None, y3_decimated=dec is not None)
    torch.cuda.synchronize()
    wgs = min(-(-M // tp), num_cu)
    _assert_bits(f"tail {variant} y3", b3, y3, tp, wgs, _dec_rows(dec) if dec else None)
    _assert_bits(f"tail {variant} y1", b1, y1, tp, wgs)


def _run_chain(J, cn, M, dec, store, num_cu):
    d, (y3, y1, _) = chain_case(J, cn, M, dec)
    lead = dec if dec else (M,)
    lead3 = (dec[0], dec[1] // 2, dec[2] // 2) if dec else (M,)
    b3, b1 = _guarded(y3.shape[0], 256, 64), _guarded(M, cn, 64)
    links = [(_g(x).reshape(*lead, 64), None if xs is None else _g(xs).reshape(*lead, 64), _g(w), _g(b, torch.float32))
             for x, xs, w, b in d["links"]]
    r3, _ = K.bottleneck_chain(links, _g(d["w1"]), _g(d["b1"], torch.float32), y1=b1[:M].view(*lead, cn),
                               y3=b3[:y3.shape[0]].view(*lead3, 256) if store else None,
                               y3_decimated=dec is not None, store_y3=store)
    torch.cuda.synchronize()
    wgs = min(-(-M // 64), num_cu)
    if store:
        _assert_bits(f"chain J{J} cn{cn} y3", b3, y3, 64, wgs, _dec_rows(dec) if dec else None)
    else:
        assert r3 is None and (b3 == SENTINEL).all()
    _assert_bits(f"chain J{J} cn{cn} y1", b1, y1, 64, wgs)


# --------------------------------------------------------------------- GPU: bit-exact cases
@pytest.mark.gpu
@pytest.mark.parametrize("num_cu", GRIDS, ids=_grid_id)
@pytest.mark.parametrize("tiles", [6, 0], ids=["7tiles", "37px"])
@pytest.mark.parametrize("variant", list(TAIL_VARIANTS))
def test_tail_bit_exact(monkeypatch, variant, tiles, num_cu):
    _run_tail(variant, tiles * TAIL_VARIANTS[variant][2] + 37, None, _grid(monkeypatch, num_cu))


@pytest.mark.gpu
@pytest.mark.parametrize("num_cu", GRIDS, ids=_grid_id)
@pytest.mark.parametrize("dec", DEC_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("variant", ["cn128-res", "cn64-res"])
def test_tail_decimated_bit_exact(monkeypatch, variant, dec, num_cu):
    _run_tail(variant, _pixels(dec), dec, _grid(monkeypatch, num_cu))


@pytest.mark.gpu
@pytest.mark.parametrize("num_cu", GRIDS, ids=_grid_id)
@pytest.mark.parametrize("store", [True, False])
@pytest.mark.parametrize("cn", [64, 128])
@pytest.mark.parametrize("J", [1, 2, 3])
def test_chain_bit_exact(monkeypatch, J, cn, store, num_cu):
    _run_chain(J, cn, 6 * 64 + 37, None, store, _grid(monkeypatch, num_cu))


@pytest.mark.gpu
@pytest.mark.parametrize("num_cu", GRIDS, ids=_grid_id)
@pytest.mark.parametrize("dec", DEC_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("J,cn", [(3, 128), (1, 64)])
def test_chain_decimated_bit_exact(monkeypatch, J, cn, dec, num_cu):
    _run_chain(J, cn, _pixels(dec), dec, True, _grid(monkeypatch, num_cu))


# (3, 13, 37): 12 tiles.  Grid 1: one workgroup, 12 tiles.  Grid 5: workgroups 0 and 1 run
# three tiles (0, 5, 10 and 1, 6, 11: the overlapping bottom / right edge tiles as later tiles),
# the others two.  Default: one tile each, edge tiles as first tiles.  (1, 8, 32): one tile.
@pytest.mark.gpu
@pytest.mark.parametrize("num_cu", [1, 5, None], ids=_grid_id)
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=_shape_id)
def test_conv3x3_c64_bit_exact(monkeypatch, shape, act, num_cu):
    num_cu = _grid(monkeypatch, num_cu)
    d, (y, _) = conv_case(shape, act)
    N, H, W = shape
    M = N * H * W
    buf = _guarded(M, 96, 8 * 32)
    K.conv3x3_c64(_g(d["x"]), _g(d["w"]), _g(d["b"], torch.float32), act, out=buf[:M].view(N, H, W, 96),
                  out_channel_offset=16)
    torch.cuda.synchronize()
    got = buf[:M].view(N, H, W, 96)[..., 16:80].cpu()
    want = y.to(BF)
    if not torch.equal(got, want):
        tiles_y, tiles_x = -(-H // 8), -(-W // 32)
        wgs = min(N * tiles_y * tiles_x, num_cu)
        bad = (got != want).nonzero()
        lines = []
        for n, yy, xx, c in bad[:12].tolist():
            tile = (n * tiles_y + yy // 8) * tiles_x + xx // 32
            lines.append(f"  (n {n}, y {yy}, x {xx}) = tile {tile} (workgroup {tile % wgs}), channel {c}:"
                         f" got {got[n, yy, xx, c].item()}, want {want[n, yy, xx, c].item()}")
        raise AssertionError(f"conv3x3c64 {shape} {act}: {bad.shape[0]} of {want.numel()} values differ ({wgs} workgroups);"
                             " first:\n" + "\n".join(lines))
    assert (buf[:M, :16] == SENTINEL).all() and (buf[:M, 80:] == SENTINEL).all() and (buf[M:] == SENTINEL).all()


# 21 tiles (20 full + the partial tile 20).  The launcher takes num_cu in multiples of
# 8 S (S = N / 128 channel slices) and runs G / S tile groups; group (xcd, g) starts at tile
# xcd * gpx + g and strides by the group count.  num_cu = 8 S: 8 groups, groups 0 to 4 run
# three tiles (group 4: tiles 4, 12 and the partial tile 20, as a later tile), groups 5 to 7
# two.  Default: every group runs at most one tile, the partial tile is a group's first tile
# and groups beyond the tile count leave before the first barrier.  The launcher accepts no
# grid at which a group runs exactly one tile and another several.
@pytest.mark.gpu
@pytest.mark.parametrize("smallest", [True, False], ids=["cu8S", "cu-default"])
@pytest.mark.parametrize("variant", list(PW_VARIANTS))
def test_pw_res_bit_exact(monkeypatch, variant, smallest):
    K_, N, tp_arg, tp = PW_VARIANTS[variant]
    S = N // 128
    num_cu = _grid(monkeypatch, 8 * S if smallest else None)
    M = 20 * tp + 37
    d, (y, _) = pw_case(variant, M)
    # the two-slice case writes at a channel offset into a wider output
    width, off = (N + 128, 64) if S == 2 else (N, 0)
    buf = _guarded(M, width, tp)
    K.pw_res(_g(d["x"]), _g(d["w"]), _g(d["b"], torch.float32), _g(d["res"]), out=buf[:M], out_channel_offset=off,
             tp=tp_arg)
    torch.cuda.synchronize()
    groups = num_cu // (8 * S) * 8
    body = torch.cat([buf[:M, off:off + N], buf[M:, off:off + N]])
    _assert_bits(f"pw_res {variant}", body, y, tp, groups)
    assert (buf[:, :off] == SENTINEL).all() and (buf[:, off + N:] == SENTINEL).all()


# ------------------------------------------------- GPU: grid invariance on continuous data
def _randn_bf(g, *shape, s=1.0):
    return (torch.randn(*shape, generator=g) * s).to(DEV, BF)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["tail", "chain", "conv3x3c64", "pw_res"])
def test_outputs_do_not_depend_on_the_grid(monkeypatch, kernel):
    """The per-tile arithmetic does not depend on which workgroup runs the tile: randn data
    as in the tolerance tests, 3 workgroups (pw_res: 8 per slice) against the device default."""
    g = torch.Generator().manual_seed(17)
    f32 = lambda n: torch.randn(n, generator=g).to(DEV)
    if kernel == "tail":
        M = 6 * 64 + 37
        a = (_randn_bf(g, M, 64), _randn_bf(g, M, 256), _randn_bf(g, 256, 64, s=0.1), f32(256),
             _randn_bf(g, 128, 256, s=0.05), f32(128))
        run = lambda: K.bottleneck_tail(*a)
    elif kernel == "chain":
        M = 6 * 64 + 37
        links = [(_randn_bf(g, M, 64), _randn_bf(g, M, 64), _randn_bf(g, 256, 128, s=1 / 11), f32(256) * 0.1)]
        links += [(_randn_bf(g, M, 64), None, _randn_bf(g, 256, 64, s=1 / 8), f32(256) * 0.1) for _ in range(2)]
        w1, b1 = _randn_bf(g, 128, 256, s=1 / 16), f32(128)
        run = lambda: K.bottleneck_chain(links, w1, b1)
    elif kernel == "conv3x3c64":
        a = (_randn_bf(g, 3, 13, 37, 64), _randn_bf(g, 64, 3, 3, 64, s=0.05), f32(64), "relu")
        run = lambda: (K.conv3x3_c64(*a),)
    else:
        M = 20 * 64 + 37
        a = (_randn_bf(g, M, 256), _randn_bf(g, 256, 256, s=1 / 16), f32(256), _randn_bf(g, M, 256))
        run = lambda: (K.pw_res(*a),)
    with monkeypatch.context() as m:
        m.setitem(K._NUM_CU, DEV.index, 16 if kernel == "pw_res" else 3)
        few = run()
    full = run()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(few, full)):
        assert bool(x.isfinite().all()), f"{kernel}: output {i} is not finite"
        rows = (x != y).any(-1).reshape(-1).nonzero().reshape(-1)
        assert rows.numel() == 0, (f"{kernel}: output {i} differs between the grids in {rows.numel()} pixels, "
                                   f"first {rows[:8].tolist()}")


# ------------------------------------------------------------------------- GPU: plan level
@pytest.mark.gpu
def test_compiled_plan_does_not_depend_on_the_grid(monkeypatch):
    """The small ResNet of tests/test_chain.py (depth 26, stage 1 at 56 x 56), batch 4, with
    fused and chained tails: the same logits with 64 workgroups per persistent kernel (the
    smallest count pw_res takes for 1024 channels) as with the device's CU count.  Both
    stage-1 tails run on the chain kernel here (one link without a y3 store, two links with
    the decimated store): 196 tiles of 64 pixels, 3 to 4 per workgroup; the stage-2 pw_res
    (25 tiles, 16 groups) runs 1 to 2; the 3x3 convs (56 tiles) stay at one tile each."""
    from flink_tensorflow_amd import config
    from flink_tensorflow_amd.graph.compiler import CompiledFunction
    from flink_tensorflow_amd.graph.graph import Graph
    from flink_tensorflow_amd.models.zoo.resnet import resnet50_graph_def

    graph = Graph.from_graph_def(resnet50_graph_def(depth=26, image_hw=(72, 72), num_classes=64))
    imgs = torch.randint(0, 256, (4, 72, 72, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).to(DEV)

    def logits():
        with config.override(fuse_block_tails=True, recompute_tails=True, chain_max_links=3):
            plan = CompiledFunction(graph, {"images:0": ((4, 72, 72, 3), "UINT8")}, ["logits:0"], DEV, strict=True)
        s = plan.summary()
        assert s["fused_tails"] == 2 and s["chained_tails"] == 1 and s["pw_res"] == 2 and s["conv3x3c64"] == 2, s
        out = plan({"images:0": imgs})[0].float().cpu()
        torch.cuda.synchronize()
        return out

    full = logits()
    with monkeypatch.context() as m:  # patched for the plan's whole life
        m.setitem(K._NUM_CU, DEV.index, 64)
        few = logits()
    assert full.isfinite().all() and torch.equal(few, full)
