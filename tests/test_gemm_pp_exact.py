"""The ping-pong 256x256 GEMM of ``kernels/gemm_pp.hip``, bit for bit: the direct epilogue, the
split-K kernel with its reduce kernel, the ``drelu`` mask epilogue, gelu / tanh and the host-side
argument checks.  Method and helpers are those of ``tests/test_igemm_exact.py``.

The operands are integers that are exact in bf16 (the bias is fp32 half-integers): x in [-8, 8],
w in [-4, 4], bias halves in [-600, 600] with both signs, residual integers in [-256, 256]; without
a bias x in [-24, 24] and w in [-8, 8], so that the sums alone pass 256, where bf16 starts to round.
Each reference asserts ``sum |x||w| + |b| + |r| < 2^23`` per output: fp32 accumulation is then exact
in any order, also across split-K slices, and the only inexact steps are the kernel's ``f2bf``
roundings (round to nearest even).  The float64 references are written from the ``.hip`` file and
round where it rounds:

direct path (``splits == 1``, or more splits requested than K-tiles)
    without residual ``y = bf16(act(acc + bias))``; with residual ``a = bf16(acc + bias)`` into the
    LDS tile, then ``y = bf16(act(float(a) + r))``: two roundings; ``drelu``: ``a = bf16(acc + bias)``,
    then ``y = mask > 0 ? a : +0``.
split path (``splits > 1``)
    ``y = bf16(act(sum_s part_s + bias (+ r)))``: one rounding, in ``gemm_pp_reduce``; ``drelu``:
    ``y = bf16(mask > 0 ? sum + bias : 0)``.

The host path of ``K.gemm_pp`` rounds once everywhere; it anchors the references where nothing
rounds twice.

The GPU tests compare bf16 bit patterns (``view(torch.int16)``).  No -0 can arise: the accumulators
start from +0 and sums of integers give +0 under round-to-nearest, the data hold no -0, ReLU is
``x > 0 ? x : 0``, the masked-out ``drelu`` value is ``f2bf(0.f)``, ``0 * rcp(..)`` of GELU at +0 is
+0 and tanh(0) is not among the inputs.  A mismatch is reported with (row, column, tile index,
K-tile count) of the first few elements.

Guards of every GPU case: the output goes through ``out=`` into a buffer pre-filled with the
sentinel 2^100, row stride ``ldy = N + 40``, a column offset from (16, 0, 8, 24) in turn and 256
guard rows (one more tile) after the last row; everything outside the written window must still
hold the sentinel and nothing inside may.  Every operand (x, w, bias, residual or mask, split
workspace) is a view between NaN bands.  Bias, residual and the workspace are plain global loads,
so a read past either end of them shows as NaN.  x and w go through buffer descriptors sized
``M * ldx`` and ``N * ldw`` exactly: a read past the end of those returns zero, and a read before the
start cannot be formed, so the NaN bands around x and w see nothing of the DMA; the value comparison
covers those reads.  What the bands cannot see, the raw-entry runs (``_hip().gemm_pp``) do: they
use ``ldx = K + 64``, ``ldw = K + 64`` and ``ldr = N + 24`` with NaN in the pad columns, which lie
inside the descriptors, so a K walk that overshoots one tile on a live row puts NaN into the output.
The split workspace is exactly ``splits_actual * M * N`` floats, pre-filled with NaN: a partial tile
that is never written reaches the reduce kernel as NaN.  Every case runs once through ``K.gemm_pp``
and once through the raw entry.

Paths that no test reached before: ``ldx != K``, ``ldw != K``, ``ldr != N``; split-K with unequal
slices (``nk = 5``: 3 + 2, 2 + 2 + 1, and 4 requested slices recomputed to 3); split slices of a
single K-tile (the ``nk == 1`` prologue at ``kt0 != 0``); ``M <= 128`` (wave row 1 computes only dead
rows while the ping-pong barrier skew still has to line up); the XCD tile remap with a tile count
that is no multiple of 8 (12 tiles, ``r = 4``).

gelu / tanh use ``v_exp_f32`` and ``v_rcp_f32``; they are driven as in the igemm file by a permutation
matrix (K = N = 64) and a zero bias, so that the pre-activation is exactly the chosen input, on the
inputs ``_kept(act)`` of that file (``apply_act`` of ``common.h`` is the same function, so the same
error budget holds): direct, direct with an all-zero residual (``a = bf16(x)`` is exact, then act)
and the split reduce with K = 128, ``splits = 2``, the permutation in the first slice and zeros in
the second.

The wrong variants (``FAULTS``), each of which must differ from the truth on every case it applies
to: ``drop_last_ktile``; ``stale_half`` (rows with ``m % 128 >= 64``, the X_h1 half-tile, see K-tile
``t - 1``); ``swap_nh`` (columns [0, 32) and [32, 64) of a 64-column group swapped); ``swap_frag`` (two
16-column fragments swapped); ``slice_overrun`` (the last split slice walks ``kt_per_split`` tiles);
``slice_gap`` (the slice count taken as requested, so the last slice is missing); ``round_once``
(direct + residual); ``round_twice`` (split + residual); ``drelu_on_acc`` (masks on the accumulator's
sign); ``res_ld`` (residual read with row stride N where ``ldr`` is wider).

The non-GPU tests check the references alone: the exactness bound, that the data make every
rounding and ReLU observable, the anchor against the host path, the wrong variants and the
coverage of the case list."""
import collections
import functools
import itertools
import zlib

import pytest
import torch

from flink_tensorflow_amd.ops import kernels as K
from test_igemm_exact import COFFS, EXACT, GAP, SENT   # the conventions of that file, not copies of them
from test_igemm_exact import _act64, _kept             # the kept inputs' conditions are asserted there

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
BT = 256                # output tile edge; also the guard rows after the last row
XPAD, RPAD = 64, 24      # raw entry: ldx - K = ldw - K, ldr - N
FAULTS = ("drop_last_ktile", "stale_half", "swap_nh", "swap_frag", "slice_overrun", "slice_gap", "round_once",
          "round_twice", "drelu_on_acc", "res_ld")

_Case = collections.namedtuple("_Case", "name M N K splits act bias res coff")
_SEQ = itertools.count()

# (M, N, K, requested splits)
SHAPES = (
    (1, 8, 64, 1),          # minimal problem
    (129, 72, 128, 1),      # one live row in wave row 1; N inside one nh half
    (257, 264, 192, 1),     # 2 x 2 tiles, 1-row and 8-column tails, nk = 3
    (300, 40, 320, 1),      # nk = 5
    (64, 256, 256, 1),      # nk = 4, M < 128
    (520, 776, 64, 1),      # 3 x 4 = 12 tiles: the remap with r = 4
    (37, 72, 320, 2),       # slices 3 + 2
    (37, 72, 320, 3),       # slices 2 + 2 + 1
    (37, 72, 320, 4),       # 4 requested, per = 2, recomputed to 3
    (260, 264, 128, 2),     # single-tile slices, the second at kt0 = 1
    (129, 72, 64, 4),       # more splits than K-tiles: the direct path
)
DRELU_SHAPES = ((257, 264, 192, 1), (37, 72, 320, 2), (260, 264, 128, 2))


def _mk(M, N, Kd, splits, act, bias, res):
    coff = COFFS[next(_SEQ) % 4]
    name = (f"{M}x{N}x{Kd}-s{splits}-{act or 'none'}{'' if bias else '-nobias'}{'-res' if res and act != 'drelu' else ''}"
            f"-off{coff}")
    return _Case(name, M, N, Kd, splits, act, bias, res, coff)


CASES = [_mk(*s, act, bias, res) for s in SHAPES for bias in (True, False) for res in (False, True)
         for act in (None, "relu")]
CASES_DRELU = [_mk(*s, "drelu", bias, True) for s, bias in zip(DRELU_SHAPES, (True, False, True))]
ALL_CASES = CASES + CASES_DRELU


def _ids(cases):
    return [c.name for c in cases]


def py_splits(Kd, s):
    """``gemm_pp_splits`` of the ``.hip`` file: the slices actually run for ``s`` requested."""
    nk = Kd // 64
    if s <= 1 or nk <= 1:
        return 1
    per = -(-nk // min(s, nk))
    return -(-nk // per)


def _slices(c, fault=None):
    """[(first K-tile, end K-tile)] per slice, as the kernel walks them."""
    nk = c.K // 64
    if py_splits(c.K, c.splits) == 1:
        return [(0, nk)]
    per = -(-nk // min(c.splits, nk))
    sl = [(a, min(a + per, nk)) for a in range(0, nk, per)]
    if fault == "slice_overrun":
        sl[-1] = (sl[-1][0], sl[-1][0] + per)
    if fault == "slice_gap":
        sl = sl[:-1]
    return sl


# ------------------------------------------------------------------------------------ data
def _bf(v):
    return v.to(BF).to(F64)


def _act(v, act):
    return torch.relu(v) if act == "relu" else v


def _gen(c, salt):
    g = torch.Generator().manual_seed(zlib.crc32(f"{c.name}/{salt}".encode()))

    def ints(lo, hi, shape):
        return torch.randint(lo, hi + 1, shape, generator=g).to(F64)

    rx, rw = (8, 4) if c.bias else (24, 8)
    d = dict(x=ints(-rx, rx, (c.M, c.K)), w=ints(-rw, rw, (c.N, c.K)), bias=None, res=None)
    if c.bias:   # halves in [-600, 600], signs alternating along a random permutation: both occur
        sign = torch.ones(c.N, dtype=F64)
        sign[torch.randperm(c.N, generator=g)[::2]] = -1
        d["bias"] = sign * ints(1, 1200, (c.N,)) / 2
    if c.act == "drelu":
        d["res"] = ints(-2, 2, (c.M, c.N))     # the mask: zeros, negatives and positives
    elif c.res:
        d["res"] = ints(-256, 256, (c.M, c.N))
    return d


@functools.lru_cache(maxsize=None)
def _data(c):
    """The case's operands as float64 (exact in bf16 / fp32, no -0).  The seed is the first of 64
    for which the conditions of ``test_data_make_the_properties_observable`` hold; that test asserts
    them (they are conditions on the data and the reference, the kernel has no part in them)."""
    for salt in range(64):
        d = _gen(c, salt)
        if not _unobservable(c, _reference(c, d=d).shares):
            break
    return d


# -------------------------------------------------------------------------------- reference
def _past_end(A, width):
    """``A [R, K]`` widened by ``width`` columns that hold what a contiguous walk past the row's end
    reads: the next row's first elements, zero past the last row (the descriptor's end)."""
    R, Kd = A.shape
    flat = torch.cat([A.reshape(-1), torch.zeros(width, dtype=F64)])
    idx = torch.arange(R)[:, None] * Kd + Kd + torch.arange(width)[None, :]
    return torch.cat([A, flat[idx.clamp(max=flat.numel() - 1)] * (idx < R * Kd)], 1)


_Ref = collections.namedtuple("_Ref", "out exact peak shares")


def _reference(c, fault=None, d=None):
    """float64 mirror of the kernel -> ``_Ref``: ``out [M, N]`` holding the bf16 values, ``exact`` =
    the unrounded epilogue (what the host path computes), ``peak`` = the largest
    ``sum |x||w| + |b| + |r|``, ``shares`` = what each rounding / activation did."""
    d = _data(c) if d is None else d
    X, W = d["x"], d["w"]
    M, N, nk = c.M, c.N, c.K // 64
    slices = _slices(c, fault)
    split = py_splits(c.K, c.splits) > 1
    Xe, We = X, W
    if fault == "slice_overrun":
        Xe, We = _past_end(X, 64 * (slices[-1][1] - nk)), _past_end(W, 64 * (slices[-1][1] - nk))
    acc = torch.zeros(M, N, dtype=F64)
    h1 = (torch.arange(M) % 128 >= 64)[:, None]
    for a, b in slices:
        for t in range(a, b):
            xt = Xe[:, 64 * t:64 * t + 64]
            if fault == "stale_half" and t > a:
                xt = torch.where(h1, Xe[:, 64 * t - 64:64 * t], xt)
            if fault == "drop_last_ktile" and t == nk - 1:
                continue
            acc += xt @ We[:, 64 * t:64 * t + 64].t()
    if fault in ("swap_nh", "swap_frag"):
        w_ = 32 if fault == "swap_nh" else 16
        n = torch.arange(N)
        src = torch.where((n // (2 * w_) + 1) * 2 * w_ <= N, n ^ w_, n)   # complete groups only
        acc = acc[:, src]
    bias = torch.zeros(N, dtype=F64) if d["bias"] is None else d["bias"]
    v = acc + bias
    r = d["res"]
    peak = float((X.abs() @ W.abs().t() + bias.abs() + (0 if r is None else r.abs())).max())
    sh = {}
    if c.act == "drelu":
        keep = v > 0 if fault == "drelu_on_acc" else r > 0
        exact = torch.where(keep, v, torch.zeros_like(v))
        out = _bf(exact)      # direct: a = bf16(v), then the mask; split: the mask, then bf16: the same values
        sh["round"] = (out != exact).double().mean().item()
        sh["kept"], sh["masked"] = (r > 0).double().mean().item(), (r <= 0).double().mean().item()
        sh["mask_signs"] = float(bool((r < 0).any()) and bool((r == 0).any()) and bool((r > 0).any()))
        sh["mask_vs_acc"] = ((r > 0) != (v > 0)).double().mean().item()
    elif r is None:
        exact = _act(v, c.act)
        out = _bf(exact)
        sh["round"] = (out != exact).double().mean().item()
    else:
        if fault == "res_ld":   # rows taken N apart in the [M, N + RPAD] buffer (zeros in its pad)
            flat = torch.cat([r, torch.zeros(M, RPAD, dtype=F64)], 1).reshape(-1)
            r = flat[torch.arange(M)[:, None] * N + torch.arange(N)[None, :]]
        exact = _act(v + r, c.act)
        a = _bf(v)
        pre = _act(a + r, c.act)
        twice = (not split) != (fault in ("round_once", "round_twice"))
        out = _bf(pre) if twice else _bf(exact)
        sh["round_a"] = (a != v).double().mean().item()
        sh["round"] = (out != (pre if twice else exact)).double().mean().item()
        sh["double"] = (_bf(pre) != _bf(exact)).double().mean().item()
    if c.act == "relu":
        sh["zeros"], sh["pos"] = (out == 0).double().mean().item(), (out > 0).double().mean().item()
    return _Ref(out, exact, peak, sh)


def _unobservable(c, s):
    """What the data fail to show, as a list of words (empty: every check is observable)."""
    bad = []
    if c.act == "relu" and min(s["zeros"], s["pos"]) < 0.05:
        bad.append("relu")
    if s["round"] == 0:
        bad.append("round")
    if c.act == "drelu" and not (s["mask_signs"] and s["mask_vs_acc"] > 0 and min(s["kept"], s["masked"]) >= 0.05):
        bad.append("mask")
    if c.act != "drelu" and c.res and (s["round_a"] == 0 or s["double"] == 0):
        bad.append("double rounding")
    return bad


@functools.lru_cache(maxsize=None)
def _ref(c):
    r = _reference(c)
    assert r.peak < EXACT, f"{c.name}: sum |x||w| + |b| + |r| = {r.peak} is not exact in fp32"
    return r


def _applies(fault, c):
    nk, sl = c.K // 64, _slices(c)
    split = len(sl) > 1
    return {"drop_last_ktile": True,
            "stale_half": c.M > 64 and any(b - a > 1 for a, b in sl),
            "swap_nh": c.N >= 64,
            "swap_frag": c.N >= 32,
            "slice_overrun": split and nk % (sl[0][1] - sl[0][0]) != 0,
            "slice_gap": split and min(c.splits, nk) != len(sl),
            "round_once": not split and c.res and c.act != "drelu",
            "round_twice": split and c.res and c.act != "drelu",
            "drelu_on_acc": c.act == "drelu",
            "res_ld": c.res and c.act != "drelu" and c.M > 1}[fault]


# ---------------------------------------------------------------------------- running a case
def _band(v, dtype, dev, ld=None):
    """``v`` on ``dev`` as a view between NaN bands (one row before and after a matrix, 8 elements
    around a vector: the view stays 16-byte aligned), rows ``ld`` apart with NaN in the pad columns.
    -> (view [rows, cols], the whole buffer, which owns the memory)."""
    if v.dim() == 1:
        big = torch.full((v.numel() + 16,), float("nan"), dtype=dtype)
        big[8:-8] = v.to(dtype)
        big = big.to(dev)
        return big[8:-8], big
    ld = v.shape[1] if ld is None else ld
    big = torch.full((v.shape[0] + 2, ld), float("nan"), dtype=dtype)
    big[1:-1, :v.shape[1]] = v.to(dtype)
    big = big.to(dev)
    return big[1:-1, :v.shape[1]], big


def _launch(c, dev, raw):
    """One launch into a fresh sentinel buffer -> the whole buffer on the host, [M + 256, ldy]."""
    d = _data(c)
    M, N, Kd = c.M, c.N, c.K
    ldy = N + GAP
    x, _x = _band(d["x"], BF, dev, Kd + XPAD if raw else None)
    w, _w = _band(d["w"], BF, dev, Kd + XPAD if raw else None)
    b, _b = (None, None) if d["bias"] is None else _band(d["bias"], F32, dev)
    r, _r = (None, None) if d["res"] is None else _band(d["res"], BF, dev, N + RPAD if raw else None)
    sp = py_splits(Kd, c.splits)
    ws, _ws = (None, None) if sp == 1 else _band(torch.full((sp * M * N,), float("nan"), dtype=F64), F32, dev)
    big = torch.full((M + BT, ldy), SENT, dtype=BF, device=dev)
    if raw:
        K._hip().gemm_pp(x.data_ptr(), w.data_ptr(), K._ptr(b), K._ptr(r), big.data_ptr(), M, N, Kd, Kd + XPAD,
                         Kd + XPAD, ldy, c.coff, N + RPAD, K.act_code(c.act), c.splits, K._ptr(ws), K._stream())
    else:
        K.gemm_pp(x, w, b, r, c.act, out=big[:M], splits=c.splits, out_col=c.coff, ws=ws)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return big.cpu()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check_window(buf, c, want, what):
    """Rows < M, columns [coff, coff + N) of ``buf`` hold ``want`` bit for bit and no sentinel;
    everything else still holds the sentinel."""
    M, N, coff = c.M, c.N, c.coff
    win = buf[:M, coff:coff + N]
    if not torch.equal(_bits(win), _bits(want)):
        bad = (_bits(win) != _bits(want)).nonzero()
        tn, nk, sl = -(-N // BT), c.K // 64, _slices(c)
        lines = [f"  row {m}  column {n}  tile {m // BT * tn + n // BT} = ({m // BT}, {n // BT}) of {-(-M // BT)} x {tn}  "
                 f"K-tiles {nk} in {len(sl)} slice(s) {sl}: got {win[m, n].item()!r}, want {want[m, n].item()!r}"
                 for m, n in bad[:8].tolist()]
        pytest.fail(f"{what}: {len(bad)} of {win.numel()} elements differ\n" + "\n".join(lines))
    assert not bool((win == SENT).any()), f"{what}: sentinel left inside the output"
    rest = buf.clone()
    rest[:M, coff:coff + N] = SENT
    if not bool((rest == SENT).all()):
        m, n = (rest != SENT).nonzero()[0].tolist()
        pytest.fail(f"{what}: written outside the output window at row {m} (M = {M}), column {n} "
                    f"(window [{coff}, {coff + N}))")


# --------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("c", ALL_CASES, ids=_ids(ALL_CASES))
def test_data_make_the_properties_observable(c):
    """Conditions on the data (not measurements): the bound; ReLU zeroes >= 5 % and passes >= 5 %;
    each rounding changes some value; with a residual the first rounding changes the final result
    of some element (else ``round_once`` / ``round_twice`` could not be told apart); the ``drelu``
    mask holds zeros, negatives and positives and disagrees somewhere with the accumulator's sign."""
    r = _ref(c)
    print(f"{c.name}: peak {r.peak:.0f} " + " ".join(f"{k} {v:.3f}" for k, v in r.shares.items()))
    assert r.peak < EXACT
    assert _unobservable(c, r.shares) == []
    assert torch.equal(r.out.to(BF).to(F64), r.out) and torch.equal(r.exact.to(F32).to(F64), r.exact)
    for k in ("x", "w", "res"):
        v = _data(c)[k]
        assert v is None or (torch.equal(v.to(BF).to(F64), v) and not bool((v.signbit() & (v == 0)).any())), k
    b = _data(c)["bias"]
    assert b is None or (bool((b < 0).any()) and bool((b > 0).any()) and torch.equal(b * 2, (b * 2).round()))


@pytest.mark.parametrize("c", ALL_CASES, ids=_ids(ALL_CASES))
def test_reference_equals_host_path_where_it_does_not_round(c):
    """``K.gemm_pp`` on host tensors computes in fp32 (exact here) and rounds nowhere into fp32."""
    d = _data(c)
    f = lambda k: None if d[k] is None else d[k].to(F32)   # noqa: E731
    got = K.gemm_pp(f("x"), f("w"), f("bias"), f("res"), c.act, splits=c.splits)
    assert got.dtype == F32 and tuple(got.shape) == (c.M, c.N)
    assert torch.equal(got.to(F64), _ref(c).exact)


def test_host_path_into_a_strided_bf16_out_rounds_once():
    """The host path writes ``out=`` windows like the kernel but rounds once: on the direct path
    with a residual it equals ``round_once``, on the split path the reference itself."""
    for c in (next(c for c in CASES if c.res and c.splits == 1 and c.M > 128),
              next(c for c in CASES if c.res and c.splits == 2), CASES_DRELU[0]):
        split = py_splits(c.K, c.splits) > 1
        want = (_ref(c) if split or c.act == "drelu" else _reference(c, "round_once")).out.to(BF)
        _check_window(_launch(c, torch.device("cpu"), raw=False), c, want, c.name)


@pytest.mark.parametrize("fault", FAULTS)
def test_wrong_variants_differ(fault):
    hit = 0
    for c in ALL_CASES:
        if _applies(fault, c):
            assert not torch.equal(_reference(c, fault).out, _ref(c).out), f"{fault} goes unnoticed on {c.name}"
            hit += 1
    assert hit >= 1, f"{fault} applies to no case"


def test_case_list_covers_every_path():
    shapes = {(c.M, c.N, c.K, c.splits) for c in ALL_CASES}
    tiles = lambda s: -(-s[0] // BT) * -(-s[1] // BT)   # noqa: E731
    sl = {s: _slices(_Case("", *s, None, True, False, 0)) for s in shapes}
    assert any(s[:3] == (1, 8, 64) for s in shapes)
    assert any(128 < s[0] <= 192 and s[0] % 128 == 1 and s[1] % 64 and s[1] // 64 % 2 == 1 for s in shapes)
    assert any(tiles(s) == 4 and s[0] % BT == 1 and s[1] % BT == 8 and s[2] // 64 % 2 == 1 for s in shapes)
    assert {s[2] // 64 for s in shapes if s[3] == 1} >= {1, 2, 3, 4, 5}
    assert any(s[0] <= 64 and s[2] // 64 == 4 for s in shapes) and any(s[0] <= 128 for s in shapes)
    assert any(tiles(s) > 8 and tiles(s) % 8 for s in shapes) and max(map(tiles, shapes)) <= 12
    assert max(s[2] for s in shapes) <= 1600
    lens = {tuple(b - a for a, b in v) for v in sl.values()}
    assert {(3, 2), (2, 2, 1), (1, 1)} <= lens                                        # unequal and single-tile slices
    assert any(s[3] == 4 and len(sl[s]) == 3 for s in shapes)                         # recomputed slice count
    assert any(s[3] > s[2] // 64 and len(sl[s]) == 1 for s in shapes)                 # the fallback to the direct path
    assert any(len(v) > 1 and v[-1][1] - v[-1][0] == 1 and v[-1][0] for v in sl.values())   # nk == 1 at kt0 != 0
    for s in SHAPES:
        combos = {(c.bias, c.res, c.act) for c in CASES if (c.M, c.N, c.K, c.splits) == s}
        assert combos == set(itertools.product((True, False), (True, False), (None, "relu"))), s
    assert {len(_slices(c)) > 1 for c in CASES_DRELU} == {True, False}
    assert sum(c.coff != 0 for c in ALL_CASES) * 2 >= len(ALL_CASES)
    for nk in range(1, 13):     # the slice walk used above against the library's formula, in Python
        for s in range(0, 17):
            c = _Case("", 1, 8, 64 * nk, s, None, True, False, 0)
            assert len(_slices(c)) == py_splits(64 * nk, s) and _slices(c)[-1][1] == nk


# --------------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("c", ALL_CASES, ids=_ids(ALL_CASES))
def test_gemm_pp_gpu(c):
    dev = torch.device("cuda", 0)
    want = _ref(c).out.to(BF)
    sl = _slices(c)
    what = f"{c.name} ({-(-c.M // BT)} x {-(-c.N // BT)} tiles, {c.K // 64} K-tiles, slices {sl})"
    _check_window(_launch(c, dev, raw=False), c, want, what + " K.gemm_pp")
    _check_window(_launch(c, dev, raw=True), c, want, what + f" raw entry, ldx = ldw = K + {XPAD}, ldr = N + {RPAD}")


@pytest.mark.gpu
@pytest.mark.parametrize("path", ("direct", "zero-residual", "split"))
@pytest.mark.parametrize("act", ("gelu", "tanh"))
def test_transcendental_activations_gpu(act, path):
    """K = N = 64, M = 5: ``y[m, n] = act(x[m, perm[n]])`` exactly on the kept inputs, each of which
    occurs in the output."""
    dev = torch.device("cuda", 0)
    vals = _kept(act)
    g = torch.Generator().manual_seed(11)
    M, N = 5, 64
    assert len(vals) <= M * N
    x = vals[torch.arange(M * N) % len(vals)][torch.randperm(M * N, generator=g)].reshape(M, N)
    perm = torch.randperm(N, generator=g)
    w = torch.zeros(N, N, dtype=F64)
    w[torch.arange(N), perm] = 1
    res = ws = None
    if path == "zero-residual":
        res = torch.zeros(M, N, dtype=BF, device=dev)
    if path == "split":     # the permutation in the first slice, zeros in the second
        x, w = torch.cat([x, torch.zeros(M, 64, dtype=F64)], 1), torch.cat([w, torch.zeros(N, 64, dtype=F64)], 1)
        ws = torch.full((2 * M * N,), float("nan"), dtype=F32, device=dev)
    big = torch.full((M + BT, N), SENT, dtype=BF, device=dev)
    K.gemm_pp(x.to(BF).to(dev), w.to(BF).to(dev), None, res, act, out=big[:M], splits=2 if path == "split" else 1, ws=ws)
    torch.cuda.synchronize()
    got, pre = big.cpu(), x[:, :N][:, perm]
    want = _act64(pre, act).to(BF)
    assert set(pre.reshape(-1).tolist()) == set(vals.tolist())
    assert bool((got[M:] == SENT).all())
    if not torch.equal(_bits(got[:M]), _bits(want)):
        bad = (_bits(got[:M]) != _bits(want)).nonzero()
        lines = []
        for m, n in bad[:8].tolist():
            f, y = _act64(pre[m, n], act).item(), got[m, n].item()
            lines.append(f"  x = {pre[m, n].item()}: got {y!r}, want {want[m, n].item()!r}, float64 {f!r}, "
                         f"relative error of the stored value {abs(y - f) / max(abs(f), 1e-300):.3e}")
        pytest.fail(f"{act} {path}: {len(bad)} of {M * N} differ\n" + "\n".join(lines))


# ----------------------------------------------------------------- host-side argument checks
_RAW_ARGS = ("x", "w", "bias", "res", "y", "M", "N", "K", "ldx", "ldw", "ldy", "y_coff", "ldr", "act", "splits", "ws",
             "stream")
# every ``invalid_argument`` of ``gemm_pp``: the arguments changed from the good launch.  "+n" = that
# pointer moved by n bytes, "res" / "ws" = that buffer's pointer is passed.
BAD_RAW = {
    "empty-M": dict(M=0), "empty-N": dict(N=0), "empty-K": dict(K=0),
    "K%64": dict(K=96, ldx=96, ldw=96),
    "N%8": dict(N=12), "ldy%8": dict(ldy=44), "y_coff%8": dict(y_coff=4), "ldx%8": dict(ldx=68), "ldw%8": dict(ldw=68),
    "ldr%8": dict(res="res", ldr=12),
    "x-2GiB": dict(M=1 << 20, ldx=1024), "w-2GiB": dict(N=1 << 20, ldw=1024, ldy=(1 << 20) + 8),
    "x+2": dict(x="+2"), "w+2": dict(w="+2"), "y+2": dict(y="+2"), "bias+4": dict(bias="+4"), "res+2": dict(res="res+2"),
    "split-without-workspace": dict(K=128, ldx=128, ldw=128, splits=2),
    "ws+4": dict(K=128, ldx=128, ldw=128, splits=2, ws="ws+4"),
    "drelu-without-mask": dict(act=K.ACT_DRELU),
    "act-sigmoid": dict(act=K.ACT_SIGMOID), "act-relu6": dict(act=K.ACT_RELU6), "act-99": dict(act=99),
}
_RAW_REASON = {"empty": "empty problem", "K%64": "multiple of 64", "%8": "alignment", "2GiB": "larger than 2 GiB",
               "split-without": "needs a workspace", "+": "16-byte aligned", "drelu": "needs the mask", "act": "unsupported"}


@functools.lru_cache(maxsize=None)
def _arg_env():
    """Buffers far larger than the 16 x 8 x 64 problem needs, y filled with the sentinel."""
    dev = torch.device("cuda", 0)
    env = {k: torch.zeros(1 << 16, dtype=BF, device=dev) for k in ("x", "w", "res")}
    env["bias"] = torch.zeros(1 << 12, dtype=F32, device=dev)
    env["ws"] = torch.zeros(1 << 16, dtype=F32, device=dev)
    env["y"] = torch.full((1 << 16,), SENT, dtype=BF, device=dev)
    return env


def _raw_call(changes):
    ptr = {k: t.data_ptr() for k, t in _arg_env().items()}
    a = dict(x=ptr["x"], w=ptr["w"], bias=ptr["bias"], res=0, y=ptr["y"], M=16, N=8, K=64, ldx=64, ldw=64, ldy=16,
             y_coff=8, ldr=8, act=K.ACT_RELU, splits=1, ws=0, stream=K._stream())
    for k, v in changes.items():
        if isinstance(v, str):
            name, _, off = v.partition("+")
            a[k] = ptr[name or k] + int(off or 0)
        else:
            a[k] = v
    K._hip().gemm_pp(*[a[k] for k in _RAW_ARGS])


def _bad_launches(dev):
    """(good keyword arguments of ``K.gemm_pp``, [(what, overrides)]) for every refusal of the wrapper."""
    z = lambda *s, dtype=BF, device=dev: torch.zeros(s, dtype=dtype, device=device)   # noqa: E731
    cpu = torch.device("cpu")
    good = dict(x=z(16, 128), w_nk=z(8, 128), bias=z(8, dtype=F32), residual=z(16, 8), act="relu", out=z(16, 24),
                splits=2, out_col=8, ws=z(2 * 16 * 8, dtype=F32))
    bad = [("K mismatch", dict(w_nk=z(8, 64))), ("out rows", dict(out=z(15, 24))), ("window past the row", dict(out_col=24)),
           ("residual size", dict(residual=z(16, 16))), ("K % 64", dict(x=z(16, 96), w_nk=z(8, 96))),
           ("N % 8", dict(w_nk=z(12, 128), bias=z(12, dtype=F32), residual=z(16, 12))), ("ldy % 8", dict(out=z(16, 28))),
           ("out_col % 8", dict(out_col=4)), ("x dtype", dict(x=z(16, 128, dtype=F32))),
           ("w dtype", dict(w_nk=z(8, 128, dtype=F32))), ("out dtype", dict(out=z(16, 24, dtype=F32))),
           ("bias dtype", dict(bias=z(8))), ("residual dtype", dict(residual=z(16, 8, dtype=F32))),
           ("x not contiguous", dict(x=z(16, 256)[:, ::2])), ("w not contiguous", dict(w_nk=z(8, 256)[:, ::2])),
           ("residual not contiguous", dict(residual=z(16, 16)[:, ::2])), ("out not contiguous", dict(out=z(16, 48)[:, ::2])),
           ("bias not contiguous", dict(bias=z(16, dtype=F32)[::2])), ("w device", dict(w_nk=z(8, 128, device=cpu))),
           ("out device", dict(out=z(16, 24, device=cpu))), ("bias device", dict(bias=z(8, dtype=F32, device=cpu))),
           ("residual device", dict(residual=z(16, 8, device=cpu))), ("ws dtype", dict(ws=z(2 * 16 * 8))),
           ("ws too small", dict(ws=z(2 * 16 * 8 - 1, dtype=F32))), ("ws device", dict(ws=z(2 * 16 * 8, dtype=F32, device=cpu))),
           ("unknown activation", dict(act="swish")), ("sigmoid", dict(act="sigmoid")), ("relu6", dict(act="relu6")),
           ("drelu without mask", dict(act="drelu", residual=None))]
    return good, bad


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch_gpu():
    """Every ``invalid_argument`` of ``gemm_pp`` and every ``ValueError`` / ``TypeError`` of ``K.gemm_pp``
    is raised by a launch that differs from an accepted one in that respect alone; nothing is written.
    ``gemm_pp_splits`` of the library equals the Python formula."""
    y = _arg_env()["y"]
    _raw_call({})
    _raw_call(dict(K=128, ldx=128, ldw=128, splits=2, ws="ws"))
    _raw_call(dict(act=K.ACT_DRELU, res="res"))
    torch.cuda.synchronize()
    got = y.cpu()
    y.fill_(SENT)
    assert bool((got[:16 * 16].reshape(16, 16)[:, 8:] == 0).all()) and bool((got[16 * 16:] == SENT).all())
    for what, changes in BAD_RAW.items():
        reason = next(msg for key, msg in _RAW_REASON.items() if key in what)
        with pytest.raises(ValueError, match=reason):
            _raw_call(changes)
            pytest.fail(f"not refused: {what}")
    torch.cuda.synchronize()
    assert bool((y == SENT).all()), "a refused raw launch wrote the output"
    good, bad = _bad_launches(torch.device("cuda", 0))
    good["out"].fill_(SENT)
    for what, over in bad:
        with pytest.raises((ValueError, TypeError)):
            K.gemm_pp(**{**good, **over})
            pytest.fail(f"not refused: {what}")
    torch.cuda.synchronize()
    assert bool((good["out"] == SENT).all()), "a refused launch wrote the output"
    K.gemm_pp(**good)
    torch.cuda.synchronize()
    assert bool((good["out"][:, 8:16] == 0).all()) and bool((good["out"][:, :8] == SENT).all())
    for nk in range(1, 13):
        for s in range(0, 17):
            assert K._hip().gemm_pp_splits(64 * nk, s) == py_splits(64 * nk, s), (nk, s)


def test_wrapper_refusals_that_need_no_gpu():
    """The shape checks of ``K.gemm_pp`` come before the device branch."""
    good, bad = _bad_launches(torch.device("cpu"))
    host = {"K mismatch", "out rows", "window past the row", "residual size", "unknown activation", "drelu without mask"}
    for what, over in bad:
        if what in host:
            with pytest.raises(ValueError):
                K.gemm_pp(**{**good, **over})
                pytest.fail(f"not refused: {what}")
