"""The training GEMM of ``kernels/gemm_train.hip``, bit for bit: K tails, both rings, split-K,
the column sums and their reduction.

The operands are integers that are exact in bf16, the bias is fp32 integers, and the amplitude
is chosen per K so that every product and every partial sum stays below 2^24: fp32
accumulation is then exact in any order and in any split, and the only inexact step is the
kernel's one bf16 rounding.  The float64 reference rounds where the kernel rounds:

non-split epilogue
    ``r = bf16(acc + bias)``, then ReLU or the mask (``mask > 0 ? r : 0``) on the rounded value.
split-K reduce
    the slabs summed in order, ``+ bias``, ReLU or mask, then one rounding.  The two agree
    (ReLU and the mask commute with the rounding), and ``test_split_and_unsplit_references_agree``
    asserts it.
column sums
    ``colsum[t]`` = the sum of the stored bf16 rows of 128-row tile t (amplitude chosen so that
    128 of them stay below 2^24 too); ``colsum_reduce`` sums rows of integers.

Every tensor a kernel sees is a view inside a larger allocation.  Inputs are surrounded by
poison (2^60, and NaN in a second parametrisation: ``0 * NaN`` shows where ``0 * 2^60`` does
not), in the rows before and after the view (``GUARD`` >= one K tile after it, so a mis-clipped
read of a partial K tile shows as a wrong value) and in the gap columns of the row stride.
Outputs, the split workspace and the column sums are surrounded by a sentinel that must be
intact afterwards.  Before every case with a partial last K tile the same kernel variant runs
on all-nonzero data with K rounded up to 64 and the same grid, so that an out-of-range DMA
lane that skipped its LDS write would leave non-zero bytes behind.

The ring (4 stages when ``tiles * splits <= CUs``, else 2) is decided from the device's CU
count with ``launch_tr``'s expression, and each case asserts the ring it is meant to hit.

The non-GPU tests check the reference alone: against the ``K.*`` host paths where nothing
rounds, that the data make the rounding, ReLU and mask observable, that the exactness bound
holds, and that each deliberately wrong variant (``FAULTS``) differs on every case it applies to."""
import collections
import functools
import math
import zlib

import pytest
import torch

from flink_tensorflow_amd.ops import kernels as K

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EXACT = 2 ** 24          # integers below this are exact in fp32
SENT = -77.0             # output sentinel, exact in bf16
POISON = {"big": 2.0 ** 60, "nan": float("nan")}
FRONT, GUARD = 8, 72     # poison / sentinel rows before and after every view (GUARD >= 64 + 128-column spill)
GAP = 24                 # gap columns of every row-strided view
FAULTS = ("poison_tail", "drop_chunk", "stale_stage", "swap_m", "swap_n", "wrong_layout_x", "wrong_layout_w",
          "split_drop", "split_twice", "bias_late", "mask_ge", "colsum_no_tail")
LAYOUTS = [(False, False), (False, True), (True, True), (True, False)]  # (x_t, w_t): NT, dX, dW, TN


def _cus():
    """CU count the ring is chosen from (256 where no GPU is visible: the data tests still run)."""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _ring(M, N, splits):
    tiles = -(-M // 128) * -(-N // 128)
    return 4 if tiles * (splits if splits > 1 else 1) <= _cus() else 2  # launch_tr's ``deep``


def _splits_used(Kd, s):
    nk = -(-Kd // 64)
    if s <= 1 or nk <= 1:
        return 1
    per = -(-nk // min(s, nk))
    return -(-nk // per)


# ----------------------------------------------------------------------------------- cases
_Case = collections.namedtuple("_Case", "name M N K x_t w_t epi ring splits split_ring colsum amp grid",
                               defaults=((), None, False, None, None))


def _lay(x_t, w_t):
    return ("T" if x_t else "N") + ("N" if w_t else "T")  # NT forward, NN dX, TN dW, TT


def _mk(tag, M, N, Kd, x_t, w_t, epi, ring, **kw):
    shape = f"{M}x{N}x{Kd}" if kw.get("grid") is None else f"{kw['grid']}-K{Kd or 'deep'}"  # grid: sized from the CUs
    return _Case(f"{tag}-{_lay(x_t, w_t)}-{shape}-{epi}", M, N, Kd, x_t, w_t, epi, ring, **kw)


K_LADDER = (8, 56, 64, 72, 128, 136, 192, 200, 256, 264, 320, 328)
CASES_LADDER = [_mk("ladder", 200, 72, k, xt, wt, "f32", 4) for xt, wt in LAYOUTS for k in K_LADDER]
CASES_LADDER += [_mk("ladder", 200, 132, 200, xt, wt, "f32", 4) for xt, wt in LAYOUTS]
# grid just above the CU count (M, N filled in from the device by _resolve)
CASES_WIDE = [_mk("ring2", 0, 0, k, xt, wt, "f32", 2, grid="wide") for xt, wt in LAYOUTS for k in (8, 72, 200)]
CASES_WIDE += [_mk("ring2", 0, 0, k, False, False, "bf16_bias_relu", 2, grid="wide") for k in (8, 72, 200)]
CASES_EPI = [_mk("epi", 200, 72, k, False, wt, epi, 4, splits=(2, 3))
             for k in (72, 200) for wt, epi in ((False, "bf16"), (False, "bf16_bias"), (False, "bf16_bias_relu"),
                                                (True, "bf16_mask"))]
CASES_SPLIT = [_mk("split", 200, 72, 328, True, True, "f32", 4, splits=(2, 4, 5, 6, 9)),
               _mk("split", 200, 72, 264, True, True, "f32", 4, splits=(2, 3, 4)),   # 5 tiles: uneven slices
               _mk("split", 200, 72, 72, True, True, "f32", 4, splits=(2,)),
               _mk("split", 0, 72, 0, True, True, "f32", 4, splits=("nk+1",), split_ring=2, grid="tall_split")]
CASES_COLSUM = [_mk("colsum", M, N, 72, False, True, epi, 4, colsum=True, amp=16)
                for M in (200, 384) for N in (72, 136) for epi in ("bf16", "bf16_mask")]
CASES_COLSUM += [_mk("colsum", 0, 72, 72, False, True, "bf16_mask", 2, colsum=True, amp=16, grid="tall")]
ALL_CASES = CASES_LADDER + CASES_WIDE + CASES_EPI + CASES_SPLIT + CASES_COLSUM


def _ids(cases):
    return [c.name for c in cases]


def _resolve(c):
    """Fills in the shapes that depend on the CU count."""
    cus = _cus()
    if c.grid == "wide":      # (cus // 16 + 1) x 16 tiles, both with tails: 272 tiles on 256 CUs
        c = c._replace(M=(cus // 16 + 1) * 128 - 120, N=16 * 128 - 120)
    elif c.grid == "tall":    # cus + 1 tiles in one column
        c = c._replace(M=(cus + 1) * 128 - 56)
    elif c.grid == "tall_split":  # 17 x 1 tiles, one K tile per slice: 17 * nk just above the CU count
        nk = cus // 17 + 3
        c = c._replace(M=17 * 128 - 120, K=(nk - 1) * 64 + 8, splits=(nk + 1,))
    return c


def _amp(c):
    return c.amp or max(1, min(127, math.isqrt(2 ** 22 // c.K)))


_Data = collections.namedtuple("_Data", "x w bias mask")


@functools.lru_cache(maxsize=None)
def _data(c):
    """The case's operands as stored (float64 integers): x [M, K] or [K, M], w [N, K] or [K, N]."""
    g = torch.Generator().manual_seed(zlib.crc32(repr(tuple(c)).encode()))
    a = _amp(c)

    def ints(lo, hi, shape):
        return torch.randint(lo, hi + 1, shape, generator=g).to(F64)

    x = ints(-a, a, (c.K, c.M) if c.x_t else (c.M, c.K))
    w = ints(-a, a, (c.K, c.N) if c.w_t else (c.N, c.K))
    bias = ints(-2000, 2000, (c.N,)) if "bias" in c.epi else None
    mask = None
    if "mask" in c.epi:       # +0, -0, negatives and positives
        mask = ints(-3, 3, (c.M, c.N))
        neg0 = (mask == 0) & (torch.rand(mask.shape, generator=g) < 0.5)
        mask = torch.where(neg0, torch.full_like(mask, -0.0), mask)
    return _Data(x, w, bias, mask)


# --------------------------------------------------------------------------- guarded memory
def _ld(cols, mult):
    return -(-(cols + GAP) // mult) * mult


class _Slot:
    """A [rows, cols] view with row stride ``ld`` inside an allocation filled with ``fill``."""

    def __init__(self, vals, shape, ld, fill, dtype, dev, front=FRONT, back=GUARD):
        self.rows, self.cols, self.ld, self.dtype, self.front = shape[0], shape[1], ld, dtype, front
        self.buf = torch.full((front + self.rows + back, ld), fill, dtype=dtype)
        if vals is not None:
            self.buf[front:front + self.rows, :self.cols] = vals.to(dtype)
        self.dev = self.buf.to(dev)
        self.view = self.dev[front:front + self.rows, :self.cols]
        self.base = front * ld

    def logical(self, t, mn, Kd):
        """Element (m, k) of a [mn, Kd] operand read from this memory in layout ``t`` — the view's
        own values inside it, poison (or the next row) outside."""
        flat = self.buf.reshape(-1).to(F64)
        m, k = torch.arange(mn)[:, None], torch.arange(Kd)[None, :]
        idx = self.base + (k * self.ld + m if t else m * self.ld + k)
        return flat[idx % flat.numel()]

    def assert_surroundings_intact(self, what):
        bits = torch.int32 if self.dtype == F32 else torch.int16
        got = self.dev.cpu().clone()
        got[self.front:self.front + self.rows, :self.cols] = self.buf[0, 0]
        assert torch.equal(got.view(bits), torch.full_like(self.buf, self.buf[0, 0].item()).view(bits)), \
            f"{what}: written outside the view"


class _Mem:
    def __init__(self, c, poison, dev):
        d, p = _data(c), POISON[poison]
        self.c, self.dev = c, dev
        self.x = _Slot(d.x, d.x.shape, _ld(d.x.shape[1], 8), p, BF, dev)
        self.w = _Slot(d.w, d.w.shape, _ld(d.w.shape[1], 8), p, BF, dev)
        self.bias = None if d.bias is None else _Slot(d.bias[None], (1, c.N), _ld(c.N, 4), p, F32, dev)
        self.mask = None if d.mask is None else _Slot(d.mask, d.mask.shape, _ld(c.N, 8), p, BF, dev)
        self.f32 = c.epi == "f32"

    def out_slot(self):
        c = self.c
        return _Slot(None, (c.M, c.N), _ld(c.N, 8), SENT, F32 if self.f32 else BF, self.dev)

    def launch(self, splits=1):
        """One ``K.gemm_train`` call into fresh sentinel-filled slots -> (out, colsum or None) on the host."""
        c = self.c
        out = self.out_slot()
        used = _splits_used(c.K, splits)
        ws = _Slot(None, (1, used * c.M * c.N), used * c.M * c.N + 64, SENT, F32, self.dev, 1, 1) if used > 1 else None
        cs = _Slot(None, (-(-c.M // 128), c.N), c.N, SENT, F32, self.dev) if c.colsum else None
        K.gemm_train(self.x.view, self.w.view, x_t=c.x_t, w_t=c.w_t,
                     bias=None if self.bias is None else self.bias.view[0],
                     mask=None if self.mask is None else self.mask.view,
                     act="relu" if "relu" in c.epi else None, out=out.view, splits=splits,
                     ws=None if ws is None else ws.view[0], colsum=None if cs is None else cs.view)
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        for s, nm in ((out, "out"), (ws, "split workspace"), (cs, "colsum")):
            if s is not None:
                s.assert_surroundings_intact(f"{c.name}: {nm}")
        return out.view.cpu(), None if cs is None else cs.view.cpu()


# -------------------------------------------------------------------------------- reference
def _bf(v):
    """bf16 round-to-nearest-even of float64 integers below 2^24 (float64 -> fp32 is exact)."""
    return v.to(BF).to(F64)


_Ref = collections.namedtuple("_Ref", "out colsum peak changed zeroed kept")


def ref_gemm(mem, splits=1, fault=None):
    """float64 mirror of ``gemm_train`` on ``mem``'s operands -> ``_Ref`` (out [M, N] float64 holding
    the fp32 or bf16 values).  ``splits`` = slices actually run.  Faults: see ``_applies``."""
    c = mem.c
    M, N, Kd = c.M, c.N, c.K
    nk = -(-Kd // 64)
    Kp = nk * 64 if fault == "poison_tail" else Kd       # partial K tile not zeroed
    Mp = -(-M // 128) * 128 if fault == "colsum_no_tail" else M
    X = mem.x.logical(c.x_t != (fault == "wrong_layout_x"), Mp, Kp)
    W = mem.w.logical(c.w_t != (fault == "wrong_layout_w"), N, Kp)
    if fault == "drop_chunk":                            # one 8-element K chunk of one fragment
        k0 = 8 if Kd >= 16 else 0
        X[16:32, k0:k0 + 8] = 0
    if fault == "stale_stage":                           # K tile kt read one stage early
        Y = X.clone()
        for kt in range(1, nk):
            wd = min(64, Kd - kt * 64)
            Y[:, kt * 64:kt * 64 + wd] = X[:, (kt - 1) * 64:(kt - 1) * 64 + wd]
        X = Y
    bias = torch.zeros(N, dtype=F64) if mem.bias is None else mem.bias.buf[FRONT, :N].to(F64)
    peak = float((X.abs() @ W.abs().t() + bias.abs()).max()) if fault is None else 0.0
    per = -(-nk // splits)
    slabs = [X[:, s * per * 64:(s + 1) * per * 64] @ W[:, s * per * 64:(s + 1) * per * 64].t() for s in range(splits)]
    if fault == "split_drop":
        slabs = slabs[:-1]
    if fault == "split_twice":
        slabs = slabs + slabs[:1]
    acc = sum(slabs[1:], slabs[0])
    for f, dim in (("swap_m", 0), ("swap_n", 1)):        # two 16-wide fragments of the tail tile
        if fault == f:
            n = acc.shape[dim]
            r0 = (n - 1) // 128 * 128 if n - (n - 1) // 128 * 128 >= 32 else 0
            perm = torch.arange(n)
            perm[r0:r0 + 32] = torch.cat([torch.arange(r0 + 16, r0 + 32), torch.arange(r0, r0 + 16)])
            acc = acc.index_select(dim, perm)
    v = acc + bias
    if c.epi == "f32":
        return _Ref(v, None, peak, 0.0, 0.0, 1.0)
    mask = None if mem.mask is None else mem.mask.buf[FRONT:FRONT + M, :N].to(F64)
    if mask is not None and Mp > M:
        mask = torch.cat([mask, torch.ones(Mp - M, N, dtype=F64)])

    def act(t):
        if mask is not None:
            return torch.where((mask >= 0) if fault == "mask_ge" else (mask > 0), t, torch.zeros_like(t))
        return torch.relu(t) if "relu" in c.epi else t

    r = _bf(v)
    if fault == "bias_late":
        out = _bf(act(acc) + bias)
    elif splits > 1:
        out = _bf(act(v))
    else:
        out = act(r)
    colsum = None
    if c.colsum:
        tiles = -(-M // 128)
        colsum = torch.stack([out[t * 128:(t + 1) * 128].sum(0) for t in range(tiles)])
        if fault is None:
            peak = max(peak, float(torch.stack([out[t * 128:(t + 1) * 128].abs().sum(0) for t in range(tiles)]).max()))
    out = out[:M]
    changed = (r[:M] != v[:M]).double().mean().item()
    zeroed = ((out == 0) & (r[:M] != 0)).double().mean().item()
    kept = (out != 0).double().mean().item()
    return _Ref(out, colsum, peak, changed, zeroed, kept)


def _applies(fault, c, splits):
    nk = -(-c.K // 64)
    return {"poison_tail": c.K % 64 != 0, "drop_chunk": True, "stale_stage": nk >= 2, "swap_m": True, "swap_n": True,
            "wrong_layout_x": True, "wrong_layout_w": True, "split_drop": splits > 1, "split_twice": splits > 1,
            "bias_late": c.epi == "bf16_bias_relu", "mask_ge": "mask" in c.epi,
            "colsum_no_tail": c.colsum and c.M % 128 != 0}[fault]


def ref_colsum_reduce(part, fault=None):
    """``out[n] = sum_t part[t, n]``.  Fault: stop after the 8-way unrolled part of each wave's loop
    (wave w owns t = w, w + 4, ...; a round of 8 runs while ``t + 28 < T``)."""
    T = part.shape[0]
    if fault == "unrolled_only":
        rows = [t + 4 * u for w in range(4) for t in range(w, T, 32) if t + 28 < T for u in range(8)]
        return part[rows].sum(0) if rows else torch.zeros(part.shape[1], dtype=F64)
    return part.sum(0)


def _as_out(ref, f32):
    return ref.to(F32) if f32 else ref.to(BF)


def _assert_equal(got, ref, what):
    """``torch.equal`` with a report that names, for the first mismatches, the tile, the wave, the
    16x16 fragment and the lane row / quad that own the element."""
    if torch.equal(got, ref):
        return
    bad = (got != ref).nonzero()
    lines = []
    for m, n in bad[:8].tolist():
        ml, nl = m % 128, n % 128
        lines.append(f"  (m, n) = ({m}, {n})  tile ({m // 128}, {n // 128})  wave ({ml // 64}, {nl // 64})  "
                     f"fragment ({ml % 64 // 16}, {nl % 64 // 16})  lane row {ml % 16} quad {nl % 16 // 4}: "
                     f"got {got[m, n].item()!r}, expected {ref[m, n].item()!r}")
    pytest.fail(f"{what}: {len(bad)} of {got.numel()} elements differ\n" + "\n".join(lines))


# --------------------------------------------------------------------------------- CPU tests
CPU = torch.device("cpu")


@pytest.mark.parametrize("x_t,w_t", LAYOUTS)
def test_reference_equals_host_path_fp32(x_t, w_t):
    c = _mk("host", 200, 72, 200, x_t, w_t, "f32", 4)
    mem = _Mem(c, "big", CPU)
    got, _ = mem.launch()
    ref = ref_gemm(mem)
    assert ref.peak < EXACT
    assert torch.equal(got.to(F64), ref.out)


def test_colsum_reference_equals_host_paths():
    c = _mk("host", 200, 72, 72, False, True, "bf16_mask", 4, colsum=True, amp=16)
    mem = _Mem(c, "big", CPU)
    got, cs = mem.launch()
    ref = ref_gemm(mem)
    assert torch.equal(got.to(F64), ref.out) and torch.equal(cs.to(F64), ref.colsum)
    wide = torch.full((5, 96), float("nan"))
    wide[:, 16:88] = torch.randint(-1000, 1001, (5, 72), generator=torch.Generator().manual_seed(5)).float()
    out = torch.full((72,), SENT)
    K.colsum_reduce(wide[:, 16:88], out)
    assert torch.equal(out.to(F64), ref_colsum_reduce(wide[:, 16:88].to(F64)))


@pytest.mark.parametrize("c", ALL_CASES, ids=_ids(ALL_CASES))
def test_data_make_the_properties_observable(c):
    c = _resolve(c)
    mem = _Mem(c, "big", CPU)
    ref = ref_gemm(mem)
    print(f"{c.name}: amp {_amp(c)} peak {ref.peak:.0f} changed {ref.changed:.3f} zeroed {ref.zeroed:.3f} "
          f"kept {ref.kept:.3f}")
    assert ref.peak < EXACT, "an intermediate is not exact in fp32"
    assert torch.equal(ref.out.float().to(F64), ref.out)
    if c.epi != "f32":
        assert ref.changed >= 0.10, "the bf16 rounding changes too few outputs"
    if "relu" in c.epi or "mask" in c.epi:
        assert ref.zeroed >= 0.10 and ref.kept >= 0.10
    if "mask" in c.epi:
        mk = mem.mask.view
        z = mk == 0
        assert (z & mk.signbit()).any() and (z & ~mk.signbit()).any() and (mk < 0).any() and (mk > 0).any()


@pytest.mark.parametrize("c", CASES_EPI + CASES_SPLIT, ids=_ids(CASES_EPI + CASES_SPLIT))
def test_split_and_unsplit_references_agree(c):
    c = _resolve(c)
    mem = _Mem(c, "big", CPU)
    one = ref_gemm(mem).out
    for s in c.splits:
        used = _splits_used(c.K, s)
        assert used > 1
        assert torch.equal(ref_gemm(mem, splits=used).out, one)


@pytest.mark.parametrize("fault", FAULTS)
def test_wrong_variants_differ(fault):
    """Each wrong variant of the reference changes the output (or the column sums) of every case
    it applies to, under either poison where poison is what it reads."""
    hit = 0
    for c0 in ALL_CASES:
        c = _resolve(c0)
        for s in (1,) + tuple(c.splits):
            used = _splits_used(c.K, s)
            if (s > 1) != (fault.startswith("split_")) or not _applies(fault, c, used):
                continue
            for poison in (("big", "nan") if fault in ("poison_tail", "wrong_layout_x", "wrong_layout_w") else ("big",)):
                mem = _Mem(c, poison, CPU)
                good, bad = ref_gemm(mem, splits=used), ref_gemm(mem, splits=used, fault=fault)
                if fault == "colsum_no_tail":
                    same = torch.equal(_as_out(good.colsum, True), _as_out(bad.colsum, True))
                else:
                    same = torch.equal(_as_out(good.out, c.epi == "f32"), _as_out(bad.out, c.epi == "f32"))
                assert not same, f"{fault} goes unnoticed on {c.name} (splits {s}, poison {poison})"
                hit += 1
    assert hit > 0


CSR_T = (1, 2, 3, 4, 5, 28, 29, 32, 33, 36, 37, 64, 65, 70)
CSR_N = (8, 64, 72, 200)


def _csr_part(T, N):
    g = torch.Generator().manual_seed(1000 * T + N)
    return torch.randint(-1000, 1001, (T, N), generator=g).to(F64)


def test_colsum_reduce_wrong_variant_differs():
    for T in CSR_T:
        for N in CSR_N:
            part = _csr_part(T, N)
            assert float(part.abs().sum(0).max()) < EXACT
            if T % 32:  # a remainder exists
                assert not torch.equal(ref_colsum_reduce(part), ref_colsum_reduce(part, "unrolled_only")), (T, N)
            else:
                assert torch.equal(ref_colsum_reduce(part), ref_colsum_reduce(part, "unrolled_only")), (T, N)


# --------------------------------------------------------------------------------- GPU tests
def _dev():
    return torch.device("cuda", 0)


def _prelaunch(c, splits):
    """Stale-LDS probe: the same kernel variant (layout, epilogue, ring, split) and grid on
    all-nonzero data with K rounded up to a whole number of K tiles."""
    dev, K64 = _dev(), -(-c.K // 64) * 64
    assert _splits_used(K64, splits) == _splits_used(c.K, splits)
    def full(rows, cols, v):  # row stride rounded up to 8 elements (N = 132 K-major)
        return torch.full((rows, -(-cols // 8) * 8), v, dtype=BF, device=dev)[:, :cols]

    x = full(*((K64, c.M) if c.x_t else (c.M, K64)), 3.0)
    w = full(*((K64, c.N) if c.w_t else (c.N, K64)), 5.0)
    f32 = c.epi == "f32"
    y = K.gemm_train(x, w, x_t=c.x_t, w_t=c.w_t, bias=torch.ones(c.N, device=dev) if "bias" in c.epi else None,
                     mask=torch.ones(c.M, c.N, dtype=BF, device=dev) if "mask" in c.epi else None,
                     act="relu" if "relu" in c.epi else None, out_dtype=F32 if f32 else BF, splits=splits,
                     colsum=torch.empty(-(-c.M // 128), c.N, device=dev) if c.colsum else None)
    want = torch.tensor(15.0 * K64 + ("bias" in c.epi), dtype=F64).to(y.dtype)
    assert bool((y == want).all()), f"{c.name}: all-nonzero pre-launch is off"


def _gpu_case(c, poison):
    """Runs the case unsplit and at each of its split counts -> the unsplit reference."""
    c = _resolve(c)
    mem = _Mem(c, poison, _dev())
    ref = ref_gemm(mem)
    assert ref.peak < EXACT
    f32 = c.epi == "f32"
    want = _as_out(ref.out, f32)
    first = None
    for s in (1,) + tuple(c.splits):
        used = _splits_used(c.K, s)
        assert used == K._hip().gemm_train_splits(c.K, s) and (used > 1) == (s > 1)
        ring = c.ring if s == 1 else (c.split_ring or c.ring)
        assert _ring(c.M, c.N, used) == ring, f"{c.name}: meant for the {ring}-stage ring"
        print(f"launched {c.name}: layout {_lay(c.x_t, c.w_t)} {c.M}x{c.N}x{c.K} ring {ring} requested splits {s} "
              f"used {used} tiles {-(-c.M // 128)}x{-(-c.N // 128)} nk {-(-c.K // 64)} poison {poison}")
        if c.K % 64:
            _prelaunch(c, s)
        got, cs = mem.launch(s)
        _assert_equal(got, want, f"{c.name} splits {s} ({poison} poison)")
        if first is None:
            first = got
        assert torch.equal(got, first), f"{c.name}: splits {s} differs from the unsplit result"
        if c.colsum:
            _assert_equal(cs, ref.colsum.to(F32), f"{c.name} colsum ({poison} poison)")


@pytest.mark.gpu
@pytest.mark.parametrize("poison", list(POISON))
@pytest.mark.parametrize("c", CASES_LADDER, ids=_ids(CASES_LADDER))
def test_layouts_k_ladder_deep_ring_gpu(c, poison):
    _gpu_case(c, poison)


@pytest.mark.gpu
@pytest.mark.parametrize("poison", list(POISON))
@pytest.mark.parametrize("c", CASES_WIDE, ids=_ids(CASES_WIDE))
def test_two_stage_ring_no_split_gpu(c, poison):
    _gpu_case(c, poison)


@pytest.mark.gpu
@pytest.mark.parametrize("poison", list(POISON))
@pytest.mark.parametrize("c", CASES_EPI, ids=_ids(CASES_EPI))
def test_bf16_epilogues_and_their_splits_gpu(c, poison):
    _gpu_case(c, poison)


@pytest.mark.gpu
@pytest.mark.parametrize("poison", list(POISON))
@pytest.mark.parametrize("c", CASES_SPLIT, ids=_ids(CASES_SPLIT))
def test_split_k_slicing_gpu(c, poison):
    _gpu_case(c, poison)


@pytest.mark.gpu
@pytest.mark.parametrize("poison", list(POISON))
@pytest.mark.parametrize("c", CASES_COLSUM, ids=_ids(CASES_COLSUM))
def test_colsum_gpu(c, poison):
    _gpu_case(c, poison)


@pytest.mark.gpu
@pytest.mark.parametrize("T", CSR_T)
def test_colsum_reduce_gpu(T):
    dev = _dev()
    for N in CSR_N:
        part = _csr_part(T, N)
        want = ref_colsum_reduce(part).to(F32)
        for a, width in ((0, N), (16, N + 40)):  # contiguous, and a column slice of a wider buffer
            wide = torch.full((FRONT + T + GUARD, width), float("nan"), device=dev)
            wide[FRONT:FRONT + T, a:a + N] = part.to(F32).to(dev)
            out = torch.full((N + 2 * GUARD,), SENT, device=dev)
            K.colsum_reduce(wide[FRONT:FRONT + T, a:a + N], out[GUARD:GUARD + N])
            got = out.cpu()
            assert torch.equal(got[GUARD:GUARD + N], want), (T, N, a)
            assert bool((got[:GUARD] == SENT).all()) and bool((got[GUARD + N:] == SENT).all()), (T, N, a)


_RAW = ("x", "w", "bias", "res", "y", "M", "N", "K", "ldx", "ldw", "ldy", "ldr", "x_t", "w_t", "act", "out_f32",
        "splits", "ws", "colsum")


@pytest.mark.gpu
def test_argument_checks_gpu():
    """Every rejection happens before any launch."""
    dev = _dev()
    M, N, Kd = 16, 16, 128
    x, w = torch.zeros(M, Kd, dtype=BF, device=dev), torch.zeros(N, Kd, dtype=BF, device=dev)
    y16, y32 = torch.zeros(M, N, dtype=BF, device=dev), torch.zeros(M, N, device=dev)
    res, ws, cs = torch.zeros(M, N, dtype=BF, device=dev), torch.zeros(2 * M * N, device=dev), torch.zeros(1, N, device=dev)

    def raw(**kw):
        a = dict(x=x.data_ptr(), w=w.data_ptr(), bias=0, res=0, y=y16.data_ptr(), M=M, N=N, K=Kd, ldx=Kd, ldw=Kd, ldy=N,
                 ldr=0, x_t=False, w_t=False, act=K.ACT_NONE, out_f32=False, splits=1, ws=0, colsum=0)
        a.update(kw)
        K._hip().gemm_train(*[a[k] for k in _RAW], K._stream())

    bad = {
        "K % 8": dict(K=124),
        "ldx % 8": dict(ldx=Kd + 4),
        "ldw % 8": dict(ldw=Kd + 4),
        "bf16 N % 8": dict(N=12),
        "bf16 ldy % 8": dict(ldy=N + 4),
        "fp32 N % 4": dict(N=14, out_f32=True, y=y32.data_ptr()),
        "fp32 ldy % 4": dict(ldy=N + 2, out_f32=True, y=y32.data_ptr()),
        "ldx too small": dict(ldx=Kd - 8),
        "ldw too small": dict(ldw=Kd - 8),
        "K-major ldx too small": dict(x_t=True, ldx=M - 8),
        "K-major ldw too small": dict(w_t=True, ldw=N - 8),
        "x offset by 4 elements": dict(x=x.data_ptr() + 8),
        "w offset by 4 elements": dict(w=w.data_ptr() + 8),
        "y offset by 4 elements": dict(y=y16.data_ptr() + 8),
        "fp32 with activation": dict(out_f32=True, y=y32.data_ptr(), act=K.ACT_RELU),
        "fp32 with mask": dict(out_f32=True, y=y32.data_ptr(), act=K.ACT_DRELU, res=res.data_ptr(), ldr=N),
        "drelu without mask": dict(act=K.ACT_DRELU),
        "res without drelu": dict(res=res.data_ptr(), ldr=N),
        "res with relu": dict(res=res.data_ptr(), ldr=N, act=K.ACT_RELU),
        "split-K without workspace": dict(splits=2),
        "colsum with fp32 output": dict(out_f32=True, y=y32.data_ptr(), colsum=cs.data_ptr()),
        "colsum with split-K": dict(splits=2, ws=ws.data_ptr(), colsum=cs.data_ptr()),
        "empty M": dict(M=0), "empty N": dict(N=0), "empty K": dict(K=0),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            raw(**kw)
            pytest.fail(f"accepted: {what}")
    # through the wrapper: a view's stride and offset reach the library as ld and pointer
    wide = torch.zeros(M, Kd + 4, dtype=BF, device=dev)
    flat = torch.zeros(M * Kd + 8, dtype=BF, device=dev)
    for kw in (dict(x=x[:, :12], w=w[:, :12]), dict(x=wide[:, :Kd]), dict(x=flat[4:4 + M * Kd].view(M, Kd)),
               dict(out_dtype=F32, act="relu"), dict(out_dtype=F32, mask=res), dict(act="drelu"),
               dict(mask=res, act="relu")):
        a = dict(x=x, w=w)
        a.update(kw)
        with pytest.raises(ValueError):
            K.gemm_train(a.pop("x"), a.pop("w"), **a)
    torch.cuda.synchronize()
    assert not y16.any() and not y32.any()
