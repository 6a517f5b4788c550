"""The row-sparse gradient kernels of ``kernels/sort_segments.hip`` and ``kernels/embedding.hip``,
each launched on its own: ``sort_segments`` / ``group_keys`` against a stable torch sort,
``segment_sum_sorted`` and ``segment_sum_rows`` bitwise on integer data, ``owner_buckets``
against the host placement of ``BucketedSparseExchange._bucket`` (restated here),
``rows_gather`` / ``rows_scatter`` / ``embedding_bag_fwd`` / ``sparse_adagrad`` bitwise.

Gradients are integers in [-8, 8] (exact in bf16) and every sum stays below 2^24, so fp32
accumulation is exact in any order and the float64 references need no tolerance.  The sliced
reference of ``segment_sum_sorted`` (``ref_sliced``) restates the two-pass algorithm (slice
partials into out / head / tail, then the fix-up) over a NaN-filled workspace and takes
``fault=``; the non-GPU tests assert that it equals the direct per-run sum, that every fault
differs on every case, and that the run layout of every case has a run inside a slice, one
starting and one ending exactly on a slice boundary, one over 2 slices, one over >= 3 slices and
one over more slices than the fix-up wave has row groups.

Every GPU launch reads its inputs from views between NaN bands (``0x7fffffff`` for int32) and
writes into views between sentinel bands (2^100, ``-12345`` for int32); scratch that production
allocates with ``torch.empty`` (the radix sort's ``work`` / ``temp``, the segment-sum ``ws``,
the owner ``counts``) is filled with NaN or garbage first.  A second launch gives the same bits."""
import functools

import pytest
import torch

from flink_tensorflow_amd import _ext
from flink_tensorflow_amd.ops import embedding as E

BF, F32, F64, I32, I64 = torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64
EXACT = 2 ** 24
SENT = 2.0 ** 100
ISENT = -12345
IBAND = 0x7FFFFFFF
NAN = float("nan")
BAND = 4096
I32MAX, I32MIN = 2 ** 31 - 1, -(2 ** 31)


# ------------------------------------------------------------------------------- helpers
def _banded(t, fill, dev, band=BAND):
    """``t`` as a view into a larger allocation filled with ``fill`` -> (view, whole buffer)."""
    n = t.numel()
    buf = torch.full((band + n + band,), fill, dtype=t.dtype, device=dev)
    v = buf[band:band + n].view(t.shape)
    v.copy_(t)
    return v, buf


def _bands_intact(buf, n, fill, band=BAND):
    h = buf.cpu()
    lo, hi = h[:band], h[band + n:]
    if fill != fill:
        return bool(torch.isnan(lo).all() and torch.isnan(hi).all())
    return bool((lo == fill).all() and (hi == fill).all())


def _in(t, dev):
    return _banded(t, NAN if t.is_floating_point() else IBAND, dev)[0]


def _out(shape, dtype, dev):
    fill = ISENT if dtype == I32 else SENT
    return _banded(torch.full(shape, fill, dtype=dtype), fill, dev)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == BF else t.contiguous().view(I32)


def _bf16_bits(x32):
    """bf16 bits (int16) of finite fp32 values, round to nearest even on the bit pattern."""
    u = x32.contiguous().view(I32).to(I64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return torch.where(r >= 32768, r - 65536, r).to(torch.int16).view(x32.shape)


def _ulp32(x):
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 23)


# ============================================================================= 5. sort_segments
SORT_PAIRS = {
    1: (1, 64, 2049),
    255: (63, 2048, 3 * 2048 + 5),
    256: (1, 65, 2047),
    65535: (64, 2049, 3 * 2048 + 5),
    65536: (63, 2047, 2048),
    2 ** 24 - 1: (65, 2048, 3 * 2048 + 5),
    2 ** 24: (1, 2047, 2049, 3 * 2048 + 5),
    2 ** 30 - 1: (64, 65, 3 * 2048 + 5),
}
SORT_PATTERNS = ("uniform", "equal", "invalid", "sorted", "reversed", "hot", "mixed")


def _sort_keys(pattern, n, num_rows):
    g = torch.Generator().manual_seed(5000 + n + num_rows % 9973 + len(pattern))
    uni = torch.randint(0, num_rows, (n,), generator=g)        # the whole range: the high digits differ
    if pattern == "uniform":
        k = uni
    elif pattern == "equal":
        k = torch.full((n,), num_rows - 1)
    elif pattern == "invalid":
        k = torch.tensor([-1, num_rows, I32MAX, I32MIN, num_rows + 7])[torch.arange(n) % 5]
    elif pattern == "sorted":
        k = torch.sort(uni).values
    elif pattern == "reversed":
        k = torch.sort(uni, descending=True).values
    elif pattern == "hot":
        k = uni.clone()
        k[::4] = num_rows // 2
    else:
        k = uni.clone()
        k[::7] = -1
        k[3::11] = num_rows
        k[5::13] = I32MAX
        k[1::17] = num_rows - 1
        k[2::19] = 0
    return k.to(I32)


def ref_group(keys, num_rows):
    """-> (perm, seg_id, seg [n + 1], uids [n], sorted clamped keys) as int64, by a stable
    comparison sort."""
    n = keys.numel()
    k = keys.long()
    kk = torch.where((k >= 0) & (k < num_rows), k, torch.full_like(k, num_rows))
    sk, sp = torch.sort(kk, stable=True)
    runs, counts = torch.unique_consecutive(sk, return_counts=True)
    nr = runs.numel()
    seg = torch.full((n + 1,), n, dtype=I64)
    seg[:nr] = torch.cat([torch.zeros(1, dtype=I64), counts.cumsum(0)])[:nr]
    uids = torch.full((n,), -1, dtype=I64)
    uids[:nr] = torch.where(runs < num_rows, runs, torch.full_like(runs, -1))
    return sp, torch.repeat_interleave(torch.arange(nr), counts), seg, uids, sk


def test_sort_reference_properties():
    k = torch.tensor([5, -1, 2, 5, 9, 2, 100, 5], dtype=I32)
    perm, seg_id, seg, uids, sk = ref_group(k, 9)
    assert perm.tolist() == [2, 5, 0, 3, 7, 1, 4, 6]            # stable; 9 and 100 are out of [0, 9)
    assert seg_id.tolist() == [0, 0, 1, 1, 1, 2, 2, 2]
    assert seg.tolist() == [0, 2, 5, 8, 8, 8, 8, 8, 8] and uids.tolist() == [2, 5, -1, -1, -1, -1, -1, -1]
    for nr, ns in SORT_PAIRS.items():                          # the patterns are what they say
        n = ns[-1]
        assert _sort_keys("uniform", n, nr).max() >= (nr - 1) * 3 // 4 or n < 8
        assert (_sort_keys("hot", n, nr) == nr // 2).sum() >= n // 4
        inv = _sort_keys("invalid", n, nr).long()
        assert ((inv < 0) | (inv >= nr)).all()
        m = _sort_keys("mixed", n, nr).long()
        assert (m == -1).any() and (m == nr).any() and (m == I32MAX).any()


def _launch_sort(keys, num_rows, dev):
    H = _ext.hip()
    n = keys.numel()
    kv = _in(keys, dev)
    outs = {nm: _out((n + 1 if nm == "seg" else n,), I32, dev) for nm in ("sorted", "perm", "seg_id", "seg", "uids")}
    work, workb = _banded(torch.full((3 * n,), 0x5A5A5A5A, dtype=I32), ISENT, dev)
    tb = H.sort_segments_temp_bytes(n, num_rows)
    temp, tempb = _banded(torch.full((tb,), 0xA5, dtype=torch.uint8), 0x3C, dev)
    H.sort_segments(kv.data_ptr(), n, num_rows, *(outs[nm][0].data_ptr() for nm in ("sorted", "perm", "seg_id", "seg",
                                                                                  "uids")),
                    work.data_ptr(), temp.data_ptr(), tb, _stream())
    torch.cuda.synchronize()
    for nm, (v, b) in outs.items():
        assert _bands_intact(b, v.numel(), ISENT), nm
    assert _bands_intact(workb, 3 * n, ISENT) and _bands_intact(tempb, tb, 0x3C)
    assert torch.equal(kv.cpu(), keys)
    return {nm: v.cpu() for nm, (v, _) in outs.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("num_rows", list(SORT_PAIRS), ids=lambda r: f"rows{r}")
def test_sort_segments_exact_gpu(num_rows):
    dev = torch.device("cuda", 0)
    for n in SORT_PAIRS[num_rows]:
        for pattern in SORT_PATTERNS:
            keys = _sort_keys(pattern, n, num_rows)
            perm, seg_id, seg, uids, sk = ref_group(keys, num_rows)
            nr = int(seg_id[-1]) + 1
            o = _launch_sort(keys, num_rows, dev)
            tag = (num_rows, n, pattern)
            assert torch.equal(o["perm"].long(), perm), tag
            assert torch.equal(o["sorted"].long(), sk), tag
            assert torch.equal(o["seg_id"].long(), seg_id), tag
            assert torch.equal(o["seg"].long(), seg) and (o["seg"][nr:] == n).all(), tag
            assert torch.equal(o["uids"].long(), uids) and (o["uids"][nr:] == -1).all(), tag
        again = _launch_sort(keys, num_rows, dev)
        assert all(torch.equal(o[k], again[k]) for k in o)
    # the wrapper: same grouping from int32 and from int64 keys (narrowed after the range check)
    keys = _sort_keys("mixed", SORT_PAIRS[num_rows][-1], num_rows)
    want = ref_group(keys, num_rows)
    for kk in (keys, keys.long()):
        got = E.group_keys(_in(kk, dev), num_rows)
        assert all(torch.equal(a.cpu().long(), b) for a, b in zip(got, want[:4]))


# ====================================================================== 6. segment sums (sorted)
SLICED_FAULTS = ("boundary_both", "head_for_tail", "drop_last_slice", "lo_not_subtracted", "empty_not_zeroed")
# (S, D, L, fp32 gradients)
SORTED_CASES = [(8, 8, 1, False), (8, 8, 2, True), (8, 32, 2, False), (8, 64, 1, True), (8, 512, 1, False),
                (16, 8, 2, False), (16, 32, 1, True), (16, 64, 1, False), (16, 512, 2, True), (64, 8, 1, True),
                (64, 32, 2, True), (64, 64, 2, False), (64, 512, 1, False)]


def _sid(c):
    return "S{}D{}L{}{}".format(c[0], c[1], c[2], "f32" if c[3] else "bf16")


def _run_plan(S, D):
    """(length, members) per run, in sorted order: A / B = rows of one table only, N = of neither
    (a zero row), M = mixed."""
    rg = 64 // (D // 8)
    return [(3, "M"),               # [0, 3): inside slice 0
            (S - 3, "A"),           # [3, S): ends exactly on a boundary
            (2, "B"),               # [S, S + 2): starts exactly on one
            (S, "M"),               # over 2 slices
            (3 * S, "M"),           # over 4 slices: two of them wholly inside the run
            (S - 2, "N"),           # ends on a boundary again; no table's rows: a zero row
            (2 * S, "A"),           # boundary to boundary: tail + head, nothing written direct
            ((rg + 2) * S + 5, "M"),    # more slices than the fix-up wave has row groups
            (1, "B"),
            (2 * S + 1, "B"),
            (5, "M")]


@functools.lru_cache(maxsize=None)
def _sorted_data(c):
    """Two tables (A: L lookups per gradient row, B: one) and some foreign positions in one key
    space -> dict(keys, perm, seg_id, seg, n, nr, gA, gB, loA, hiA, loB, hiB)."""
    S, D, L, fp32 = c
    g = torch.Generator().manual_seed(6000 + S + D + L)
    kinds = []
    plan = _run_plan(S, D)
    for r, (ln, kind) in enumerate(plan):
        for j in range(ln):
            kinds.append((r, "ABN"[int(torch.randint(0, 3, (1,), generator=g))] if kind == "M" else kind))
    last = len(plan) - 1
    while sum(k == "A" for _, k in kinds) % L:
        kinds.append((last, "A"))
    while len(kinds) % 8 == 0 or len(kinds) % S == 0:
        kinds.append((last, "N"))
    n = len(kinds)
    cnt = {t: sum(k == t for _, k in kinds) for t in "ABN"}
    base = {"A": 0, "B": cnt["A"], "N": cnt["A"] + cnt["B"]}
    order = {t: (torch.randperm(cnt[t], generator=g) + base[t]).tolist() for t in "ABN"}
    keys = torch.empty(n, dtype=I64)
    for r, t in kinds:
        keys[order[t].pop()] = 3 * r + 1
    num_rows = 3 * len(plan) + 2
    perm, seg_id, seg, uids, _ = ref_group(keys.to(I32), num_rows)
    gA = torch.randint(-8, 9, (cnt["A"] // L, D), generator=g).double()
    gB = torch.randint(-8, 9, (cnt["B"], D), generator=g).double()
    return dict(keys=keys.to(I32), num_rows=num_rows, perm=perm, seg_id=seg_id, seg=seg, n=n, nr=len(plan), gA=gA, gB=gB,
                A=(0, cnt["A"], L), B=(cnt["A"], cnt["A"] + cnt["B"], 1))


def _contrib(d, tab, fault=None):
    """float64 [n, D]: what sorted position i adds for table ``tab`` (NaN: a row outside the table)."""
    lo, hi, L = d[tab]
    grad = d["g" + tab]
    p = d["perm"]
    inr = (p >= lo) & (p < hi)
    src = (p if fault == "lo_not_subtracted" else p - lo) // L
    bad = inr & (src >= grad.shape[0])
    rows = grad[src.clamp(0, grad.shape[0] - 1)]
    rows = torch.where(bad[:, None], torch.tensor(NAN, dtype=F64), rows)
    return torch.where(inr[:, None], rows, torch.zeros((), dtype=F64))


def ref_direct(d, tab):
    """out [n, D]: the sum of every run's rows of table ``tab``; zero rows past the runs."""
    c = _contrib(d, tab)
    out = torch.zeros(d["n"], c.shape[1], dtype=F64)
    out.index_add_(0, d["seg_id"], c)
    return out


def ref_sliced(d, tab, S, fault=None):
    """The two-pass algorithm restated: slice partials -> out / head / tail (NaN where nobody
    writes), then the fix-up.  out starts as the sentinel."""
    n, seg, seg_id = d["n"], d["seg"], d["seg_id"]
    c = _contrib(d, tab, fault)
    D = c.shape[1]
    P = torch.cat([torch.zeros(1, D, dtype=F64), c.cumsum(0)])
    ns = -(-n // S)
    out = torch.full((n, D), SENT, dtype=F64)
    head = torch.full((ns, D), NAN, dtype=F64)
    tail = torch.full((ns, D), NAN, dtype=F64)
    for k in range(ns):
        i0, i1 = k * S, min(k * S + S, n)
        for r in range(int(seg_id[i0]), int(seg_id[i1 - 1]) + 1):
            rs, re = int(seg[r]), int(seg[r + 1])
            part = P[min(re, i1)] - P[max(rs, i0)]
            if rs >= i0 and re <= i1:
                out[r] = part
            elif rs < i0:
                head[k] = part
            else:
                tail[k] = part
    for u in range(n):
        rs, re = int(seg[u]), int(seg[u + 1])
        if re <= rs:
            if fault != "empty_not_zeroed":
                out[u] = 0
            continue
        k0 = rs // S
        k1 = (re // S if fault == "boundary_both" else (re - 1) // S)
        k1 = min(k1, ns - 1)
        if k0 == k1:
            continue
        first = head[k0] if fault == "head_for_tail" else tail[k0]
        ks = range(k0 + 1, k1 if fault == "drop_last_slice" else k1 + 1)
        out[u] = first + sum((head[k] for k in ks), torch.zeros(D, dtype=F64))
    return out


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-SENT), torch.nan_to_num(b, nan=-SENT))


@pytest.mark.parametrize("c", SORTED_CASES, ids=_sid)
def test_sorted_data_and_faults(c):
    S, D, L, fp32 = c
    d = _sorted_data(c)
    n, seg, nr = d["n"], d["seg"], d["nr"]
    assert n % S and n % 8 and d["A"][1] % L == 0
    rg = 64 // (D // 8)
    spans = [(int(seg[r]), int(seg[r + 1])) for r in range(nr)]
    nsl = [(re - 1) // S - rs // S + 1 for rs, re in spans]
    assert any(k == 1 and rs % S and re % S for k, (rs, re) in zip(nsl, spans))       # inside a slice
    assert any(rs % S == 0 and rs for rs, re in spans) and any(re % S == 0 for rs, re in spans)
    assert 2 in nsl and any(k >= 3 for k in nsl) and max(nsl) > rg
    if D == 8 and S == 8:
        assert max(re - rs for rs, re in spans) >= 520
    p, sid = d["perm"], d["seg_id"]
    inA, inB = (p < d["A"][1]), (p >= d["B"][0]) & (p < d["B"][1])
    kinds = set()
    for r in range(nr):
        m = sid == r
        kinds.add((bool(inA[m].any()), bool(inB[m].any())))
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    for tab in "AB":
        truth = ref_direct(d, tab)
        assert truth.abs().max() < EXACT and (d["g" + tab].abs().sum(0) < EXACT).all()   # any order is exact
        assert torch.equal(d["g" + tab].to(BF).double(), d["g" + tab])
        assert torch.equal(ref_sliced(d, tab, S), truth)
        assert (truth[nr:] == 0).all() and (truth[:nr].abs().sum(1) == 0).any()            # padding, a zero run
    for fault in SLICED_FAULTS:
        tabs = "B" if fault == "lo_not_subtracted" else "AB"       # table A's lo is 0
        for tab in tabs:
            assert not _same(ref_sliced(d, tab, S, fault), ref_direct(d, tab)), (fault, tab)


def _launch_sorted(c, tab, dev):
    H = _ext.hip()
    S, D, L, fp32 = c
    d = _sorted_data(c)
    n = d["n"]
    lo, hi, Lt = d[tab]
    grad = d["g" + tab].to(F32 if fp32 else BF)
    gv = _in(grad, dev) if fp32 else _banded(grad, NAN, dev)[0]
    pv, sv, gvseg = _in(d["perm"].to(I32), dev), _in(d["seg_id"].to(I32), dev), _in(d["seg"].to(I32), dev)
    out, outb = _out((n, D), F32, dev)
    nws = 2 * (-(-n // S)) * D
    ws, wsb = _banded(torch.full((nws,), NAN, dtype=F32), SENT, dev)
    H.segment_sum_sorted(gv.data_ptr(), pv.data_ptr(), sv.data_ptr(), gvseg.data_ptr(), out.data_ptr(), ws.data_ptr(), n,
                         n, D, Lt, S, int(fp32), lo, hi, _stream())
    torch.cuda.synchronize()
    assert _bands_intact(outb, n * D, SENT) and _bands_intact(wsb, nws, SENT)
    return out.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("c", SORTED_CASES, ids=_sid)
def test_segment_sum_sorted_bitwise_gpu(c):
    dev = torch.device("cuda", 0)
    S, D, L, fp32 = c
    d = _sorted_data(c)
    for tab in "AB":
        want = ref_direct(d, tab)
        got = _launch_sorted(c, tab, dev)
        assert torch.equal(got.double(), want), (tab, (got.double() != want).nonzero()[:8])
        assert torch.equal(_bits(got), _bits(_launch_sorted(c, tab, dev)))
    if S == 8:      # the production slice length, end to end: the radix sort's grouping + the wrapper
        keys = _in(d["keys"], dev)
        groups = E.group_keys(keys, d["num_rows"])
        for tab in "AB":
            lo, hi, Lt = d[tab]
            rows = _banded(d["g" + tab].to(F32 if fp32 else BF), NAN, dev)[0]
            got = E.segment_sum_grouped(groups, rows, Lt, lo, hi)
            assert torch.equal(got.cpu().double(), ref_direct(d, tab)), tab


# ======================================================================== 6b. segment_sum_rows
ROWS_D = (8, 16, 64, 24, 40, 72, 128, 512, 1024)
ROWS_LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 18, 70, 600)


@functools.lru_cache(maxsize=None)
def _rows_data(D, L, fp32):
    g = torch.Generator().manual_seed(6500 + D + L)
    G = D // 8
    per_block = 4 * (64 // G) if G in (1, 2, 4, 8) else 4
    U = max(2 * per_block + 3, 13)                  # not a multiple of the destinations per block
    lens = [ROWS_LENGTHS[i % len(ROWS_LENGTHS)] for i in range(U)]
    lens = [lens[i] for i in torch.randperm(U, generator=g).tolist()]   # long and short share a wave
    num_rows = 100003
    uid = torch.sort(torch.randperm(num_rows, generator=g)[:U]).values
    keys = torch.repeat_interleave(uid, torch.tensor(lens))
    inval = torch.tensor([-1, num_rows, I32MAX, -7, num_rows + 1])
    keys = torch.cat([keys, inval])
    keys = torch.cat([keys, torch.full(((-keys.numel()) % L,), -1)])
    keys = keys[torch.randperm(keys.numel(), generator=g)]
    rows = torch.randint(-8, 9, (keys.numel() // L, D), generator=g).double()
    return keys.to(I32), rows, num_rows, uid, lens


def ref_rows(keys, rows, num_rows, L):
    k = keys.long()
    ok = (k >= 0) & (k < num_rows)
    uid, inv = torch.unique(k[ok], return_inverse=True)
    out = torch.zeros(uid.numel(), rows.shape[1], dtype=F64)
    out.index_add_(0, inv, rows[torch.arange(k.numel())[ok] // L])
    return uid, out


@pytest.mark.parametrize("D", ROWS_D)
def test_rows_data_properties(D):
    for L in (1, 3):
        keys, rows, num_rows, uid, lens = _rows_data(D, L, True)
        assert set(lens) == set(ROWS_LENGTHS) and keys.numel() % L == 0
        G = D // 8
        per_block = 4 * (64 // G) if G in (1, 2, 4, 8) else 4
        assert len(lens) % per_block and len(lens) > per_block
        per_wave = per_block // 4
        if per_wave > 1:    # some wave holds a long (> 16) and a short segment
            assert any(max(lens[i:i + per_wave]) > 16 and min(lens[i:i + per_wave]) <= 16
                       for i in range(0, len(lens), per_wave))
        u, out = ref_rows(keys, rows, num_rows, L)
        assert torch.equal(u, uid) and out.abs().max() < EXACT and torch.equal(rows.to(BF).double(), rows)


@pytest.mark.gpu
@pytest.mark.parametrize("D", ROWS_D)
def test_segment_sum_rows_bitwise_gpu(D):
    dev = torch.device("cuda", 0)
    for L in (1, 3):
        for fp32 in (False, True):
            keys, rows, num_rows, uid, _ = _rows_data(D, L, True)
            want_u, want = ref_rows(keys, rows, num_rows, L)
            kd = _in(keys, dev)
            rd = _banded(rows.to(F32 if fp32 else BF), NAN, dev)[0]
            u, out = E.segment_sum(kd, rd, num_rows, L, static=False)
            assert torch.equal(u.cpu().long(), want_u), (D, L, fp32)
            assert torch.equal(out.cpu().double(), want), (D, L, fp32, (out.cpu().double() != want).nonzero()[:8])
            u2, out2 = E.segment_sum(kd, rd, num_rows, L, static=False)
            assert torch.equal(_bits(out.cpu()), _bits(out2.cpu()))
    # the raw binding between bands (the wrapper sizes ``out`` exactly: a spill would go unseen)
    H = _ext.hip()
    keys, rows, num_rows, uid, _ = _rows_data(D, 3, True)
    perm, seg_id, seg, uids, _ = ref_group(keys, num_rows)
    U = uid.numel()
    want = ref_rows(keys, rows, num_rows, 3)[1]
    out, outb = _out((U, D), F32, dev)
    # named, so that they live until the kernel has run: a temporary's block goes back to the
    # caching allocator at once and the next allocation overwrites it
    gv, pv, sv = _banded(rows.to(BF), NAN, dev)[0], _in(perm.to(I32), dev), _in(seg[:U + 1].to(I32), dev)
    H.segment_sum_rows(gv.data_ptr(), pv.data_ptr(), sv.data_ptr(), out.data_ptr(), U, D, 3, 0, _stream())
    torch.cuda.synchronize()
    assert _bands_intact(outb, U * D, SENT) and torch.equal(out.cpu().double(), want)


# ============================================================================= 7. owner_buckets
OWNER_N = (0, 1, 1023, 1024, 1025, 4096, 4097, 9000)
OWNER_V = 5000


def _owner_ids(n, off, seed=0):
    g = torch.Generator().manual_seed(7000 + n + off + seed)
    ids = torch.randperm(max(off + OWNER_V + 700, 2 * n), generator=g)[:n]  # distinct; some below off, some >= off + V
    ids[torch.arange(n) % 9 == 4] = -1
    return ids.to(I32)


def ref_buckets(ids, off, V, ws, cap, need, over):
    """The host branch of ``BucketedSparseExchange._bucket`` -> (send, src, need, over)."""
    loc = ids.long() - off
    valid = (ids >= 0) & (loc >= 0) & (loc < V)
    owner = torch.where(valid, loc.remainder(ws), torch.full_like(loc, ws))
    send = torch.full((ws * cap,), -1, dtype=I64)
    src = torch.full((ws * cap,), -1, dtype=I64)
    for o in range(ws):
        idx = torch.nonzero(owner == o).reshape(-1)
        k = min(idx.numel(), cap)
        send[o * cap:o * cap + k] = loc[idx[:k]]
        src[o * cap:o * cap + k] = idx[:k]
        need = max(need, idx.numel())
        over = max(over, idx.numel() - cap)
    return send, src, need, over


def test_owner_reference_properties():
    for n in OWNER_N:
        for off in (0, 1000):
            ids = _owner_ids(n, off).long()
            if n >= 1023:
                assert (ids == -1).any() and ((ids >= 0) & (ids < off)).any() == (off > 0) and (ids >= off + OWNER_V).any()
            v = ids[ids >= 0]
            assert v.unique().numel() == v.numel()
    send, src, need, over = ref_buckets(torch.tensor([7, -1, 3, 12, 5, 9], dtype=I32), 3, 8, 2, 2, 0, 0)
    # local ids 4, -, 0, (9: out), 2, 6 -> owner 0 gets all four, two kept; owner 1 none
    assert send.tolist() == [4, 0, -1, -1] and src.tolist() == [0, 2, -1, -1] and (need, over) == (4, 2)


def _launch_buckets(ids, off, ws, cap, need, over, dev):
    H = _ext.hip()
    n = ids.numel()
    iv = _in(ids, dev)
    send, sendb = _out((ws * cap,), I32, dev)
    src, srcb = _out((ws * cap,), I32, dev)
    nc = ws * H.owner_buckets_segments(n)
    counts, cb = _banded(torch.full((nc,), 0x5A5A5A5A, dtype=I32), ISENT, dev)
    H.owner_buckets(iv.data_ptr(), n, off, OWNER_V, ws, cap, send.data_ptr(), src.data_ptr(), need.data_ptr(),
                    over.data_ptr(), counts.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _bands_intact(sendb, ws * cap, ISENT) and _bands_intact(srcb, ws * cap, ISENT) and _bands_intact(cb, nc, ISENT)
    return send.cpu().long(), src.cpu().long()


@pytest.mark.gpu
@pytest.mark.parametrize("n", OWNER_N, ids=lambda n: f"n{n}")
def test_owner_buckets_exact_gpu(n):
    dev = torch.device("cuda", 0)
    assert _ext.hip().owner_buckets_segments(n) == max(1, -(-n // 4096))
    for ws in (1, 2, 3, 8):
        for off in (0, 1000):
            ids = _owner_ids(n, off)
            demand = ref_buckets(ids, off, OWNER_V, ws, 1, 0, 0)[2]
            for cap in sorted({n + 1, max(1, demand), max(1, demand // 2)}, reverse=True):
                nv, nb = _banded(torch.zeros(1, dtype=I32), ISENT, dev)
                ov, ob = _banded(torch.zeros(1, dtype=I32), ISENT, dev)
                rn, ro = 0, 0
                # a small call, the full one, the small one again: need / over only ever grow
                for sub in (ids[:n // 3], ids, ids[:n // 3]):
                    sub = sub.contiguous()
                    ws_, wr_, rn, ro = ref_buckets(sub, off, OWNER_V, ws, cap, rn, ro)
                    send, src = _launch_buckets(sub, off, ws, cap, nv, ov, dev)
                    tag = (n, ws, off, cap, sub.numel())
                    assert torch.equal(send, ws_) and torch.equal(src, wr_), tag
                    assert (nv.item(), ov.item()) == (rn, ro), tag
                    assert _bands_intact(nb, 1, ISENT) and _bands_intact(ob, 1, ISENT)
                if cap < demand:
                    assert ro == demand - cap > 0


# ================================================================= 7b. rows_gather / rows_scatter
MOVE_D = (4, 8, 32, 256)


def _move_data(D):
    g = torch.Generator().manual_seed(7500 + D)
    V = 400
    n = 2 * (256 // min(D // 4, 64)) + 5 if D <= 32 else 77        # not a multiple of a block's rows
    n = min(n, 301)
    ids = torch.randperm(V, generator=g)[:n]
    ids[3], ids[10], ids[n - 1], ids[n - 2] = -1, V, V + 5, I32MAX
    bits = lambda *s: torch.randint(-2 ** 31, 2 ** 31, s, generator=g).to(I32).view(F32)   # any bit pattern
    return V, n, ids.to(I32), bits(V, D), bits(n, D)


@pytest.mark.gpu
@pytest.mark.parametrize("D", MOVE_D)
def test_rows_gather_scatter_exact_gpu(D):
    dev = torch.device("cuda", 0)
    H = _ext.hip()
    V, n, ids, table, rows = _move_data(D)
    ok = (ids >= 0) & (ids < V)
    lid = ids.long().clamp(0, V - 1)
    want_g = torch.where(ok[:, None], _bits(table)[lid], torch.zeros((), dtype=I32))
    want_s = _bits(table).clone()
    want_s[lid[ok]] = _bits(rows)[ok]
    assert ok.sum() < n and (want_s != _bits(table)).any(1).sum() <= ok.sum() < V      # rows that must stay
    tv, tb = _banded(table, SENT, dev)
    iv = _in(ids, dev)
    out, outb = _out((n, D), F32, dev)
    H.rows_gather(tv.data_ptr(), iv.data_ptr(), out.data_ptr(), n, D, V, _stream())
    torch.cuda.synchronize()
    assert _bands_intact(outb, n * D, SENT) and torch.equal(_bits(out.cpu()), want_g)
    assert torch.equal(_bits(E.rows_gather(tv, iv.long()).cpu()), want_g)              # the wrapper, int64 ids
    rv = _banded(rows, NAN, dev)[0]
    H.rows_scatter(tv.data_ptr(), iv.data_ptr(), rv.data_ptr(), n, D, V, _stream())
    torch.cuda.synchronize()
    assert _bands_intact(tb, V * D, SENT) and torch.equal(_bits(tv.cpu()), want_s)
    t2, t2b = _banded(table, SENT, dev)
    E.rows_scatter(t2, iv.long(), rv)
    assert _bands_intact(t2b, V * D, SENT) and torch.equal(_bits(t2.cpu()), want_s)


# =========================================================================== 7c. embedding_bag_fwd
BAG_CASES = [(D, L) for D in (8, 32, 512) for L in (1, 3)]


def _bag_data(D, L):
    g = torch.Generator().manual_seed(7700 + D + L)
    V, R = 23, 37
    table = torch.randint(-2 ** 14, 2 ** 14 + 1, (V, D), generator=g).double() * 2.0 ** -10
    # column 0: odd 9-bit integers 2m + 1 (m in 128..255, even and odd): exact halves between two
    # bf16 values when L = 1, with an even and with an odd lower neighbour
    table[:, 0] = (2 * torch.randint(128, 256, (V,), generator=g) + 1).double() * 2.0 ** -3
    ids = torch.randint(0, V, (R, L), generator=g)
    fl = ids.view(-1)
    for i, s in enumerate([-1, V, V + 7, I32MAX, I32MIN]):
        fl[(2 + 7 * i) % fl.numel()] = s
    if L == 3:
        ids[5] = -1                                   # an empty bag: a zero row
    return V, R, ids.to(I32), table


def ref_bag(ids, table, V):
    i = ids.long()
    ok = (i >= 0) & (i < V)
    s = (table[i.clamp(0, V - 1)] * ok[..., None]).sum(1)
    assert torch.equal(s.float().double(), s)         # the L-sum is exact in fp32
    return _bf16_bits(s.float())


@pytest.mark.parametrize("c", BAG_CASES, ids=lambda c: f"D{c[0]}L{c[1]}")
def test_bag_data_properties(c):
    D, L = c
    V, R, ids, table = _bag_data(D, L)
    assert torch.equal(table.float().double(), table) and (table.abs().sum(0) * 2 ** 10 < EXACT).all()
    i = ids.long()
    s = (table[i.clamp(0, V - 1)] * ((i >= 0) & (i < V))[..., None]).sum(1)
    b = ref_bag(ids, table, V)
    assert torch.equal(b, _bits(s.float().to(BF)))
    assert (s.float().to(BF).double() != s).any()     # the rounding is observable
    if L == 1:                                        # ... column 0: exact ties, to even and to odd
        bits = s[:, 0].float().view(I32).long()
        valid = s[:, 0] != 0
        assert valid.sum() >= 8 and ((bits & 0xFFFF) == 0x8000)[valid].all()
        low = (bits >> 16) & 1
        assert (low[valid] == 0).any() and (low[valid] == 1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("c", BAG_CASES, ids=lambda c: f"D{c[0]}L{c[1]}")
def test_embedding_bag_fwd_bitwise_gpu(c):
    dev = torch.device("cuda", 0)
    D, L = c
    V, R, ids, table = _bag_data(D, L)
    want = ref_bag(ids, table, V)
    tv, iv = _in(table.float(), dev), _in(ids, dev)
    out, outb = _out((R, D), BF, dev)
    _ext.hip().embedding_bag_fwd(iv.data_ptr(), tv.data_ptr(), out.data_ptr(), R, L, D, V, _stream())
    torch.cuda.synchronize()
    assert _bands_intact(outb, R * D, SENT)
    assert torch.equal(_bits(out.cpu()), want), (_bits(out.cpu()) != want).nonzero()[:8]
    got = E.embedding_bag(iv, tv)
    assert got.dtype == BF and torch.equal(_bits(got.cpu()), want)


# ============================================================================== 7d. sparse_adagrad
ADAGRAD_D = (4, 8, 32, 256)


def _adagrad_data(D, off, dyadic):
    g = torch.Generator().manual_seed(7900 + D + off + dyadic)
    V, U = 61, 45
    uids = torch.randperm(V, generator=g)[:U] + off
    uids[2], uids[7], uids[11], uids[U - 1] = -1, off + V, off + V + 9, I32MAX
    if off:
        uids[4], uids[9] = off - 1, 0
    if dyadic:
        k = torch.randint(-3, 4, (U, D), generator=g).double()
        grads = torch.pow(torch.tensor(2.0, dtype=F64), k) * (torch.randint(0, 2, (U, D), generator=g) * 2 - 1)
        table = torch.randint(-512, 513, (V, D), generator=g).double() * 2.0 ** -8
        accum = torch.ones(V, D, dtype=F64)
        loc = (uids - off).long()
        ok = (uids >= 0) & (loc >= 0) & (loc < V)
        accum[loc[ok]] = 3 * torch.pow(torch.tensor(4.0, dtype=F64), k[ok])   # + g^2 = 4^(k+1): the root is 2^(k+1)
        lr, eps = 2.0 ** -3, 0.0
    else:
        grads = torch.randn(U, D, generator=g).float().double()
        table = ((1 + torch.rand(V, D, generator=g)) * (torch.randint(0, 2, (V, D), generator=g) * 2 - 1)).float().double()
        accum = (0.05 + torch.rand(V, D, generator=g)).float().double()
        lr, eps = 0.05, 1e-8
    return V, U, uids.to(I32), grads, table, accum, lr, eps


def ref_adagrad(uids, grads, table, accum, lr, eps, off):
    """float64, on the fp32 values of lr and eps -> (table, accum, touched rows)."""
    V = table.shape[0]
    lr, eps = float(torch.tensor(lr, dtype=F32)), float(torch.tensor(eps, dtype=F32))
    loc = uids.long() - off
    ok = (uids >= 0) & (loc >= 0) & (loc < V)
    t, a = table.clone(), accum.clone()
    a[loc[ok]] = accum[loc[ok]] + grads[ok] ** 2
    t[loc[ok]] = table[loc[ok]] - lr * grads[ok] / (a[loc[ok]].sqrt() + eps)
    touched = torch.zeros(V, dtype=torch.bool)
    touched[loc[ok]] = True
    return t, a, touched


def _launch_adagrad(D, off, dyadic, dev, wrapper=False):
    V, U, uids, grads, table, accum, lr, eps = _adagrad_data(D, off, dyadic)
    tv, tb = _banded(table.float(), SENT, dev)
    av, ab = _banded(accum.float(), SENT, dev)
    uv, gv = _in(uids, dev), _in(grads.float(), dev)
    if wrapper:
        E.sparse_adagrad(tv, av, uv, gv, lr, eps, off)
    else:
        _ext.hip().sparse_adagrad(tv.data_ptr(), av.data_ptr(), uv.data_ptr(), gv.data_ptr(), U, D, V, lr, eps, off,
                                  _stream())
    torch.cuda.synchronize()
    assert _bands_intact(tb, V * D, SENT) and _bands_intact(ab, V * D, SENT)
    return tv.cpu(), av.cpu()


@pytest.mark.parametrize("D", ADAGRAD_D)
def test_adagrad_data_properties(D):
    for off in (0, 1000):
        V, U, uids, grads, table, accum, lr, eps = _adagrad_data(D, off, True)
        t, a, touched = ref_adagrad(uids, grads, table, accum, lr, eps, off)
        assert 0 < touched.sum() < V and touched.sum() < U          # rows that stay, slots that are skipped
        for x in (t, a, a.sqrt(), lr * grads):
            assert torch.equal(x.float().double(), x)               # every intermediate is exact in fp32
        loc = uids.long() - off
        ok = (uids >= 0) & (loc >= 0) & (loc < V)
        assert (a[loc[ok]].sqrt() == 2 * grads[ok].abs()).all()     # the root is a power of two
        assert ((t - table).abs()[touched] == 2.0 ** -4).all()      # lr / 2 whatever k


@pytest.mark.gpu
@pytest.mark.parametrize("D", ADAGRAD_D)
def test_sparse_adagrad_gpu(D):
    dev = torch.device("cuda", 0)
    for off in (0, 1000):
        V, U, uids, grads, table, accum, lr, eps = _adagrad_data(D, off, True)
        t, a, touched = ref_adagrad(uids, grads, table, accum, lr, eps, off)
        for wrapper in (False, True):
            gt, ga = _launch_adagrad(D, off, True, dev, wrapper)
            assert torch.equal(_bits(gt), _bits(t.float())) and torch.equal(_bits(ga), _bits(a.float())), (off, wrapper)
        # an ordinary case against float64: 4 ulp; the untouched rows keep their bits
        V, U, uids, grads, table, accum, lr, eps = _adagrad_data(D, off, False)
        t, a, touched = ref_adagrad(uids, grads, table, accum, lr, eps, off)
        gt, ga = _launch_adagrad(D, off, False, dev)
        assert ((gt.double() - t).abs() <= 4 * _ulp32(t)).all() and ((ga.double() - a).abs() <= 4 * _ulp32(a)).all()
        assert torch.equal(_bits(gt)[~touched], _bits(table.float())[~touched])
        assert torch.equal(_bits(ga)[~touched], _bits(accum.float())[~touched])
        assert (gt.double() != table)[touched].any()
        gt2, ga2 = _launch_adagrad(D, off, False, dev)
        assert torch.equal(_bits(gt), _bits(gt2)) and torch.equal(_bits(ga), _bits(ga2))
