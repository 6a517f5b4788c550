"""The BERT-path kernels at their edges: exact where the answer can be made exact.

``attention_fwd_kernel<64,64>`` / ``<128,128>``, ``cls_attention_kernel``, ``pack_tokens_kernel``,
``embed_ln_kernel<1|2|4>`` and ``layernorm_kernel<1|2|4>`` (``kernels/attention.hip``,
``kernels/transformer.hip``).

Attention, exact ("selection data").  Every key carries ``16 * code`` and every query
``16 * code(target)`` with codes in {+-1}^64 that differ pairwise in at least 7 places.  All
values are exact in bf16, every score is a multiple of 256 below 2^24 (exact in fp32 in any
order), and the best score beats every other by >= 3584, i.e. >= 646 after ``scale * log2e``:
``exp2`` of every other key is exactly 0 and that of the best keys exactly 1.  Groups of
m in {1, 2, 4} valid keys share a code; V is m times an integer in [-8, 8], so the output is the
group's mean of V, an integer of magnitude <= 32 — the kernel has no freedom, and the GPU tests
assert ``torch.equal``.  Every masked key is a decoy: it carries a valid key's code and that
key's ``V + 64``, so a mask that is ignored, shifted or applied to the wrong column moves the
output by tens.  In packed batches the codes depend on the position within the sequence and V
on the sequence, so a read across ``cu[b + 1]`` ties with the neighbour's key.

Attention, continuous: ``randn`` data with logits of standard deviation ~9, and the same with
logits near 110 (``exp`` without the running-max subtraction overflows), against float64
softmax attention, with a tolerance measured on a float64 emulation of the kernel's algorithm.

``pack_tokens`` against an independent numpy reference, bit for bit, including the overflow
branch; ``cls_attention`` exact on selection data; ``embed_layernorm`` / ``layernorm`` on both
sides of every ``MAXV`` dispatch boundary, on rows of mean 3, against float64 layer norm.

The non-GPU tests check references and data alone: gaps and magnitudes, agreement with the
``K.*`` host paths, and that deliberately wrong variants of each reference differ."""
import functools
import math

import numpy as np
import pytest
import torch

from flink_tensorflow_amd.ops import kernels as K

BF = torch.bfloat16
F64 = torch.float64
D = 64                       # head dim
SCALE = 0.125                # 1 / sqrt(64): a power of two, so the host path's scores are exact too
SCALE_LOG2E = SCALE * 1.4426950408889634
SENTINEL = -77.0             # exact in bf16
GUARD = 37                   # guard rows behind every output
NEG_INF = float("-inf")
ATT_FAULTS = ("mask_ignored", "mask_shift", "no_rescale", "drop_last", "swap_heads", "overread", "swap_frag")
_SWAP = torch.cat([torch.arange(16, 32), torch.arange(0, 16)])


def _kb(S):
    """Key (and query) block of the template the launcher picks for ``seq`` = S."""
    return 64 if S <= 64 else 128


def _bf(v):
    return v.to(BF).to(F64)


# ------------------------------------------------------------------------- selection data
@functools.lru_cache(maxsize=None)
def _codes(H):
    """[512, H, 64] in {+-1}: the 9 bits of j seven times plus one fixed entry, times a fixed
    sign pattern per head.  Distinct j differ in >= 7 places whatever the head."""
    j = torch.arange(512)
    bits = ((j[:, None] >> torch.arange(9)) & 1) * 2 - 1
    base = torch.cat([bits.repeat(1, 7), torch.ones(512, 1, dtype=torch.long)], 1)
    sign = torch.randint(0, 2, (H, D), generator=torch.Generator().manual_seed(77)) * 2 - 1
    return (base[:, None, :] * sign[None]).to(F64)


def _valid_mask(S, g, B=3):
    """[B, S] bool, True = real token.  Element 0: a padded tail (S // 5 keys) and ~20 % pads
    inside the valid range.  Element 1: fully padded.  Element 2: S above the key block: the
    first ``nkb // 2`` key blocks entirely masked, valid keys (and pads) only behind them;
    otherwise a leading pad, ~20 % pads and no tail."""
    KB = _kb(S)
    valid = torch.zeros(B, S, dtype=torch.bool)
    L0 = S - S // 5
    valid[0, :L0] = torch.rand(L0, generator=g) >= 0.2
    valid[0, L0 - 1] = True
    if L0 >= 3:
        valid[0, 1] = False                      # a pad in the middle of the row, always
    nkb = -(-S // KB)
    lo = (nkb // 2) * KB if S > KB else min(1, S - 1)
    valid[2, lo:] = torch.rand(S - lo, generator=g) >= 0.2
    valid[2, S - 1] = True
    return valid


def _randint(lo, hi, shape, g):
    return torch.randint(lo, hi, shape, generator=g)


@functools.lru_cache(maxsize=None)
def padded_case(S, H, m, B=3):
    """Selection data of a padded batch.  ``qkv`` [B*S, 3*H*64] and ``want`` [B*S, H*64] float64
    (exact in bf16), ``ids`` [B*S] int32, ``valid`` [B, S]."""
    g = torch.Generator().manual_seed(100000 + 1000 * S + 10 * H + m)
    codes = _codes(H)
    valid = _valid_mask(S, g, B)
    kcode = torch.zeros(B, S, dtype=torch.long)
    qcode = torch.zeros(B, S, dtype=torch.long)
    v = torch.zeros(B, S, H * D, dtype=F64)
    want = torch.zeros(B, S, H * D, dtype=F64)
    sizes = []
    for b in range(B):
        pos = valid[b].nonzero().flatten()
        pads = (~valid[b]).nonzero().flatten()
        n = pos.numel()
        if n == 0:  # fully padded: decoys with any code; every output row is zero
            kcode[b] = _randint(0, 512, (S,), g)
            qcode[b] = kcode[b][_randint(0, S, (S,), g)]
            v[b] = _randint(-8, 9, (S, H * D), g).to(F64) + 64
            continue
        pos = pos[torch.randperm(n, generator=g)]            # a group's members are spread at random
        full = n // m
        gid = torch.cat([torch.arange(full).repeat_interleave(m), full + torch.arange(n - full * m)])
        G = int(gid[-1]) + 1                                  # groups of m, then singletons
        gcode = torch.randperm(512, generator=g)[:G]
        kcode[b, pos] = gcode[gid]
        v[b, pos] = m * _randint(-8, 9, (n, H * D), g).to(F64)
        src = pos[(torch.arange(pads.numel()) * m) % n]       # each masked key copies a valid key, group after group
        kcode[b, pads] = kcode[b, src]
        v[b, pads] = v[b, src] + 64
        size = torch.bincount(gid, minlength=G).to(F64)
        mean = torch.zeros(G, H * D, dtype=F64).index_add_(0, gid, v[b, pos]) / size[:, None]
        target = _randint(0, G, (S,), g)
        qcode[b] = gcode[target]
        want[b] = mean[target]
        sizes += size.tolist()
    q = 16 * codes[qcode].reshape(B, S, H * D)
    k = 16 * codes[kcode].reshape(B, S, H * D)
    ids = torch.where(valid, _randint(1, 30000, (B, S), g), torch.zeros(B, S, dtype=torch.long))
    return dict(qkv=torch.cat([q, k, v], -1).reshape(B * S, 3 * H * D), ids=ids.reshape(-1).to(torch.int32),
                valid=valid, want=want.reshape(B * S, H * D), B=B, S=S, H=H, m=m, sizes=sizes, cu=None)


def _spread_groups(seq, m, g):
    """Position -> tie group: groups of m positions of [0, seq), members spread at random."""
    group = torch.empty(seq, dtype=torch.long)
    group[torch.randperm(seq, generator=g)] = torch.arange(seq) // m
    return group


def _cls_groups(seq=512):
    """Pairs (j, j + 64) below 256 (one lane of ``cls_attention_kernel``, two strides) and
    (j, j + 1) above (neighbouring lanes)."""
    p = torch.arange(seq)
    return torch.where(p < 256, (p // 128) * 64 + p % 64, 128 + (p - 256) // 2)


@functools.lru_cache(maxsize=None)
def packed_case(lengths, seq, H, m, cls=False):
    """Selection data of a packed batch: the code of a key depends on its position within the
    sequence (all sequences use the same map), V on the sequence.  m in {1, 2}: a sequence
    holds a prefix of the positions, so a group keeps 1 or 2 of its members and ``1 / lrow``
    stays a power of two.  Rows past ``cu[B]`` of ``qkv`` are NaN."""
    assert m in (1, 2) and max(lengths) <= seq <= 512
    g = torch.Generator().manual_seed(200000 + 1000 * seq + 10 * H + m + len(lengths))
    codes = _codes(H)
    group = _cls_groups(seq) if cls else _spread_groups(seq, m, g)
    pcode = torch.randperm(512, generator=g)[group]
    B, T = len(lengths), sum(lengths)
    cu = torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32)
    qkv = torch.full((T + GUARD, 3 * H * D), float("nan"), dtype=F64)
    want = torch.zeros(T, H * D, dtype=F64)
    sizes = []
    for b, L in enumerate(lengths):
        if L == 0:
            continue
        a = int(cu[b])
        v = m * _randint(-8, 9, (L, H * D), g).to(F64)
        same = (group[:L, None] == group[None, :L]).to(F64)
        target = _randint(0, L, (L,), g)
        qkv[a:a + L] = torch.cat([16 * codes[pcode[target]].reshape(L, H * D), 16 * codes[pcode[:L]].reshape(L, H * D), v], 1)
        want[a:a + L] = (same / same.sum(1, keepdim=True))[target] @ v
        sizes += same.sum(1).tolist()
    return dict(qkv=qkv, ids=None, valid=None, want=want, B=B, S=seq, H=H, m=m, sizes=sizes, cu=cu, lengths=lengths)


PADDED = [(1, 1, 1), (1, 3, 2), (16, 3, 1), (16, 1, 4), (17, 1, 1), (17, 3, 2), (64, 3, 1), (64, 1, 4), (65, 1, 1),
          (65, 3, 4), (128, 3, 1), (128, 1, 2), (129, 1, 1), (129, 3, 4), (200, 3, 1), (200, 1, 2), (257, 1, 1),
          (257, 3, 4), (512, 3, 1), (512, 3, 2)]                                   # (S, H, m), B = 3
PACKED = [((0, 1, 16, 17, 63, 64, 65, 127, 128, 129, 200, 0, 5), 200, 3, 1),
          ((0, 1, 16, 17, 63, 64, 65, 127, 128, 129, 200, 0, 5), 200, 3, 2),
          ((0, 1, 15, 16, 17, 33, 64), 64, 3, 1), ((0, 1, 15, 16, 17, 33, 64), 64, 3, 2)]  # (lengths, seq, H, m)
CLS_LENGTHS = (0, 1, 2, 63, 64, 65, 128, 511, 512)


def _sel_cases():
    return ([(f"padded S{S} H{H} m{m}", functools.partial(padded_case, S, H, m)) for S, H, m in PADDED]
            + [(f"packed seq{seq} m{m}", functools.partial(packed_case, L, seq, H, m)) for L, seq, H, m in PACKED]
            + [("packed cls", functools.partial(packed_case, CLS_LENGTHS, 512, 3, 2, True))])


SEL_CASES = _sel_cases()
SEL_IDS = [n for n, _ in SEL_CASES]


# ------------------------------------------------------------------- attention references
def _sequences(d):
    """(first row, length, key validity or None) of every sequence of a case."""
    if d["cu"] is not None:
        cu = d["cu"].tolist()
        return [(cu[b], cu[b + 1] - cu[b], None) for b in range(d["B"])]
    return [(b * d["S"], d["S"], d["valid"][b]) for b in range(d["B"])]


def _rows(d):
    return int(d["cu"][-1]) if d["cu"] is not None else d["B"] * d["S"]


def _split(x, n, H):
    q, k, v = x.reshape(n, 3, H, D).permute(1, 2, 0, 3)
    return q, k, v


def attention_f64(d):
    """Plain softmax attention in float64, unrounded: the reference of the continuous tests."""
    H = d["H"]
    out = torch.zeros(_rows(d), H * D, dtype=F64)
    for a, n, valid in _sequences(d):
        if n == 0:
            continue
        q, k, v = _split(d["qkv"][a:a + n], n, H)
        s = (q @ k.transpose(-1, -2)) * SCALE
        if valid is not None:
            s = s.masked_fill(~valid[None, None, :], NEG_INF)
        p = torch.softmax(s, -1).nan_to_num(0.0)
        out[a:a + n] = (p @ v).permute(1, 0, 2).reshape(n, H * D)
    return out


def emulate(d, fault=None):
    """``attention_fwd_kernel`` step by step in float64: key blocks of KB keys (rows past the
    sequence are zero K / V with a -inf mask), ``s = q.k * scale*log2e + mask``, running maximum
    with ``mref = 0`` while it is -inf, ``alpha = exp2(m_old - mref)``, ``P = exp2(s - mref)``,
    ``lrow`` from the unrounded P, ``O = O * alpha + bf16(P) . V``, output ``bf16(O / lrow)`` or a
    zero row when ``lrow == 0``.  ``fault`` selects one of the wrong variants ``ATT_FAULTS``."""
    H, KB = d["H"], _kb(d["S"])
    out = torch.zeros(_rows(d), H * D, dtype=F64)
    for a, n, valid in _sequences(d):
        if n == 0:
            continue
        nread = n + 1 if fault == "overread" else n        # keys taken for the sequence's own
        q = _split(d["qkv"][a:a + n], n, H)[0]
        _, k, v = _split(d["qkv"][a:a + nread], nread, H)
        if fault == "swap_heads":
            k, v = k.roll(1, 0), v.roll(1, 0)
        keep = torch.ones(nread, dtype=torch.bool) if valid is None or fault == "mask_ignored" else valid.clone()
        if fault == "mask_shift":
            keep = torch.cat([torch.ones(1, dtype=torch.bool), keep[:-1]])
        nkb = -(-nread // KB)
        pad = nkb * KB - nread
        k = torch.cat([k, torch.zeros(H, pad, D, dtype=F64)], 1)
        v = torch.cat([v, torch.zeros(H, pad, D, dtype=F64)], 1)
        mask = torch.cat([torch.zeros(nread, dtype=F64).masked_fill(~keep, NEG_INF), torch.full((pad,), NEG_INF, dtype=F64)])
        o = torch.zeros(H, n, D, dtype=F64)
        mrow = torch.full((H, n), NEG_INF, dtype=F64)
        lrow = torch.zeros(H, n, dtype=F64)
        for kb in range(nkb - 1 if fault == "drop_last" else nkb):
            blk = slice(kb * KB, (kb + 1) * KB)
            s = (q @ k[:, blk].transpose(-1, -2)) * SCALE_LOG2E + mask[blk]
            mnew = torch.maximum(mrow, s.max(-1).values)
            mref = torch.where(torch.isinf(mnew), torch.zeros_like(mnew), mnew)
            alpha = torch.exp2(mrow - mref)
            p = torch.exp2(s - mref[..., None])
            lrow = lrow * alpha + p.sum(-1)
            if fault != "no_rescale":
                o = o * alpha[..., None]
            pb = _bf(p)
            if fault == "swap_frag":
                pb = torch.cat([pb[..., _SWAP], pb[..., 32:]], -1)
            o = o + pb @ v[:, blk]
            mrow = mnew
        res = torch.where(lrow[..., None] > 0, o / lrow[..., None], torch.zeros_like(o))
        out[a:a + n] = _bf(res).permute(1, 0, 2).reshape(n, H * D)
    return out


def _host_attention(d):
    """``K.attention`` on the CPU (fp32), on the bf16 operands the kernel gets."""
    rows = d["qkv"].shape[0]
    out = torch.full((rows, d["H"] * D), SENTINEL, dtype=BF)
    K.attention(d["qkv"].to(BF), d["ids"], d["B"], d["S"], d["H"], out=out, cu_seqlens=d["cu"])
    return out


def _spans_blocks(d):
    """Some sequence has valid keys in more than one key block (S = 129 has not: element 0's
    padded tail covers the one-key second block, element 2's first block is masked)."""
    KB = _kb(d["S"])
    return any(n > KB if valid is None else (valid.nonzero().flatten() // KB).unique().numel() > 1
               for _, n, valid in _sequences(d))


def _fault_applies(fault, d):
    packed = d["cu"] is not None
    return {"mask_ignored": not packed, "mask_shift": not packed, "no_rescale": _spans_blocks(d),
            "drop_last": True, "swap_heads": d["H"] > 1, "overread": packed, "swap_frag": True}[fault]


# ----------------------------------------------------------- non-GPU: attention, exact data
@pytest.mark.parametrize("name,case", SEL_CASES, ids=SEL_IDS)
def test_selection_data_are_exact_and_decisive(name, case):
    """All operands are exact in bf16, every |score| is below 2^24, every key of the target
    group has the best score and every other valid key is >= 200 below it in log2 units (fp32
    ``exp2`` is 0 below -149), the expected outputs are integers of magnitude <= 32, and the
    structure the case is for is present: ties of the stated size, and for padded batches a
    pad in the middle, a fully padded element and (S above the key block) a masked first block."""
    d = case()
    real = d["qkv"][:_rows(d)]
    assert torch.equal(_bf(real), real) and torch.isnan(d["qkv"][_rows(d):]).all()
    assert torch.equal(d["want"], d["want"].round()) and d["want"].abs().max() <= 32
    gap = math.inf
    for a, n, valid in _sequences(d):
        if n == 0 or (valid is not None and not valid.any()):
            continue
        q, k, _ = _split(real[a:a + n], n, d["H"])
        s = q @ k.transpose(-1, -2)
        assert s.abs().max() < 2 ** 24 and torch.equal(s, s.round())
        s = s * SCALE_LOG2E
        if valid is not None:
            s = s.masked_fill(~valid[None, None, :], NEG_INF)
        top = s.max(-1, keepdim=True).values
        assert (top == 64 * 256 * SCALE_LOG2E).all()           # every query finds its own code
        gap = min(gap, float((top - s.masked_fill(s == top, NEG_INF)).min()))
    print(name, "gap", gap, "tie sizes", sorted(set(d["sizes"])))
    assert gap >= 200
    if max(d["sizes"], default=0) > 1 or d["m"] > 1 and _rows(d) > 3:
        assert d["m"] in d["sizes"]
    assert set(d["sizes"]) <= {1.0, 2.0, 4.0}
    if d["cu"] is None:
        v, S = d["valid"], d["S"]
        assert not v[1].any() and v[0].any() and v[2].any()
        if S >= 5:
            assert not v[0, 1] and v[0, 2:].any() and not v[0, S - S // 5:].any()
        if S > _kb(S):
            assert not v[2, :_kb(S)].any()


@pytest.mark.parametrize("name,case", SEL_CASES, ids=SEL_IDS)
def test_selection_expected_equals_host_path_and_emulation(name, case):
    """The expected tensor is what the fp32 host path ``K.attention`` computes and what the
    float64 emulation of the kernel's blockwise algorithm computes, exactly.  The host path
    leaves rows past ``cu[B]`` alone."""
    d = case()
    T = _rows(d)
    host = _host_attention(d)
    assert torch.equal(host[:T].to(F64), d["want"]) and (host[T:] == SENTINEL).all()
    assert torch.equal(emulate(d), d["want"])


@pytest.mark.parametrize("fault", ATT_FAULTS)
def test_wrong_attention_variants_differ_on_selection_data(fault):
    """Ignored mask, mask shifted by one key, O not rescaled when the maximum moves to a later
    block, last key block dropped, heads swapped, a packed sequence reading one row past
    ``cu[b + 1]``, two 16-key score fragments swapped: each differs from the expected tensor
    on every case it applies to (mask faults: padded; rescale: valid keys in two key blocks; heads:
    H > 1; overread: packed)."""
    hit = 0
    for name, case in SEL_CASES:
        d = case()
        if _fault_applies(fault, d):
            wrong = emulate(d, fault)
            assert not torch.equal(wrong, d["want"]), name
            hit += 1
    assert hit >= 4


def test_removing_the_mask_changes_most_rows():
    """Decoys make the mask matter in many rows, not in a few: without it at least 40 % of all
    rows change (every row of the fully padded element, a third of all, and each row of the
    other elements whose target group has a decoy; S = 1: the one fully padded row)."""
    for S, H, m in PADDED:
        d = padded_case(S, H, m)
        diff = (emulate(d, "mask_ignored") != d["want"]).any(-1).double().mean().item()
        print("S", S, "H", H, "m", m, "rows changed without the mask", round(diff, 3))
        assert diff >= (0.4 if S > 1 else 0.3), (S, H, m, diff)


# ------------------------------------------------------ non-GPU: attention, continuous data
CONT = [(S, mode, outlier) for S in (50, 200, 384) for mode in ("padded", "packed") for outlier in (False, True)]
# max |emulation - float64 reference| per case, as measured by the non-GPU test below (the
# emulation holds the kernel's two bf16 roundings, of P and of the output); the GPU gets twice
# this.  Values are rounded up to 3 digits; the non-GPU test keeps them honest.
CONT_MEASURED = {
    (50, "padded", False): 0.00809, (50, "padded", True): 0.00875, (50, "packed", False): 0.00786,
    (50, "packed", True): 0.00802, (200, "padded", False): 0.00807, (200, "padded", True): 0.0116,
    (200, "packed", False): 0.00787, (200, "packed", True): 0.00871, (384, "padded", False): 0.00834,
    (384, "padded", True): 0.00904, (384, "packed", False): 0.0092, (384, "packed", True): 0.0145}


@functools.lru_cache(maxsize=None)
def cont_case(S, mode, outlier):
    """``randn`` Q, K times 3 (logit standard deviation ~9), V ``randn``; ``outlier`` adds 30 to
    column 5 of every head's Q and K (logits near 110).  Padded: the masks of the exact tests.
    Packed: full, empty, one-token and partial sequences."""
    H = 3
    g = torch.Generator().manual_seed(300000 + 10 * S + (mode == "packed") + 2 * outlier)
    if mode == "padded":
        B, valid, cu, T, lengths = 3, _valid_mask(S, g), None, 3 * S, None
        ids = torch.where(valid, _randint(1, 30000, (B, S), g), torch.zeros(B, S, dtype=torch.long)).reshape(-1).to(torch.int32)
    else:
        lengths = (S, 0, 1, 2 * S // 3 + 1, 17)
        B, valid, ids, T = len(lengths), None, None, sum(lengths)
        cu = torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32)
    x = torch.randn(T, 3, H, D, generator=g, dtype=F64)
    x[:, :2] *= 3
    if outlier:
        x[:, :2, :, 5] += 30
    qkv = torch.full((T + (GUARD if cu is not None else 0), 3 * H * D), float("nan"), dtype=F64)
    qkv[:T] = _bf(x.reshape(T, 3 * H * D))
    d = dict(qkv=qkv, ids=ids, valid=valid, B=B, S=S, H=H, cu=cu, lengths=lengths)
    d["ref"] = attention_f64(d)
    d["emu_dev"] = float((emulate(d) - d["ref"]).abs().max())
    return d


def _cont_id(c):
    return f"S{c[0]}-{c[1]}-{'outlier' if c[2] else 'peaked'}"


@pytest.mark.parametrize("case", CONT, ids=_cont_id)
def test_continuous_data_and_measured_tolerance(case):
    """The logits are as peaked as stated (standard deviation >= 8; outlier variant: largest
    logit >= 100, where fp32 ``exp`` without the max subtraction is inf), the emulation stays
    finite, and its largest deviation from the float64 reference is the recorded one."""
    d = cont_case(*case)
    H = d["H"]
    logits = []
    for a, n, valid in _sequences(d):
        if n:
            q, k, _ = _split(d["qkv"][a:a + n], n, H)
            logits.append(((q @ k.transpose(-1, -2)) * SCALE).flatten())
    logits = torch.cat(logits)
    print(_cont_id(case), "logit std", float(logits.std()), "max", float(logits.max()), "emulation deviation", d["emu_dev"])
    assert logits.std() >= 8
    if case[2]:
        assert logits.max() >= 100 and torch.isinf(torch.exp(logits.max().float()))
    assert torch.isfinite(d["ref"]).all() and d["emu_dev"] > 0
    rec = CONT_MEASURED[case]
    assert d["emu_dev"] <= rec <= 1.05 * d["emu_dev"], (d["emu_dev"], rec)
    # the host path agrees with the float64 reference to fp32 + one bf16 rounding
    host = _host_attention(d)[:_rows(d)].to(F64)
    assert (host - d["ref"]).abs().max() <= rec


# ------------------------------------------------------------------- non-GPU: cls_attention
@functools.lru_cache(maxsize=None)
def cls_case():
    return packed_case(CLS_LENGTHS, 512, 3, 2, True)


def _cls_want(d):
    """Row ``cu[b]`` of the full attention's expected tensor; a zero row for an empty sequence."""
    want = torch.zeros(d["B"], d["H"] * D, dtype=F64)
    for b, (a, n, _) in enumerate(_sequences(d)):
        if n:
            want[b] = d["want"][a]
    return want


def test_cls_attention_host_path_is_exact_on_selection_data():
    """``K.cls_attention`` (host) == the expected first rows == row ``cu[b]`` of ``K.attention``;
    ties sit in one lane's two strides (j, j + 64) and in neighbouring lanes; B * H = 27."""
    d = cls_case()
    B, H = d["B"], d["H"]
    assert (B * H) % 4 and 2.0 in d["sizes"]
    group = _cls_groups()
    assert group[3] == group[67] and group[300] == group[301] and group[3] != group[4]
    want = _cls_want(d)
    got = K.cls_attention(d["qkv"].to(BF), d["cu"], B, 512, H)
    assert torch.equal(got.to(F64), want)
    full = _host_attention(d)
    for b, (a, n, _) in enumerate(_sequences(d)):
        assert torch.equal(got[b], full[a]) if n else not got[b].any()


def test_cls_attention_refuses_sequences_longer_than_its_lds_row():
    """The kernel keeps 512 scores per wave; a longer ``seq`` raises instead of truncating."""
    qkv = torch.zeros(4, 3 * D, dtype=BF)
    cu = torch.tensor([0, 4], dtype=torch.int32)
    assert K.cls_attention(qkv, cu, 1, 512, 1).shape == (1, D)
    with pytest.raises(ValueError, match="512"):
        K.cls_attention(qkv, cu, 1, 513, 1)


# --------------------------------------------------------------------- non-GPU: pack_tokens
PACK_SHAPES = [(1, 1), (5, 77), (17, 64), (33, 65), (64, 128), (300, 130), (1024, 3)]
PACK_PATTERNS = ("tail", "middle", "leading", "empty_rows", "all_empty")


@functools.lru_cache(maxsize=None)
def pack_ids(B, S, pattern):
    """ids [B, S] int32 and the pad id (3 for the 33 x 65 shape, else 0)."""
    pad_id = 3 if (B, S) == (33, 65) else 0
    rng = np.random.default_rng(B * 1000 + S + len(pattern))
    ids = rng.integers(pad_id + 1, 30000, (B, S)).astype(np.int32)
    if pattern == "all_empty":
        ids[:] = pad_id
        return ids, pad_id
    lens = rng.integers(1, S + 1, B)
    lens[0] = S                                           # one full row
    ids[np.arange(S)[None, :] >= lens[:, None]] = pad_id
    if pattern != "tail":
        ids[rng.random((B, S)) < 0.2] = pad_id
    if pattern == "leading":
        ids[:, 0] = pad_id
        ids[::2, :2] = pad_id
    if pattern == "empty_rows":
        ids[1::3] = pad_id
        ids[0] = pad_id
        ids[-1] = pad_id
    return ids, pad_id


def ref_pack(ids, pad_id, t_cap):
    """What ``pack_tokens`` leaves in (packed, pos, cu, cls): row by row in numpy.  Beyond the
    capacity the device keeps the first ``t_cap`` tokens, leaves ``cu`` unclamped and clamps
    ``cls`` to ``t_cap - 1``."""
    B, S = ids.shape
    toks, poss, cu = [], [], [0]
    for b in range(B):
        for s in range(S):
            if ids[b, s] != pad_id:
                toks.append(int(ids[b, s]))
                poss.append(s)
        cu.append(len(toks))
    packed = np.full(t_cap, pad_id, dtype=np.int32)
    pos = np.zeros(t_cap, dtype=np.int32)
    n = min(len(toks), t_cap)
    packed[:n], pos[:n] = toks[:n], poss[:n]
    cls = np.minimum(np.array(cu[:-1], dtype=np.int32), t_cap - 1)
    return packed, pos, np.array(cu, dtype=np.int32), cls


def _t_caps(t_eff):
    return [c for c in (t_eff + 7, t_eff, t_eff - 5) if c > 0]


@pytest.mark.parametrize("pattern", PACK_PATTERNS)
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_reference_equals_host_path(shape, pattern):
    """The numpy reference == ``K.pack_tokens`` (host) wherever the capacity suffices; below
    it the host path raises.  The patterns hold what their names say."""
    ids, pad_id = pack_ids(*shape, pattern)
    B, S = shape
    keep = ids != pad_id
    t_eff = int(keep.sum())
    if pattern == "all_empty":
        assert t_eff == 0
    elif S >= 64:
        assert keep[0].all() or pattern in ("leading", "empty_rows", "middle")
        if pattern in ("middle", "leading", "empty_rows"):
            inner = [(~r[:np.flatnonzero(r)[-1]]).any() for r in keep if r.any()]
            assert any(inner)                             # a pad before a row's last token
        if pattern == "leading":
            assert not keep[:, 0].any()
        if pattern == "empty_rows":
            assert not keep[0].any() and not keep[-1].any() and keep.any()
    for t_cap in _t_caps(t_eff):
        want = ref_pack(ids, pad_id, t_cap)
        outs = [torch.full((t_cap,), -7, dtype=torch.int32), torch.full((t_cap,), -7, dtype=torch.int32),
                torch.full((B + 1,), -7, dtype=torch.int32), torch.full((B,), -7, dtype=torch.int32)]
        if t_cap < t_eff:
            with pytest.raises(ValueError):
                K.pack_tokens(torch.from_numpy(ids), pad_id, t_cap, *outs)
            assert want[2][-1] == t_eff and want[3].max() <= t_cap - 1 and (want[0] != pad_id).all()
            continue
        assert K.pack_tokens(torch.from_numpy(ids), pad_id, t_cap, *outs) == t_eff
        for name, w, o in zip(("packed", "pos", "cu", "cls"), want, outs):
            assert np.array_equal(w, o.numpy()), (name, t_cap)


# ---------------------------------------------------------------- non-GPU: layer norm data
LN_DIMS = [8, 128, 512, 520, 768, 1024, 1032, 1536, 2048]
LN_EPS = 1e-12
VOCAB, TYPES, POSITIONS, EMBED_SEQ = 50, 2, 40, 7


def ln_f64(x, gamma, beta):
    """float64 layer norm: (output, x_hat)."""
    mean = x.mean(-1, keepdim=True)
    xh = (x - mean) / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + LN_EPS)
    return xh * gamma + beta, xh


def ln_tol(ref, xh, gamma, beta):
    """``2^-8 |ref|``: one bf16 rounding of the output.  ``1e-5 (|x_hat gamma| + |beta|)``: about
    ten times the fp32 error of the ~16 operations and reductions (eps = 6e-8 each) before it."""
    return 2.0 ** -8 * ref.abs() + 1e-5 * ((xh * gamma).abs() + beta.abs())


def _affine(Dm, g):
    """gamma in +-[0.5, 1], beta in +-[0.5, 1.5], fp32."""
    sg = torch.randint(0, 2, (2, Dm), generator=g) * 2.0 - 1
    gamma = (sg[0] * (0.5 + 0.5 * torch.rand(Dm, generator=g))).float()
    beta = (sg[1] * (0.5 + torch.rand(Dm, generator=g))).float()
    return gamma, beta


LN_FLAT_DIMS = [512, 1024, 2048]


@functools.lru_cache(maxsize=None)
def ln_case(Dm, rows, residual, flat=False):
    """Rows of mean 3 and standard deviation 0.5 (the sum x + r, with a residual).  ``flat``
    (D a power of two): every value is 3 or 3 + 2^-6, one bf16 step apart.  The two-pass
    algorithm's sum, mean (a division by 2^k) and differences are then exact in fp32 and
    nothing cancels, so the tolerance below holds with room; E[x^2] - mean^2 subtracts two
    rounded numbers near 9 to get 6e-5 and is off by percents."""
    g = torch.Generator().manual_seed(400000 + 10 * Dm + rows + 5 * residual + 7 * flat)
    if flat:
        step = torch.randint(0, 2, (rows, Dm), generator=g) * 2.0 ** -6
        x, r = ((2 if residual else 3) + step).to(BF), (torch.ones(rows, Dm).to(BF) if residual else None)
    elif residual:
        x = (2 + 0.4 * torch.randn(rows, Dm, generator=g)).to(BF)
        r = (1 + 0.3 * torch.randn(rows, Dm, generator=g)).to(BF)
    else:
        x, r = (3 + 0.5 * torch.randn(rows, Dm, generator=g)).to(BF), None
    gamma, beta = _affine(Dm, g)
    s = x.to(F64) + (r.to(F64) if residual else 0)
    ref, xh = ln_f64(s, gamma.to(F64), beta.to(F64))
    return dict(x=x, r=r, gamma=gamma, beta=beta, sum=s, ref=ref, tol=ln_tol(ref, xh, gamma.to(F64), beta.to(F64)))


@functools.lru_cache(maxsize=None)
def embed_case(Dm, T, with_pos):
    """Embedding tables of mean 1 each (their sum: mean 3, standard deviation ~0.5); ids with
    -3, V and V + 100 among them (clamped to [0, V - 1]); type ids in {0, 1}."""
    g = torch.Generator().manual_seed(500000 + 10 * Dm + T + 3 * with_pos)
    word = (1 + 0.3 * torch.randn(VOCAB, Dm, generator=g)).to(BF)
    pos = (1 + 0.3 * torch.randn(POSITIONS, Dm, generator=g)).to(BF)
    typ = (1 + 0.3 * torch.randn(TYPES, Dm, generator=g)).to(BF)
    gamma, beta = _affine(Dm, g)
    ids = _randint(0, VOCAB, (T,), g).to(torch.int32)
    for i, bad in enumerate((-3, VOCAB, VOCAB + 100)):
        if T > i + 1 or i == 0:
            ids[(i * 2) % T] = bad
    tt = _randint(0, TYPES, (T,), g).to(torch.int32)
    pos_ids = _randint(0, POSITIONS, (T,), g).to(torch.int32) if with_pos else None
    p = pos_ids.long() if with_pos else torch.arange(T) % EMBED_SEQ
    s = word.to(F64)[ids.long().clamp(0, VOCAB - 1)] + pos.to(F64)[p] + typ.to(F64)[tt.long()]
    ref, xh = ln_f64(s, gamma.to(F64), beta.to(F64))
    return dict(ids=ids, tt=tt, pos_ids=pos_ids, word=word, pos=pos, typ=typ, gamma=gamma, beta=beta, sum=s, ref=ref,
                tol=ln_tol(ref, xh, gamma.to(F64), beta.to(F64)))


def _assert_ln(what, got, d):
    err = (got.to(F64) - d["ref"]).abs()
    over = err - d["tol"]
    if (over > 0).any():
        i = over.argmax()
        r, c = divmod(int(i), got.shape[1])
        raise AssertionError(f"{what}: {(over > 0).sum().item()} of {got.numel()} values out of tolerance; worst row {r}"
                             f" column {c}: got {got[r, c].item()}, want {d['ref'][r, c].item()},"
                             f" tolerance {d['tol'][r, c].item():.3g}")
    return float((err / d["tol"]).max())


def _two_pass_f32(s, gamma, beta):
    """The kernels' algorithm in fp32: mean, then the mean of the squared differences."""
    s = s.float()
    mean = s.sum(-1, keepdim=True) / s.shape[-1]
    var = ((s - mean) * (s - mean)).sum(-1, keepdim=True) / s.shape[-1]
    return ((s - mean) * torch.rsqrt(var + LN_EPS) * gamma + beta).to(BF)


def _one_pass_f32(s, gamma, beta):
    """Layer norm with the variance as E[x^2] - mean^2 in fp32: the variant the data must expose."""
    s = s.float()
    mean = s.mean(-1, keepdim=True)
    var = (s * s).mean(-1, keepdim=True) - mean * mean
    return ((s - mean) * torch.rsqrt(var + LN_EPS) * gamma + beta).to(BF)


@pytest.mark.parametrize("Dm", LN_DIMS)
def test_layernorm_reference_data_and_tolerance(Dm):
    """Rows have mean ~3 and standard deviation ~0.5; the fp32 host paths of ``K.layernorm``
    and ``K.embed_layernorm`` pass the tolerance the GPU gets, and ``sum_out`` is the rounded
    sum; clamped ids are among the inputs."""
    worst = 0.0
    for rows in (1, 5, 33):
        for residual in (False, True):
            d = ln_case(Dm, rows, residual)
            if Dm >= 128:
                assert abs(d["sum"].mean() - 3) < 0.1 and abs(d["sum"].std() - 0.5) < 0.1
            so = torch.zeros(rows, Dm, dtype=BF)
            got = K.layernorm(d["x"], d["gamma"], d["beta"], residual=d["r"], eps=LN_EPS, sum_out=so)
            worst = max(worst, _assert_ln(f"layernorm host D{Dm} rows{rows}", got, d))
            assert torch.equal(so, (d["x"].float() + (d["r"].float() if residual else 0)).to(BF))
    for T in (1, 5, 130):
        for with_pos in (False, True):
            d = embed_case(Dm, T, with_pos)
            if T >= 5:
                assert {-3, VOCAB, VOCAB + 100} <= set(d["ids"].tolist())
            got = K.embed_layernorm(d["ids"], d["tt"], d["word"], d["pos"], d["typ"], d["gamma"], d["beta"], EMBED_SEQ,
                                    eps=LN_EPS, pos_ids=d["pos_ids"])
            worst = max(worst, _assert_ln(f"embed_layernorm host D{Dm} T{T}", got, d))
    print("D", Dm, "largest host error / tolerance", worst)


def test_one_pass_variance_fails_the_layernorm_tolerance():
    """E[x^2] - mean^2 in fp32.  On the rows of mean 3 and standard deviation 0.5 it loses a
    factor 9.25 / 0.25 = 37 of fp32's precision, which a carefully summed one-pass variance
    (as here: pairwise sums) still hides below the tolerance — the ratio is printed.  The
    ``flat`` rows (ratio 1.5e5) are what exposes it: there it misses the tolerance in most
    rows at every D, while the two-pass algorithm in fp32 passes.  (``K.layernorm``'s host path
    is no witness there: ``F.layer_norm`` on the CPU merges partial moments and is itself off
    by 3e-5 on these rows.)"""
    for Dm in LN_DIMS:
        d = ln_case(Dm, 33, True)
        err = (_one_pass_f32(d["sum"], d["gamma"], d["beta"]).to(F64) - d["ref"]).abs()
        print("D", Dm, "mean-3 rows: one-pass error / tolerance", float((err / d["tol"]).max()))
    for Dm in LN_FLAT_DIMS:
        for residual in (False, True):
            d = ln_case(Dm, 33, residual, True)
            bad = ((_one_pass_f32(d["sum"], d["gamma"], d["beta"]).to(F64) - d["ref"]).abs() > d["tol"]).any(-1)
            print("D", Dm, "flat rows: one-pass misses the tolerance in", int(bad.sum()), "of 33 rows")
            assert bad.double().mean() > 0.5, (Dm, residual)
            two_pass = _two_pass_f32(d["sum"], d["gamma"], d["beta"])
            print("D", Dm, "flat rows: two-pass fp32 error / tolerance", _assert_ln(f"two-pass fp32 flat D{Dm}", two_pass, d))


# ------------------------------------------------------------------------------ GPU helpers
DEV = torch.device("cuda", 0)


def _guarded(rows, width, guard=GUARD):
    return torch.full((rows + guard, width), SENTINEL, dtype=BF, device=DEV)


def _row_owner(d):
    """(sequence, query) of every output row."""
    seq, qry = [], []
    for b, (a, n, _) in enumerate(_sequences(d)):
        seq += [b] * n
        qry += list(range(n))
    return seq, qry


def _assert_attention_bits(what, buf, d):
    """Rows < T of ``buf`` equal the expected tensor exactly, the guard rows still hold the
    sentinel.  A mismatch names sequence, head, query, query block, wave and channel."""
    T = _rows(d)
    got, want = buf[:T].cpu(), d["want"].to(BF)
    if not torch.equal(got, want):
        seq, qry = _row_owner(d)
        QB = _kb(d["S"])
        bad = (got != want).nonzero()
        lines = [f"  sequence {seq[r]} head {c // D} query {qry[r]} (query block {qry[r] // QB}, wave {qry[r] % QB // 16})"
                 f" channel {c % D}: got {got[r, c].item()}, want {want[r, c].item()}" for r, c in bad[:12].tolist()]
        raise AssertionError(f"{what}: {bad.shape[0]} of {want.numel()} values differ ({(got != want).any(-1).sum().item()}"
                             f" of {T} rows); first:\n" + "\n".join(lines))
    assert (buf[T:] == SENTINEL).all(), f"{what}: {(buf[T:] != SENTINEL).sum().item()} values written past row {T}"


def _gpu_attention(d):
    """``K.attention`` on the device into a guarded buffer.  Packed: ``qkv`` and the buffer carry
    the same guard rows (NaN in ``qkv``); padded: the guard rows lie behind the B*S rows."""
    T = _rows(d)
    buf = _guarded(T, d["H"] * D)
    qkv = d["qkv"].to(DEV, BF)
    if d["cu"] is not None:
        K.attention(qkv, None, d["B"], d["S"], d["H"], out=buf, cu_seqlens=d["cu"].to(DEV))
    else:
        K.attention(qkv, d["ids"].to(DEV), d["B"], d["S"], d["H"], out=buf[:T])
    torch.cuda.synchronize()
    return buf


# -------------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("S,H,m", PADDED, ids=[f"S{S}-H{H}-m{m}" for S, H, m in PADDED])
def test_attention_padded_exact(S, H, m):
    """Padded batches, bit for bit: pads in the middle and at the tail (each a decoy), a fully
    padded element (zero rows), an element whose first key block(s) are entirely masked (the
    ``mnew == -inf`` branch, then ``alpha = 0``), ties across key blocks, 1 to 4 query blocks."""
    d = padded_case(S, H, m)
    _assert_attention_bits(f"attention padded S={S} H={H} m={m}", _gpu_attention(d), d)


@pytest.mark.gpu
@pytest.mark.parametrize("lengths,seq,H,m", PACKED, ids=[f"seq{s}-m{m}" for _, s, _, m in PACKED])
def test_attention_packed_exact(lengths, seq, H, m):
    """Packed batches, bit for bit: empty and one-token sequences, lengths around every
    fragment and block size, NaN rows behind ``cu[B]`` that must not be read, guard rows that
    must not be written; the neighbour's keys tie with the sequence's own."""
    d = packed_case(lengths, seq, H, m)
    _assert_attention_bits(f"attention packed seq={seq} m={m}", _gpu_attention(d), d)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CONT, ids=_cont_id)
def test_attention_peaked_and_outlier_logits(case):
    """Finite, and within twice the emulation's deviation of the float64 reference.

    Measured max |bf16 emulation - float64 reference| (``CONT_MEASURED``; the allowance is twice
    this), peaked / outlier logits:
      S = 50   padded 0.00809 / 0.00875   packed 0.00786 / 0.00802
      S = 200  padded 0.00807 / 0.0116    packed 0.00787 / 0.00871
      S = 384  padded 0.00834 / 0.00904   packed 0.0092  / 0.0145
    Half a bf16 step of outputs in [2, 4) is 0.0078 and of outputs in [4, 8) 0.0156: the
    deviation is the output rounding.  On an MI355X the kernel's own deviation came out equal
    to the emulation's in all twelve cases (the same element, rounded the same way)."""
    d = cont_case(*case)
    T = _rows(d)
    buf = _gpu_attention(d)
    got = buf[:T].cpu().to(F64)
    assert torch.isfinite(got).all() and (buf[T:] == SENTINEL).all()
    err = float((got - d["ref"]).abs().max())
    print(_cont_id(case), "gpu deviation", err, "emulation deviation", d["emu_dev"])
    assert err <= 2 * d["emu_dev"], (err, d["emu_dev"])


@pytest.mark.gpu
def test_cls_attention_exact():
    """Lengths 0 to 512, B * H = 27 (the last workgroup has an idle wave), ties within a lane
    and across lanes: equal to the expected first rows and to row ``cu[b]`` of the host
    ``K.attention``; a zero row for the empty sequence; guard rows untouched; ``seq`` > 512
    refused."""
    d = cls_case()
    B, H = d["B"], d["H"]
    buf = _guarded(B, H * D)
    qkv, cu = d["qkv"].to(DEV, BF), d["cu"].to(DEV)
    K.cls_attention(qkv, cu, B, 512, H, out=buf[:B])
    torch.cuda.synchronize()
    got, want = buf[:B].cpu(), _cls_want(d).to(BF)
    host = _host_attention(d)
    for b, (a, n, _) in enumerate(_sequences(d)):
        bad = (got[b] != want[b]).nonzero().flatten().tolist()
        assert not bad, f"sequence {b} (length {n}): channels {bad[:8]} got {got[b, bad[:8]].tolist()} want {want[b, bad[:8]].tolist()}"
        assert torch.equal(got[b], host[a]) if n else not got[b].any()
    assert (buf[B:] == SENTINEL).all()
    with pytest.raises(ValueError, match="512"):
        K.cls_attention(qkv, cu, B, 513, H, out=buf[:B])


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PACK_PATTERNS)
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_tokens_exact(shape, pattern):
    """Against the numpy reference, all four outputs bit for bit, at a capacity above, at and
    below the token count; nothing written past the capacity or past ``cu`` / ``cls``."""
    ids, pad_id = pack_ids(*shape, pattern)
    B = shape[0]
    dev_ids = torch.from_numpy(ids).to(DEV)
    t_eff = int((ids != pad_id).sum())
    for t_cap in _t_caps(t_eff):
        want = ref_pack(ids, pad_id, t_cap)
        bufs = [torch.full((n + 16,), -7, dtype=torch.int32, device=DEV) for n in (t_cap, t_cap, B + 1, B)]
        K.pack_tokens(dev_ids, pad_id, t_cap, bufs[0], bufs[1], bufs[2][:B + 1], bufs[3][:B])
        torch.cuda.synchronize()
        for name, w, buf in zip(("packed", "pos", "cu", "cls"), want, bufs):
            got = buf.cpu().numpy()
            bad = np.flatnonzero(got[:len(w)] != w)
            assert bad.size == 0, (f"{name} at capacity {t_cap} ({t_eff} tokens): {bad.size} differ, first at {bad[:8].tolist()}:"
                                   f" got {got[bad[:8]].tolist()} want {w[bad[:8]].tolist()}")
            assert (got[len(w):] == -7).all(), f"{name} written past {len(w)} at capacity {t_cap}"


@pytest.mark.gpu
@pytest.mark.parametrize("with_pos", [False, True], ids=["pos-modulo", "pos-ids"])
@pytest.mark.parametrize("Dm", LN_DIMS)
def test_embed_layernorm_dispatch(Dm, with_pos):
    """Every ``MAXV`` and both sides of its boundaries, T = 1, 5, 130 (partial and many
    workgroups), type ids, clamped ids, positions by modulo or by ``pos_ids``; guard rows."""
    for T in (1, 5, 130):
        d = embed_case(Dm, T, with_pos)
        buf = _guarded(T, Dm)
        g = {k: (None if d[k] is None else d[k].to(DEV)) for k in ("ids", "tt", "pos_ids", "word", "pos", "typ", "gamma", "beta")}
        K.embed_layernorm(g["ids"], g["tt"], g["word"], g["pos"], g["typ"], g["gamma"], g["beta"], EMBED_SEQ, eps=LN_EPS,
                          out=buf[:T], pos_ids=g["pos_ids"])
        torch.cuda.synchronize()
        print("D", Dm, "T", T, "error / tolerance", _assert_ln(f"embed_layernorm D{Dm} T{T}", buf[:T].cpu(), d))
        assert (buf[T:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("Dm", LN_DIMS)
def test_layernorm_dispatch(Dm, residual):
    """Every ``MAXV`` and both sides of its boundaries, 1, 5 and 33 rows, with and without a
    residual, and at D = 512, 1024, 2048 the ``flat`` rows on which a one-pass variance fails; ``sum_out`` is the bf16 rounding of the fp32 sum, bit for bit; guard rows."""
    for rows, flat in [(1, False), (5, False), (33, False)] + ([(33, True)] if Dm in LN_FLAT_DIMS else []):
        d = ln_case(Dm, rows, residual, flat)
        buf, sbuf = _guarded(rows, Dm), _guarded(rows, Dm)
        K.layernorm(d["x"].to(DEV), d["gamma"].to(DEV), d["beta"].to(DEV), residual=d["r"].to(DEV) if residual else None,
                    eps=LN_EPS, out=buf[:rows], sum_out=sbuf[:rows])
        torch.cuda.synchronize()
        print("D", Dm, "rows", rows, "error / tolerance", _assert_ln(f"layernorm D{Dm} rows{rows}", buf[:rows].cpu(), d))
        assert torch.equal(sbuf[:rows].cpu(), (d["x"].float() + (d["r"].float() if residual else 0)).to(BF))
        assert (buf[rows:] == SENTINEL).all() and (sbuf[rows:] == SENTINEL).all()
