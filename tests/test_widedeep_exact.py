"""The fused Wide&Deep training-step kernels of ``kernels/widedeep.hip``, each launched on its
own through the raw bindings: ``wd_keys`` / ``wd_gather`` (bitwise), ``wd_loss`` (bitwise where
it only copies or rounds, toleranced against float64 where it calls exp / rcp / log1p),
``wd_head_bwd2`` + ``colsum_reduce`` (bitwise) and ``wd_adam`` (bitwise bf16 copies,
toleranced against float64 Adam).

Every reference is written here from the formula in float64 / int64 and takes ``fault=``: a
deliberately wrong variant.  The non-GPU tests assert that every variant differs from the
truth on the committed data (by >= 100x the tolerance on >= 5 % of the elements where a
tolerance is used) and the data properties the GPU tests rely on (exact sums, both ReLU
outcomes, observable bf16 rounding with ties to even and to odd).

Every GPU launch reads its inputs from views between NaN bands (``0x7fffffff`` for int32:
the same bits) and writes into views between sentinel bands (2^100, ``-12345`` for int32);
scratch that production allocates with ``torch.empty`` is NaN-filled first.  A second launch
on the same inputs must give the same bits.

Tolerances (none is derived from what the kernels give):

``dlogit``   ``|dlogit * norm - (sigmoid(l) - y)| <= 2^-19``.  The logits of the data are exact
             in fp32 (multiples of 1/32), so the float64 reference sees the kernel's logit.
             With v_exp_f32 / v_rcp_f32 good to 1 ulp the error is below 8 * 2^-24 for
             |l| <= 8; their accuracy is assumed, not measured here, hence the x4 margin.
``loss``     ``|loss - ref| <= 2^-17 * sum|loss_b| / norm``.
``g_wbias``  ``|g - sum(dlogit as stored)| <= B * 2^-24 * max|dlogit|`` (fp32 summation order).
``adam``     m, v within 2 fp32 ulp of float64 (the data keep ``m`` and ``g`` of one sign, so
             nothing cancels); the update ``p_new - p_old`` within
             ``4 * 2^-23 * (1 + 1/(1-b1^t) + 1/(1-b2^t))`` relative plus one ulp of p:
             ``exp2(t log2 b)`` can do no better than 1 ulp of b^t, which ``1 - b^t`` amplifies
             by 1/(1-b^t) (1000x at t = 1 for b2 = 0.999); the 4 is margin for undocumented
             instruction accuracy.

Observed on an MI355X (largest over all cases; the GPU tests print them with ``-s``):
``dlogit`` 0.066 of its bound (1.3e-7 absolute), ``loss`` 0.014 of its bound, ``g_wbias`` 0.35 of its
bound; Adam ``m`` 0.97 ulp and ``v`` 1.28 ulp; the Adam update 0.49 / 0.49 / 0.50 / 0.50 of its bound at
t = 1 / 2 / 10 / 1000: that is the half ulp of rounding ``p``, which dominates the bound wherever
|p| >> |update|.  One element in eight has p = 0, where the relative part stands alone
(``rel<t>`` in the printed figures): there the update is off by 0.0040 / 0.026 / 0.033 / 0.16 of
``4 * 2^-23 * (1 + 1/(1-b1^t) + 1/(1-b2^t))`` at t = 1 / 2 / 10 / 1000, so the x4 margin holds with
room at t = 1 (b2 = 0.999 included), where 1/(1-b^t) amplifies most."""
import functools
import math

import pytest
import torch

from flink_tensorflow_amd import _ext
from flink_tensorflow_amd.ops import kernels as K

BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
EXACT = 2 ** 24
SENT = 2.0 ** 100            # output sentinel (exact in bf16 and fp32)
ISENT = -12345               # int32 output sentinel
IBAND = 0x7FFFFFFF           # int32 input band (a NaN when read as fp32)
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


def _out(shape, dtype, dev, fill=None):
    """A sentinel-filled output view between sentinel bands."""
    fill = (ISENT if dtype == I32 else SENT) if fill is None else fill
    return _banded(torch.full(shape, fill, dtype=dtype), ISENT if dtype == I32 else SENT, dev)


def _scratch(n, dev):
    """NaN-filled fp32 scratch between sentinel bands."""
    return _banded(torch.full((n,), NAN, dtype=F32), SENT, dev)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _u32(x32):
    return x32.contiguous().view(I32).to(torch.int64) & 0xFFFFFFFF


def _i16(r):
    return torch.where(r >= 32768, r - 65536, r).to(torch.int16)


def _bf16_bits(x32, trunc=False):
    """bf16 bit pattern (int16) of finite / infinite fp32 values: round to nearest, ties to even,
    done on the bit pattern (``trunc``: the high half as is)."""
    u = _u32(x32)
    r = (u >> 16) if trunc else ((u + 0x7FFF + ((u >> 16) & 1)) >> 16)
    return _i16(r & 0xFFFF).view(x32.shape)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == BF else t.contiguous().view(I32)


def _ulp32(x):
    """Spacing of fp32 at the float64 values ``x`` (normal range)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 23)


SENT_BF_BITS = int(_bits(torch.tensor([SENT], dtype=BF))[0])


# =========================================================================== 1. gather / keys
GATHER_FAULTS = ("no_field_offset", "clamp_invalid", "bad_key", "wide_no_offset", "pad_unwritten", "trunc")
# (B, F, V, D, ND, C, WV, WD, extra pad columns)
GATHER_CASES = [
    (1, 1, 11, 8, 0, 0, 5, 1, 0),
    (8, 3, 11, 16, 5, 1, 7, 4, 0),
    (37, 4, 13, 64, 13, 3, 9, 1, 16),
    (8, 3, 11, 512, 5, 3, 7, 4, 16),
    (37, 1, 11, 8, 13, 1, 5, 4, 0),
    (37, 3, 17, 16, 0, 3, 9, 1, 16),
    (1, 4, 11, 64, 5, 0, 7, 4, 16),
    (8, 4, 11, 512, 13, 1, 7, 1, 0),
]


def _gid(c):
    return "B{}F{}V{}D{}ND{}C{}WV{}WD{}+{}".format(*c)


def _xp(c):
    B, F, V, D, ND, C, WV, WD, extra = c
    return -(-(F * D + ND) // 8) * 8 + extra


@functools.lru_cache(maxsize=None)
def _gather_data(c):
    B, F, V, D, ND, C, WV, WD, _ = c
    g = torch.Generator().manual_seed(1000 + sum(c))
    FV = F * V
    cats = torch.randint(0, V, (B, F), generator=g)
    special = [-1, -(1 << 30), V, V + 3, I32MAX, I32MIN, V - 1, 0]
    flat = cats.view(-1)
    for i, s in enumerate(special):     # spread over the (b, f) slots that exist
        if B * F > 1:
            flat[(1 + i * 5) % (B * F)] = s
    if F >= 3 and B >= 8:               # out-of-field ids in a field f >= 1: they alias a neighbour's row
        cats[1, 1], cats[2, 2], cats[3, 1], cats[4, F - 1] = V, V + 3, -1, V
    cross = torch.randint(0, WV, (B, C), generator=g)
    fc = cross.view(-1)
    for i, s in enumerate([-1, WV, WV + 2, I32MAX, I32MIN, WV - 1]):
        if B * C > 1:
            fc[(1 + i * 3) % (B * C)] = s
    dense = torch.randn(B, ND, generator=g).float()
    # emb: arbitrary finite bit patterns (denormals included), an infinity, and in columns 0 / 1
    # exact halves between two bf16 values with an even / odd lower neighbour
    bits = torch.randint(-2 ** 31, 2 ** 31, (FV, D), generator=g)
    bits = torch.where(((bits >> 23) & 0xFF) == 0xFF, bits & ~(1 << 30), bits)
    hi = torch.randint(0x0080, 0x7F00, (FV, 2), generator=g)
    sign = torch.randint(0, 2, (FV, 2), generator=g) << 31
    bits[:, 0] = ((hi[:, 0] & ~1) << 16 | 0x8000 | sign[:, 0])
    bits[:, 1] = ((hi[:, 1] | 1) << 16 | 0x8000 | sign[:, 1])
    bits[0, 2] = 0x7F800000
    bits[FV - 1, 3] = 0x00000001        # the smallest denormal: rounds to +0
    bits = (bits & 0xFFFFFFFF)
    emb = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(I32).view(F32)
    wide = torch.full((WV, WD), NAN, dtype=F32)
    wide[:, 0] = torch.randint(-8, 9, (WV,), generator=g).float()
    return cats.to(I32), dense, cross.to(I32), emb, wide


def ref_gather(c, cats, dense, cross, emb, wide, fault=None):
    """-> (x bf16 bits int16 [B, XP], wsum float64 [B], keys int64 [B*F + B*C])."""
    B, F, V, D, ND, C, WV, WD, _ = c
    XP, FV = _xp(c), F * V
    BAD = FV + (0 if fault == "bad_key" else WV)
    gid = cats.long() + (0 if fault == "no_field_offset" else torch.arange(F) * V)
    ok = (gid >= 0) & (gid < FV)
    rows = emb[gid.clamp(0, FV - 1)]
    if fault != "clamp_invalid":
        rows = torch.where(ok.unsqueeze(-1), rows, torch.zeros((), dtype=F32))
    x = torch.zeros(B, XP, dtype=F32)
    x[:, :F * D] = rows.reshape(B, F * D)
    x[:, F * D:F * D + ND] = dense
    xb = _bf16_bits(x, trunc=fault == "trunc")
    if fault == "pad_unwritten":
        xb[:, F * D + ND:] = SENT_BF_BITS
    idc = cross.long()
    okc = (idc >= 0) & (idc < WV)
    kw = torch.where(okc, idc + (0 if fault == "wide_no_offset" else FV), torch.full_like(idc, BAD))
    keys = torch.cat([torch.where(ok, gid, torch.full_like(gid, BAD)).reshape(-1), kw.reshape(-1)])
    w0 = wide[:, 0].double()[idc.clamp(0, WV - 1)]
    wsum = torch.where(okc, w0, torch.zeros((), dtype=F64)).sum(1) if C else torch.zeros(B, dtype=F64)
    return xb, wsum, keys


@pytest.mark.parametrize("c", GATHER_CASES, ids=_gid)
def test_gather_data_and_rounding(c):
    cats, dense, cross, emb, wide = _gather_data(c)
    assert not torch.isnan(emb).any() and torch.isinf(emb).any()
    assert torch.isnan(wide[:, 1:]).all() and wide[:, 0].abs().max() <= 8
    # the bit-level rounding is the rounding of a plain cast
    assert torch.equal(_bf16_bits(emb), _bits(emb.to(BF)))
    assert torch.equal(_bf16_bits(dense), _bits(dense.to(BF)))
    u = _u32(emb)
    tie = (u & 0xFFFF) == 0x8000
    up = _bf16_bits(emb) != _bf16_bits(emb, trunc=True)
    assert (tie & up).any() and (tie & ~up).any()      # ties to odd+1 and ties kept at even
    assert (~tie & up).any()
    xb, wsum, keys = ref_gather(c, cats, dense, cross, emb, wide)
    assert wsum.abs().max() < EXACT


def _gather_applies(c, fault):
    B, F, V, D, ND, C, WV, WD, extra = c
    return {"no_field_offset": F > 1, "clamp_invalid": B * F > 1, "bad_key": B * F > 1,
            "wide_no_offset": B * C > 1, "pad_unwritten": _xp(c) > F * D + ND, "trunc": True}[fault]


@pytest.mark.parametrize("fault", GATHER_FAULTS)
def test_gather_faults_differ(fault):
    hit = 0
    for c in GATHER_CASES:
        if not _gather_applies(c, fault):
            continue
        hit += 1
        d = _gather_data(c)
        good, bad = ref_gather(c, *d), ref_gather(c, *d, fault=fault)
        assert any(not torch.equal(a, b) for a, b in zip(good, bad)), (fault, c)
    assert hit >= 3


def _launch_gather(c, dev):
    H = _ext.hip()
    B, F, V, D, ND, C, WV, WD, _ = c
    XP = _xp(c)
    cats, dense, cross, emb, wide = _gather_data(c)
    W = F + ND + C + 3                                  # one packed record buffer, 3 gap columns
    rec = torch.full((B, W), IBAND, dtype=I32)
    rec[:, :F] = cats
    rec[:, F:F + ND] = dense.view(I32)
    rec[:, F + ND:F + ND + C] = cross
    rv, rbuf = _banded(rec, IBAND, dev)
    cv, dv, xv = rv[:, :F], rv[:, F:F + ND].view(F32), rv[:, F + ND:F + ND + C]
    ev, _ = _banded(emb, NAN, dev)
    wv, _ = _banded(wide, NAN, dev)
    x, xbuf = _out((B, XP), BF, dev)
    ws, wbuf = _out((B,), F32, dev)
    keys, kbuf = _out((B * (F + C),), I32, dev)
    keys2, k2buf = _out((B * (F + C),), I32, dev)
    ld = rv.stride(0)
    assert ld > F and ld > ND and ld > C
    H.wd_gather(cv.data_ptr(), ld, dv.data_ptr(), ld, xv.data_ptr(), ld, ev.data_ptr(), wv.data_ptr(), x.data_ptr(),
                ws.data_ptr(), keys.data_ptr(), B, F, V, D, ND, XP, C, WV, WD, _stream())
    H.wd_keys(cv.data_ptr(), ld, xv.data_ptr(), ld, keys2.data_ptr(), B, F, V, C, WV, _stream())
    torch.cuda.synchronize()
    assert _bands_intact(xbuf, x.numel(), SENT) and _bands_intact(wbuf, B, SENT)
    assert _bands_intact(kbuf, keys.numel(), ISENT) and _bands_intact(k2buf, keys.numel(), ISENT)
    assert torch.equal(rv.cpu(), rec)                   # inputs untouched
    return _bits(x).cpu(), ws.cpu(), keys.cpu(), keys2.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("c", GATHER_CASES, ids=_gid)
def test_gather_keys_bitwise_gpu(c):
    dev = torch.device("cuda", 0)
    xb, wsum, keys = ref_gather(c, *_gather_data(c))
    got = _launch_gather(c, dev)
    assert torch.equal(got[0], xb), (got[0] != xb).nonzero()[:8]
    assert torch.equal(got[1].double(), wsum)
    assert torch.equal(got[2].long(), keys)
    assert torch.equal(got[3], got[2])                  # wd_keys: the very keys wd_gather writes
    again = _launch_gather(c, dev)
    assert all(torch.equal(_bits(a) if a.is_floating_point() else a, _bits(b) if b.is_floating_point() else b)
               for a, b in zip(got, again))


# ===================================================================================== 2. loss
LOSS_FAULTS = ("no_wbias", "no_wsum", "sign_y", "div_B", "pad_not_zeroed", "drop_last_partial", "wgrad_col1")
WBIAS = 17.0 / 32.0
TOL_DLOGIT = 2.0 ** -19
TOL_LOSS = 2.0 ** -17
# (B, nvalid, C, WD, norm): norm None = nvalid, else a larger global count
LOSS_CASES = [
    (8, 8, 0, 1, None), (8, 5, 1, 4, 64), (40, 40, 3, 6, 100), (40, 37, 1, 8, None),
    (257, 257, 1, 1, 1000), (257, 254, 3, 4, None), (520, 520, 1, 6, None), (520, 517, 3, 8, 4096),
]


def _lid(c):
    return "B{}v{}C{}WD{}n{}".format(*c)


@functools.lru_cache(maxsize=None)
def _loss_data(B):
    g = torch.Generator().manual_seed(2000 + B)
    head = torch.randint(-80, 81, (B,), generator=g).double() / 16    # exact in bf16
    wsum = torch.randint(-3, 4, (B,), generator=g).double()
    y = torch.randint(0, 2, (B,), generator=g).double()
    head[1], wsum[1] = 32.0, 8.0                                      # logit +40.53 / -39.47: saturation
    head[2], wsum[2] = -32.0, -8.0
    y[1], y[2], y[3], y[4] = 0.0, 1.0, 0.25, 0.75
    if B > 8:
        head[B - 2], wsum[B - 2], y[B - 2] = 32.0, 8.0, 1.0
        head[B - 5], wsum[B - 5], y[B - 5] = -32.0, -8.0, 0.0
        head[B - 1], wsum[B - 1], y[B - 1] = 32.0, 8.0, 0.0            # a confident miss in the last block
    return head, wsum, y


def ref_loss(c, fault=None, nvalid=None, norm=None):
    """float64 -> dict(dl [B], lb [B] per-row loss, loss, g, wgrad [B*C, WD])."""
    B, nv, C, WD, nm = c
    nv = nv if nvalid is None else nvalid
    norm = float(norm if norm is not None else (nm if nm is not None else nv))
    head, wsum, y = _loss_data(B)
    l = head + (0 if fault == "no_wsum" else wsum) + (0 if fault == "no_wbias" else WBIAS)
    lb = l.clamp_min(0) - l * y + torch.log1p(torch.exp(-l.abs()))
    s = 1.0 / (1.0 + torch.exp(-l))
    div = float(B) if fault == "div_B" else norm
    dl = ((s + y) if fault == "sign_y" else (s - y)) / div
    if fault != "pad_not_zeroed":
        valid = torch.arange(B) < nv
        dl, lb = dl * valid, lb * valid
    inc = torch.ones(B, dtype=torch.bool)
    if fault == "drop_last_partial":
        inc = torch.arange(B) < ((B + 255) // 256 - 1) * 256
    wgrad = torch.zeros(B * C, WD, dtype=F64)
    if C:
        wgrad[:, 1 if (fault == "wgrad_col1" and WD > 1) else 0] = dl.repeat_interleave(C)
    return dict(dl=dl, lb=lb, loss=(lb * inc).sum() / div, g=(dl * inc).sum(), wgrad=wgrad, norm=norm, l=l)


def test_loss_data_properties():
    for B in (8, 40, 257, 520):
        head, wsum, y = _loss_data(B)
        assert torch.equal(head.to(BF).double(), head)
        l = head + wsum + WBIAS
        assert torch.equal(l.float().double(), l) and torch.equal((head.float() + wsum.float()).double(), head + wsum)
        assert (l > 40).any() and (l < -39).any()
        assert ((y > 0) & (y < 1)).any() and (y == 0).any() and (y == 1).any()
        body = l[l.abs() <= 9]
        if B >= 257:   # dense cover of [-8, 8]: no gap above 1/2 between neighbouring logits
            sl = torch.sort(body).values
            assert sl[0] < -7 and sl[-1] > 8 and (sl[1:] - sl[:-1]).max() <= 0.5


def _loss_applies(c, fault):
    B, nv, C, WD, nm = c
    return {"no_wbias": True, "no_wsum": True, "sign_y": True, "div_B": (nm or nv) != B, "pad_not_zeroed": nv < B,
            "drop_last_partial": nv > ((B + 255) // 256 - 1) * 256,     # else the last block is all padding
            "wgrad_col1": C > 0 and WD > 1}[fault]


@pytest.mark.parametrize("fault", LOSS_FAULTS)
def test_loss_faults_differ(fault):
    hit = 0
    for c in LOSS_CASES:
        if not _loss_applies(c, fault):
            continue
        hit += 1
        B = c[0]
        r, f = ref_loss(c), ref_loss(c, fault=fault)
        norm = r["norm"]
        if fault == "wgrad_col1":
            assert not torch.equal(r["wgrad"], f["wgrad"])
            continue
        if fault == "pad_not_zeroed":       # exact-zero assertions on the padding rows
            assert (f["dl"][c[1]:] != 0).any() and (r["dl"][c[1]:] == 0).all()
            continue
        if fault == "drop_last_partial":
            tol_l = TOL_LOSS * r["lb"].abs().sum() / norm
            tol_g = B * 2.0 ** -24 * r["dl"].abs().max()
            assert (f["loss"] - r["loss"]).abs() > 100 * tol_l and (f["g"] - r["g"]).abs() > 100 * tol_g, c
            continue
        far = ((f["dl"] - r["dl"]).abs() * norm > 100 * TOL_DLOGIT).double().mean()
        assert far >= 0.05, (fault, c, far)
        if fault != "sign_y":               # the sign of y is the same in the loss here: l * y either way
            assert (f["loss"] - r["loss"]).abs() > 100 * TOL_LOSS * r["lb"].abs().sum() / norm
    assert hit >= 3


def _launch_loss(c, dev, mode, nvalid=None, norm=None, step0=None):
    """mode 'host' / 'args'.  -> dict of CPU outputs."""
    H = _ext.hip()
    B, nv, C, WD, nm = c
    nv = nv if nvalid is None else nvalid
    norm = float(norm if norm is not None else (nm if nm is not None else nv))
    head, wsum, y = _loss_data(B)
    hd = torch.full((B, 8), NAN, dtype=BF)
    hd[:, 0] = head.to(BF)
    lab = torch.full((B, 2), NAN, dtype=F32)
    lab[:, 0] = y.float()
    hv, _ = _banded(hd, NAN, dev)
    lv, _ = _banded(lab, NAN, dev)
    wsv, _ = _banded(wsum.float(), NAN, dev)
    wbv, _ = _banded(torch.tensor([WBIAS], dtype=F32), NAN, dev)
    nb = (B + 255) // 256
    dl, dlb = _out((B,), F32, dev)
    d16, d16b = _out((B,), BF, dev)
    loss, lossb = _out((1,), F32, dev)
    gw, gwb = _out((1,), F32, dev)
    gh, ghb = _out((1,), F32, dev)
    wg, wgb = _out((B * C, WD), F32, dev)
    part, partb = _scratch(2 * nb, dev)
    step, stepb = _banded(torch.tensor([step0 if step0 is not None else 0.0], dtype=F32), SENT, dev)
    args = torch.tensor([nv, 0], dtype=I32)
    args[1:] = torch.tensor([norm], dtype=F32).view(I32)
    av, _ = _banded(args, IBAND, dev)
    if mode == "args":      # the host values must be ignored: give wrong ones
        hn, hnorm, ap = B, 12345.0, av.data_ptr()
    else:
        hn, hnorm, ap = nv, norm, 0
    H.wd_loss(hv.data_ptr(), 8, wsv.data_ptr(), wbv.data_ptr(), lv.data_ptr(), 2, B, hn, hnorm, dl.data_ptr(),
              d16.data_ptr(), loss.data_ptr(), gw.data_ptr(), gh.data_ptr(), wg.data_ptr(), C, WD, part.data_ptr(),
              step.data_ptr() if step0 is not None else 0, ap, _stream())
    torch.cuda.synchronize()
    for buf, n in ((dlb, B), (d16b, B), (lossb, 1), (gwb, 1), (ghb, 1), (wgb, B * C * WD), (partb, 2 * nb),
                   (stepb, 1)):
        assert _bands_intact(buf, n, SENT)
    return dict(dl=dl.cpu(), d16=d16.cpu(), loss=loss.cpu(), gw=gw.cpu(), gh=gh.cpu(), wg=wg.cpu(), step=step.cpu(),
                part=part.cpu())


def _check_loss(c, o, nv, norm, seen):
    B, _, C, WD, _ = c
    r = ref_loss(c, nvalid=nv, norm=norm)
    dl = o["dl"]
    assert torch.equal(_bits(o["d16"]), _bf16_bits(dl))
    assert torch.equal(_bits(o["d16"]), _bits(dl.to(BF)))
    want_wg = torch.zeros(B * C, WD, dtype=F32)
    if C:
        want_wg[:, 0] = dl.repeat_interleave(C)
    assert torch.equal(_bits(o["wg"]), _bits(want_wg))
    for t in (dl[nv:], o["d16"][nv:], o["wg"][nv * C:]):
        assert torch.equal(_bits(t), torch.zeros_like(_bits(t)))      # padding rows: +0 exactly
    assert torch.equal(_bits(o["gw"]), _bits(o["gh"]))
    assert not torch.isnan(o["part"]).any()
    err = ((dl.double() * norm - r["dl"] * norm).abs().max() / TOL_DLOGIT).item() if B else 0.0
    tol_l = TOL_LOSS * r["lb"].abs().sum().item() / norm
    el = abs(o["loss"].double().item() - r["loss"].item())
    tol_g = B * 2.0 ** -24 * dl.abs().max().item()
    eg = abs(o["gw"].double().item() - dl.double().sum().item())
    seen["dlogit"] = max(seen.get("dlogit", 0.0), err)
    seen["loss"] = max(seen.get("loss", 0.0), el / tol_l if tol_l else 0.0)
    seen["g"] = max(seen.get("g", 0.0), eg / tol_g if tol_g else 0.0)
    print(f"wd_loss {_lid(c)} nv={nv} norm={norm}: dlogit err {err:.4f} of 2^-19, loss err {el:.3e} (bound {tol_l:.3e}),"
          f" g err {eg:.3e} (bound {tol_g:.3e})")
    assert err <= 1.0, err
    assert el <= tol_l, (el, tol_l)
    assert eg <= tol_g, (eg, tol_g)


@pytest.mark.gpu
@pytest.mark.parametrize("c", LOSS_CASES, ids=_lid)
def test_loss_gpu(c):
    dev = torch.device("cuda", 0)
    B, nv, C, WD, nm = c
    seen = {}
    for norm in sorted({float(nv), float(nm if nm is not None else nv), float(4 * B + 3)}):
        host = _launch_loss(c, dev, "host", norm=norm, step0=5.0)
        _check_loss(c, host, nv, norm, seen)
        assert host["step"].item() == 6.0                       # exactly one more
        nostep = _launch_loss(c, dev, "host", norm=norm)        # step = 0: no counter
        assert nostep["step"].item() == 0.0
        viaargs = _launch_loss(c, dev, "args", norm=norm, step0=1000.0)
        assert viaargs["step"].item() == 1001.0
        for k in ("dl", "d16", "loss", "gw", "gh", "wg", "part"):   # same bits on every path, run to run
            assert torch.equal(_bits(host[k]), _bits(nostep[k])), k
            assert torch.equal(_bits(host[k]), _bits(viaargs[k])), k
    print("wd_loss observed maxima (units of the bound):", seen)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [8, 257])
def test_loss_args_nvalid_zero_gpu(B):
    """A captured agreed step replayed for a rank that brings no records: everything is +0."""
    dev = torch.device("cuda", 0)
    c = (B, B, 3, 4, None)
    o = _launch_loss(c, dev, "args", nvalid=0, norm=64.0, step0=2.0)
    for k in ("dl", "d16", "loss", "gw", "gh", "wg"):
        assert torch.equal(_bits(o[k]), torch.zeros_like(_bits(o[k]))), k
    assert o["step"].item() == 3.0


# ================================================================================ 3. head bwd
HEAD_FAULTS = ("mask_ge", "db_before_round", "dw_masked", "rows_past_b1", "drop_last_group")
# (H, blocks, B)
HEAD_CASES = [(8, 1, 1), (8, 64, 8), (8, 1, 517), (8, 64, 517), (64, 1, 37), (64, 64, 37), (64, 64, 8),
              (256, 64, 8), (256, 1, 37), (256, 64, 517), (2048, 1, 8), (2048, 64, 37), (2048, 64, 517)]


def _hid(c):
    return "H{}x{}blk-B{}".format(*c)


@functools.lru_cache(maxsize=None)
def _head_data(H, B):
    g = torch.Generator().manual_seed(3000 + H + B)
    h = torch.randint(-3, 4, (B, H), generator=g).double()
    neg0 = (h == 0) & (torch.randint(0, 2, (B, H), generator=g) == 1)
    h = torch.where(neg0, torch.tensor(-0.0, dtype=F64), h)
    d = torch.randint(-15, 16, (B,), generator=g).double() * 2.0 ** -6
    d = torch.where(d == 0, torch.tensor(2.0 ** -6, dtype=F64), d)
    w = torch.randint(-31, 32, (H,), generator=g).double() * 2.0 ** -3
    w = torch.where(w == 0, torch.tensor(2.0 ** -3, dtype=F64), w)
    return h, d, w


def ref_head(c, fault=None):
    """-> (dh bf16 bits int16 [B, H], db float64 [H], dw float64 [H])."""
    H, blocks, B = c
    h, d, w = _head_data(H, B)
    rows = -(-B // blocks)
    RL = 256 // (H // 8)
    b = torch.arange(B)
    mask = (h >= 0) if fault == "mask_ge" else (h > 0)
    prod = d[:, None] * w[None, :]                      # one exact fp32 product
    raw = torch.where(mask, prod, torch.zeros((), dtype=F64))
    dhb = _bf16_bits(raw.float())
    dh = torch.tensor(dhb.numpy().astype("int32") << 16).view(F32).double() if B * H else raw
    wt = torch.ones(B, dtype=F64)                       # how often a row enters the column sums
    if fault == "rows_past_b1":                         # every block runs on to row B
        wt = torch.clamp(b // rows + 1, max=blocks).double()
    if fault == "drop_last_group":                      # the partial last row group of every block
        inblk = b - (b // rows) * rows
        nrow = torch.clamp(B - (b // rows) * rows, max=rows)
        done = inblk < (nrow // RL) * RL
        wt = done.double()
        dhb = torch.where(done[:, None], dhb, torch.tensor(SENT_BF_BITS, dtype=torch.int16))
    db = ((raw if fault == "db_before_round" else dh) * wt[:, None]).sum(0)
    dwm = (h > 0).double() if fault == "dw_masked" else 1.0
    dw = (d[:, None] * h * dwm * wt[:, None]).sum(0)
    return dhb, db, dw


@pytest.mark.parametrize("c", HEAD_CASES, ids=_hid)
def test_head_data_properties(c):
    H, blocks, B = c
    h, d, w = _head_data(H, B)
    assert torch.equal(h.to(BF).double(), h)
    if B * H >= 256:
        sign = torch.signbit(h)
        assert (h > 0).any() and (h < 0).any() and ((h == 0) & sign).any() and ((h == 0) & ~sign).any()
    prod = d[:, None] * w[None, :]
    assert torch.equal(prod.float().double(), prod)     # exact in fp32
    if B * H >= 256:
        assert (prod.float().to(BF).double() != prod).any()     # ... and the bf16 rounding shows
    # sums exact in any order: everything is an integer number of 2^-9 (dh, d*w) / 2^-6 (d*h) units
    assert (prod.abs() * 2 ** 9).sum(0).max() * 1.01 < EXACT and ((d[:, None] * h).abs() * 2 ** 6).sum(0).max() < EXACT
    dhb, db, dw = ref_head(c)
    assert torch.equal(db.float().double(), db) and torch.equal(dw.float().double(), dw)


def _head_applies(c, fault):
    H, blocks, B = c
    rows, RL = -(-B // blocks), 256 // (H // 8)
    return {"mask_ge": B * H >= 256, "db_before_round": B * H >= 256, "dw_masked": B * H >= 256,
            "rows_past_b1": blocks > 1 and B > rows, "drop_last_group": rows % RL != 0 or B % rows % RL != 0}[fault]


@pytest.mark.parametrize("fault", HEAD_FAULTS)
def test_head_faults_differ(fault):
    hit = 0
    for c in HEAD_CASES:
        if not _head_applies(c, fault):
            continue
        hit += 1
        good, bad = ref_head(c), ref_head(c, fault=fault)
        assert any(not torch.equal(a, b) for a, b in zip(good, bad)), (fault, c)
        if fault == "db_before_round":
            assert not torch.equal(good[1], bad[1])
        if fault == "dw_masked":
            assert not torch.equal(good[2], bad[2])
    assert hit >= 3


def _launch_head(c, dev):
    Hh = _ext.hip()
    H, blocks, B = c
    h, d, w = _head_data(H, B)
    hv, _ = _banded(h.to(BF), NAN, dev)
    dv, _ = _banded(d.float(), NAN, dev)
    wv, _ = _banded(w.float(), NAN, dev)
    dh, dhb = _out((B, H), BF, dev)
    part, pb = _banded(torch.full((blocks, 2 * H), NAN, dtype=F32), SENT, dev)   # production: torch.empty
    db, dbb = _out((H,), F32, dev)
    dw, dwb = _out((H,), F32, dev)
    Hh.wd_head_bwd2(hv.data_ptr(), dv.data_ptr(), wv.data_ptr(), dh.data_ptr(), part.data_ptr(), B, H, blocks,
                    _stream())
    K.colsum_reduce(part[:, :H], db)
    K.colsum_reduce(part[:, H:], dw)
    torch.cuda.synchronize()
    assert _bands_intact(dhb, B * H, SENT) and _bands_intact(pb, blocks * 2 * H, SENT)
    assert _bands_intact(dbb, H, SENT) and _bands_intact(dwb, H, SENT)
    return _bits(dh).cpu(), db.cpu(), dw.cpu(), part.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("c", HEAD_CASES, ids=_hid)
def test_head_bwd_bitwise_gpu(c):
    dev = torch.device("cuda", 0)
    H, blocks, B = c
    dhb, db, dw = ref_head(c)
    got = _launch_head(c, dev)
    assert torch.equal(got[0], dhb), (got[0] != dhb).nonzero()[:8]
    assert not torch.isnan(got[3]).any()                # every partial row written, the idle blocks' too
    rows = -(-B // blocks)
    idle = got[3][-(-B // rows):]
    assert torch.equal(_bits(idle), torch.zeros_like(_bits(idle)))
    assert torch.equal(got[1].double(), db), (got[1].double() - db).abs().max()
    assert torch.equal(got[2].double(), dw), (got[2].double() - dw).abs().max()
    again = _launch_head(c, dev)
    assert all(torch.equal(_bits(a) if a.dtype == F32 else a, _bits(b) if b.dtype == F32 else b)
               for a, b in zip(got, again))


# ===================================================================================== 4. adam
ADAM_FAULTS = ("no_bias_correction", "t_minus_1", "gscale_ignored", "eps_in_sqrt", "copy_short", "copy_no_offset")
ADAM_T = (1, 2, 10, 1000)
ADAM_BETAS = ((0.9, 0.999), (0.8, 0.99))
ADAM_GSCALE = (1.0, 0.5)
LR, EPS = 1e-3, 1e-8
# n -> weight segments (offset, count): 64-float alignment gaps, a bias run without a copy between
# them, the last one ending at n - 1 (the layout FusedWideDeepStep builds)
ADAM_LAYOUT = {
    1: [(0, 1)],
    255: [(0, 100), (192, 63)],
    256: [(0, 64), (64, 70), (192, 64)],
    257: [(0, 130), (192, 65)],
    3 * 256 + 64: [(0, 300), (320, 256), (640, 192)],
}


def _f32(x):
    return float(torch.tensor(x, dtype=F32))


@functools.lru_cache(maxsize=None)
def _adam_data(n):
    g = torch.Generator().manual_seed(4000 + n)
    p = torch.randn(n, generator=g).float()
    gr = torch.randn(n, generator=g).float()
    m = (torch.rand(n, generator=g) * 0.1).float() * torch.sign(gr)      # same sign as g: nothing cancels
    v = (torch.rand(n, generator=g) * 0.01 + 1e-4).float()
    idx = torch.arange(n)
    p = torch.where(idx % 8 == 1, torch.zeros(()), p)    # p = 0: the ulp of p hides nothing of the update
    tiny = idx % 8 == 3                  # tiny g, m, v: eps matters to the denominator
    gr = torch.where(tiny, gr * 1e-7, gr)
    m = torch.where(tiny, m * 1e-7, m)
    v = torch.where(tiny, v * 1e-12, v)
    zero = idx % 8 == 5                  # g = 0 (m, v decay only)
    gr = torch.where(zero, torch.zeros(()), gr)
    dead = idx % 16 == 13                # g = m = v = 0: the update is 0 / eps = 0
    m = torch.where(dead, torch.zeros(()), m)
    v = torch.where(dead, torch.zeros(()), v)
    return p, gr, m, v


def ref_adam(n, t, betas, gscale, fault=None):
    """float64 Adam on the fp32 values of lr, betas, eps -> dict(m, v, upd, p, copies [int16 bits])."""
    p, g, m, v = (x.double() for x in _adam_data(n))
    b1, b2, lr, eps = _f32(betas[0]), _f32(betas[1]), _f32(LR), _f32(EPS)
    gi = g * (1.0 if fault == "gscale_ignored" else gscale)
    mi = b1 * m + (1 - b1) * gi
    vi = b2 * v + (1 - b2) * gi * gi
    tt = t - 1 if fault == "t_minus_1" else t
    bc1, bc2 = (1.0, 1.0) if fault == "no_bias_correction" else (1 - b1 ** tt, 1 - b2 ** tt)
    if bc1 == 0 or bc2 == 0:                 # t - 1 = 0: a division by zero
        upd = torch.full_like(mi, float("inf"))
    else:
        den = torch.sqrt(vi / bc2 + eps) if fault == "eps_in_sqrt" else torch.sqrt(vi / bc2) + eps
        upd = -(lr / bc1) * mi / den
    pn = p + upd
    copies = []
    for off, cnt in ADAM_LAYOUT[n]:
        c = torch.full((cnt,), SENT_BF_BITS, dtype=torch.int16)
        src = _bf16_bits(pn[off:off + cnt].float())
        k = cnt - 1 if fault == "copy_short" else cnt
        if fault == "copy_no_offset":        # written at [i], not [i - off]; what falls outside is lost
            lo = min(off, cnt)
            c[lo:cnt] = src[:cnt - lo] if off < cnt else c[lo:cnt]
        else:
            c[:k] = src[:k]
        copies.append(c)
    return dict(m=mi, v=vi, upd=upd, p=pn, copies=copies)


def _adam_tol(t, betas):
    b1, b2 = _f32(betas[0]), _f32(betas[1])
    return 4 * 2.0 ** -23 * (1 + 1 / (1 - b1 ** t) + 1 / (1 - b2 ** t))


def test_adam_data_properties():
    for n in ADAM_LAYOUT:
        p, g, m, v = _adam_data(n)
        assert (m * g >= 0).all() and (v >= 0).all()
        segs = ADAM_LAYOUT[n]
        assert segs[-1][0] + segs[-1][1] == n                   # one segment ends at n - 1
        assert all(o % 64 == 0 for o, _ in segs)
        if n >= 255:
            assert (g == 0).any() and any(a + b < c for (a, b), (c, _) in zip(segs, segs[1:]))    # a gap / bias run
        r = ref_adam(n, 1, ADAM_BETAS[0], 1.0)
        if n >= 255:    # the bf16 rounding of the copies is observable
            assert any((_bf16_bits(r["p"][o:o + c].float()) != _bf16_bits(r["p"][o:o + c].float(), trunc=True)).any()
                       for o, c in segs)


def _bias_fault_change(fault, t, betas):
    """Relative change of the update under a bias-correction fault, from the formula (eps aside):
    the update scales with sqrt(1 - b2^t) / (1 - b1^t)."""
    b1, b2 = _f32(betas[0]), _f32(betas[1])
    scale = lambda k: math.sqrt(1 - b2 ** k) / (1 - b1 ** k)
    if fault == "no_bias_correction":
        wrong = 1.0
    else:
        wrong = float("inf") if t == 1 else scale(t - 1)
    return abs(wrong / scale(t) - 1)


@pytest.mark.parametrize("fault", ADAM_FAULTS)
def test_adam_faults_differ(fault):
    """Every variant is >= 100x the tolerance away on >= 5 % of the elements in EVERY configuration
    in which it can differ at all.  It cannot where gscale = 1 (``gscale_ignored`` is then the
    truth), and for the two bias-correction variants where b^t has decayed so far that the formula
    itself changes the update by less than 100x the bound (t = 1000 with betas (0.8, 0.99):
    0.99^1000 = 4e-5 changes it by 2e-5, the bound there is 1.4e-6): that is asserted, not assumed."""
    n = 3 * 256 + 64
    seen = cannot = 0
    for t in ADAM_T:
        for betas in ADAM_BETAS:
            for gs in ADAM_GSCALE:
                r, f = ref_adam(n, t, betas, gs), ref_adam(n, t, betas, gs, fault=fault)
                if fault in ("copy_short", "copy_no_offset"):
                    for nn in ADAM_LAYOUT:      # the bitwise comparisons: every layout shows it
                        a, b = ref_adam(nn, t, betas, gs), ref_adam(nn, t, betas, gs, fault=fault)
                        differs = any(not torch.equal(x, y) for x, y in zip(a["copies"], b["copies"]))
                        assert differs or (fault == "copy_no_offset" and nn == 1)
                    seen += 1
                    continue
                tol = _adam_tol(t, betas) * r["upd"].abs() + _ulp32(r["p"])
                diff = (f["upd"] - r["upd"]).abs()
                far = (torch.nan_to_num(diff, nan=float("inf")) > 100 * tol).double().mean()
                if fault == "gscale_ignored" and gs == 1.0:
                    assert torch.equal(f["upd"], r["upd"])
                    continue
                if fault in ("no_bias_correction", "t_minus_1") and (
                        _bias_fault_change(fault, t, betas) <= 100 * _adam_tol(t, betas)):
                    assert t == 1000 and betas == ADAM_BETAS[1]
                    cannot += 1
                    continue
                assert far >= 0.05, (fault, t, betas, gs, far)
                seen += 1
    assert seen >= 8 and cannot <= 2, (fault, seen, cannot)


def _launch_adam(n, t, betas, gscale, dev):
    H = _ext.hip()
    p, g, m, v = _adam_data(n)
    pv, pb = _banded(p, SENT, dev)
    gv, _ = _banded(g, NAN, dev)
    mv, mb = _banded(m, SENT, dev)
    vv, vb = _banded(v, SENT, dev)
    sv, sb = _banded(torch.tensor([float(t)], dtype=F32), SENT, dev)
    segs = ADAM_LAYOUT[n]
    copies = [_out((cnt,), BF, dev) for _, cnt in segs]
    seg = torch.tensor([[o for o, _ in segs], [c for _, c in segs], [cv.data_ptr() for cv, _ in copies]],
                       dtype=torch.int64)
    # poison around the table: an offset / count read from the band is -2^62 (no element lies in
    # [off, off + cnt)), a copy pointer read from it is no address at all
    segv, _ = _banded(seg, -(2 ** 62), dev)
    H.wd_adam(pv.data_ptr(), gv.data_ptr(), mv.data_ptr(), vv.data_ptr(), n, sv.data_ptr(), LR, betas[0], betas[1], EPS,
              gscale, segv.data_ptr(), len(segs), _stream())
    torch.cuda.synchronize()
    for buf in (pb, mb, vb):
        assert _bands_intact(buf, n, SENT)
    assert _bands_intact(sb, 1, SENT) and sv.item() == float(t)             # step is read only
    for (cv, cb), (_, cnt) in zip(copies, segs):
        assert _bands_intact(cb, cnt, SENT)
    return pv.cpu(), mv.cpu(), vv.cpu(), [cv.cpu() for cv, _ in copies]


@pytest.mark.gpu
@pytest.mark.parametrize("n", list(ADAM_LAYOUT), ids=lambda n: f"n{n}")
def test_adam_gpu(n):
    dev = torch.device("cuda", 0)
    p0 = _adam_data(n)[0].double()
    worst = {}
    for t in ADAM_T:
        for betas in ADAM_BETAS:
            for gs in ADAM_GSCALE:
                r = ref_adam(n, t, betas, gs)
                pn, mn, vn, copies = _launch_adam(n, t, betas, gs, dev)
                for (off, cnt), c in zip(ADAM_LAYOUT[n], copies):       # bf16(p_new) of the kernel's own fp32
                    assert torch.equal(_bits(c), _bf16_bits(pn[off:off + cnt])), (t, betas, gs, off)
                em = ((mn.double() - r["m"]).abs() / _ulp32(r["m"])).max().item()
                ev = ((vn.double() - r["v"]).abs() / _ulp32(r["v"])).max().item()
                assert em <= 2 and ev <= 2, (em, ev)
                upd = pn.double() - p0
                tol = _adam_tol(t, betas) * r["upd"].abs() + torch.maximum(_ulp32(p0), _ulp32(r["p"]))
                worst[t] = max(worst.get(t, 0.0), ((upd - r["upd"]).abs() / tol).max().item())
                z = (p0 == 0) & (r["upd"] != 0)     # where p = 0 the relative part of the bound stands alone
                if z.any():
                    rel = ((upd - r["upd"]).abs()[z] / (_adam_tol(t, betas) * r["upd"].abs()[z])).max().item()
                    worst[f"rel{t}"] = max(worst.get(f"rel{t}", 0.0), rel)
                worst["m_ulp"] = max(worst.get("m_ulp", 0.0), em)
                worst["v_ulp"] = max(worst.get("v_ulp", 0.0), ev)
                assert ((upd - r["upd"]).abs() <= tol).all(), (t, betas, gs, ((upd - r["upd"]).abs() / tol).max())
                # every flat element moved, the alignment gaps too (zero-gradient dead elements excepted)
                live = r["upd"] != 0
                assert (pn.double()[live] != p0[live]).all()
                again = _launch_adam(n, t, betas, gs, dev)
                assert torch.equal(_bits(pn), _bits(again[0])) and torch.equal(_bits(mn), _bits(again[1]))
                assert torch.equal(_bits(vn), _bits(again[2]))
    print(f"wd_adam n={n}: observed maxima (update: units of its bound, per t):", worst)
