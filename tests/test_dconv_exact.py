"""The LDS-resident direct convolution of ``kernels/dconv.hip``, bit for bit: plain, with the
fused 3x3 / stride-2 max pool, and the stem that reads the raw uint8 batch.

The rules are those of ``test_igemm_exact.py`` and ``test_fp8_exact.py``.  Operands are small
integers, every product and partial sum is exact in fp32 in any order, ``acc * scale + bias``
is exact whether or not the compiler contracts it, and the only inexact steps are the
roundings the ``.hip`` file documents:

bf16 in      x in [-8, 8], w in [-4, 4], bias = fp32 half-integers in [-600, 600] (no scale).
fp8 in       x = e4m3 integers in [0, 8] (a ReLU predecessor), w = e4m3 integers in [-4, 4],
             ``chan_scale`` = per-channel powers of two 2^-3 .. 2^-7, bias = multiples of 1/4 in
             [-8, 8]; ``out_scale`` in {1/8, 1, 64}: 1/8 saturates at 448, 64 reaches the e4m3
             subnormals.
uint8 stem   x = random bytes, mean = half-integers (60.5, 100.5, 140.5): ``v - mean`` then has
             up to 9 significant bits and the patch's ``f2bf`` rounds (always a tie, so round
             to nearest EVEN shows); std = powers of two (64, 32, 128): ``1 / std`` is exact;
             w in [-4, 4], bias = multiples of 1/4 in [-32, 32].

The float64 mirrors are written from the definition (loops over the taps on a zero-padded
image, nothing of ``ops/`` called) and round where the kernel rounds:

plain     ``v = act(acc * scale[c] + bias[c])``; bf16 out = ``bf16_rne(v)``, fp8 out =
          ``e4m3_rne(clamp(fp32(v * out_q), +-448))``, one rounding.
pooled    (ReLU only) the plain mirror, then the max over the 3x3 / stride-2 window of the
          ROUNDED values (bf16 values, or the values of the e4m3 bytes); pool padding and conv
          positions outside [0, Ho) x [0, Wo) never win.
uint8     patch = ``bf16_rne(fp32(fp32(v) - mean[c]) * fp32(1 / std[c]))`` at channel
          ``(2a + b) * 3 + c`` of block (y, x) from pixel (2y + a, 2x + b); channels 12..15 and
          pixels past an odd edge are zero; then the plain mirror with the ``s2d_stem_weights``
          weights and block pads.

Every mirror asserts its own preconditions on every case: the bound of every intermediate
(``sum |x| |w|``, then ``bound * scale + |bias|``) in units of the data's least significant bit
is below 2^24, ``acc * scale + bias`` (and ``v * out_q``) survives a float32 round trip.  The
CPU tests assert that each rounding changes at least 5 % of the outputs, that a ReLU zeroes at
least 5 % and passes at least 5 %, that saturated and subnormal bytes occur where the case is
built for them, that each mirror equals the host paths of ``ops/`` where both are defined, and
that every deliberately wrong variant (``FAULTS``) changes the output of every case it applies to.

The GPU tests keep every operand between NaN bands (uint8 images: a byte pattern) and every
output between sentinel bands inside a wider row (pitch Cout + 32, channel offset 16), launch
twice, and compare with equality only: bf16 on the bit patterns, fp8 bytes after mapping 0x80
to 0x00.  A mismatch names image, tile row / column, channel tile, wave, pixel and channel."""
import collections
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from flink_tensorflow_amd.ops import fp8 as Q
from flink_tensorflow_amd.ops import kernels as K

BF, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
E4M3 = torch.float8_e4m3fn
EXACT = 2 ** 24         # integers below this are exact in fp32
SENT16 = 2.0 ** 100     # bf16 output sentinel: exact in bf16, far above any result
SENT8 = 0x7F            # fp8 output sentinel: the e4m3 NaN byte, no launch stores it
NAN8 = 0xFF             # band byte of uint8 operands: NaN as e4m3, half of a NaN as bf16
PIX8 = 0xA5             # band byte of the raw uint8 images
BAND = 4096             # band length in elements
LDS_MAX = 160 * 1024
FAULTS = ("tap_swap", "drop_kstep", "edge_pad", "pad_swapped", "scale_shift4", "round_via_bf16",
          "pool_outside_live", "pool_shift", "s2d_phase")
CONV_FAULTS = FAULTS[:6]
FP8_OUT_SCALES = (0.125, 1.0, 64.0)     # fp8 in: saturation at 1/8, subnormals at 64
BF16_OUT_SCALES = (1.0, 16.0)           # bf16 in: |v| reaches 448 at 1, the 16..32 binade at 16
U8_OUT_SCALES = (0.25,)
U8_MEAN, U8_STD = (60.5, 100.5, 140.5), (64.0, 32.0, 128.0)


def _round_up(a, b):
    return -(-a // b) * b


# ------------------------------------------------------------------------ rounding helpers
def _f32(v):
    """float64 -> fp32 (RNE) -> float64: one fp32 rounding of an exactly known value."""
    return v.float().double()


def _e4m3(v):
    """float64 -> e4m3 bytes as ``pack4_fp8`` does: fp32, clamp to +-448, round to nearest even."""
    return v.float().clamp(-448.0, 448.0).to(E4M3).view(U8)


def _dec(b):
    return b.contiguous().view(E4M3).double()


def _bf(v):
    """bf16 RNE of values that are exact in fp32 (float64 -> fp32 then changes nothing)."""
    return v.float().to(BF).double()


def _canon(b):
    """fp8 bytes with both zero encodings mapped to 0x00."""
    return torch.where(b == 0x80, torch.zeros_like(b), b)


def _bits(t):
    """What is compared: int16 bit patterns of bf16 values, canonical bytes of e4m3."""
    if t.dtype == U8:
        return _canon(t.contiguous())
    return t.to(BF).contiguous().view(torch.int16)


class _Trace:
    """What a mirror saw: an upper bound of every intermediate magnitude (partial sums included)
    in units of the data's least significant bit, and the shares the observability tests read."""

    def __init__(self):
        self.peak, self.stats = 0.0, {}

    def see(self, bound, unit=1.0):
        self.peak = max(self.peak, float(bound.max()) / unit)

    def exact(self, v, what):
        assert torch.equal(_f32(v), v), f"{what} is not exact in fp32"
        return v

    def note(self, **kw):
        self.stats.update(kw)

    def close(self):
        assert self.peak < EXACT, f"intermediate magnitude {self.peak} is not exact in fp32"
        return self


# ------------------------------------------------------------------------------- geometry
def _out_hw(H, W, KH, KW, s, pad):
    pt, pb, pl, pr = pad
    return (H + pt + pb - KH) // s + 1, (W + pl + pr - KW) // s + 1


def _pad_is_read(H, W, KH, KW, s, pad):
    """True when some tap of some output pixel lies in the padding."""
    pt, pb, pl, pr = pad
    Ho, Wo = _out_hw(H, W, KH, KW, s, pad)
    return pt > 0 or pl > 0 or (Ho - 1) * s + KH > H + pt or (Wo - 1) * s + KW > W + pl


def _pool_hw(Ho, Wo, ppad):
    ppt, ppb, ppl, ppr = ppad
    return (Ho + ppt + ppb - 3) // 2 + 1, (Wo + ppl + ppr - 3) // 2 + 1


def _same_pool_pads(Ho, Wo):
    """TF "SAME" pads of a 3x3 / stride-2 window."""
    ph = max((-(-Ho // 2) - 1) * 2 + 3 - Ho, 0)
    pw = max((-(-Wo // 2) - 1) * 2 + 3 - Wo, 0)
    return (ph // 2, ph - ph // 2, pw // 2, pw - pw // 2)


def _lds_bytes(es, bn, KH, KW, s, Cin, pool, waves):
    """The launcher's LDS need of one tile: patch (rounded up to 1 KiB) + filter bank + slack
    for a short last DMA, or the bf16 output tile if that is larger."""
    kl = 16 if es == 2 else 32
    wp = _round_up(KH * KW * Cin * es, 4 * kl) + 16
    npx = 64 * waves
    ph = ((npx - 1) // 17 if pool else npx // 16 - 1) * s + KH
    pw = (16 if pool else 15) * s + KW
    return max(_round_up(ph * pw * Cin * es, 1024) + bn * wp + 1024, npx * (bn * 2 + 16))


def _eff_waves(es, bn, KH, KW, s, Cin, pool, waves):
    """The wave count that runs: an 8-wave request whose tile does not fit falls back to 4;
    None when not even the 4-wave tile fits (the launcher refuses)."""
    if waves == 8 and _lds_bytes(es, bn, KH, KW, s, Cin, pool, 8) > LDS_MAX:
        waves = 4
    return waves if _lds_bytes(es, bn, KH, KW, s, Cin, pool, waves) <= LDS_MAX else None


# ------------------------------------------------------------------------------ the mirrors
def _conv_acc(tr, x, w, s, pad, es, unit=1.0, fault=None):
    """The exact accumulation over the taps of a zero-padded image.  x [N, H, W, Cin],
    w [Cout, KH, KW, Cin], float64.  Faults: (dy, dx) transposed; the last K-step (4 * KL bytes
    of the padded K) treated as zero; the border replicated into the padding; top / left pads
    exchanged with bottom / right."""
    N, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    Ho, Wo = _out_hw(H, W, KH, KW, s, pad)
    pt, pb, pl, pr = (pad[1], pad[0], pad[3], pad[2]) if fault == "pad_swapped" else pad
    if fault == "drop_kstep":
        step = 4 * (16 if es == 2 else 32) // es          # K elements per MFMA K-step
        kel = KH * KW * Cin
        w = w.reshape(Cout, kel).clone()
        w[:, _round_up(kel, step) - step:] = 0
        w = w.reshape(Cout, KH, KW, Cin)
    xn = x.permute(0, 3, 1, 2)
    if fault == "edge_pad":
        for _ in range(max(pt, pb, pl, pr)):              # replicate needs pad < size: one pixel at a time
            cur = [min(1, p) for p in (pl, pr, pt, pb)]
            xn = F.pad(xn, cur, mode="replicate")
            pl, pr, pt, pb = (p - c for p, c in zip((pl, pr, pt, pb), cur))
    extra = max(KH, KW)                                   # room for the transposed taps of tap_swap
    xp = F.pad(xn, (pl, pr + extra, pt, pb + extra)).permute(0, 2, 3, 1)
    acc = torch.zeros((N, Ho, Wo, Cout), dtype=F64)
    bound = torch.zeros((N, Ho, Wo, Cout), dtype=F64)
    for kh in range(KH):
        for kw in range(KW):
            dy, dx = (kw, kh) if fault == "tap_swap" else (kh, kw)
            sl = xp[:, dy:dy + (Ho - 1) * s + 1:s, dx:dx + (Wo - 1) * s + 1:s, :]
            acc += sl @ w[:, kh, kw, :].t()
            bound += sl.abs() @ w[:, kh, kw, :].abs().t()
    tr.see(bound, unit)
    return acc, bound


def ref_plain(x, w, scale, bias, s, pad, act, out_q, es, lsb, unit=1.0, fault=None, tr=None):
    """``dconv_kernel`` without the pool.  ``out_q`` None = bf16 output.  ``unit``: the lsb of the
    products, ``lsb``: that of ``acc * scale + bias``.  Returns (bf16 values as float64, or e4m3
    bytes, [N, Ho, Wo, Cout]; trace)."""
    tr = tr or _Trace()
    acc, bound = _conv_acc(tr, x, w, s, pad, es, unit, fault)
    if fault == "scale_shift4":
        scale, bias = scale.roll(-4), bias.roll(-4)
    tr.see(bound * scale + bias.abs(), lsb)
    v = tr.exact(acc * scale + bias, "acc * scale + bias")
    if act == "relu":
        tr.note(zeroed=(v <= 0).double().mean().item(), passed=(v > 0).double().mean().item())
        v = torch.relu(v)
    if out_q is None:
        y = _bf(v)
        tr.note(changed=(y != v).double().mean().item())
        return y, tr.close()
    t = tr.exact(v * out_q, "v * out_q")
    if fault == "round_via_bf16":
        t = _bf(v) * out_q
    y = _e4m3(t)
    m = y & 0x7F
    tr.note(changed=(_dec(y) != t).double().mean().item(), saturated=(t.abs() > 448).sum().item(),
            subnormal=((m >= 1) & (m <= 7)).sum().item())
    return y, tr.close()


def _pool3x3s2(vals, ppad, Hp, Wp, fault=None):
    """Max over the 3x3 / stride-2 windows of vals [N, Ho, Wo, C]; padding is -inf.  Fault
    ``pool_shift``: on every padded axis the window origin is off by the pool pad (2 py where
    it is 2 py - 1, and the other way round)."""
    ppt, ppb, ppl, ppr = ppad
    if fault == "pool_shift":
        ppt = 1 - ppt if ppt + ppb else 0
        ppl = 1 - ppl if ppl + ppr else 0
    P = F.pad(vals.permute(0, 3, 1, 2), (ppl, 3, ppt, 3), value=float("-inf"))
    out = torch.full((vals.shape[0], vals.shape[3], Hp, Wp), float("-inf"), dtype=F64)
    for dy in range(3):
        for dx in range(3):
            out = torch.maximum(out, P[:, :, dy:dy + 2 * (Hp - 1) + 1:2, dx:dx + 2 * (Wp - 1) + 1:2])
    return out.permute(0, 2, 3, 1).contiguous()


def ref_pooled(x, w, scale, bias, s, pad, ppad, out_q, es, lsb, fault=None):
    """``dconv_kernel<..., POOL>``: ReLU conv, rounded per element, then the window max of the
    rounded values.  Fault ``pool_outside_live``: the conv positions a padded window reaches
    beyond [0, Ho) x [0, Wo) are computed from more zero padding and enter the max."""
    N, H, W, _ = x.shape
    KH, KW = w.shape[1:3]
    Ho, Wo = _out_hw(H, W, KH, KW, s, pad)
    Hp, Wp = _pool_hw(Ho, Wo, ppad)
    assert Hp >= 1 and (Hp - 1) * 2 + 3 <= Ho + ppad[0] + ppad[1] and (Wp - 1) * 2 + 3 <= Wo + ppad[2] + ppad[3]
    if fault == "pool_outside_live":
        pad = tuple(p + q * s for p, q in zip(pad, ppad))
        ppad = (0, 0, 0, 0)
        fault = None
    y, tr = ref_plain(x, w, scale, bias, s, pad, "relu", out_q, es, lsb, fault=fault if fault in CONV_FAULTS else None)
    vals = y if out_q is None else _dec(y)
    assert (vals >= 0).all()                     # the unsigned-integer max of the kernel needs it
    m = _pool3x3s2(vals, ppad, Hp, Wp, fault)
    tr.note(pooled_zero=(m == 0).double().mean().item())
    return (m if out_q is None else _e4m3(m)), tr


def ref_patch(xu8, mean, std, fault=None):
    """The uint8 stem's patch source: the normalised 2x2 space-to-depth image
    [N, ceil(Hi/2), ceil(Wi/2), 16] as float64 bf16 values.  Fault ``s2d_phase``: a and b
    exchanged.  Returns (blocks, share of values the bf16 rounding changed)."""
    N, Hi, Wi, _ = xu8.shape
    Hb, Wb = (Hi + 1) // 2, (Wi + 1) // 2
    tr = _Trace()
    d = tr.exact(xu8.double() - torch.tensor(mean, dtype=F64), "v - mean")
    istd = _f32(1.0 / torch.tensor(std, dtype=F64))
    v = tr.exact(d * istd, "(v - mean) * istd")
    p = _bf(v)
    full = torch.zeros((N, 2 * Hb, 2 * Wb, 3), dtype=F64)
    full[:, :Hi, :Wi] = p
    blk = torch.zeros((N, Hb, Wb, 16), dtype=F64)
    for a in range(2):
        for b in range(2):
            for c in range(3):
                ch = ((2 * b + a) if fault == "s2d_phase" else (2 * a + b)) * 3 + c
                blk[..., ch] = full[:, a::2, b::2, c]
    return blk, (p != v).double().mean().item()


# ----------------------------------------------------------------------------------- the data
Plain = collections.namedtuple("Plain", "kind N H W Cin Cout k s pad")
Pooled = collections.namedtuple("Pooled", "kind N H W Cin Cout k s pad ppad")
Stem = collections.namedtuple("Stem", "N Hi Wi Cout k pad")

PLAIN = (
    Plain("bf16", 2, 71, 39, 8, 40, (3, 3), 2, (0, 1, 0, 1)),     # 35 x 19; K 144 B -> 192; Cout 40
    Plain("bf16", 2, 35, 19, 16, 64, (4, 4), 1, (2, 1, 2, 1)),    # the s2d stem form, K 512 B exact
    Plain("bf16", 1, 5, 3, 64, 8, (3, 3), 1, (1, 1, 1, 1)),       # one partial tile, smallest Cout
    Plain("bf16", 1, 16, 16, 32, 32, (1, 7), 1, (0, 0, 3, 3)),    # exactly one 4-wave tile
    Plain("bf16", 3, 32, 16, 8, 72, (7, 1), 1, (3, 3, 0, 0)),     # exactly one 8-wave tile
    Plain("bf16", 2, 34, 38, 16, 48, (3, 3), 2, (1, 1, 1, 1)),    # stride 2 with top / left padding
    Plain("bf16", 1, 20, 18, 64, 32, (5, 5), 1, (2, 2, 2, 2)),    # 50 K-steps; 8 waves fall back; bn 64 refused
    Plain("fp8", 2, 35, 19, 32, 48, (3, 3), 1, (1, 1, 1, 1)),     # K 288 B -> 384
    Plain("fp8", 1, 17, 17, 128, 64, (1, 7), 1, (0, 0, 3, 3)),    # K 896 B exact, largest 8-wave patch
    Plain("fp8", 2, 37, 41, 64, 96, (3, 3), 2, (0, 1, 0, 1)),     # stride 2; K 576 B -> 640
    Plain("fp8", 1, 5, 3, 32, 16, (3, 3), 1, (1, 1, 1, 1)),       # one partial tile
)
POOLED = (
    Pooled("bf16", 2, 35, 19, 16, 64, (4, 4), 1, (2, 1, 2, 1), "SAME"),      # pads (1,1,1,1), 18 x 10
    Pooled("bf16", 1, 33, 30, 16, 40, (3, 3), 1, (1, 1, 1, 1), "VALID"),     # 16 x 14, Cout 40
    Pooled("bf16", 1, 16, 16, 16, 32, (3, 3), 1, (1, 1, 1, 1), (0, 1, 0, 1)),  # 8 x 8: one row past a 7-row tile
    Pooled("bf16", 1, 40, 40, 16, 64, (7, 7), 2, (2, 3, 2, 3), "SAME"),      # stride-2 conv; 14 rows fall back at bn 64
    Pooled("fp8", 2, 37, 37, 32, 64, (3, 3), 1, (0, 0, 0, 0), "VALID"),
    Pooled("fp8", 1, 30, 41, 32, 32, (3, 3), 1, (1, 1, 1, 1), "SAME"),
)
STEMS = (
    Stem(2, 37, 35, 32, (3, 3), (0, 0, 0, 0)),      # odd both ways -> 2x2 blocks
    Stem(2, 70, 38, 64, (7, 7), (2, 3, 2, 3)),      # -> 4x4 blocks, 35 x 19 output
    Stem(1, 32, 32, 40, (7, 7), (2, 3, 2, 3)),      # even, one 4-wave tile, Cout 40
    Stem(1, 33, 31, 16, (4, 4), (0, 1, 0, 1)),      # odd, and the pixels past the edge meet non-zero weights
)


def _cid(c):
    if isinstance(c, Stem):
        return f"u8-{c.N}x{c.Hi}x{c.Wi}-{c.Cout}-{c.k[0]}x{c.k[1]}"
    tail = "" if isinstance(c, Plain) else "-pool" + (c.ppad if isinstance(c.ppad, str) else "".join(map(str, c.ppad)))
    return f"{c.kind}-{c.N}x{c.H}x{c.W}x{c.Cin}-{c.Cout}-{c.k[0]}x{c.k[1]}s{c.s}{tail}"


def _es(kind):
    return 2 if kind == "bf16" else 1


def _lsb(kind):
    return {"bf16": 0.5, "fp8": 2.0 ** -7, "u8": 2.0 ** -8}[kind]


def _out_cout(c, out_fp8):
    """The e4m3 variant of a case whose Cout is no multiple of 16 uses the next multiple."""
    return _round_up(c.Cout, 16) if out_fp8 else c.Cout


def _ppad(c):
    KH, KW = c.k
    Ho, Wo = _out_hw(c.H, c.W, KH, KW, c.s, c.pad)
    return {"SAME": _same_pool_pads(Ho, Wo), "VALID": (0, 0, 0, 0)}.get(c.ppad, c.ppad)


# The single-tile fp8 case has 240 outputs and ~1 % saturate at out_scale 1/8: its stream is the
# first of its seeds (0, 1, ..) with a saturated output under both activations.
SALT = {("fp8", 1, 5, 3, 32, 16, (3, 3)): (9,)}


@functools.lru_cache(maxsize=None)
def _data(kind, N, H, W, Cin, Cout, k):
    """(x [N, H, W, Cin], w [Cout, KH, KW, Cin], scale [Cout], bias [Cout]) as float64."""
    key = (kind, N, H, W, Cin, Cout, k)
    g = torch.Generator().manual_seed(zlib.crc32(repr(key + SALT.get(key, ())).encode()))
    w = torch.randint(-4, 5, (Cout, *k, Cin), generator=g).to(F64)
    if kind == "bf16":
        x = torch.randint(-8, 9, (N, H, W, Cin), generator=g).to(F64)
        return x, w, torch.ones(Cout, dtype=F64), torch.randint(-1200, 1201, (Cout,), generator=g).to(F64) / 2
    x = torch.randint(0, 9, (N, H, W, Cin), generator=g).to(F64)
    scale = 2.0 ** -(3 + (torch.arange(Cout) * 3 + 1) % 5).to(F64)
    return x, w, scale, torch.randint(-32, 33, (Cout,), generator=g).to(F64) / 4


@functools.lru_cache(maxsize=None)
def _stem_data(c, Cout):
    """(x uint8 [N, Hi, Wi, 3], w_hwio float64 [KH, KW, 3, Cout], bias float64, w2 [Cout, KBH, KBW, 16],
    block pads)."""
    g = torch.Generator().manual_seed(zlib.crc32(repr((tuple(c), Cout)).encode()))
    x = torch.randint(0, 256, (c.N, c.Hi, c.Wi, 3), generator=g).to(U8)
    w = torch.randint(-4, 5, (*c.k, 3, Cout), generator=g).to(F64)
    bias = torch.randint(-128, 129, (Cout,), generator=g).to(F64) / 4
    w2, bpad = K.s2d_stem_weights(w, c.Hi, c.Wi, c.pad)
    return x, w, bias, w2.double(), tuple(bpad)


@functools.lru_cache(maxsize=None)
def _plain_ref(c, out_fp8, act, out_scale, fault=None):
    x, w, scale, bias = _data(c.kind, c.N, c.H, c.W, c.Cin, _out_cout(c, out_fp8), c.k)
    return ref_plain(x, w, scale, bias, c.s, c.pad, act, 1.0 / out_scale if out_fp8 else None, _es(c.kind),
                     _lsb(c.kind), fault=fault)


@functools.lru_cache(maxsize=None)
def _pooled_ref(c, out_scale, fault=None):
    x, w, scale, bias = _data(c.kind, c.N, c.H, c.W, c.Cin, c.Cout, c.k)
    return ref_pooled(x, w, scale, bias, c.s, c.pad, _ppad(c), None if c.kind == "bf16" else 1.0 / out_scale,
                      _es(c.kind), _lsb(c.kind), fault=fault)


@functools.lru_cache(maxsize=None)
def _stem_ref(c, out_fp8, act, out_scale, fault=None):
    Cout = _out_cout(c, out_fp8)
    x, _, bias, w2, bpad = _stem_data(c, Cout)
    blk, changed = ref_patch(x, U8_MEAN, U8_STD, fault)
    tr = _Trace()
    tr.note(patch_changed=changed)
    return ref_plain(blk, w2, torch.ones(Cout, dtype=F64), bias, 1, bpad, act, 1.0 / out_scale if out_fp8 else None, 2,
                     _lsb("u8"), unit=_lsb("u8"), fault=fault if fault in CONV_FAULTS else None, tr=tr)


def _out_scales(kind, out_fp8):
    if not out_fp8:
        return (None,)
    return {"bf16": BF16_OUT_SCALES, "fp8": FP8_OUT_SCALES, "u8": U8_OUT_SCALES}[kind]


def _variants(kind):
    """(out_fp8, act, out_scale) of the plain sweep."""
    return [(o, a, s) for o in (False, True) for a in (None, "relu") for s in _out_scales(kind, o)]


# ============================================================================ CPU: the mirrors
def _observable(tr, out_fp8, act, what):
    st = tr.stats
    assert st["changed"] >= 0.05, f"{what}: the output rounding changes only {st['changed']:.3f}"
    if act == "relu":
        assert st["zeroed"] >= 0.05 and st["passed"] >= 0.05, (what, st)


@pytest.mark.parametrize("case", PLAIN, ids=_cid)
def test_plain_mirror_equals_host_paths(case):
    """bf16 in: ``K.conv2d_nhwc`` on the host accumulates in fp32 (exact on these data) and
    returns the unrounded fp32 value, so its bf16 output is compared after one ``bf16_rne``;
    with ``out_scale`` it rounds once to e4m3 like the kernel.  fp8 in: ``Q.conv2d_nhwc_fp8``
    scales the weights before the sum instead of the sum after it, exact for power-of-two
    scales; bf16 again rounded here, e4m3 in the same place."""
    KH, KW = case.k
    sat = sub = 0
    for out_fp8, act, so in _variants(case.kind):
        x, w, scale, bias = _data(case.kind, case.N, case.H, case.W, case.Cin, _out_cout(case, out_fp8), case.k)
        y, tr = _plain_ref(case, out_fp8, act, so)
        what = f"{_cid(case)} out_fp8={out_fp8} act={act} out_scale={so}"
        if case.kind == "bf16":
            host = K.conv2d_nhwc(x.float(), w.float(), bias.float(), None, (case.s, case.s), case.pad, (1, 1), act,
                                 out_scale=so)
        else:
            host = Q.conv2d_nhwc_fp8(_e4m3(x), 1.0, _e4m3(w).reshape(w.shape[0], -1), (KH, KW), scale.float(),
                                     bias.float(), (case.s, case.s), case.pad, act=act, out_scale=so)
        assert host.shape == y.shape
        if out_fp8:
            assert torch.equal(_canon(host), _canon(y)), what
            sat += tr.stats["saturated"] * (so == min(_out_scales(case.kind, True)))
            sub += tr.stats["subnormal"] * (so == max(_out_scales(case.kind, True)))
        else:
            assert host.dtype == F32 and torch.equal(_bf(host.double()), y), what
        _observable(tr, out_fp8, act, what)
    # the smallest and the largest out_scale are there for saturation and for subnormals
    assert sat > 0, f"{_cid(case)}: no output saturates at 448"
    if case.kind == "fp8":
        assert sub > 0, f"{_cid(case)}: no subnormal output"


def _applies(fault, case, out_fp8):
    KH, KW = case.k
    pt, pb, pl, pr = case.pad
    if fault == "tap_swap":
        return KH * KW > 1
    if fault == "edge_pad":
        return _pad_is_read(case.H, case.W, KH, KW, case.s, case.pad)
    if fault == "pad_swapped":
        return (pt, pl) != (pb, pr)
    if fault == "round_via_bf16":
        return out_fp8
    return fault in ("drop_kstep", "scale_shift4")


@pytest.mark.parametrize("case", PLAIN, ids=_cid)
def test_plain_faults_change_every_case(case):
    for out_fp8, act, so in _variants(case.kind):
        if so is not None and so != _out_scales(case.kind, True)[1 if case.kind != "u8" else 0]:
            continue                            # one out_scale is enough for the wrong variants
        y, _ = _plain_ref(case, out_fp8, act, so)
        for fault in CONV_FAULTS:
            if _applies(fault, case, out_fp8):
                z, _ = _plain_ref(case, out_fp8, act, so, fault)
                assert z.shape == y.shape and not torch.equal(_bits(z), _bits(y)), (fault, out_fp8, act, so)


@pytest.mark.parametrize("case", POOLED, ids=_cid)
def test_pooled_mirror_equals_host_paths_and_faults_show(case):
    """conv (host path, rounded as in ``test_plain_mirror_equals_host_paths``), then
    ``K.pool2d_nhwc`` / ``Q.pool2d_nhwc_fp8`` of the rounded tensor: the same places."""
    KH, KW = case.k
    x, w, scale, bias = _data(case.kind, case.N, case.H, case.W, case.Cin, case.Cout, case.k)
    ppad = _ppad(case)
    assert (bias > 0).sum() >= 4 and (bias < 0).sum() >= 4     # an unmasked outside position would win
    for so in _out_scales(case.kind, case.kind == "fp8"):
        y, tr = _pooled_ref(case, so)
        if case.kind == "bf16":
            conv = K.conv2d_nhwc(x.float(), w.float(), bias.float(), None, (case.s, case.s), case.pad, (1, 1), "relu")
            host = K.pool2d_nhwc(conv.to(BF).float(), (3, 3), (2, 2), ppad, "max").double()
            assert torch.equal(host, y)
        else:
            conv = Q.conv2d_nhwc_fp8(_e4m3(x), 1.0, _e4m3(w).reshape(case.Cout, -1), (KH, KW), scale.float(),
                                     bias.float(), (case.s, case.s), case.pad, act="relu", out_scale=so)
            host = Q.pool2d_nhwc_fp8(conv, (3, 3), (2, 2), ppad, "max")
            assert torch.equal(_canon(host), _canon(y))
        _observable(tr, case.kind == "fp8", "relu", f"{_cid(case)} out_scale={so}")
        assert 0.02 <= tr.stats["pooled_zero"] <= 0.9, tr.stats
        for fault in ("tap_swap", "drop_kstep", "scale_shift4", "pool_outside_live", "pool_shift"):
            z, _ = _pooled_ref(case, so, fault)
            assert z.shape == y.shape
            if fault in ("pool_outside_live", "pool_shift") and not any(ppad):
                # an unpadded (VALID) pool has no window that reaches outside the conv output
                # and no pad to get wrong: these two variants cannot differ there
                assert torch.equal(_bits(z), _bits(y)), fault
            else:
                assert not torch.equal(_bits(z), _bits(y)), (fault, so)


@pytest.mark.parametrize("case", STEMS, ids=_cid)
def test_stem_mirror_equals_host_paths_and_faults_show(case):
    """``K.preprocess_images(..., s2d=True)`` on the host keeps fp32 (the device writes bf16): its
    output is exact on these data and is rounded here; then ``K.conv2d_nhwc`` as above."""
    blk, changed = ref_patch(_stem_data(case, case.Cout)[0], U8_MEAN, U8_STD)
    assert changed >= 0.05, f"the patch's f2bf changes only {changed:.3f}"
    x = _stem_data(case, case.Cout)[0]
    pre = K.preprocess_images(x, (case.Hi, case.Wi), U8_MEAN, U8_STD, s2d=True)
    assert pre.dtype == F32 and torch.equal(_bf(pre.double()), blk)
    assert (blk[..., 12:] == 0).all()
    if case.Hi % 2:
        assert (blk[:, -1, :, 6:12] == 0).all()           # a = 1 of the last block row is past the image
    if case.Wi % 2:
        assert (blk[:, :, -1, 3:6] == 0).all() and (blk[:, :, -1, 9:12] == 0).all()
    for out_fp8, act, so in _variants("u8"):
        Cout = _out_cout(case, out_fp8)
        _, _, bias, w2, bpad = _stem_data(case, Cout)
        blk_c = ref_patch(_stem_data(case, Cout)[0], U8_MEAN, U8_STD)[0]
        y, tr = _stem_ref(case, out_fp8, act, so)
        host = K.conv2d_nhwc(blk_c.float(), w2.float(), bias.float(), None, (1, 1), bpad, (1, 1), act, out_scale=so)
        what = f"{_cid(case)} out_fp8={out_fp8} act={act}"
        if out_fp8:
            assert torch.equal(_canon(host), _canon(y)), what
        else:
            assert torch.equal(_bf(host.double()), y), what
        _observable(tr, out_fp8, act, what)
        KH, KW = w2.shape[1:3]
        geo = Plain("u8", case.N, blk.shape[1], blk.shape[2], 16, Cout, (KH, KW), 1, bpad)
        for fault in ("s2d_phase",) + CONV_FAULTS:
            if fault == "s2d_phase" or _applies(fault, geo, out_fp8):
                z, _ = _stem_ref(case, out_fp8, act, so, fault)
                assert not torch.equal(_bits(z), _bits(y)), (fault, what)


def test_stem_is_the_strided_conv_of_the_normalised_image():
    """The whole uint8 mirror (patch layout + s2d weights + block pads) against the stride-2
    conv it stands for, taps looped over the normalised RGB image itself."""
    for case in STEMS:
        x, w, bias, _, _ = _stem_data(case, case.Cout)
        y, _ = _stem_ref(case, False, None, None)
        img = _bf(_f32(x.double() - torch.tensor(U8_MEAN, dtype=F64)) * _f32(1.0 / torch.tensor(U8_STD, dtype=F64)))
        acc, _ = _conv_acc(_Trace(), img, w.permute(3, 0, 1, 2), 2, case.pad, 2, _lsb("u8"))
        assert torch.equal(_bf(acc + bias), y), _cid(case)


def test_lds_budget_and_wave_fallback_figures():
    """The tile sizes the cases are chosen by."""
    assert _lds_bytes(2, 32, 5, 5, 1, 64, False, 8) == 196096 and _lds_bytes(2, 32, 5, 5, 1, 64, False, 4) == 155136
    assert _eff_waves(2, 32, 5, 5, 1, 64, False, 8) == 4 and _eff_waves(2, 64, 5, 5, 1, 64, False, 4) is None
    assert _lds_bytes(1, 64, 1, 7, 1, 128, False, 8) == 149504 and _eff_waves(1, 64, 1, 7, 1, 128, False, 8) == 8
    assert _lds_bytes(2, 64, 7, 7, 2, 16, True, 8) == 188416 and _lds_bytes(2, 64, 7, 7, 2, 16, True, 4) == 151552
    assert _eff_waves(2, 64, 7, 7, 2, 16, True, 8) == 4 and _eff_waves(2, 32, 7, 7, 2, 16, True, 8) == 8
    for c in PLAIN + POOLED:
        for bn in (32, 64):
            for waves in (4, 8):
                eff = _eff_waves(_es(c.kind), bn, *c.k, c.s, c.Cin, isinstance(c, Pooled), waves)
                assert eff is not None or (c.k == (5, 5) and bn == 64)


@pytest.mark.parametrize("es,bn,Cout,k,Cin", [(2, 32, 40, (3, 3), 8), (2, 64, 40, (3, 3), 8), (2, 64, 64, (4, 4), 16),
                                              (2, 32, 8, (3, 3), 64), (1, 32, 48, (3, 3), 32), (1, 64, 96, (3, 3), 64),
                                              (1, 64, 64, (1, 7), 128), (2, 64, 72, (7, 1), 8)])
def test_weight_layout(es, bn, Cout, k, Cin):
    """Pitch = round_up(K bytes, 4 * KL) + 16; the K padding (the kernel reads it against tap 0
    of the patch) and the rows from Cout to round_up(Cout, bn) (DMA'd by the last channel tile)
    are zero."""
    kind = "bf16" if es == 2 else "fp8"
    _, w, _, _ = _data(kind, 1, 4, 4, Cin, Cout, k)
    kb = k[0] * k[1] * Cin * es
    if es == 2:
        arr = K.dconv_bf16_weight_bytes(w.float(), bn)
        src = w.to(BF).reshape(Cout, -1).view(U8)
    else:
        src = _e4m3(w).reshape(Cout, -1)
        arr = K.dconv_weights(src, Cout, 1, bn)
    kl = 16 if es == 2 else 32
    assert arr.dtype == U8 and arr.is_contiguous()
    assert tuple(arr.shape) == (_round_up(Cout, bn), _round_up(kb, 4 * kl) + 16)
    assert torch.equal(arr[:Cout, :kb], src)
    assert (arr[:, kb:] == 0).all() and (arr[Cout:] == 0).all()
    if es == 2:      # K order (kh, kw, ci), little-endian bf16
        back = arr[:Cout, :kb].contiguous().view(BF).double().reshape(Cout, *k, Cin)
        assert torch.equal(back, w)


def test_host_side_refusals_need_no_device():
    x = torch.zeros((1, 16, 16, 16), dtype=BF)
    arr = K.dconv_bf16_weight_bytes(torch.zeros(32, 3, 3, 16), 32)
    b = torch.zeros(32)
    with pytest.raises(ValueError, match="stride"):
        K.conv2d_direct(x, arr, (3, 3), 32, b, (1, 2), (1, 1, 1, 1), "relu", bn=32)
    with pytest.raises(ValueError, match="stride"):
        K.conv2d_direct(x, arr, (3, 3), 32, b, (2, 1), (1, 1, 1, 1), "relu", bn=32)
    with pytest.raises(ValueError, match="chan_scale"):
        K.conv2d_direct(torch.zeros((1, 16, 16, 32), dtype=U8), arr, (3, 3), 32, b, (1, 1), (1, 1, 1, 1), bn=32)
    with pytest.raises(ValueError, match="cannot hold"):
        K.conv2d_direct(x, arr, (3, 3), 32, b, (1, 1), (1, 1, 1, 1), out=torch.zeros((1, 16, 15, 32), dtype=BF), bn=32)
    with pytest.raises(ValueError, match="cannot hold"):
        K.conv2d_direct(x, arr, (3, 3), 32, b, (1, 1), (1, 1, 1, 1), out=torch.zeros((1, 16, 16, 40), dtype=BF),
                        out_channel_offset=16, bn=32)
    with pytest.raises(TypeError):
        K.conv2d_direct(x, arr.float(), (3, 3), 32, b, (1, 1), (1, 1, 1, 1), bn=32)
    with pytest.raises(TypeError):
        K.conv2d_direct(x, arr, (3, 3), 32, b.to(BF), (1, 1), (1, 1, 1, 1), bn=32)
    with pytest.raises(TypeError):
        K.conv2d_direct(x, arr, (3, 3), 32, b, (1, 1), (1, 1, 1, 1), out=torch.zeros((1, 16, 16, 32)), bn=32)


# ================================================================================ GPU harness
def _dev():
    return torch.device("cuda", 0)


def _banded(t, fill, dev):
    """``t`` as a view into a larger allocation filled with ``fill`` -> (view, whole buffer)."""
    n = t.numel()
    buf = torch.full((BAND + n + BAND,), fill, dtype=t.dtype, device=dev)
    v = buf[BAND:BAND + n].view(t.shape)
    v.copy_(t)
    return v, buf


def _is_fill(h, fill):
    return torch.isnan(h) if isinstance(fill, float) and fill != fill else h == fill


def _bands_intact(buf, t, fill, what):
    """Both bands still hold ``fill`` and the operand between them came back unchanged."""
    h, n = buf.cpu(), t.numel()
    assert _is_fill(h[:BAND], fill).all() and _is_fill(h[BAND + n:], fill).all(), f"{what}: band overwritten"
    assert torch.equal(h[BAND:BAND + n].view(t.shape), t), f"{what}: operand changed"


class _Operands:
    """The device operands of one case, each between guard bands."""

    def __init__(self, dev, **host):
        self.host, self.fill, self.buf = {}, {}, {}
        for name, t in host.items():
            if t is None:
                setattr(self, name, None)
                continue
            fill = float("nan") if t.dtype.is_floating_point else (PIX8 if name == "xu8" else NAN8)
            v, buf = _banded(t, fill, dev)
            setattr(self, name, v)
            self.host[name], self.fill[name], self.buf[name] = t, fill, buf

    def intact(self, what):
        for name, t in self.host.items():
            _bands_intact(self.buf[name], t, self.fill[name], f"{what}: {name}")


def _launch_twice(run, shape3, Cout, out_fp8, dev, what, slot=True):
    """Runs ``run(out, channel offset)`` twice into fresh sentinel buffers: the output is a slot
    of a wider row (pitch Cout + 32, offset 16; ``slot=False``: contiguous; ``slot="tail"``: offset
    0) between sentinel bands.  Requires identical bytes, intact bands and neighbours; returns
    the slot on the host."""
    ld, off = {True: (Cout + 32, 16), False: (Cout, 0), "tail": (Cout + 32, 0)}[slot]
    n = shape3[0] * shape3[1] * shape3[2] * ld
    sent, dt = (SENT8, U8) if out_fp8 else (SENT16, BF)
    runs = []
    for _ in range(2):
        obuf = torch.full((BAND + n + BAND,), sent, dtype=dt, device=dev)
        out = obuf[BAND:BAND + n].view(*shape3, ld)
        r = run(out, off)
        assert r is out or r.data_ptr() == out.data_ptr()
        runs.append(obuf.cpu())
    a, b = (r.view(torch.int16) if dt == BF else r for r in runs)
    assert torch.equal(a, b), f"{what}: two launches differ"
    o = runs[0]
    assert (o[:BAND] == sent).all() and (o[BAND + n:] == sent).all(), f"{what}: stray store outside the output"
    o = o[BAND:BAND + n].view(*shape3, ld)
    assert (o[..., :off] == sent).all() and (o[..., off + Cout:] == sent).all(), f"{what}: neighbours of the slot written"
    return o[..., off:off + Cout].contiguous()


def _show(t, n, y, x, c):
    v = t[n, y, x, c]
    if t.dtype == U8:
        return f"0x{int(v):02x} ({float(_dec(v.reshape(1))[0])})"
    return f"{float(v)} (0x{int(_bits(v.reshape(1))[0]) & 0xFFFF:04x})"


def _exact(got, ref, what, where):
    """Equality on bits / canonical bytes; on failure the first mismatches with their place."""
    ref = ref if ref.dtype == U8 else ref.to(BF)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype)
    bad = (_bits(got) != _bits(ref)).nonzero()
    if len(bad) == 0:
        return
    lines = [f"{what}: {len(bad)} of {ref.numel()} differ"]
    for n, y, x, c in bad[:6].tolist():
        lines.append(f"  image {n} {where(y, x, c)} pixel ({y}, {x}) channel {c}: got {_show(got, n, y, x, c)} "
                     f"want {_show(ref, n, y, x, c)}")
    raise AssertionError("\n".join(lines))


def _where_plain(waves, bn):
    """Plain tiles are 4 * waves rows x 16 columns; wave w owns tile rows 4w .. 4w + 3."""
    rows = 4 * waves
    return lambda y, x, c: (f"tile row {y // rows} col {x // 16} channel tile {c // bn} wave {y % rows // 4} "
                            f"(of {waves})")


def _where_pooled(waves, bn):
    """Pooled tiles are 7 (4 waves) or 14 (8) x 8 pooled pixels over a 17-column conv tile whose
    pixel p = row * 17 + col belongs to wave p // 64; a window spans three conv rows."""
    rows = 7 * waves // 4

    def where(y, x, c):
        p0 = (2 * (y % rows)) * 17 + 2 * (x % 8)
        return (f"tile row {y // rows} col {x // 8} channel tile {c // bn} waves {p0 // 64}..{(p0 + 36) // 64} "
                f"(of {waves})")
    return where


def _device_weights(kind, w, Cout, bn):
    if kind == "fp8":
        return K.dconv_weights(_e4m3(w).reshape(Cout, -1), Cout, 1, bn)
    return K.dconv_bf16_weight_bytes(w.float(), bn)


def _operands(kind, x, w, scale, bias, Cout, bn, dev):
    return _Operands(dev, x=x.to(BF) if kind == "bf16" else _e4m3(x), w=_device_weights(kind, w, Cout, bn),
                     bias=bias.to(F32), scale=None if kind == "bf16" else scale.to(F32))


# ================================================================================== GPU: plain
@pytest.mark.gpu
@pytest.mark.parametrize("bn", (32, 64))
@pytest.mark.parametrize("waves", (4, 8))
@pytest.mark.parametrize("case", PLAIN, ids=_cid)
def test_plain_bit_exact_gpu(case, waves, bn):
    """Every act x output type of the plain kernel at this tile configuration.  A wave count
    that does not fit LDS must silently run the 4-wave kernel (same bytes as the mirror); a
    channel tile whose 4-wave tile does not fit must be refused."""
    dev = _dev()
    KH, KW = case.k
    es = _es(case.kind)
    eff = _eff_waves(es, bn, KH, KW, case.s, case.Cin, False, waves)
    Ho, Wo = _out_hw(case.H, case.W, KH, KW, case.s, case.pad)
    for out_fp8 in (False, True):
        Cout = _out_cout(case, out_fp8)
        x, w, scale, bias = _data(case.kind, case.N, case.H, case.W, case.Cin, Cout, case.k)
        ops = _operands(case.kind, x, w, scale, bias, Cout, bn, dev)
        for act in (None, "relu"):
            for so in _out_scales(case.kind, out_fp8):
                what = f"{_cid(case)} waves={waves} (runs {eff}) bn={bn} act={act} out_fp8={out_fp8} out_scale={so}"

                def run(out, off):
                    return K.conv2d_direct(ops.x, ops.w, case.k, Cout, ops.bias, (case.s, case.s), case.pad, act,
                                           out=out, out_channel_offset=off, bn=bn, chan_scale=ops.scale, out_scale=so,
                                           waves=waves)
                if eff is None:
                    with pytest.raises(ValueError, match="LDS"):
                        run(torch.empty((case.N, Ho, Wo, Cout), dtype=U8 if out_fp8 else BF, device=dev), 0)
                    continue
                ref, _ = _plain_ref(case, out_fp8, act, so)
                got = _launch_twice(run, (case.N, Ho, Wo), Cout, out_fp8, dev, what)
                _exact(got, ref, what, _where_plain(eff, bn))
        ops.intact(f"{_cid(case)} waves={waves} bn={bn} out_fp8={out_fp8}")


# ================================================================================= GPU: pooled
@pytest.mark.gpu
@pytest.mark.parametrize("bn", (32, 64))
@pytest.mark.parametrize("pool_rows", (7, 14))
@pytest.mark.parametrize("case", POOLED, ids=_cid)
def test_pooled_bit_exact_gpu(case, pool_rows, bn):
    """ReLU conv + fused max pool, bf16 -> bf16 and fp8 -> fp8, contiguous and into a concat
    slot.  Where the 14-row tile does not fit LDS the 7-row kernel runs: same mirror, so the
    two ``pool_rows`` runs are equal too."""
    dev = _dev()
    KH, KW = case.k
    es = _es(case.kind)
    waves = {7: 4, 14: 8}[pool_rows]
    eff = _eff_waves(es, bn, KH, KW, case.s, case.Cin, True, waves)
    assert eff is not None
    ppad = _ppad(case)
    Hp, Wp = _pool_hw(*_out_hw(case.H, case.W, KH, KW, case.s, case.pad), ppad)
    x, w, scale, bias = _data(case.kind, case.N, case.H, case.W, case.Cin, case.Cout, case.k)
    ops = _operands(case.kind, x, w, scale, bias, case.Cout, bn, dev)
    out_fp8 = case.kind == "fp8"
    for so in _out_scales(case.kind, out_fp8):
        ref, _ = _pooled_ref(case, so)
        assert tuple(ref.shape) == (case.N, Hp, Wp, case.Cout)
        for slot in (False, True):
            what = f"{_cid(case)} pool_rows={pool_rows} (runs {eff} waves) bn={bn} out_scale={so} slot={slot}"

            def run(out, off):
                return K.conv2d_direct(ops.x, ops.w, case.k, case.Cout, ops.bias, (case.s, case.s), case.pad, "relu",
                                       out=out, out_channel_offset=off, bn=bn, chan_scale=ops.scale, out_scale=so,
                                       maxpool_pad=ppad, pool_rows=pool_rows)
            got = _launch_twice(run, (case.N, Hp, Wp), case.Cout, out_fp8, dev, what, slot=slot)
            _exact(got, ref, what, _where_pooled(eff, bn))
    ops.intact(f"{_cid(case)} pool_rows={pool_rows} bn={bn}")


# ============================================================================= GPU: uint8 stem
@pytest.mark.gpu
@pytest.mark.parametrize("bn", (32, 64))
@pytest.mark.parametrize("waves", (4, 8))
@pytest.mark.parametrize("case", STEMS, ids=_cid)
def test_u8_stem_bit_exact_gpu(case, waves, bn):
    """``dconv_u8s2d``: the patch built from the raw bytes.  The launcher takes no channel
    offset: the output row is wider than Cout and its tail keeps the sentinel."""
    dev = _dev()
    for out_fp8 in (False, True):
        Cout = _out_cout(case, out_fp8)
        x, _, bias, w2, bpad = _stem_data(case, Cout)
        KBH, KBW = w2.shape[1:3]
        eff = _eff_waves(2, bn, KBH, KBW, 1, 16, False, waves)
        Ho, Wo = _out_hw((case.Hi + 1) // 2, (case.Wi + 1) // 2, KBH, KBW, 1, bpad)
        ops = _Operands(dev, xu8=x, w=K.dconv_bf16_weight_bytes(w2.float(), bn), bias=bias.to(F32))
        for act in (None, "relu"):
            for so in _out_scales("u8", out_fp8):
                what = f"{_cid(case)} waves={waves} bn={bn} act={act} out_fp8={out_fp8} out_scale={so}"
                ref, _ = _stem_ref(case, out_fp8, act, so)
                assert tuple(ref.shape) == (case.N, Ho, Wo, Cout)

                def run(out, off):
                    assert off == 0
                    return K.conv2d_direct_u8s2d(ops.xu8, ops.w, (KBH, KBW), Cout, ops.bias, bpad, act, U8_MEAN,
                                                 U8_STD, out=out, bn=bn, out_scale=so, waves=waves)
                got = _launch_twice(run, (case.N, Ho, Wo), Cout, out_fp8, dev, what, slot="tail")
                _exact(got, ref, what, _where_plain(eff, bn))
        ops.intact(f"{_cid(case)} waves={waves} bn={bn} out_fp8={out_fp8}")


# ============================================================================== GPU: refusals
@pytest.mark.gpu
def test_launcher_refusals_gpu():
    """Raised on the host before any launch."""
    dev = _dev()
    x = torch.zeros((1, 16, 16, 16), dtype=BF, device=dev)
    arr = K.dconv_bf16_weight_bytes(torch.zeros(32, 3, 3, 16), 32).to(dev)
    b = torch.zeros(64, device=dev)
    x8 = torch.zeros((1, 16, 16, 32), dtype=U8, device=dev)
    arr8 = K.dconv_weights(torch.zeros((32, 288), dtype=U8), 32, 1, 32).to(dev)
    cs = torch.ones(32, device=dev)

    def call(x=x, w=arr, k=(3, 3), Cout=32, bias=b, stride=(1, 1), pad=(1, 1, 1, 1), act="relu", bn=32, **kw):
        return K.conv2d_direct(x, w, k, Cout, bias, stride, pad, act, bn=bn, **kw)

    def out(c, dt=BF, hw=(16, 16)):
        return torch.zeros((1, *hw, c), dtype=dt, device=dev)

    refused = {
        "bn 48": dict(bn=48),
        "Cin * es no multiple of KL": dict(x=torch.zeros((1, 16, 16, 4), dtype=BF, device=dev)),
        "fp8 Cin * es no multiple of KL": dict(x=torch.zeros((1, 16, 16, 16), dtype=U8, device=dev), w=arr8, chan_scale=cs),
        "weight pitch": dict(w=torch.zeros((32, arr.shape[1] + 16), dtype=U8, device=dev)),
        "stride 3": dict(stride=(3, 3)),
        "stride differs per axis": dict(stride=(1, 2)),
        "pooled, act none": dict(act=None, maxpool_pad=(0, 1, 0, 1)),
        "pooled bf16 -> fp8": dict(maxpool_pad=(0, 1, 0, 1), out_scale=1.0),
        "pooled fp8 -> bf16": dict(x=x8, w=arr8, chan_scale=cs, maxpool_pad=(0, 1, 0, 1)),
        "pool pad 2": dict(maxpool_pad=(2, 0, 0, 0)),
        "pool pad 2 left": dict(maxpool_pad=(0, 0, 2, 0)),
        "pooled shape inconsistent": dict(maxpool_pad=(0, 3, 0, 0)),
        "pooled shape inconsistent, width": dict(maxpool_pad=(0, 0, 0, 3)),
        "Cout % 8": dict(Cout=36),
        "row width % 8": dict(out=out(36)),
        "offset % 8": dict(out=out(48), out_channel_offset=4),
        "e4m3 Cout % 16": dict(Cout=40, out_scale=1.0),
        "e4m3 row width % 16": dict(out=out(40, U8), out_scale=1.0),
        "e4m3 offset % 16": dict(out=out(64, U8), out_channel_offset=8, out_scale=1.0),
        "tile does not fit LDS": dict(x=torch.zeros((1, 16, 16, 64), dtype=BF, device=dev), k=(5, 5), pad=(2, 2, 2, 2),
                                      w=K.dconv_bf16_weight_bytes(torch.zeros(64, 5, 5, 64), 64).to(dev), Cout=64, bn=64),
        "fp8 without chan_scale": dict(x=x8, w=arr8),
        "out of the wrong shape": dict(out=out(32, hw=(16, 15))),
        "out too narrow for the slot": dict(out=out(40), out_channel_offset=16),
        "activation": dict(act="sigmoid"),
        "waves": dict(waves=2),
    }
    for name, kw in refused.items():
        with pytest.raises(ValueError):
            call(**kw)
            pytest.fail(f"{name}: not refused")
    typed = {
        "bias bf16": dict(bias=b.to(BF)),
        "weights not bytes": dict(w=arr.float()),
        "out float32": dict(out=out(32, F32)),
        "out bytes without out_scale": dict(out=out(32, U8)),
        "chan_scale bf16": dict(x=x8, w=arr8, chan_scale=cs.to(BF)),
    }
    for name, kw in typed.items():
        with pytest.raises(TypeError):
            call(**kw)
            pytest.fail(f"{name}: not refused")
    xu = torch.zeros((1, 32, 32, 3), dtype=U8, device=dev)
    aru = K.dconv_bf16_weight_bytes(torch.zeros(32, 4, 4, 16), 32).to(dev)
    for name, kw in {"bn 48": dict(bn=48), "row width % 8": dict(out=out(36)), "wrong shape": dict(out=out(32, hw=(16, 15))),
                     "weight pitch": dict(w=arr)}.items():
        with pytest.raises(ValueError):
            K.conv2d_direct_u8s2d(xu, kw.get("w", aru), (4, 4), 32, b, (1, 2, 1, 2), "relu", U8_MEAN, U8_STD,
                                  out=kw.get("out"), bn=kw.get("bn", 32))
            pytest.fail(f"u8 stem {name}: not refused")
    # and the launcher still takes the arguments the refusals were derived from
    y = call()
    assert tuple(y.shape) == (1, 16, 16, 32) and (y == 0).all()
