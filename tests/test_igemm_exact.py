"""The implicit-GEMM conv / GEMM kernel of ``kernels/igemm_bf16.hip``, bit for bit: all five tile
configs, the divide-free (tap, channel) K walk, dilation, unequal strides, the 64-tap mask, both
residual paths, the fused dual kernel and the host-side argument checks.

The operands are integers that are exact in bf16 (the bias is fp32 half-integers), in ranges
chosen so that every product and every partial sum stays below 2^23: fp32 accumulation is then
exact in any order, and the only inexact steps are the kernel's ``f2bf`` roundings (round to
nearest even).  The float64 references round where the ``.hip`` file rounds:

without residual
    ``y = bf16(act(acc + bias))``.
with residual
    ``a = bf16(acc + bias)`` into the LDS tile, then ``y = bf16(act(float(a) + r))``: two
    roundings, the first before the residual add.  The host path of ``ops/kernels.py`` rounds
    once; ``round_once`` is one of the wrong variants below.
dual (``conv1x1_dual``)
    ``y = bf16(act(acc1 + acc2 + bias))``, one accumulator over ``[x | x2 strided]``.

Every operation is brought to one form: an im2col matrix ``X [M, K]`` (built from the definition,
a loop over the filter taps on a zero-padded float64 image with strided / dilated slices, K in
(kh, kw, ci) order as the kernel walks it), the weight matrix ``W [Cout, K]`` and the epilogue.

The GPU tests assert ``torch.equal`` on bf16 tensors.  That is a value comparison; it is a bit
comparison here because no -0 can occur: sums of integers that start from +0 give +0 under
round-to-nearest, ReLU is ``x > 0 ? x : 0``, ReLU6 is ``min(max(x, 0), 6)`` of a value that is
never -0, the data hold no -0 and ``0 * rcp(..)`` of GELU at +0 is +0.  A mismatch is reported with
pixel, channel, tile and K-tile count of the first few elements.

Every GPU case writes through ``out=`` into a buffer pre-filled with a sentinel (2^100, which no
result can equal): row stride ``ldy = Cout + 40``, a channel offset from (16, 0, 8, 24) in turn,
and one more image of guard rows after the last pixel.  Every element outside the written channel
window must still hold the sentinel and none inside may.  ``K.gemm`` has no row stride of its
own: the GEMM cases run once through it (guard rows only) and once through the raw entry with
``ldy > N`` and an offset pointer.  Every operand (x, w, bias, residual, x2) is a view between NaN
guard rows, so a read past either end of it that reaches an accumulator or the epilogue shows.

gelu / sigmoid / tanh use ``v_exp_f32`` and ``v_rcp_f32`` and cannot match float64 everywhere.
They are driven by a permutation matrix and a zero bias, so the pre-activation is exactly the
chosen input (multiples of 1/8 in [-8, 8]), and only inputs whose float64 activation lies farther
than a relative 2^-16 from a bf16 rounding boundary are kept.  Error budget of ``apply_act``
(``E = 2^-24``, one fp32 rounding; ``v_exp_f32`` and ``v_rcp_f32`` are 1 ulp = 2 E):

* exponent ``t``: sigmoid / tanh one rounded constant and one multiply, ``2 E``; gelu the two
  rounded constants (``c1`` is a rounded product of rounded factors), ``x * x``, the fma and the
  multiply, ``6 E`` (both fma terms have the same sign, so nothing cancels);
* ``e = exp2(t)``: ``ln 2 * |t| * err(t) + 2 E``;
* ``s = rcp(1 + e)``: ``e / (1 + e) * err(e) + E + 2 E``;
* sigmoid = ``s``; gelu = ``x * s`` adds ``E``; tanh = ``2 s - 1`` (the subtraction is exact by
  Sterbenz) has the absolute error ``2 s err(s)``, relative ``2 s err(s) / |tanh x|``.

With ``|t| <= 11.6`` (sigmoid) and ``<= 23.1`` (tanh) that is below 2^-18 for sigmoid and for tanh
at ``|x| >= 1/8`` (tanh(0) = 0 has no relative budget and is not a candidate); gelu reaches
``|t| = 71`` at x = -8, where the bound is 2^-16 itself, so a value is kept only if its distance
also exceeds twice its own budget (``_budget``): never a value the 2^-16 rule drops, and none
whose exactness the budget does not guarantee.

The non-GPU tests check the references alone: against ``torch.nn.functional.conv2d`` in float64,
against the ``K.*`` host paths where nothing rounds, that the data make every rounding, ReLU and
ReLU6 observable, that the exactness bound holds, and that each deliberately wrong variant
(``FAULTS``) differs on every case it applies to."""
import collections
import functools
import itertools
import math
import zlib

import pytest
import torch

from flink_tensorflow_amd.ops import kernels as K

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EXACT = 2 ** 23          # half-integers below this are exact in fp32
SENT = 2.0 ** 100        # output sentinel: exact in bf16, far above any result
GAP = 40                 # ldy - Cout
COFFS = (16, 0, 8, 24)   # channel offsets, in turn
CFGS = (0, 1, 2, 3, 4, -1)
TILES = {0: (128, 128), 1: (256, 64), 2: (128, 128), 3: (256, 64), 4: (64, 128)}  # cfg -> (BM, BN)
FAULTS = ("drop_tap", "edge_neighbour", "pad_swap", "dil_swap", "stride_swap", "chunk_next_tap", "k_tail",
          "stale_tile", "round_once", "res_ld", "dual_switch_64", "shortcut_stride1")


def _tile(cfg, Cout):
    return TILES[(3 if Cout <= 64 else 2) if cfg < 0 else cfg]   # auto_config


# ----------------------------------------------------------------------------------- cases
# kind: "conv" (launch<true>), "pw" (1x1 / stride 1 / no pad through conv2d_nhwc: launch<false>),
# "gemm" (K.gemm and the raw entry), "dual" (conv1x1_dual; Cin = K1, H x W = Ho x Wo).
# data: "std" x in [-8, 8], w in [-4, 4], bias = halves in [-600, 600], residual in [-256, 256]; without a
#       bias x in [-24, 24], w in [-8, 8], so that the sums alone pass 256 (where bf16 starts to round);
#       "low" x, w in [-1, 1], bias = halves in [-3, 9] (ReLU6 without residual);
#       "anti" std operands and a residual that cancels acc + bias down to [-3, 9] (ReLU6 with one).
_Case = collections.namedtuple("_Case", "name fam kind N H W Cin Cout KH KW stride pad dil act bias res data coff "
                                        "C2 s2")
_SEQ = itertools.count()


def _mk(fam, tag, N, H, W, Cin, Cout, KH=1, KW=1, stride=(1, 1), pad=(0, 0, 0, 0), dil=(1, 1), act=None, bias=True,
        res=False, data="std", kind=None, C2=0, s2=1):
    if kind is None:
        kind = "pw" if (KH, KW, stride, pad) == (1, 1, (1, 1), (0, 0, 0, 0)) else "conv"
    coff = COFFS[next(_SEQ) % 4]
    name = f"{fam}-{tag}-{act or 'none'}{'' if bias else '-nobias'}{'-res' if res else ''}-off{coff}"
    return _Case(name, fam, kind, N, H, W, Cin, Cout, KH, KW, stride, pad, dil, act, bias, res, data, coff, C2, s2)


def same_pads(size, k, s, d):
    """TF SAME padding (before, after): the extra pixel goes after."""
    total = max((-(-size // s) - 1) * s + (k - 1) * d + 1 - size, 0)
    return total // 2, total - total // 2


def _same(H, W, k, s, d):
    return same_pads(H, k, s[0], d[0]) + same_pads(W, k, s[1], d[1])


CIN_SWEEP = (8, 16, 24, 40, 48, 64, 72, 96, 160, 192)
_ACT2 = ("relu", None)
CASES_CIN = [_mk("cin", f"3x3-c{ci}", 2, 9, 11, ci, 72, 3, 3, pad=(1, 1, 1, 1), act=_ACT2[i % 2])
             for i, ci in enumerate(CIN_SWEEP)]
CASES_TILES = [_mk("tiles", "3x3-c16-m338-n136", 2, 13, 13, 16, 136, 3, 3, pad=(1, 1, 1, 1), act="relu")]
CASES_GEOM = [
    _mk("stem", "7x7s2", 1, 20, 20, 8, 64, 7, 7, stride=(2, 2), pad=(2, 3, 2, 3), act="relu"),
    _mk("taps64", "8x8-on-6x6", 1, 6, 6, 8, 8, 8, 8, pad=(3, 4, 3, 4)),
    _mk("asym", "1x7", 1, 9, 10, 24, 40, 1, 7, pad=(0, 0, 3, 3), act="relu"),
    _mk("asym", "7x1", 1, 9, 10, 24, 40, 7, 1, pad=(3, 3, 0, 0)),
]
CASES_GEOM += [_mk("dil", f"3x3-d{d[0]}{d[1]}-{H}x{W}", 1, H, W, 16, 40, 3, 3, pad=_same(H, W, 3, (1, 1), d), dil=d,
                   act=_ACT2[i % 2]) for H, W in ((7, 9), (2, 3)) for i, d in enumerate(((2, 2), (1, 3), (3, 1)))]
CASES_GEOM += [
    _mk("stride", "3x3-s21", 1, 10, 9, 16, 40, 3, 3, stride=(2, 1), pad=_same(10, 9, 3, (2, 1), (1, 1)), act="relu"),
    _mk("stride", "3x3-s12", 1, 9, 10, 16, 40, 3, 3, stride=(1, 2), pad=_same(9, 10, 3, (1, 2), (1, 1))),
    _mk("stride", "5x5-s21-c48", 1, 10, 9, 48, 40, 5, 5, stride=(2, 1), pad=_same(10, 9, 5, (2, 1), (1, 1))),
    _mk("stride", "1x1-s12", 1, 9, 10, 16, 40, stride=(1, 2), act="relu"),
    _mk("stride", "3x3-s2-valid", 1, 9, 9, 16, 40, 3, 3, stride=(2, 2)),     # Ho = 4: every row is read
    _mk("stride", "3x3-s2-valid-10", 1, 10, 10, 16, 40, 3, 3, stride=(2, 2)),  # rows 9 and columns 9 left over
    _mk("stride", "1x1-s2", 2, 9, 9, 24, 72, stride=(2, 2), act="relu"),     # stays in conv mode
]
# residual in conv mode: K = 72 (RES_PF) and K = 216, x three activations, with and without bias
CASES_CRES = [_mk("convres", f"3x3-c{ci}-k{9 * ci}", 2, 9, 11, ci, 72, 3, 3, pad=(1, 1, 1, 1), act=a, bias=b, res=True,
                  data="anti" if a == "relu6" else "std")
              for ci in (8, 24) for a in (None, "relu", "relu6") for b in (True, False)]
CASES_RELU6 = [_mk("relu6", "3x3-c8", 2, 9, 11, 8, 72, 3, 3, pad=(1, 1, 1, 1), act="relu6", data="low"),
               _mk("relu6", "3x3-c24-nobias", 2, 9, 11, 24, 72, 3, 3, pad=(1, 1, 1, 1), act="relu6", data="low"),
               _mk("relu6", "gemm-129x72x72", 1, 1, 129, 72, 72, act="relu6", data="low", kind="gemm")]
CASES_CONV = CASES_CIN + CASES_TILES + CASES_GEOM + CASES_CRES + CASES_RELU6[:2]

# GEMM mode.  M in {1, 5, 129, 338}, N in {8, 72, 200}, K in {8, 64, 72, 136, 200}
GEMM_SHAPES = ((1, 200, 8), (5, 72, 64), (129, 8, 72), (338, 200, 136), (338, 72, 200), (129, 200, 64),
               (5, 200, 200), (1, 200, 136), (338, 8, 8), (129, 72, 72))
CASES_GEMM = [_mk("gemm", f"{M}x{N}x{Kd}", 1, 1, M, Kd, N, act=_ACT2[i % 2], kind="gemm")
              for i, (M, N, Kd) in enumerate(GEMM_SHAPES)]
# nwg = 18 (128x128), 20 (256x64), 36 (64x128): none a multiple of 8
CASES_GEMM += [_mk("remap", "1100x200x72", 1, 1, 1100, 72, 200, act="relu", kind="gemm")]
CASES_GRES = [_mk("gemmres", f"{M}x{N}x{Kd}", 1, 1, M, Kd, N, act=a, res=True, kind="gemm")
              for (M, N, Kd), a in (((129, 72, 72), "relu"), ((338, 200, 128), None), ((338, 200, 136), "relu"),
                                    ((129, 200, 200), None))]
# the same through conv2d_nhwc 1x1 / stride 1: stride-write with an offset, ldr = Cout != ldy
CASES_PW = [_mk("pwres", f"1x1-c{ci}", 2, 13, 13, ci, 136, act=a, bias=b, res=True)
            for ci, a, b in ((72, "relu", True), (128, None, True), (136, "relu", False), (200, "relu", True))]
CASES_PW += [_mk("pw", f"1x1-c{ci}", 2, 9, 11, ci, 72, act=a) for ci, a in ((40, "relu"), (160, None))]
CASES_GEMM_ALL = CASES_GEMM + CASES_GRES + CASES_PW + CASES_RELU6[2:]

# dual: A = (K1 72, C2 40): the switch to x2 lands inside K tile 1 and K = 112 leaves a tail;
#       B = (K1 64, C2 136): the switch on a tile edge, K = 200.  H2 = 2 Ho - 1 at stride 2.
CASES_DUAL = [_mk("dual", f"{ab}-k{K1}+{C2}-s{s2}-m{2 * hw * hw}-n{Cout}", 2, hw, hw, K1, Cout, act=_ACT2[i % 2],
                  kind="dual", C2=C2, s2=s2)
              for i, (ab, K1, C2, s2, hw, Cout) in enumerate(
                  (ab, K1, C2, s2, hw, Cout) for ab, K1, C2 in (("A", 72, 40), ("B", 64, 136))
                  for s2 in (1, 2) for hw, Cout in ((7, 72), (13, 136)))]
ALL_CASES = CASES_CONV + CASES_GEMM_ALL + CASES_DUAL


def _ids(cases):
    return [c.name for c in cases]


def _geom(c):
    """(Ho, Wo, M, K) from the definition."""
    if c.kind == "dual":
        return c.H, c.W, c.N * c.H * c.W, c.Cin + c.C2
    (sh, sw), (pt, pb, pl, pr), (dh, dw) = c.stride, c.pad, c.dil
    Ho = (c.H + pt + pb - ((c.KH - 1) * dh + 1)) // sh + 1
    Wo = (c.W + pl + pr - ((c.KW - 1) * dw + 1)) // sw + 1
    return Ho, Wo, c.N * Ho * Wo, c.KH * c.KW * c.Cin


# ------------------------------------------------------------------------------------ data
def _bf(v):
    """bf16 round-to-nearest-even of float64 half-integers below 2^23 (float64 -> fp32 is exact)."""
    return v.to(BF).to(F64)


def _act(v, act):
    if act == "relu":
        return torch.relu(v)
    if act == "relu6":
        return torch.clamp(v, 0, 6)
    return v


@functools.lru_cache(maxsize=None)
def _data(c):
    """The case's operands as float64 (all exact in bf16 / fp32, no -0): x NHWC, w OHWI, bias or
    None, res [M, Cout] or None, x2 NHWC (dual)."""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    Ho, Wo, M, Kd = _geom(c)

    def ints(lo, hi, shape):
        return torch.randint(lo, hi + 1, shape, generator=g).to(F64)

    rx, rw = (1, 1) if c.data == "low" else (8, 4) if c.bias else (24, 8)
    x = ints(-rx, rx, (c.N, c.H, c.W, c.Cin))
    w = ints(-rw, rw, (c.Cout, c.KH, c.KW, Kd // (c.KH * c.KW)))
    x2 = None
    if c.kind == "dual":
        h2 = c.H if c.s2 == 1 else 2 * c.H - 1
        x2 = ints(-rx, rx, (c.N, h2, h2, c.C2))
    bias = None
    if c.bias:
        bias = ints(-6, 18, (c.Cout,)) / 2 if c.data == "low" else ints(-1200, 1200, (c.Cout,)) / 2
    res = None
    if c.res and c.data == "anti":  # bf16(acc + bias) + res lands in [-3, 9]: both clamps and the inside
        v0 = _im2col(c, x, x2) @ w.reshape(c.Cout, Kd).t() + (0 if bias is None else bias)
        res = _bf(3 - v0 + ints(-6, 6, (M, c.Cout))) + 0.0
    elif c.res:
        res = ints(-256, 256, (M, c.Cout))
    return dict(x=x, w=w, bias=bias, res=res, x2=x2)


# -------------------------------------------------------------------------------- reference
def _edge_tap(c, Ho, Wo):
    """``edge_neighbour``: the padded column next to the image (left if there is left padding, else
    right) and the first tap (kh, kw) that reads it at an in-image row, or None."""
    (sh, sw), (pt, pb, pl, pr), (dh, dw) = c.stride, c.pad, c.dil
    if pl == 0 and pr == 0:
        return None
    col = pl - 1 if pl else pl + c.W
    for kw in range(c.KW):
        if any(wo * sw + kw * dw == col for wo in range(Wo)):
            for kh in range(c.KH):
                if any(pt <= ho * sh + kh * dh < pt + c.H for ho in range(Ho)):
                    return col, kh, kw
    return None


def _im2col(c, x, x2, fault=None):
    """``X [M, K]``: row m = output pixel (n, ho, wo), column k = (kh, kw, ci) — the zero-padded
    image sliced per filter tap; gemm: x itself; dual: ``[x | x2 at (ho s2, wo s2)]``."""
    Ho, Wo, M, Kd = _geom(c)
    if c.kind == "dual":
        s = 1 if fault == "shortcut_stride1" else c.s2
        return torch.cat([x.reshape(M, c.Cin), x2[:, ::s, ::s][:, :Ho, :Wo].reshape(M, c.C2)], 1)
    (sh, sw), (pt, pb, pl, pr), (dh, dw) = c.stride, c.pad, c.dil
    edge = _edge_tap(c, Ho, Wo) if fault == "edge_neighbour" else None
    if fault == "pad_swap":
        pt, pb, pl, pr = pb, pt, pr, pl
    if fault == "dil_swap":
        dh, dw = dw, dh
    if fault == "stride_swap":
        sh, sw = sw, sh
    # the canvas: the padded image, extended with zeros (what an out-of-image tap reads) as far as
    # the last tap of the last output pixel reaches
    Hp = max(pt + c.H + pb, (c.KH - 1) * dh + (Ho - 1) * sh + 1)
    Wp = max(pl + c.W + pr, (c.KW - 1) * dw + (Wo - 1) * sw + 1)
    xp = torch.zeros(c.N, Hp, Wp, c.Cin, dtype=F64)
    xp[:, pt:pt + c.H, pl:pl + c.W] = x
    cols = []
    for kh in range(c.KH):
        for kw in range(c.KW):
            src = xp
            if edge is not None and (kh, kw) == edge[1:]:   # this tap reads the neighbour, not the zero
                src = xp.clone()
                src[:, :, edge[0]] = xp[:, :, edge[0] + (1 if pl else -1)]
            t = src[:, kh * dh:kh * dh + (Ho - 1) * sh + 1:sh, kw * dw:kw * dw + (Wo - 1) * sw + 1:sw]
            if fault == "drop_tap" and (kh, kw) == (c.KH // 2, c.KW // 2):
                t = torch.zeros_like(t)
            cols.append(t.reshape(M, c.Cin))
    return torch.cat(cols, 1)


_Ref = collections.namedtuple("_Ref", "out exact peak shares")


def _reference(c, fault=None):
    """float64 mirror of the kernel -> ``_Ref``: ``out [M, Cout]`` holding the bf16 values,
    ``exact`` = ``act(acc + bias + res)`` unrounded (what the host paths compute), ``peak`` = an upper
    bound of every intermediate magnitude, ``shares`` = what each rounding / activation did."""
    d = _data(c)
    Ho, Wo, M, Kd = _geom(c)
    nk = -(-Kd // 64)
    X = _im2col(c, d["x"], d["x2"], fault)
    Wm = d["w"].reshape(c.Cout, Kd)
    if fault == "chunk_next_tap":   # 8 channels of one K tile read at the next tap (zeros past the last)
        k0, X = (64 if Kd > 64 else 0), X.clone()
        X[:, k0:k0 + 8] = X[:, k0 + c.Cin:k0 + c.Cin + 8] if k0 + c.Cin + 8 <= Kd else 0
    if fault == "k_tail":
        X = X.clone()
        X[:, Kd // 64 * 64:] = 0
    if fault == "dual_switch_64":   # k in [K1, 64-aligned K1) still read from x: the next pixel's row
        flat, K1 = d["x"].reshape(-1), c.Cin
        k = torch.arange(K1, min(-(-K1 // 64) * 64, Kd))
        X = X.clone()
        X[:, k] = flat[(torch.arange(M)[:, None] * K1 + k[None, :]) % flat.numel()]
    bias = torch.zeros(c.Cout, dtype=F64) if d["bias"] is None else d["bias"]
    acc = X @ Wm.t()
    if fault == "stale_tile":       # K tile 1 computed from the buffer that still holds K tile 0
        acc = acc - X[:, 64:128] @ Wm[:, 64:128].t() + X[:, :64] @ Wm[:, :64].t()
    v = acc + bias
    peak = float((X.abs() @ Wm.abs().t() + bias.abs()).max())
    sh = {}
    if d["res"] is None:
        exact = _act(v, c.act)
        out = _bf(exact)
        sh["round"] = (out != exact).double().mean().item()
    else:
        r = d["res"]
        if fault == "res_ld":       # residual rows taken ldy apart
            flat = r.reshape(-1)
            idx = torch.arange(M)[:, None] * (c.Cout + GAP) + torch.arange(c.Cout)[None, :]
            r = flat[idx % flat.numel()]
        peak = max(peak * (1 + 2.0 ** -8) + float(r.abs().max()), peak)
        exact = _act(v + r, c.act)
        a = _bf(v)
        pre = _act(a + r, c.act)
        out = _bf(exact) if fault == "round_once" else _bf(pre)
        sh["round_a"] = (a != v).double().mean().item()
        sh["round"] = (_bf(pre) != pre).double().mean().item()
        sh["double"] = (_bf(pre) != _bf(exact)).double().mean().item()
    if c.act == "relu":
        sh["zeros"] = (out == 0).double().mean().item()
    if c.act == "relu6":
        pre6 = v if d["res"] is None else a + r
        sh["lo"] = (pre6 <= 0).double().mean().item()
        sh["hi"] = (pre6 >= 6).double().mean().item()
        sh["in"] = ((pre6 > 0) & (pre6 < 6)).double().mean().item()
    return _Ref(out, exact, peak, sh)


@functools.lru_cache(maxsize=None)
def _ref(c):
    r = _reference(c)
    assert r.peak < EXACT, f"{c.name}: intermediate magnitude {r.peak} is not exact in fp32"
    return r


def _applies(fault, c):
    Ho, Wo, M, Kd = _geom(c)
    conv = c.kind == "conv"
    return {"drop_tap": conv,
            "edge_neighbour": conv and _edge_tap(c, Ho, Wo) is not None,
            "pad_swap": conv and (c.pad[0] != c.pad[1] or c.pad[2] != c.pad[3]),
            "dil_swap": conv and c.dil[0] != c.dil[1],
            "stride_swap": conv and c.stride[0] != c.stride[1],
            "chunk_next_tap": conv and c.KH * c.KW > 1,
            "k_tail": Kd % 64 != 0 and bool(_im2col(c, _data(c)["x"], _data(c)["x2"])[:, Kd // 64 * 64:].any()),
            "stale_tile": Kd > 64,
            "round_once": c.res,
            "res_ld": c.res,
            "dual_switch_64": c.kind == "dual" and c.Cin % 64 != 0,
            "shortcut_stride1": c.kind == "dual" and c.s2 == 2}[fault]


# ----------------------------------------------------------- transcendental activations
TRANS = ("gelu", "sigmoid", "tanh")
_LOG2E = 1.4426950408889634
_K0 = 0.7978845608028654


def _act64(x, act):
    if act == "sigmoid":
        return 1 / (1 + torch.exp(-x))
    if act == "tanh":
        return torch.tanh(x)
    # 0.5 x (1 + tanh u) = x / (1 + exp(-2 u)); the first form cancels for u << 0 (in float64 it is
    # off by 2^-7 at x = -7 and 0 from x = -7.25 down, where the value x exp(2 u) is a normal bf16 number)
    return x / (1 + torch.exp(-2 * _K0 * (x + 0.044715 * x ** 3)))


def _budget(x, act):
    """Relative error bound of ``apply_act`` in fp32 (module docstring), per input value."""
    E = 2.0 ** -24
    if act == "gelu":
        t, et = -2 * _K0 * _LOG2E * x * (1 + 0.044715 * x * x), 6 * E
    else:
        t, et = -(2 if act == "tanh" else 1) * _LOG2E * x, 2 * E
    e = torch.exp2(t)
    frac = torch.where(torch.isinf(e), torch.ones_like(e), e / (1 + e))
    s_err = frac * (math.log(2) * t.abs() * et + 2 * E) + 3 * E
    if act == "sigmoid":
        return s_err
    if act == "gelu":
        return s_err + E
    return 2 / (1 + e) * s_err / torch.tanh(x).abs()   # inf at x = 0


def _boundary_distance(f):
    """Relative distance of float64 ``f`` to the nearest bf16 rounding boundary (the midpoint of
    two neighbouring bf16 values); inf for 0."""
    a = f.abs()
    b = a.to(BF)
    bits = b.view(torch.int16)
    up, dn = (bits + 1).view(BF).to(F64), (bits - 1).view(BF).to(F64)
    b = b.to(F64)
    dist = torch.minimum((a - (b + up) / 2).abs(), (a - (b + dn) / 2).abs()) / a
    return torch.where(a == 0, torch.full_like(a, float("inf")), dist)


@functools.lru_cache(maxsize=None)
def _kept(act):
    """The multiples of 1/8 in [-8, 8] on which ``bf16(apply_act(x))`` must equal ``bf16(act64(x))``."""
    x = torch.arange(-64, 65, dtype=F64) / 8
    if act == "tanh":
        x = x[x != 0]
    dist = _boundary_distance(_act64(x, act))
    return x[(dist > 2.0 ** -16) & (dist > 2 * _budget(x, act))]


# ---------------------------------------------------------------------------- running a case
def _t(v, dtype, dev):
    """``v`` on ``dev`` as a contiguous view between NaN guard rows (one leading-dim row before and
    after, 8 elements for a vector: the view stays 16-byte aligned)."""
    if v is None:
        return None
    g = 8 if v.dim() == 1 else 1
    big = torch.full((v.shape[0] + 2 * g, *v.shape[1:]), float("nan"), dtype=dtype)
    big[g:-g] = v.to(dtype)
    return big.to(dev)[g:-g]


def _launch(c, cfg, dev, raw=False):
    """One launch into a fresh sentinel buffer -> (whole buffer on the host as [rows, ldy], window
    rows M, window start).  ``raw``: gemm through the library entry with ldy > N and an offset pointer."""
    d = _data(c)
    Ho, Wo, M, Kd = _geom(c)
    x, w, x2, res = (_t(d[k], BF, dev) for k in ("x", "w", "x2", "res"))
    bias = _t(d["bias"], F32, dev)
    if c.kind == "gemm":
        ldy, coff = (c.Cout + GAP, c.coff) if raw else (c.Cout, 0)
        big = torch.full((2 * M, ldy), SENT, dtype=BF, device=dev)
        x, w = x.reshape(M, Kd), w.reshape(c.Cout, Kd)
        if raw:
            zb = bias if bias is not None else torch.zeros(c.Cout, device=dev)
            K._hip().gemm_bf16(x.data_ptr(), w.data_ptr(), zb.data_ptr(), K._ptr(res), big.data_ptr() + 2 * coff, M,
                               c.Cout, Kd, Kd, ldy, c.Cout, K.act_code(c.act), K._stream(), cfg)
        else:
            K.gemm(x, w, bias, res, act=c.act, out=big[:M], cfg=cfg)
    else:
        ldy, coff = c.Cout + GAP, c.coff
        big = torch.full((c.N + 1, Ho, Wo, ldy), SENT, dtype=BF, device=dev)
        if c.kind == "dual":
            K.conv1x1_dual(x, x2, w.reshape(c.Cout, Kd), bias, stride2=c.s2, act=c.act, out=big[:c.N],
                           out_channel_offset=coff, cfg=cfg)
        else:
            K.conv2d_nhwc(x, w, bias, None if res is None else res.reshape(c.N, Ho, Wo, c.Cout), stride=c.stride,
                          pad=c.pad, dilation=c.dil, act=c.act, out=big[:c.N], out_channel_offset=coff, cfg=cfg)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return big.cpu().reshape(-1, ldy), M, coff


def _assert_case(got, want, c, cfg, what):
    """``torch.equal`` with a report of the first mismatches: pixel, channel, tile, K tiles."""
    if torch.equal(got, want):
        return
    Ho, Wo, M, Kd = _geom(c)
    BM, BN = _tile(cfg, c.Cout)
    bad = (got != want).nonzero()
    lines = []
    for m, ch in bad[:8].tolist():
        lines.append(f"  pixel m = {m} (n, ho, wo) = ({m // (Ho * Wo)}, {m // Wo % Ho}, {m % Wo})  channel {ch}  "
                     f"tile ({m // BM}, {ch // BN}) of {-(-M // BM)} x {-(-c.Cout // BN)} ({BM}x{BN})  "
                     f"K tiles {-(-Kd // 64)} (K = {Kd}): got {got[m, ch].item()!r}, want {want[m, ch].item()!r}")
    pytest.fail(f"{what}: {len(bad)} of {got.numel()} elements differ\n" + "\n".join(lines))


def _check_window(buf, M, coff, want, c, cfg, what):
    """``buf [rows, ldy]``: rows < M, channels [coff, coff + Cout) hold ``want`` and no sentinel;
    everything else still holds the sentinel."""
    Cout = want.shape[1]
    win = buf[:M, coff:coff + Cout]
    _assert_case(win, want, c, cfg, what)
    assert not bool((win == SENT).any()), f"{what}: sentinel left inside the output"
    rest = buf.clone()
    rest[:M, coff:coff + Cout] = SENT
    if not bool((rest == SENT).all()):
        r, ch = (rest != SENT).nonzero()[0].tolist()
        pytest.fail(f"{what}: written outside the output window at row {r} (M = {M}), channel {ch} "
                    f"(window [{coff}, {coff + Cout}))")


def _gpu_case(c, cfg):
    dev = torch.device("cuda", 0)
    want = _ref(c).out.to(BF)
    BM, BN = _tile(cfg, c.Cout)
    M, Kd = _geom(c)[2:]
    what = f"{c.name} cfg {cfg} ({BM}x{BN}, {-(-M // BM) * -(-c.Cout // BN)} workgroups, {-(-Kd // 64)} K tiles)"
    buf, M, coff = _launch(c, cfg, dev)
    _check_window(buf, M, coff, want, c, cfg, what)
    if c.kind == "gemm":
        buf, M, coff = _launch(c, cfg, dev, raw=True)
        _check_window(buf, M, coff, want, c, cfg, what + " raw entry, ldy > N")


# --------------------------------------------------------------------------------- CPU tests
CPU = torch.device("cpu")


def _torch_conv(c, d):
    pt, pb, pl, pr = c.pad
    xn = torch.nn.functional.pad(d["x"].permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = torch.nn.functional.conv2d(xn, d["w"].permute(0, 3, 1, 2), stride=c.stride, dilation=c.dil)
    return y.permute(0, 2, 3, 1).reshape(-1, c.Cout)


@pytest.mark.parametrize("c", CASES_CONV + CASES_PW, ids=_ids(CASES_CONV + CASES_PW))
def test_conv_reference_equals_torch_conv2d_float64(c):
    d = _data(c)
    Ho, Wo, M, Kd = _geom(c)
    acc = _im2col(c, d["x"], None) @ d["w"].reshape(c.Cout, Kd).t()
    ref = _torch_conv(c, d)
    assert ref.shape == (M, c.Cout) and torch.equal(acc, ref)


@pytest.mark.parametrize("c", ALL_CASES, ids=_ids(ALL_CASES))
def test_reference_equals_host_path_where_it_does_not_round(c):
    """The ``K.*`` host paths compute in fp32 (exact here) and, into an fp32 ``out``, round nowhere."""
    d = _data(c)
    Ho, Wo, M, Kd = _geom(c)
    f = lambda k: None if d[k] is None else d[k].to(F32)
    if c.kind == "gemm":
        got = K.gemm(f("x").reshape(M, Kd), f("w").reshape(c.Cout, Kd), f("bias"), f("res"), act=c.act)
    elif c.kind == "dual":
        got = K.conv1x1_dual(f("x"), f("x2"), f("w").reshape(c.Cout, Kd), f("bias"), stride2=c.s2, act=c.act)
    else:
        res = None if d["res"] is None else f("res").reshape(c.N, Ho, Wo, c.Cout)
        got = K.conv2d_nhwc(f("x"), f("w"), f("bias"), res, stride=c.stride, pad=c.pad, dilation=c.dil, act=c.act)
    assert got.dtype == F32 and tuple(got.shape[:-1]) in ((c.N, Ho, Wo), (M,))
    assert torch.equal(got.reshape(M, c.Cout).to(F64), _ref(c).exact)


def test_host_path_into_a_strided_bf16_out_rounds_once():
    """The host paths write ``out=`` windows like the kernel does, but round once: with a residual
    they equal the ``round_once`` variant, not the reference."""
    for c in (CASES_CRES[1], CASES_PW[0], CASES_DUAL[0]):
        buf, M, coff = _launch(c, -1, CPU)
        want = (_reference(c, "round_once") if c.res else _ref(c)).out.to(BF)
        _check_window(buf, M, coff, want, c, -1, c.name)


@pytest.mark.parametrize("c", ALL_CASES, ids=_ids(ALL_CASES))
def test_data_make_the_properties_observable(c):
    """Conditions on the data (not measurements): the bound; >= 5 % of the values changed by each
    rounding that sees unclamped values (ReLU6 outputs are half-integers in [0, 6], exact in bf16);
    ReLU zeroes 10 - 90 %; ReLU6 leaves >= 5 % at each clamp and strictly inside; the double
    rounding differs from the single one in >= 1 %."""
    r = _ref(c)
    s = r.shares
    print(f"{c.name}: peak {r.peak:.0f} " + " ".join(f"{k} {v:.3f}" for k, v in s.items()))
    assert r.peak < EXACT
    assert torch.equal(r.out.to(BF).to(F64), r.out) and torch.equal(r.exact.to(F32).to(F64), r.exact)
    for k in ("x", "w", "res", "x2"):
        d = _data(c)[k]
        assert d is None or (torch.equal(d.to(BF).to(F64), d) and not bool((d.signbit() & (d == 0)).any())), k
    if c.act != "relu6":
        assert s["round"] >= 0.05, "the output rounding changes too few values"
    if c.res:
        assert s["round_a"] >= 0.05, "the rounding before the residual add changes too few values"
        assert s["double"] >= 0.01, "double and single rounding agree too often"
    if c.act == "relu":
        assert 0.10 <= s["zeros"] <= 0.90
    if c.act == "relu6":
        assert min(s["lo"], s["hi"], s["in"]) >= 0.05


@pytest.mark.parametrize("fault", FAULTS)
def test_wrong_variants_differ(fault):
    """Each wrong variant of the reference changes the bf16 output of every case it applies to,
    and applies to at least three cases."""
    hit = 0
    for c in ALL_CASES:
        if _applies(fault, c):   # k_tail: not where the tail's taps all lie outside the image
            assert not torch.equal(_reference(c, fault).out.to(BF), _ref(c).out.to(BF)), \
                f"{fault} goes unnoticed on {c.name}"
            hit += 1
    assert hit >= 3, f"{fault} applies to {hit} cases"


def test_case_table_covers_every_axis():
    geo = {c.name: _geom(c) for c in ALL_CASES}
    conv = [c for c in ALL_CASES if c.kind == "conv"]
    assert {c.Cin for c in CASES_CIN} == set(CIN_SWEEP)
    assert {geo[c.name][3] % 64 != 0 for c in CASES_CIN} == {True, False}          # K tails and none
    assert {-(-geo[c.name][3] // 64) % 2 for c in CASES_CIN} == {0, 1}            # nk odd and even
    assert any(c.KH * c.KW == 64 and c.H < c.KH for c in conv) and any(c.KH * c.KW == 49 for c in conv)
    assert any((c.KH, c.KW) == (7, 1) for c in conv) and any((c.KH, c.KW) == (1, 7) for c in conv)
    assert {c.dil for c in conv} >= {(2, 2), (1, 3), (3, 1)} and {c.stride for c in conv} >= {(2, 1), (1, 2), (2, 2)}
    for kind in ("conv", "pw", "gemm"):                                           # RES_PF and the plain residual
        ks = {geo[c.name][3] <= 128 for c in ALL_CASES if c.kind == kind and c.res}
        assert ks == {True, False}, kind
    assert {(c.act, c.bias) for c in CASES_CRES} == {(a, b) for a in (None, "relu", "relu6") for b in (True, False)}
    assert {c.Cin % 64 for c in CASES_DUAL} == {8, 0} and {c.s2 for c in CASES_DUAL} == {1, 2}
    assert sum(c.coff != 0 for c in ALL_CASES) * 2 >= len(ALL_CASES)
    assert {s[0] for s in GEMM_SHAPES} == {1, 5, 129, 338} and {s[1] for s in GEMM_SHAPES} == {8, 72, 200}
    assert {s[2] for s in GEMM_SHAPES} == {8, 64, 72, 136, 200}
    remap = CASES_GEMM[-1]
    for cfg in range(5):   # a grid that xcd_remap permutes with a remainder
        BM, BN = TILES[cfg]
        nwg = -(-geo[remap.name][2] // BM) * -(-remap.Cout // BN)
        assert nwg > 8 and nwg % 8 != 0, (cfg, nwg)
    BM, BN = TILES[4]
    assert -(-geo[CASES_TILES[0].name][2] // BM) * -(-CASES_TILES[0].Cout // BN) == 12


@pytest.mark.parametrize("act", TRANS)
def test_transcendental_inputs_kept(act):
    x = _kept(act)
    print(f"{act}: {len(x)} of 129 inputs kept, {int((x < 0).sum())} negative, {int((x > 0).sum())} positive")
    assert len(x) >= 24 and int((x < 0).sum()) >= 8 and int((x > 0).sum()) >= 8
    f = _act64(x, act)
    assert bool((_boundary_distance(f) > 2 * _budget(x, act)).all())
    assert torch.equal(x.to(BF).to(F64), x)
    if act == "gelu":   # the stable form is the tanh formula (compared where that one does not cancel)
        near = x[x >= -3]
        tf = torch.nn.functional.gelu(near, approximate="tanh")
        assert bool(((_act64(near, act) - tf).abs() <= 1e-12 * tf.abs()).all()) and bool((f[x < 0] < 0).all())
    if act != "gelu":   # the budget stays below 2^-18: the 2^-16 rule alone decides
        assert float(_budget(x, act).max()) < 2.0 ** -18


def test_boundary_distance():
    one = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 - 2.0 ** -9, 0.0], dtype=F64)
    d = _boundary_distance(one)
    assert d[0] == 2.0 ** -9 and d[1] == 0 and abs(d[2] * one[2] - 2.0 ** -20) < 1e-15 and d[3] == 0
    assert math.isinf(d[4])


# --------------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("c", CASES_CONV, ids=_ids(CASES_CONV))
def test_conv_mode_gpu(c, cfg):
    _gpu_case(c, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("c", CASES_GEMM_ALL, ids=_ids(CASES_GEMM_ALL))
def test_gemm_mode_gpu(c, cfg):
    _gpu_case(c, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("c", CASES_DUAL, ids=_ids(CASES_DUAL))
def test_dual_gpu(c, cfg):
    _gpu_case(c, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("act", TRANS)
def test_transcendental_activations_gpu(act, cfg):
    """K = N = 72 (a K tail), M = 5: ``y[m, n] = act(x[m, perm[n]])`` exactly on the kept inputs."""
    dev = torch.device("cuda", 0)
    vals = _kept(act)
    g = torch.Generator().manual_seed(7)
    M, N = 5, 72
    x = vals[torch.arange(M * N) % len(vals)][torch.randperm(M * N, generator=g)].reshape(M, N)
    perm = torch.randperm(N, generator=g)
    w = torch.zeros(N, N, dtype=F64)
    w[torch.arange(N), perm] = 1
    big = torch.full((2 * M, N), SENT, dtype=BF, device=dev)
    K.gemm(x.to(BF).to(dev), w.to(BF).to(dev), None, None, act=act, out=big[:M], cfg=cfg)
    torch.cuda.synchronize()
    got, pre = big.cpu(), x[:, perm]
    want = _act64(pre, act).to(BF)
    assert bool((got[M:] == SENT).all())
    if not torch.equal(got[:M], want):
        bad = (got[:M] != want).nonzero()
        lines = []
        for m, n in bad[:8].tolist():
            f, y = _act64(pre[m, n], act).item(), got[m, n].item()
            lines.append(f"  x = {pre[m, n].item()}: got {y!r}, want {want[m, n].item()!r}, float64 {f!r}, "
                         f"relative error of the stored value {abs(y - f) / max(abs(f), 1e-300):.3e}")
        pytest.fail(f"{act} cfg {cfg}: {len(bad)} of {M * N} differ\n" + "\n".join(lines))


# ----------------------------------------------------------------- host-side argument checks
_CONV_ARGS = ("x", "w", "bias", "res", "y", "N", "H", "W", "Cin", "Cout", "KH", "KW", "sh", "sw", "ph", "pw", "dh",
              "dw", "Ho", "Wo", "ldy", "y_coff", "ldr", "act", "stream", "cfg")
_GEMM_ARGS = ("x", "w", "bias", "res", "y", "M", "N", "K", "ldx", "ldy", "ldr", "act", "stream", "cfg")
_DUAL_ARGS = ("x", "x2", "w", "bias", "y", "N", "Ho", "Wo", "K1", "C2", "H2", "W2", "s2", "Cout", "ldy", "y_coff",
              "act", "stream", "cfg")
# what each entry rejects: entry, the arguments changed from a valid small problem.  "+2" = that
# pointer moved by 2 bytes; "res" = a residual pointer is passed.
BAD_ARGS = {
    "conv-Cin%8": ("conv", dict(Cin=12)),
    "conv-Cout%8": ("conv", dict(Cout=12)),
    "conv-ldy%8": ("conv", dict(ldy=20)),
    "conv-y_coff%8": ("conv", dict(y_coff=4)),
    "conv-residual-stride%8": ("conv", dict(res="res", ldr=12)),
    "conv-empty-N": ("conv", dict(N=0)),
    "conv-empty-Ho": ("conv", dict(Ho=0)),
    "conv-empty-Cout": ("conv", dict(Cout=0)),
    "conv-72-taps-9x8": ("conv", dict(KH=9, KW=8, ph=4, pw=4)),
    "conv-input-2^31-bytes": ("conv", dict(N=1 << 23)),                   # 2^23 * 4 * 4 * 8 * 2 bytes
    "conv-2^31-pixels": ("conv", dict(Ho=1 << 16, Wo=1 << 15)),
    "conv-weights-2^31-bytes": ("conv", dict(Cout=1 << 20, KH=8, KW=8, Cin=16)),
    "conv-cfg5": ("conv", dict(cfg=5)),
    "conv-cfg99": ("conv", dict(cfg=99)),
    "conv-gelu": ("conv", dict(act=K.ACT_GELU)),
    "conv-sigmoid": ("conv", dict(act=K.ACT_SIGMOID)),
    "conv-no-bias-pointer": ("conv", dict(bias=0)),
    "conv-x+2": ("conv", dict(x="+2")),
    "conv-w+2": ("conv", dict(w="+2")),
    "conv-y+2": ("conv", dict(y="+2")),
    "conv-bias+2": ("conv", dict(bias="+2")),
    "conv-res+2": ("conv", dict(res="res+2")),
    "pointwise-cfg5": ("conv", dict(KH=1, KW=1, ph=0, pw=0, cfg=5)),
    "pointwise-drelu": ("conv", dict(KH=1, KW=1, ph=0, pw=0, act=K.ACT_DRELU)),
    "gemm-K%8": ("gemm", dict(K=12)),
    "gemm-ldx%8": ("gemm", dict(ldx=20)),
    "gemm-N%8": ("gemm", dict(N=12)),
    "gemm-ldy%8": ("gemm", dict(ldy=20)),
    "gemm-residual-stride%8": ("gemm", dict(res="res", ldr=12)),
    "gemm-empty-M": ("gemm", dict(M=0)),
    "gemm-empty-N": ("gemm", dict(N=0)),
    "gemm-x-2^31-elements": ("gemm", dict(M=1 << 20, ldx=2048)),
    "gemm-weights-2^31-bytes": ("gemm", dict(N=1 << 20, K=1024, ldx=1024, ldy=1 << 20)),
    "gemm-cfg5": ("gemm", dict(cfg=5)),
    "gemm-cfg99": ("gemm", dict(cfg=99)),
    "gemm-drelu": ("gemm", dict(act=K.ACT_DRELU)),
    "gemm-no-bias-pointer": ("gemm", dict(bias=0)),
    "gemm-x+2": ("gemm", dict(x="+2")),
    "gemm-w+2": ("gemm", dict(w="+2")),
    "gemm-y+2": ("gemm", dict(y="+2")),
    "gemm-bias+2": ("gemm", dict(bias="+2")),
    "gemm-res+2": ("gemm", dict(res="res+2")),
    "dual-K1%8": ("dual", dict(K1=12)),
    "dual-C2%8": ("dual", dict(C2=12)),
    "dual-Cout%8": ("dual", dict(Cout=12)),
    "dual-ldy%8": ("dual", dict(ldy=20)),
    "dual-y_coff%8": ("dual", dict(y_coff=4)),
    "dual-geometry-H": ("dual", dict(s2=2, H2=6)),     # (Ho - 1) s2 = 6 >= H2
    "dual-geometry-W": ("dual", dict(s2=2, W2=6)),
    "dual-x2-2^31-elements": ("dual", dict(N=1 << 20, H2=16, W2=16)),     # 2^20 * 16 * 16 * 8
    "dual-x-2^31-elements": ("dual", dict(N=1 << 11, K1=16, Ho=1 << 8, Wo=1 << 8, H2=1 << 8, W2=1 << 8)),
    "dual-weights-2^31-bytes": ("dual", dict(Cout=1 << 20, K1=512, C2=512)),
    "dual-relu6": ("dual", dict(act=K.ACT_RELU6)),
    "dual-gelu": ("dual", dict(act=K.ACT_GELU)),
    "dual-cfg5": ("dual", dict(cfg=5)),
    "dual-cfg99": ("dual", dict(cfg=99)),
    "dual-no-bias-pointer": ("dual", dict(bias=0)),
    "dual-x+2": ("dual", dict(x="+2")),
    "dual-x2+2": ("dual", dict(x2="+2")),
    "dual-w+2": ("dual", dict(w="+2")),
    "dual-y+2": ("dual", dict(y="+2")),
    "dual-bias+2": ("dual", dict(bias="+2")),
}


@functools.lru_cache(maxsize=None)
def _arg_env():
    """Buffers far larger than the 1 x 4 x 4 x 8 problems need (an accepted bad call would stay
    inside them), y filled with the sentinel."""
    dev = torch.device("cuda", 0)
    env = {k: torch.zeros(1 << 16, dtype=BF, device=dev) for k in ("x", "x2", "w", "res")}
    env["bias"] = torch.zeros(1 << 12, dtype=F32, device=dev)
    env["y"] = torch.full((1 << 16,), SENT, dtype=BF, device=dev)
    return env


def _raw_call(entry, changes):
    env = _arg_env()
    ptr = {k: t.data_ptr() for k, t in env.items()}
    if entry == "conv":     # 3x3 / pad 1 on 1 x 4 x 4 x 8 -> 8 channels
        a = dict(N=1, H=4, W=4, Cin=8, Cout=8, KH=3, KW=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, Ho=4, Wo=4, ldy=16,
                 y_coff=8, ldr=8)
        names, fn = _CONV_ARGS, K._hip().conv2d_nhwc_bf16
    elif entry == "gemm":
        a = dict(M=16, N=8, K=8, ldx=8, ldy=16, ldr=8)
        names, fn = _GEMM_ARGS, K._hip().gemm_bf16
    else:                   # 1 x 4 x 4 pixels, x2 1 x 7 x 7 at stride 1
        a = dict(N=1, Ho=4, Wo=4, K1=8, C2=8, H2=7, W2=7, s2=1, Cout=8, ldy=16, y_coff=8)
        names, fn = _DUAL_ARGS, K._hip().conv1x1_dual_bf16
    a.update(x=ptr["x"], x2=ptr["x2"], w=ptr["w"], bias=ptr["bias"], res=0, y=ptr["y"], act=K.ACT_RELU,
             stream=K._stream(), cfg=-1)
    for k, v in changes.items():
        if v == "+2":
            a[k] = ptr[k] + 2
        elif v == "res":
            a[k] = ptr["res"]
        elif v == "res+2":
            a[k], a["ldr"] = ptr["res"] + 2, 8
        else:
            a[k] = v
    fn(*[a[k] for k in names])


@pytest.mark.gpu
@pytest.mark.parametrize("what", list(BAD_ARGS))
def test_bad_arguments_are_rejected_before_any_launch_gpu(what):
    entry, changes = BAD_ARGS[what]
    reason = next(msg for key, msg in (("%8", "8"), ("empty", "empty problem"), ("2^31", "too large"),
                                       ("taps", "more than 64 filter taps"), ("cfg", "config"),
                                       ("no-bias", "bias pointer is required"), ("+2", "16-byte aligned"),
                                       ("geometry", "shortcut geometry"), ("", "activation|act must be"))
                  if key in what)
    with pytest.raises(ValueError, match=reason):
        _raw_call(entry, changes)
    torch.cuda.synchronize()
    assert bool((_arg_env()["y"] == SENT).all()), f"{what}: the output was written"


@pytest.mark.gpu
def test_valid_raw_calls_are_accepted_gpu():
    """The problems the rejected calls are derived from are themselves accepted."""
    y = _arg_env()["y"]
    for entry in ("conv", "gemm", "dual"):
        _raw_call(entry, {})
    torch.cuda.synchronize()
    got = y.cpu()
    y.fill_(SENT)
    assert bool((got[:16 * 16].reshape(16, 16)[:, 8:] == 0).all()) and bool((got[16 * 16:] == SENT).all())


@pytest.mark.gpu
def test_wrappers_reject_bad_arguments_gpu():
    """The same checks reached through ``K.*`` (a view's shape becomes Cin / ldy / the offset)."""
    dev = torch.device("cuda", 0)
    z = lambda *s: torch.zeros(*s, dtype=BF, device=dev)
    out = torch.full((1, 4, 4, 16), SENT, dtype=BF, device=dev)
    b8 = torch.zeros(8, device=dev)
    bad = [
        lambda: K.conv2d_nhwc(z(1, 4, 4, 12), z(8, 3, 3, 12), pad=(1, 1, 1, 1), out=out),
        lambda: K.conv2d_nhwc(z(1, 4, 4, 8), z(8, 3, 3, 8), pad=(1, 1, 1, 1), out=out, out_channel_offset=4),
        lambda: K.conv2d_nhwc(z(1, 4, 4, 8), z(8, 3, 3, 8), pad=(1, 1, 1, 1), out=out, out_channel_offset=16),
        lambda: K.conv2d_nhwc(z(1, 4, 4, 8), z(8, 9, 8, 8), pad=(4, 4, 4, 3), out=out),
        lambda: K.conv2d_nhwc(z(1, 4, 4, 8), z(8, 3, 3, 8), pad=(1, 1, 1, 1), out=out, act="gelu"),
        lambda: K.conv2d_nhwc(z(1, 4, 4, 8), z(8, 3, 3, 8), pad=(1, 1, 1, 1), out=out, cfg=5),
        lambda: K.conv2d_nhwc(z(1, 4, 4, 8), z(8, 3, 3, 8), pad=(1, 1, 1, 1), out=out, residual=z(1, 4, 4, 16)),
        lambda: K.gemm(z(16, 12), z(8, 12)),
        lambda: K.gemm(z(16, 8), z(8, 8), cfg=99),
        lambda: K.conv1x1_dual(z(1, 4, 4, 8), z(1, 7, 7, 8), z(8, 16), b8, act="relu6", out=out),
        lambda: K.conv1x1_dual(z(1, 4, 4, 8), z(1, 6, 6, 8), z(8, 16), b8, stride2=2, out=out),
        lambda: K.conv1x1_dual(z(1, 4, 4, 8), z(1, 7, 7, 8), z(8, 16), b8, out=out, out_channel_offset=16),
        lambda: K.conv1x1_dual(z(1, 4, 4, 8), z(1, 7, 7, 8), z(8, 16), b8, out=out[:, :3]),
        lambda: K.conv1x1_dual(z(1, 4, 4, 8), z(2, 7, 7, 8), z(8, 16), b8, out=out),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"accepted: bad call {i}")
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def test_dual_wrapper_checks_its_output_window_on_the_host_too():
    z = lambda *s: torch.zeros(*s)
    out = torch.full((1, 4, 4, 16), SENT)
    for kw in (dict(out=out, out_channel_offset=16), dict(out=out[:, :3]), dict(stride2=2, out=out)):
        with pytest.raises(ValueError):
            K.conv1x1_dual(z(1, 4, 4, 8), z(1, 6, 6, 8), z(8, 16), z(8), **kw)
    with pytest.raises(ValueError):
        K.conv1x1_dual(z(1, 4, 4, 8), z(2, 7, 7, 8), z(8, 16), z(8), out=out)
    assert bool((out == SENT).all())
