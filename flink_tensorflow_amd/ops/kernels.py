"""Python entry points of the hand-written CDNA4 kernels.

Every op has exactly two implementations:

* **HBM tensors (``cuda``)** → the gfx950 HIP kernel in ``_hip`` (``kernels/*.hip``).  If
  the library is missing on a GPU machine the call raises — there is no silent PyTorch
  fallback on the device path.
* **host tensors** → a plain PyTorch fp32 reference with identical semantics, used by the
  CPU test-suite and as the numerics oracle for the GPU tests.

Shapes, dtypes, alignment and contiguity are validated on the host before any launch
(a malformed launch can fault the whole GPU).  All launches go to the caller's current
stream, so the ops are hipGraph-capturable.
"""
from __future__ import annotations

import copy
import functools
import math
import os

import torch
import torch.nn.functional as F

from .. import _ext

ACT_NONE, ACT_RELU, ACT_GELU, ACT_SIGMOID, ACT_TANH, ACT_RELU6, ACT_DRELU = 0, 1, 2, 3, 4, 5, 6
_ACT_NAMES = {None: ACT_NONE, "none": ACT_NONE, "relu": ACT_RELU, "gelu": ACT_GELU, "gelu_tanh": ACT_GELU,
              "sigmoid": ACT_SIGMOID, "tanh": ACT_TANH, "relu6": ACT_RELU6, "drelu": ACT_DRELU}


def act_code(act) -> int:
    if isinstance(act, int):
        return act
    try:
        return _ACT_NAMES[act]
    except KeyError:
        raise ValueError(f"unknown activation {act!r}") from None


def _apply_act_ref(y: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_RELU:
        return torch.relu(y)
    if act == ACT_GELU:
        return F.gelu(y, approximate="tanh")
    if act == ACT_SIGMOID:
        return torch.sigmoid(y)
    if act == ACT_TANH:
        return torch.tanh(y)
    if act == ACT_RELU6:
        return torch.clamp(y, 0, 6)
    return y


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: torch.Tensor | None) -> int:
    return 0 if t is None else t.data_ptr()


def _check(t: torch.Tensor, name: str, dtype=torch.bfloat16, device=None):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: on {t.device}, expected {device}")


def _hip():
    return _ext.hip(required=True)


_ZERO_BIAS: dict = {}


def _zeros_bias(n: int, device) -> torch.Tensor:
    """Cached zero bias for bias-less layers (no allocation inside captured launches)."""
    key = (device, n)
    t = _ZERO_BIAS.get(key)
    if t is None:
        t = _ZERO_BIAS[key] = torch.zeros(n, dtype=torch.float32, device=device)
    return t


# ------------------------------------------------------------------------------ conv
# tile configs 0..4 are the register-staged igemm_bf16 tiles (-1: chosen by shape); the
# pipelined 256-pixel LDS-DMA kernel (igemm_v2) was in no default plan and was removed (r06)
def conv_out_hw(H, W, KH, KW, sh, sw, ph, pw, dh=1, dw=1, ph_hi=None, pw_hi=None):
    ph_hi = ph if ph_hi is None else ph_hi
    pw_hi = pw if pw_hi is None else pw_hi
    Ho = (H + ph + ph_hi - ((KH - 1) * dh + 1)) // sh + 1
    Wo = (W + pw + pw_hi - ((KW - 1) * dw + 1)) // sw + 1
    return Ho, Wo


def conv2d_nhwc(x: torch.Tensor, w_ohwi: torch.Tensor, bias: torch.Tensor | None = None,
                residual: torch.Tensor | None = None, stride=(1, 1), pad=(0, 0, 0, 0), dilation=(1, 1),
                act=None, out: torch.Tensor | None = None, out_channel_offset: int = 0, cfg: int = -1,
                out_scale: float | None = None) -> torch.Tensor:
    """NHWC conv, weights [Cout, KH, KW, Cin]; ``pad = (top, bottom, left, right)``.

    Fused epilogue ``act(conv + bias + residual)``.  With ``out`` given, the result is
    written at channel offset ``out_channel_offset`` of ``out`` (concat-by-stride-write).
    ``out_scale`` stores the result as OCP e4m3 bytes (``y / out_scale``, uint8): host
    reference only (the reference of ``conv2d_direct``'s fp8 epilogue).
    """
    a = act_code(act)
    N, H, W, Cin = x.shape
    Cout, KH, KW, Cin2 = w_ohwi.shape
    if Cin2 != Cin:
        raise ValueError(f"conv2d_nhwc: input has {Cin} channels, weights expect {Cin2}")
    sh, sw = stride
    pt, pb, pl, pr = pad
    dh, dw = dilation
    Ho, Wo = conv_out_hw(H, W, KH, KW, sh, sw, pt, pl, dh, dw, pb, pr)
    if out_scale is not None:
        if residual is not None:
            raise ValueError("conv2d_nhwc: fp8 output does not take a residual")
        if x.is_cuda:
            raise ValueError("conv2d_nhwc: e4m3 output is host-reference only on the implicit GEMM; "
                             "fp8 stems run on conv2d_direct")
    if out is None:
        odt = torch.uint8 if out_scale is not None else (x.dtype if x.is_cuda else torch.float32)
        out = torch.empty((N, Ho, Wo, Cout), dtype=odt, device=x.device)
        out_channel_offset = 0
    if out.shape[:3] != (N, Ho, Wo) or out_channel_offset + Cout > out.shape[3]:
        raise ValueError(f"conv2d_nhwc: out {tuple(out.shape)} cannot hold [{N},{Ho},{Wo},{Cout}] at "
                         f"offset {out_channel_offset}")
    if residual is not None and tuple(residual.shape) != (N, Ho, Wo, Cout):
        raise ValueError(f"conv2d_nhwc: residual {tuple(residual.shape)} != {(N, Ho, Wo, Cout)}")
    if x.is_cuda:
        for t, n in ((x, "x"), (w_ohwi, "w")):
            _check(t, n, device=x.device)
        _check(out, "out", torch.uint8 if out_scale is not None else torch.bfloat16, x.device)
        if residual is not None:
            _check(residual, "residual", device=x.device)
        if bias is not None:
            _check(bias, "bias", torch.float32, x.device)
            if bias.numel() != Cout:
                raise ValueError("conv2d_nhwc: bias size != Cout")
        else:
            bias = _zeros_bias(Cout, x.device)
        # bottom/right padding is implied by the kernel's bounds check (Ho/Wo carry it)
        _hip().conv2d_nhwc_bf16(x.data_ptr(), w_ohwi.data_ptr(), bias.data_ptr(), _ptr(residual), out.data_ptr(),
                                N, H, W, Cin, Cout, KH, KW, sh, sw, pt, pl, dh, dw, Ho, Wo, out.shape[3],
                                out_channel_offset, Cout if residual is None else residual.shape[3], a, _stream(), cfg)
        return out
    # host reference
    xn = x.float().permute(0, 3, 1, 2)
    xn = F.pad(xn, (pl, pr, pt, pb))
    y = F.conv2d(xn, w_ohwi.float().permute(0, 3, 1, 2), stride=(sh, sw), dilation=(dh, dw))
    y = y.permute(0, 2, 3, 1)
    if bias is not None:
        y = y + bias.float()
    if residual is not None:
        y = y + residual.float()
    y = _apply_act_ref(y, a)
    if out_scale is not None:
        from .fp8 import to_fp8_bytes

        out[..., out_channel_offset:out_channel_offset + Cout] = to_fp8_bytes(y / out_scale)
        return out
    out[..., out_channel_offset:out_channel_offset + Cout] = y.to(out.dtype)
    return out


def conv3x3_c64_eligible(x_shape, w_shape, stride, pad, dilation, residual, act) -> bool:
    """The persistent LDS-resident-weights kernel (kernels/conv3x3c64.hip): 3x3, stride 1,
    SAME padding, 64 -> 64 channels, no residual, bias (+ReLU) epilogue, H >= 8, W >= 32."""
    N, H, W, Cin = x_shape
    Cout, KH, KW, _ = w_shape
    return (Cin == 64 and Cout == 64 and (KH, KW) == (3, 3) and tuple(stride) == (1, 1) and tuple(pad) == (1, 1, 1, 1)
            and tuple(dilation) == (1, 1) and residual is None and act_code(act) in (ACT_NONE, ACT_RELU)
            and H >= 8 and W >= 32 and N * H * W * Cin * 2 < 2 ** 31)


_NUM_CU: dict = {}


class _PersistentCUs(dict):
    """CU count the persistent kernels size their grid to: the device's (caps of 224 / 192 /
    160 CUs, room for the sibling lane, measured -0.6 to -5 %: profiles/r04_ab)."""

    def __missing__(self, dev):
        self[dev] = torch.cuda.get_device_properties(dev).multi_processor_count
        return self[dev]


_NUM_CU = _PersistentCUs()


def conv3x3_c64(x: torch.Tensor, w_ohwi: torch.Tensor, bias: torch.Tensor, act=None, out: torch.Tensor | None = None,
                out_channel_offset: int = 0) -> torch.Tensor:
    """3x3 / s1 / SAME conv, 64 -> 64 channels, ``act(conv + bias)``; GPU: persistent
    kernel with the filter bank resident in LDS; host: the fp32 reference conv."""
    N, H, W, _ = x.shape
    a = act_code(act)
    if out is None:
        out = torch.empty((N, H, W, 64), dtype=x.dtype if x.is_cuda else torch.float32, device=x.device)
        out_channel_offset = 0
    if not conv3x3_c64_eligible(tuple(x.shape), tuple(w_ohwi.shape), (1, 1), (1, 1, 1, 1), (1, 1), None, a):
        raise ValueError(f"conv3x3_c64: unsupported shapes x {tuple(x.shape)} w {tuple(w_ohwi.shape)}")
    if out.shape[:3] != (N, H, W) or out_channel_offset + 64 > out.shape[3]:
        raise ValueError("conv3x3_c64: output buffer does not fit")
    if x.is_cuda:
        _check(x, "x", device=x.device)
        _check(w_ohwi, "w", device=x.device)
        _check(out, "out", device=x.device)
        _check(bias, "bias", torch.float32, x.device)
        dev = x.device.index if x.device.index is not None else torch.cuda.current_device()
        _hip().conv3x3c64_bf16(x.data_ptr(), w_ohwi.data_ptr(), bias.data_ptr(), out.data_ptr(), N, H, W, out.shape[3],
                               out_channel_offset, a, _NUM_CU[dev], _stream())
        return out
    return conv2d_nhwc(x, w_ohwi, bias, None, (1, 1), (1, 1, 1, 1), (1, 1), a, out=out,
                       out_channel_offset=out_channel_offset)


def bottleneck_tail(x2: torch.Tensor, res: torch.Tensor | None, w3: torch.Tensor, b3: torch.Tensor, w1: torch.Tensor,
                    b1: torch.Tensor, y3: torch.Tensor | None = None, y1: torch.Tensor | None = None,
                    xs: torch.Tensor | None = None, y3_decimated: bool = False):
    """Fused ResNet bottleneck block boundary (kernels/bottleneck.hip):
    ``y3 = relu(x2 @ w3^T + b3 + res)`` (1x1 expand CX -> 4 CX with residual) and
    ``y1 = relu(y3 @ w1^T + b1)`` (the next block's 1x1 reduce 4 CX -> CN); returns
    ``(y3, y1)``.  Variants: CX = 64 (stage 1) with CN = 64 or 128 (a stage-2 form with the
    weights streamed through LDS measured no faster than the two convs and was removed:
    profiles/r01_tail).  Dual form (stage 1's first block, stride-1
    projection shortcut): ``xs [..., 64]`` instead of ``res`` and ``w3 [256, 128]`` =
    [expand | projection] — ``y3 = relu([x2 | xs] @ w3^T + b3)`` (CN = 64).  Weights are 1x1
    OHWI squeezed ([out, in]), biases fp32.  GPU: one persistent kernel, y3 reused from LDS;
    host: the fp32 reference with y3 rounded to the output dtype before the second GEMM.

    ``y3_decimated``: ``x2`` is ``[N, H, W, 64]`` and only the even-(h, w) pixels of y3 are
    stored, compact as ``[N, H/2, W/2, 256]`` — for a y3 whose only other reader is a
    stride-2 1x1 projection shortcut (ResNet v1.5's stage-1 -> stage-2 boundary)."""
    lead = x2.shape[:-1]
    dec_hw = (0, 0)
    if y3_decimated:
        if x2.dim() != 4 or x2.shape[1] % 2 or x2.shape[2] % 2 or x2.shape[-1] != 64:
            raise ValueError("bottleneck_tail: decimated y3 needs x2 [N, H, W, 64] with even H, W")
        dec_hw = (x2.shape[1], x2.shape[2])
    dual = xs is not None
    cx = x2.shape[-1]
    co = 4 * cx
    cn = w1.shape[0]
    if (res is None) != dual:
        raise ValueError("bottleneck_tail: pass exactly one of res and xs")
    if (cx, dual, cn) not in ((64, True, 64), (64, False, 64), (64, False, 128)):
        raise ValueError(f"bottleneck_tail: unsupported variant x2 [..., {cx}], dual {dual}, reduce width {cn}")
    k3 = 2 * cx if dual else cx
    if (dual and tuple(xs.shape) != (*lead, cx)) or (not dual and tuple(res.shape) != (*lead, co)):
        raise ValueError(f"bottleneck_tail: the second input must be [..., {cx if dual else co}]")
    if tuple(w3.reshape(w3.shape[0], -1).shape) != (co, k3) or tuple(w1.reshape(cn, -1).shape) != (cn, co):
        raise ValueError(f"bottleneck_tail: weights must be [{co}, {k3}] and [{cn}, {co}], got {tuple(w3.shape)} "
                         f"{tuple(w1.shape)}")
    if b3.numel() != co or b1.numel() != cn:
        raise ValueError("bottleneck_tail: bias sizes must match the output channels")
    odt = x2.dtype if x2.is_cuda else torch.float32
    lead3 = (lead[0], dec_hw[0] // 2, dec_hw[1] // 2) if y3_decimated else lead
    y3 = torch.empty((*lead3, co), dtype=odt, device=x2.device) if y3 is None else y3
    y1 = torch.empty((*lead, cn), dtype=odt, device=x2.device) if y1 is None else y1
    if tuple(y3.shape) != (*lead3, co) or tuple(y1.shape) != (*lead, cn):
        raise ValueError("bottleneck_tail: output buffers do not fit")
    M = x2.numel() // cx
    second = xs if dual else res
    if x2.is_cuda:
        for t, n in ((x2, "x2"), (second, "xs" if dual else "res"), (w3, "w3"), (w1, "w1"), (y3, "y3"), (y1, "y1")):
            _check(t, n, device=x2.device)
        _check(b3, "b3", torch.float32, x2.device)
        _check(b1, "b1", torch.float32, x2.device)
        dev = x2.device.index if x2.device.index is not None else torch.cuda.current_device()
        _hip().bottleneck_tail_bf16(x2.data_ptr(), _ptr(xs), _ptr(res), w3.data_ptr(), b3.data_ptr(),
                                    w1.data_ptr(), b1.data_ptr(), y3.data_ptr(), y1.data_ptr(), M, cn,
                                    _NUM_CU[dev], _stream(), dec_hw[0], dec_hw[1])
        return y3, y1
    xin = torch.cat([x2.reshape(M, cx), xs.reshape(M, cx)], 1) if dual else x2.reshape(M, cx)
    a = xin.float() @ w3.reshape(co, k3).float().t() + b3.float()
    a = a.to(odt).float()  # the kernel rounds acc + bias first
    a = torch.relu(a if dual else a + res.reshape(M, co).float()).to(y3.dtype)
    y3.copy_(a.reshape(*lead, co)[:, ::2, ::2] if y3_decimated else a.reshape(y3.shape))
    b = torch.relu(a.float() @ w1.reshape(cn, co).float().t() + b1.float())
    y1.copy_(b.reshape(y1.shape).to(y1.dtype))
    return y3, y1


def bottleneck_chain(links, w1: torch.Tensor, b1: torch.Tensor, y1: torch.Tensor | None = None,
                     y3: torch.Tensor | None = None, y3_decimated: bool = False, store_y3: bool = True):
    """ResNet stage 1's residual stream recomputed instead of re-read (kernels/bottleneck_chain.hip):
    ``links`` = [(c1, x0, w_a, b_a), (c2, None, w_b, b_b), ...] (1 to 3), ``y = relu([c1|x0] .
    w_a^T + b_a)`` then ``y = relu(c_j . w_j^T + b_j + y)`` per further link — each link rounded
    exactly as ``bottleneck_tail`` rounds it (acc + b -> bf16, + residual, relu -> bf16) — then
    ``y1 = relu(y . w1^T + b1)``.  The last ``y`` is stored into ``y3`` only with
    ``store_y3`` (``y3_decimated``: the even-(h, w) pixels, compact).  Returns ``(y3 or None, y1)``.
    All sources [..., 64] of one pixel count; w_a [256, 128], the others [256, 64]; w1 [cn, 256]."""
    x0 = links[0][0]
    lead = x0.shape[:-1]
    M = x0.numel() // 64
    cn = w1.shape[0]
    if not 1 <= len(links) <= 3 or links[0][1] is None or any(l[1] is not None for l in links[1:]):
        raise ValueError("bottleneck_chain: 1 to 3 links, the first dual ([x | xs]), the others plain")
    for j, (x, xs, w, b) in enumerate(links):
        if x.shape[-1] != 64 or x.numel() != M * 64 or (xs is not None and tuple(xs.shape) != tuple(x.shape)):
            raise ValueError("bottleneck_chain: every source is [..., 64] over the same pixels")
        if tuple(w.reshape(w.shape[0], -1).shape) != (256, 128 if j == 0 else 64) or b.numel() != 256:
            raise ValueError(f"bottleneck_chain: link {j} weights must be [256, {128 if j == 0 else 64}]")
    if cn not in (64, 128) or tuple(w1.reshape(cn, -1).shape) != (cn, 256) or b1.numel() != cn:
        raise ValueError("bottleneck_chain: w1 must be [64 or 128, 256]")
    dec_hw = (0, 0)
    if y3_decimated:
        if x0.dim() != 4 or x0.shape[1] % 2 or x0.shape[2] % 2:
            raise ValueError("bottleneck_chain: decimated y3 needs [N, H, W, 64] sources with even H, W")
        dec_hw = (x0.shape[1], x0.shape[2])
    odt = x0.dtype if x0.is_cuda else torch.float32
    lead3 = (lead[0], dec_hw[0] // 2, dec_hw[1] // 2) if y3_decimated else lead
    if store_y3 and y3 is None:
        y3 = torch.empty((*lead3, 256), dtype=odt, device=x0.device)
    y1 = torch.empty((*lead, cn), dtype=odt, device=x0.device) if y1 is None else y1
    if (store_y3 and tuple(y3.shape) != (*lead3, 256)) or tuple(y1.shape) != (*lead, cn):
        raise ValueError("bottleneck_chain: output buffers do not fit")
    if x0.is_cuda:
        for j, (x, xs, w, b) in enumerate(links):
            for t, n in ((x, "x"), (w, "w")) + (((xs, "xs"),) if xs is not None else ()):
                _check(t, f"link {j} {n}", device=x0.device)
            _check(b, f"link {j} bias", torch.float32, x0.device)
        _check(w1, "w1", device=x0.device)
        _check(b1, "b1", torch.float32, x0.device)
        _check(y1, "y1", device=x0.device)
        if store_y3:
            _check(y3, "y3", device=x0.device)
        dev = x0.device.index if x0.device.index is not None else torch.cuda.current_device()
        _hip().bottleneck_chain_bf16([(x.data_ptr(), _ptr(xs), w.data_ptr(), b.data_ptr()) for x, xs, w, b in links],
                                     w1.data_ptr(), b1.data_ptr(), y3.data_ptr() if store_y3 else 0, y1.data_ptr(), M,
                                     cn, _NUM_CU[dev], _stream(), dec_hw[0], dec_hw[1])
        return (y3 if store_y3 else None), y1
    y = None
    rdt = y1.dtype  # each link's y3 rounded as the unfused tail's y3 buffer would hold it
    for x, xs, w, b in links:
        xin = torch.cat([x.reshape(M, 64), xs.reshape(M, 64)], 1) if xs is not None else x.reshape(M, 64)
        a = (xin.float() @ w.reshape(256, -1).float().t() + b.float()).to(odt).float()
        y = torch.relu(a if y is None else a + y).to(rdt).float()
    if store_y3:
        y3.copy_(y.reshape(*lead, 256)[:, ::2, ::2] if y3_decimated else y.reshape(y3.shape))
    y1.copy_(torch.relu(y @ w1.reshape(cn, 256).float().t() + b1.float()).reshape(y1.shape).to(y1.dtype))
    return (y3 if store_y3 else None), y1


def gemm(x: torch.Tensor, w_nk: torch.Tensor, bias: torch.Tensor | None = None, residual: torch.Tensor | None = None,
         act=None, out: torch.Tensor | None = None, cfg: int = -1) -> torch.Tensor:
    """``act(x[M,K] @ w[N,K]^T + bias + residual)``; leading dims of x are flattened."""
    a = act_code(act)
    lead = x.shape[:-1]
    K = x.shape[-1]
    N, K2 = w_nk.shape
    if K != K2:
        raise ValueError(f"gemm: K mismatch {K} vs {K2}")
    x2 = x.reshape(-1, K)
    M = x2.shape[0]
    if out is None:
        out = torch.empty((*lead, N), dtype=x.dtype if x.is_cuda else torch.float32, device=x.device)
    out2 = out.reshape(M, N)
    if residual is not None and residual.numel() != M * N:
        raise ValueError("gemm: residual shape mismatch")
    if x.is_cuda:
        _check(x2, "x", device=x.device)
        _check(w_nk, "w", device=x.device)
        _check(out2, "out", device=x.device)
        if bias is not None:
            _check(bias, "bias", torch.float32, x.device)
        else:
            bias = _zeros_bias(N, x.device)
        if residual is not None:
            _check(residual, "residual", device=x.device)
        _hip().gemm_bf16(x2.data_ptr(), w_nk.data_ptr(), bias.data_ptr(), _ptr(residual), out2.data_ptr(), M, N, K, K,
                         N, N, a, _stream(), cfg)
        return out
    y = x2.float() @ w_nk.float().t()
    if bias is not None:
        y = y + bias.float()
    if residual is not None:
        y = y + residual.reshape(M, N).float()
    out2.copy_(_apply_act_ref(y, a).to(out.dtype))
    return out


# ------------------------------------------------------------------------------ gemm_train
_TR_KTILE_US = 0.45       # one 128x128x64 K step, two workgroups sharing a CU (2-stage ring)
_TR_KTILE_DEEP_US = 0.3   # the same with the CU to itself (4-stage ring, grids <= one per CU)
_TR_SLOTS = 512           # resident 128x128 workgroups (2 per CU)


def _tr_time(tiles: int, per: int, se: int, num_cu: int = 256) -> float:
    wgs = tiles * se
    if wgs <= num_cu:
        return per * _TR_KTILE_DEEP_US
    return -(-wgs // _TR_SLOTS) * per * _TR_KTILE_US


def gemm_train_splits(M: int, N: int, K: int) -> int:
    """Split-K factor for ``gemm_train``: rounds of resident 128x128 workgroups times K
    steps, plus the fp32 slab round trip of the reduction and its launch."""
    tiles = -(-M // 128) * -(-N // 128)
    nk = -(-K // 64)
    best_s, best_t = 1, _tr_time(tiles, nk, 1)
    for s in (2, 3, 4, 6, 8, 12, 16, 24, 32):
        if s > nk:
            break
        per = -(-nk // s)
        se = -(-nk // per)
        t = _tr_time(tiles, per, se) + se * M * N * 8 / _PP_SPLIT_BW + 2.0
        if t < 0.9 * best_t:
            best_s, best_t = se, t
    return best_s


def gemm_train(x: torch.Tensor, w: torch.Tensor, *, x_t: bool = False, w_t: bool = False,
               bias: torch.Tensor | None = None, mask: torch.Tensor | None = None, act=None,
               out: torch.Tensor | None = None, out_dtype=torch.bfloat16, splits: int | None = None,
               ws: torch.Tensor | None = None, colsum: torch.Tensor | None = None) -> torch.Tensor:
    """``epi(X @ W^T)`` on the layout-general training GEMM (``kernels/gemm_train.hip``).

    ``X`` is ``x`` [M, K] (K-contiguous) or, with ``x_t``, ``x`` stored [K, M]; ``W`` is
    ``w`` [N, K] or, with ``w_t``, ``w`` stored [K, N] — so a dense layer's three GEMMs need
    no transposed copies: forward ``gemm_train(h, W)``, dX ``gemm_train(dA, W, w_t=True)``,
    dW ``gemm_train(dA, h, x_t=True, w_t=True, out_dtype=torch.float32)``.  ``mask`` (bf16
    [M, N], e.g. the layer input) applies the ReLU backward ``mask > 0 ? y : 0`` (and takes no
    other activation); ``out`` and ``mask`` may be row-strided views.  fp32 output takes no activation.  ``splits`` > 1 runs split-K
    (None: cost model) with an fp32 workspace ``ws`` (>= splits*M*N floats).  ``colsum``
    (fp32 [ceil(M/128), N], bf16 output, no split) receives every 128-row tile's column sums
    of the stored values — ``colsum_reduce`` turns them into the next layer's bias gradient.
    K must be a multiple of 8 (a partial last K tile reads zeros)."""
    a = act_code(act)
    if mask is not None:
        if a not in (ACT_NONE, ACT_DRELU):
            raise ValueError("gemm_train: mask is the ReLU-backward operand; it takes no other activation")
        a = ACT_DRELU
    M, K = (x.shape[1], x.shape[0]) if x_t else (x.shape[0], x.shape[1])
    N, K2 = (w.shape[1], w.shape[0]) if w_t else (w.shape[0], w.shape[1])
    if K != K2:
        raise ValueError(f"gemm_train: K mismatch {K} vs {K2}")
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=x.device)
    if tuple(out.shape) != (M, N):
        raise ValueError(f"gemm_train: out shape {tuple(out.shape)} != {(M, N)}")
    f32 = out.dtype == torch.float32
    if not x.is_cuda:  # reference path (CPU): same math in fp32
        X = x.float().t() if x_t else x.float()
        W = w.float() if w_t else w.float().t()
        y = X @ W
        if bias is not None:
            y = y + bias.float()
        if mask is not None:
            y = torch.where(mask.float() > 0, y, torch.zeros_like(y))
        else:
            y = _apply_act_ref(y, a)
        out.copy_(y.to(out.dtype))
        if colsum is not None:
            yq = out.float()
            for t in range(colsum.shape[0]):
                colsum[t].copy_(yq[t * 128:(t + 1) * 128].sum(0))
        return out
    for t, nm in ((x, "x"), (w, "w")):  # row-strided views are fine (ld = stride(0))
        if t.dtype != torch.bfloat16 or t.device != x.device or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"gemm_train: {nm} must be a bf16 [rows, cols] view with contiguous rows on {x.device}")
    if out.stride(1) != 1:
        raise ValueError("gemm_train: out rows must be contiguous")
    if bias is not None:
        _check(bias, "bias", torch.float32, x.device)
    if mask is not None:
        if mask.dtype != torch.bfloat16 or mask.device != x.device:
            raise ValueError(f"gemm_train: mask must be bf16 on {x.device}")
        if tuple(mask.shape) != (M, N) or mask.stride(1) != 1:  # a row-strided view is fine (ldr = stride(0))
            raise ValueError("gemm_train: mask must be [M, N] with contiguous rows")
    if colsum is not None:
        if f32 or tuple(colsum.shape) != (-(-M // 128), N) or colsum.dtype != torch.float32 or not colsum.is_contiguous():
            raise ValueError("gemm_train: colsum must be contiguous fp32 [ceil(M/128), N] with bf16 output")
        splits = 1
    s = gemm_train_splits(M, N, K) if splits is None else int(splits)
    s = _hip().gemm_train_splits(K, s)
    wsp = 0
    if s > 1:
        need = s * M * N
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.float32, device=x.device)
        wsp = ws.data_ptr()
    _hip().gemm_train(x.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(mask), out.data_ptr(), M, N, K, x.stride(0),
                      w.stride(0), out.stride(0), mask.stride(0) if mask is not None else 0, bool(x_t), bool(w_t), a,
                      f32, s, wsp, _ptr(colsum), _stream())
    return out


def colsum_reduce(part: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """``out[n] = sum_t part[t, n]`` in fixed order (``gemm_train``'s per-tile column sums ->
    a bias gradient); ``part`` may be a column slice of a wider partial buffer."""
    T, N = part.shape
    if out.numel() != N:
        raise ValueError("colsum_reduce: out must hold N floats")
    if not part.is_cuda:
        out.copy_(part.sum(0).reshape(out.shape))
        return out
    if part.stride(1) != 1 or not out.is_contiguous():
        raise ValueError("colsum_reduce: contiguous rows / output")
    _hip().colsum_reduce(part.data_ptr(), T, part.stride(0), N, out.data_ptr(), _stream())
    return out


# ------------------------------------------------------------------------------ gemm_pp
_PP_KTILE_US = 1.5    # one 256x256x64 K step of one workgroup (measured: 1.39 PF at 8192^3)
_PP_SPLIT_BW = 5.0e6  # bytes per microsecond of the fp32 partial round trip (write + read)


def gemm_pp_splits(M: int, N: int, K: int, num_cu: int = 256) -> int:
    """Split-K factor for ``gemm_pp`` from a small cost model: waves of 256x256 tiles times
    K steps, plus the fp32 partial slices written and re-read by the reduction and one
    extra launch.  Splits only when that wins by >10 % (small-M heads, few-tile shapes)."""
    tiles = -(-M // 256) * -(-N // 256)
    nk = K // 64
    best_s, best_t = 1, -(-tiles // num_cu) * nk * _PP_KTILE_US
    for s in range(2, min(16, nk) + 1):
        per = -(-nk // s)
        se = -(-nk // per)
        t = -(-tiles * se // num_cu) * per * _PP_KTILE_US + 2.0 * se * M * N * 4 / _PP_SPLIT_BW + 2.0
        if t < 0.9 * best_t:
            best_s, best_t = se, t
    return best_s


def gemm_pp(x: torch.Tensor, w_nk: torch.Tensor, bias: torch.Tensor | None = None,
            residual: torch.Tensor | None = None, act=None, out: torch.Tensor | None = None,
            splits: int | None = None, out_col: int = 0, ws: torch.Tensor | None = None) -> torch.Tensor:
    """``act(x[M,K] @ w[N,K]^T + bias (+ residual))`` on the ping-pong 256x256 MFMA kernel
    (``kernels/gemm_pp.hip``).  ``out`` may be wider than N (``out_col`` = first column:
    concat-by-stride-write).  ``splits`` > 1 runs split-K (None: cost model) through the
    fp32 workspace ``ws`` (>= splits*M*N floats); without one a temporary is allocated per
    call — stream-ordered, and inside hipGraph capture it comes from the graph's pool."""
    a = act_code(act)
    lead = x.shape[:-1]
    K = x.shape[-1]
    N, K2 = w_nk.shape
    if K != K2:
        raise ValueError(f"gemm_pp: K mismatch {K} vs {K2}")
    x2 = x.reshape(-1, K)
    M = x2.shape[0]
    if out is None:
        out = torch.empty((*lead, N), dtype=x.dtype if x.is_cuda else torch.float32, device=x.device)
    ldy = out.shape[-1]
    out2 = out.reshape(-1, ldy)
    if out2.shape[0] != M or out_col + N > ldy:
        raise ValueError("gemm_pp: output shape mismatch")
    if residual is not None and residual.numel() != M * N:
        raise ValueError("gemm_pp: residual shape mismatch")
    if x.is_cuda:
        if K % 64 or N % 8 or ldy % 8 or out_col % 8:
            raise ValueError("gemm_pp: needs K % 64 == 0 and N, ldy, out_col % 8 == 0")
        _check(x2, "x", device=x.device)
        _check(w_nk, "w", device=x.device)
        _check(out2, "out", device=x.device)
        if bias is not None:
            _check(bias, "bias", torch.float32, x.device)
        if residual is not None:
            _check(residual, "residual", device=x.device)
        if splits is None:
            splits = gemm_pp_splits(M, N, K)
        splits = _hip().gemm_pp_splits(K, splits)
        if splits > 1:
            if ws is None:
                ws = torch.empty(splits * M * N, dtype=torch.float32, device=x.device)
            elif ws.dtype != torch.float32 or ws.device != x.device or ws.numel() < splits * M * N:
                raise ValueError(f"gemm_pp: workspace needs {splits * M * N} fp32 elements on {x.device}")
        else:
            ws = None
        _hip().gemm_pp(x2.data_ptr(), w_nk.data_ptr(), _ptr(bias), _ptr(residual), out2.data_ptr(), M, N, K, K, K,
                       ldy, out_col, N, a, splits, _ptr(ws), _stream())
        return out
    y = x2.float() @ w_nk.float().t()
    if bias is not None:
        y = y + bias.float()
    if a == ACT_DRELU:  # the residual operand is the ReLU mask source, not an addend
        if residual is None:
            raise ValueError("gemm_pp: act 'drelu' needs the mask operand (residual)")
        out2[:, out_col:out_col + N] = torch.where(residual.reshape(M, N).float() > 0, y, 0.0).to(out.dtype)
        return out
    if residual is not None:
        y = y + residual.reshape(M, N).float()
    out2[:, out_col:out_col + N] = _apply_act_ref(y, a).to(out.dtype)
    return out


class ConvPP:
    """A planned ``conv_lite`` launch (kernels/conv_pp.hip): implicit-GEMM NHWC convolution
    of one or two sources into one accumulator on the 4-wave 128x128 LDS-DMA tile, the only
    tile: the ping-pong / wide / wave-split / two-wave / deeper-prefetch tiles and split-K
    measured slower and were removed (``kernels/conv_pp.hip``).

    ``srcs``: [(x_shape NHWC, (KH, KW), (sh, sw), (pt, pl), (dh, dw))]; the weight is the
    concatenation of the sources' OHWI filters, [Cout, sum KH*KW*C] bf16; a second source
    must be 1x1, unpadded and in range (a projection shortcut).  The plan holds shapes only:
    nothing is allocated on ``device``.  ``tile`` / ``splits`` no longer select anything:
    a caller written against the earlier signature may still pass ``None`` (it meant "the
    default"); any value is a ``TypeError``."""

    def __init__(self, srcs, Cout: int, out_hw, device, tile: None = None, splits: None = None):
        if tile is not None or splits is not None:
            raise TypeError("conv_pp: the tile and splits arguments are gone (one tile, no split-K)")
        self.srcs = [(tuple(xs), tuple(k), tuple(st), tuple(pd), tuple(dl)) for xs, k, st, pd, dl in srcs]
        self.N = self.srcs[0][0][0]
        self.OH, self.OW = out_hw
        self.Cout = Cout
        self.K = sum(k[0] * k[1] * xs[3] for xs, k, _, _, _ in self.srcs)
        for xs, _, _, _, _ in self.srcs:
            if xs[3] % 64 or xs[0] != self.N:
                raise ValueError("conv_pp: channels must be multiples of 64 and batches equal")
        if Cout % 8:
            raise ValueError("conv_pp: Cout % 8")
        self.M = self.N * self.OH * self.OW
        if len(self.srcs) == 2:
            (xs1, k1, st1, pd1, dl1) = self.srcs[1]
            if tuple(k1) != (1, 1) or tuple(pd1) != (0, 0) or (self.OH - 1) * st1[0] >= xs1[1] \
                    or (self.OW - 1) * st1[1] >= xs1[2]:
                raise ValueError("conv_pp: the 4-wave tile's second source must be 1x1, unpadded, in range")

    def for_batch(self, n: int) -> "ConvPP":
        """The same convolution planned for ``n`` images (a batch slice: the compiler's
        batch-slice chain); cached per ``n`` on the full-batch plan."""
        if n == self.N:
            return self
        subs = self.__dict__.setdefault("_subs", {})
        sub = subs.get(n)
        if sub is None:
            sub = copy.copy(self)
            sub.srcs = [((n, *xs[1:]), k, st, pd, dl) for xs, k, st, pd, dl in self.srcs]
            sub.N, sub.M, sub._subs = n, n * self.OH * self.OW, {}
            if n > self.N:
                raise ValueError("conv_pp: a batch slice larger than the planned batch")
            subs[n] = sub
        return sub

    def __call__(self, xs, w, bias=None, residual=None, act=None, out=None, out_channel_offset: int = 0):
        if len(xs) != len(self.srcs):
            raise ValueError("conv_pp: source count")
        if xs and xs[0].dim() == 4 and xs[0].shape[0] != self.N:
            return self.for_batch(int(xs[0].shape[0]))(xs, w, bias, residual, act, out, out_channel_offset)
        for x, (shape, *_r) in zip(xs, self.srcs):
            if tuple(x.shape) != shape:
                raise ValueError(f"conv_pp: input shape {tuple(x.shape)} != planned {shape}")
        if out is None:
            out = torch.empty((self.N, self.OH, self.OW, self.Cout), dtype=torch.bfloat16, device=xs[0].device)
        ldy = out.shape[-1]
        if tuple(out.shape[:3]) != (self.N, self.OH, self.OW) or out_channel_offset + self.Cout > ldy:
            raise ValueError("conv_pp: output shape mismatch")
        if tuple(w.shape) != (self.Cout, self.K):
            raise ValueError(f"conv_pp: weight {tuple(w.shape)} != ({self.Cout}, {self.K})")
        if not xs[0].is_cuda:
            return self._reference(xs, w, bias, residual, act, out, out_channel_offset)
        for i, x in enumerate(xs):
            _check(x, f"x{i}", device=out.device)
        _check(w, "w", device=out.device)
        _check(out, "out", device=out.device)
        if bias is not None:
            _check(bias, "bias", torch.float32, out.device)
        if residual is not None:
            _check(residual, "residual", device=out.device)
            if residual.numel() != self.M * self.Cout:
                raise ValueError("conv_pp: residual shape")
        srcs = [(x.data_ptr(), self.N, sh[1], sh[2], sh[3], k[0], k[1], st[0], st[1], pd[0], pd[1], dl[0], dl[1])
                for x, (sh, k, st, pd, dl) in zip(xs, self.srcs)]
        _hip().conv_pp(srcs, w.data_ptr(), _ptr(bias), _ptr(residual), out.data_ptr(), self.N, self.OH, self.OW,
                       self.Cout, ldy, out_channel_offset, self.Cout, act_code(act), _stream())
        return out

    def _reference(self, xs, w, bias, residual, act, out, coff):
        """fp32 host reference (CPU tests): the sum of the sources' convolutions."""
        import torch.nn.functional as F

        y = 0
        k0 = 0
        for x, (sh, (KH, KW), (s_h, s_w), (pt, pl), (dh, dw)) in zip(xs, self.srcs):
            C = sh[3]
            wk = w[:, k0:k0 + KH * KW * C].float().reshape(self.Cout, KH, KW, C).permute(0, 3, 1, 2)
            k0 += KH * KW * C
            xi = x.float().permute(0, 3, 1, 2)
            ph_hi = max(0, (self.OH - 1) * s_h + (KH - 1) * dh + 1 - sh[1] - pt)
            pw_hi = max(0, (self.OW - 1) * s_w + (KW - 1) * dw + 1 - sh[2] - pl)
            xi = F.pad(xi, (pl, pw_hi, pt, ph_hi))
            yi = F.conv2d(xi, wk, stride=(s_h, s_w), dilation=(dh, dw))[:, :, :self.OH, :self.OW]
            y = y + yi
        y = y.permute(0, 2, 3, 1)
        if bias is not None:
            y = y + bias.float()
        if residual is not None:
            y = y + residual.reshape(y.shape).float()
        out[..., coff:coff + self.Cout] = _apply_act_ref(y, act_code(act)).to(out.dtype)
        return out


# ------------------------------------------------------------------------------ preprocess
def preprocess_images(images_u8: torch.Tensor, out_hw=(224, 224), mean=(117.0, 117.0, 117.0),
                      std=(1.0, 1.0, 1.0), align_corners=False, half_pixel_centers=False,
                      out: torch.Tensor | None = None, s2d: bool = False) -> torch.Tensor:
    """uint8 [B,H,W,3] → resize (TF ResizeBilinear) → (v-mean)/std → bf16.

    Layout ``[B,Ho,Wo,8]`` (channels 3..7 zero), or with ``s2d`` the 2x2 space-to-depth
    layout ``[B,ceil(Ho/2),ceil(Wo/2),16]`` consumed by the stride-2 stem conv
    (``s2d_stem_weights``); an odd size zero-fills the pixels past the image."""
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
        raise ValueError("preprocess_images expects uint8 [B,H,W,3]")
    B, Hi, Wi, _ = images_u8.shape
    Ho, Wo = out_hw
    oshape = (B, (Ho + 1) // 2, (Wo + 1) // 2, 16) if s2d else (B, Ho, Wo, 8)
    if out is None:
        out = torch.empty(oshape, dtype=torch.bfloat16 if images_u8.is_cuda else torch.float32,
                          device=images_u8.device)
    if tuple(out.shape) != oshape:
        raise ValueError(f"preprocess_images: out must be {oshape}, got {tuple(out.shape)}")
    if images_u8.is_cuda:
        if not images_u8.is_contiguous():
            raise ValueError("preprocess_images: input must be contiguous")
        _check(out, "out", device=images_u8.device)
        _hip().preprocess_u8_to_bf16(images_u8.data_ptr(), out.data_ptr(), B, Hi, Wi, Ho, Wo, int(align_corners),
                                     int(half_pixel_centers), float(mean[0]), float(mean[1]), float(mean[2]),
                                     1.0 / std[0], 1.0 / std[1], 1.0 / std[2], Hi * Wi * 3, int(s2d), _stream())
        return out
    from ..graph.ops_nn import resize_bilinear_tf

    y = resize_bilinear_tf(images_u8.float(), Ho, Wo, align_corners, half_pixel_centers)
    y = (y - torch.tensor(mean)) / torch.tensor(std)
    out.zero_()
    if s2d:
        Hb, Wb = (Ho + 1) // 2, (Wo + 1) // 2
        y = F.pad(y, (0, 0, 0, 2 * Wb - Wo, 0, 2 * Hb - Ho))
        blk = y.reshape(B, Hb, 2, Wb, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, Hb, Wb, 12)
        out[..., :12] = blk.to(out.dtype)
    else:
        out[..., :3] = y.to(out.dtype)
    return out


def jpeg_idct_rgb(coef: torch.Tensor, headers: torch.Tensor, out: torch.Tensor, n: int, H: int, W: int,
                  stream: int | None = None, threads: int = 8) -> torch.Tensor:
    """The arithmetic half of the JPEG decode: ``n`` coefficient rows (``coef[i]``, one
    contiguous row of int16 coefficients per image, viewed as any dtype) and their headers
    (``_native.jpeg_entropy_into``) -> RGB ``out[i]`` of uint8 ``[H, W, 3]``.  Images whose
    header status is non-zero are skipped: their rows are not touched.  On the GPU the HIP
    kernel (``kernels/jpeg.hip``) on ``stream`` (None: the current one), no allocation, no
    synchronisation; on the host the scalar back half of ``csrc/jpeg.cpp`` on ``threads``
    pool threads — the same arithmetic, so both give the same bytes."""
    if out.dtype != torch.uint8 or out.dim() != 4 or tuple(out.shape[1:]) != (H, W, 3) or not out.is_contiguous():
        raise ValueError(f"jpeg_idct_rgb: out must be contiguous uint8 [n, {H}, {W}, 3]")
    if coef.dim() != 2 or headers.dim() != 2 or not coef.is_contiguous() or not headers.is_contiguous():
        raise ValueError("jpeg_idct_rgb: coef and headers are contiguous [n, row bytes]")
    if n < 0 or n > min(coef.shape[0], headers.shape[0], out.shape[0]):
        raise ValueError("jpeg_idct_rgb: n exceeds the rows given")
    if coef.device != out.device or headers.device != out.device:
        raise ValueError("jpeg_idct_rgb: coef, headers and out must be on one device")
    stride = coef.shape[1] * coef.element_size()
    hbytes = headers.shape[1] * headers.element_size()
    if hbytes != _ext.native().jpeg_coeff_layout(H, W)[1]:
        raise ValueError("jpeg_idct_rgb: headers are not jpeg_coeff_layout's size")
    if out.is_cuda:
        _hip().jpeg_idct_rgb(coef.data_ptr(), headers.data_ptr(), out.data_ptr(), n, H, W, stride,
                             _stream() if stream is None else stream)
    else:
        _ext.native().jpeg_coeffs_to_rgb(coef.data_ptr(), n * stride, headers.data_ptr(), n * hbytes, out.data_ptr(),
                                         n * H * W * 3, n, stride, H * W * 3, H, W, threads)
    return out


def s2d_stem_weights(w_hwio: torch.Tensor, H: int, W: int, pads):
    """Rewrites a stride-2 KxK conv over RGB (pads top/left even) as a stride-1
    ceil(K/2)² conv over the 2x2 space-to-depth input (16 channels, 12 used).

    Returns ``(w_ohwi [Cout, KBH, KBW, 16], block_pads (t, b, l, r))``.  Cuts the stem's
    MFMA work from K = 7·7·8 = 392 to 4·4·16 = 256 and makes every 16-B im2col load useful.
    """
    KH, KW, C, Cout = w_hwio.shape
    pt, pb, pl, pr = pads
    if C != 3 or pt % 2 or pl % 2:
        raise ValueError("s2d stem needs RGB input and even top/left padding")
    KBH, KBW = (KH + 1) // 2, (KW + 1) // 2
    w2 = torch.zeros(Cout, KBH, KBW, 16, dtype=torch.float32)
    wf = w_hwio.float()
    for kh in range(KH):
        for kw in range(KW):
            ch = ((kh % 2) * 2 + (kw % 2)) * 3
            w2[:, kh // 2, kw // 2, ch:ch + 3] = wf[kh, kw].t()
    Ho = (H + pt + pb - KH) // 2 + 1
    Wo = (W + pl + pr - KW) // 2 + 1
    Hb, Wb = (H + 1) // 2, (W + 1) // 2  # an odd size's last block is zero-filled past the image
    pt_b, pl_b = pt // 2, pl // 2
    pb_b = Ho - 1 + KBH - Hb - pt_b
    pr_b = Wo - 1 + KBW - Wb - pl_b
    if pb_b < 0 or pr_b < 0:
        raise ValueError("s2d stem: negative block padding")
    return w2, (pt_b, pb_b, pl_b, pr_b)


# ------------------------------------------------------------------------------ depthwise conv
# output tile per thread of the 3x3 kernel (kernels/dwconv.hip); 0 = the launcher's choice
DWCONV_TILES = {"1x4": 1, "2x2": 2}
DWCONV_GENERIC = -1


def dwconv_eligible(C: int, KH: int, KW: int, stride=(1, 1), dilation=(1, 1)) -> bool:
    """What ``dwconv_nhwc_bf16`` takes: 8-channel vectors, a filter of at most 7x7."""
    return (C > 0 and C % 8 == 0 and 1 <= KH <= 7 and 1 <= KW <= 7 and min(stride) >= 1 and min(dilation) >= 1)


def dwconv_impl(KH: int, KW: int, stride=(1, 1), dilation=(1, 1)) -> str:
    """The kernel the host launcher picks: the register-tiled 3x3 (dilation 1, stride 1 or
    2: every MobileNet layer) or the generic one."""
    if (KH, KW) == (3, 3) and tuple(dilation) == (1, 1) and tuple(stride) in ((1, 1), (2, 2)):
        return "dwconv3x3"
    return "dwconv_generic"


def dwconv2d_nhwc(x: torch.Tensor, w_taps_c: torch.Tensor, bias: torch.Tensor | None = None, stride=(1, 1),
                  pad=(0, 0, 0, 0), dilation=(1, 1), act=None, out: torch.Tensor | None = None,
                  out_channel_offset: int = 0, kernel=None, tile: int = 0) -> torch.Tensor:
    """Depthwise NHWC conv (channel multiplier 1), ``act(conv + bias)``.

    ``w_taps_c`` is ``[KH * KW, C]``, TF's ``[KH, KW, C, 1]`` filter flattened (give
    ``kernel=(KH, KW)`` unless it is square); ``pad = (top, bottom, left, right)``.  With
    ``out`` given, the result is written at channel offset ``out_channel_offset`` of it.
    ``tile`` pins the 3x3 kernel's tile (``DWCONV_TILES``) or the generic kernel
    (``DWCONV_GENERIC``): measurement and tests only."""
    a = act_code(act)
    if a not in (ACT_NONE, ACT_RELU, ACT_RELU6):
        raise ValueError("dwconv2d_nhwc: act must be none, relu or relu6")
    N, H, W, C = x.shape
    taps, C2 = w_taps_c.shape
    if kernel is None:
        k = int(round(taps ** 0.5))
        kernel = (k, k)
    KH, KW = kernel
    if KH * KW != taps or C2 != C:
        raise ValueError(f"dwconv2d_nhwc: weights {tuple(w_taps_c.shape)} do not match a {KH}x{KW} filter over {C} "
                         f"channels")
    sh, sw = stride
    pt, pb, pl, pr = pad
    dh, dw = dilation
    if not dwconv_eligible(C, KH, KW, stride, dilation) or min(pad) < 0:
        raise ValueError(f"dwconv2d_nhwc: unsupported C={C}, {KH}x{KW}, stride {stride}, dilation {dilation}, "
                         f"pad {pad}")
    Ho, Wo = conv_out_hw(H, W, KH, KW, sh, sw, pt, pl, dh, dw, pb, pr)
    if Ho < 1 or Wo < 1:
        raise ValueError("dwconv2d_nhwc: empty output")
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=x.dtype if x.is_cuda else torch.float32, device=x.device)
        out_channel_offset = 0
    if out.dim() != 4 or out.shape[:3] != (N, Ho, Wo) or out_channel_offset < 0 \
            or out_channel_offset + C > out.shape[3]:
        raise ValueError(f"dwconv2d_nhwc: out {tuple(out.shape)} cannot hold [{N},{Ho},{Wo},{C}] at "
                         f"offset {out_channel_offset}")
    if x.is_cuda:
        for t, n in ((x, "x"), (w_taps_c, "w"), (out, "out")):
            _check(t, n, device=x.device)
        if bias is not None:
            _check(bias, "bias", torch.float32, x.device)
            if bias.numel() != C:
                raise ValueError("dwconv2d_nhwc: bias must have C elements")
        if out.shape[3] % 8 or out_channel_offset % 8:
            raise ValueError("dwconv2d_nhwc: output row pitch and channel offset must be multiples of 8")
        _hip().dwconv_nhwc_bf16(x.data_ptr(), w_taps_c.data_ptr(), _ptr(bias), out.data_ptr(), N, H, W, C, Ho, Wo,
                                KH, KW, sh, sw, dh, dw, pt, pl, a, out.shape[3], out_channel_offset, tile, _stream())
        return out
    xn = F.pad(x.float().permute(0, 3, 1, 2), (pl, pr, pt, pb))
    wn = w_taps_c.float().reshape(KH, KW, C).permute(2, 0, 1).unsqueeze(1)  # [C, 1, KH, KW]
    y = F.conv2d(xn, wn, stride=(sh, sw), dilation=(dh, dw), groups=C)
    if bias is not None:
        y = y + bias.float().view(1, -1, 1, 1)
    y = _apply_act_ref(y, a)
    out[..., out_channel_offset:out_channel_offset + C] = y.permute(0, 2, 3, 1).to(out.dtype)
    return out


# ------------------------------------------------------------------------------ transposed conv
# tile configurations of ``deconv_nhwc_bf16`` (kernels/deconv.hip); -1 = the launcher's choice
DECONV_TILES = {"128x128": 0, "256x64": 1}


def deconv_eligible(Cin: int, Cout: int, KH: int, KW: int, stride=(2, 2)) -> bool:
    """What ``deconv_nhwc_bf16`` takes: 8-channel vectors on both sides, a filter of at most
    8x8, strides 1..4 per axis."""
    return (Cin > 0 and Cin % 8 == 0 and Cout > 0 and Cout % 8 == 0 and 1 <= KH <= 8 and 1 <= KW <= 8
            and len(stride) == 2 and all(1 <= s <= 4 for s in stride))


def _deconv_pads(pad) -> tuple[int, int]:
    """(top, left) of ``pad = (top, bottom, left, right)`` or ``(top, left)``; the far sides are
    implied by the output size."""
    return (int(pad[0]), int(pad[2])) if len(pad) == 4 else (int(pad[0]), int(pad[1]))


def deconv_phases(kernel, stride, pad, Cin: int = 1, Cout: int = 1) -> list[dict]:
    """The per-phase table of a transposed conv, in packing order (``py * sw + px``): ``taps`` is
    the list of ``(ky, kx, dy, dx)`` with ``ky = (py + pt) mod sh`` and ``kx = (px + pl) mod sw``, in
    (ky, kx) order, read at input pixel ``(qy + dy, qx + dx)``; ``k`` the K extent ``len(taps) * Cin``; ``offset`` the
    element offset of the phase's ``[Cout, k]`` matrix in the packed tensor."""
    (KH, KW), (sh, sw), (pt, pl) = kernel, stride, _deconv_pads(pad)
    out, off = [], 0
    for py in range(sh):
        for px in range(sw):
            taps = [(ky, kx, (py + pt - ky) // sh, (px + pl - kx) // sw)
                    for ky in range(KH) if (py + pt - ky) % sh == 0
                    for kx in range(KW) if (px + pl - kx) % sw == 0]
            out.append({"py": py, "px": px, "taps": taps, "k": len(taps) * Cin, "offset": off})
            off += len(taps) * Cin * Cout
    return out


def deconv_pack_weights(w: torch.Tensor, stride, pad) -> torch.Tensor:
    """TF's ``[KH, KW, Cout, Cin]`` filter as the flat tensor the kernel reads: phase-major, per
    phase ``[Cout, taps * Cin]`` with K-contiguous rows (``deconv_phases``).  Same dtype and
    device as ``w``; ``KH * KW * Cout * Cin`` elements, since every tap is in exactly one phase."""
    KH, KW, Cout, Cin = w.shape
    parts = []
    for ph in deconv_phases((KH, KW), stride, pad, Cin, Cout):
        if ph["taps"]:
            parts.append(torch.stack([w[ky, kx] for ky, kx, _, _ in ph["taps"]], dim=1).reshape(-1))
    return torch.cat(parts).contiguous()


def deconv_unpack_weights(w_packed: torch.Tensor, kernel, stride, pad, Cin: int, Cout: int) -> torch.Tensor:
    """Inverse of ``deconv_pack_weights``: the ``[KH, KW, Cout, Cin]`` filter."""
    KH, KW = kernel
    w = torch.zeros((KH, KW, Cout, Cin), dtype=w_packed.dtype, device=w_packed.device)
    for ph in deconv_phases(kernel, stride, pad, Cin, Cout):
        m = w_packed[ph["offset"]:ph["offset"] + Cout * ph["k"]].reshape(Cout, len(ph["taps"]), Cin)
        for t, (ky, kx, _, _) in enumerate(ph["taps"]):
            w[ky, kx] = m[:, t]
    return w


def deconv2d_nhwc(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor | None, out_hw, kernel, stride=(2, 2),
                  pad=(0, 0, 0, 0), act=None, out: torch.Tensor | None = None, out_channel_offset: int = 0,
                  cfg: int = -1) -> torch.Tensor:
    """Transposed NHWC conv ``act(deconv(x, w) + bias)`` to ``out_hw = (Ho, Wo)``:
    ``y[n, oy, ox, co] = sum x[n, iy, ix, ci] w[ky, kx, co, ci]`` over ``oy + pt - ky == iy * sh``.

    ``w_packed`` comes from ``deconv_pack_weights`` (its length gives ``Cout``); ``pad`` is
    ``(top, bottom, left, right)`` of the forward conv, of which top and left are used.  With
    ``out`` given, the result is written at channel offset ``out_channel_offset`` of it.
    ``cfg`` pins a tile configuration (``DECONV_TILES``): measurement and tests only."""
    a = act_code(act)
    if a not in (ACT_NONE, ACT_RELU, ACT_RELU6):
        raise ValueError("deconv2d_nhwc: act must be none, relu or relu6")
    if x.dim() != 4 or w_packed.dim() != 1:
        raise ValueError("deconv2d_nhwc: x must be [N, Hi, Wi, Cin] and w_packed flat")
    N, Hi, Wi, Cin = x.shape
    (KH, KW), (sh, sw), (Ho, Wo) = (int(v) for v in kernel), (int(v) for v in stride), (int(v) for v in out_hw)
    pt, pl = _deconv_pads(pad)
    taps = KH * KW
    if min(N, Hi, Wi, Cin, taps) < 1 or w_packed.numel() % (taps * Cin) or w_packed.numel() == 0:
        raise ValueError(f"deconv2d_nhwc: {w_packed.numel()} packed weights do not match a {KH}x{KW} filter over "
                         f"{Cin} input channels")
    Cout = w_packed.numel() // (taps * Cin)
    if not deconv_eligible(Cin, Cout, KH, KW, (sh, sw)) or not (0 <= pt < KH and 0 <= pl < KW):
        raise ValueError(f"deconv2d_nhwc: unsupported Cin={Cin}, Cout={Cout}, {KH}x{KW}, stride {(sh, sw)}, "
                         f"pad {(pt, pl)}")
    if Ho < 1 or Wo < 1:
        raise ValueError("deconv2d_nhwc: empty output")
    if cfg not in (-1, *DECONV_TILES.values()):
        raise ValueError(f"deconv2d_nhwc: unknown tile configuration {cfg}")
    if out is None:
        out = torch.empty((N, Ho, Wo, Cout), dtype=x.dtype if x.is_cuda else torch.float32, device=x.device)
        out_channel_offset = 0
    if out.dim() != 4 or out.shape[:3] != (N, Ho, Wo) or out_channel_offset < 0 \
            or out_channel_offset + Cout > out.shape[3]:
        raise ValueError(f"deconv2d_nhwc: out {tuple(out.shape)} cannot hold [{N},{Ho},{Wo},{Cout}] at "
                         f"offset {out_channel_offset}")
    if bias is not None and bias.numel() != Cout:
        raise ValueError("deconv2d_nhwc: bias must have Cout elements")
    if x.is_cuda:
        for t, n in ((x, "x"), (w_packed, "w_packed"), (out, "out")):
            _check(t, n, device=x.device)
        if bias is not None:
            _check(bias, "bias", torch.float32, x.device)
        else:
            bias = _zeros_bias(Cout, x.device)
        if out.shape[3] % 8 or out_channel_offset % 8:
            raise ValueError("deconv2d_nhwc: output row pitch and channel offset must be multiples of 8")
        _hip().deconv_nhwc_bf16(x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr(), N, Hi, Wi, Cin,
                                Ho, Wo, Cout, KH, KW, sh, sw, pt, pl, a, out.shape[3], out_channel_offset,
                                w_packed.numel(), cfg, _stream())
        return out
    # host reference, phase by phase from the packed layout, as the kernel walks it
    xf = x.float()
    y = torch.zeros((N, Ho, Wo, Cout), dtype=torch.float32)
    for ph in deconv_phases((KH, KW), (sh, sw), (pt, pl), Cin, Cout):
        sub = y[:, ph["py"]::sh, ph["px"]::sw]
        Hq, Wq = sub.shape[1:3]
        m = w_packed[ph["offset"]:ph["offset"] + Cout * ph["k"]].float().reshape(Cout, len(ph["taps"]), Cin)
        for t, (_, _, dy, dx) in enumerate(ph["taps"]):
            # output (qy, qx) of the phase reads input (qy + dy, qx + dx) where that is inside x
            q0, q1 = max(0, -dy), min(Hq, Hi - dy)
            r0, r1 = max(0, -dx), min(Wq, Wi - dx)
            if q0 < q1 and r0 < r1:
                sub[:, q0:q1, r0:r1] += xf[:, q0 + dy:q1 + dy, r0 + dx:r1 + dx] @ m[:, t].t()
    if bias is not None:
        y = y + bias.float()
    y = _apply_act_ref(y, a)
    out[..., out_channel_offset:out_channel_offset + Cout] = y.to(out.dtype)
    return out


# ------------------------------------------------------------------------------ 3-D conv / 3-D pooling
# tile configurations of ``conv3d_ndhwc_bf16`` (kernels/conv3d.hip); -1 = the launcher's choice
CONV3D_TILES = {"128x128": 0, "256x64": 1}


def conv3d_eligible(Cin: int, Cout: int, kernel, stride, dilation=(1, 1, 1)) -> bool:
    """What ``conv3d_ndhwc_bf16`` takes: 8-channel vectors on both sides, filter extents 1..7,
    strides 1..4, no dilation."""
    return (Cin > 0 and Cin % 8 == 0 and Cout > 0 and Cout % 8 == 0 and len(kernel) == 3 and len(stride) == 3
            and all(1 <= k <= 7 for k in kernel) and all(1 <= s <= 4 for s in stride) and tuple(dilation) == (1, 1, 1))


def conv3d_pack_weights(w: torch.Tensor) -> torch.Tensor:
    """TF's ``[KD, KH, KW, Cin, Cout]`` filter as the ``[Cout, KD * KH * KW * Cin]`` matrix the
    kernel reads: K-contiguous rows, taps in (kd, kh, kw) order.  Same dtype and device as ``w``."""
    KD, KH, KW, Cin, Cout = w.shape
    return w.permute(4, 0, 1, 2, 3).reshape(Cout, KD * KH * KW * Cin).contiguous()


def conv3d_unpack_weights(w_packed: torch.Tensor, kernel, Cin: int) -> torch.Tensor:
    """Inverse of ``conv3d_pack_weights``: the ``[KD, KH, KW, Cin, Cout]`` filter."""
    KD, KH, KW = kernel
    return w_packed.reshape(w_packed.shape[0], KD, KH, KW, Cin).permute(1, 2, 3, 4, 0).contiguous()


def _out3d(name: str, ext, k, s, pad):
    """Output extents of a window ``k`` / stride ``s`` over ``ext`` with the six ``pad`` values
    (front, back, top, bottom, left, right)."""
    if len(pad) != 6 or min(pad) < 0:
        raise ValueError(f"{name}: pad must be six non-negative values (front, back, top, bottom, left, right)")
    return tuple((ext[a] + pad[2 * a] + pad[2 * a + 1] - k[a]) // s[a] + 1 for a in range(3))


def _out3d_target(name, x, out, out_channel_offset, N, O, C):
    """The output tensor of a 3-D launcher and its channel offset, checked."""
    if out is None:
        out = torch.empty((N, *O, C), dtype=x.dtype if x.is_cuda else torch.float32, device=x.device)
        out_channel_offset = 0
    if out.dim() != 5 or tuple(out.shape[:4]) != (N, *O) or out_channel_offset < 0 or out_channel_offset + C > out.shape[4]:
        raise ValueError(f"{name}: out {tuple(out.shape)} cannot hold [{N},{O[0]},{O[1]},{O[2]},{C}] at offset "
                         f"{out_channel_offset}")
    if x.is_cuda and (out.shape[4] % 8 or out_channel_offset % 8):
        raise ValueError(f"{name}: output row pitch and channel offset must be multiples of 8")
    return out, out_channel_offset


def conv3d_ndhwc(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor | None, kernel, stride=(1, 1, 1),
                 pad=(0, 0, 0, 0, 0, 0), act=None, out: torch.Tensor | None = None, out_channel_offset: int = 0,
                 cfg: int = -1) -> torch.Tensor:
    """NDHWC 3-D conv ``act(conv3d(x, w) + bias)``: ``y[n, od, oh, ow, co] = sum x[n, od sd + kd - pf,
    oh sh + kh - pt, ow sw + kw - pl, ci] w[co, (kd, kh, kw), ci]`` over the taps inside ``x``.

    ``w_packed`` is ``[Cout, KD * KH * KW * Cin]`` from ``conv3d_pack_weights``; ``pad`` is (front,
    back, top, bottom, left, right).  With ``out`` given, the result is written at channel offset
    ``out_channel_offset`` of it.  ``cfg`` pins a tile configuration (``CONV3D_TILES``):
    measurement and tests only."""
    a = act_code(act)
    if a not in (ACT_NONE, ACT_RELU, ACT_RELU6):
        raise ValueError("conv3d_ndhwc: act must be none, relu or relu6")
    if x.dim() != 5 or w_packed.dim() != 2:
        raise ValueError("conv3d_ndhwc: x must be [N, D, H, W, Cin] and w_packed [Cout, K]")
    N, D, H, W, Cin = x.shape
    k, s = tuple(int(v) for v in kernel), tuple(int(v) for v in stride)
    pad = tuple(int(v) for v in pad)
    if len(k) != 3 or len(s) != 3 or min(k) < 1:
        raise ValueError("conv3d_ndhwc: kernel and stride are (depth, height, width) triples")
    Cout, taps = w_packed.shape[0], k[0] * k[1] * k[2]
    if min(N, D, H, W, Cin) < 1 or w_packed.shape[1] != taps * Cin:
        raise ValueError(f"conv3d_ndhwc: packed weights {tuple(w_packed.shape)} do not match a {k} filter over {Cin} "
                         "input channels")
    if not conv3d_eligible(Cin, Cout, k, s):
        raise ValueError(f"conv3d_ndhwc: unsupported Cin={Cin}, Cout={Cout}, filter {k}, stride {s}")
    O = _out3d("conv3d_ndhwc", (D, H, W), k, s, pad)
    if any(pad[2 * i] >= k[i] for i in range(3)):
        raise ValueError(f"conv3d_ndhwc: pads {pad} must be below the filter size {k}")
    if min(O) < 1:
        raise ValueError("conv3d_ndhwc: empty output")
    if N * O[0] * O[1] * O[2] >= 2 ** 31:
        raise ValueError("conv3d_ndhwc: more than 2^31 output pixels")
    if cfg not in (-1, *CONV3D_TILES.values()):
        raise ValueError(f"conv3d_ndhwc: unknown tile configuration {cfg}")
    out, out_channel_offset = _out3d_target("conv3d_ndhwc", x, out, out_channel_offset, N, O, Cout)
    if bias is not None and bias.numel() != Cout:
        raise ValueError("conv3d_ndhwc: bias must have Cout elements")
    if x.is_cuda:
        for t, n in ((x, "x"), (w_packed, "w_packed"), (out, "out")):
            _check(t, n, device=x.device)
        if bias is not None:
            _check(bias, "bias", torch.float32, x.device)
        else:
            bias = _zeros_bias(Cout, x.device)
        _hip().conv3d_ndhwc_bf16(x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr(), N, D, H, W, Cin,
                                 *O, Cout, *k, *s, pad[0], pad[2], pad[4], a, out.shape[4], out_channel_offset,
                                 w_packed.numel(), cfg, _stream())
        return out
    # host reference, tap by tap from the packed layout, as the kernel walks it
    xf = x.float()
    wm = w_packed.float().reshape(Cout, taps, Cin)
    y = torch.zeros((N, *O, Cout), dtype=torch.float32)
    ext = (D, H, W)
    t = 0
    for kd in range(k[0]):
        for kh in range(k[1]):
            for kw in range(k[2]):
                # output o of an axis reads input o * s + tap - pad where that is inside x
                rng = []
                for ax, tap in enumerate((kd, kh, kw)):
                    off = tap - pad[2 * ax]
                    lo = max(0, -(off // s[ax]))
                    hi = min(O[ax], (ext[ax] - 1 - off) // s[ax] + 1)
                    rng.append((lo, hi, off))
                if all(lo < hi for lo, hi, _ in rng):
                    (d0, d1, do), (h0, h1, ho), (w0, w1, wo) = rng
                    xs = xf[:, d0 * s[0] + do:(d1 - 1) * s[0] + do + 1:s[0], h0 * s[1] + ho:(h1 - 1) * s[1] + ho + 1:s[1],
                            w0 * s[2] + wo:(w1 - 1) * s[2] + wo + 1:s[2]]
                    y[:, d0:d1, h0:h1, w0:w1] += xs @ wm[:, t].t()
                t += 1
    if bias is not None:
        y = y + bias.float()
    y = _apply_act_ref(y, a)
    out[..., out_channel_offset:out_channel_offset + Cout] = y.to(out.dtype)
    return out


def pool3d_eligible(C: int, ksize, stride) -> bool:
    """What ``pool3d_ndhwc_bf16`` takes: 8-channel vectors, window extents and strides 1..8."""
    return (C > 0 and C % 8 == 0 and len(ksize) == 3 and len(stride) == 3 and all(1 <= k <= 8 for k in ksize)
            and all(1 <= s <= 8 for s in stride))


def pool3d_ndhwc(x: torch.Tensor, ksize, stride, pad=(0, 0, 0, 0, 0, 0), mode: str = "max",
                 out: torch.Tensor | None = None, out_channel_offset: int = 0) -> torch.Tensor:
    """NDHWC 3-D max / average pooling; ``pad`` is (front, back, top, bottom, left, right).
    Window elements outside ``x`` take no part: they never win a max, and an average divides by
    the number of elements inside.  With ``out`` given, the result is written at channel offset
    ``out_channel_offset`` of it."""
    if mode not in ("max", "avg"):
        raise ValueError("pool3d_ndhwc: mode must be max or avg")
    if x.dim() != 5:
        raise ValueError("pool3d_ndhwc: x must be [N, D, H, W, C]")
    N, D, H, W, C = x.shape
    k, s = tuple(int(v) for v in ksize), tuple(int(v) for v in stride)
    pad = tuple(int(v) for v in pad)
    if min(N, D, H, W, C) < 1 or not pool3d_eligible(C, k, s):
        raise ValueError(f"pool3d_ndhwc: unsupported C={C}, window {k}, stride {s}")
    O = _out3d("pool3d_ndhwc", (D, H, W), k, s, pad)
    if any(pad[2 * i] >= k[i] for i in range(3)):
        raise ValueError(f"pool3d_ndhwc: pads {pad} must be below the window size {k}")
    if min(O) < 1:
        raise ValueError("pool3d_ndhwc: empty output")
    if any((O[i] - 1) * s[i] - pad[2 * i] >= (D, H, W)[i] for i in range(3)):
        raise ValueError("pool3d_ndhwc: a window lies outside the input")
    out, out_channel_offset = _out3d_target("pool3d_ndhwc", x, out, out_channel_offset, N, O, C)
    if x.is_cuda:
        _check(x, "x", device=x.device)
        _check(out, "out", device=x.device)
        _hip().pool3d_ndhwc_bf16(x.data_ptr(), out.data_ptr(), N, D, H, W, C, *O, *k, *s, pad[0], pad[2], pad[4],
                                 1 if mode == "avg" else 0, out.shape[4], out_channel_offset, _stream())
        return out
    # host reference: window element by window element, outside elements predicated out
    xf = x.float()
    acc = torch.full((N, *O, C), float("-inf") if mode == "max" else 0.0)
    cnt = torch.zeros((1, *O, 1))
    ext = (D, H, W)
    for i in range(k[0]):
        for j in range(k[1]):
            for l in range(k[2]):
                rng = []
                for ax, tap in enumerate((i, j, l)):
                    off = tap - pad[2 * ax]
                    rng.append((max(0, -(off // s[ax])), min(O[ax], (ext[ax] - 1 - off) // s[ax] + 1), off))
                if not all(lo < hi for lo, hi, _ in rng):
                    continue
                (d0, d1, do), (h0, h1, ho), (w0, w1, wo) = rng
                xs = xf[:, d0 * s[0] + do:(d1 - 1) * s[0] + do + 1:s[0], h0 * s[1] + ho:(h1 - 1) * s[1] + ho + 1:s[1],
                        w0 * s[2] + wo:(w1 - 1) * s[2] + wo + 1:s[2]]
                sub = acc[:, d0:d1, h0:h1, w0:w1]
                if mode == "max":
                    torch.maximum(sub, xs, out=sub)
                else:
                    sub += xs
                    cnt[:, d0:d1, h0:h1, w0:w1] += 1
    y = acc / cnt if mode == "avg" else acc
    out[..., out_channel_offset:out_channel_offset + C] = y.to(out.dtype)
    return out


# ------------------------------------------------------------------------------ bilinear resize / ArgMax
# kernel of ``resize_argmax_nhwc`` (kernels/resize.hip); 0 = the launcher's choice
RESIZE_ARGMAX_PATHS = {"staged": 1, "simple": -1}
_LABEL_BYTES = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}


def _resize_args(name: str, x: torch.Tensor, out_hw, channels):
    if x.dim() != 4:
        raise ValueError(f"{name}: x must be [N, H, W, C], got {tuple(x.shape)}")
    N, H, W, ldx = x.shape
    C = ldx if channels is None else int(channels)
    Ho, Wo = (H, W) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    if min(N, H, W, ldx) < 1 or Ho < 1 or Wo < 1:
        raise ValueError(f"{name}: empty input {tuple(x.shape)} or output {(Ho, Wo)}")
    if ldx % 8:
        raise ValueError(f"{name}: the pixel pitch {ldx} of x must be a multiple of 8")
    if not 1 <= C <= ldx:
        raise ValueError(f"{name}: channels={C} outside 1..{ldx}")
    return N, H, W, ldx, C, Ho, Wo


def resize_bilinear_nhwc(x: torch.Tensor, out_hw, align_corners: bool = False, half_pixel_centers: bool = False,
                         out: torch.Tensor | None = None, out_channel_offset: int = 0,
                         channels: int | None = None) -> torch.Tensor:
    """TF ``ResizeBilinear`` of an NHWC activation (``graph/ops_nn.py:resize_bilinear_tf`` is
    the definition): fp32 lerps, one rounding.  ``channels`` is the logical ``C`` when
    ``x.shape[-1]`` is a padded pitch.  With ``out`` given, the ``C`` result channels are
    written at channel offset ``out_channel_offset`` of it (a concat slot)."""
    N, H, W, ldx, C, Ho, Wo = _resize_args("resize_bilinear_nhwc", x, out_hw, channels)
    if C % 8:
        raise ValueError(f"resize_bilinear_nhwc: C={C} must be a multiple of 8")
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
        out_channel_offset = 0
    if out.dim() != 4 or tuple(out.shape[:3]) != (N, Ho, Wo) or out_channel_offset < 0 \
            or out_channel_offset + C > out.shape[3]:
        raise ValueError(f"resize_bilinear_nhwc: out {tuple(out.shape)} cannot hold [{N},{Ho},{Wo},{C}] at "
                         f"offset {out_channel_offset}")
    if out.shape[3] % 8 or out_channel_offset % 8:
        raise ValueError("resize_bilinear_nhwc: output row pitch and channel offset must be multiples of 8")
    if x.is_cuda:
        _check(x, "x", device=x.device)
        _check(out, "out", device=x.device)
        _hip().resize_bilinear_nhwc_bf16(x.data_ptr(), out.data_ptr(), N, H, W, C, Ho, Wo, ldx, out.shape[3],
                                         out_channel_offset, bool(align_corners), bool(half_pixel_centers), _stream())
        return out
    from ..graph.ops_nn import resize_bilinear_tf

    y = resize_bilinear_tf(x[..., :C], Ho, Wo, align_corners, half_pixel_centers)
    out[..., out_channel_offset:out_channel_offset + C] = y.to(out.dtype)
    return out


def resize_argmax_nhwc(x: torch.Tensor, out_hw=None, align_corners: bool = False, half_pixel_centers: bool = False,
                       channels: int | None = None, out: torch.Tensor | None = None, out_dtype=torch.int32,
                       path: int = 0) -> torch.Tensor:
    """Channel ArgMax of the bilinearly resized logits ``x`` ``[N, H, W, ldx]`` as a
    ``[N, Ho, Wo]`` label map (uint8, int32 or int64); the resized tensor is never stored.
    ``channels`` is the logical ``C <= 256`` when ``x.shape[-1]`` is a padded pitch: the
    padding columns are ignored.  Values are interpolated and compared in fp32, ties go to
    the lowest channel.  Without ``out_hw`` it is a plain ArgMax over the last axis.
    ``path`` pins the kernel (``RESIZE_ARGMAX_PATHS``): measurement and tests only."""
    N, H, W, ldx, C, Ho, Wo = _resize_args("resize_argmax_nhwc", x, out_hw, channels)
    if C > 256:
        raise ValueError(f"resize_argmax_nhwc: C={C} exceeds 256")
    if out is not None:
        out_dtype = out.dtype
    if out_dtype not in _LABEL_BYTES:
        raise TypeError(f"resize_argmax_nhwc: labels are uint8, int32 or int64, not {out_dtype}")
    if path not in (0, 1, -1):
        raise ValueError(f"resize_argmax_nhwc: path {path!r} is not one of 0, 1, -1")
    if out is None:
        out = torch.empty((N, Ho, Wo), dtype=out_dtype, device=x.device)
    if tuple(out.shape) != (N, Ho, Wo):
        raise ValueError(f"resize_argmax_nhwc: out {tuple(out.shape)} is not [{N},{Ho},{Wo}]")
    if x.is_cuda:
        _check(x, "x", device=x.device)
        _check(out, "out", out_dtype, x.device)
        _hip().resize_argmax_nhwc_bf16(x.data_ptr(), out.data_ptr(), N, H, W, C, Ho, Wo, ldx, _LABEL_BYTES[out_dtype],
                                       bool(align_corners), bool(half_pixel_centers), path, _stream())
        return out
    from ..graph.ops_nn import resize_bilinear_tf

    y = resize_bilinear_tf(x[..., :C].float(), Ho, Wo, align_corners, half_pixel_centers)
    # the first of the largest: torch.argmax does not promise which of several it returns
    first = torch.where(y == y.amax(-1, keepdim=True), torch.arange(C), C).amin(-1)
    out.copy_(first.to(out.dtype))
    return out


# ------------------------------------------------------------------------------ generators: instance norm, pad, image out
_IN_ACTS = (ACT_NONE, ACT_RELU, ACT_RELU6)
_IN_THREADS, _IN_PT = 256, 8  # kernels/instnorm.hip: threads per workgroup, pixels a thread holds
PAD_MODES = {"constant": 0, "reflect": 1, "symmetric": 2}
IMAGE_OUT_ACTS = {None: 0, "none": 0, "tanh": 1, "sigmoid": 2}


def instance_norm_eligible(H: int, W: int, C: int) -> bool:
    """What ``instance_norm`` takes (the lowering asks before it emits an ``instnorm`` step)."""
    return C >= 8 and C % 8 == 0 and H >= 1 and W >= 1


def _in_chunks(H: int, W: int, C: int) -> int:
    rows = _IN_THREADS // min(C // 8, _IN_THREADS)
    return -(-(H * W) // (rows * _IN_PT))


def instance_norm_scratch_numel(N: int, H: int, W: int, C: int) -> int:
    """fp32 elements of the scratch ``instance_norm`` needs: the per-chunk partials ``[N, chunks,
    C, 2]`` (mean, M2) and, behind them, the statistics ``[N, C, 2]`` (mean, gamma / sqrt(var + eps))."""
    if not instance_norm_eligible(H, W, C) or N < 1:
        raise ValueError(f"instance_norm: shape [{N},{H},{W},{C}] outside the kernel's envelope (C % 8 == 0)")
    return N * _in_chunks(H, W, C) * C * 2 + N * C * 2


def instance_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5, act=None,
                  out: torch.Tensor | None = None, out_channel_offset: int = 0,
                  scratch: torch.Tensor | None = None) -> torch.Tensor:
    """Instance normalisation of an NHWC activation: ``act((x - m) * rsqrt(v + eps) * gamma + beta)``
    with ``m`` / ``v`` the mean and the biased variance over the ``H W`` pixels of one image and
    channel.  ``x`` is bf16, the arithmetic fp32 with centred statistics, one rounding at the store.
    ``act`` is none, relu or relu6.  With ``out`` given, the ``C`` result channels are written at
    channel offset ``out_channel_offset`` of it (a concat slot).  ``scratch`` is an fp32 tensor of
    ``instance_norm_scratch_numel`` elements: a captured launch passes it, so nothing is allocated."""
    if x.dim() != 4:
        raise ValueError(f"instance_norm: x must be [N, H, W, C], got {tuple(x.shape)}")
    N, H, W, C = x.shape
    if N < 1 or not instance_norm_eligible(H, W, C):
        raise ValueError(f"instance_norm: shape {tuple(x.shape)} outside the kernel's envelope (C % 8 == 0, no empty axis)")
    a = act_code(act)
    if a not in _IN_ACTS:
        raise ValueError(f"instance_norm: activation {act!r} is not none, relu or relu6")
    if tuple(gamma.shape) != (C,) or tuple(beta.shape) != (C,):
        raise ValueError(f"instance_norm: gamma {tuple(gamma.shape)} / beta {tuple(beta.shape)} are not [{C}]")
    if gamma.dtype != torch.float32 or beta.dtype != torch.float32:
        raise TypeError(f"instance_norm: gamma / beta are fp32, not {gamma.dtype} / {beta.dtype}")
    if x.dtype != torch.bfloat16:
        raise TypeError(f"instance_norm: x is bf16, not {x.dtype}")
    if not float(eps) >= 0.0:
        raise ValueError(f"instance_norm: eps {eps!r} is negative")
    if out is None:
        out = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
        out_channel_offset = 0
    if out.dim() != 4 or tuple(out.shape[:3]) != (N, H, W) or out_channel_offset < 0 \
            or out_channel_offset + C > out.shape[3]:
        raise ValueError(f"instance_norm: out {tuple(out.shape)} cannot hold [{N},{H},{W},{C}] at offset "
                         f"{out_channel_offset}")
    if out.shape[3] % 8 or out_channel_offset % 8:
        raise ValueError("instance_norm: output row pitch and channel offset must be multiples of 8")
    if x.is_cuda:
        dev = x.device
        _check(x, "x", device=dev)
        _check(out, "out", device=dev)
        _check(gamma, "gamma", torch.float32, dev)
        _check(beta, "beta", torch.float32, dev)
        need = instance_norm_scratch_numel(N, H, W, C)
        if scratch is None:
            scratch = torch.empty(need, dtype=torch.float32, device=dev)
        _check(scratch, "scratch", torch.float32, dev)
        if scratch.numel() < need:
            raise ValueError(f"instance_norm: scratch has {scratch.numel()} fp32 elements, {need} needed")
        _hip().instance_norm_nhwc_bf16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                       scratch.data_ptr(), scratch.numel(), N, H, W, C, out.shape[3],
                                       out_channel_offset, float(eps), a, _stream())
        return out
    xf = x.float()
    m = xf.mean((1, 2), keepdim=True)
    d = xf - m
    v = (d * d).mean((1, 2), keepdim=True)
    y = _apply_act_ref(d * (gamma / torch.sqrt(v + float(eps))) + beta, a)
    out[..., out_channel_offset:out_channel_offset + C] = y.to(out.dtype)
    return out


def mirror_index(size: int, lo: int, hi: int, mode: str) -> torch.Tensor:
    """Source indices of an axis of ``size`` padded by ``lo`` / ``hi``: output ``i`` reads ``r = i -
    lo`` inside the axis, else ``-r`` / ``2 (size - 1) - r`` (reflect), ``-r - 1`` / ``2 size - 1 - r``
    (symmetric); constant mode marks the outside ``-1``."""
    r = torch.arange(-lo, size + hi)
    if mode == "reflect":
        return torch.where(r < 0, -r, torch.where(r >= size, 2 * (size - 1) - r, r))
    if mode == "symmetric":
        return torch.where(r < 0, -r - 1, torch.where(r >= size, 2 * size - 1 - r, r))
    return torch.where((r < 0) | (r >= size), -1, r)


def pad_nhwc(x: torch.Tensor, pads, mode: str = "constant", value: float = 0.0, out: torch.Tensor | None = None,
             out_channel_offset: int = 0, channels: int | None = None) -> torch.Tensor:
    """TF ``Pad`` / ``PadV2`` (``mode="constant"``) or ``MirrorPad`` (``"reflect"``, ``"symmetric"``)
    of the two spatial axes of a bf16 NHWC activation; ``pads = (top, bottom, left, right)``.  A
    reflect pad is at most ``size - 1``, a symmetric one at most ``size``.  All ``x.shape[-1]``
    physical channels are copied; ``channels`` is the logical ``C`` of a channel-padded ``x``: a
    constant fill writes ``value`` to those and zero to the padding.  With ``out`` given the result is
    written at channel offset ``out_channel_offset`` of it (a concat slot)."""
    if x.dim() != 4:
        raise ValueError(f"pad_nhwc: x must be [N, H, W, C], got {tuple(x.shape)}")
    if mode not in PAD_MODES:
        raise ValueError(f"pad_nhwc: mode {mode!r} is not one of {sorted(PAD_MODES)}")
    if x.dtype != torch.bfloat16:
        raise TypeError(f"pad_nhwc: x is bf16, not {x.dtype}")
    N, H, W, C = x.shape
    Cl = C if channels is None else int(channels)
    if len(pads) != 4 or any(int(p) != p or p < 0 for p in pads):
        raise ValueError(f"pad_nhwc: pads {pads!r} are not four non-negative integers (top, bottom, left, right)")
    pt, pb, pl, pr = (int(p) for p in pads)
    if min(N, H, W, C) < 1 or C % 8 or not 1 <= Cl <= C:
        raise ValueError(f"pad_nhwc: shape {tuple(x.shape)} (channels={Cl}) needs C % 8 == 0 and no empty axis")
    if mode != "constant":
        lim = 1 if mode == "reflect" else 0
        for axis, size, lo, hi in ((1, H, pt, pb), (2, W, pl, pr)):
            if max(lo, hi) > size - lim:
                raise ValueError(f"pad_nhwc: {mode} pad ({lo}, {hi}) of axis {axis} exceeds {size - lim}")
    Ho, Wo = H + pt + pb, W + pl + pr
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
        out_channel_offset = 0
    if out.dim() != 4 or tuple(out.shape[:3]) != (N, Ho, Wo) or out_channel_offset < 0 \
            or out_channel_offset + C > out.shape[3]:
        raise ValueError(f"pad_nhwc: out {tuple(out.shape)} cannot hold [{N},{Ho},{Wo},{C}] at offset "
                         f"{out_channel_offset}")
    if out.shape[3] % 8 or out_channel_offset % 8:
        raise ValueError("pad_nhwc: output row pitch and channel offset must be multiples of 8")
    if x.is_cuda:
        _check(x, "x", device=x.device)
        _check(out, "out", device=x.device)
        _hip().pad_nhwc_bf16(x.data_ptr(), out.data_ptr(), N, H, W, C, Cl, pt, pb, pl, pr, PAD_MODES[mode],
                             float(value), C, out.shape[3], out_channel_offset, _stream())
        return out
    iy, ix = mirror_index(H, pt, pb, mode), mirror_index(W, pl, pr, mode)
    y = x[:, iy.clamp(min=0)][:, :, ix.clamp(min=0)]
    if mode == "constant":
        fill = torch.zeros(C, dtype=x.dtype)
        fill[:Cl] = torch.tensor(float(value)).to(x.dtype)
        outside = (iy < 0)[:, None] | (ix < 0)[None, :]
        y = torch.where(outside[None, :, :, None], fill, y)
    out[..., out_channel_offset:out_channel_offset + C] = y
    return out


def image_out(x: torch.Tensor, channels: int, act=None, scale: float = 1.0, offset: float = 0.0, clamp=None,
              dtype=torch.float32, out: torch.Tensor | None = None) -> torch.Tensor:
    """The output stage of a generator: ``clamp(act(x[..., :channels]) * scale + offset)`` of a bf16
    NHWC buffer (``x.shape[-1]`` its physical channels) as a compact ``[N, H, W, channels]`` fp32 or
    uint8 image.  ``channels`` is 1, 3 or 4, ``act`` none / tanh / sigmoid, ``clamp`` None or ``(lo,
    hi)``.  fp32 arithmetic, every operation rounded on its own; uint8 truncates after the clamp
    (TF's ``Cast``) and needs a clamp inside ``[0, 255]``."""
    if x.dim() != 4:
        raise ValueError(f"image_out: x must be [N, H, W, C], got {tuple(x.shape)}")
    if x.dtype != torch.bfloat16:
        raise TypeError(f"image_out: x is bf16, not {x.dtype}")
    N, H, W, ldx = x.shape
    Cl = int(channels)
    if Cl not in (1, 3, 4):
        raise ValueError(f"image_out: channels={channels!r} is not 1, 3 or 4")
    if min(N, H, W) < 1 or ldx % 8 or ldx < Cl:
        raise ValueError(f"image_out: x {tuple(x.shape)} needs a pixel pitch that is a multiple of 8 and no empty axis")
    if act not in IMAGE_OUT_ACTS:
        raise ValueError(f"image_out: activation {act!r} is not none, tanh or sigmoid")
    if out is not None:
        dtype = out.dtype
    if dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"image_out: the image is fp32 or uint8, not {dtype}")
    if clamp is not None:
        lo, hi = (float(v) for v in clamp)
        if not lo <= hi:
            raise ValueError(f"image_out: clamp {clamp!r} is empty")
    if dtype == torch.uint8 and (clamp is None or lo < 0.0 or hi > 255.0):
        raise ValueError("image_out: a uint8 image needs a clamp inside [0, 255]")
    if out is None:
        out = torch.empty((N, H, W, Cl), dtype=dtype, device=x.device)
    if tuple(out.shape) != (N, H, W, Cl):
        raise ValueError(f"image_out: out {tuple(out.shape)} is not [{N},{H},{W},{Cl}]")
    if x.is_cuda:
        _check(x, "x", device=x.device)
        _check(out, "out", dtype, x.device)
        _hip().image_out_bf16(x.data_ptr(), out.data_ptr(), N * H * W, ldx, Cl, IMAGE_OUT_ACTS[act], float(scale),
                              float(offset), clamp is not None, lo if clamp is not None else 0.0,
                              hi if clamp is not None else 0.0, 1 if dtype == torch.uint8 else 4, _stream())
        return out
    v = x[..., :Cl].float()
    v = torch.tanh(v) if IMAGE_OUT_ACTS[act] == 1 else torch.sigmoid(v) if IMAGE_OUT_ACTS[act] == 2 else v
    v = v * torch.tensor(float(scale), dtype=torch.float32) + torch.tensor(float(offset), dtype=torch.float32)
    if clamp is not None:
        v = v.clamp(lo, hi)
    out.copy_(v.to(dtype))  # uint8: truncation, as TF's Cast
    return out


# ------------------------------------------------------------------------------ detection: box decode + NMS
# The envelope of ``kernels/detection.hip``, from its LDS budget (160 KiB per CU).  The
# per-class kernel sorts ``N`` rounded up to a power of two 8-byte keys (at most 4096 * 8 B =
# 32 KiB) and keeps ``max_per_class`` canonical boxes with their areas (at most 256 * 20 B =
# 5 KiB): dynamic LDS sized per launch, always under 64 KiB, so no function attribute has to be
# set (18 KiB for an SSD's N = 1917 and 100 per class: eight workgroups per CU).  The merge
# kernel gives every class one of its 256 threads and stages 16 keys per class (32 KiB) next
# to the ``max_total`` merged keys (1024 * 8 B = 8 KiB), static.  Class and box index travel in
# 16 bits each of a kept key.  Per-class boxes (q = C) have no kernel.
NMS_MAX_BOXES = 4096
NMS_MAX_CLASSES = 256
NMS_MAX_PER_CLASS = 256
NMS_MAX_TOTAL = 1024


def nms_eligible(N: int, C: int, max_per_class: int, max_total: int, q: int = 1) -> bool:
    """What ``combined_nms`` takes on the GPU (the lowering asks before it emits an ``nms`` step)."""
    return (q == 1 and 1 <= N <= NMS_MAX_BOXES and 1 <= C <= NMS_MAX_CLASSES
            and 1 <= max_per_class <= NMS_MAX_PER_CLASS and 1 <= max_total <= NMS_MAX_TOTAL)


def nms_scratch_numel(B: int, C: int, max_per_class: int) -> int:
    """int64 elements of the scratch ``combined_nms`` needs: the kept keys ``[B, C,
    max_per_class]`` and, behind them, the int32 kept counts ``[B, C]``."""
    return B * C * min(max_per_class, NMS_MAX_PER_CLASS) + (B * C + 1) // 2


def combined_nms(boxes: torch.Tensor, scores: torch.Tensor, max_per_class: int, max_total: int, iou_threshold: float,
                 score_threshold: float, pad_per_class: bool = False, clip_boxes: bool = True,
                 anchors: torch.Tensor | None = None, box_scales=None, num_classes: int | None = None,
                 class_offset: int = 0, out=None, scratch: torch.Tensor | None = None):
    """TF ``CombinedNonMaxSuppression`` with one box per anchor shared by the classes
    (``graph/ops_nn.py:combined_nms_host`` is the definition, ties pinned there).

    ``scores`` is ``[B, N, ld]`` bf16 or fp32; the classes are its columns ``class_offset ..
    class_offset + num_classes`` (all of them by default), read in place.  ``boxes`` is
    ``[B, N, 1, 4]`` or ``[B, N, 4]`` bf16 or fp32 corners (ymin, xmin, ymax, xmax); with
    ``anchors`` (fp32 ``[N, 4]`` = yc, xc, h, w) and ``box_scales`` (four reciprocal scale
    factors) it holds bf16 or fp32 encodings (ty, tx, th, tw) instead, decoded in fp32 inside the kernel
    (``ops_nn.decode_boxes_yxhw`` is the order of operations).  Returns ``(boxes [B, T, 4],
    scores [B, T], classes [B, T])`` fp32 and ``valid [B]`` int32, ``T = max_total`` (with
    ``pad_per_class``, ``min(max_total, max_per_class * C)``); rows past ``valid`` are zero.
    ``out`` is that tuple preallocated and ``scratch`` an int64 tensor of ``nms_scratch_numel``
    elements: a captured launch passes both, so nothing is allocated."""
    if boxes.dim() == 4 and boxes.shape[2] == 1:
        boxes = boxes[:, :, 0]
    fused = anchors is not None
    if boxes.dim() != 3 or boxes.shape[-1] != 4 or scores.dim() != 3 or tuple(boxes.shape[:2]) != tuple(scores.shape[:2]):
        raise ValueError(f"combined_nms: boxes {tuple(boxes.shape)} / scores {tuple(scores.shape)} are not "
                         "[B,N,(1,)4] / [B,N,C]")
    B, N, ld = scores.shape
    C = ld - class_offset if num_classes is None else int(num_classes)
    if class_offset < 0 or C < 1 or class_offset + C > ld:
        raise ValueError(f"combined_nms: classes {class_offset}..{class_offset + C} outside the {ld} score columns")
    mpc, T = int(max_per_class), int(max_total)
    if B < 1 or N < 1 or mpc < 1 or T < 1:
        raise ValueError("combined_nms: empty problem")
    if pad_per_class:
        T = min(T, mpc * C)
    mpc = min(mpc, N)  # selection stops at min(max_per_class, N)
    if fused:
        if box_scales is None or len(box_scales) != 4 or tuple(anchors.shape) != (N, 4):
            raise ValueError(f"combined_nms: fused decode needs anchors [{N}, 4] and four box_scales")
        box_scales = [float(v) for v in box_scales]
    if not scores.is_cuda:
        from ..graph.ops_nn import combined_nms_host, decode_boxes_yxhw

        bx = decode_boxes_yxhw(boxes, anchors, box_scales) if fused else boxes.float()
        res = combined_nms_host(bx[:, :, None], scores[..., class_offset:class_offset + C].float(), mpc, T,
                                iou_threshold, score_threshold, False, clip_boxes)
        if out is None:
            return res
        for o, r in zip(out, res):
            o.copy_(r)
        return tuple(out)
    if not nms_eligible(N, C, mpc, T):
        raise ValueError(f"combined_nms: N={N}, C={C}, max_per_class={mpc}, max_total={T} outside the kernel's "
                         f"envelope ({NMS_MAX_BOXES}, {NMS_MAX_CLASSES}, {NMS_MAX_PER_CLASS}, {NMS_MAX_TOTAL})")
    dev = scores.device
    if scores.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"combined_nms: scores are bf16 or fp32, not {scores.dtype}")
    _check(scores, "scores", scores.dtype, dev)
    if fused:
        if boxes.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"combined_nms: encodings are bf16 or fp32, not {boxes.dtype}")
        _check(boxes, "boxes (encodings)", boxes.dtype, dev)
        _check(anchors, "anchors", torch.float32, dev)
        mode = 2 if boxes.dtype == torch.bfloat16 else 3
    else:
        if boxes.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"combined_nms: boxes are bf16 or fp32, not {boxes.dtype}")
        _check(boxes, "boxes", boxes.dtype, dev)
        mode = 0 if boxes.dtype == torch.float32 else 1
        box_scales = [0.0] * 4
    if out is None:
        out = (torch.empty((B, T, 4), dtype=torch.float32, device=dev), torch.empty((B, T), dtype=torch.float32, device=dev),
               torch.empty((B, T), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
    ob, os_, oc, ov = out
    for t, name, shape, dt in ((ob, "out boxes", (B, T, 4), torch.float32), (os_, "out scores", (B, T), torch.float32),
                               (oc, "out classes", (B, T), torch.float32), (ov, "out valid", (B,), torch.int32)):
        _check(t, name, dt, dev)
        if tuple(t.shape) != shape:
            raise ValueError(f"combined_nms: {name} {tuple(t.shape)} is not {shape}")
    need = nms_scratch_numel(B, C, mpc)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.int64, device=dev)
    _check(scratch, "scratch", torch.int64, dev)
    if scratch.numel() < need:
        raise ValueError(f"combined_nms: scratch has {scratch.numel()} int64 elements, {need} needed")
    _hip().combined_nms(boxes.data_ptr(), mode, _ptr(anchors), *box_scales, scores.data_ptr(),
                        scores.dtype == torch.float32, B, N, C, ld, class_offset, mpc, T, float(iou_threshold),
                        float(score_threshold), bool(clip_boxes), scratch.data_ptr(),
                        scratch.data_ptr() + 8 * B * C * mpc, ob.data_ptr(), os_.data_ptr(), oc.data_ptr(), ov.data_ptr(),
                        _stream())
    return out


# ------------------------------------------------------------------------------ LSTM recurrence
LSTM_MAX_HIDDEN = 512
LSTM_RESIDENT_HIDDEN = 128  # up to here the recurrent weights stay in registers for all steps


def lstm_eligible(T: int, B: int, I: int, H: int) -> bool:
    """What ``lstm_seq`` (and the projection GEMM in front of it) takes on the GPU."""
    return T >= 1 and B >= 1 and I >= 8 and I % 8 == 0 and 16 <= H <= LSTM_MAX_HIDDEN and H % 16 == 0


def lstm_impl(H: int) -> str:
    """The form of ``kernels/lstm.hip`` the launcher picks for ``H`` hidden units."""
    return "lstm_resident" if H <= LSTM_RESIDENT_HIDDEN else "lstm_streamed"


def lstm_pack_weights(wh: torch.Tensor, H: int) -> torch.Tensor:
    """The recurrent weights ``wh [H, 4H]`` (gate columns i, ci, f, o: ``w[I:]`` of a
    ``BlockLSTM``) as the A fragments of ``v_mfma_f32_16x16x32_bf16`` with gate units on M:
    ``[H/16, 4, KS, 64, 8]`` bf16, ``KS = ceil(H / 32)``, where element ``e`` of lane ``l`` in
    ``[u, g, ks]`` is ``wh[32 ks + 8 (l >> 4) + e, g H + 16 u + (l & 15)]`` and rows past ``H``
    (the upper half of the last K step when ``H % 32 == 16``) are zero."""
    if wh.dim() != 2 or tuple(wh.shape) != (H, 4 * H) or H % 16 or H < 16:
        raise ValueError(f"lstm_pack_weights: weights {tuple(wh.shape)} are not [H, 4H] with H = {H} a multiple of 16")
    KS = -(-H // 32)
    w = torch.zeros((KS * 32, 4 * H), dtype=torch.bfloat16, device=wh.device)
    w[:H] = wh.to(torch.bfloat16)
    w = w.reshape(KS, 4, 8, 4, H // 16, 16)  # [ks, lane >> 4, e, gate, unit group, lane & 15]
    return w.permute(4, 3, 0, 1, 5, 2).reshape(H // 16, 4, KS, 64, 8).contiguous()


def lstm_unpack_weights(wpk: torch.Tensor) -> torch.Tensor:
    """Inverse of ``lstm_pack_weights``: ``[H, 4H]`` bf16."""
    if wpk.dim() != 5 or tuple(wpk.shape[3:]) != (64, 8) or wpk.shape[1] != 4:
        raise ValueError(f"lstm_unpack_weights: {tuple(wpk.shape)} is not [H/16, 4, KS, 64, 8]")
    G, _, KS = wpk.shape[:3]
    H = G * 16
    if KS != -(-H // 32):
        raise ValueError(f"lstm_unpack_weights: {KS} K steps do not belong to H = {H}")
    w = wpk.reshape(G, 4, KS, 4, 16, 8).permute(2, 3, 5, 1, 0, 4).reshape(KS * 32, 4 * H)
    return w[:H].contiguous()


def lstm_seq(xproj: torch.Tensor, wh_packed: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor, *,
             wci: torch.Tensor | None = None, wcf: torch.Tensor | None = None, wco: torch.Tensor | None = None,
             cell_clip: float = 3.0, steps: int | None = None, h_out: torch.Tensor | None = None,
             cs_out: torch.Tensor | None = None, c_last: torch.Tensor | None = None,
             last_only: bool = False) -> torch.Tensor:
    """The recurrence of one ``BlockLSTM`` layer in one launch (``kernels/lstm.hip``).

    ``xproj [T, B, 4H]`` bf16 is the input projection ``x . w[:I] + b`` (forget bias folded
    in), gate columns i, ci, f, o; ``wh_packed = lstm_pack_weights(w[I:], H)``; ``h0 [B, H]``
    bf16, ``c0 [B, H]`` fp32 or bf16; the peephole vectors fp32 ``[H]``, all three or none.
    ``xproj``, ``h_out`` and ``cs_out`` are addressed through their own strides for ``t`` and
    ``b`` (last axis contiguous): a batch-major buffer goes in as ``buf.transpose(0, 1)``.
    ``h_out`` is ``[T, B, H]`` bf16, or ``[B, H]`` = the hidden state after the last step with
    ``last_only``; ``cs_out [T, B, H]`` bf16 and ``c_last [B, H]`` fp32 (the cell state after
    ``steps``) are optional.  Steps ``>= steps`` (default ``T``) of the ``[T, ..]`` outputs are
    zero; ``steps == 0`` with ``last_only`` writes zeros.  ``cell_clip <= 0``: no clip.

    Rounding points, the same on both paths: ``xproj`` is bf16; ``h`` is rounded to bf16
    before it is stored and fed back; ``c`` is never rounded (``cs_out`` on store only)."""
    if xproj.dim() != 3 or xproj.shape[-1] % 4:
        raise ValueError(f"lstm_seq: xproj {tuple(xproj.shape)} is not [T, B, 4H]")
    T, B, H4 = xproj.shape
    H = H4 // 4
    if T < 1 or B < 1 or H < 16 or H > LSTM_MAX_HIDDEN or H % 16:
        raise ValueError(f"lstm_seq: T={T}, B={B}, H={H} outside the kernel's envelope (H a multiple of 16 in "
                         f"16..{LSTM_MAX_HIDDEN})")
    KS = -(-H // 32)
    if tuple(wh_packed.shape) != (H // 16, 4, KS, 64, 8):
        raise ValueError(f"lstm_seq: packed weights {tuple(wh_packed.shape)} are not {(H // 16, 4, KS, 64, 8)} "
                         "(lstm_pack_weights)")
    steps = T if steps is None else int(steps)
    if not 0 <= steps <= T:
        raise ValueError(f"lstm_seq: steps={steps} outside 0..{T}")
    dev = xproj.device
    peep = [wci, wcf, wco]
    if any(p is None for p in peep) != all(p is None for p in peep):
        raise ValueError("lstm_seq: the three peephole vectors come together")
    peep = None if wci is None else peep
    if xproj.dtype != torch.bfloat16 or xproj.stride(2) != 1:
        raise TypeError("lstm_seq: xproj must be bf16 with a contiguous last axis")
    _check(wh_packed, "wh_packed", device=dev)
    _check(h0, "h0", device=dev)
    if c0.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"lstm_seq: c0 is fp32 or bf16, not {c0.dtype}")
    _check(c0, "c0", c0.dtype, dev)
    if tuple(h0.shape) != (B, H) or tuple(c0.shape) != (B, H):
        raise ValueError(f"lstm_seq: h0 {tuple(h0.shape)} / c0 {tuple(c0.shape)} are not [{B}, {H}]")
    for p in peep or ():
        _check(p, "peephole vector", torch.float32, dev)
        if tuple(p.shape) != (H,):
            raise ValueError(f"lstm_seq: peephole vector {tuple(p.shape)} is not [{H}]")
    hshape = (B, H) if last_only else (T, B, H)
    if h_out is None:
        h_out = torch.empty(hshape, dtype=torch.bfloat16, device=dev)
    for t, name, shape, dt in ((h_out, "h_out", hshape, torch.bfloat16), (cs_out, "cs_out", (T, B, H), torch.bfloat16),
                               (c_last, "c_last", (B, H), torch.float32)):
        if t is None:
            continue
        if t.dtype != dt or t.device != dev or tuple(t.shape) != shape or t.stride(-1) != 1:
            raise ValueError(f"lstm_seq: {name} must be {dt} {shape} on {dev} with a contiguous last axis, got "
                             f"{t.dtype} {tuple(t.shape)} strides {t.stride()}")
    if c_last is not None and not c_last.is_contiguous():
        raise ValueError("lstm_seq: c_last must be contiguous")
    clip = float(cell_clip)
    if xproj.is_cuda:
        views = [("xproj", xproj), ("h_out", h_out)] + ([("cs_out", cs_out)] if cs_out is not None else [])
        for name, t in views:
            if t.data_ptr() % 16 or any(s % 8 for s in t.stride()[:-1]):
                raise ValueError(f"lstm_seq: {name} must be 16-byte aligned with row strides that are multiples of 8")
            if min(t.stride()[:-1]) < t.shape[-1]:
                raise ValueError(f"lstm_seq: {name} rows overlap (strides {t.stride()})")
        hs_t, hs_b = (0, h_out.stride(0)) if last_only else (h_out.stride(0), h_out.stride(1))
        cs_t, cs_b = (cs_out.stride(0), cs_out.stride(1)) if cs_out is not None else (0, 0)
        _hip().lstm_seq_bf16(xproj.data_ptr(), wh_packed.data_ptr(), h0.data_ptr(), c0.data_ptr(),
                             c0.dtype == torch.bfloat16, _ptr(wci), _ptr(wcf), _ptr(wco), h_out.data_ptr(), _ptr(cs_out),
                             _ptr(c_last), T, B, H, steps, xproj.stride(0), xproj.stride(1), hs_t, hs_b, cs_t, cs_b,
                             bool(last_only), clip, _stream())
        return h_out
    wh = lstm_unpack_weights(wh_packed).float()
    c, h = c0.float(), h0.float()
    if not last_only:
        h_out[steps:] = 0
    if cs_out is not None:
        cs_out[steps:] = 0
    for t in range(steps):
        gi, gc, gf, go = (xproj[t].float() + h @ wh).split(H, dim=1)
        if peep:
            gi, gf = gi + c * wci, gf + c * wcf
        c = torch.tanh(gc) * torch.sigmoid(gi) + c * torch.sigmoid(gf)
        if clip > 0:
            c = c.clamp(-clip, clip)
        if peep:
            go = go + c * wco
        h = (torch.tanh(c) * torch.sigmoid(go)).to(torch.bfloat16).float()
        if not last_only:
            h_out[t] = h.to(torch.bfloat16)
        if cs_out is not None:
            cs_out[t] = c.to(torch.bfloat16)
    if last_only:
        h_out.copy_(h.to(torch.bfloat16) if steps else torch.zeros_like(h_out))
    if c_last is not None:
        c_last.copy_(c)
    return h_out


# ------------------------------------------------------------------------------ audio front end
AUDIO_FFT_LENGTHS = (256, 512, 1024, 2048)
AUDIO_MAX_CHANNELS = 128
AUDIO_FRAMES_PER_WG = 8  # frames one workgroup of kernels/audio.hip owns (four FFTs of two frames)
_AUDIO_MODES = {"mfcc_f32": 0, "mfcc_bf16": 1, "mfcc_bf16_pad8": 2, "spec_squared": 3, "spec_magnitude": 4}


def audio_fft_length(window_size: int) -> int:
    """The smallest power of two ``>= window_size``."""
    n = 1
    while n < window_size:
        n *= 2
    return n


def audio_frames(samples: int, window_size: int, stride: int) -> int:
    return 1 + (samples - window_size) // stride if samples >= window_size else 0


@functools.lru_cache(maxsize=64)
def _audio_tables(window: int, sample_rate, lower, upper, C: int, D: int):
    from ..graph.ops_nn import mel_filterbank

    N = audio_fft_length(window)
    n = torch.arange(window, dtype=torch.float64)
    k = torch.arange(N // 2, dtype=torch.float64)
    ang = 2.0 * math.pi * k / N
    t = {"window": window, "fft": N, "C": C, "D": D,
         "hann": (0.5 - 0.5 * torch.cos(2.0 * math.pi * n / window)).float(),
         "twiddle": torch.stack([torch.cos(ang), -torch.sin(ang)], dim=1).float().contiguous()}
    if C:
        bins = N // 2 + 1
        start, end, band, weight = mel_filterbank(bins, sample_rate, lower, upper, C)
        chan = torch.zeros((C, 3), dtype=torch.int32)
        for c in range(C):
            prev = [i for i in range(start, end + 1) if band[i] == c - 1]  # they weigh in with 1 - w
            own = [i for i in range(start, end + 1) if band[i] == c]
            lo = prev[0] if prev else own[0]
            mid = own[0] if own else prev[-1] + 1
            chan[c] = torch.tensor([lo, mid, own[-1] + 1 if own else mid], dtype=torch.int32)
        w = torch.from_numpy(weight)
        j = torch.arange(C, dtype=torch.float64)
        d = torch.arange(D, dtype=torch.float64)
        t.update(chan=chan, wa=w.float(), wb=(1.0 - w).float(),
                 dct=(math.sqrt(2.0 / C) * torch.cos(d[:, None] * (math.pi / C) * (j[None, :] + 0.5))).float().contiguous())
    return t


def mfcc_tables(window_size: int, sample_rate=None, lower: float = 20.0, upper: float = 4000.0, channels: int = 0,
                dct_count: int = 0, device=None) -> dict:
    """The fp32 tables of ``kernels/audio.hip``, computed in float64: ``hann [window]`` (periodic),
    ``twiddle [N/2, 2]`` = ``(cos, -sin)(2 pi k / N)`` and, with ``channels > 0``, the mel filter
    bank of ``graph.ops_nn.mel_filterbank`` per channel: ``chan [C, 3]`` int32 = ``(lo, mid, hi)``,
    where bins ``[lo, mid)`` (those of the band below) weigh in with ``wb[i] = 1 - w_i`` and bins
    ``[mid, hi)`` with ``wa[i] = w_i``; and ``dct [D, C]``.  ``ValueError`` when a channel receives
    no bin or ``D > C``.  The CPU tables are cached; ``device`` moves a copy there."""
    window_size, channels, dct_count = int(window_size), int(channels), int(dct_count)
    if window_size < 2:
        raise ValueError(f"mfcc_tables: window_size={window_size}")
    if channels and not 1 <= dct_count <= channels:
        raise ValueError(f"mfcc_tables: dct_count={dct_count} must be in 1..channels={channels}")
    t = _audio_tables(window_size, None if not channels else float(sample_rate), float(lower), float(upper), channels,
                      dct_count if channels else 0)
    if device is None or torch.device(device).type == "cpu":
        return t
    return {k: v.to(device) if isinstance(v, torch.Tensor) else v for k, v in t.items()}


def mfcc_eligible(samples: int, window_size: int, stride: int, channels: int = 0, dct_count: int = 0, sample_rate=None,
                  lower: float = 20.0, upper: float = 4000.0) -> bool:
    """What ``kernels/audio.hip`` takes: an FFT length of 256..2048 (``window_size`` 129..2048), any
    ``stride >= 1``, at least one frame and, for the MFCC forms, ``D <= C <= 128`` with every mel
    channel non-empty.  ``channels == 0`` asks for the spectrogram alone."""
    if window_size < 2 or audio_fft_length(window_size) not in AUDIO_FFT_LENGTHS or stride < 1 \
            or audio_frames(samples, window_size, stride) < 1:
        return False
    if not channels:
        return True
    if not (1 <= dct_count <= channels <= AUDIO_MAX_CHANNELS) or sample_rate is None or sample_rate <= 0:
        return False
    try:
        mfcc_tables(window_size, sample_rate, lower, upper, channels, dct_count)
    except ValueError:
        return False
    return True


def _audio_args(name: str, x: torch.Tensor, tables: dict, stride: int, need_mfcc: bool):
    if x.dim() != 2:
        raise ValueError(f"{name}: x {tuple(x.shape)} is not [samples, clips]")
    if x.dtype not in (torch.float32, torch.int16):
        raise TypeError(f"{name}: x is fp32 or int16, not {x.dtype}")
    S, B = x.shape
    window, N = tables["window"], tables["fft"]
    if N not in AUDIO_FFT_LENGTHS or stride < 1:
        raise ValueError(f"{name}: FFT length {N} (window {window}) / stride {stride} outside the kernel's envelope")
    F_ = audio_frames(S, window, stride)
    if F_ < 1 or B < 1:
        raise ValueError(f"{name}: {S} samples hold no frame of {window}, or no clip")
    if (S > 1 and x.stride(0) < 1) or (B > 1 and x.stride(1) < 1):
        raise ValueError(f"{name}: x strides {x.stride()} must be positive")
    names = ("hann", "twiddle") + (("chan", "wa", "wb", "dct") if need_mfcc else ())
    if need_mfcc and not tables.get("C"):
        raise ValueError(f"{name}: the tables hold no filter bank (mfcc_tables with channels > 0)")
    shapes = {"hann": (window,), "twiddle": (N // 2, 2), "chan": (tables["C"], 3), "wa": (N // 2 + 1,),
              "wb": (N // 2 + 1,), "dct": (tables["D"], tables["C"])}
    for k in names:
        t = tables[k]
        _check(t, f"{name}: table {k}", torch.int32 if k == "chan" else torch.float32, x.device)
        if tuple(t.shape) != shapes[k]:
            raise ValueError(f"{name}: table {k} is {tuple(t.shape)}, not {shapes[k]}")
    return S, B, F_, window, N


def _audio_frames_host(x: torch.Tensor, tables: dict, stride: int, scale: float, F_: int) -> torch.Tensor:
    """fp32 power spectrogram ``[B, F, bins]`` on the host path."""
    window, N = tables["window"], tables["fft"]
    xf = x.float() * scale if x.dtype == torch.int16 else x
    fr = xf.t()[:, :(F_ - 1) * stride + window].unfold(1, window, stride) * tables["hann"]
    z = torch.fft.rfft(fr.contiguous(), n=N, dim=-1)
    return z.real * z.real + z.imag * z.imag


def _launch_audio(x, tables, stride, scale, out, mode, S, B):
    mf = mode.startswith("mfcc")
    _hip().audio_frontend(x.data_ptr(), x.dtype == torch.int16, float(scale), max(x.stride(0), 1), max(x.stride(1), 1), S, B,
                          tables["window"], int(stride), tables["fft"], tables["hann"].data_ptr(),
                          tables["twiddle"].data_ptr(), tables["chan"].data_ptr() if mf else 0,
                          tables["wa"].data_ptr() if mf else 0, tables["wb"].data_ptr() if mf else 0,
                          tables["dct"].data_ptr() if mf else 0, tables["C"] if mf else 0, tables["D"] if mf else 0,
                          out.data_ptr(), _AUDIO_MODES[mode], _stream())


def audio_spectrogram(x: torch.Tensor, tables: dict, stride: int, magnitude_squared: bool = True, scale: float = 1.0,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """``AudioSpectrogram`` of ``B`` clips in one launch (``kernels/audio.hip``): ``x [S, B]`` fp32, or
    int16 times ``scale``, read through its own strides (a ``[B, S]`` buffer goes in as ``buf.t()``),
    to fp32 ``[B, F, N/2 + 1]``.  ``tables = mfcc_tables(window_size, device=x.device)``."""
    S, B, F_, window, N = _audio_args("audio_spectrogram", x, tables, stride, False)
    shape = (B, F_, N // 2 + 1)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    _check(out, "audio_spectrogram: out", torch.float32, x.device)
    if tuple(out.shape) != shape:
        raise ValueError(f"audio_spectrogram: out {tuple(out.shape)} is not {shape}")
    if x.is_cuda:
        _launch_audio(x, tables, stride, scale, out, "spec_squared" if magnitude_squared else "spec_magnitude", S, B)
        return out
    p = _audio_frames_host(x, tables, stride, scale, F_)
    out.copy_(p if magnitude_squared else p.sqrt())
    return out


def audio_mfcc(x: torch.Tensor, tables: dict, stride: int, scale: float = 1.0, out: torch.Tensor | None = None,
               out_dtype=torch.float32, pad8: bool = False) -> torch.Tensor:
    """PCM to MFCC in one launch (``kernels/audio.hip``): ``AudioSpectrogram(magnitude_squared)``
    followed by ``Mfcc``, with nothing in memory in between.  ``x [S, B]`` as for
    ``audio_spectrogram``; ``tables = mfcc_tables(window_size, sample_rate, lower, upper, C, D,
    device=x.device)``.  The result is ``[B, F, D]`` fp32 or bf16, or with ``pad8`` bf16 ``[B, F, D,
    8]`` whose channel 0 holds the coefficients and channels 1..7 zeros (the padded input of a
    convolution over ``[B, F, D, 1]``).  bf16 results are the fp32 ones rounded to nearest even."""
    S, B, F_, window, N = _audio_args("audio_mfcc", x, tables, stride, True)
    C, D = tables["C"], tables["D"]
    if not 1 <= D <= C <= AUDIO_MAX_CHANNELS:
        raise ValueError(f"audio_mfcc: D={D}, C={C} outside 1 <= D <= C <= {AUDIO_MAX_CHANNELS}")
    if pad8:
        out_dtype = torch.bfloat16
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"audio_mfcc: out_dtype is fp32 or bf16, not {out_dtype}")
    shape = (B, F_, D, 8) if pad8 else (B, F_, D)
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=x.device)
    _check(out, "audio_mfcc: out", out_dtype, x.device)
    if tuple(out.shape) != shape:
        raise ValueError(f"audio_mfcc: out {tuple(out.shape)} is not {shape}")
    if x.is_cuda:
        if pad8 and out.data_ptr() % 16:
            raise ValueError("audio_mfcc: the padded output must be 16-byte aligned")
        mode = "mfcc_bf16_pad8" if pad8 else ("mfcc_f32" if out_dtype == torch.float32 else "mfcc_bf16")
        _launch_audio(x, tables, stride, scale, out, mode, S, B)
        return out
    v = _audio_frames_host(x, tables, stride, scale, F_).sqrt()  # [B, F, bins]
    bank = torch.zeros((N // 2 + 1, C), dtype=torch.float32)
    for c, (lo, mid, hi) in enumerate(tables["chan"].tolist()):
        bank[lo:mid, c] = tables["wb"][lo:mid]
        bank[mid:hi, c] = tables["wa"][mid:hi]
    res = torch.log((v @ bank).clamp_min(1e-12)) @ tables["dct"].t()
    if pad8:
        out.zero_()
        out[..., 0] = res.to(torch.bfloat16)
    else:
        out.copy_(res.to(out_dtype))
    return out


# ------------------------------------------------------------------------------ pooling
def pool2d_nhwc(x: torch.Tensor, ksize, stride, pad=(0, 0, 0, 0), mode="max", out=None, out_channel_offset=0):
    N, H, W, C = x.shape
    kh, kw = ksize
    sh, sw = stride
    pt, pb, pl, pr = pad
    Ho = (H + pt + pb - kh) // sh + 1
    Wo = (W + pl + pr - kw) // sw + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
        out_channel_offset = 0
    if x.is_cuda:
        _check(x, "x", device=x.device)
        _check(out, "out", device=x.device)
        _hip().pool2d_nhwc_bf16(x.data_ptr(), out.data_ptr(), N, H, W, C, Ho, Wo, kh, kw, sh, sw, pt, pl,
                                int(mode == "max"), out.shape[3], out_channel_offset, _stream())
        return out
    xn = x.float().permute(0, 3, 1, 2)
    if mode == "max":
        y = F.max_pool2d(F.pad(xn, (pl, pr, pt, pb), value=float("-inf")), (kh, kw), (sh, sw))
    else:
        s = F.avg_pool2d(F.pad(xn, (pl, pr, pt, pb)), (kh, kw), (sh, sw), divisor_override=1)
        c = F.avg_pool2d(F.pad(torch.ones_like(xn[:, :1]), (pl, pr, pt, pb)), (kh, kw), (sh, sw), divisor_override=1)
        y = s / c
    out[..., out_channel_offset:out_channel_offset + C] = y.permute(0, 2, 3, 1).to(out.dtype)
    return out


def global_avgpool(x: torch.Tensor, out=None) -> torch.Tensor:
    N, H, W, C = x.shape
    if out is None:
        out = torch.empty((N, C), dtype=x.dtype, device=x.device)
    if x.is_cuda:
        _check(x, "x", device=x.device)
        _check(out, "out", device=x.device)
        _hip().global_avgpool_bf16(x.data_ptr(), out.data_ptr(), N, H * W, C, _stream())
        return out
    out.copy_(x.float().mean((1, 2)).to(out.dtype))
    return out


# ------------------------------------------------------------------------------ softmax/top-k
def softmax_topk(logits: torch.Tensor, k: int, want_probs: bool = False, vals=None, idxs=None, probs=None):
    """Row softmax + top-k → (values fp32 [R,k], indices int32 [R,k], probs or None)."""
    R, C = logits.shape
    dev = logits.device
    if vals is None:
        vals = torch.empty((R, k), dtype=torch.float32, device=dev)
    if idxs is None:
        idxs = torch.empty((R, k), dtype=torch.int32, device=dev)
    if want_probs and probs is None:
        probs = torch.empty((R, C), dtype=logits.dtype, device=dev)
    if logits.is_cuda:
        if logits.stride(1) != 1:
            raise ValueError("softmax_topk: logits rows must be contiguous")
        _check(vals, "vals", torch.float32, dev)
        _check(idxs, "idxs", torch.int32, dev)
        _hip().softmax_topk_bf16(logits.data_ptr(), R, C, logits.stride(0), k, vals.data_ptr(), idxs.data_ptr(),
                                 _ptr(probs), _stream())
        return vals, idxs, probs
    p = torch.softmax(logits.float(), -1)
    v, i = torch.topk(p, k, -1)
    vals.copy_(v)
    idxs.copy_(i.to(torch.int32))
    if probs is not None:
        probs.copy_(p.to(probs.dtype))
    return vals, idxs, probs


# ------------------------------------------------------------------------------ attention
def attention(qkv: torch.Tensor, ids: torch.Tensor | None, batch: int, seq: int, heads: int, pad_id: int = 0,
              scale: float | None = None, out: torch.Tensor | None = None,
              cu_seqlens: torch.Tensor | None = None) -> torch.Tensor:
    """Multi-head self-attention over the fused QKV projection output.

    Padded batch: ``qkv`` [B*S, 3*H*64] bf16 (Q|K|V blocks, head h at h*64), ``ids`` [B*S]
    int32 token ids (keys whose id == ``pad_id`` are masked).  Packed batch
    (``cu_seqlens`` [B+1] int32 given, ``seq`` = the longest sequence): sequence b is rows
    ``cu[b]:cu[b+1]`` of ``qkv``, no padding; rows past ``cu[B]`` are left untouched.
    Returns ctx [rows, H*64]."""
    T = qkv.shape[0] if cu_seqlens is not None else batch * seq
    Dh = qkv.shape[1] // (3 * heads)
    if qkv.shape != (T, 3 * heads * Dh):
        raise ValueError(f"attention: qkv shape {tuple(qkv.shape)} != {(T, 3 * heads * Dh)}")
    if cu_seqlens is None and (ids is None or ids.numel() != T):
        raise ValueError("attention: ids must have B*S entries")
    if cu_seqlens is not None and cu_seqlens.numel() != batch + 1:
        raise ValueError("attention: cu_seqlens must have B+1 entries")
    scale = (1.0 / Dh ** 0.5) if scale is None else scale
    if out is None:
        out = torch.empty((T, heads * Dh), dtype=qkv.dtype, device=qkv.device)
    if qkv.is_cuda:
        _check(qkv, "qkv", device=qkv.device)
        _check(out, "out", device=qkv.device)
        if cu_seqlens is not None:
            _check(cu_seqlens, "cu_seqlens", torch.int32, qkv.device)
        else:
            _check(ids, "ids", torch.int32, qkv.device)
        _hip().attention_fwd_bf16(qkv.data_ptr(), _ptr(ids) if cu_seqlens is None else 0, _ptr(cu_seqlens),
                                  out.data_ptr(), batch, seq, heads, Dh, pad_id, float(scale), _stream())
        return out
    if cu_seqlens is not None:
        cu = cu_seqlens.tolist()
        for b in range(batch):
            a, e = cu[b], cu[b + 1]
            if e > a:
                q, k, v = qkv[a:e].float().reshape(e - a, 3, heads, Dh).permute(1, 2, 0, 3)
                p = torch.softmax((q @ k.transpose(-1, -2)) * scale, -1)
                out[a:e] = (p @ v).permute(1, 0, 2).reshape(e - a, heads * Dh).to(out.dtype)
        return out
    q, k, v = qkv.float().reshape(batch, seq, 3, heads, Dh).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale
    mask = (ids.reshape(batch, 1, 1, seq) == pad_id)
    s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, -1).nan_to_num(0.0)
    o = (p @ v).permute(0, 2, 1, 3).reshape(T, heads * Dh)
    out.copy_(o.to(out.dtype))
    return out


CLS_ATTENTION_MAX_SEQ = 512  # keys per sequence the cls_attention kernel holds in LDS


def cls_attention(qkv: torch.Tensor, cu_seqlens: torch.Tensor, batch: int, seq: int, heads: int,
                  scale: float | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Attention of each packed sequence's FIRST token only (the classifier's final layer):
    ``qkv`` [T, 3*H*64] packed rows, ``cu_seqlens`` [B+1] → [B, H*64].  ``seq`` is the
    longest possible sequence, as for ``attention``; the kernel keeps a sequence's scores in
    LDS and handles at most 512 keys, so ``seq`` > 512 raises ``ValueError`` on the device
    and on the host path alike (no sequence is ever silently truncated)."""
    if seq > CLS_ATTENTION_MAX_SEQ:
        raise ValueError(f"cls_attention: seq {seq} exceeds the {CLS_ATTENTION_MAX_SEQ} keys per sequence the "
                         "kernel supports")
    Dh = qkv.shape[1] // (3 * heads)
    scale = (1.0 / Dh ** 0.5) if scale is None else scale
    if out is None:
        out = torch.empty((batch, heads * Dh), dtype=qkv.dtype, device=qkv.device)
    if qkv.is_cuda:
        _check(qkv, "qkv", device=qkv.device)
        _check(out, "out", device=qkv.device)
        _check(cu_seqlens, "cu_seqlens", torch.int32, qkv.device)
        _hip().cls_attention_bf16(qkv.data_ptr(), cu_seqlens.data_ptr(), out.data_ptr(), batch, heads, Dh,
                                  float(scale), _stream())
        return out
    cu = cu_seqlens.tolist()
    for b in range(batch):
        a, e = cu[b], cu[b + 1]
        if e <= a:
            out[b] = 0
            continue
        q = qkv[a, :heads * Dh].float().reshape(heads, 1, Dh)
        k = qkv[a:e, heads * Dh:2 * heads * Dh].float().reshape(e - a, heads, Dh).transpose(0, 1)
        v = qkv[a:e, 2 * heads * Dh:].float().reshape(e - a, heads, Dh).transpose(0, 1)
        p = torch.softmax((q @ k.transpose(-1, -2)) * scale, -1)
        out[b] = (p @ v).reshape(heads * Dh).to(out.dtype)
    return out


def pack_tokens(ids: torch.Tensor, pad_id: int, t_cap: int, packed: torch.Tensor, pos: torch.Tensor,
                cu: torch.Tensor, cls: torch.Tensor) -> int | None:
    """Padding-free packing of ``ids`` [B, S]: the non-pad tokens in row order into
    ``packed[:T_eff]`` (their in-row positions into ``pos``), row offsets ``cu`` [B+1] and
    the first-token row of each sequence ``cls`` [B]; ``packed[T_eff:t_cap]`` = pad.
    Device path: one kernel, no host sync (returns None); host path returns T_eff."""
    B, S = ids.shape
    if ids.is_cuda:
        for t, n in ((ids, "ids"), (packed, "packed"), (pos, "pos"), (cu, "cu"), (cls, "cls")):
            _check(t, n, torch.int32, ids.device)
        _hip().pack_tokens(ids.data_ptr(), B, S, pad_id, t_cap, packed.data_ptr(), pos.data_ptr(), cu.data_ptr(),
                           cls.data_ptr(), _stream())
        return None
    keep = ids != pad_id
    lens = keep.sum(1)
    offs = torch.zeros(B + 1, dtype=torch.int64)
    offs[1:] = torch.cumsum(lens, 0)
    n = int(offs[-1])
    if n > t_cap:
        raise ValueError(f"pack_tokens: {n} tokens exceed the capacity {t_cap}")
    packed.zero_().add_(pad_id)
    pos.zero_()
    packed[:n] = ids[keep]
    pos[:n] = torch.arange(S, dtype=torch.int32).expand(B, S)[keep]
    cu.copy_(offs.to(torch.int32))
    cls.copy_(offs[:-1].clamp(max=t_cap - 1).to(torch.int32))
    return n


def embed_layernorm(ids: torch.Tensor, type_ids: torch.Tensor | None, word: torch.Tensor, pos: torch.Tensor,
                    type_emb: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, seq: int, eps: float = 1e-12,
                    out: torch.Tensor | None = None, pos_ids: torch.Tensor | None = None) -> torch.Tensor:
    """``LN(word[ids] + pos[p] + type[type_ids])`` → [T, D] bf16 (one fused pass), with the
    position ``p = t % seq`` (padded batch) or ``pos_ids[t]`` (packed batch)."""
    T = ids.numel()
    V, D = word.shape
    if out is None:
        out = torch.empty((T, D), dtype=word.dtype, device=word.device)
    if ids.is_cuda:
        _check(ids, "ids", torch.int32, ids.device)
        for t, n in ((word, "word"), (pos, "pos"), (type_emb, "type"), (out, "out")):
            _check(t, n, device=ids.device)
        if type_ids is not None:
            _check(type_ids, "type_ids", torch.int32, ids.device)
        if pos_ids is not None:
            _check(pos_ids, "pos_ids", torch.int32, ids.device)
        if pos.shape[0] < seq:
            raise ValueError("embed_layernorm: position table shorter than the sequence")
        _hip().embed_ln_bf16(ids.data_ptr(), _ptr(type_ids), _ptr(pos_ids), word.data_ptr(), pos.data_ptr(),
                             type_emb.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), T, seq, D, V,
                             float(eps), _stream())
        return out
    idx = ids.long().clamp(0, V - 1)
    p = pos_ids.long() if pos_ids is not None else torch.arange(T) % seq
    x = word.float()[idx] + pos.float()[p]
    x = x + type_emb.float()[type_ids.long() if type_ids is not None else torch.zeros(T, dtype=torch.long)]
    out.copy_(F.layer_norm(x, (D,), gamma.float(), beta.float(), eps).to(out.dtype))
    return out


# ------------------------------------------------------------------------------ layernorm
def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, residual: torch.Tensor | None = None,
              eps: float = 1e-12, out=None, sum_out=None) -> torch.Tensor:
    """``LN(x + residual)``; optionally also writes the pre-norm sum to ``sum_out``."""
    D = x.shape[-1]
    rows = x.numel() // D
    if out is None:
        out = torch.empty_like(x)
    if x.is_cuda:
        _check(x, "x", device=x.device)
        _check(out, "out", device=x.device)
        _check(gamma, "gamma", torch.float32, x.device)
        _check(beta, "beta", torch.float32, x.device)
        if residual is not None:
            _check(residual, "residual", device=x.device)
        _hip().layernorm_bf16(x.data_ptr(), _ptr(residual), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                              _ptr(sum_out), rows, D, float(eps), _stream())
        return out
    s = x.float() + (residual.float() if residual is not None else 0)
    if sum_out is not None:
        sum_out.copy_(s.to(sum_out.dtype))
    out.copy_(F.layer_norm(s, (D,), gamma.float(), beta.float(), eps).to(out.dtype))
    return out


# ------------------------------------------------------------------------------ direct conv
def dconv_eligible(Cin: int, KH: int, KW: int, stride, dilation, es: int, bn: int = 64) -> bool:
    """Narrow-layer direct conv (kernels/dconv.hip): stride 1/2, no dilation, Cin*es a
    multiple of the MFMA lane segment, weights + input patch within LDS."""
    sh, sw = stride
    if sh != sw or sh not in (1, 2) or tuple(dilation) != (1, 1) or KH * KW == 1:
        return False
    kl = 16 if es == 2 else 32
    if (Cin * es) % kl:
        return False
    kb = KH * KW * Cin * es
    wp = -(-kb // (4 * kl)) * (4 * kl) + 16
    ph, pw = 15 * sh + KH, 15 * sw + KW
    lds = ((ph * pw * Cin * es + 1023) & ~1023) + bn * wp + 1024
    return lds <= 96 * 1024  # leave room for >= 1 more resident workgroup


def dconv_weights(w_ohwi_bytes: torch.Tensor, Cout: int, es: int, bn: int) -> torch.Tensor:
    """[Cout, KH*KW*Cin*es] weight bytes → [round_up(Cout, bn), wp] with the kernel's pitch."""
    kl = 16 if es == 2 else 32
    kb = w_ohwi_bytes.shape[1]
    wp = -(-kb // (4 * kl)) * (4 * kl) + 16
    cpad = -(-Cout // bn) * bn
    out = torch.zeros((cpad, wp), dtype=torch.uint8, device=w_ohwi_bytes.device)
    out[:Cout, :kb] = w_ohwi_bytes
    return out


def dconv_bf16_weight_bytes(w_ohwi: torch.Tensor, bn: int) -> torch.Tensor:
    Cout = w_ohwi.shape[0]
    wb = w_ohwi.to(torch.bfloat16).contiguous().reshape(Cout, -1).view(torch.uint8)
    return dconv_weights(wb, Cout, 2, bn)


def _dconv_waves(waves, pool_rows, bn) -> int:
    """8-wave tiles pay where the filter-bank fetch dominates: BN = 64 (ResNet stem 180 -> 174 µs,
    Inception 2b 251 -> 223 µs; fp8 2b at 4 waves measured -1.7 % end to end, profiles/r05_k);
    BN = 32 tiles lose occupancy for little weight saving (2a 148 -> 156 µs) and stay at 4 waves
    (``bench/dconv_tune.py``, profiles/r02_dconv_waves)."""
    if waves is None and pool_rows is not None:
        waves = {7: 4, 14: 8}[int(pool_rows)]
    return int(waves or (8 if bn == 64 else 4))


def conv2d_direct(x: torch.Tensor, w_arr: torch.Tensor, kshape, Cout: int, bias: torch.Tensor, stride=(1, 1),
                  pad=(0, 0, 0, 0), act=None, out: torch.Tensor | None = None, out_channel_offset: int = 0,
                  bn: int = 64, chan_scale: torch.Tensor | None = None, out_scale: float | None = None,
                  maxpool_pad: tuple | None = None, pool_rows: int | None = None,
                  waves: int | None = None) -> torch.Tensor:
    """Direct conv on device: ``x`` NHWC bf16 (``chan_scale`` None) or e4m3 bytes (uint8, with
    the per-channel dequant scale ``chan_scale``); ``w_arr`` from :func:`dconv_weights`;
    ``out_scale`` → e4m3 output.  ``maxpool_pad = (top, bottom, left, right)`` fuses a 3x3 /
    stride-2 max pool of the ReLU output (ResNet stem → pool1).  ``waves`` (4 or 8, default
    8 for ``bn=64`` and 4 for ``bn=32``) sets the workgroup / tile size: 8 waves cover 32 x 16 conv
    pixels (pooled: 14 x 8 pooled pixels, ``pool_rows=14``; 4 waves = 16 x 16 / 7 x 8) and
    fetch the filter bank half as often; tiles whose patch would not fit LDS fall back to 4.
    The kernel has one stride for both axes: ``stride[0] != stride[1]`` is refused.
    Device-only (the host paths use the reference convs)."""
    N, H, W, Cin = x.shape
    KH, KW = kshape
    if stride[0] != stride[1]:
        raise ValueError(f"conv2d_direct: stride {tuple(stride)} must be the same on both axes")
    s = stride[0]
    pt, pb, pl, pr = pad
    Ho, Wo = conv_out_hw(H, W, KH, KW, s, s, pt, pl, 1, 1, pb, pr)
    es = 2 if x.dtype == torch.bfloat16 else 1
    out_fp8 = out_scale is not None
    Hp = Wp = ppt = ppl = 0
    oh, ow = Ho, Wo
    if maxpool_pad is not None:
        ppt, ppb, ppl, ppr = maxpool_pad
        Hp, Wp = (Ho + ppt + ppb - 3) // 2 + 1, (Wo + ppl + ppr - 3) // 2 + 1
        oh, ow = Hp, Wp
    if out is None:
        out = torch.empty((N, oh, ow, Cout), dtype=torch.uint8 if out_fp8 else torch.bfloat16, device=x.device)
        out_channel_offset = 0
    if out.shape[:3] != (N, oh, ow) or out_channel_offset + Cout > out.shape[3]:
        raise ValueError(f"conv2d_direct: out {tuple(out.shape)} cannot hold [{N},{oh},{ow},{Cout}]")
    if es == 1 and chan_scale is None:
        raise ValueError("conv2d_direct: fp8 input needs chan_scale")
    _check(x, "x", x.dtype, x.device)
    _check(w_arr, "w", torch.uint8, x.device)
    _check(bias, "bias", torch.float32, x.device)
    if chan_scale is not None:
        _check(chan_scale, "chan_scale", torch.float32, x.device)
    if bias.numel() < Cout or (chan_scale is not None and chan_scale.numel() < Cout):
        raise ValueError(f"conv2d_direct: bias / chan_scale shorter than Cout = {Cout}")  # read as float4 per quad
    _check(out, "out", torch.uint8 if out_fp8 else torch.bfloat16, x.device)  # the kernel writes out_fp8 ? 1 : 2 B
    _hip().dconv(x.data_ptr(), w_arr.data_ptr(), _ptr(chan_scale), bias.data_ptr(), out.data_ptr(), es, N, H, W, Cin,
                 Cout, KH, KW, s, pt, pl, Ho, Wo, w_arr.shape[1], out.shape[3], out_channel_offset, int(out_fp8),
                 1.0 / out_scale if out_fp8 else 1.0, act_code(act), bn, _stream(), Hp, Wp, ppt, ppl,
                 _dconv_waves(waves, pool_rows, bn))
    return out


def conv2d_direct_u8s2d(x_u8: torch.Tensor, w_arr: torch.Tensor, kshape, Cout: int, bias: torch.Tensor, pad, act,
                        mean, std, out: torch.Tensor | None = None, bn: int = 64, out_scale: float | None = None,
                        waves: int | None = None) -> torch.Tensor:
    """The s2d RGB stem (``s2d_stem_weights``) straight from the raw uint8 batch ``x_u8``
    [N, Hi, Wi, 3]: the kernel builds each patch as the normalised space-to-depth rows the
    preprocess kernel would write ((v - mean) / std, no resize), so the preprocess pass and
    its bf16 tensor disappear.  ``pad``: the block-space pads; device-only."""
    N, Hi, Wi, _ = x_u8.shape
    KH, KW = kshape
    pt, pb, pl, pr = pad
    Hb, Wb = (Hi + 1) // 2, (Wi + 1) // 2
    Ho, Wo = conv_out_hw(Hb, Wb, KH, KW, 1, 1, pt, pl, 1, 1, pb, pr)
    out_fp8 = out_scale is not None
    if out is None:
        out = torch.empty((N, Ho, Wo, Cout), dtype=torch.uint8 if out_fp8 else torch.bfloat16, device=x_u8.device)
    if tuple(out.shape[:3]) != (N, Ho, Wo) or out.shape[3] < Cout:
        raise ValueError(f"conv2d_direct_u8s2d: out {tuple(out.shape)} cannot hold [{N},{Ho},{Wo},{Cout}]")
    _check(x_u8, "x", torch.uint8, x_u8.device)
    _check(w_arr, "w", torch.uint8, x_u8.device)
    _check(bias, "bias", torch.float32, x_u8.device)
    _check(out, "out", torch.uint8 if out_fp8 else torch.bfloat16, x_u8.device)
    _hip().dconv_u8s2d(x_u8.data_ptr(), w_arr.data_ptr(), bias.data_ptr(), out.data_ptr(), N, Hi, Wi, Cout, KH, KW, pt,
                       pl, Ho, Wo, w_arr.shape[1], out.shape[3], 0, int(out_fp8), 1.0 / out_scale if out_fp8 else 1.0,
                       act_code(act), bn, float(mean[0]), float(mean[1]), float(mean[2]), 1.0 / std[0], 1.0 / std[1],
                       1.0 / std[2], _stream(), _dconv_waves(waves, None, bn))
    return out


# ------------------------------------------------------------------------------ fused shortcut
def conv1x1_dual(x: torch.Tensor, x2: torch.Tensor, w_cat: torch.Tensor, bias: torch.Tensor, stride2: int = 1,
                 act=None, out: torch.Tensor | None = None, out_channel_offset: int = 0, cfg: int = -1) -> torch.Tensor:
    """``act(conv1x1(x, W[:, :K1]) + conv1x1_stride(x2, W[:, K1:]) + bias)`` in ONE K loop —
    a bottleneck's expansion conv with its projection shortcut fused (the shortcut output
    never touches HBM).  ``x`` [N,Ho,Wo,K1], ``x2`` [N,H2,W2,C2], ``w_cat`` [Cout, K1+C2]."""
    N, Ho, Wo, K1 = x.shape
    _, H2, W2, C2 = x2.shape
    Cout = w_cat.shape[0]
    if w_cat.shape[1] != K1 + C2:
        raise ValueError(f"conv1x1_dual: weights K {w_cat.shape[1]} != {K1} + {C2}")
    if out is None:
        out = torch.empty((N, Ho, Wo, Cout), dtype=x.dtype if x.is_cuda else torch.float32, device=x.device)
        out_channel_offset = 0
    if x2.shape[0] != N or (Ho - 1) * stride2 >= H2 or (Wo - 1) * stride2 >= W2:
        raise ValueError(f"conv1x1_dual: shortcut source {tuple(x2.shape)} at stride {stride2} does not cover "
                         f"[{N},{Ho},{Wo}]")
    if out.shape[:3] != (N, Ho, Wo) or out_channel_offset + Cout > out.shape[3]:
        raise ValueError(f"conv1x1_dual: out {tuple(out.shape)} cannot hold [{N},{Ho},{Wo},{Cout}] at "
                         f"offset {out_channel_offset}")
    a = act_code(act)
    if x.is_cuda:
        for t, n in ((x, "x"), (x2, "x2"), (w_cat, "w"), (out, "out")):
            _check(t, n, device=x.device)
        _check(bias, "bias", torch.float32, x.device)
        _hip().conv1x1_dual_bf16(x.data_ptr(), x2.data_ptr(), w_cat.data_ptr(), bias.data_ptr(), out.data_ptr(), N, Ho,
                                 Wo, K1, C2, H2, W2, stride2, Cout, out.shape[3], out_channel_offset, a, _stream(), cfg)
        return out
    xs = x2[:, ::stride2, ::stride2, :][:, :Ho, :Wo, :]
    y = x.float() @ w_cat[:, :K1].float().t() + xs.float() @ w_cat[:, K1:].float().t() + bias.float()
    out[..., out_channel_offset:out_channel_offset + Cout] = _apply_act_ref(y, a).to(out.dtype)
    return out


def pw_res_ok(K_: int, N: int, num_cu: int = 256) -> bool:
    """Shapes ``pw_res`` takes: K = 128 / 256, N in 128-channel slices, every slice group
    of the 8 XCDs resident at once."""
    return K_ in (128, 256) and N % 128 == 0 and 8 * (N // 128) <= num_cu


def pw_res(x: torch.Tensor, w_nk: torch.Tensor, bias: torch.Tensor, residual: torch.Tensor,
           out: torch.Tensor | None = None, out_channel_offset: int = 0, tp: int = 0) -> torch.Tensor:
    """``relu(x @ w^T + bias + residual)`` for a 1x1 / stride-1 expansion conv over NHWC ``x``
    ``[..., K]`` (``pw_res_ok``: K = 128 / 256, N % 128 == 0), ``w_nk`` ``[N, K]``, ``residual``
    ``[..., N]``; ``tp`` = pixels per tile for K 256 (0: the measured default, 64).
    GPU: the persistent kernel with a resident 128-channel weight slice per workgroup and
    one-tile-ahead x / residual prefetch (kernels/pw_res.hip); host: the fp32 reference."""
    K_ = x.shape[-1]
    N = w_nk.shape[0]
    lead = tuple(x.shape[:-1])
    if not pw_res_ok(K_, N) or tuple(w_nk.reshape(N, -1).shape) != (N, K_):
        raise ValueError(f"pw_res: unsupported shapes x {tuple(x.shape)}, w {tuple(w_nk.shape)}")
    if tuple(residual.shape) != (*lead, N) or bias.numel() != N:
        raise ValueError("pw_res: residual must be [..., N] and bias [N]")
    if out is None:
        out = torch.empty((*lead, N), dtype=x.dtype if x.is_cuda else torch.float32, device=x.device)
        out_channel_offset = 0
    if tuple(out.shape[:-1]) != lead or out_channel_offset + N > out.shape[-1]:
        raise ValueError(f"pw_res: out {tuple(out.shape)} cannot hold [..., {N}] at offset {out_channel_offset}")
    M = x.numel() // K_
    if x.is_cuda:
        for t, n in ((x, "x"), (w_nk, "w"), (residual, "residual"), (out, "out")):
            _check(t, n, device=x.device)
        _check(bias, "bias", torch.float32, x.device)
        dev = x.device.index if x.device.index is not None else torch.cuda.current_device()
        _hip().pw_res_bf16(x.data_ptr(), w_nk.data_ptr(), bias.data_ptr(), residual.data_ptr(), out.data_ptr(), M, N,
                           K_, out.shape[-1], out_channel_offset, residual.shape[-1], _NUM_CU[dev], _stream(), tp)
        return out
    y = x.reshape(M, K_).float() @ w_nk.reshape(N, K_).float().t() + bias.float()
    y = torch.relu(y.to(out.dtype).float() + residual.reshape(M, N).float())
    out[..., out_channel_offset:out_channel_offset + N] = y.reshape(*lead, N).to(out.dtype)
    return out


# ------------------------------------------------------------------------------ elementwise
BIN_OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3, "max": 4, "min": 5, "rsub": 6, "rdiv": 7}
_BIN_REF = {0: lambda a, b: a + b, 1: lambda a, b: a - b, 2: lambda a, b: a * b, 3: lambda a, b: a / b,
            4: torch.maximum, 5: torch.minimum, 6: lambda a, b: b - a, 7: lambda a, b: b / a}


def binary(a: torch.Tensor, b, op: str, act=None, out: torch.Tensor | None = None) -> torch.Tensor:
    """``act(a OP b)`` with ``b`` a Python scalar, a fp32 vector over the last dim of ``a``,
    or a tensor of ``a``'s shape (the standalone elementwise kernel)."""
    code = BIN_OPS[op]
    a_act = act_code(act)
    if out is None:
        out = torch.empty(a.shape, dtype=a.dtype if a.is_cuda else torch.float32, device=a.device)
    if a.is_cuda:
        _check(a, "a", device=a.device)
        _check(out, "out", device=a.device)
        if isinstance(b, (int, float)):
            _hip().binary_bf16(code, a.data_ptr(), 0, out.data_ptr(), a.numel(), 0, 0, float(b), a_act, _stream())
        elif b.dim() == 1 and b.numel() == a.shape[-1]:
            _check(b, "b", torch.float32, a.device)
            _hip().binary_bf16(code, a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), 1, b.numel(), 0.0, a_act,
                               _stream())
        else:
            if tuple(b.shape) != tuple(a.shape):
                raise ValueError(f"binary: cannot broadcast {tuple(b.shape)} to {tuple(a.shape)}")
            _check(b, "b", device=a.device)
            _hip().binary_bf16(code, a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), 2, 0, 0.0, a_act, _stream())
        return out
    bb = b if isinstance(b, (int, float)) else b.float()
    out.copy_(_apply_act_ref(_BIN_REF[code](a.float(), bb if not isinstance(bb, (int, float)) else torch.tensor(bb)),
                             a_act).to(out.dtype))
    return out


def gather_rows(x: torch.Tensor, idx: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """``out[r] = x[idx[r]]`` over the rows of a 2-D tensor (int32 indices; an index out of
    range gives a zero row).  On the GPU one HIP kernel (16-byte chunks), no ATen gather."""
    n = idx.numel()
    if out is None:
        out = torch.empty((n, x.shape[-1]), dtype=x.dtype, device=x.device)
    if x.is_cuda:
        _check(x, "x", x.dtype, x.device)
        _check(out, "out", x.dtype, x.device)
        _check(idx, "idx", torch.int32, x.device)
        rb = x.shape[-1] * x.element_size()
        _hip().gather_rows(x.data_ptr(), idx.data_ptr(), out.data_ptr(), n, x.shape[0], rb, _stream())
        return out
    ok = (idx >= 0) & (idx < x.shape[0])
    out.zero_()
    out[ok] = x[idx[ok].long()]
    return out


def lrn(x: torch.Tensor, depth_radius: int = 5, bias: float = 1.0, alpha: float = 1.0, beta: float = 0.5,
        out: torch.Tensor | None = None) -> torch.Tensor:
    """TF ``LRN`` on NHWC (normalisation across channels)."""
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype if x.is_cuda else torch.float32, device=x.device)
    C = x.shape[-1]
    if x.is_cuda:
        _check(x, "x", device=x.device)
        _check(out, "out", device=x.device)
        _hip().lrn_bf16(x.data_ptr(), out.data_ptr(), x.numel() // C, C, int(depth_radius), float(bias), float(alpha),
                        float(beta), _stream())
        return out
    sq = x.float() ** 2
    acc = torch.zeros_like(sq)
    for d in range(-depth_radius, depth_radius + 1):
        lo, hi = max(0, -d), min(C, C - d)
        acc[..., lo:hi] += sq[..., lo + d:hi + d]
    out.copy_((x.float() / (bias + alpha * acc) ** beta).to(out.dtype))
    return out
