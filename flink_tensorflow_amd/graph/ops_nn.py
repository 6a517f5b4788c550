"""Neural-network op kernels with exact TF 1.x semantics (NHWC, SAME/VALID padding,
legacy ResizeBilinear coordinates, inference-mode FusedBatchNorm, LRN).

These are the semantic reference used by the interpreter and by CPU tests; the compiled
GPU plan (``graph/compiler.py``) lowers the same ops onto the hand-written CDNA4 kernels.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from .op_registry import register


def same_pads(in_size: int, k: int, s: int, d: int = 1) -> tuple[int, int]:
    """TF SAME padding: (before, after), asymmetric with the extra pixel after."""
    eff = (k - 1) * d + 1
    out = math.ceil(in_size / s)
    total = max((out - 1) * s + eff - in_size, 0)
    return total // 2, total - total // 2


def conv_out_size(in_size: int, k: int, s: int, padding: str, d: int = 1, pads=(0, 0)) -> int:
    eff = (k - 1) * d + 1
    if padding == "SAME":
        return math.ceil(in_size / s)
    if padding == "VALID":
        return (in_size - eff) // s + 1
    return (in_size + pads[0] + pads[1] - eff) // s + 1


def _hw(attr, fmt):
    if attr is None:
        return 1, 1
    if len(attr) == 4:
        return (attr[1], attr[2]) if fmt == "NHWC" else (attr[2], attr[3])
    if len(attr) == 2:
        return attr[0], attr[1]
    return attr[0], attr[0]


def _explicit_pads(node, fmt):
    p = node.attr("explicit_paddings", []) or []
    if not p:
        return (0, 0), (0, 0)
    p = list(p)
    if fmt == "NHWC":
        return (p[2], p[3]), (p[4], p[5])
    return (p[4], p[5]), (p[6], p[7])


def conv2d_tf(x, w_hwio, strides=(1, 1), padding="SAME", dilations=(1, 1), explicit=((0, 0), (0, 0)), groups=1):
    """NHWC conv with TF padding semantics (torch reference)."""
    sh, sw = strides
    dh, dw = dilations
    kh, kw = w_hwio.shape[0], w_hwio.shape[1]
    xn = x.permute(0, 3, 1, 2)
    if padding == "SAME":
        ph = same_pads(x.shape[1], kh, sh, dh)
        pw = same_pads(x.shape[2], kw, sw, dw)
    elif padding == "VALID":
        ph, pw = (0, 0), (0, 0)
    else:
        ph, pw = explicit
    if any(ph) or any(pw):
        xn = F.pad(xn, (pw[0], pw[1], ph[0], ph[1]))
    w = w_hwio.permute(3, 2, 0, 1)  # OIHW
    y = F.conv2d(xn, w.to(xn.dtype), stride=(sh, sw), dilation=(dh, dw), groups=groups)
    return y.permute(0, 2, 3, 1).contiguous()


@register("Conv2D")
def _conv2d(ctx, node, x, w):
    fmt = node.attr("data_format", "NHWC")
    s = _hw(node.attr("strides"), fmt)
    d = _hw(node.attr("dilations"), fmt)
    pad = node.attr("padding", "SAME")
    if fmt == "NCHW":
        x = x.permute(0, 2, 3, 1)
    y = conv2d_tf(x, w, s, pad, d, _explicit_pads(node, fmt))
    if fmt == "NCHW":
        y = y.permute(0, 3, 1, 2).contiguous()
    return (y,)


def conv2d_transpose_tf(x, w, out_hw, strides=(2, 2), padding="SAME", dilations=(1, 1), explicit=((0, 0), (0, 0))):
    """NHWC transposed conv (``Conv2DBackpropInput``): ``x`` is ``[N, Hi, Wi, Cin]``, ``w`` is
    ``[KH, KW, Cout, Cin]``, the result ``[N, Ho, Wo, Cout]`` with ``(Ho, Wo) = out_hw``::

        y[n, oy, ox, co] = sum x[n, iy, ix, ci] * w[ky, kx, co, ci]

    over the taps with ``oy + pt - ky == iy * sh``, ``0 <= iy < Hi``, and likewise in x;
    ``pt = same_pads(Ho, KH, sh)[0]`` for ``SAME`` and ``0`` for ``VALID``.  Output rows that no
    tap reaches are zero.  Arithmetic is float64 or the input dtype, like ``conv2d_tf``.  An
    ``out_hw`` whose forward conv would not produce ``[Hi, Wi]`` is rejected, as TF does.
    With ``dilations`` the tap offset is ``ky * dh``; ``padding="EXPLICIT"`` takes ``pt`` from
    ``explicit = ((top, bottom), (left, right))`` (interpreter only: neither is lowered)."""
    sh, sw = strides
    KH, KW, Cout, Cin = w.shape
    N, Hi, Wi, C = x.shape
    Ho, Wo = (int(v) for v in out_hw)
    if C != Cin:
        raise ValueError(f"conv2d_transpose: input has {C} channels, the filter expects {Cin}")
    dh, dw = dilations
    if padding not in ("SAME", "VALID", "EXPLICIT"):
        raise ValueError(f"conv2d_transpose: padding {padding!r} is not SAME, VALID or EXPLICIT")
    fwd = (conv_out_size(Ho, KH, sh, padding, dh, explicit[0]), conv_out_size(Wo, KW, sw, padding, dw, explicit[1]))
    if Ho < 1 or Wo < 1 or fwd != (Hi, Wi):
        raise ValueError(f"conv2d_transpose: a {KH}x{KW}/{sh}x{sw} {padding} conv of [{Ho}, {Wo}] does not give "
                         f"[{Hi}, {Wi}]")
    if padding == "SAME":
        pt, pl = same_pads(Ho, KH, sh, dh)[0], same_pads(Wo, KW, sw, dw)[0]
    else:
        pt, pl = (explicit[0][0], explicit[1][0]) if padding == "EXPLICIT" else (0, 0)
    # the scatter form: input pixel iy adds to rows iy * sh + ky - pt; then the window [pt, pt + Ho)
    full = F.conv_transpose2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1).to(x.dtype), stride=(sh, sw),
                              dilation=(dh, dw))
    full = full[:, :, pt:pt + Ho, pl:pl + Wo]
    if full.shape[2] != Ho or full.shape[3] != Wo:  # VALID with extra rows: no tap reaches them
        full = F.pad(full, (0, Wo - full.shape[3], 0, Ho - full.shape[2]))
    return full.permute(0, 2, 3, 1).contiguous()


@register("Conv2DBackpropInput")
def _conv2d_backprop_input(ctx, node, input_sizes, w, x):
    fmt = node.attr("data_format", "NHWC")
    pad = node.attr("padding", "SAME")
    sizes = [int(v) for v in torch.as_tensor(input_sizes).reshape(-1).tolist()]
    if len(sizes) == 4:
        out_hw = (sizes[1], sizes[2]) if fmt == "NHWC" else (sizes[2], sizes[3])
    elif len(sizes) == 2:
        out_hw = tuple(sizes)
    else:
        raise ValueError(f"Conv2DBackpropInput {node.name}: input_sizes must have 2 or 4 elements")
    if fmt == "NCHW":
        x = x.permute(0, 2, 3, 1)
    # TF's filter is [KH, KW, in, out] of the forward conv: ``in`` is this op's output channels
    y = conv2d_transpose_tf(x, w, out_hw, _hw(node.attr("strides"), fmt), pad, _hw(node.attr("dilations"), fmt),
                            _explicit_pads(node, fmt))
    if len(sizes) == 4 and (sizes[0], sizes[3 if fmt == "NHWC" else 1]) != (y.shape[0], y.shape[3]):
        raise ValueError(f"Conv2DBackpropInput {node.name}: input_sizes {sizes} != result {tuple(y.shape)}")
    if fmt == "NCHW":
        y = y.permute(0, 3, 1, 2).contiguous()
    return (y,)


def _dhw(attr, fmt, name):
    """The (depth, height, width) entries of a 5-vector attribute; TF rejects a batch or channel
    entry other than 1."""
    a = [1] * 5 if attr is None else [int(v) for v in attr]
    if len(a) != 5:
        raise ValueError(f"{name} must have 5 entries, got {a}")
    n, c = (0, 4) if fmt == "NDHWC" else (0, 1)
    if a[n] != 1 or a[c] != 1:
        raise ValueError(f"{name} {a}: the batch and channel entries must be 1")
    return tuple(a[1:4]) if fmt == "NDHWC" else tuple(a[2:5])


def conv3d_tf(x, w, strides=(1, 1, 1), padding="SAME", dilations=(1, 1, 1)):
    """NDHWC 3-D conv (``Conv3D``): ``x`` is ``[N, D, H, W, Cin]``, ``w`` is ``[KD, KH, KW, Cin,
    Cout]``, the result ``[N, Do, Ho, Wo, Cout]``::

        y[n, od, oh, ow, co] = sum x[n, od sd + kd dd - pf, oh sh + kh dh - pt, ow sw + kw dw - pl, ci]
                                   * w[kd, kh, kw, ci, co]

    over the taps whose input index is inside ``x`` on all three axes.  Per axis ``SAME`` gives
    ``out = ceil(in / s)`` and the front pad ``same_pads(in, k, s, d)[0]`` (the extra element goes
    behind); ``VALID`` gives ``out = (in - (k - 1) d - 1) // s + 1`` and no pad.  Arithmetic is
    float64 or the input dtype, like ``conv2d_tf``.  A channel mismatch and an empty output are
    rejected, as TF does."""
    if x.dim() != 5 or w.dim() != 5:
        raise ValueError(f"conv3d: input {tuple(x.shape)} / filter {tuple(w.shape)} are not 5-D")
    KD, KH, KW, Cin, Cout = w.shape
    N, D, H, W, C = x.shape
    if C != Cin:
        raise ValueError(f"conv3d: input has {C} channels, the filter expects {Cin}")
    if padding not in ("SAME", "VALID"):
        raise ValueError(f"conv3d: padding {padding!r} is not SAME or VALID")
    ext, ks = (D, H, W), (KD, KH, KW)
    pads = [same_pads(i, k, s, d) if padding == "SAME" else (0, 0) for i, k, s, d in zip(ext, ks, strides, dilations)]
    outs = [conv_out_size(i, k, s, padding, d) for i, k, s, d in zip(ext, ks, strides, dilations)]
    if min(outs) < 1:
        raise ValueError(f"conv3d: a {KD}x{KH}x{KW} {padding} conv of {ext} has an empty output {tuple(outs)}")
    xn = x.permute(0, 4, 1, 2, 3)
    if any(any(p) for p in pads):
        xn = F.pad(xn, (*pads[2], *pads[1], *pads[0]))
    y = F.conv3d(xn, w.permute(4, 3, 0, 1, 2).to(xn.dtype), stride=tuple(strides), dilation=tuple(dilations))
    return y.permute(0, 2, 3, 4, 1).contiguous()


@register("Conv3D")
def _conv3d(ctx, node, x, w):
    fmt = node.attr("data_format", "NDHWC")
    s = _dhw(node.attr("strides"), fmt, f"Conv3D {node.name}: strides")
    d = _dhw(node.attr("dilations"), fmt, f"Conv3D {node.name}: dilations")
    if fmt == "NCDHW":
        x = x.permute(0, 2, 3, 4, 1)
    y = conv3d_tf(x, w, s, node.attr("padding", "SAME"), d)
    if fmt == "NCDHW":
        y = y.permute(0, 4, 1, 2, 3).contiguous()
    return (y,)


def pool3d_tf(x, ksize, strides, padding, mode):
    """NDHWC 3-D pooling (``MaxPool3D`` / ``AvgPool3D``) with windows ``ksize = (kd, kh, kw)``::

        y[n, od, oh, ow, c] = max | mean of x[n, od sd + i - pf, oh sh + j - pt, ow sw + k - pl, c]

    over the window elements inside ``x``; output sizes and pads per axis as ``conv3d_tf``.
    Padding never wins a max, and a mean divides by the number of elements inside the input
    (TF's rule, and ``pool_tf``'s)."""
    if x.dim() != 5:
        raise ValueError(f"pool3d: input {tuple(x.shape)} is not 5-D")
    if padding not in ("SAME", "VALID") or mode not in ("max", "avg"):
        raise ValueError(f"pool3d: padding {padding!r} / mode {mode!r}")
    ext = tuple(x.shape[1:4])
    pads = [same_pads(i, k, s) if padding == "SAME" else (0, 0) for i, k, s in zip(ext, ksize, strides)]
    if min(conv_out_size(i, k, s, padding) for i, k, s in zip(ext, ksize, strides)) < 1:
        raise ValueError(f"pool3d: a {tuple(ksize)} {padding} window over {ext} has an empty output")
    xn = x.permute(0, 4, 1, 2, 3)
    flat = (*pads[2], *pads[1], *pads[0])
    if mode == "max":
        if any(flat):
            xn = F.pad(xn, flat, value=float("-inf"))
        y = F.max_pool3d(xn, tuple(ksize), tuple(strides))
    elif any(flat):
        ssum = F.avg_pool3d(F.pad(xn, flat), tuple(ksize), tuple(strides), divisor_override=1)
        cnt = F.avg_pool3d(F.pad(torch.ones_like(xn[:, :1]), flat), tuple(ksize), tuple(strides), divisor_override=1)
        y = ssum / cnt
    else:
        y = F.avg_pool3d(xn, tuple(ksize), tuple(strides))
    return y.permute(0, 2, 3, 4, 1).contiguous()


def _pool3d(node, x, mode):
    if node.attr("data_format", "NDHWC") != "NDHWC":
        raise NotImplementedError(f"{node.op} {node.name}: only NDHWC is supported")
    k = _dhw(node.attr("ksize"), "NDHWC", f"{node.op} {node.name}: ksize")
    s = _dhw(node.attr("strides"), "NDHWC", f"{node.op} {node.name}: strides")
    return (pool3d_tf(x, k, s, node.attr("padding", "VALID"), mode),)


@register("MaxPool3D")
def _maxpool3d(ctx, node, x):
    return _pool3d(node, x, "max")


@register("AvgPool3D")
def _avgpool3d(ctx, node, x):
    return _pool3d(node, x, "avg")


@register("DepthwiseConv2dNative")
def _dwconv(ctx, node, x, w):
    fmt = node.attr("data_format", "NHWC")
    s = _hw(node.attr("strides"), fmt)
    d = _hw(node.attr("dilations"), fmt)
    kh, kw, cin, mult = w.shape
    w2 = w.reshape(kh, kw, 1, cin * mult)
    return (conv2d_tf(x, w2, s, node.attr("padding", "SAME"), d, groups=cin),)


def pool_tf(x, ksize, strides, padding, mode):
    kh, kw = ksize
    sh, sw = strides
    xn = x.permute(0, 3, 1, 2)
    if padding == "SAME":
        ph = same_pads(x.shape[1], kh, sh)
        pw = same_pads(x.shape[2], kw, sw)
    else:
        ph, pw = (0, 0), (0, 0)
    if mode == "max":
        if any(ph) or any(pw):
            xn = F.pad(xn, (pw[0], pw[1], ph[0], ph[1]), value=float("-inf"))
        y = F.max_pool2d(xn, (kh, kw), (sh, sw))
    else:
        # TF AvgPool SAME excludes padding from the divisor
        if any(ph) or any(pw):
            xp = F.pad(xn, (pw[0], pw[1], ph[0], ph[1]))
            ones = F.pad(torch.ones_like(xn[:, :1]), (pw[0], pw[1], ph[0], ph[1]))
            ssum = F.avg_pool2d(xp, (kh, kw), (sh, sw), divisor_override=1)
            cnt = F.avg_pool2d(ones, (kh, kw), (sh, sw), divisor_override=1)
            y = ssum / cnt
        else:
            y = F.avg_pool2d(xn, (kh, kw), (sh, sw))
    return y.permute(0, 2, 3, 1).contiguous()


@register("MaxPool", "MaxPoolV2")
def _maxpool(ctx, node, x, *rest):
    fmt = node.attr("data_format", "NHWC")
    k = _hw(node.attr("ksize"), fmt)
    s = _hw(node.attr("strides"), fmt)
    return (pool_tf(x, k, s, node.attr("padding", "VALID"), "max"),)


@register("AvgPool")
def _avgpool(ctx, node, x):
    fmt = node.attr("data_format", "NHWC")
    k = _hw(node.attr("ksize"), fmt)
    s = _hw(node.attr("strides"), fmt)
    return (pool_tf(x, k, s, node.attr("padding", "VALID"), "avg"),)


def fused_batch_norm_inference(x, scale, offset, mean, var, eps):
    inv = torch.rsqrt(var.float() + eps) * scale.float()
    return (x.float() * inv + (offset.float() - mean.float() * inv)).to(x.dtype)


@register("FusedBatchNorm", "FusedBatchNormV2", "FusedBatchNormV3")
def _fused_bn(ctx, node, x, scale, offset, mean, var):
    eps = node.attr("epsilon", 1e-3)
    fmt = node.attr("data_format", "NHWC")
    if node.attr("is_training", True) and mean.numel() == 0:
        dims = (0, 1, 2) if fmt == "NHWC" else (0, 2, 3)
        mean = x.float().mean(dims)
        var = x.float().var(dims, unbiased=False)
    if fmt == "NCHW":
        sh = (1, -1, 1, 1)
        y = (x - mean.reshape(sh)) * torch.rsqrt(var.reshape(sh) + eps) * scale.reshape(sh) + offset.reshape(sh)
    else:
        y = fused_batch_norm_inference(x, scale, offset, mean, var, eps)
    z = torch.zeros(0, device=x.device)
    return (y, mean, var, z, z, z)


@register("LRN")
def _lrn(ctx, node, x):
    r = node.attr("depth_radius", 5)
    bias = node.attr("bias", 1.0)
    alpha = node.attr("alpha", 1.0)
    beta = node.attr("beta", 0.5)
    sq = (x.float() ** 2).permute(0, 3, 1, 2)  # N C H W
    c = sq.shape[1]
    pad = F.pad(sq, (0, 0, 0, 0, r, r))
    acc = torch.zeros_like(sq)
    for i in range(2 * r + 1):
        acc = acc + pad[:, i:i + c]
    y = x.float() / (bias + alpha * acc.permute(0, 2, 3, 1)) ** beta
    return (y.to(x.dtype),)


def resize_bilinear_tf(x, oh, ow, align_corners=False, half_pixel_centers=False):
    """TF ResizeBilinear on NHWC (float math; legacy coordinates by default)."""
    n, ih, iw, c = x.shape
    dev = x.device

    def scale(i, o):
        if align_corners and o > 1:
            return (i - 1) / (o - 1)
        return i / o

    sy, sx = scale(ih, oh), scale(iw, ow)
    ys = torch.arange(oh, device=dev, dtype=torch.float32)
    xs = torch.arange(ow, device=dev, dtype=torch.float32)
    if half_pixel_centers:
        fy = (ys + 0.5) * sy - 0.5
        fx = (xs + 0.5) * sx - 0.5
    else:
        fy = ys * sy
        fx = xs * sx
    y0 = torch.clamp(torch.floor(fy), min=0).long()
    x0 = torch.clamp(torch.floor(fx), min=0).long()
    y1 = torch.clamp(y0 + 1, max=ih - 1)
    x1 = torch.clamp(x0 + 1, max=iw - 1)
    wy = (fy - torch.floor(fy)).clamp(0, 1) if not half_pixel_centers else (fy - y0.float()).clamp(0, 1)
    wx = (fx - torch.floor(fx)).clamp(0, 1) if not half_pixel_centers else (fx - x0.float()).clamp(0, 1)
    xf = x.float()
    top = xf[:, y0][:, :, x0] * (1 - wx)[None, None, :, None] + xf[:, y0][:, :, x1] * wx[None, None, :, None]
    bot = xf[:, y1][:, :, x0] * (1 - wx)[None, None, :, None] + xf[:, y1][:, :, x1] * wx[None, None, :, None]
    return top * (1 - wy)[None, :, None, None] + bot * wy[None, :, None, None]


@register("ResizeBilinear")
def _resize_bilinear(ctx, node, x, size):
    oh, ow = [int(v) for v in size.reshape(-1).tolist()]
    return (resize_bilinear_tf(x, oh, ow, node.attr("align_corners", False), node.attr("half_pixel_centers", False)),)


@register("ResizeNearestNeighbor")
def _resize_nn(ctx, node, x, size):
    oh, ow = [int(v) for v in size.reshape(-1).tolist()]
    n, ih, iw, c = x.shape
    ys = torch.clamp((torch.arange(oh, device=x.device) * (ih / oh)).floor().long(), max=ih - 1)
    xs = torch.clamp((torch.arange(ow, device=x.device) * (iw / ow)).floor().long(), max=iw - 1)
    return (x[:, ys][:, :, xs],)


@register("L2Normalize")
def _l2n(ctx, node, x):
    return (F.normalize(x, dim=-1),)


# ------------------------------------------------------------------------------ detection: box decode + NMS
# The semantic reference of the detection heads (TF's ``non_max_suppression_op.cc``), with what
# TF leaves open pinned down.  ``kernels/detection.hip`` computes the same thing operation for
# operation in fp32; ``K.combined_nms`` runs these routines on host tensors.
#
# * Per image and class the candidates are the boxes with ``score > score_threshold`` (a NaN
#   never passes), visited in descending score, **equal scores lower box index first** (TF's
#   priority queue leaves ties open).  A candidate is kept unless its IoU with a box already
#   kept for that class is ``> iou_threshold``; selection stops at ``min(max_per_class, N)``.
# * IoU is taken on the canonicalised corners (min / max of the two y and of the two x values),
#   every operation rounded to fp32: ``area = (y2 - y1) * (x2 - x1)``, ``inter = max(0, min(y2) -
#   max(y1)) * max(0, min(x2) - max(x1))``, ``iou = inter / ((area_a + area_b) - inter)``, and 0
#   when either area is <= 0.
# * The kept boxes of all classes are merged in descending score, **equal scores lower class
#   first, then lower box index**, and the first ``T`` are taken.
def decode_boxes_yxhw(enc, anchors, scales):
    """SSD box decoding in fp32, every operation rounded, in this order (``scales`` are the
    four *reciprocal* scale factors ``s0..s3``, ``anchors`` is ``[N, 4]`` = (yc, xc, h, w))::

        cy = (ty * s0) * ha + yca        cx = (tx * s1) * wa + xca
        h  = exp(th * s2) * ha           w  = exp(tw * s3) * wa
        box = (cy - 0.5 * h, cx - 0.5 * w, cy + 0.5 * h, cx + 0.5 * w)

    ``enc`` is ``[..., N, 4]`` = (ty, tx, th, tw); the result has its shape, fp32."""
    enc = torch.as_tensor(enc).float()
    a = torch.as_tensor(anchors).float()
    s = torch.as_tensor(scales, dtype=torch.float32)
    c = enc[..., 0:2] * s[0:2] * a[:, 2:4] + a[:, 0:2]
    hw = torch.exp(enc[..., 2:4] * s[2:4]) * a[:, 2:4]
    half = hw * 0.5
    return torch.cat([c - half, c + half], dim=-1)


def _nms_class_np(boxes, scores, max_out, iou_thr, score_thr):
    """Greedy NMS of one class: ``boxes`` [N, 4] and ``scores`` [N] fp32 numpy arrays; the kept
    box indices in selection order."""
    import numpy as np

    cand = np.nonzero(scores > score_thr)[0]
    order = cand[np.argsort(-scores[cand], kind="stable")]  # equal scores: lower index first
    y1, y2 = np.minimum(boxes[:, 0], boxes[:, 2]), np.maximum(boxes[:, 0], boxes[:, 2])
    x1, x2 = np.minimum(boxes[:, 1], boxes[:, 3]), np.maximum(boxes[:, 1], boxes[:, 3])
    area = (y2 - y1) * (x2 - x1)
    thr = np.float32(iou_thr)
    zero = np.float32(0)
    kept: list[int] = []
    for i in order.tolist():
        if len(kept) >= max_out:
            break
        if kept and area[i] > 0:
            k = np.asarray(kept)
            inter = np.maximum(zero, np.minimum(y2[i], y2[k]) - np.maximum(y1[i], y1[k])) * \
                np.maximum(zero, np.minimum(x2[i], x2[k]) - np.maximum(x1[i], x1[k]))
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = np.where(area[k] > 0, inter / ((area[i] + area[k]) - inter), zero)
            if bool((iou > thr).any()):
                continue
        kept.append(i)
    return kept


def combined_nms_host(boxes, scores, max_per_class, max_total, iou_threshold, score_threshold, pad_per_class=False,
                      clip_boxes=True):
    """``CombinedNonMaxSuppression`` on host tensors: ``boxes`` [B, N, q, 4] (q = 1 or C),
    ``scores`` [B, N, C].  Returns ``(boxes [B, T, 4], scores [B, T], classes [B, T])`` fp32 and
    ``valid [B]`` int32; rows past ``valid`` are zero."""
    import numpy as np

    bx = torch.as_tensor(boxes).detach().float().cpu().numpy()
    sc = torch.as_tensor(scores).detach().float().cpu().numpy()
    if bx.ndim != 4 or sc.ndim != 3 or bx.shape[3] != 4 or bx.shape[:2] != sc.shape[:2]:
        raise ValueError(f"combined_nms: boxes {bx.shape} / scores {sc.shape} are not [B,N,q,4] / [B,N,C]")
    B, N, C = sc.shape
    q = bx.shape[2]
    if q not in (1, C):
        raise ValueError(f"combined_nms: boxes have q={q} per-class boxes, expected 1 or {C}")
    mpc, T = int(max_per_class), int(max_total)
    if mpc < 1 or T < 1:
        raise ValueError("combined_nms: max_output_size_per_class and max_total_size must be positive")
    if pad_per_class:
        T = min(T, mpc * C)
    sc = sc + np.float32(0)  # -0.0 is 0.0: equal scores
    ob = np.zeros((B, T, 4), np.float32)
    os_ = np.zeros((B, T), np.float32)
    oc = np.zeros((B, T), np.float32)
    ov = np.zeros((B,), np.int32)
    for b in range(B):
        ent = []
        for c in range(C):
            cb = bx[b, :, c if q > 1 else 0]
            for i in _nms_class_np(cb, sc[b, :, c], min(mpc, N), float(iou_threshold), np.float32(score_threshold)):
                ent.append((-float(sc[b, i, c]), c, i))
        ent.sort()
        ent = ent[:T]
        ov[b] = len(ent)
        for t, (_, c, i) in enumerate(ent):
            ob[b, t] = bx[b, i, c if q > 1 else 0]
            os_[b, t] = sc[b, i, c]
            oc[b, t] = c
    if clip_boxes:
        ob = np.clip(ob, np.float32(0), np.float32(1))
    return torch.from_numpy(ob), torch.from_numpy(os_), torch.from_numpy(oc), torch.from_numpy(ov)


def _scalar(t):
    return torch.as_tensor(t).reshape(-1)[0].item()


@register("CombinedNonMaxSuppression")
def _combined_nms(ctx, node, boxes, scores, max_per_class, max_total, iou_thr, score_thr):
    outs = combined_nms_host(boxes, scores, int(_scalar(max_per_class)), int(_scalar(max_total)),
                             float(_scalar(iou_thr)), float(_scalar(score_thr)),
                             bool(node.attr("pad_per_class", False)), bool(node.attr("clip_boxes", True)))
    return tuple(o.to(boxes.device) for o in outs)


def _nms_single(node, boxes, scores, max_out, iou_thr, score_thr, pad):
    import numpy as np

    bx = torch.as_tensor(boxes).detach().float().cpu().numpy()
    sc = torch.as_tensor(scores).detach().float().cpu().numpy()
    if bx.ndim != 2 or bx.shape[1] != 4 or sc.shape != (bx.shape[0],):
        raise ValueError(f"{node.op}: boxes {bx.shape} / scores {sc.shape} are not [N,4] / [N]")
    m = int(_scalar(max_out))
    kept = _nms_class_np(bx, sc + np.float32(0), m, float(_scalar(iou_thr)), np.float32(score_thr))
    valid = len(kept)
    sel_scores = sc[kept] if kept else np.zeros((0,), np.float32)
    if pad:
        kept = kept + [0] * (m - valid)
        sel_scores = np.concatenate([sel_scores, np.zeros((m - valid,), np.float32)])
    dev = boxes.device
    return (torch.tensor(kept, dtype=torch.int32, device=dev), torch.from_numpy(np.asarray(sel_scores, np.float32)).to(dev),
            torch.tensor(valid, dtype=torch.int32, device=dev))


@register("NonMaxSuppressionV2")
def _nms_v2(ctx, node, boxes, scores, max_out, iou_thr):
    return _nms_single(node, boxes, scores, max_out, iou_thr, float("-inf"), False)[:1]


@register("NonMaxSuppressionV3")
def _nms_v3(ctx, node, boxes, scores, max_out, iou_thr, score_thr):
    return _nms_single(node, boxes, scores, max_out, iou_thr, _scalar(score_thr), False)[:1]


@register("NonMaxSuppressionV4")
def _nms_v4(ctx, node, boxes, scores, max_out, iou_thr, score_thr):
    idx, _, valid = _nms_single(node, boxes, scores, max_out, iou_thr, _scalar(score_thr),
                                bool(node.attr("pad_to_max_output_size", False)))
    return idx, valid


@register("NonMaxSuppressionV5")
def _nms_v5(ctx, node, boxes, scores, max_out, iou_thr, score_thr, soft_nms_sigma):
    if float(_scalar(soft_nms_sigma)) != 0.0:
        raise NotImplementedError(f"{node.op} {node.name}: soft_nms_sigma != 0 (Soft-NMS) is not supported")
    return _nms_single(node, boxes, scores, max_out, iou_thr, _scalar(score_thr),
                       bool(node.attr("pad_to_max_output_size", False)))


def block_lstm(seq_len_max, x, cs_prev, h_prev, w, wci, wcf, wco, b, forget_bias=1.0, cell_clip=3.0,
               use_peephole=False):
    """TF ``BlockLSTM`` (the fused cell of ``LSTMBlockFusedCell``): ``x [T, B, I]``, ``w [I + H,
    4H]`` and ``b [4H]`` with gate columns in the order i, ci, f, o.  Returns ``(i, cs, f, o, ci,
    co, h)``, each ``[T, B, H]``; steps ``t >= seq_len_max`` of every output are zero."""
    if x.dim() != 3 or cs_prev.dim() != 2 or w.dim() != 2:
        raise ValueError(f"BlockLSTM: x {tuple(x.shape)} / cs_prev {tuple(cs_prev.shape)} / w {tuple(w.shape)} are not "
                         "[T,B,I] / [B,H] / [I+H,4H]")
    T, B, I = x.shape
    H = cs_prev.shape[1]
    if tuple(w.shape) != (I + H, 4 * H) or tuple(h_prev.shape) != (B, H) or tuple(cs_prev.shape) != (B, H) \
            or b.numel() != 4 * H:
        raise ValueError(f"BlockLSTM: w {tuple(w.shape)}, b {tuple(b.shape)}, h_prev {tuple(h_prev.shape)} do not match "
                         f"T={T}, B={B}, I={I}, H={H}")
    steps = max(0, min(T, int(_scalar(seq_len_max))))
    outs = [torch.zeros((T, B, H), dtype=x.dtype, device=x.device) for _ in range(7)]
    cs, h = cs_prev, h_prev
    for t in range(steps):
        gi, gc, gf, go = (torch.cat([x[t], h], dim=1) @ w + b).split(H, dim=1)
        gf = gf + forget_bias
        if use_peephole:
            gi, gf = gi + cs * wci, gf + cs * wcf
        gi, gf, ci = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gc)
        cs = ci * gi + cs * gf
        if cell_clip > 0:
            cs = cs.clamp(-cell_clip, cell_clip)
        if use_peephole:
            go = go + cs * wco
        go, co = torch.sigmoid(go), torch.tanh(cs)
        h = co * go
        for o, v in zip(outs, (gi, cs, gf, go, ci, co, h)):
            o[t] = v
    return tuple(outs)


@register("BlockLSTM")
def _block_lstm(ctx, node, seq_len_max, x, cs_prev, h_prev, w, wci, wcf, wco, b):
    return block_lstm(seq_len_max, x, cs_prev, h_prev, w, wci, wcf, wco, b, float(node.attr("forget_bias", 1.0)),
                      float(node.attr("cell_clip", 3.0)), bool(node.attr("use_peephole", False)))


# ------------------------------------------------------------------ audio front end
def spectrogram_fft_length(window_size: int) -> int:
    """The smallest power of two ``>= window_size`` (TF ``Spectrogram::Initialize``)."""
    n = 1
    while n < window_size:
        n *= 2
    return n


def spectrogram_frames(samples: int, window_size: int, stride: int) -> int:
    return 1 + (samples - window_size) // stride if samples >= window_size else 0


def audio_spectrogram(x, window_size: int, stride: int, magnitude_squared: bool = False):
    """TF ``AudioSpectrogram``: ``x [S, Ch]`` float to ``[Ch, F, N/2 + 1]`` float32, with ``N`` the
    smallest power of two ``>= window_size`` and ``F = 1 + (S - window_size) // stride`` frames
    (0 when ``S < window_size``).  Frame ``f`` is samples ``[f stride, f stride + window_size)``
    times the periodic Hann window ``0.5 - 0.5 cos(2 pi n / window_size)``, zero-padded to ``N``;
    the output is ``re^2 + im^2`` of its real DFT, or the square root of that when
    ``magnitude_squared`` is false.  Computed in float64, as TF does."""
    if x.dim() != 2:
        raise ValueError(f"AudioSpectrogram: input {tuple(x.shape)} is not [samples, channels]")
    window_size, stride = int(window_size), int(stride)
    if window_size < 2 or stride < 1:
        raise ValueError(f"AudioSpectrogram: window_size={window_size} (>= 2) / stride={stride} (>= 1)")
    S, Ch = x.shape
    N = spectrogram_fft_length(window_size)
    F_ = spectrogram_frames(S, window_size, stride)
    if F_ == 0:
        return torch.zeros((Ch, 0, N // 2 + 1), dtype=torch.float32, device=x.device)
    n = torch.arange(window_size, dtype=torch.float64, device=x.device)
    hann = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / window_size)
    xt = x.to(torch.float64).t().contiguous()  # [Ch, S]
    frames = xt[:, :(F_ - 1) * stride + window_size].unfold(1, window_size, stride) * hann  # [Ch, F, window]
    z = torch.fft.rfft(frames, n=N, dim=-1)
    p = z.real * z.real + z.imag * z.imag
    return (p if magnitude_squared else p.sqrt()).to(torch.float32)


def mel_filterbank(bins: int, sample_rate: float, lower: float, upper: float, channels: int):
    """TF's ``MfccMelFilterbank`` for spectrogram rows of ``bins`` values, as float64 numpy:
    ``(start, end, band [bins] int, weight [bins])``.  ``mel(f) = 1127 ln(1 + f / 700)``; the
    ``channels + 1`` centres are ``mel_lo + span / (channels + 1) (i + 1)``; ``hz_per_bin =
    0.5 sample_rate / (bins - 1)``; bins ``start = int(1.5 + lower / hz_per_bin)`` to ``end =
    int(upper / hz_per_bin)`` take part.  ``band[i]`` is the last centre (of the first
    ``channels``) below the bin's mel, -1 below the first centre, and ``weight[i] = (centre[band
    + 1] - mel_i) / (centre[band + 1] - centre[band])`` with ``mel_lo`` for ``centre[-1]``.
    Raises ``ValueError`` when a channel receives no bin."""
    import numpy as np

    if bins < 2 or channels < 1 or sample_rate <= 0 or lower < 0 or upper <= lower:
        raise ValueError(f"Mfcc: bins={bins}, channels={channels}, sample_rate={sample_rate}, "
                         f"limits {lower}..{upper} are not a filter bank")

    def mel(f):
        return 1127.0 * math.log1p(f / 700.0)

    mel_lo, mel_hi = mel(float(lower)), mel(float(upper))
    spacing = (mel_hi - mel_lo) / (channels + 1)
    centre = [mel_lo + spacing * (i + 1) for i in range(channels + 1)]
    hz_per_bin = 0.5 * float(sample_rate) / (bins - 1)
    start, end = int(1.5 + lower / hz_per_bin), min(int(upper / hz_per_bin), bins - 1)
    band = np.full((bins,), -2, dtype=np.int64)
    weight = np.zeros((bins,), dtype=np.float64)
    ch = 0
    for i in range(start, end + 1):
        m = mel(i * hz_per_bin)
        while ch < channels and centre[ch] < m:
            ch += 1
        band[i] = ch - 1
        if ch - 1 >= 0:
            weight[i] = (centre[ch] - m) / (centre[ch] - centre[ch - 1])
        else:
            weight[i] = (centre[0] - m) / (centre[0] - mel_lo)
    hit = np.zeros((channels,), dtype=bool)
    for i in range(start, end + 1):
        if band[i] >= 0:
            hit[band[i]] = True
        if band[i] + 1 < channels:
            hit[band[i] + 1] = True
    if not hit.all():
        raise ValueError(f"Mfcc: mel channels {np.nonzero(~hit)[0].tolist()} receive no spectrogram bin "
                         f"({bins} bins, {sample_rate} Hz, {lower}..{upper} Hz, {channels} channels)")
    return start, end, band, weight


def mfcc(spectrogram, sample_rate, upper_frequency_limit=4000.0, lower_frequency_limit=20.0,
         filterbank_channel_count=40, dct_coefficient_count=13):
    """TF ``Mfcc``: squared-magnitude ``spectrogram [Ch, F, bins]`` to ``[Ch, F, D]`` float32.
    With the filter bank of ``mel_filterbank`` and ``v = sqrt(spectrogram[i])``, taking the bins
    in ascending order, channel ``band[i]`` gains ``v weight[i]`` (when ``band[i] >= 0``) and
    channel ``band[i] + 1`` gains ``v - v weight[i]`` (when it is ``< C``); then ``log(max(.,
    1e-12))``; then ``out[d] = sum_j sqrt(2 / C) cos(d pi / C (j + 0.5)) logmel[j]``.  ``D <= C``
    is required.  Computed in float64."""
    import numpy as np

    if spectrogram.dim() != 3:
        raise ValueError(f"Mfcc: spectrogram {tuple(spectrogram.shape)} is not [channels, frames, bins]")
    C, D = int(filterbank_channel_count), int(dct_coefficient_count)
    if D < 1 or D > C:
        raise ValueError(f"Mfcc: dct_coefficient_count={D} must be in 1..filterbank_channel_count={C}")
    Ch, F_, bins = spectrogram.shape
    start, end, band, weight = mel_filterbank(bins, float(_scalar(sample_rate)), float(lower_frequency_limit),
                                              float(upper_frequency_limit), C)
    v = spectrogram.detach().to(torch.float64).cpu().numpy().reshape(Ch * F_, bins)
    v = np.sqrt(v)
    mel = np.zeros((Ch * F_, C), dtype=np.float64)
    for i in range(start, end + 1):
        c = int(band[i])
        wv = v[:, i] * weight[i]
        if c >= 0:
            mel[:, c] += wv
        if c + 1 < C:
            mel[:, c + 1] += v[:, i] - wv
    logmel = np.log(np.maximum(mel, 1e-12))
    j = np.arange(C, dtype=np.float64)
    dct = math.sqrt(2.0 / C) * np.cos(np.arange(D, dtype=np.float64)[:, None] * (math.pi / C) * (j[None, :] + 0.5))
    out = logmel @ dct.T
    return torch.from_numpy(out.astype(np.float32)).reshape(Ch, F_, D).to(spectrogram.device)


def decode_wav(contents: bytes, desired_channels: int = -1, desired_samples: int = -1):
    """TF ``DecodeWav``: RIFF / WAVE with 16-bit PCM only.  Returns ``(audio [samples, channels]
    float32 = int16 / 32768, sample_rate)``; truncated or zero-padded to ``desired_samples``."""
    import struct

    import numpy as np

    b = bytes(contents)
    if len(b) < 12 or b[:4] != b"RIFF" or b[8:12] != b"WAVE":
        raise ValueError("DecodeWav: not a RIFF/WAVE file")
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(b):
        cid, size = b[pos:pos + 4], struct.unpack_from("<I", b, pos + 4)[0]
        body = b[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            if size < 16 or len(body) < 16:
                raise ValueError("DecodeWav: short fmt chunk")
            fmt = struct.unpack_from("<HHIIHH", body, 0)
        elif cid == b"data":
            if len(body) != size:
                raise ValueError("DecodeWav: data chunk runs past the end of the file")
            data = body
            break
        pos += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError("DecodeWav: missing fmt or data chunk")
    tag, channels, rate, _, _, bits = fmt
    if tag != 1 or bits != 16:
        raise ValueError(f"DecodeWav: only 16-bit PCM is supported (format {tag}, {bits} bits)")
    if channels < 1:
        raise ValueError("DecodeWav: no channels")
    if desired_channels not in (-1, channels):
        raise ValueError(f"DecodeWav: the file has {channels} channels, desired_channels={desired_channels}")
    pcm = np.frombuffer(data[:len(data) // (2 * channels) * 2 * channels], dtype="<i2").reshape(-1, channels)
    if desired_samples >= 0:
        if pcm.shape[0] >= desired_samples:
            pcm = pcm[:desired_samples]
        else:
            pcm = np.concatenate([pcm, np.zeros((desired_samples - pcm.shape[0], channels), dtype=pcm.dtype)])
    return torch.from_numpy(pcm.astype(np.float32) / np.float32(32768.0)), int(rate)


@register("AudioSpectrogram")
def _audio_spectrogram(ctx, node, x):
    return (audio_spectrogram(x, int(node.attr("window_size")), int(node.attr("stride")),
                              bool(node.attr("magnitude_squared", False))),)


@register("Mfcc")
def _mfcc(ctx, node, spectrogram, sample_rate):
    return (mfcc(spectrogram, sample_rate, float(node.attr("upper_frequency_limit", 4000.0)),
                 float(node.attr("lower_frequency_limit", 20.0)), int(node.attr("filterbank_channel_count", 40)),
                 int(node.attr("dct_coefficient_count", 13))),)


@register("DecodeWav")
def _decode_wav(ctx, node, contents):
    from ..types.tensor import StringTensor

    if not isinstance(contents, StringTensor) or contents.numel() != 1:
        raise TypeError("DecodeWav: contents is a scalar STRING tensor")
    audio, rate = decode_wav(contents.array.reshape(-1)[0], int(node.attr("desired_channels", -1)),
                             int(node.attr("desired_samples", -1)))
    return audio.to(ctx.device), torch.tensor(rate, dtype=torch.int32, device=ctx.device)
