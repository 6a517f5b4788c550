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
