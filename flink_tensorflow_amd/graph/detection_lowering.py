"""Lowering of detection heads (a mixin of ``CompiledFunction``): ``CombinedNonMaxSuppression``
to one ``nms`` step on ``kernels/detection.hip``, with the SSD box decoding and the score
slice in front of it absorbed.

**The NMS.**  ``CombinedNonMaxSuppression`` lowers when its four scalar inputs are constants,
its boxes are shared by the classes (``q == 1``), ``boxes`` and ``scores`` are activations and
the shapes are inside ``K.nms_eligible``; anything else stays a glue op (``CompileError`` under
``strict``) in a host plan.  The glue op is the interpreter's host routine (Python loops over
host copies): a plan on a GPU cannot capture it in a hipGraph, and run eagerly it would be the
per-record host work a plan exists to remove, so there a glue NMS (``CombinedNonMaxSuppression``
or a padded ``NonMaxSuppressionV4`` / ``V5``) raises ``CompileError`` in non-strict mode too and
``ModelFunction`` falls back to the interpreter.  The step writes four values, ``[B, T, 4]``,
``[B, T]``, ``[B, T]`` fp32 and ``[B]`` int32, and takes its scratch from the plan's slab.  The unpadded ``NonMaxSuppressionV2..V5``
have a data-dependent output shape: a plan refuses them in non-strict mode too (the glue dry
run on zeros would plan the wrong shape), and ``ModelFunction`` falls back to the interpreter.

**The score slice.**  A ``StridedSlice`` / ``Slice`` that cuts only the last axis of the
scores (the background column) and feeds nothing but the NMS emits no ``copy`` step: the kernel
reads the columns in place through a pitch and a class offset.

**The fused decode.**  ``GraphBuilder.decode_boxes`` emits SSD box decoding in this one form,
which ``_match_decode`` recognises from the NMS's ``boxes`` input backwards::

    t_yx = StridedSlice(enc)[..., 0:2]            t_hw = StridedSlice(enc)[..., 2:4]
    c = Add(Mul(Mul(t_yx, inv_scale_yx[2]), anchors_hw[N, 2]), anchors_yx[N, 2])
    s = Mul(Exp(Mul(t_hw, inv_scale_hw[2])), anchors_hw[N, 2])
    half = Mul(s, 0.5)
    boxes = ExpandDims(ConcatV2([Sub(c, half), Add(c, half)], axis=-1), 2)

Every node of it must be consumed inside the pattern only (``boxes`` by the NMS alone) and not
be fetched, and the constants must validate: ``[N, 2]`` anchor halves (the same ``anchors_hw``
in both branches), two-element reciprocal scales, the scalar 0.5.  The group then lowers into
the ``nms`` step with ``meta["fused_decode"]``: the kernel decodes in fp32
(``ops_nn.decode_boxes_yxhw`` is the order of operations) and the encodings are never expanded
to bf16 boxes.  Otherwise the subgraph is lowered op by op and the step reads decoded boxes.
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops import kernels as K
from .plan import CompileError, Val, _root, _view

_UNPADDED_NMS = ("NonMaxSuppression", "NonMaxSuppressionV2", "NonMaxSuppressionV3", "NonMaxSuppressionV4",
                 "NonMaxSuppressionV5")
_ADD = ("Add", "AddV2")


class DetectionLowering:
    """Mixin of ``CompiledFunction`` (uses its graph, ``cons``, ``vals``, ``_fetched`` and emitters).
    It also uses the graph helpers of the ``TransformerLowering`` mixin next to it: ``_consumers``,
    ``_is_const_node``, ``_const_of`` and ``_add_group`` (a matched decode is a ``_groups`` entry
    of kind ``"decode"``, dispatched by ``_lower_group``)."""

    # ------------------------------------------------------------------ matching
    def _prematch_detection(self):
        for name in self.order:
            node = self.graph[name]
            if node.op == "CombinedNonMaxSuppression":
                grp = self._match_decode(node)
                if grp is not None:
                    self._add_group(grp)

    def _match_decode(self, nms):
        """The ``decode_boxes`` form behind ``nms``'s boxes input as a group, or None."""
        g = self.graph

        def prod(src, ops):
            n = g.nodes.get(src[0])
            return n if n is not None and src[1] == 0 and n.op in ops and n.name in self.needed else None

        def split(node):  # (activation operand, constant operand) of a binary node
            a, b = node.inputs[0], node.inputs[1]
            if self._is_const_node(b) and not self._is_const_node(a):
                return a, b
            if self._is_const_node(a) and not self._is_const_node(b) and node.op != "Sub":
                return b, a
            return None, None

        ex = prod(nms.inputs[0], ("ExpandDims",))
        cat = prod(ex.inputs[0], ("ConcatV2",)) if ex is not None else None
        if cat is None or len(cat.inputs) != 3:
            return None
        lo, hi = prod(cat.inputs[0], ("Sub",)), prod(cat.inputs[1], _ADD)
        if lo is None or hi is None or lo.inputs[0] != hi.inputs[0] or lo.inputs[1] != hi.inputs[1]:
            return None
        centre, half = prod(lo.inputs[0], _ADD), prod(lo.inputs[1], ("Mul",))
        if centre is None or half is None:
            return None
        size_src, half_c = split(half)
        size = prod(size_src, ("Mul",)) if size_src else None
        exp_src, a_hw = split(size) if size is not None else (None, None)
        ex_node = prod(exp_src, ("Exp",)) if exp_src else None
        sc_hw = prod(ex_node.inputs[0], ("Mul",)) if ex_node is not None else None
        t_hw_src, inv_hw = split(sc_hw) if sc_hw is not None else (None, None)
        off_src, a_yx = split(centre)
        off = prod(off_src, ("Mul",)) if off_src else None
        sc_src, a_hw2 = split(off) if off is not None else (None, None)
        sc_yx = prod(sc_src, ("Mul",)) if sc_src else None
        t_yx_src, inv_yx = split(sc_yx) if sc_yx is not None else (None, None)
        t_yx = prod(t_yx_src, ("StridedSlice",)) if t_yx_src else None
        t_hw = prod(t_hw_src, ("StridedSlice",)) if t_hw_src else None
        if t_yx is None or t_hw is None or t_yx.inputs[0] != t_hw.inputs[0] or a_hw2 != a_hw:
            return None
        inner = [t_yx, t_hw, sc_yx, off, centre, sc_hw, ex_node, size, half, lo, hi, cat, ex]
        members = {n.name for n in inner}
        for n in inner:  # read inside the pattern only (the boxes by the NMS alone), never fetched
            allowed = members if n is not ex else {nms.name}
            if self._fetched(n.name) or any(c not in allowed for c in self._consumers(n.name)):
                return None
        if self._consumers(ex.name) != [nms.name]:
            return None
        return {"kind": "decode", "members": members, "enc": t_yx.inputs[0], "slices": (t_yx, t_hw), "out": ex.name,
                "consts": {"a_yx": a_yx, "a_hw": a_hw, "inv_yx": inv_yx, "inv_hw": inv_hw, "half": half_c,
                           "axis": cat.inputs[2], "dim": ex.inputs[1]}}

    def _last_axis_range(self, node, shape):
        """``(lo, hi)`` when ``node`` (StridedSlice / Slice with constant bounds) keeps every
        axis of ``shape`` whole but cuts the last one to ``[lo, hi)``; else None."""
        r = len(shape)
        if node.op == "Slice":
            b, sz = (self._const_of(node.inputs[i]) for i in (1, 2))
            if b is None or sz is None or b.numel() != r or sz.numel() != r:
                return None
            b, sz = b.reshape(-1).tolist(), sz.reshape(-1).tolist()
            if any(b[d] != 0 or sz[d] not in (-1, shape[d]) for d in range(r - 1)):
                return None
            lo, hi = b[-1], shape[-1] if sz[-1] == -1 else b[-1] + sz[-1]
        elif node.op == "StridedSlice":
            b, e, s = (self._const_of(node.inputs[i]) for i in (1, 2, 3))
            if b is None or e is None or s is None or b.numel() != r:
                return None
            if any(node.attr(k, 0) for k in ("ellipsis_mask", "new_axis_mask", "shrink_axis_mask")):
                return None
            b, e, s = (t.reshape(-1).tolist() for t in (b, e, s))
            bm, em = node.attr("begin_mask", 0), node.attr("end_mask", 0)
            if any(v != 1 for v in s):
                return None
            for d in range(r - 1):
                if not (bm >> d & 1 or b[d] == 0) or not (em >> d & 1 or e[d] >= shape[d]):
                    return None
            n = shape[-1]
            lo = 0 if bm >> (r - 1) & 1 else (b[-1] + n if b[-1] < 0 else b[-1])
            hi = n if em >> (r - 1) & 1 else (e[-1] + n if e[-1] < 0 else min(e[-1], n))
        else:
            return None
        return (int(lo), int(hi)) if 0 <= lo < hi <= shape[-1] else None

    # ------------------------------------------------------------------ lowering
    def _lower_decode_group(self, grp) -> bool:
        """Validates the constants of a matched decode; on success the boxes become a value
        without a buffer (``decode_of``) that only the ``nms`` step reads."""
        enc = self._get(grp["enc"])
        c = {k: self._const_of(v) for k, v in grp["consts"].items()}
        if enc is None or enc.is_const or len(enc.shape) != 3 or enc.shape[-1] != 4 or enc.phys_c or enc.rows is not None \
                or any(v is None for v in c.values()):
            return False
        B, N, _ = enc.shape
        if any(self._last_axis_range(s, enc.shape) != r for s, r in zip(grp["slices"], ((0, 2), (2, 4)))):
            return False
        if tuple(c["a_yx"].shape) != (N, 2) or tuple(c["a_hw"].shape) != (N, 2) or c["inv_yx"].numel() != 2 \
                or c["inv_hw"].numel() != 2 or c["half"].numel() != 1 or float(c["half"].reshape(-1)[0]) != 0.5 \
                or int(c["axis"].reshape(-1)[0]) not in (-1, 2) or int(c["dim"].reshape(-1)[0]) != 2:
            return False
        anchors = torch.cat([c["a_yx"].float(), c["a_hw"].float()], dim=1).contiguous()
        scales = [float(v) for v in torch.cat([c["inv_yx"].float().reshape(-1), c["inv_hw"].float().reshape(-1)])]
        if not bool(torch.isfinite(anchors).all()) or not all(np.isfinite(scales)):
            return False
        out = self._new((B, N, 1, 4))
        out.decode_of = (enc, anchors, scales)
        self.vals[(grp["out"], 0)] = out
        return True

    def _lower_score_slice(self, node) -> bool:
        """A last-axis slice of the scores read by nothing but a ``CombinedNonMaxSuppression``:
        no step, the NMS reads the columns in place (``slice_of``)."""
        nxt = self._single_consumer(node.name)
        if nxt is None or nxt.op != "CombinedNonMaxSuppression" or nxt.inputs[1] != (node.name, 0) \
                or [s for s, _ in nxt.inputs].count(node.name) != 1:
            return False
        x = self._get(node.inputs[0])
        if x is None or x.is_const or len(x.shape) != 3 or x.rows is not None or x.pre_cfg is not None \
                or x.slice_of is not None:
            return False
        rng = self._last_axis_range(node, x.shape)
        if rng is None:
            return False
        out = self._new((*x.shape[:-1], rng[1] - rng[0]), x.dtype)
        out.slice_of = (x, rng[0])
        self.vals[(node.name, 0)] = out
        return True

    def _materialise(self, v: Val, name: str) -> Val:
        """A buffer for a value that exists only as a decode or a slice of another (the NMS that
        was to read it in place stays glue)."""
        dec, sl = v.decode_of, v.slice_of
        if dec is None and sl is None:
            return v
        src = dec[0] if dec is not None else sl[0]
        if dec is not None:
            from .ops_nn import decode_boxes_yxhw

            a_dev, s_dev = self._dev(dec[1], torch.float32), self._dev(torch.tensor(dec[2]), torch.float32)
            self.params += [a_dev, s_dev]

            def run(src=src, v=v, a=a_dev, s=s_dev):
                v.buf.copy_(decode_boxes_yxhw(_view(src), a, s)[:, :, None])
        else:
            def run(src=src, v=v, lo=sl[1]):
                v.buf.copy_(_view(src)[..., lo:lo + v.shape[-1]])
        v.decode_of = v.slice_of = None
        self._emit(name, "glue" if dec is not None else "copy", run, [src], [v])
        return v

    def _host_nms_glue(self, node):
        """The interpreter's NMS routines run on the host: no glue step on a GPU plan."""
        if self.device.type == "cuda":
            raise CompileError(f"op {node.op} ({node.name}) has no CDNA4 lowering in this form and its host routine "
                               "cannot be part of a GPU plan (it runs on the interpreter)")
        return self._lower_glue(node)

    def _nms_glue(self, node):
        if self.device.type == "cuda":
            return self._host_nms_glue(node)
        for i in (0, 1):
            v = self.vals.get(node.inputs[i])
            if v is not None and not self.strict:
                self._materialise(v, f"{node.name}/in{i}")
        return self._lower_glue(node)

    def _lower_unpadded_nms(self, node):
        if node.op in ("NonMaxSuppressionV4", "NonMaxSuppressionV5") and node.attr("pad_to_max_output_size", False):
            return self._host_nms_glue(node)
        raise CompileError(f"{node.op} ({node.name}) has a data-dependent output shape: no compiled plan can hold it "
                           "(pad_to_max_output_size, CombinedNonMaxSuppression, or the interpreter)")

    def _lower_combined_nms(self, node):
        boxes, scores = self._in(node, 0), self._in(node, 1)
        scal = [self._get(node.inputs[i]) for i in (2, 3, 4, 5)]
        if any(s is None or not s.is_const for s in scal) or boxes.is_const or scores.is_const \
                or len(boxes.shape) != 4 or len(scores.shape) != 3 or boxes.rows is not None or scores.rows is not None:
            return self._nms_glue(node)
        mpc, T = (int(s.const.reshape(-1)[0]) for s in scal[:2])
        iou_thr, score_thr = (float(s.const.reshape(-1)[0]) for s in scal[2:])
        B, N, C = scores.shape
        pad, clip = bool(node.attr("pad_per_class", False)), bool(node.attr("clip_boxes", True))
        if mpc < 1 or T < 1 or tuple(boxes.shape[:2]) != (B, N) or boxes.shape[3] != 4:
            return self._nms_glue(node)
        T = min(T, mpc * C) if pad else T
        if not K.nms_eligible(N, C, min(mpc, N), T, q=boxes.shape[2]):
            return self._nms_glue(node)
        # scores: read in place through a pitch and a class offset
        src, coff = scores.slice_of or (scores, 0)
        if src.qscale is not None or src.dtype not in (torch.bfloat16, torch.float32):
            if src.dtype not in (torch.bfloat16, torch.float32, torch.uint8) or src.phys_c:
                return self._nms_glue(node)
            src = self._as_bf16(src, node.name + "/scores")
        if src.phys_c and src is not _root(src):
            return self._nms_glue(node)
        ld = src.phys_c or src.shape[-1]
        # boxes: a fused decode of the encodings, or decoded corners
        dec = boxes.decode_of
        bsrc = dec[0] if dec is not None else boxes
        if bsrc.phys_c or (bsrc.qscale is None and bsrc.dtype not in (torch.bfloat16, torch.float32)):
            return self._nms_glue(node)
        if bsrc.qscale is not None:
            bsrc = self._as_bf16(bsrc, node.name + "/boxes")
        a_dev = None
        if dec is not None:
            a_dev = self._dev(dec[1], torch.float32)
            self.params.append(a_dev)
        outs = [self._new((B, T, 4), torch.float32), self._new((B, T), torch.float32), self._new((B, T), torch.float32),
                self._new((B,), torch.int32)]
        scratch = self._new((K.nms_scratch_numel(B, C, min(mpc, N)),), torch.int64)

        def run(bsrc=bsrc, src=src, outs=outs, scratch=scratch, a_dev=a_dev, scales=dec[2] if dec is not None else None):
            sbuf = _root(src).buf if src.phys_c else _view(src)
            K.combined_nms(_view(bsrc).reshape(B, N, 4), sbuf.reshape(B, N, ld), mpc, T, iou_thr, score_thr, False, clip,
                           anchors=a_dev, box_scales=scales, num_classes=C, class_offset=coff,
                           out=tuple(o.buf for o in outs), scratch=scratch.buf)

        self._emit(node.name, "nms", run, [bsrc, src], outs + [scratch],
                   {"fused_decode": dec is not None, "class_offset": coff, "pitch": ld})
        for k, o in enumerate(outs):
            self.vals[(node.name, k)] = o
