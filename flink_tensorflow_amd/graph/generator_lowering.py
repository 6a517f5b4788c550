"""Lowering of the generator-network ops (a mixin of ``CompiledFunction``): instance
normalisation, spatial pads and the image output stage of style-transfer / CycleGAN / pix2pix
generators, onto ``kernels/instnorm.hip`` and ``kernels/pad.hip``.

**Instance norm.**  ``tf.contrib.layers.instance_norm`` exports ``nn.moments(x, [1, 2],
keep_dims=True)`` + ``nn.batch_normalization``: the node pattern ``TransformerLowering._match_ln``
matches for BERT's last-axis ``layer_norm``, with other axes.  A matched ``ln`` group becomes one
``instnorm`` step when

* both ``Mean`` axes are ``[1, 2]`` with ``keep_dims`` over a 4-D NHWC activation (bf16; fp32 feeds
  and fp8 values through ``_as_bf16``) that is not channel-padded;
* ``gamma`` / ``beta`` are constants of ``C`` elements shaped ``[C]`` or ``[1, 1, 1, C]``;
* the shape passes ``K.instance_norm_eligible`` (``C % 8 == 0``).

A ``Relu`` / ``Relu6`` that is the sole reader becomes the step's activation; a sole ``ConcatV2``
reader gets the slice written in place (``"instnorm"`` is a concat-writable step kind; the norm's
own input is never a concat slot, since the kernel reads a buffer of pitch ``C``:
``CompiledFunction._norm_group_reads``); a residual
``Add`` behind it stays an ``elementwise`` step.  The step's fp32 scratch (per-chunk partials and the
per-image statistics) is a value of the plan's slab.  Any other axes go to
``TransformerLowering._lower_ln_group`` unchanged, so last-axis groups still become ``layernorm``
steps; a channel-padded input, a fed ``gamma`` (the matcher wants constants), the hand-written
``(x - mu) / sqrt(var + eps)`` form and the reshape-based group norm stay glue ops.

**Pad.**  ``MirrorPad`` (``REFLECT`` / ``SYMMETRIC``) and ``Pad`` / ``PadV2`` become one ``pad`` step
when the value is a 4-D activation (bf16; fp32 feeds and fp8 values through ``_as_bf16``; a
channel-padded one is copied at its physical width and the result is padded the same way), the
paddings (and the ``PadV2`` value) are constants and only the two spatial axes are padded, within
TF's bounds for the mode.  It writes a concat slot when only
a ``ConcatV2`` reads it.  A padded batch or channel axis or fed ``paddings`` stay glue.  A zero
``Pad`` is not folded into the next conv's padding.

**Image output.**  ``[Tanh | Sigmoid] → [Mul(scalar)] → [Add | Sub(scalar)] → [ClipByValue(consts)] →
[Cast(UINT8)]`` behind a conv / deconv output of 1, 3 or 4 logical channels (stored over a padded
buffer) becomes one ``image_out`` step that writes the compact fp32 or uint8 image.  Every link is
read only by the next and only the end may be fetched; the chain must hold a ``Mul``, ``Add`` /
``Sub`` or ``ClipByValue`` (a bare activation stays what it was); the ``Cast`` is absorbed only
behind a clamp inside ``[0, 255]``.  A ``Conv2D`` chain leaves a ``Tanh`` / ``Sigmoid`` that heads
such a chain to this step (``_image_out_keeps``), so it is applied in fp32 and not rounded to bf16.

In an fp8 plan all three run bf16 (on ``_as_bf16(x)``), like ``dwconv``, ``resize`` and ``deconv``.
"""
from __future__ import annotations

import torch

from ..ops import kernels as K
from ..types.dtypes import DataType
from .conv_lowering import _DW_ACTS
from .plan import _coff, _root, _target

_PAD_OPS = ("Pad", "PadV2", "MirrorPad")
_IMAGE_OUT_OPS = ("Tanh", "Sigmoid", "Mul", "Add", "AddV2", "Sub", "ClipByValue")
_IMAGE_OUT_ACTS = {"Tanh": "tanh", "Sigmoid": "sigmoid"}


class GeneratorLowering:
    """Mixin of ``CompiledFunction`` (uses its values, emitters and the ``ln`` groups of
    ``TransformerLowering``; it precedes that mixin in the MRO)."""

    # ------------------------------------------------------------------ instance norm
    def _instnorm_axes(self, grp) -> bool:
        """Both reductions of the ``ln`` group run over axes ``[1, 2]`` of a 4-D value."""
        x = self._get(grp["x"])
        if x is None or len(x.shape) != 4:
            return False
        for a in grp["axes"]:
            c = self._const_of(a)
            if c is None or sorted(int(v) % 4 for v in c.reshape(-1).tolist()) != [1, 2]:
                return False
        return True

    def _lower_ln_group(self, grp) -> bool:
        if self._instnorm_axes(grp):
            return self._lower_instnorm_group(grp)
        return super()._lower_ln_group(grp)

    def _plain_activation(self, x, preprocessed: bool = False) -> bool:
        """A 4-D activation on a buffer of its own shape that ``_as_bf16`` can hand to a kernel.
        With ``preprocessed`` the fused preprocess kernel's output counts too, while it is the
        channel-padded NHWC image (a stem conv that were its only reader could still make it
        space-to-depth; a second reader, as the step asking here, rules that out: ``_s2d_ok``)."""
        if x is None or x.is_const or len(x.shape) != 4 or x.rows is not None or x.alias_of is not None \
                or x.concat_slot is not None:
            return False
        if x.pre_cfg is not None:
            if not preprocessed or x.pre_cfg["s2d"] or tuple(x.buf_shape) != (*x.shape[:-1], x.phys_c):
                return False
        elif x.buf_shape:
            return False
        return x.dtype in (torch.bfloat16, torch.float32) or x.qscale is not None

    def _lower_instnorm_group(self, grp) -> bool:
        x = self._get(grp["x"])
        gamma, beta, eps = (self._const_of(grp[k]) for k in ("gamma", "beta", "eps"))
        if not self._plain_activation(x) or x.phys_c or any(t is None for t in (gamma, beta, eps)):
            return False
        N, H, W, C = x.shape
        means = [self.graph[m] for m in grp["members"] if self.graph[m].op == "Mean"]
        if len(means) != 2 or not all(m.attr("keep_dims", False) for m in means):
            return False
        if any(tuple(t.shape) not in ((C,), (1, 1, 1, C)) for t in (gamma, beta)) or eps.numel() != 1 \
                or not K.instance_norm_eligible(H, W, C):
            return False
        out_name = grp["out"]
        act, relu = K.ACT_NONE, self._single_consumer(out_name)
        if relu is not None and relu.op in _DW_ACTS:
            act = _DW_ACTS[relu.op]
        else:
            relu = None
        xin = self._as_bf16(x, out_name)
        g_dev = self._dev(gamma.float().reshape(-1), torch.float32)
        b_dev = self._dev(beta.float().reshape(-1), torch.float32)
        self.params += [g_dev, b_dev]
        out = self._new(x.shape)
        scratch = self._new((K.instance_norm_scratch_numel(N, H, W, C),), torch.float32)
        eps = float(eps.float().reshape(-1)[0])

        def run(xin=xin, out=out, scratch=scratch, g=g_dev, b=b_dev):
            K.instance_norm(xin.buf, g, b, eps, act, out=_target(out), out_channel_offset=_coff(out), scratch=scratch.buf)

        self._emit(out_name, "instnorm", run, [xin], [out, scratch], {"multi_out": True, "act": act})
        self.vals[(out_name, 0)] = out
        if relu is not None:
            self._fused.add(relu.name)
            self.vals[(relu.name, 0)] = out
        return True

    # ------------------------------------------------------------------ pad
    def _lower_pad(self, node):
        # as a glue op the paddings and the PadV2 value stay on the host: the op reads them into Python
        x = self._get(node.inputs[0])
        pv = self._get(node.inputs[1])
        if not self._plain_activation(x, preprocessed=True) or pv is None or not pv.is_const \
                or (x.dtype != torch.bfloat16 and x.phys_c):
            return self._lower_glue(node, host_consts=(1, 2))
        p = [int(v) for v in pv.const.reshape(-1).tolist()]
        phys = x.phys_c or x.shape[-1]
        if len(p) != 8 or any(p[:2] + p[6:]) or min(p) < 0 or phys % 8:
            return self._lower_glue(node, host_consts=(1, 2))
        pads = tuple(p[2:6])  # (top, bottom, left, right)
        value = 0.0
        if node.op == "MirrorPad":
            mode = node.attr("mode", "REFLECT")
            mode = (mode.decode() if isinstance(mode, bytes) else mode).lower()
            lim = 1 if mode == "reflect" else 0
            if mode not in ("reflect", "symmetric") or max(pads[:2]) > x.shape[1] - lim or max(pads[2:]) > x.shape[2] - lim:
                return self._lower_glue(node, host_consts=(1, 2))  # the interpreter op raises TF's error when the glue step is sized
        else:
            mode = "constant"
            if node.op == "PadV2":
                cv = self._get(node.inputs[2])
                if cv is None or not cv.is_const or cv.const.numel() != 1:
                    return self._lower_glue(node, host_consts=(1, 2))
                value = float(cv.const.float().reshape(-1)[0])
        N, H, W, C = x.shape
        x = self._as_bf16(x, node.name)
        out = self._new((N, H + pads[0] + pads[1], W + pads[2] + pads[3], C), phys_c=x.phys_c)

        def run(x=x, out=out):
            K.pad_nhwc(x.buf, pads, mode, value, out=_target(out), out_channel_offset=_coff(out), channels=C)

        self._emit(node.name, "pad", run, [x], [out], {"mode": mode})
        self.vals[(node.name, 0)] = out

    # ------------------------------------------------------------------ image output
    def _scalar_operand(self, node, data_src):
        """``(value, position of the data input)`` of a binary ``node`` whose other operand is a
        one-element constant, or None."""
        pos = [i for i, s in enumerate(node.inputs) if s == data_src]
        if len(node.inputs) != 2 or len(pos) != 1:
            return None
        c = self._const_of(node.inputs[1 - pos[0]])
        if not isinstance(c, torch.Tensor) or c.numel() != 1:
            return None
        return float(c.float().reshape(-1)[0]), pos[0]

    def _match_image_out(self, first):
        """The image-output chain that starts at graph node ``first``: a dict of its links and
        parameters, or None when it holds no ``Mul`` / ``Add`` / ``Sub`` / ``ClipByValue``."""
        m = {"links": [], "act": None, "scale": 1.0, "offset": 0.0, "clamp": None, "dtype": torch.float32}
        stage, node, src = 0, first, first.inputs[0] if first.inputs else None
        if first.op in ("Mul", "Add", "AddV2"):  # the data operand of a commutative link: the non-constant one
            src = next((s for s in first.inputs if self._const_of(s) is None), None)
        while node is not None and src is not None:
            if node.op in _IMAGE_OUT_ACTS and stage < 1 and node.inputs[0] == src:
                m["act"], stage = _IMAGE_OUT_ACTS[node.op], 1
            elif node.op == "Mul" and stage < 2 and self._scalar_operand(node, src) is not None:
                m["scale"], stage = self._scalar_operand(node, src)[0], 2
            elif node.op in ("Add", "AddV2") and stage < 3 and self._scalar_operand(node, src) is not None:
                m["offset"], stage = self._scalar_operand(node, src)[0], 3
            elif node.op == "Sub" and stage < 3 and (self._scalar_operand(node, src) or (0, 1))[1] == 0:
                m["offset"], stage = -self._scalar_operand(node, src)[0], 3
            elif node.op == "ClipByValue" and stage < 4 and len(node.inputs) == 3 and node.inputs[0] == src:
                lo, hi = (self._const_of(node.inputs[i]) for i in (1, 2))
                if not all(isinstance(t, torch.Tensor) and t.numel() == 1 for t in (lo, hi)):
                    break
                lo, hi = float(lo.float().reshape(-1)[0]), float(hi.float().reshape(-1)[0])
                if not lo <= hi:
                    break
                m["clamp"], stage = (lo, hi), 4
            elif node.op == "Cast" and stage == 4 and DataType.of(node.attr("DstT")).torch == torch.uint8 \
                    and m["clamp"][0] >= 0.0 and m["clamp"][1] <= 255.0:
                m["dtype"], stage = torch.uint8, 5
            else:
                break
            m["links"].append(node)
            src = (node.name, 0)
            node = self._single_consumer(node.name) if stage < 5 else None
        if not any(n.op not in _IMAGE_OUT_ACTS for n in m["links"]):
            return None
        return m

    def _image_out_keeps(self, start, act_node) -> bool:
        """A ``Conv2D`` chain from ``start`` leaves ``act_node`` (``Tanh`` / ``Sigmoid``) alone: it
        heads an image-output chain of a 1, 3 or 4 channel conv."""
        if act_node.op not in _IMAGE_OUT_ACTS or start.op != "Conv2D":
            return False
        w = self._const_of(start.inputs[1])
        if not isinstance(w, torch.Tensor) or w.dim() != 4 or int(w.shape[3]) not in (1, 3, 4):
            return False
        return self._match_image_out(act_node) is not None

    def _lower_image_out(self, node) -> bool:
        if node.op in _IMAGE_OUT_ACTS or node.op in ("Sub", "ClipByValue"):
            src = node.inputs[0]
        else:
            src = next((s for s in node.inputs if s in self.vals and not self.vals[s].is_const), None)
        x = self.vals.get(src) if src is not None else None
        if not self._plain_activation(x) or x.dtype != torch.bfloat16 or not x.phys_c or x.phys_c % 8 \
                or x.shape[-1] not in (1, 3, 4):
            return False
        prods = [s for s in self.steps if any(o is x for o in s.outputs)]
        if len(prods) != 1 or prods[0].kind not in ("conv", "deconv"):
            return False
        m = self._match_image_out(node)
        if m is None:
            return False
        out = self._new(x.shape, m["dtype"])
        act, scale, offset, clamp, Cl = m["act"], m["scale"], m["offset"], m["clamp"], x.shape[-1]

        def run(x=x, out=out):
            K.image_out(_root(x).buf, Cl, act, scale, offset, clamp, out=out.buf)

        self._emit(m["links"][-1].name, "image_out", run, [x], [out], {"act": act, "dtype": str(m["dtype"])})
        for n in m["links"]:
            self._fused.add(n.name)
            self.vals[(n.name, 0)] = out
        return True
