"""Lowering of video models (a mixin of ``CompiledFunction``): ``Conv3D`` chains, ``MaxPool3D`` /
``AvgPool3D``, the 5-D ``Mean`` and the uint8 clip prefix, on ``kernels/conv3d.hip``.

**The chain.**  ``Conv3D → [BiasAdd | inference FusedBatchNorm*]* → [Relu | Relu6]`` becomes one
``conv3d`` step (``meta["impl"]`` = ``"conv3d"``); the BN scale of output channel ``co`` multiplies
``w[..., co]``.  It lowers when

* the filter is a constant ``[KD, KH, KW, Cin, Cout]``;
* the input is a 5-D ``NDHWC`` activation or feed, bf16 (fp32 feeds and fp8 values through
  ``_as_bf16``);
* the padding is ``SAME`` or ``VALID``, dilations are 1, the batch and channel strides are 1;
* the shape passes ``K.conv3d_eligible``: filter extents 1..7, strides 1..4 (channels are made
  multiples of 8 here, see below).

``Cout`` that is no multiple of 8 is zero-padded: the value keeps its logical shape over a padded
buffer (``phys_c``), as ``_lower_conv`` and ``_lower_deconv`` do.  ``Cin`` that is no multiple of
8 (RGB) goes through ``_ensure_padded``; a channel-padded input is read in place against zero
filter rows.  ``Sigmoid`` / ``Tanh`` end the chain and stay elementwise steps; a residual ``Add``
stays its own step.

**A 3-D conv that is really 2-D** emits no ``conv3d`` step.  A 5-D ``NDHWC`` buffer is also a 4-D
NHWC one over the same memory: ``KD == 1`` with depth stride 1 is the 2-D conv of ``[N * D, H, W,
C]``, and ``KH == KW == 1`` with spatial strides 1 is the 2-D conv of ``[N, D, H * W, C]`` with a
``(KD, 1)`` filter and stride ``(sd, 1)``.  Both lower through ``_prepare_conv`` /
``select_conv_kernel`` as ``conv`` steps over alias values, so R(2+1)D and the separable blocks of
S3D run on the tuned 2-D kernels.  Only unpadded values route (``Cin % 8 == 0``, ``Cout % 8 ==
0``, no ``phys_c``), and a conv whose result only a last-axis ``ConcatV2`` reads stays on the
``conv3d`` kernel, which writes its concat slice: an alias value cannot own one.

**Pools.**  ``MaxPool3D`` / ``AvgPool3D`` become one ``pool3d`` step when ``C % 8 == 0`` and
``K.pool3d_eligible`` passes (window and strides 1..8).  **Mean.**  ``Mean(axes=[1, 2, 3])`` of a
5-D value becomes the ``gap`` step over the ``[N, D, H * W, C]`` view.  **ConcatV2** on the last
axis of 5-D values produced by ``conv3d`` / ``pool3d`` steps has them write their channel slices
(the I3D module), as the 4-D concat does.

**uint8 clips.**  A ``Cast(UINT8 → FLOAT)`` of a 5-D feed that only a ``Mul`` / ``RealDiv`` by a
scalar constant reads, which in turn only one lowered ``Conv3D`` reads, emits no step: the
scalar folds into that conv's filter and the cast happens in its ``pad_cin`` copy (0..255 are
exact in bf16), so the plan's feed is the raw uint8 frames, a quarter of the H2D bytes.  A
second reader anywhere in that prefix leaves it to the existing paths.

**What stays glue** (a ``CompileError`` under ``strict``): a non-constant filter, ``NCDHW``,
dilations above 1, a filter extent above 7 or a stride above 4 that does not route to 2-D,
``C % 8 != 0`` for a pool, a pool window above 8.

In an fp8 plan these steps run bf16 on ``_as_bf16(x)``, like ``dwconv``, ``resize`` and ``deconv``.
"""
from __future__ import annotations

import torch

from ..ops import kernels as K
from ..types.dtypes import DataType
from .conv_lowering import _DW_ACTS, select_conv_kernel
from .ops_nn import conv_out_size, same_pads
from .plan import Val, _coff, _target


class Conv3DLowering:
    """Mixin of ``CompiledFunction`` (uses its values, emitters and the ``ConvLowering`` chain
    helpers)."""

    def _conv3d_geometry(self, node, xshape):
        """``(w [KD, KH, KW, Cin, Cout] fp32, strides, pads (front, back, top, bottom, left, right),
        (Do, Ho, Wo))`` of a ``Conv3D`` over an input of ``xshape`` that lowers, or None."""
        wv = self._get(node.inputs[1])
        if wv is None or not wv.is_const or len(wv.const.shape) != 5 or len(xshape) != 5:
            return None
        if node.attr("data_format", "NDHWC") != "NDHWC" or node.attr("padding", "SAME") not in ("SAME", "VALID"):
            return None
        strides = [int(v) for v in node.attr("strides") or [1] * 5]
        if len(strides) != 5 or strides[0] != 1 or strides[4] != 1 \
                or tuple(node.attr("dilations") or [1] * 5) != (1, 1, 1, 1, 1):
            return None  # the interpreter op raises TF's error when the glue step is sized
        w = wv.const.float()
        k, s, ext = tuple(w.shape[:3]), tuple(strides[1:4]), tuple(xshape[1:4])
        if xshape[4] != w.shape[3]:
            return None
        padding = node.attr("padding", "SAME")
        pads = tuple(p for i in range(3) for p in (same_pads(ext[i], k[i], s[i]) if padding == "SAME" else (0, 0)))
        out = tuple(conv_out_size(ext[i], k[i], s[i], padding) for i in range(3))
        routes = (k[0] == 1 and s[0] == 1) or (k[1:] == (1, 1) and s[1:] == (1, 1))
        if min(out) < 1 or not (routes or K.conv3d_eligible(8, 8, k, s)):
            return None
        return w, s, pads, out

    def _conv3d_input_ok(self, x) -> bool:
        if x is None or x.is_const or len(x.shape) != 5 or x.pre_cfg is not None or x.rows is not None or x.buf_shape:
            return False
        return x.u8_of is not None or x.dtype in (torch.bfloat16, torch.float32) or x.qscale is not None

    def _lower_conv3d(self, node):
        x = self._in(node, 0)
        geo = self._conv3d_geometry(node, x.shape) if self._conv3d_input_ok(x) else None
        if geo is None:
            return self._lower_glue(node)
        w, s, pads, (Do, Ho, Wo) = geo
        KD, KH, KW, Cin, Cout = w.shape
        N, D, H, W, _ = x.shape
        last, scale, bias, _, act, absorbed = self._conv_chain(node, absorb_residual=False, acts=_DW_ACTS)
        if scale is not None:
            w = w * scale
        n_pad = -(-Cout // 8) * 8
        # the 2-D routes: unpadded values only, and not a concat branch (an alias owns no slot)
        plain = x.u8_of is None and not x.phys_c and Cin % 8 == 0 and n_pad == Cout and not self._only_concat_reads(last)
        if plain and KD == 1 and s[0] == 1:
            return self._lower_conv3d_as_conv(node, x, w[0], bias, act, last, absorbed, (N * D, H, W, Cin), s[1:],
                                              pads[2:], (Ho, Wo), (N, Do, Ho, Wo, Cout))
        if plain and (KH, KW) == (1, 1) and s[1:] == (1, 1):
            return self._lower_conv3d_as_conv(node, x, w[:, 0], bias, act, last, absorbed, (N, D, H * W, Cin), (s[0], 1),
                                              (pads[0], pads[1], 0, 0), (Do, H * W), (N, Do, Ho, Wo, Cout))
        if not K.conv3d_eligible(8, 8, (KD, KH, KW), s):
            return self._lower_glue(node)
        if n_pad != Cout:
            w = torch.nn.functional.pad(w, (0, n_pad - Cout))
            bias = torch.nn.functional.pad(bias if bias is not None else torch.zeros(Cout), (0, n_pad - Cout))
        if x.u8_of is not None:
            x, factor = x.u8_of  # the raw uint8 feed: cast by the pad_cin copy, scaled by the filter
            w = w * factor
        else:
            x = self._as_bf16(x, node.name)
        cin_phys = -(-((x.phys_c or Cin) if x.dtype == torch.bfloat16 else Cin) // 8) * 8
        if cin_phys != Cin:
            w = torch.nn.functional.pad(w, (0, 0, 0, cin_phys - Cin))  # zero filter rows against the padding columns
        w_dev = self._dev(K.conv3d_pack_weights(w), torch.bfloat16)
        b_dev = self._dev(bias if bias is not None else torch.zeros(n_pad), torch.float32)
        self.params += [w_dev, b_dev]
        xin = self._ensure_padded(x, cin_phys, node.name)
        out = self._new((N, Do, Ho, Wo, Cout), phys_c=n_pad if n_pad != Cout else None)
        for a in absorbed:
            self._fused.add(a.name)
        kernel = (KD, KH, KW)

        def run(xin=xin, out=out, w_dev=w_dev, b_dev=b_dev):
            K.conv3d_ndhwc(xin.buf, w_dev, b_dev, kernel, s, pads, act, out=_target(out), out_channel_offset=_coff(out))

        self._emit(node.name, "conv3d", run, [xin], [out], {"impl": "conv3d"})
        self._finish_conv(last, absorbed, out)

    def _only_concat_reads(self, last) -> bool:
        nxt = self._single_consumer(last.name)
        return nxt is not None and nxt.op == "ConcatV2"

    def _lower_conv3d_as_conv(self, node, x, w_hwio, bias, act, last, absorbed, x4_shape, stride, pads, out_hw, out5_shape):
        """A 3-D conv that is a 2-D one over the same memory: the input as the 4-D alias
        ``x4_shape``, the result a 5-D alias of the ``conv`` step's 4-D output."""
        xb = self._as_bf16(x, node.name)
        x4 = Val(tuple(x4_shape), xb.dtype, alias_of=xb)
        self.vals[(node.name + "/as_nhwc", 0)] = x4
        c = self._prepare_conv(node, x4, w_hwio.contiguous(), bias, None, act, last, absorbed, tuple(stride), tuple(pads),
                               (1, 1), tuple(out_hw))
        impl = select_conv_kernel(c.site)
        {"dconv": self._emit_dconv, "conv3x3c64": self._emit_conv3x3c64, "gemm_pp": self._emit_gemm_pp,
         "conv_lite": self._emit_conv_lite, "igemm": self._emit_igemm}[impl](c)
        out4 = self.vals[(last.name, 0)]
        self._finish_conv(last, absorbed, Val(tuple(out5_shape), out4.dtype, alias_of=out4))

    # ---- pools / mean
    def _lower_pool3d(self, node):
        x = self._in(node, 0)
        k, s = node.attr("ksize"), node.attr("strides")
        if (node.attr("data_format", "NDHWC") != "NDHWC" or x.is_const or len(x.shape) != 5 or x.phys_c or x.u8_of is not None
                or k is None or s is None or len(k) != 5 or len(s) != 5 or (k[0], k[4], s[0], s[4]) != (1, 1, 1, 1)
                or not K.pool3d_eligible(x.shape[-1], tuple(k[1:4]), tuple(s[1:4]))
                or node.attr("padding", "VALID") not in ("SAME", "VALID")
                or not (x.dtype in (torch.bfloat16, torch.float32) or x.qscale is not None)):
            return self._lower_glue(node)
        k, s = tuple(int(v) for v in k[1:4]), tuple(int(v) for v in s[1:4])
        N, C, ext = x.shape[0], x.shape[4], x.shape[1:4]
        padding = node.attr("padding", "VALID")
        pads = tuple(p for i in range(3) for p in (same_pads(ext[i], k[i], s[i]) if padding == "SAME" else (0, 0)))
        O = tuple(conv_out_size(ext[i], k[i], s[i], padding) for i in range(3))
        if min(O) < 1:
            return self._lower_glue(node)
        mode = "max" if node.op == "MaxPool3D" else "avg"
        xin = self._as_bf16(x, node.name)
        out = self._new((N, *O, C))

        def run(xin=xin, out=out):
            K.pool3d_ndhwc(xin.buf, k, s, pads, mode, out=_target(out), out_channel_offset=_coff(out))

        self._emit(node.name, "pool3d", run, [xin], [out])
        self.vals[(node.name, 0)] = out

    def _lower_mean3d(self, node) -> bool:
        """``Mean(axes=[1, 2, 3])`` of a 5-D value: the global average pool over ``D * H * W``."""
        x = self._in(node, 0)
        av = self._get(node.inputs[1])
        if av is None or not av.is_const or x.is_const or len(x.shape) != 5 or x.phys_c or x.u8_of is not None:
            return False
        if sorted(int(a) % 5 for a in av.const.reshape(-1).tolist()) != [1, 2, 3] or x.shape[-1] % 8:
            return False
        N, D, H, W, C = x.shape
        out = self._new((N, 1, 1, 1, C) if node.attr("keep_dims", False) else (N, C))
        xin = self._as_bf16(x, node.name)

        def run(xin=xin, out=out):
            K.global_avgpool(xin.buf.view(N, D, H * W, C), out=out.buf.view(N, C))

        self._emit(node.name, "gap", run, [xin], [out])
        self.vals[(node.name, 0)] = out
        return True

    # ---- uint8 clips
    def _lower_clip_cast(self, cast) -> bool:
        """``Cast(UINT8 → FLOAT) → Mul | RealDiv (scalar) → Conv3D`` over a 5-D feed, each read by
        the next only: no step; the conv reads the feed (``Val.u8_of``)."""
        src = cast.inputs[0]
        x = self.vals.get(src)
        if x is None or x.is_const or x.dtype != torch.uint8 or x.qscale is not None or len(x.shape) != 5 \
                or f"{src[0]}:{src[1]}" not in self.feed_names or self.cons.get(src[0], []) != [cast.name] \
                or DataType.of(cast.attr("DstT")).torch != torch.float32:
            return False
        mul = self._single_consumer(cast.name)
        if mul is None or mul.op not in ("Mul", "RealDiv") or len(mul.inputs) != 2:
            return False
        ci = [i for i, (n, _) in enumerate(mul.inputs) if n == cast.name]
        if len(ci) != 1 or (mul.op == "RealDiv" and ci[0] != 0):
            return False
        cv = self._get(mul.inputs[1 - ci[0]])
        if cv is None or not cv.is_const or not isinstance(cv.const, torch.Tensor) or cv.const.numel() != 1:
            return False
        conv = self._single_consumer(mul.name)
        if conv is None or conv.op != "Conv3D" or conv.inputs[0][0] != mul.name or conv.inputs[1][0] == mul.name \
                or self._conv3d_geometry(conv, x.shape) is None \
                or not K.conv3d_eligible(8, 8, tuple(self._get(conv.inputs[1]).const.shape[:3]),
                                         tuple(conv.attr("strides")[1:4])):
            return False
        c = float(cv.const.reshape(-1)[0].item())
        v = Val(tuple(x.shape), torch.float32)
        v.u8_of = (x, c if mul.op == "Mul" else 1.0 / c)
        self.vals[(cast.name, 0)] = v
        self.vals[(mul.name, 0)] = v
        self._fused.add(mul.name)
        return True
