"""Lowering of transposed convolutions (a mixin of ``CompiledFunction``): a
``Conv2DBackpropInput`` chain to one step on ``kernels/deconv.hip``.

**The chain.**  ``Conv2DBackpropInput → [BiasAdd | inference FusedBatchNorm*]* → [Relu | Relu6]``
becomes one ``deconv`` step (``meta["phases"]`` = ``sh * sw``, ``meta["impl"]`` = ``"deconv"``);
the BN scale of output channel ``co`` multiplies ``w[:, :, co, :]``.  It lowers when

* the filter and ``input_sizes`` are constants (the 4-vector or TF's 2-vector ``[Ho, Wo]``);
* the input is a 4-D NHWC activation, bf16 (fp32 feeds and fp8 values through ``_as_bf16``);
* dilations are 1 and the padding is ``SAME`` or ``VALID``;
* the shape passes ``K.deconv_eligible``: ``Cin % 8 == 0`` (of the input *buffer*: a
  channel-padded input is read in place against zero filter rows), a filter of at most 8x8,
  strides 1..4.

``Cout`` that is no multiple of 8 (a 3-channel autoencoder output) is zero-padded: the value
keeps its logical shape over a padded buffer (``phys_c``), as ``_lower_conv`` does.  ``Sigmoid`` /
``Tanh`` end the chain and stay elementwise steps; a residual ``Add`` stays its own step.  An
up-conv that only a ``ConcatV2`` reads writes its channel slice of the concat buffer.

**Stride (1, 1)** emits no ``deconv`` step: it is the plain convolution with the spatially
flipped, channel-transposed filter and pads ``(KH - 1 - pt, ...)``, lowered through
``_prepare_conv`` / ``select_conv_kernel`` as a ``conv`` step.

**What stays glue** (a ``CompileError`` under ``strict``): a non-constant filter, a computed
``input_sizes`` (Keras's ``Shape → StridedSlice → Pack``), dilations above 1, explicit paddings,
NCHW, ``Cin % 8 != 0`` of an unpadded input, a filter above 8x8, a stride above 4.

In an fp8 plan the step runs bf16 on ``_as_bf16(x)``, like ``dwconv`` and ``resize``.
"""
from __future__ import annotations

import torch

from ..ops import kernels as K
from .conv_lowering import _DW_ACTS, select_conv_kernel
from .ops_nn import conv_out_size, same_pads
from .plan import _coff, _target


class DeconvLowering:
    """Mixin of ``CompiledFunction`` (uses its values, emitters and the ``ConvLowering`` chain
    helpers)."""

    def _deconv_geometry(self, node):
        """``(x, w [KH, KW, Cout, Cin] fp32, (sh, sw), padding, (Ho, Wo))`` of a
        ``Conv2DBackpropInput`` the kernels take, or None (it runs as a glue op)."""
        sv, wv, x = (self._get(node.inputs[i]) for i in range(3))
        if sv is None or not sv.is_const or wv is None or not wv.is_const or x is None or x.is_const:
            return None
        if node.attr("data_format", "NHWC") != "NHWC" or len(x.shape) != 4 or len(wv.const.shape) != 4:
            return None
        if x.pre_cfg is not None or x.rows is not None or x.buf_shape:
            return None
        if not (x.dtype in (torch.bfloat16, torch.float32) or x.qscale is not None):
            return None
        padding = node.attr("padding", "SAME")
        if padding not in ("SAME", "VALID") or tuple(node.attr("dilations") or [1, 1, 1, 1]) != (1, 1, 1, 1):
            return None
        strides = node.attr("strides")
        sh, sw = strides[1], strides[2]
        sizes = [int(v) for v in sv.const.reshape(-1).tolist()]
        if len(sizes) not in (2, 4):
            return None
        Ho, Wo = sizes[1:3] if len(sizes) == 4 else sizes
        w = wv.const.float()
        KH, KW, Cout, Cin = w.shape
        N, Hi, Wi, C = x.shape
        if C != Cin or Ho < 1 or Wo < 1 or (len(sizes) == 4 and (sizes[0], sizes[3]) != (N, Cout)) \
                or (conv_out_size(Ho, KH, sh, padding), conv_out_size(Wo, KW, sw, padding)) != (Hi, Wi):
            return None  # the interpreter op raises TF's error when the glue step is sized
        return x, w, (sh, sw), padding, (Ho, Wo)

    def _lower_deconv(self, node):
        geo = self._deconv_geometry(node)
        if geo is None:
            return self._lower_glue(node, host_consts=(0,))  # input_sizes is read on the host
        x, w, (sh, sw), padding, (Ho, Wo) = geo
        KH, KW, Cout, Cin = w.shape
        N = x.shape[0]
        cin_phys = (x.phys_c or Cin) if x.dtype == torch.bfloat16 else Cin
        n_pad = -(-Cout // 8) * 8
        if not K.deconv_eligible(cin_phys, n_pad, KH, KW, (sh, sw)):
            return self._lower_glue(node, host_consts=(0,))
        pt = same_pads(Ho, KH, sh)[0] if padding == "SAME" else 0
        pl = same_pads(Wo, KW, sw)[0] if padding == "SAME" else 0
        last, scale, bias, _, act, absorbed = self._conv_chain(node, absorb_residual=False, acts=_DW_ACTS)
        if scale is not None:
            w = w * scale[:, None]
        if n_pad != Cout:
            w = torch.nn.functional.pad(w, (0, 0, 0, n_pad - Cout))
            bias = torch.nn.functional.pad(bias if bias is not None else torch.zeros(Cout), (0, n_pad - Cout))
        if (sh, sw) == (1, 1):
            return self._lower_deconv_as_conv(node, x, w, bias, act, last, absorbed, (pt, pl), (Ho, Wo), Cout)
        if cin_phys != Cin:
            w = torch.nn.functional.pad(w, (0, cin_phys - Cin))  # zero filter rows against the padding columns
        w_dev = self._dev(K.deconv_pack_weights(w, (sh, sw), (pt, pl)), torch.bfloat16)
        b_dev = self._dev(bias if bias is not None else torch.zeros(n_pad), torch.float32)
        self.params += [w_dev, b_dev]
        xin = self._as_bf16(x, node.name)
        out = self._new((N, Ho, Wo, Cout), phys_c=n_pad if n_pad != Cout else None)
        for a in absorbed:
            self._fused.add(a.name)

        def run(xin=xin, out=out, w_dev=w_dev, b_dev=b_dev):
            K.deconv2d_nhwc(xin.buf, w_dev, b_dev, (Ho, Wo), (KH, KW), (sh, sw), (pt, 0, pl, 0), act, out=_target(out),
                            out_channel_offset=_coff(out))

        self._emit(node.name, "deconv", run, [xin], [out], {"phases": sh * sw, "impl": "deconv"})
        self._finish_conv(last, absorbed, out)

    def _lower_deconv_as_conv(self, node, x, w, bias, act, last, absorbed, pads, out_hw, cout_logical):
        """Stride 1: ``y[oy] = sum x[oy + pt - ky] w[ky]`` is the correlation of ``x`` with the
        flipped filter ``w[KH - 1 - k]`` at top pad ``KH - 1 - pt``; the bottom pad is what the
        output size leaves."""
        KH, KW = w.shape[:2]
        Hi, Wi = x.shape[1:3]
        pt, pl = KH - 1 - pads[0], KW - 1 - pads[1]
        pb, pr = out_hw[0] - Hi + KH - 1 - pt, out_hw[1] - Wi + KW - 1 - pl
        if min(pb, pr) < 0:
            return self._lower_glue(node, host_consts=(0,))
        w_hwio = w.flip(0, 1).permute(0, 1, 3, 2).contiguous()
        c = self._prepare_conv(node, x, w_hwio, bias, None, act, last, absorbed, (1, 1), (pt, pb, pl, pr), (1, 1),
                               out_hw, cout_logical)
        impl = select_conv_kernel(c.site)
        if c.out.phys_c and impl == "dconv":
            impl = "igemm"  # as ``_lower_conv``: the direct conv's fusions assume an unpadded output
        {"dconv": self._emit_dconv, "conv3x3c64": self._emit_conv3x3c64, "gemm_pp": self._emit_gemm_pp,
         "conv_lite": self._emit_conv_lite, "igemm": self._emit_igemm}[impl](c)
