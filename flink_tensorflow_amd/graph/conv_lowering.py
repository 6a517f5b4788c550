"""Conv2D lowering for the graph compiler: which hand-written kernel a ``Conv2D`` chain runs
on, and the emission of its launch step (a mixin of ``CompiledFunction``).

The kernel choice of a single conv is a pure function of a :class:`ConvSite`
(:func:`select_conv_kernel`, :func:`select_conv_fp8_kernel`): it needs no plan and no GPU.
The fusions that depend on plan state — the preprocess fold and the fused max pool of the
direct conv, the projection shortcut, the bottleneck block tail, the sibling group of an
Inception module, the commuted average pool — stay methods, as do the two post-passes that
rewrite block tails (``_decimate_tails``, ``_chain_tails``).  A ``DepthwiseConv2dNative``
chain has one kernel (kernels/dwconv.hip) and one lowering, ``_lower_dwconv``."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from ..ops import fp8 as F8
from ..ops import kernels as K
from .graph import Node
from .ops_nn import same_pads
from .plan import CompileError, Val, _cfg, _coff, _eff_scale, _root, _target, _view

_ACTS = {"Relu": K.ACT_RELU, "Relu6": K.ACT_RELU6, "Sigmoid": K.ACT_SIGMOID, "Tanh": K.ACT_TANH}

# The fp8 conv_lite tile (kernels/fp8.hip conv_lite_fp8): cfg 11 = per layer, the channel
# tile (192 / 160 / 128 / 96 / 64) that stages the fewest rows (profiles/r04_af); -1 = the
# register-staged kernel.  The bf16 conv_lite (kernels/conv_pp.hip) has one tile, 128 pixels
# x 128 channels on 4 waves and two LDS-DMA stages.  The other tiles and tile choosers were
# measured slower and removed with their kernels (numbers in the profile READMEs: r04_ad,
# r04_u, r04_w, r04_s-u, r04_ac, r04_ah, r03_conv, r01_tail, r02_pw_res2, r02_conv_pp).
LITE_FP8_CFG = 11
# smallest K of a 1x1 reduce conv that runs on gemm_pp when it has >= 256 output channels
_PP_MIN_K = 512

_PLAIN_ACTS = (K.ACT_NONE, K.ACT_RELU)
# the depthwise kernel's epilogue: Sigmoid / Tanh end its chain before them
_DW_ACTS = {"Relu": K.ACT_RELU, "Relu6": K.ACT_RELU6}


@dataclass(frozen=True)
class ConvSite:
    """What the kernel choice of one Conv2D chain depends on, and nothing else."""

    on_gpu: bool
    x_shape: tuple                # NHWC shape of the conv's input value
    cin: int                      # the filter's input channels
    cin_phys: int                 # channels of the input buffer (padded to 8; the s2d stem: 16)
    cout: int
    kernel: tuple                 # (KH, KW) as launched (the s2d stem: its 2x2-block filter)
    stride: tuple = (1, 1)
    pads: tuple = (0, 0, 0, 0)    # (top, bottom, left, right)
    dil: tuple = (1, 1)
    act: int = K.ACT_NONE
    residual: bool = False
    res_plain: bool = False       # the residual has the output's shape, no concat slot, no qscale
    res_alias: bool = False       # the residual is a view of another value
    x_dtype: torch.dtype = torch.bfloat16
    x_fp8: bool = False           # fp8 plans: the input is stored as e4m3
    out_dtype: torch.dtype = torch.bfloat16
    out_fp8: bool = False
    out_coff: int = 0             # channel offset of the output in its concat buffer
    s2d: bool = False             # the input is the space-to-depth preprocess output (RGB stem)
    conv3x3c64_kernel: bool = True  # EngineConfig toggles
    pw_res_kernel: bool = True

    @property
    def pointwise(self) -> bool:
        return (*self.kernel, *self.stride, *self.pads, *self.dil) == (1, 1, 1, 1, 0, 0, 0, 0, 1, 1)

    @property
    def unpadded_cin(self) -> bool:
        return not self.s2d and self.cin_phys == self.cin


def _dconv_ok(on_gpu, cin_phys, kernel, stride, dil, es, residual, act, bn=64) -> bool:
    """Direct LDS conv for narrow layers (input row <= 32 B: RGB stems, Inception's
    32-channel fp8 layers); measured faster there by bench/dconv_tune.py, slower for
    wider inputs, which stay on the implicit GEMM."""
    return (on_gpu and not residual and act in _PLAIN_ACTS
            and cin_phys * es <= 32 and K.dconv_eligible(cin_phys, *kernel, stride, dil, es, bn))


IGEMM_MAX_TAPS = 64  # the implicit GEMM keeps the in-image taps of a pixel in one 64-bit mask


# the choices tried after the graph-structural fusions of a residual 1x1 conv
# (``_fuse_shortcut``, ``_fuse_block_tail``); the others win before them
AFTER_FUSIONS = ("pw_res", "conv_lite", "igemm")


def select_conv_kernel(s: ConvSite) -> str:
    """The kernel of a bf16 Conv2D chain, in priority order: ``dconv``, ``conv3x3c64``,
    ``gemm_pp``, then (after the fusions of ``AFTER_FUSIONS``) ``pw_res``, ``conv_lite``
    and the register-staged implicit GEMM ``igemm``, which takes everything."""
    if _dconv_ok(s.on_gpu, s.cin_phys, s.kernel, s.stride, s.dil, 2, s.residual, s.act):
        return "dconv"
    if s.kernel[0] * s.kernel[1] > IGEMM_MAX_TAPS and _dconv_ok(s.on_gpu, s.cin_phys, s.kernel, s.stride, s.dil, 2,
                                                                s.residual, s.act, bn=32):
        # a filter the implicit GEMM cannot take (the keyword spotter's 20 x 8 first conv over
        # one padded input channel) whose bank fits LDS in 32-channel tiles only
        return "dconv"
    if (not s.residual and not s.out_fp8 and s.unpadded_cin and s.conv3x3c64_kernel
            and K.conv3x3_c64_eligible(s.x_shape, (s.cout, *s.kernel, s.cin_phys), s.stride, s.pads, s.dil, None,
                                       s.act)):
        # 64-channel 3x3 (ResNet stage 1): persistent kernel, filter bank resident in LDS
        return "conv3x3c64"
    if (s.on_gpu and s.pointwise and not s.residual and s.act in _PLAIN_ACTS and not s.out_fp8 and s.unpadded_cin
            and (s.cin >= 1024 or (s.cin >= _PP_MIN_K and s.cout >= 256)) and s.cin % 64 == 0 and s.cout % 8 == 0
            and s.out_coff % 8 == 0):
        # deep-K 1x1 reduce convs (ResNet stages 3/4: K = 1024 / 2048; the stage-3 entry
        # reduce K = 512 -> 256) are plain GEMMs over the pixel matrix: the ping-pong
        # 256x256 MFMA kernel (kernels/gemm_pp.hip)
        return "gemm_pp"
    if (s.residual and s.pointwise and s.act == K.ACT_RELU and not s.out_fp8 and s.out_dtype == torch.bfloat16
            and s.unpadded_cin and K.pw_res_ok(s.cin, s.cout) and s.res_plain and s.pw_res_kernel):
        # identity-residual expansion conv (ResNet stages 2/3): persistent kernel, resident
        # weight slice, next tile's x / residual prefetched (kernels/pw_res.hip)
        return "pw_res"
    if (s.on_gpu and not s.out_fp8 and s.unpadded_cin and s.cin % 64 == 0 and s.cout % 8 == 0
            and s.out_coff % 8 == 0 and s.out_dtype == torch.bfloat16 and s.x_dtype == torch.bfloat16
            and not s.pointwise and s.act in _PLAIN_ACTS
            and (not s.residual or (s.res_plain and not s.res_alias))
            and max(s.pads[:2]) < 1024 and max(s.pads[2:]) < 1024):
        # KxK convs (stage 2-4 3x3): 4-wave 128x128 implicit GEMM on two LDS-DMA stages
        # (kernels/conv_pp.hip conv_lite): 6-24 % faster than the register-staged igemm
        # per layer and 64 KiB of LDS, so it shares a CU with the sibling lane
        # (the 32-deep-K tile, 256x128 (4 or 8 waves) and 3-stage variants (raw-barrier,
        # counted vmcnt) measured slower: profiles/r03_conv, r04_a, r04_c)
        return "conv_lite"
    return "igemm"


def select_conv_fp8_kernel(s: ConvSite) -> str:
    """The kernel of an fp8 Conv2D chain: ``dconv`` for narrow fp8 inputs, else the 4-wave
    LDS-DMA tile ``conv_lite_fp8`` for an fp8 input; a bf16 input (the layer after a bf16
    stem) is quantised on load by the register-staged kernel, ``igemm_fp8``.
    (An eight-wave 256-pixel tile on three LDS stages measured 5-40 % slower per layer
    and -2 % in the bench: profiles/r04_d.)"""
    if s.x_fp8 and _dconv_ok(s.on_gpu, s.cin, s.kernel, s.stride, s.dil, 1, False, s.act):
        return "dconv"
    return "conv_lite_fp8" if s.x_fp8 else "igemm_fp8"


@dataclass
class _ConvJob:
    """One bf16 Conv2D chain on its way to a launch step: the site, the values and the
    prepared weights the ``_emit_<impl>`` methods read."""

    node: Node
    site: ConvSite
    x: Val                      # the conv's graph input
    xin: Val                    # what the kernel reads (``x``, channel-padded when needed)
    out: Val
    res_val: Val | None
    add_node: Node | None       # the residual Add
    w_ohwi: torch.Tensor        # host filter, BN folded, input channels padded
    bias: torch.Tensor | None   # host bias
    w_dev: torch.Tensor
    b_dev: torch.Tensor | None
    last: Node                  # last node of the fused chain
    absorbed: list


class ConvLowering:
    # ---- conv chain
    def _conv_chain(self, start: Node, absorb_residual: bool = True, acts=_ACTS):
        """Follows Conv2D/MatMul → BiasAdd/FusedBatchNorm* → Add(res)? → act? .  Without
        ``absorb_residual`` a residual Add ends the chain before it (the depthwise kernel has
        no residual operand); ``acts`` are the activations the kernel's epilogue has."""
        scale = None
        bias = None
        residual = None
        act = K.ACT_NONE
        cur = start
        absorbed = []
        while True:
            nxt = self._single_consumer(cur.name)
            if nxt is None:
                break
            if nxt.op in ("BiasAdd", "Add", "AddV2") and residual is None and act == K.ACT_NONE:
                other = [i for i, (s, _) in enumerate(nxt.inputs) if s != cur.name]
                if len(other) != 1:
                    break
                ov = self._get(nxt.inputs[other[0]])
                if ov is not None and ov.is_const and ov.const.dim() == 1:
                    b = ov.const.float()
                    bias = b if bias is None else bias + b
                elif nxt.op != "BiasAdd" and ov is not None and not ov.is_const and absorb_residual:
                    residual = (nxt, other[0])
                else:
                    break
            elif nxt.op.startswith("FusedBatchNorm") and residual is None and act == K.ACT_NONE:
                if nxt.attr("is_training", False):
                    break
                p = [self._get(nxt.inputs[i]) for i in range(1, 5)]
                if not all(v is not None and v.is_const for v in p):
                    break
                g, b, m, v = (t.const.float() for t in p)
                eps = nxt.attr("epsilon", 1e-3)
                s = g * torch.rsqrt(v + eps)
                shift = b - m * s
                scale = s if scale is None else scale * s
                bias = shift if bias is None else bias * s + shift
            elif nxt.op in acts and act == K.ACT_NONE and not self._image_out_keeps(start, nxt):
                act = acts[nxt.op]  # (a Tanh / Sigmoid that heads an image-output chain is that step's)
            else:
                break
            absorbed.append(nxt)
            cur = nxt
        return cur, scale, bias, residual, act, absorbed

    def _finish_conv(self, last: Node, absorbed, out: Val):
        """The fused chain's value: every absorbed node's output is ``out``."""
        self.vals[(last.name, 0)] = out
        for a in absorbed:
            self.vals[(a.name, 0)] = out

    def _conv_geometry(self, node: Node, x: Val, wv: Val):
        """``(w HWIO fp32, (sh, sw), (dh, dw), (pt, pb, pl, pr), (Ho, Wo))`` of a Conv2D the
        kernels take, or None (it runs as a glue op)."""
        if not wv.is_const or node.attr("data_format", "NHWC") != "NHWC":
            return None
        strides = node.attr("strides")
        dil = node.attr("dilations") or [1, 1, 1, 1]
        sh, sw = strides[1], strides[2]
        dh, dw = dil[1], dil[2]
        w = wv.const.float()  # HWIO
        KH, KW, Cin, Cout = w.shape
        N, H, W, C = x.shape
        if C != Cin:
            raise CompileError(f"{node.name}: input channels {C} != filter {Cin}")
        padding = node.attr("padding", "SAME")
        if padding == "SAME":
            pt, pb = same_pads(H, KH, sh, dh)
            pl, pr = same_pads(W, KW, sw, dw)
        elif padding == "VALID":
            pt = pb = pl = pr = 0
        else:
            return None
        Ho = (H + pt + pb - ((KH - 1) * dh + 1)) // sh + 1
        Wo = (W + pl + pr - ((KW - 1) * dw + 1)) // sw + 1
        return w, (sh, sw), (dh, dw), (pt, pb, pl, pr), (Ho, Wo)

    def _lower_conv(self, node: Node):
        if self.precision == "fp8" and self._lower_sibling_group(node):
            return
        x = self._in(node, 0)
        # 1. geometry
        geo = self._conv_geometry(node, x, self._in(node, 1))
        if geo is None:
            return self._lower_glue(node)
        w, stride, dil, pads, out_hw = geo
        # 2. the fused chain; BN folds into the output channels
        last, scale, bias, residual, act, absorbed = self._conv_chain(node)
        if scale is not None:
            w = w * scale
        KH, KW, Cin, Cout = w.shape
        n_pad = -(-Cout // 8) * 8
        if n_pad != Cout:
            # e.g. 21 classes: zero filters and biases up to a multiple of 8, as _lower_matmul
            # pads GEMM columns; the output value keeps its logical shape over a padded buffer
            # (``phys_c``).  Only the plain chain: a residual would need the same padding.
            if residual is not None:
                return self._lower_glue(node)
            w = torch.nn.functional.pad(w, (0, n_pad - Cout))
            bias = torch.nn.functional.pad(bias if bias is not None else torch.zeros(Cout), (0, n_pad - Cout))
        if self.precision == "fp8" and self._conv_fp8_ok(node, x, Cin, Cout, residual, act):
            return self._lower_conv_fp8(node, x, w, bias, act, last, absorbed, (KH, KW, Cin, Cout), stride, pads, dil,
                                        (x.shape[0], *out_hw))
        c = self._prepare_conv(node, x, w, bias, residual, act, last, absorbed, stride, pads, dil, out_hw, Cout)
        # 3./4. the kernel; a residual 1x1 conv first tries the fusions that need plan state
        impl = select_conv_kernel(c.site)
        if n_pad != Cout and impl == "dconv":
            impl = "igemm"  # the direct conv's pool / preprocess fusions assume an unpadded output
        if impl in AFTER_FUSIONS and self._fuse_residual_conv(c):
            return
        # 5. one launch step
        {"dconv": self._emit_dconv, "conv3x3c64": self._emit_conv3x3c64, "gemm_pp": self._emit_gemm_pp,
         "pw_res": self._emit_pw_res, "conv_lite": self._emit_conv_lite, "igemm": self._emit_igemm}[impl](c)

    # ---- depthwise conv
    def _lower_dwconv(self, node: Node):
        """``DepthwiseConv2dNative → [BiasAdd | FusedBatchNorm*]* → [Relu | Relu6]`` as one
        launch of the depthwise kernel (kernels/dwconv.hip); the BN scale of channel ``c``
        multiplies ``w[:, :, c, 0]``.  A residual Add stays an elementwise step."""
        x = self._in(node, 0)
        wv = self._in(node, 1)
        if (not wv.is_const or node.attr("data_format", "NHWC") != "NHWC" or len(x.shape) != 4
                or len(wv.const.shape) != 4 or wv.const.shape[3] != 1 or x.is_const
                or node.attr("padding", "SAME") not in ("SAME", "VALID")):
            return self._lower_glue(node)
        w = wv.const.float()  # [KH, KW, C, 1]
        KH, KW, C, _ = w.shape
        N, H, W, Cx = x.shape
        strides = node.attr("strides")
        dil = node.attr("dilations") or [1, 1, 1, 1]
        stride, dil = (strides[1], strides[2]), (dil[1], dil[2])
        if Cx != C or x.phys_c or not K.dwconv_eligible(C, KH, KW, stride, dil) \
                or not (x.dtype in (torch.bfloat16, torch.float32) or x.qscale is not None):
            return self._lower_glue(node)
        if node.attr("padding", "SAME") == "SAME":
            pads = (*same_pads(H, KH, stride[0], dil[0]), *same_pads(W, KW, stride[1], dil[1]))
        else:
            pads = (0, 0, 0, 0)
        Ho = (H + pads[0] + pads[1] - ((KH - 1) * dil[0] + 1)) // stride[0] + 1
        Wo = (W + pads[2] + pads[3] - ((KW - 1) * dil[1] + 1)) // stride[1] + 1
        if Ho < 1 or Wo < 1:
            return self._lower_glue(node)
        last, scale, bias, _, act, absorbed = self._conv_chain(node, absorb_residual=False, acts=_DW_ACTS)
        w = w[..., 0]
        if scale is not None:
            w = w * scale
        w_dev = self._dev(w.reshape(KH * KW, C).contiguous(), torch.bfloat16)
        b_dev = self._dev(bias, torch.float32) if bias is not None else None
        self.params += [w_dev] + ([b_dev] if b_dev is not None else [])
        xin = self._as_bf16(x, node.name)
        out = self._new((N, Ho, Wo, C))
        for a in absorbed:
            self._fused.add(a.name)

        def run(xin=xin, out=out, w_dev=w_dev, b_dev=b_dev):
            K.dwconv2d_nhwc(xin.buf, w_dev, b_dev, stride, pads, dil, act, out=_target(out),
                            out_channel_offset=_coff(out), kernel=(KH, KW))

        self._emit(node.name, "dwconv", run, [xin], [out], {"impl": K.dwconv_impl(KH, KW, stride, dil)})
        self._finish_conv(last, absorbed, out)

    def _prepare_conv(self, node, x, w, bias, residual, act, last, absorbed, stride, pads, dil, out_hw,
                      cout_logical: int | None = None) -> _ConvJob:
        """Weights, input and output values of a bf16 conv chain, and its ``ConvSite``.  With
        ``cout_logical`` below the filter's (zero-padded) output channels, the output value has
        that many channels over a buffer of the padded width."""
        KH, KW, Cin, Cout = w.shape
        padded = cout_logical is not None and cout_logical != Cout
        N, H, W, C = x.shape
        s2d = self._s2d_ok(x, node, C, *stride, *dil, pads[0], pads[2], H, W)
        if s2d:
            # stride-2 RGB stem over the space-to-depth preprocess output (K 392 -> 256)
            w_ohwi, pads = K.s2d_stem_weights(w, H, W, pads)
            x.pre_cfg["s2d"] = True
            x.buf_shape = (N, (H + 1) // 2, (W + 1) // 2, 16)
            x.phys_c = 16
            stride = (1, 1)
            cin_pad = 16
        else:
            phys = x.phys_c or C
            cin_pad = -(-phys // 8) * 8
            w_ohwi = w.permute(3, 0, 1, 2).contiguous()
            if cin_pad != Cin:
                w_ohwi = torch.nn.functional.pad(w_ohwi, (0, cin_pad - Cin))
        w_dev = self._dev(w_ohwi, torch.bfloat16)
        b_dev = self._dev(bias, torch.float32) if bias is not None else None
        self.params += [w_dev] + ([b_dev] if b_dev is not None else [])
        out = self._new((N, *out_hw, cout_logical if padded else Cout), phys_c=Cout if padded else None)
        kernel = tuple(w_ohwi.shape[1:3])
        if (not padded and self.precision == "fp8" and residual is None and act in _PLAIN_ACTS and Cout % 16 == 0
                and self._fp8_consumers_ok(last.name) and self._qscale(last.name) is not None
                and _dconv_ok(self.device.type == "cuda", cin_pad, kernel, stride, dil, 2, False, act)):
            # bf16 direct-conv layer (the RGB stem) feeding fp8 consumers: emit e4m3 directly
            # (a wider bf16 layer hands bf16 on; its fp8 successor quantises on load)
            out = self._new((N, *out_hw, Cout), torch.uint8)
            out.qscale = self._qscale(last.name)
        res_val = add_node = None
        if residual is not None:
            add_node, ri = residual
            res_val = self.vals[add_node.inputs[ri]]
        xin = x if s2d else self._ensure_padded(x, cin_pad, node.name)
        for a in absorbed:
            self._fused.add(a.name)
        cfg = _cfg()
        site = ConvSite(
            on_gpu=self.device.type == "cuda", x_shape=tuple(xin.shape), cin=Cin, cin_phys=xin.phys_c or Cin, cout=Cout,
            kernel=kernel, stride=tuple(stride), pads=tuple(pads), dil=tuple(dil), act=act,
            residual=res_val is not None,
            res_plain=(res_val is not None and res_val.qscale is None and res_val.concat_slot is None
                       and tuple(res_val.shape) == tuple(out.shape)),
            res_alias=res_val is not None and res_val.alias_of is not None,
            x_dtype=xin.dtype, out_dtype=out.dtype, out_fp8=out.qscale is not None, out_coff=_coff(out), s2d=s2d,
            conv3x3c64_kernel=cfg.conv3x3c64_kernel, pw_res_kernel=cfg.pw_res_kernel)
        return _ConvJob(node, site, x, xin, out, res_val, add_node, w_ohwi, bias, w_dev, b_dev, last, absorbed)

    def _zero_bias(self, c: _ConvJob) -> torch.Tensor:
        return c.b_dev if c.b_dev is not None else self._dev(torch.zeros(c.site.cout), torch.float32)

    # ---- one launch step per kernel
    def _emit_dconv(self, c: _ConvJob):
        s, out = c.site, c.out
        Cout, conv_out = s.cout, tuple(c.out.shape)
        bn = 64 if Cout >= 64 and K.dconv_eligible(s.cin_phys, *s.kernel, s.stride, s.dil, 2, 64) else 32
        w_arr = self._dev(K.dconv_bf16_weight_bytes(c.w_ohwi, bn))
        b_dev = c.b_dev if c.b_dev is not None else torch.zeros(Cout, dtype=torch.float32, device=self.device)
        self.params += [w_arr, b_dev]
        pool = self._fusable_maxpool(c.last, s.act, out)
        mpad = None
        if pool is not None:
            # ReLU stem + 3x3/s2 max pool in one kernel: the full-resolution stem
            # output never reaches HBM
            pnode, mpad, (Hp, Wp) = pool
            out = self._new((conv_out[0], Hp, Wp, Cout))
            self._fused.add(pnode.name)
        elif self._fold_preprocess(c, w_arr, b_dev, bn):
            return

        def run_d(xin=c.xin, out=out, w_arr=w_arr, b_dev=b_dev, bn=bn, mpad=mpad):
            K.conv2d_direct(xin.buf, w_arr, s.kernel, Cout, b_dev, s.stride, s.pads, s.act,
                            out=_target(out), out_channel_offset=_coff(out), bn=bn,
                            out_scale=_eff_scale(out) if out.qscale is not None else None, maxpool_pad=mpad)

        # the MACs of a pool-fused stem are those of its full-resolution (pre-pool) output
        self._emit(c.node.name, "conv", run_d, [c.xin], [out], {"conv_out": conv_out} if pool else None)
        if pool is not None:
            self.vals[(pool[0].name, 0)] = out
            self.stats["fused_pools"] += 1
            return
        self._finish_conv(c.last, c.absorbed, out)

    def _fold_preprocess(self, c: _ConvJob, w_arr, b_dev, bn) -> bool:
        """The plan's head preprocess kernel folds into this s2d stem: the conv builds its
        s2d patches from the raw uint8 batch (Inception-v3's Conv2d_1a: no resize)."""
        s, x, out = c.site, c.x, c.out
        pp = x.pre_params
        if not (s.s2d and pp is not None and not pp["resize"]
                and _cfg().fuse_preprocess_stem and len(self.steps) == 1 and self.steps[0].kind == "preprocess"
                and self.steps[0].outputs[0] is x and _root(out) is out and _coff(out) == 0):
            return False
        self.steps.pop()
        xu = pp["x"]
        osc = _eff_scale(out) if out.qscale is not None else None

        def head(src, dst):
            K.conv2d_direct_u8s2d(src, w_arr, s.kernel, s.cout, b_dev, s.pads, s.act, pp["mean"], pp["std"], out=dst,
                                  bn=bn, out_scale=osc)

        # kind "preprocess": still the plan's head, launched per H2D piece by the runner
        self._emit(c.node.name, "preprocess", lambda: head(xu.buf, out.buf), [xu], [out],
                   {"impl": "dconv_u8s2d", "conv_out": tuple(out.shape)}, head=head)
        self.stats["fused_preprocess"] = 1
        self._finish_conv(c.last, c.absorbed, out)
        return True

    def _emit_conv3x3c64(self, c: _ConvJob):
        bz, act = self._zero_bias(c), c.site.act

        def run_c(xin=c.xin, out=c.out, w_dev=c.w_dev, bz=bz):
            K.conv3x3_c64(xin.buf, w_dev, bz, act, out=_target(out), out_channel_offset=_coff(out))

        self._emit(c.node.name, "conv", run_c, [c.xin], [c.out], {"impl": "conv3x3c64"})
        self.stats["conv3x3c64"] += 1
        self._finish_conv(c.last, c.absorbed, c.out)

    def _emit_gemm_pp(self, c: _ConvJob):
        Cin, Cout = c.site.cin, c.site.cout
        w_nk = c.w_dev.reshape(Cout, Cin)
        bz = self._zero_bias(c)
        M = int(np.prod(c.xin.shape[:-1]))
        splits = K.gemm_pp_splits(M, Cout, Cin)
        ws = torch.empty(splits * M * Cout, dtype=torch.float32, device=self.device) if splits > 1 else None

        def run_pp(xin=c.xin, out=c.out, w_nk=w_nk, bz=bz, act=c.site.act, splits=splits, ws=ws):
            K.gemm_pp(xin.buf.view(-1, Cin), w_nk, bz, None, act, out=_target(out), out_col=_coff(out),
                      splits=splits, ws=ws)

        self._emit(c.node.name, "gemm", run_pp, [c.xin], [c.out], {"impl": "gemm_pp"})
        self._finish_conv(c.last, c.absorbed, c.out)

    def _emit_pw_res(self, c: _ConvJob):
        w_nk = c.w_dev.reshape(c.site.cout, c.site.cin)
        bz = self._zero_bias(c)

        def run_pw(xin=c.xin, out=c.out, res_val=c.res_val, w_nk=w_nk, bz=bz):
            K.pw_res(xin.buf, w_nk, bz, res_val.buf, out=_target(out), out_channel_offset=_coff(out))

        self._emit(c.node.name, "conv", run_pw, [c.xin, c.res_val], [c.out], {"impl": "pw_res"})
        self.stats["pw_res"] += 1
        self._finish_conv(c.last, c.absorbed, c.out)

    def _emit_conv_lite(self, c: _ConvJob):
        s = c.site
        cl = K.ConvPP([(tuple(c.xin.shape), s.kernel, s.stride, (s.pads[0], s.pads[2]), s.dil)], s.cout,
                      tuple(c.out.shape[1:3]), self.device)

        def run_l(xin=c.xin, out=c.out, res_val=c.res_val, cl=cl, w2=c.w_dev.reshape(s.cout, -1), b_dev=c.b_dev):
            cl([xin.buf], w2, b_dev, res_val.buf if res_val is not None else None, s.act, out=_target(out),
               out_channel_offset=_coff(out))

        self.stats["conv_lite"] += 1
        self._emit_single_conv(c, run_l)

    def _emit_igemm(self, c: _ConvJob):
        s = c.site

        def run(xin=c.xin, out=c.out, res_val=c.res_val, w_dev=c.w_dev, b_dev=c.b_dev):
            K.conv2d_nhwc(xin.buf, w_dev, b_dev, res_val.buf if res_val is not None else None, s.stride,
                          s.pads, s.dil, s.act, out=_target(out), out_channel_offset=_coff(out),
                          out_scale=_eff_scale(out) if out.qscale is not None else None)

        self._emit_single_conv(c, run)

    def _emit_single_conv(self, c: _ConvJob, run):
        """The step of a conv_lite / igemm conv; an unpadded 1x1 projection (no residual, no
        act) records what ``_fuse_shortcut`` needs to fold it into the conv it feeds."""
        s = c.site
        shortcut_ok = (s.kernel == (1, 1) and s.stride[0] == s.stride[1] and s.pads == (0, 0, 0, 0) and s.dil == (1, 1)
                       and not s.residual and s.act == K.ACT_NONE and not s.out_fp8 and s.unpadded_cin)
        meta = {"shortcut": dict(x=c.xin, w=c.w_ohwi, bias=c.bias, stride=s.stride[0],
                                 params=[c.w_dev, c.b_dev])} if shortcut_ok else None
        self._emit(c.node.name, "conv", run, [c.xin] + ([c.res_val] if c.res_val else []), [c.out], meta)
        self._finish_conv(c.last, c.absorbed, c.out)

    # ---- fusions of a residual 1x1 conv (plan state)
    def _fuse_residual_conv(self, c: _ConvJob) -> bool:
        s = c.site
        if c.res_val is None or not s.pointwise or s.s2d:
            return False
        if not s.out_fp8 and self._fuse_shortcut(c):
            return True
        return self._fuse_block_tail(c.xin, c.out, c.w_ohwi.reshape(c.w_ohwi.shape[0], -1), c.w_dev, c.b_dev,
                                     c.res_val, None, s.act, c.absorbed, c.last, c.node.name)

    def _fuse_shortcut(self, c: _ConvJob) -> bool:
        """Pointwise conv whose residual is a 1x1 (strided) projection conv used by nothing
        else: drop the projection's launch and run both as one K loop
        (``conv1x1_dual``) — the projection output never round-trips through HBM."""
        xin, out, res_val, w_ohwi, bias, act = c.xin, c.out, c.res_val, c.w_ohwi, c.bias, c.site.act
        prod = [st for st in self.steps if any(o is res_val for o in st.outputs)]
        if len(prod) != 1 or "shortcut" not in prod[0].meta or res_val.concat_slot is not None:
            return False
        readers = self._readers(res_val)  # the projection feeds only this Add
        if readers is None or any(k != c.add_node.name and k not in self._fused for k in readers):
            return False
        sc = prod[0].meta["shortcut"]
        x2 = sc["x"]
        s2 = sc["stride"]
        N, Ho, Wo, _ = out.shape
        if x2.shape[0] != N or (Ho - 1) * s2 >= x2.shape[1] or (Wo - 1) * s2 >= x2.shape[2]:
            return False
        Cout, K1 = w_ohwi.shape[0], w_ohwi.shape[3]
        C2 = sc["w"].shape[3]
        if K1 % 8 or C2 % 8:
            return False
        self.steps.remove(prod[0])
        for t in sc["params"]:
            if t is not None:
                self.params = [q for q in self.params if q is not t]
        w_cat = torch.cat([w_ohwi.reshape(Cout, K1), sc["w"].reshape(Cout, C2)], 1)
        b = (bias if bias is not None else torch.zeros(Cout)) + (sc["bias"] if sc["bias"] is not None else 0)
        w_dev = self._dev(w_cat, torch.bfloat16)
        b_dev = self._dev(b, torch.float32)
        self.params += [w_dev, b_dev]
        for a in c.absorbed:
            self._fused.add(a.name)
        if not (s2 == 1 and self._fuse_block_tail(xin, out, w_cat, w_dev, b_dev, None, x2, act, c.absorbed, c.last,
                                                  c.node.name)):
            self._emit_dual(c, x2, s2, w_dev, b_dev, K1, C2)
        self.stats["fused_shortcuts"] += 1
        return True

    def _emit_dual(self, c: _ConvJob, x2: Val, s2: int, w_dev, b_dev, K1: int, C2: int):
        """Expand conv + projection shortcut of ``x2`` (stride ``s2``) as one launch."""
        xin, out, act = c.xin, c.out, c.site.act
        N, Ho, Wo, Cout = out.shape
        s2cfg = {"s2": s2}  # _decimate_tails: x2 stored already decimated -> stride 1
        meta = {"s2cfg": s2cfg}
        if (self.device.type == "cuda" and K1 % 64 == 0
                and C2 % 64 == 0 and (xin.phys_c or K1) == K1 and (x2.phys_c or C2) == C2
                and act in _PLAIN_ACTS and out.dtype == torch.bfloat16 and out.qscale is None
                and _coff(out) % 8 == 0 and len(xin.shape) == 4 and N * Ho * Wo <= 65536):
            # expand + projection shortcut as one 4-wave LDS-DMA implicit GEMM over two
            # sources (kernels/conv_pp.hip conv_lite, DUAL); planned for x2 as it is and, when
            # _decimate_tails later stores x2 decimated, for the compact stride-1 layout.
            # Stages 3/4 only (ResNet-50 B=256: 111 / 100 µs vs 114 / 111 on the dual igemm);
            # stage 2's 200k-row GEMM stays on the igemm (141 vs 158 µs, profiles/r03_operating_points)
            xs0 = (tuple(xin.shape), (1, 1), (1, 1), (0, 0), (1, 1))
            lite = {s2: K.ConvPP([xs0, (tuple(x2.shape), (1, 1), (s2, s2), (0, 0), (1, 1))], Cout, (Ho, Wo),
                                 self.device)}
            N2, H2, W2, _ = x2.shape
            if s2 == 2 and H2 % 2 == 0 and W2 % 2 == 0:
                lite[1] = K.ConvPP([xs0, ((N2, H2 // 2, W2 // 2, C2), (1, 1), (1, 1), (0, 0), (1, 1))], Cout, (Ho, Wo),
                                   self.device)

            def run(xin=xin, x2=x2, out=out, w_dev=w_dev, b_dev=b_dev, s2cfg=s2cfg, lite=lite):
                lite[s2cfg["s2"]]([xin.buf, x2.buf], w_dev, b_dev, None, act, out=_target(out),
                                  out_channel_offset=_coff(out))

            meta["impl"] = "conv_lite_dual"
            self.stats["conv_lite"] += 1
        else:
            def run(xin=xin, x2=x2, out=out, w_dev=w_dev, b_dev=b_dev, s2cfg=s2cfg):
                K.conv1x1_dual(xin.buf, x2.buf, w_dev, b_dev, s2cfg["s2"], act, out=_target(out),
                               out_channel_offset=_coff(out))

        self._emit(c.node.name, "conv", run, [xin, x2], [out], meta)
        self._finish_conv(c.last, c.absorbed, out)

    def _fuse_block_tail(self, xin, out, w3, w_dev, b_dev, res_val, xs_val, act, absorbed, last, name) -> bool:
        """ResNet bottleneck block boundary: this 1x1 CX -> 4 CX expand conv (+ residual,
        ReLU) and the next block's 1x1 reduce conv (+ ReLU) that reads its output run as one
        persistent kernel (``bottleneck_tail``): the wide output is still stored (it is the
        next residual) but the reduce GEMM reads it from LDS instead of HBM.  Stage 1
        (CX = 64, reduce to 64 or 128) and stage 2 (CX = 128, reduce to 128).  ``w3`` is the
        host [4 CX, K] expand weight; with ``xs_val`` (stage 1's first block) K = 64 + 64
        covers the stride-1 projection shortcut of ``xs_val`` too."""
        if not _cfg().fuse_block_tails or self.precision == "fp8":
            return False
        cx = xin.shape[-1]
        co = 4 * cx
        # (stage 2, its weights streamed through LDS, measured no faster than the two convs
        # it would replace: profiles/r01_tail — stage 1 only)
        widths = {64: (64, 128)}.get(cx, ()) if xs_val is None else ((64,) if cx == 64 else ())

        def plain(v):
            return v.shape[-1] == cx and (v.phys_c or cx) == cx and v.concat_slot is None and v.qscale is None \
                and v.dtype == torch.bfloat16 and tuple(v.shape[:-1]) == tuple(out.shape[:-1])

        if not widths or act != K.ACT_RELU or out.qscale is not None \
                or tuple(w3.shape) != (co, cx if xs_val is None else 2 * cx) or not plain(xin):
            return False
        if res_val is not None and (res_val.shape != out.shape or res_val.qscale is not None
                                    or res_val.concat_slot is not None):
            return False
        if xs_val is not None and not plain(xs_val):
            return False
        cand = [self.graph[c] for c in self.cons.get(last.name, []) if c not in self._fused]

        def reduce_conv(c):  # 1x1 / s1 reduce conv reading this output (not the stage's projection)
            if c.op != "Conv2D" or c.inputs[0] != (last.name, 0) or c.attr("data_format", "NHWC") != "NHWC" \
                    or list(c.attr("strides")) != [1, 1, 1, 1] \
                    or list(c.attr("dilations") or [1, 1, 1, 1]) != [1, 1, 1, 1]:
                return None
            wv = self._get(c.inputs[1])
            if wv is None or not wv.is_const:
                return None
            w = wv.const.float()  # HWIO
            return w if tuple(w.shape[:3]) == (1, 1, co) and w.shape[3] in widths else None

        cand = [(c, w) for c in cand for w in [reduce_conv(c)] if w is not None]
        if len(cand) != 1:
            return False
        c, w2 = cand[0]
        last2, scale2, bias2, residual2, act2, absorbed2 = self._conv_chain(c)
        if residual2 is not None or act2 != K.ACT_RELU:
            return False
        cn = w2.shape[3]
        if scale2 is not None:
            w2 = w2 * scale2
        w3_dev = w_dev  # row-major [4 CX][K] (1x1 OHWI [4 CX, 1, 1, CX], or the dual [W3 | Wsc])
        b3_dev = b_dev if b_dev is not None else self._dev(torch.zeros(co), torch.float32)
        w1_dev = self._dev(w2.reshape(co, cn).t().contiguous(), torch.bfloat16)
        b1_dev = self._dev(bias2 if bias2 is not None else torch.zeros(cn), torch.float32)
        self.params += [b3_dev, w1_dev, b1_dev]
        N, H, W, _ = out.shape
        out2 = self._new((N, H, W, cn))
        for a in absorbed + absorbed2:
            self._fused.add(a.name)
        self._fused.add(c.name)

        second = res_val if xs_val is None else xs_val
        dec = {"on": False}  # set by _decimate_tails when y3's only other reader is a stride-2 projection
        # set by _chain_tails: recompute the residual chain from its narrow sources
        # (``links``) instead of reading y3 of the previous tail; ``store``: y3 is written
        chain = {"links": None, "store": True}

        def run(xin=xin, second=second, out=out, out2=out2, dual=xs_val is not None, dec=dec, chain=chain):
            if chain["links"] is not None:
                K.bottleneck_chain([(x.buf, s.buf if s is not None else None, w, b) for x, s, w, b in chain["links"]],
                                   w1_dev, b1_dev, y1=out2.buf, y3=out.buf if chain["store"] else None,
                                   y3_decimated=dec["on"], store_y3=chain["store"])
                return
            K.bottleneck_tail(xin.buf, None if dual else second.buf, w3_dev, b3_dev, w1_dev, b1_dev, y3=out.buf,
                              y1=out2.buf, xs=second.buf if dual else None, y3_decimated=dec["on"])

        self._emit(name, "conv", run, [xin, second], [out, out2],
                   {"impl": "bottleneck_tail", "dec": dec if xs_val is None and cx == 64 else None,
                    "tail": {"x": xin, "xs": xs_val, "res": res_val, "w3": w3_dev, "b3": b3_dev, "cn": cn,
                             "chain": chain}})
        self._finish_conv(last, absorbed, out)
        self._finish_conv(last2, absorbed2, out2)
        self.stats["fused_tails"] += 1
        return True

    def _fusable_maxpool(self, last: Node, act, out: Val, fp8: bool = False):
        """The single consumer of a ReLU conv chain when it is a 3x3 / stride-2 NHWC
        MaxPool whose padding is at most one row/column per side (ResNet's pool1; with
        ``fp8``, Inception's MaxPool_3a after an fp8 -> fp8 direct conv):
        ``(pool node, (top, bottom, left, right), (Hp, Wp))`` or None."""
        if act != K.ACT_RELU:
            return None
        if (out.qscale is not None or out.dtype != torch.bfloat16) if not fp8 else \
                (out.qscale is None or out.dtype != torch.uint8):
            return None
        if self._fetched(last.name):
            return None
        cons = [c for c in self.cons.get(last.name, []) if c not in self._fused]
        if len(cons) != 1 or self.graph[cons[0]].op != "MaxPool":
            return None
        pn = self.graph[cons[0]]
        if pn.attr("data_format", "NHWC") != "NHWC" or list(pn.attr("ksize")) != [1, 3, 3, 1] \
                or list(pn.attr("strides")) != [1, 2, 2, 1]:
            return None
        _, Ho, Wo, _ = out.shape
        if pn.attr("padding", "VALID") == "SAME":
            pt, pb = same_pads(Ho, 3, 2)
            pl, pr = same_pads(Wo, 3, 2)
        else:
            pt = pb = pl = pr = 0
        if max(pt, pb, pl, pr) > 1:
            return None
        return pn, (pt, pb, pl, pr), ((Ho + pt + pb - 3) // 2 + 1, (Wo + pl + pr - 3) // 2 + 1)

    # ---- fp8 conv chain
    def _conv_fp8_ok(self, node: Node, x: Val, Cin, Cout, residual, act) -> bool:
        if residual is not None or act not in _PLAIN_ACTS or Cin % 16 or Cout % 16 or x.phys_c:
            return False
        if x.qscale is not None:
            return True
        return x.dtype == torch.bfloat16 and self._qscale(node.inputs[0][0]) is not None

    def _lower_conv_fp8(self, node, x, w, bias, act, last, absorbed, kdims, stride, pads, dil, out_nhw):
        KH, KW, Cin, Cout = kdims
        w_ohwi = w.permute(3, 0, 1, 2).contiguous()
        wq, ws = F8.quantize_weight(w_ohwi)
        x_scale = x.qscale if x.qscale is not None else self._qscale(node.inputs[0][0])
        wq_dev = self._dev(wq)
        ws_dev = self._dev(ws)
        cs_dev = self._dev(ws * x_scale, torch.float32)
        b_dev = self._dev(bias, torch.float32) if bias is not None else \
            torch.zeros(Cout, dtype=torch.float32, device=self.device)
        self.params += [wq_dev, cs_dev, b_dev]
        o_scale = self._qscale(last.name) if self._fp8_consumers_ok(last.name) else None
        out = self._new((*out_nhw, Cout), torch.uint8 if o_scale is not None else torch.bfloat16)
        out.qscale = o_scale
        for a in absorbed:
            self._fused.add(a.name)
        self.fp8_layers += 1
        site = ConvSite(on_gpu=self.device.type == "cuda", x_shape=tuple(x.shape), cin=Cin, cin_phys=Cin, cout=Cout,
                        kernel=(KH, KW), stride=tuple(stride), pads=tuple(pads), dil=tuple(dil), act=act,
                        x_dtype=x.dtype, x_fp8=x.qscale is not None, out_dtype=out.dtype, out_fp8=o_scale is not None)
        impl = select_conv_fp8_kernel(site)
        if impl == "dconv":
            return self._emit_dconv_fp8(node, site, x, out, wq, cs_dev, b_dev, last, absorbed)
        # fp8 input: conv_lite_fp8; a bf16 input is quantised on load by the register-staged kernel
        cfg = LITE_FP8_CFG if impl == "conv_lite_fp8" else -1

        def run(x=x, out=out, wq=wq_dev, ws=ws_dev, cs=cs_dev, b=b_dev, x_scale=x_scale, cfg=cfg):
            F8.conv2d_nhwc_fp8(_view(x), x_scale, wq, (KH, KW), ws, b, stride, pads, dil, act,
                               out_scale=_eff_scale(out), out=_target(out), out_channel_offset=_coff(out), chan_scale=cs,
                               cfg=cfg)

        self._emit(node.name, "conv_fp8", run, [x], [out], {"impl": impl} if impl == "conv_lite_fp8" else None)
        if impl == "conv_lite_fp8":
            self.stats["conv_lite"] += 1
        self._finish_conv(last, absorbed, out)

    def _emit_dconv_fp8(self, node, s: ConvSite, x, out, wq, cs_dev, b_dev, last, absorbed):
        Cout, conv_out = s.cout, tuple(out.shape)
        bn = 64 if Cout >= 64 else 32
        w_arr = self._dev(K.dconv_weights(wq, Cout, 1, bn))
        self.params.append(w_arr)
        pool = self._fusable_maxpool(last, s.act, out, fp8=True) if s.stride == (1, 1) else None
        if pool is not None:
            # pooled tiles cover 14 x 8 pooled pixels with 8 waves x 64 conv pixels; fuse
            # only when that tiling wastes little conv work (Inception's 73x73 pool rounds to
            # 84 x 80 and costs 1.42x the convs: 445 µs fused vs 236 + 132 µs apart)
            Hp_, Wp_ = pool[2]
            waves = K._dconv_waves(None, None, bn)
            pr_ = 14 if waves == 8 else 7
            work = -(-Hp_ // pr_) * -(-Wp_ // 8) * 64 * waves
            if work > 1.15 * conv_out[1] * conv_out[2]:
                pool = None
        mpad = None
        if pool is not None:
            # fp8 ReLU conv + 3x3/s2 max pool in one kernel (Inception's Conv2d_2b ->
            # MaxPool_3a): the pre-pool output never reaches HBM; the pooled values keep
            # the conv output's scale (a max never leaves the input range)
            pnode, mpad, (Hp, Wp) = pool
            q = out.qscale
            out = self._new((conv_out[0], Hp, Wp, Cout), torch.uint8)
            out.qscale = q
            self._fused.add(pnode.name)

        def run_d(x=x, out=out, w_arr=w_arr, cs=cs_dev, b=b_dev, bn=bn, mpad=mpad):
            K.conv2d_direct(_view(x), w_arr, s.kernel, Cout, b, s.stride, s.pads, s.act, out=_target(out),
                            out_channel_offset=_coff(out), bn=bn, chan_scale=cs, out_scale=_eff_scale(out),
                            maxpool_pad=mpad)

        self._emit(node.name, "conv_fp8", run_d, [x], [out], {"conv_out": conv_out} if pool else None)
        if pool is not None:
            self.vals[(pool[0].name, 0)] = out
            self.stats["fused_pools"] += 1
            return
        self._finish_conv(last, absorbed, out)

    def _s2d_ok(self, x: Val, node: Node, C, sh, sw, dh, dw, pt, pl, H, W) -> bool:
        if x.pre_cfg is None or C != 3 or (sh, sw) != (2, 2) or (dh, dw) != (1, 1) or pt % 2 or pl % 2:
            return False
        users = self._readers(x)
        return users is not None and users - x.pre_chain == {node.name}

    def _ensure_padded(self, x: Val, cin_pad: int, name: str) -> Val:
        if x.qscale is not None:
            x = self._as_bf16(x, name)
        phys = x.phys_c or x.shape[-1]
        if phys == cin_pad and x.dtype == torch.bfloat16:
            return x
        y = self._new((*x.shape[:-1], cin_pad), phys_c=cin_pad)
        c = x.shape[-1]

        def run(x=x, y=y, c=c):
            y.buf.zero_()
            y.buf[..., :c].copy_(x.buf[..., :c])

        self._emit(name + "/pad_cin", "glue", run, [x], [y])
        return y

    # ---- horizontal fusion of sibling pointwise convs (Inception module heads)
    def _pw_member(self, c: Node, x: Val, src, max_cout: int | None = None):
        """``c`` as a member of a sibling group: a 1x1 / stride-1 Conv2D of ``src`` with a
        constant filter and a chain without residual ending in ReLU or nothing."""
        if c.op != "Conv2D" or c.name in self._fused or c.inputs[0] != src or c.attr("data_format", "NHWC") != "NHWC":
            return None
        if list(c.attr("strides") or [1, 1, 1, 1]) != [1, 1, 1, 1] or list(c.attr("dilations") or [1, 1, 1, 1]) != [1, 1, 1, 1]:
            return None
        wv = self._get(c.inputs[1])
        if wv is None or not wv.is_const or tuple(wv.const.shape[:3]) != (1, 1, x.shape[-1]):
            return None
        Cout = int(wv.const.shape[3])
        if Cout % 16 or (max_cout is not None and Cout > max_cout):
            return None
        last, scale, bias, residual, act, absorbed = self._conv_chain(c)
        if residual is not None or act not in _PLAIN_ACTS:
            return None
        w = wv.const.float()
        if scale is not None:
            w = w * scale
        return {"conv": c, "w": w.reshape(-1, Cout).t().contiguous(), "bias": bias, "act": act, "last": last,
                "absorbed": absorbed, "Cout": Cout}

    def _lower_sibling_group(self, entry: Node) -> bool:
        """The 1x1 convs that read one fp8 value — an Inception module's branch heads, and
        its AvgPool(3x3/1) -> 1x1 branch commuted to 1x1 -> pool — run as ONE implicit GEMM
        over their concatenated filters (``conv2d_nhwc_fp8_multi``): the input is read once
        instead of 3-4 times, and the combined channel count tiles better than 32-64-channel
        GEMMs.  Its epilogue sends each branch's channels to that branch's destination (a
        concat slot, an fp8 buffer with its own scale, or the bf16 pre-pool value)."""
        if not _cfg().sibling_conv_fusion:
            return False
        src = entry.inputs[0] if entry.inputs else None
        x = self.vals.get(src) if src is not None else None
        if x is None or x.qscale is None or x.phys_c or x.rows is not None or len(x.shape) != 4 or x.shape[-1] % 16:
            return False
        N, H, W, C = x.shape
        members = []
        for cname in dict.fromkeys(self.cons.get(src[0], [])):
            c = self.graph[cname]
            if c.name in self._fused or not c.inputs or c.inputs[0] != src or any(i == src for i in c.inputs[1:]):
                continue
            if c.op == "Conv2D":
                m = self._pw_member(c, x, src)
                if m is not None:
                    m["kind"], m["entry"] = "conv", c.name
                    members.append(m)
            elif c.op == "AvgPool" and c.attr("data_format", "NHWC") == "NHWC" and list(c.attr("ksize")) == [1, 3, 3, 1] \
                    and list(c.attr("strides")) == [1, 1, 1, 1]:
                pc = self._single_consumer(c.name)
                if pc is None:
                    continue
                m = self._pw_member(pc, x, (c.name, 0), max_cout=C // 2)
                if m is None:
                    continue
                if c.attr("padding", "VALID") == "SAME":
                    pads = (*same_pads(H, 3, 1), *same_pads(W, 3, 1))
                else:
                    continue  # a VALID 3x3/1 pool changes the spatial size: not a sibling of the 1x1s
                m["kind"], m["entry"], m["pool"], m["pads"] = "pool", c.name, c, pads
                members.append(m)
        if len(members) < 2 or entry.name not in {m["entry"] for m in members} or len(members) > 6:
            return False
        xs = x.qscale
        ws_rows, bias_parts, lo_parts, segs = [], [], [], []
        c0 = 0
        for m in members:
            Cout = m["Cout"]
            ws_rows.append(m["w"])
            if m["kind"] == "conv":
                last = m["last"]
                o_scale = self._qscale(last.name) if self._fp8_consumers_ok(last.name) else None
                out = self._new((N, H, W, Cout), torch.uint8 if o_scale is not None else torch.bfloat16)
                out.qscale = o_scale
                bias_parts.append(m["bias"] if m["bias"] is not None else torch.zeros(Cout))
                lo_parts.append(torch.full((Cout,), 0.0 if m["act"] == K.ACT_RELU else float("-inf")))
                m["out"] = out
                segs.append((out, c0, c0 + Cout))
            else:
                y = self._new((N, H, W, Cout))  # pre-bias conv output, pooled next
                bias_parts.append(torch.zeros(Cout))
                lo_parts.append(torch.full((Cout,), float("-inf")))
                last = m["last"]
                o_scale = self._qscale(last.name) if self._fp8_consumers_ok(last.name) else None
                out = self._new((N, H, W, Cout), torch.uint8 if o_scale is not None else torch.bfloat16)
                out.qscale = o_scale
                m["y"], m["out"] = y, out
                segs.append((y, c0, c0 + Cout))
            c0 += Cout
        wq, wsc = F8.quantize_weight(torch.cat(ws_rows, 0))
        wq_dev, ws_dev = self._dev(wq), self._dev(wsc)
        cs_dev = self._dev(wsc * xs, torch.float32)
        b_dev = self._dev(torch.cat(bias_parts), torch.float32)
        lo_dev = self._dev(torch.cat(lo_parts), torch.float32)
        self.params += [wq_dev, cs_dev, b_dev, lo_dev]
        self.fp8_layers += len(members)

        def run(x=x, segs=segs, wq=wq_dev, ws=ws_dev, cs=cs_dev, b=b_dev, lo=lo_dev, xs=xs):
            F8.conv2d_nhwc_fp8_multi(_view(x), xs, wq, (1, 1), ws, b, lo,
                                     [(_target(v), a, e, _coff(v), _eff_scale(v) if v.qscale is not None else None)
                                      for v, a, e in segs], chan_scale=cs)

        self._emit("+".join(m["conv"].name for m in members), "conv_fp8", run, [x], [v for v, _, _ in segs],
                   {"impl": "conv_lite_fp8_multi", "multi_out": True})
        for m in members:
            self._fused.add(m["conv"].name)
            for a in m["absorbed"]:
                self._fused.add(a.name)
            if m["kind"] == "pool":
                self._fused.add(m["pool"].name)
                y, out, act = m["y"], m["out"], m["act"]
                bp = self._dev(m["bias"] if m["bias"] is not None else torch.zeros(m["Cout"]), torch.float32)
                self.params.append(bp)

                def run_pool(y=y, out=out, b=bp, act=act, pads=m["pads"]):
                    F8.avgpool_bias_act(y.buf, (3, 3), (1, 1), pads, b, act,
                                        out_scale=_eff_scale(out) if out.qscale is not None else None,
                                        out=_target(out), out_channel_offset=_coff(out))

                self._emit(m["pool"].name, "pool_fp8" if out.qscale is not None else "pool", run_pool, [y], [out],
                           {"impl": "avgpool_bias_act"})
                self.stats["commuted_pools"] += 1
            self._finish_conv(m["last"], m["absorbed"], m["out"])
        self.stats["sibling_groups"] += 1
        return True

    def _commute_avgpool(self, node: Node, x: Val, ksize, pads) -> bool:
        """AvgPool(stride 1) -> 1x1 Conv2D (+ BN/bias, ReLU) lowered as 1x1 conv (no bias or
        act, bf16 out) -> avgpool with the bias + act + fp8 quantisation in its epilogue.
        Both operators are linear and the conv is pointwise, so they commute exactly (the
        pool's count-excluding-padding divisor depends on the position only); the pool then
        runs over Cout instead of Cin channels (Inception's pool branches: 32-192 vs
        192-2048), and in fp8 the pooled value is no longer rounded to e4m3 before the
        conv.  Taken when Cout <= Cin / 2 (the extra bf16 round trip of the conv output is
        cheaper than pooling the wide input)."""
        c = self._single_consumer(node.name)
        if c is None or c.op != "Conv2D" or c.inputs[0][0] != node.name or c.attr("data_format", "NHWC") != "NHWC":
            return False
        if list(c.attr("strides") or [1, 1, 1, 1]) != [1, 1, 1, 1] or list(c.attr("dilations") or [1, 1, 1, 1]) != [1, 1, 1, 1]:
            return False
        wv = self._get(c.inputs[1])
        if wv is None or not wv.is_const or tuple(wv.const.shape[:2]) != (1, 1) or x.phys_c or x.concat_slot is not None:
            return False
        N, H, W, C = x.shape
        w = wv.const.float()
        Cin, Cout = w.shape[2], w.shape[3]
        if Cin != C or C % 16 or Cout % 16 or 2 * Cout > C or x.rows is not None:
            return False
        last, scale, bias, residual, act, absorbed = self._conv_chain(c)
        if residual is not None or act not in _PLAIN_ACTS:
            return False
        fp8_in = x.qscale is not None
        if not fp8_in and x.dtype != torch.bfloat16:
            return False
        if scale is not None:
            w = w * scale
        w_ohwi = w.permute(3, 0, 1, 2).contiguous()
        b_dev = self._dev(bias if bias is not None else torch.zeros(Cout), torch.float32)
        y = self._new((N, H, W, Cout))  # the conv's output before bias / act (bf16, real units)
        o_scale = self._qscale(last.name) if (self.precision == "fp8" and self._fp8_consumers_ok(last.name)) else None
        out = self._new((N, H, W, Cout), torch.uint8 if o_scale is not None else torch.bfloat16)
        out.qscale = o_scale
        zero = self._dev(torch.zeros(Cout), torch.float32)
        if fp8_in:
            wq, ws = F8.quantize_weight(w_ohwi)
            wq_dev, ws_dev, cs_dev = self._dev(wq), self._dev(ws), self._dev(ws * x.qscale, torch.float32)
            self.params += [wq_dev, cs_dev, zero, b_dev]
            self.fp8_layers += 1
            cfg = LITE_FP8_CFG if self.device.type == "cuda" else -1

            def run_conv8(x=x, y=y, wq=wq_dev, ws=ws_dev, cs=cs_dev, zero=zero, cfg=cfg, xs=x.qscale):
                F8.conv2d_nhwc_fp8(_view(x), xs, wq, (1, 1), ws, zero, act=K.ACT_NONE, out=y.buf, chan_scale=cs,
                                   cfg=cfg)

            self._emit(c.name, "conv_fp8", run_conv8, [x], [y], {"impl": "pointwise_before_avgpool"})
        else:
            w_dev = self._dev(w_ohwi, torch.bfloat16)
            self.params += [w_dev, zero, b_dev]

            def run_conv(x=x, y=y, w_dev=w_dev, zero=zero):
                K.conv2d_nhwc(x.buf, w_dev, zero, None, (1, 1), (0, 0, 0, 0), (1, 1), K.ACT_NONE, out=y.buf)

            self._emit(c.name, "conv", run_conv, [x], [y], {"impl": "pointwise_before_avgpool"})

        def run_pool(y=y, out=out, b=b_dev, act=act, ksize=tuple(ksize), pads=tuple(pads)):
            F8.avgpool_bias_act(y.buf, ksize, (1, 1), pads, b, act,
                                out_scale=_eff_scale(out) if out.qscale is not None else None, out=_target(out),
                                out_channel_offset=_coff(out))

        self._emit(node.name, "pool_fp8" if o_scale is not None else "pool", run_pool, [y], [out],
                   {"impl": "avgpool_bias_act"})
        self._fused.add(c.name)
        for a in absorbed:
            self._fused.add(a.name)
        self._finish_conv(last, absorbed, out)
        self.stats["commuted_pools"] += 1
        return True

    # ---- post-passes over the fused block tails
    def _fetched_roots(self) -> set:
        return {id(_root(self._val_of(f))) for f in self.fetch_names}

    def _chain_tails(self):
        """ResNet stage 1's residual stream by recomputation (kernels/bottleneck_chain.hip):
        a fused tail whose residual is the previous tail's y3, read by nothing else, computes
        that y3 again from the previous tails' 64-channel sources (the 3x3 outputs and the
        stem output, kept alive until it) instead of reading the 256-channel tensor, and the
        previous tail stops storing it.  Chains start at the dual (projection) tail and hold
        up to ``chain_max_links`` links (2: tail 1 -> tail 2, the third tail reads y3 again;
        three links still recompute more than the saved traffic buys, also on the
        rescheduled kernels: stage-1 tails 100 + 154 + 256 us against 102 + 176 + 161,
        79.1-80.1k vs 80.6-81.5k records/s, profiles/r07_tail_sched)."""
        if not _cfg().recompute_tails:
            return
        fetched = self._fetched_roots()
        links_of: dict[int, list] = {}
        for st in self.steps:
            t = st.meta.get("tail")
            if t is None or t["w3"] is None:
                continue
            if t["xs"] is not None:  # a chain head: the dual tail
                links_of[id(st)] = [(t["x"], t["xs"], t["w3"], t["b3"])]
                continue
            res = t["res"]
            prods = [p for p in self.steps if p.outputs and p.outputs[0] is res and id(p) in links_of]
            if len(prods) != 1:
                continue
            prev = prods[0]
            prev_links = links_of[id(prev)]
            if len(prev_links) >= _cfg().chain_max_links or id(res) in fetched or res.alias_of is not None or res.concat_slot is not None \
                    or res.buf_shape is not None \
                    or any(v is not res and _root(v) is res for v in self.vals.values()):
                continue
            readers = [r for r in self.steps if r is not prev and any(_root(i) is res for i in r.inputs)]
            if readers != [st]:
                continue
            links = prev_links + [(t["x"], None, t["w3"], t["b3"])]
            links_of[id(st)] = links
            t["chain"]["links"] = links
            st.meta["impl"] = "bottleneck_chain"
            # the sources of every link are this step's inputs (the planner keeps them alive)
            st.inputs = [v for x, xs, _, _ in links for v in ((x,) if xs is None else (x, xs))]
            # the previous tail no longer writes y3 (it runs as a one-or-more-link chain)
            pt = prev.meta["tail"]
            pt["chain"]["links"] = prev_links
            pt["chain"]["store"] = False
            prev.meta["impl"] = "bottleneck_chain"
            prev.outputs = [o for o in prev.outputs if o is not res]
            self.stats["chained_tails"] += 1

    def _decimate_tails(self):
        """A fused block tail's wide output y3 whose only other reader is the next stage's
        stride-2 1x1 projection shortcut (fused into that stage's first expand conv) is
        stored decimated: only the even-(h, w) pixels the projection reads, compact — 1/4 of
        the bytes (ResNet v1.5's stage-1 -> stage-2 boundary: 308 MB less HBM write traffic
        per 256 images); the projection then reads it at stride 1."""
        if not _cfg().decimate_tails:
            return
        fetched = self._fetched_roots()
        for st in self.steps:
            dec = st.meta.get("dec")
            if dec is None:
                continue
            y3 = st.outputs[0]
            if id(y3) in fetched or y3.alias_of is not None or y3.concat_slot is not None \
                    or y3.buf_shape is not None:
                continue
            if any(v is not y3 and _root(v) is y3 for v in self.vals.values()):
                continue  # reshaped / sliced views of y3 read the full layout
            readers = [r for r in self.steps if r is not st and any(_root(i) is y3 for i in r.inputs)]
            if len(readers) != 1:
                continue
            r = readers[0]
            cfg = (r.meta or {}).get("s2cfg")
            N, H, W, C = y3.shape
            if cfg is None or cfg["s2"] != 2 or len(r.inputs) != 2 or r.inputs[1] is not y3 or H % 2 or W % 2 \
                    or tuple(r.outputs[0].shape[1:3]) != (H // 2, W // 2):
                continue
            y3.buf_shape = (N, H // 2, W // 2, C)
            dec["on"] = True
            cfg["s2"] = 1
            self.stats["decimated_tails"] += 1
