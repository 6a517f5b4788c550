"""``GraphBuilder``: emits TF GraphDefs from Python.

Covers the op DSL of the reference's ``EX/common/GraphBuilder.java:10-100`` (div, sub,
resizeBilinear, expandDims, cast, decodeJpeg, constant, variable, placeholder, build /
buildGraphDef) and extends it with the NN ops needed to express the model zoo
(ResNet-50, Inception-v3, MLPs) as real TF graphs that the executor imports and the
compiler lowers onto the CDNA4 kernels.

Every method returns the output tensor name (``"node:0"``); node names are uniquified
under an optional ``name_scope``.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from ..proto.messages import AttrListValue, AttrValue, GraphDef, NodeDef, TensorShapeProto, VersionDef
from ..types.dtypes import DataType
from ..types.tensor import as_tensor
from .graph import Graph
from .tensor_proto import make_tensor_proto


def _t(x) -> str:
    return x if ":" in x or x.startswith("^") else x


class GraphBuilder:
    def __init__(self):
        self.nodes: list[NodeDef] = []
        self._names: set[str] = set()
        self._scope: list[str] = []
        self.variables: dict[str, str] = {}  # var node name -> initializer Assign node

    # ------------------------------------------------------------------ naming
    @contextlib.contextmanager
    def name_scope(self, scope: str):
        self._scope.append(scope)
        try:
            yield
        finally:
            self._scope.pop()

    def _unique(self, base: str) -> str:
        name = "/".join(self._scope + [base]) if self._scope else base
        if name not in self._names:
            self._names.add(name)
            return name
        i = 1
        while f"{name}_{i}" in self._names:
            i += 1
        self._names.add(f"{name}_{i}")
        return f"{name}_{i}"

    def op(self, op_type: str, inputs=(), name: str | None = None, control=(), **attrs) -> str:
        nm = self._unique(name or op_type)
        ins = [_t(i) for i in inputs] + [f"^{c.split(':')[0]}" for c in control]
        nd = NodeDef(name=nm, op=op_type, input=ins, attr={k: _attr(v) for k, v in attrs.items() if v is not None})
        self.nodes.append(nd)
        return f"{nm}:0"

    # ------------------------------------------------------------------ reference DSL
    def constant(self, name: str, value, dtype=None) -> str:
        t = as_tensor(value if not isinstance(value, np.ndarray) else value, dtype=dtype)
        tp = make_tensor_proto(t)
        return self.op("Const", name=name, value=AttrValue(tensor=tp), dtype=DataType(tp.dtype))

    def placeholder(self, name: str, dtype, shape=None) -> str:
        return self.op("Placeholder", name=name, dtype=DataType.of(dtype),
                       shape=TensorShapeProto.of(shape) if shape is not None else TensorShapeProto(unknown_rank=True))

    def variable(self, name: str, dtype, shape) -> str:
        return self.op("VariableV2", name=name, dtype=DataType.of(dtype), shape=TensorShapeProto.of(shape),
                       container=b"", shared_name=b"")

    def variable_with_init(self, name: str, value) -> str:
        t = as_tensor(value)
        init = self.constant(f"{name}/initial_value", t)
        v = self.variable(name, DataType.of(t.dtype if isinstance(t, torch.Tensor) else DataType.STRING), tuple(t.shape))
        asg = self.op("Assign", [v, init], name=f"{name}/Assign", validate_shape=True, use_locking=True)
        self.variables[v.split(":")[0]] = asg.split(":")[0]
        return self.op("Identity", [v], name=f"{name}/read")

    def div(self, x, y, name=None) -> str:
        return self.op("Div", [x, y], name=name)

    def sub(self, x, y, name=None) -> str:
        return self.op("Sub", [x, y], name=name)

    def add(self, x, y, name=None) -> str:
        return self.op("Add", [x, y], name=name)

    def mul(self, x, y, name=None) -> str:
        return self.op("Mul", [x, y], name=name)

    def resize_bilinear(self, images, size, name=None, align_corners=False, half_pixel_centers=None) -> str:
        return self.op("ResizeBilinear", [images, size], name=name, align_corners=align_corners,
                       half_pixel_centers=half_pixel_centers)

    def argmax(self, x, axis, output_type="INT64", name=None) -> str:
        a = self.constant(f"{(name or 'ArgMax')}/dimension", np.asarray(axis, dtype=np.int32))
        return self.op("ArgMax", [x, a], name=name, output_type=DataType.of(output_type))

    def expand_dims(self, x, dim, name=None) -> str:
        return self.op("ExpandDims", [x, dim], name=name)

    def cast(self, x, dst, name=None) -> str:
        return self.op("Cast", [x], name=name, DstT=DataType.of(dst))

    def decode_jpeg(self, contents, channels=3, name=None) -> str:
        return self.op("DecodeJpeg", [contents], name=name, channels=channels)

    # ------------------------------------------------------------------ NN extensions
    def identity(self, x, name=None) -> str:
        return self.op("Identity", [x], name=name)

    def relu(self, x, name=None) -> str:
        return self.op("Relu", [x], name=name)

    def relu6(self, x, name=None) -> str:
        return self.op("Relu6", [x], name=name)

    def depthwise_conv2d(self, x, w, strides=(1, 1), padding="SAME", name=None, dilations=(1, 1)) -> str:
        """``w`` is ``[KH, KW, C, channel_multiplier]``."""
        return self.op("DepthwiseConv2dNative", [x, w], name=name, strides=[1, strides[0], strides[1], 1],
                       padding=padding.encode(), data_format=b"NHWC", dilations=[1, dilations[0], dilations[1], 1])

    def conv2d(self, x, w, strides=(1, 1), padding="SAME", name=None, dilations=(1, 1)) -> str:
        return self.op("Conv2D", [x, w], name=name, strides=[1, strides[0], strides[1], 1], padding=padding.encode(),
                       data_format=b"NHWC", dilations=[1, dilations[0], dilations[1], 1], use_cudnn_on_gpu=True)

    def conv2d_transpose(self, x, w, output_hw, strides=(2, 2), padding="SAME", name=None) -> str:
        """``Conv2DBackpropInput`` of ``x`` with ``w [KH, KW, Cout, Cin]`` to ``output_hw``.  The
        ``input_sizes`` operand is TF's 2-vector ``[Ho, Wo]``, so the graph does not bake in its
        batch."""
        nm = name or "conv2d_transpose"
        sizes = self.constant(f"{nm}/input_sizes", np.asarray(output_hw, dtype=np.int32))
        return self.op("Conv2DBackpropInput", [sizes, w, x], name=nm, strides=[1, strides[0], strides[1], 1],
                       padding=padding.encode(), data_format=b"NHWC", dilations=[1, 1, 1, 1], use_cudnn_on_gpu=True)

    def conv3d(self, x, w, strides=(1, 1, 1), padding="SAME", name=None, dilations=(1, 1, 1)) -> str:
        """``Conv3D`` of NDHWC ``x`` with ``w [KD, KH, KW, Cin, Cout]``."""
        return self.op("Conv3D", [x, w], name=name, strides=[1, *strides, 1], padding=padding.encode(),
                       data_format=b"NDHWC", dilations=[1, *dilations, 1])

    def max_pool3d(self, x, ksize, strides, padding="VALID", name=None) -> str:
        return self.op("MaxPool3D", [x], name=name, ksize=[1, *ksize, 1], strides=[1, *strides, 1],
                       padding=padding.encode(), data_format=b"NDHWC")

    def avg_pool3d(self, x, ksize, strides, padding="VALID", name=None) -> str:
        return self.op("AvgPool3D", [x], name=name, ksize=[1, *ksize, 1], strides=[1, *strides, 1],
                       padding=padding.encode(), data_format=b"NDHWC")

    def fused_batch_norm(self, x, scale, offset, mean, var, epsilon=1e-3, name=None) -> str:
        return self.op("FusedBatchNormV3", [x, scale, offset, mean, var], name=name, epsilon=float(epsilon),
                       is_training=False, data_format=b"NHWC")

    def lrn(self, x, depth_radius=5, bias=1.0, alpha=1.0, beta=0.5, name=None) -> str:
        return self.op("LRN", [x], name=name, depth_radius=int(depth_radius), bias=float(bias), alpha=float(alpha),
                       beta=float(beta))

    def max_pool(self, x, ksize, strides, padding="VALID", name=None) -> str:
        return self.op("MaxPool", [x], name=name, ksize=[1, ksize[0], ksize[1], 1],
                       strides=[1, strides[0], strides[1], 1], padding=padding.encode(), data_format=b"NHWC")

    def avg_pool(self, x, ksize, strides, padding="VALID", name=None) -> str:
        return self.op("AvgPool", [x], name=name, ksize=[1, ksize[0], ksize[1], 1],
                       strides=[1, strides[0], strides[1], 1], padding=padding.encode(), data_format=b"NHWC")

    def mean(self, x, axes, keep_dims=False, name=None) -> str:
        a = self.constant(f"{(name or 'Mean')}/reduction_indices", np.asarray(axes, dtype=np.int32))
        return self.op("Mean", [x, a], name=name, keep_dims=keep_dims)

    def matmul(self, a, b, transpose_a=False, transpose_b=False, name=None) -> str:
        return self.op("MatMul", [a, b], name=name, transpose_a=transpose_a, transpose_b=transpose_b)

    def bias_add(self, x, b, name=None) -> str:
        return self.op("BiasAdd", [x, b], name=name, data_format=b"NHWC")

    def softmax(self, x, name=None) -> str:
        return self.op("Softmax", [x], name=name)

    def reshape(self, x, shape, name=None) -> str:
        s = self.constant(f"{(name or 'Reshape')}/shape", np.asarray(shape, dtype=np.int32))
        return self.op("Reshape", [x, s], name=name)

    def concat(self, xs, axis, name=None) -> str:
        a = self.constant(f"{(name or 'concat')}/axis", np.asarray(axis, dtype=np.int32))
        return self.op("ConcatV2", list(xs) + [a], name=name, N=len(xs))

    def sigmoid(self, x, name=None) -> str:
        return self.op("Sigmoid", [x], name=name)

    def tanh(self, x, name=None) -> str:
        return self.op("Tanh", [x], name=name)

    def clip_by_value(self, x, lo, hi, name=None) -> str:
        nm = name or "clip_by_value"
        lo_c = self.constant(f"{nm}/clip_value_min", np.asarray(lo, dtype=np.float32))
        hi_c = self.constant(f"{nm}/clip_value_max", np.asarray(hi, dtype=np.float32))
        return self.op("ClipByValue", [x, lo_c, hi_c], name=nm)

    def pad(self, x, paddings, value=0, name=None) -> str:
        """``Pad`` of ``x`` by ``paddings [rank, 2]``; a ``value`` other than 0 makes it a ``PadV2``."""
        nm = name or "Pad"
        p = self.constant(f"{nm}/paddings", np.asarray(paddings, dtype=np.int32).reshape(-1, 2))
        if value == 0:
            return self.op("Pad", [x, p], name=nm, Tpaddings=DataType.INT32)
        cv = self.constant(f"{nm}/constant_values", np.asarray(value, dtype=np.float32))
        return self.op("PadV2", [x, p, cv], name=nm, Tpaddings=DataType.INT32)

    def mirror_pad(self, x, paddings, mode="REFLECT", name=None) -> str:
        """``MirrorPad`` of ``x`` by ``paddings [rank, 2]``; ``mode`` is ``REFLECT`` or ``SYMMETRIC``."""
        if mode not in ("REFLECT", "SYMMETRIC"):
            raise ValueError(f"mirror_pad: mode {mode!r} is not REFLECT or SYMMETRIC")
        nm = name or "MirrorPad"
        p = self.constant(f"{nm}/paddings", np.asarray(paddings, dtype=np.int32).reshape(-1, 2))
        return self.op("MirrorPad", [x, p], name=nm, mode=mode.encode(), Tpaddings=DataType.INT32)

    def instance_norm(self, x, gamma, beta, eps=1e-6, name="InstanceNorm") -> str:
        """``tf.contrib.layers.instance_norm`` of NHWC ``x`` node for node: ``nn.moments(x, [1, 2],
        keep_dims=True)`` and ``nn.batch_normalization`` (the form of ``bert_graph.layer_norm`` with
        the two spatial axes).  ``gamma`` / ``beta`` are tensor names of ``[C]`` values."""
        with self.name_scope(name):
            axes = self.constant("moments/mean/reduction_indices", np.asarray([1, 2], np.int32))
            mean = self.op("Mean", [x, axes], name="moments/mean", keep_dims=True, T=DataType.FLOAT, Tidx=DataType.INT32)
            sg = self.op("StopGradient", [mean], name="moments/StopGradient", T=DataType.FLOAT)
            sq = self.op("SquaredDifference", [x, sg], name="moments/SquaredDifference", T=DataType.FLOAT)
            axes2 = self.constant("moments/variance/reduction_indices", np.asarray([1, 2], np.int32))
            var = self.op("Mean", [sq, axes2], name="moments/variance", keep_dims=True, T=DataType.FLOAT,
                          Tidx=DataType.INT32)
            e = self.constant("instancenorm/add/y", np.float32(eps))
            ve = self.add(var, e, name="instancenorm/add")
            rs = self.op("Rsqrt", [ve], name="instancenorm/Rsqrt", T=DataType.FLOAT)
            inv = self.mul(rs, gamma, name="instancenorm/mul")
            xm = self.mul(x, inv, name="instancenorm/mul_1")
            mm = self.mul(mean, inv, name="instancenorm/mul_2")
            sh = self.sub(beta, mm, name="instancenorm/sub")
            return self.add(xm, sh, name="instancenorm/add_1")

    def exp(self, x, name=None) -> str:
        return self.op("Exp", [x], name=name)

    def strided_slice(self, x, begin, end, strides=None, name=None, begin_mask=0, end_mask=0, shrink_axis_mask=0) -> str:
        """``x[begin:end:strides]`` over the leading ``len(begin)`` axes; bit ``d`` of
        ``begin_mask`` / ``end_mask`` opens that side of axis ``d``."""
        nm = name or "StridedSlice"
        strides = [1] * len(begin) if strides is None else strides
        b, e, s = (self.constant(f"{nm}/{k}", np.asarray(v, dtype=np.int32))
                   for k, v in (("begin", begin), ("end", end), ("strides", strides)))
        return self.op("StridedSlice", [x, b, e, s], name=name, begin_mask=int(begin_mask), end_mask=int(end_mask),
                       ellipsis_mask=0, new_axis_mask=0, shrink_axis_mask=int(shrink_axis_mask), Index=DataType.INT32)

    def last_axis_slice(self, x, lo, hi, rank=3, name=None) -> str:
        """``x[..., lo:hi]`` of a rank-``rank`` tensor as one ``StridedSlice``."""
        lead = (1 << (rank - 1)) - 1
        return self.strided_slice(x, [0] * (rank - 1) + [lo], [0] * (rank - 1) + [hi], name=name, begin_mask=lead,
                                  end_mask=lead)

    def decode_boxes(self, encodings, anchors_yxhw, scales=(10.0, 10.0, 5.0, 5.0), name="decode_boxes") -> str:
        """SSD box decoding of ``encodings`` ``[B, N, 4]`` = (ty, tx, th, tw) against the anchor
        table ``anchors_yxhw`` ``[N, 4]`` = (yc, xc, h, w), as ``[B, N, 1, 4]`` corner boxes (the
        ``boxes`` input of ``combined_nms``).  Emitted in primitive ops in one fixed form, which
        ``graph/detection_lowering.py`` documents and recognises; constants are split per
        (y, x) pair so that every op is a plain broadcast."""
        a = np.asarray(anchors_yxhw, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != 4 or len(scales) != 4:
            raise ValueError("decode_boxes: anchors must be [N, 4] and scales four numbers")
        inv = (np.float32(1) / np.asarray(scales, dtype=np.float32)).astype(np.float32)
        with self.name_scope(name):
            t_yx = self.last_axis_slice(encodings, 0, 2, name="t_yx")
            t_hw = self.last_axis_slice(encodings, 2, 4, name="t_hw")
            a_yx = self.constant("anchors_yx", np.ascontiguousarray(a[:, 0:2]))
            a_hw = self.constant("anchors_hw", np.ascontiguousarray(a[:, 2:4]))
            c = self.mul(t_yx, self.constant("inv_scale_yx", inv[0:2]), name="scaled_yx")
            c = self.mul(c, a_hw, name="offset_yx")
            c = self.add(c, a_yx, name="centre")
            s = self.mul(t_hw, self.constant("inv_scale_hw", inv[2:4]), name="scaled_hw")
            s = self.exp(s, name="Exp")
            s = self.mul(s, a_hw, name="size")
            half = self.mul(s, self.constant("half", np.float32(0.5)), name="half_size")
            lo = self.sub(c, half, name="min_corner")
            hi = self.add(c, half, name="max_corner")
            boxes = self.concat([lo, hi], -1, name="corners")
            return self.expand_dims(boxes, self.constant("boxes/dim", np.asarray(2, dtype=np.int32)), name="boxes")

    def combined_nms(self, boxes, scores, max_per_class, max_total, iou_threshold=0.5, score_threshold=0.0,
                     pad_per_class=False, clip_boxes=True, name=None) -> str:
        """``CombinedNonMaxSuppression``; outputs ``:0`` boxes, ``:1`` scores, ``:2`` classes,
        ``:3`` valid_detections.  A scalar argument may be a tensor name instead of a number."""
        nm = name or "CombinedNonMaxSuppression"

        def scalar(key, v, dt):
            return v if isinstance(v, str) else self.constant(f"{nm}/{key}", np.asarray(v, dtype=dt))

        return self.op("CombinedNonMaxSuppression",
                       [boxes, scores, scalar("max_output_size_per_class", max_per_class, np.int32),
                        scalar("max_total_size", max_total, np.int32), scalar("iou_threshold", iou_threshold, np.float32),
                        scalar("score_threshold", score_threshold, np.float32)],
                       name=name, pad_per_class=bool(pad_per_class), clip_boxes=bool(clip_boxes))

    def transpose(self, x, perm, name=None) -> str:
        p = self.constant(f"{(name or 'transpose')}/perm", np.asarray(perm, dtype=np.int32))
        return self.op("Transpose", [x, p], name=name or "transpose", Tperm=DataType.INT32)

    def block_lstm(self, x, w, b, cs_prev, h_prev, seq_len_max, hidden, wci=None, wcf=None, wco=None,
                   forget_bias=1.0, cell_clip=3.0, name=None) -> str:
        """``BlockLSTM`` over time-major ``x [T, B, I]`` with ``w [I + H, 4H]`` / ``b [4H]`` (gate
        columns i, ci, f, o).  Returns the node NAME: the outputs are ``name:0 .. name:6`` =
        i, cs, f, o, ci, co, h.  ``seq_len_max`` is a number or a tensor name; the peephole is on
        when the three vectors are given (else zero vectors of ``hidden`` elements are wired in, as
        TF does)."""
        nm = name or "BlockLSTM"
        peep = wci is not None
        if peep != (wcf is not None) or peep != (wco is not None):
            raise ValueError("block_lstm: the three peephole vectors come together")
        if not isinstance(seq_len_max, str):
            seq_len_max = self.constant(f"{nm}/seq_len_max", np.asarray(seq_len_max, dtype=np.int64))
        if not peep:
            zero = self.constant(f"{nm}/no_peephole", np.zeros((hidden,), dtype=np.float32))
            wci = wcf = wco = zero
        out = self.op("BlockLSTM", [seq_len_max, x, cs_prev, h_prev, w, wci, wcf, wco, b], name=name,
                      forget_bias=float(forget_bias), cell_clip=float(cell_clip), use_peephole=peep, T=DataType.FLOAT)
        return out.split(":")[0]

    def audio_spectrogram(self, x, window_size, stride, magnitude_squared=False, name=None) -> str:
        """``AudioSpectrogram`` of ``x [samples, channels]``: ``[channels, frames, N/2 + 1]``."""
        return self.op("AudioSpectrogram", [x], name=name, window_size=int(window_size), stride=int(stride),
                       magnitude_squared=bool(magnitude_squared))

    def mfcc(self, spectrogram, sample_rate, upper_frequency_limit=4000.0, lower_frequency_limit=20.0,
             filterbank_channel_count=40, dct_coefficient_count=13, name=None) -> str:
        """``Mfcc`` of a squared-magnitude spectrogram; ``sample_rate`` is a number or a tensor name."""
        nm = name or "Mfcc"
        if not isinstance(sample_rate, str):
            sample_rate = self.constant(f"{nm}/sample_rate", np.asarray(sample_rate, dtype=np.int32))
        return self.op("Mfcc", [spectrogram, sample_rate], name=name,
                       upper_frequency_limit=float(upper_frequency_limit),
                       lower_frequency_limit=float(lower_frequency_limit),
                       filterbank_channel_count=int(filterbank_channel_count),
                       dct_coefficient_count=int(dct_coefficient_count))

    def decode_wav(self, contents, desired_channels=-1, desired_samples=-1, name=None) -> str:
        """``DecodeWav``.  Returns the node NAME: ``name:0`` is the audio ``[samples, channels]``,
        ``name:1`` the sample rate."""
        out = self.op("DecodeWav", [contents], name=name, desired_channels=int(desired_channels),
                      desired_samples=int(desired_samples))
        return out.split(":")[0]

    def top_k(self, x, k, name=None) -> str:
        kk = self.constant(f"{(name or 'TopKV2')}/k", np.asarray(k, dtype=np.int32))
        return self.op("TopKV2", [x, kk], name=name, sorted=True)

    def no_op(self, name, control=()) -> str:
        return self.op("NoOp", [], name=name, control=control)

    # ------------------------------------------------------------------ TF1 control flow
    def placeholder_with_default(self, default, name: str, shape=None) -> str:
        return self.op("PlaceholderWithDefault", [default], name=name, dtype=self._dtype_of(default),
                       shape=TensorShapeProto.of(shape) if shape is not None else TensorShapeProto(unknown_rank=True))

    def _dtype_of(self, t: str) -> DataType:
        nd = next(n for n in self.nodes if n.name == t.split(":")[0])
        a = nd.attr.get("dtype") or nd.attr.get("T")
        return DataType(a.type) if a is not None else DataType.FLOAT

    def _guard_new_nodes(self, start: int, pivot: str):
        """Input-less nodes made inside a branch / loop body get a control edge on the pivot
        (as TF's CondContext / WhileContext add), so they live in its frame and die with it."""
        p = "^" + pivot.split(":")[0]
        for nd in self.nodes[start:]:
            if not nd.input:
                nd.input.append(p)

    def cond(self, pred: str, true_fn, false_fn, inputs=(), name: str = "cond") -> str:
        """``tf.cond`` as TF1 emits it: ``Switch`` every input on ``pred``, build each branch
        on its Switch output, ``Merge`` the two results (output 0).  ``true_fn`` / ``false_fn``
        take the switched inputs and return one tensor."""
        with self.name_scope(name):
            sw = self.op("Switch", [pred, pred], name="Switch")
            swn = sw.split(":")[0]
            pivot_t = self.op("Identity", [f"{swn}:1"], name="switch_t")
            pivot_f = self.op("Identity", [f"{swn}:0"], name="switch_f")
            xs = [self.op("Switch", [x, pred], name="Switch").split(":")[0] for x in inputs]
            start = len(self.nodes)
            t = true_fn(*[f"{x}:1" for x in xs])
            self._guard_new_nodes(start, pivot_t)
            start = len(self.nodes)
            f = false_fn(*[f"{x}:0" for x in xs])
            self._guard_new_nodes(start, pivot_f)
            return self.op("Merge", [f, t], name="Merge", N=2)

    def while_loop(self, cond_fn, body_fn, loop_vars, invariants=(), name: str = "while") -> list[str]:
        """``tf.while_loop`` as TF1 emits it: ``Enter`` → ``Merge`` (with the back edge) →
        ``LoopCond`` → ``Switch``; the true side runs the body into ``NextIteration``, the
        false side leaves through ``Exit``.  ``invariants`` enter as loop constants.
        ``cond_fn`` / ``body_fn`` take (*loop vars, *invariants); returns the Exit tensors."""
        with self.name_scope(name):
            frame = "/".join(self._scope)
            enters = [self.op("Enter", [v], name="Enter", frame_name=frame, is_constant=False, parallel_iterations=10)
                      for v in loop_vars]
            invs = [self.op("Enter", [v], name="Enter", frame_name=frame, is_constant=True, parallel_iterations=10)
                    for v in invariants]
            merges = [self.op("Merge", [e, e], name="Merge", N=2) for e in enters]  # back edge patched below
            start = len(self.nodes)
            c = cond_fn(*merges, *invs)
            self._guard_new_nodes(start, merges[0])
            lc = self.op("LoopCond", [c], name="LoopCond")
            sws = [self.op("Switch", [m, lc], name="Switch").split(":")[0] for m in merges]
            exits = [self.op("Exit", [f"{sw}:0"], name="Exit") for sw in sws]
            body_in = [self.op("Identity", [f"{sw}:1"], name="Identity") for sw in sws]
            start = len(self.nodes)
            outs = body_fn(*body_in, *invs)
            outs = [outs] if isinstance(outs, str) else list(outs)
            self._guard_new_nodes(start, body_in[0])
            nexts = [self.op("NextIteration", [o], name="NextIteration") for o in outs]
            for m, nx in zip(merges, nexts):
                nd = next(n for n in self.nodes if n.name == m.split(":")[0])
                nd.input[1] = nx.split(":")[0]
            return exits

    # ------------------------------------------------------------------ output
    def build_graph_def(self) -> GraphDef:
        return GraphDef(node=list(self.nodes), versions=VersionDef(producer=26))

    buildGraphDef = build_graph_def

    def build(self, prefix: str = "") -> Graph:
        return Graph.from_graph_def(self.build_graph_def(), prefix)


def _attr(v) -> AttrValue:
    if isinstance(v, AttrValue):
        return v
    if isinstance(v, DataType):
        return AttrValue(type=int(v))
    if isinstance(v, TensorShapeProto):
        return AttrValue(shape=v)
    if isinstance(v, bool):
        return AttrValue(b=v)
    if isinstance(v, int):
        return AttrValue(i=v)
    if isinstance(v, float):
        return AttrValue(f=v)
    if isinstance(v, (bytes, str)):
        return AttrValue(s=v.encode() if isinstance(v, str) else v)
    if isinstance(v, (list, tuple)):
        if all(isinstance(e, DataType) for e in v) and v:
            return AttrValue(list=AttrListValue(type=[int(e) for e in v]))
        if all(isinstance(e, int) and not isinstance(e, bool) for e in v):
            return AttrValue(list=AttrListValue(i=list(v)))
        if all(isinstance(e, float) for e in v):
            return AttrValue(list=AttrListValue(f=list(v)))
        if all(isinstance(e, (bytes, str)) for e in v):
            return AttrValue(list=AttrListValue(s=[e.encode() if isinstance(e, str) else e for e in v]))
        if all(isinstance(e, TensorShapeProto) for e in v):
            return AttrValue(list=AttrListValue(shape=list(v)))
    raise TypeError(f"cannot convert {v!r} to an AttrValue")
