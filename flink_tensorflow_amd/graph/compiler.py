"""Graph compiler: lowers a (feeds → fetches) signature of a TF graph onto the CDNA4
kernels for fixed input shapes, plans HBM buffers, and captures the launch sequence in
a hipGraph (``torch.cuda.CUDAGraph`` is HIP graph capture on ROCm).

This is the MI355X replacement of libtensorflow's session executor for the hot path
(SURVEY §2.8 N2/N3, §7.3).  Passes:

1. **prune** to the fetched subgraph, stopping at fed tensors;
2. **constant folding** of everything that depends only on Const/variables (weights are
   frozen into the plan; variables are read from the session at compile time);
3. **fusion** (pattern match, TF semantics preserved):
   * ``Conv2D → [BiasAdd | FusedBatchNorm]* → [Add(residual)] → [Relu|Relu6]`` → one
     implicit-GEMM conv launch with BN folded into the weights and a bias+residual+act
     epilogue;
   * ``DepthwiseConv2dNative → [BiasAdd | FusedBatchNorm]* → [Relu|Relu6]`` → one launch of
     the depthwise kernel (3x3 register-tiled or generic), BN folded into the per-channel
     filter; a residual ``Add`` behind it stays an elementwise step;
   * ``Conv2DBackpropInput → [BiasAdd | FusedBatchNorm]* → [Relu|Relu6]`` → one launch of the
     transposed-conv kernel (kernels/deconv.hip, ``deconv_lowering.py``), one implicit GEMM per
     output phase; stride 1 runs as a plain conv with the flipped filter;
   * ``Conv3D → [BiasAdd | FusedBatchNorm]* → [Relu|Relu6]`` → one launch of the 3-D implicit-GEMM
     kernel (kernels/conv3d.hip, ``conv3d_lowering.py``); a conv that is 2-D over the same memory
     (``KD == 1``, or ``KH == KW == 1``) runs on the 2-D kernels; ``MaxPool3D`` / ``AvgPool3D`` → the
     3-D pool kernel; a uint8 clip feed's ``Cast → Mul`` folds into the first conv;
   * ``ResizeBilinear`` of an activation → the bilinear resize kernel (it writes concat
     slots); ``[ResizeBilinear] → ArgMax(channels) → [Cast]`` → one fused resize + ArgMax
     launch that never stores the resized tensor (kernels/resize.hip);
   * ``[decode_boxes subgraph] + [last-axis score slice] → CombinedNonMaxSuppression`` → one
     ``nms`` step: box decoding, per-class greedy NMS and the top-T merge
     (kernels/detection.hip, ``detection_lowering.py``);
   * ``[Transpose] → BlockLSTM → [Transpose | last-step StridedSlice]`` → one projection
     ``gemm`` step plus one ``lstm`` step that walks the whole sequence (kernels/lstm.hip,
     ``recurrent_lowering.py``); the layout ops emit nothing;
   * ``[Cast(INT16) → Mul|RealDiv] → [Transpose] → AudioSpectrogram → Mfcc → [Reshape]`` → one
     ``mfcc`` step from PCM to coefficients (kernels/audio.hip, ``audio_lowering.py``); a lone
     ``AudioSpectrogram`` → one ``spectrogram`` step;
   * ``moments(x, [1, 2]) + batch_normalization`` (``tf.contrib.layers.instance_norm``) ``→ [Relu|Relu6]`` → one
     ``instnorm`` step (kernels/instnorm.hip); ``MirrorPad`` / ``Pad`` / ``PadV2`` of the spatial axes → one ``pad``
     step; ``[Tanh|Sigmoid] → [Mul] → [Add|Sub] → [ClipByValue] → [Cast(UINT8)]`` behind a 1, 3 or 4 channel conv →
     one ``image_out`` step that writes the compact fp32 or uint8 image (kernels/pad.hip,
     ``generator_lowering.py``);
   * ``MatMul → [BiasAdd] → [Add] → [act]`` → one MFMA GEMM launch;
   * ``uint8 feed → Cast → ResizeBilinear → Sub → Div|Mul`` → the fused preprocess kernel
     (bf16 NHWC, channels padded to 8 for the stem conv);
   * ``Mean(axes=[1,2])`` → global-avg-pool; ``MaxPool``/``AvgPool`` → pool kernel;
   * ``Softmax [→ TopKV2]`` → fused softmax+top-k kernel;
   * ``ConcatV2`` on channels → producers write straight into channel slices of one
     buffer (no copy) when every producer is a kernel that supports it;
   * everything else runs as captured PyTorch glue ops (logged; ``strict=True`` rejects).
4. **memory planning**: every intermediate gets an offset in one activation slab from the
   native liveness planner (``csrc/arena.cpp``); with a subtask ``DeviceArena`` the slab is
   shared by all of the subtask's bucket plans and identical weights are stored once;
5. **capture**: one hipGraph per (signature, batch size).

The compiler is twelve modules: ``plan.py`` (``Val``, ``Step``, ``Chain``, ``CompileError`` and the helpers that
map a value to its buffer; re-exported here), ``conv_lowering.py`` (the ``ConvLowering`` mixin: Conv2D chains, the
pure kernel choice ``select_conv_kernel`` and the block-tail post-passes), ``transformer_lowering.py`` (the
``TransformerLowering`` mixin: BERT patterns, token packing), ``detection_lowering.py`` (the ``DetectionLowering``
mixin: box decoding + NMS), ``recurrent_lowering.py`` (the ``RecurrentLowering`` mixin: ``BlockLSTM`` and the layout
ops around it), ``audio_lowering.py`` (the ``AudioLowering`` mixin: the spectrogram / MFCC front end and the
ops it absorbs), ``deconv_lowering.py`` (the ``DeconvLowering`` mixin: ``Conv2DBackpropInput`` chains),
``conv3d_lowering.py`` (the ``Conv3DLowering`` mixin: ``Conv3D`` chains, 3-D pools, uint8 clips),
``generator_lowering.py`` (the ``GeneratorLowering`` mixin: instance norm, spatial pads, the image output stage),
``plan_memory.py`` (the ``PlanMemory`` mixin: buffer planning, the batch-slice chain),
``plan_run.py`` (the ``PlanRunner`` mixin: eager runs, profiling, calibration, capture, replay, the runner's head
bypass) and this one (construction, pruning, folding, scheduling, the generic and glue lowerings).

Activations are bf16 NHWC on device; fetched outputs are cast back to the graph dtype.

``precision="fp8"`` (BASELINE "Inception-v3 fp8 weights"): a bf16 twin of the plan is
first run on calibration inputs to record every activation's absolute maximum; then each
Conv2D chain whose channels are multiples of 16 (and has no residual) is lowered onto the
fp8 MFMA kernel with per-channel e4m3 weights, and its output is stored as e4m3 with a
static per-tensor scale whenever every consumer reads fp8 (convs, pools, concats,
global-average-pool).  Concat branches write with the concat buffer's scale; max/avg
pools requantise on the fly; anything else reads a dequantised bf16 copy.
"""
from __future__ import annotations

import collections
import contextlib
import logging
from typing import Any

import numpy as np
import torch

from ..ops import fp8 as F8
from ..ops import kernels as K
from ..types.dtypes import DataType
from ..types.names import TensorName
from ..utils import tracing
from . import ops_core  # noqa: F401
from .audio_lowering import AudioLowering
from .conv3d_lowering import Conv3DLowering
from .conv_lowering import _ACTS, ConvLowering
from .deconv_lowering import DeconvLowering
from .detection_lowering import _UNPADDED_NMS, DetectionLowering
from .generator_lowering import _IMAGE_OUT_OPS, _PAD_OPS, GeneratorLowering
from .graph import Graph, Node
from .op_registry import OpContext, lookup
from .ops_nn import same_pads
from .plan import Chain, CompileError, Step, Val, _coff, _eff_scale, _host, _target, _view
from .plan_memory import PlanMemory
from .plan_run import PlanRunner
from .recurrent_lowering import RecurrentLowering
from .transformer_lowering import TransformerLowering

__all__ = ["CompiledFunction", "CompileError", "Step", "Val", "compile_signature"]

LOG = logging.getLogger("flink_tensorflow_amd.compiler")

# plan counters reported by ``summary()``, in its order
_STATS = ("fused_shortcuts", "fused_tails", "decimated_tails", "fused_pools", "conv3x3c64", "pw_res", "chained_tails",
          "conv_lite", "commuted_pools", "sibling_groups", "fused_preprocess")

_BINARY = {"Add": "add", "AddV2": "add", "Sub": "sub", "Mul": "mul", "RealDiv": "div", "Div": "div",
           "Maximum": "max", "Minimum": "min"}


class _ConstSession:
    """Minimal session facade for folding constants through interpreter kernels."""

    def __init__(self, variables):
        self.variables = variables
        self._const_cache = {}


class CompiledFunction(GeneratorLowering, TransformerLowering, DetectionLowering, RecurrentLowering, AudioLowering,
                       DeconvLowering, Conv3DLowering, ConvLowering, PlanMemory, PlanRunner):
    def __init__(self, graph: Graph, feeds: dict[str, tuple[tuple, Any]], fetches: list[str], device,
                 variables: dict | None = None, use_graph: bool = True, strict: bool = False,
                 topk_fetch: bool = True, precision: str = "bf16", calibration: dict | None = None,
                 arena=None, token_capacity: int | None = None):
        if precision not in ("bf16", "fp8"):
            raise ValueError(f"precision must be bf16 or fp8, not {precision!r}")
        from .control_flow import fold_static_control_flow
        from .functions import has_functional_ops, lower_functional_ops

        # function calls / functional If / While inline into plain dataflow first; then TF1
        # conds on compile-time-constant predicates (an exported ``is_training`` switch left
        # at its default) resolve before lowering: the plan is the cond-free one
        if has_functional_ops(graph):
            graph = lower_functional_ops(graph)
        graph = fold_static_control_flow(graph, list(feeds), list(fetches))
        self.graph = graph
        self.arena = arena  # subtask DeviceArena (shared slab + interned weights) or None
        # padding-free transformer plan: token rows packed into this capacity (graph/packed.py)
        self.token_cap = token_capacity
        self._pack: dict | None = None
        self._cls_nodes: set[str] = set()
        self._cur_cls = False
        self._cls_cache: dict[int, Val] = {}
        self.activation_bytes = 0
        self.precision = precision
        self.device = torch.device(device)
        if self.device.type != "cuda":
            use_graph = False  # host plans run the fp32 reference ops (used by CPU tests)
        self.feed_names = [str(TensorName.parse(f)) for f in feeds]
        self.feed_specs = {str(TensorName.parse(f)): v for f, v in feeds.items()}
        self.fetch_names = [str(TensorName.parse(f)) for f in fetches]
        self._fetched_nodes = frozenset(TensorName.parse(f).name for f in fetches)
        self.variables = variables or {}
        self.strict = strict
        self.steps: list[Step] = []
        self.params: list[torch.Tensor] = []  # device weights/biases baked into the plan
        self.glue_ops: list[str] = []
        self.vals: dict[tuple[str, int], Val] = {}
        self._fused: set[str] = set()
        self._const_sess = _ConstSession(self.variables)
        self._input_bufs: dict[str, torch.Tensor] = {}
        self._outputs: list = []
        self._graph_obj: torch.cuda.CUDAGraph | None = None
        # graph of steps[1:] and the (feed, step) of steps[0] when that is a head (``_head_feed_step``)
        self._graph_tail: torch.cuda.CUDAGraph | None = None
        self._head: tuple[str, Step] | None = None
        self._amax: dict[str, float] = {}
        self.fp8_layers = 0
        self.stats = collections.Counter(dict.fromkeys(_STATS, 0))
        self._debug_sync = tracing.debug_sync()
        self._poison_after: dict[int, list] = {}
        self._chain: Chain | None = None  # the batch-slice chain (``PlanMemory._find_chain``)
        if self._debug_sync or tracing.debug_poison():
            use_graph = False  # debug modes act between launches: run the plan eagerly
        if precision == "fp8":  # calibrate activation ranges on a bf16 twin of the plan
            twin = CompiledFunction(graph, feeds, fetches, device, variables, use_graph=False, strict=strict)
            self._amax = twin.calibrate(calibration)
            del twin

        with torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext():
            self._compile()
            self._plan_memory_and_bind()
            if use_graph:
                self._capture()

    # ================================================================== compile
    def _compile(self):
        g = self.graph
        fed = {TensorName.parse(f) for f in self.feed_names}
        fed_nodes = {f.name for f in fed}
        needed, stack = set(), [TensorName.parse(f).name for f in self.fetch_names]
        while stack:
            n = stack.pop()
            if n in needed:
                continue
            needed.add(n)
            if n in fed_nodes:
                continue
            node = g[n]
            stack.extend(s for s, _ in node.inputs)
            stack.extend(node.control_inputs)
        self.order = [n for n in g.topo_order(needed)]
        self.needed = needed
        # consumers restricted to the pruned subgraph
        self.cons: dict[str, list[str]] = {}
        for n in self.order:
            for s, _ in g[n].inputs:
                self.cons.setdefault(s, []).append(n)
        self._groups = {}
        self._prematch_transformer()  # layer_norm / attention / embedding patterns (BERT graphs)
        self._prematch_detection()  # the box-decode subgraph in front of a CombinedNonMaxSuppression
        if self.token_cap is not None:
            self._setup_packing()  # CompileError when the graph cannot run token-packed
        for f in fed:
            shape, dt = self.feed_specs[str(f)]
            dt = DataType.of(dt).torch
            self.vals[(f.name, f.index)] = Val(tuple(shape), dt)
        # Lower in topological order, but defer a Conv2D/MatMul whose fused chain ends in a
        # residual Add until the other Add operand has been lowered (DFS topo order often
        # visits the main path before the shortcut branch).
        pending: list[str] = []

        def ready(n: str, allow_unfused: bool = False) -> bool:
            node = g[n]
            if any(src not in self.vals for src in node.inputs):
                return False
            return allow_unfused or node.op not in ("Conv2D", "MatMul") or self._residual_ready(node)

        def drain(allow_unfused=False):
            progress = True
            while pending and progress:
                progress = False
                for p in list(pending):
                    if p in self._fused:
                        pending.remove(p)
                        progress = True
                    elif ready(p, allow_unfused):
                        pending.remove(p)
                        self._lower(g[p])
                        progress = True

        for name in self.order:
            if name in fed_nodes or name in self._fused:
                continue
            if not ready(name):
                pending.append(name)
                continue
            self._lower(g[name])
            drain()
        while pending:  # residual fusion impossible for what is left: lower unfused
            before = len(pending)
            drain(allow_unfused=True)
            if len(pending) == before:
                raise CompileError(f"cannot schedule nodes {pending[:5]}")
        for f in self.fetch_names:
            tn = TensorName.parse(f)
            if (tn.name, tn.index) not in self.vals:
                raise CompileError(f"fetch {f} was not produced by the plan")
            if self.vals[(tn.name, tn.index)].rows is not None:
                raise CompileError(f"fetch {f} is a token-packed tensor (fetch a per-sequence output)")
        self._decimate_tails()
        self._chain_tails()

    def _qscale(self, name: str) -> float | None:
        a = self._amax.get(name)
        return None if a is None else F8.scale_for(a)

    def _fp8_consumers_ok(self, name: str) -> bool:
        """True when ``name``'s value may be stored as fp8: not fetched, and every consumer
        reads fp8 natively."""
        if self._fetched(name):
            return False
        cons = self.cons.get(name, [])
        return bool(cons) and all(self.graph[c].op in ("Conv2D", "MaxPool", "AvgPool", "ConcatV2", "Mean")
                                  for c in cons)

    # ------------------------------------------------------------------ helpers
    def _fetched(self, name: str) -> bool:
        """Some output of graph node ``name`` is fetched."""
        return name in self._fetched_nodes

    def _readers(self, v: Val) -> set | None:
        """The consumers of the graph nodes whose value is ``v``; None when one of those nodes is fetched."""
        names = [n for (n, _), u in self.vals.items() if u is v]
        if any(self._fetched(n) for n in names):
            return None
        return {c for n in names for c in self.cons.get(n, [])}

    def _val_of(self, tensor_name: str) -> Val:
        """The value of a feed or fetch, by its tensor name (``node:index``)."""
        tn = TensorName.parse(tensor_name)
        return self.vals[(tn.name, tn.index)]

    def _in(self, node: Node, i: int) -> Val:
        s, k = node.inputs[i]
        v = self._get((s, k))
        if v is None:
            raise CompileError(f"input {s}:{k} of {node.name} not available")
        return v

    def _get(self, src: tuple[str, int]) -> Val | None:
        v = self.vals.get(src)
        if v is not None and self._cur_cls and v.rows == "packed":
            return self._cls_gather(v)  # first-token-only region: read each sequence's first row
        return v if v is not None else self._const_val(src)

    def _single_consumer(self, name: str) -> Node | None:
        c = self.cons.get(name, [])
        if len(c) != 1 or self._fetched(name):
            return None
        return self.graph[c[0]]

    def _const_val(self, src: tuple[str, int]) -> Val | None:
        """Value of ``src`` if it is (or can be folded to) a constant, folding on demand
        (DFS topo order may reach a consumer before its constant operands)."""
        v = self.vals.get(src)
        if v is not None:
            return v if v.is_const else None
        node = self.graph.nodes.get(src[0])
        if node is None or node.name not in self.needed:
            return None
        for s in node.inputs:
            if self._const_val(s) is None:
                return None
        if node.op in ("Placeholder", "PlaceholderV2"):
            return None
        try:
            ok = self._fold(node)
        except CompileError:
            return None
        v = self.vals.get(src)
        return v if ok and v is not None and v.is_const else None

    def _residual_ready(self, node: Node) -> bool:
        """True unless ``node``'s fusible chain contains an Add whose other operand is a
        not-yet-lowered (non-constant) value."""
        cur = node
        for _ in range(8):
            nxt = self._single_consumer(cur.name)
            if nxt is None:
                return True
            if nxt.op in ("Add", "AddV2"):
                other = [nxt.inputs[i] for i, (s, _) in enumerate(nxt.inputs) if s != cur.name]
                if len(other) != 1:
                    return True
                src = other[0]
                if src in self.vals:
                    return True
                # constants get folded when reached; only wait for computed values
                return self.graph[src[0]].op in ("Const",)
            if nxt.op in ("BiasAdd",) or nxt.op.startswith("FusedBatchNorm") or nxt.op in _ACTS:
                cur = nxt
                continue
            return True
        return True

    def _fold(self, node: Node) -> bool:
        """Constant-fold ``node`` if all its data inputs are constants."""
        ins = [self.vals.get((s, k)) for s, k in node.inputs]
        if node.op in ("Placeholder", "PlaceholderV2"):
            raise CompileError(f"placeholder {node.name} must be fed")
        if node.op in ("VariableV2", "Variable", "VarHandleOp"):
            name = node.attr("shared_name") or node.name
            v = self.variables.get(name)
            if v is None:
                raise CompileError(f"variable {name} is uninitialized at compile time")
            self.vals[(node.name, 0)] = Val(tuple(v.shape), getattr(v, "dtype", None), const=_host(v))
            return True
        if any(v is None or not v.is_const for v in ins):
            return False
        ctx = OpContext(self._const_sess, torch.device("cpu"))
        outs = lookup(node.op)(ctx, node, *[v.const for v in ins])
        for k, o in enumerate(outs):
            if isinstance(o, ops_core.VarRef):
                o = o.read()
            o = _host(o)
            self.vals[(node.name, k)] = Val(tuple(o.shape), getattr(o, "dtype", None), const=o)
        return True

    def _new(self, shape, dtype=torch.bfloat16, phys_c=None) -> Val:
        return Val(tuple(int(s) for s in shape), dtype, phys_c=phys_c)

    def _emit(self, name, kind, fn, inputs, outputs, meta=None, head=None):
        self.steps.append(Step(name, kind, fn, list(inputs), list(outputs), dict(meta or {}), head))

    # ------------------------------------------------------------------ lowering
    def _lower(self, node: Node):
        if self._fold(node):
            return
        self._cur_cls = node.name in self._cls_nodes
        try:
            self._lower_node(node)
        finally:
            self._cur_cls = False

    _ROW_OPS = ("MatMul", "Reshape", "StridedSlice", "Identity", "StopGradient", "Snapshot", "NoOp")

    def _lower_node(self, node: Node):
        grp = self._groups.get(node.name)
        if grp is not None and not grp["done"] and self._lower_group(grp):
            return
        if self._pack is not None and node.op not in self._ROW_OPS:
            for s in node.inputs:  # packed rows reach only row-wise lowerings
                v = self.vals.get(s)
                if v is not None and v.rows is not None:
                    raise CompileError(f"{node.op} {node.name} reads token-packed rows; no packed lowering")
        op = node.op
        if op == "Conv2D":
            return self._lower_conv(node)
        if op == "DepthwiseConv2dNative":
            return self._lower_dwconv(node)
        if op == "Conv2DBackpropInput":
            return self._lower_deconv(node)
        if op == "Conv3D":
            return self._lower_conv3d(node)
        if op in ("MaxPool3D", "AvgPool3D"):
            return self._lower_pool3d(node)
        if op in _PAD_OPS:
            return self._lower_pad(node)
        if op in _IMAGE_OUT_OPS and self._lower_image_out(node):
            return
        if op == "MatMul":
            return self._lower_matmul(node)
        if op == "Cast" and self._try_preprocess(node):
            return
        if op == "Cast" and self._lower_clip_cast(node):
            return
        if op == "ResizeBilinear":
            return self._lower_resize(node)
        if op == "ArgMax":
            return self._lower_argmax(node)
        if op == "CombinedNonMaxSuppression":
            return self._lower_combined_nms(node)
        if op in _UNPADDED_NMS:
            return self._lower_unpadded_nms(node)
        if op == "BlockLSTM":
            return self._lower_block_lstm(node)
        if op == "Transpose" and self._lower_tb_transpose(node):
            return
        if op in ("Cast", "Transpose", "AudioSpectrogram") and self._lower_audio_from(node):
            return
        if op in ("MaxPool", "AvgPool"):
            return self._lower_pool(node)
        if op == "Mean":
            if self._lower_mean(node) or self._lower_mean3d(node):
                return
        if op == "Softmax":
            return self._lower_softmax(node)
        if op in ("Identity", "StopGradient", "Snapshot"):
            self.vals[(node.name, 0)] = self._in(node, 0)
            return
        if op == "IdentityN":  # e.g. an inlined function call's outputs (graph/functions.py)
            for i in range(len(node.inputs)):
                self.vals[(node.name, i)] = self._in(node, i)
            return
        if op == "Reshape":
            return self._lower_reshape(node)
        if op in ("StridedSlice", "Slice") and self._lower_score_slice(node):
            return
        if op == "StridedSlice" and self._lower_strided_slice(node):
            return
        if op in ("Squeeze", "ExpandDims") and self._lower_squeeze_like(node):
            return
        if op == "ConcatV2":
            return self._lower_concat(node)
        if op == "NoOp":
            return
        if op == "LRN" and self._lower_lrn(node):
            return
        if op in _BINARY and self._lower_binary(node):
            return
        if op in _ACTS and self._lower_unary_act(node):
            return
        if op == "Cast" and self._lower_float_cast(node):
            return
        return self._lower_glue(node)

    # ---- standalone elementwise / LRN (ops no producer epilogue absorbed)
    def _ew_ok(self, v: Val) -> bool:
        # bf16 activations, fp8 activations (dequantised first) or fed fp32 tensors (cast first)
        return v is not None and not v.is_const and v.dtype in (torch.bfloat16, torch.uint8, torch.float32) and \
            (v.qscale is not None or v.dtype != torch.uint8) and not v.phys_c and int(np.prod(v.shape)) % 8 == 0

    def _lower_binary(self, node: Node) -> bool:
        a, b = self._get(node.inputs[0]), self._get(node.inputs[1])
        op = _BINARY[node.op]
        if a is not None and a.is_const and b is not None and not b.is_const:
            a, b = b, a
            op = {"sub": "rsub", "div": "rdiv"}.get(op, op)
        if not self._ew_ok(a) or b is None:
            return False
        if b.is_const:
            c = b.const.float().reshape(-1) if isinstance(b.const, torch.Tensor) else None
            if c is None:
                return False
            if c.numel() == 1:
                operand, kind = float(c.item()), "scalar"
            elif c.numel() == a.shape[-1] and c.numel() % 8 == 0 and len(b.const.shape) == 1:
                operand, kind = c.to(self.device).contiguous(), "vector"
                self.params.append(operand)
            else:
                return False
        else:
            if not self._ew_ok(b) or tuple(b.shape) != tuple(a.shape):
                return False
            operand, kind = None, "tensor"
        xa = self._as_bf16(a, node.name + "/a")
        xb = self._as_bf16(b, node.name + "/b") if kind == "tensor" else None
        out = self._new(a.shape)

        def run(xa=xa, xb=xb, out=out, operand=operand):
            K.binary(_view(xa), _view(xb) if xb is not None else operand, op, out=out.buf)

        self._emit(node.name, "elementwise", run, [xa] + ([xb] if xb is not None else []), [out])
        self.vals[(node.name, 0)] = out
        return True

    def _lower_unary_act(self, node: Node) -> bool:
        x = self._get(node.inputs[0])
        if not self._ew_ok(x):
            return False
        xa = self._as_bf16(x, node.name)
        out = self._new(x.shape)
        act = _ACTS[node.op]

        def run(xa=xa, out=out):
            K.binary(_view(xa), 0.0, "add", act=act, out=out.buf)

        self._emit(node.name, "elementwise", run, [xa], [out])
        self.vals[(node.name, 0)] = out
        return True

    def _lower_float_cast(self, node: Node) -> bool:
        x = self._get(node.inputs[0])
        dst = node.attr("DstT")
        if x is None or x.is_const or x.dtype != torch.bfloat16 or DataType.of(dst).torch not in (
                torch.float32, torch.bfloat16, torch.float16):
            return False
        self.vals[(node.name, 0)] = x  # device activations are bf16 either way
        return True

    def _lower_lrn(self, node: Node) -> bool:
        x = self._get(node.inputs[0])
        if not self._ew_ok(x) or len(x.shape) != 4 or x.shape[-1] % 8 or node.attr("depth_radius", 5) > 8:
            return False
        xa = self._as_bf16(x, node.name)
        out = self._new(x.shape)
        r, bias = int(node.attr("depth_radius", 5)), float(node.attr("bias", 1.0))
        alpha, beta = float(node.attr("alpha", 1.0)), float(node.attr("beta", 0.5))

        def run(xa=xa, out=out):
            K.lrn(_view(xa), r, bias, alpha, beta, out=out.buf)

        self._emit(node.name, "lrn", run, [xa], [out])
        self.vals[(node.name, 0)] = out
        return True

    # ---- matmul chain
    def _lower_matmul(self, node: Node):
        a = self._in(node, 0)
        b = self._in(node, 1)
        if not b.is_const or node.attr("transpose_a", False) or len(a.shape) != 2:
            return self._lower_glue(node)
        wt = b.const.float()
        w_nk = wt if node.attr("transpose_b", False) else wt.t()
        N, Kd = w_nk.shape
        if Kd % 8:
            return self._lower_glue(node)
        last, scale, bias, residual, act, absorbed = self._conv_chain(node)
        if act == K.ACT_NONE and residual is None:
            gm = self._match_gelu(last)  # BERT's tanh GELU subgraph -> the GEMM's GELU epilogue
            if gm is not None:
                last, extra = gm
                act = K.ACT_GELU
                absorbed = absorbed + extra
        if scale is not None:
            w_nk = w_nk * scale[:, None]
        n_pad = -(-N // 8) * 8  # e.g. 1001 classes: zero rows, output rows strided by n_pad
        if n_pad != N and residual is not None:
            return self._lower_glue(node)
        if n_pad != N:
            w_nk = torch.nn.functional.pad(w_nk, (0, 0, 0, n_pad - N))
            bias = torch.nn.functional.pad(bias if bias is not None else torch.zeros(N), (0, n_pad - N))
        w_dev = self._dev(w_nk, torch.bfloat16)
        b_dev = self._dev(bias, torch.float32) if bias is not None else None
        self.params += [w_dev] + ([b_dev] if b_dev is not None else [])
        out = self._new((a.shape[0], N), phys_c=n_pad if n_pad != N else None)
        out.rows = a.rows
        out.lshape = (*a.lshape[:-1], N) if a.lshape else None
        if n_pad != N:
            out.buf_shape = (a.shape[0], n_pad)
        res_val = self._get(residual[0].inputs[residual[1]]) if residual is not None else None
        if res_val is not None and (res_val.rows != a.rows or tuple(res_val.shape) != tuple(out.shape)):
            if a.rows is not None or res_val.rows is not None:
                raise CompileError(f"{node.name}: residual rows do not match the packed GEMM rows")
        xin = self._as_bf16(a, node.name)
        for n in absorbed:
            self._fused.add(n.name)

        M = a.shape[0]
        if self.device.type == "cuda" and Kd % 64 == 0:
            # ping-pong MFMA GEMM; small-M heads (e.g. the 256 x 2048 -> 1000 classifier)
            # run split-K through this step's own fp32 workspace
            splits = K.gemm_pp_splits(M, n_pad, Kd)
            ws = torch.empty(splits * M * n_pad, dtype=torch.float32, device=self.device) if splits > 1 else None

            def run_pp(xin=xin, out=out, res_val=res_val, w_dev=w_dev, b_dev=b_dev, splits=splits, ws=ws):
                K.gemm_pp(xin.buf, w_dev, b_dev, res_val.buf if res_val is not None else None, act, out=out.buf,
                          splits=splits, ws=ws)

            self._emit(node.name, "gemm", run_pp, [xin] + ([res_val] if res_val else []), [out],
                       {"impl": "gemm_pp", "splits": splits})
            return self._finish_conv(last, absorbed, out)

        def run(xin=xin, out=out, res_val=res_val, w_dev=w_dev, b_dev=b_dev):
            K.gemm(xin.buf, w_dev, b_dev, res_val.buf if res_val is not None else None, act, out=out.buf)

        self._emit(node.name, "gemm", run, [xin] + ([res_val] if res_val else []), [out])
        self._finish_conv(last, absorbed, out)

    def _as_bf16(self, v: Val, name: str) -> Val:
        if v.dtype == torch.bfloat16:
            return v
        y = self._new(v.shape)
        if v.qscale is not None:
            def deq(v=v, y=y):
                F8.dequantize(_view(v), _eff_scale(v), out=y.buf)

            self._emit(name + "/dequant", "dequant", deq, [v], [y])
            return y

        def run(v=v, y=y):
            y.buf.copy_(v.buf)

        self._emit(name + "/to_bf16", "glue", run, [v], [y])
        return y

    # ---- preprocess: uint8 → Cast → ResizeBilinear → Sub → Div|Mul
    def _try_preprocess(self, cast: Node) -> bool:
        x = self._in(cast, 0)
        if x.is_const or x.dtype != torch.uint8 or len(x.shape) != 4 or x.shape[3] != 3:
            return False
        chain = [cast]
        cur = cast
        size = None
        mean = torch.zeros(3)
        std = torch.ones(3)
        align = half = False
        nxt = self._single_consumer(cur.name)
        if nxt is not None and nxt.op == "ResizeBilinear":
            sv = self._get(nxt.inputs[1])
            if sv is None or not sv.is_const:
                return False
            size = tuple(int(v) for v in sv.const.reshape(-1).tolist())
            align = nxt.attr("align_corners", False)
            half = nxt.attr("half_pixel_centers", False)
            chain.append(nxt)
            cur = nxt
            nxt = self._single_consumer(cur.name)
        if nxt is not None and nxt.op == "Sub":
            mv = self._get(nxt.inputs[1])
            if mv is not None and mv.is_const and nxt.inputs[0][0] == cur.name:
                mean = mean + mv.const.float().reshape(-1).expand(3)
                chain.append(nxt)
                cur = nxt
                nxt = self._single_consumer(cur.name)
        if nxt is not None and nxt.op in ("Div", "RealDiv", "Mul"):
            sv2 = self._get(nxt.inputs[1])
            if sv2 is not None and sv2.is_const and nxt.inputs[0][0] == cur.name:
                f = sv2.const.float().reshape(-1).expand(3)
                std = std * f if nxt.op != "Mul" else std / f
                chain.append(nxt)
                cur = nxt
        if size is None:
            size = (x.shape[1], x.shape[2])
        out = self._new((x.shape[0], size[0], size[1], 3), phys_c=8)
        out.buf_shape = (x.shape[0], size[0], size[1], 8)
        out.pre_cfg = {"s2d": False}
        out.pre_chain = {n.name for n in chain}
        # what a stem conv needs to absorb this kernel (dconv_u8s2d): no resize, the affine only
        out.pre_params = {"x": x, "mean": tuple(mean.tolist()), "std": tuple(std.tolist()),
                          "resize": size != (x.shape[1], x.shape[2])}
        for n in chain[1:]:
            self._fused.add(n.name)
        mean_t, std_t = tuple(mean.tolist()), tuple(std.tolist())

        def head(src, dst):  # ``s2d`` is read per launch: the stem conv flips it after this step is emitted
            K.preprocess_images(src, size, mean_t, std_t, align, half, out=dst, s2d=out.pre_cfg["s2d"])

        self._emit(cast.name + "/preprocess", "preprocess", lambda: head(x.buf, out.buf), [x], [out], head=head)
        for n in chain:
            self.vals[(n.name, 0)] = out
        return True

    # ---- bilinear resize / ArgMax (dense prediction heads: kernels/resize.hip)
    def _resize_source_ok(self, x: Val | None, pitch8: bool) -> bool:
        """``x`` is a 4-D activation the resize kernels can read: bf16 (a channel-padded
        buffer included when ``pitch8`` only asks for a pitch of 8-channel vectors), fed fp32
        or fp8 (both through ``_as_bf16``)."""
        if x is None or x.is_const or len(x.shape) != 4 or x.pre_cfg is not None or x.rows is not None:
            return False
        if x.dtype == torch.bfloat16 and pitch8:
            return (x.phys_c or x.shape[-1]) % 8 == 0
        if x.dtype == torch.bfloat16:
            return not x.phys_c and x.shape[-1] % 8 == 0
        return (x.dtype == torch.float32 or x.qscale is not None) and not x.phys_c and x.shape[-1] % 8 == 0

    def _argmax_ok(self, node: Node, shape: tuple) -> bool:
        """An ``ArgMax`` over the last axis of a 4-D value with at most 256 channels."""
        av = self._get(node.inputs[1])
        if av is None or not av.is_const or len(shape) != 4 or not 1 <= shape[-1] <= 256:
            return False
        return int(av.const.reshape(-1)[0].item()) % 4 == 3 and \
            node.attr("output_type", DataType.INT64).torch in (torch.int32, torch.int64)

    def _lower_resize(self, node: Node):
        """``ResizeBilinear`` of an activation as one ``resize`` step (it can write a concat
        slot).  When its only consumer is a lowerable ``ArgMax`` and it is not fetched it
        emits nothing: the ``ArgMax`` interpolates on the fly (``_lower_argmax``)."""
        x = self._in(node, 0)
        sv = self._get(node.inputs[1])
        if sv is None or not sv.is_const or x.is_const or len(x.shape) != 4:
            return self._lower_glue(node)
        Ho, Wo = (int(v) for v in sv.const.reshape(-1).tolist())
        N, _, _, C = x.shape
        geo = (bool(node.attr("align_corners", False)), bool(node.attr("half_pixel_centers", False)))
        if Ho < 1 or Wo < 1:
            return self._lower_glue(node)
        nxt = self._single_consumer(node.name)
        if nxt is not None and nxt.op == "ArgMax" and nxt.inputs[0][0] == node.name \
                and self._argmax_ok(nxt, (N, Ho, Wo, C)) and self._resize_source_ok(x, pitch8=True):
            out = self._new((N, Ho, Wo, C))
            out.resize_of = (x, *geo)  # no step, no buffer: read only by that ArgMax
            self.vals[(node.name, 0)] = out
            return
        # a channel-padded bf16 producer (a conv of e.g. 21 classes) is resized at its padded
        # width: the padding is zeros and stays zeros, the result is padded the same way
        phys = x.phys_c if x.dtype == torch.bfloat16 and x.phys_c and x.phys_c % 8 == 0 else None
        if not self._resize_source_ok(x, pitch8=phys is not None):
            return self._lower_glue(node)
        xin = self._as_bf16(x, node.name)
        out = self._new((N, Ho, Wo, C), phys_c=phys)
        cr = phys or C

        def run(xin=xin, out=out):
            K.resize_bilinear_nhwc(xin.buf, (Ho, Wo), geo[0], geo[1], out=_target(out), out_channel_offset=_coff(out),
                                   channels=cr)

        self._emit(node.name, "resize", run, [xin], [out])
        self.vals[(node.name, 0)] = out

    def _lower_argmax(self, node: Node):
        """``ArgMax`` over the channels of a 4-D value as one ``resize_argmax`` step: fused
        with the ``ResizeBilinear`` it absorbed, else with identity geometry.  A channel-padded
        producer is read in place (the kernel takes the logical ``C``); a ``Cast`` to an
        integer type that is the only consumer becomes the store type."""
        x = self._in(node, 0)
        if x.is_const or not self._argmax_ok(node, tuple(x.shape)):
            return self._lower_glue(node)
        src, align, half = x.resize_of or (x, False, False)
        if not self._resize_source_ok(src, pitch8=True):
            return self._lower_glue(node)
        N, Ho, Wo, C = x.shape
        dtype = node.attr("output_type", DataType.INT64).torch
        cast = self._single_consumer(node.name)
        if cast is not None and cast.op == "Cast" and \
                DataType.of(cast.attr("DstT")).torch in (torch.uint8, torch.int32, torch.int64):
            dtype = DataType.of(cast.attr("DstT")).torch  # C <= 256: every label fits a byte
            self._fused.add(cast.name)
        else:
            cast = None
        xin = self._as_bf16(src, node.name)
        out = self._new((N, Ho, Wo), dtype)

        def run(xin=xin, out=out):
            K.resize_argmax_nhwc(xin.buf, (Ho, Wo), align, half, channels=C, out=out.buf)

        self._emit(node.name, "resize_argmax", run, [xin], [out], {"fused_resize": src is not x})
        self.vals[(node.name, 0)] = out
        if cast is not None:
            self.vals[(cast.name, 0)] = out

    # ---- pooling / reductions / softmax
    def _lower_pool(self, node: Node):
        x = self._in(node, 0)
        if node.attr("data_format", "NHWC") != "NHWC" or x.phys_c or x.shape[-1] % 8:
            return self._lower_glue(node)
        k = node.attr("ksize")
        s = node.attr("strides")
        kh, kw, sh, sw = k[1], k[2], s[1], s[2]
        N, H, W, C = x.shape
        if node.attr("padding", "VALID") == "SAME":
            pt, pb = same_pads(H, kh, sh)
            pl, pr = same_pads(W, kw, sw)
        else:
            pt = pb = pl = pr = 0
        Ho = (H + pt + pb - kh) // sh + 1
        Wo = (W + pl + pr - kw) // sw + 1
        mode = "max" if node.op == "MaxPool" else "avg"
        if mode == "avg" and self.precision == "fp8" and self._lower_sibling_group(node):
            return
        if mode == "avg" and (sh, sw) == (1, 1) and self._commute_avgpool(node, x, (kh, kw), (pt, pb, pl, pr)):
            return
        if x.qscale is not None and C % 16 == 0:
            # pooled values stay within the input range: keep the input scale, requantise
            # only when written into a concat buffer of another scale
            out = self._new((N, Ho, Wo, C), torch.uint8)
            out.qscale = x.qscale

            def run8(x=x, out=out):
                F8.pool2d_nhwc_fp8(_view(x), (kh, kw), (sh, sw), (pt, pb, pl, pr), mode,
                                   rq=x.qscale / _eff_scale(out), out=_target(out), out_channel_offset=_coff(out))

            self._emit(node.name, "pool_fp8", run8, [x], [out])
            self.vals[(node.name, 0)] = out
            return
        out = self._new((N, Ho, Wo, C))
        xin = self._as_bf16(x, node.name)

        def run(xin=xin, out=out):
            K.pool2d_nhwc(xin.buf, (kh, kw), (sh, sw), (pt, pb, pl, pr), mode, out=_target(out),
                          out_channel_offset=_coff(out))

        self._emit(node.name, "pool", run, [xin], [out])
        self.vals[(node.name, 0)] = out

    def _lower_mean(self, node: Node) -> bool:
        x = self._in(node, 0)
        av = self._get(node.inputs[1])
        if av is None or not av.is_const or len(x.shape) != 4:
            return False
        axes = sorted(int(a) % 4 for a in av.const.reshape(-1).tolist())
        if axes != [1, 2] or x.shape[-1] % 8:
            return False
        keep = node.attr("keep_dims", False)
        N, H, W, C = x.shape
        out = self._new((N, 1, 1, C) if keep else (N, C))
        if x.qscale is not None and C % 16 == 0:
            def run8(x=x, out=out):
                F8.global_avgpool_fp8(_view(x), _eff_scale(x), out=out.buf.view(N, C))

            self._emit(node.name, "gap_fp8", run8, [x], [out])
            self.vals[(node.name, 0)] = out
            return True
        xin = self._as_bf16(x, node.name)

        def run(xin=xin, out=out):
            K.global_avgpool(xin.buf, out=out.buf.view(N, C))

        self._emit(node.name, "gap", run, [xin], [out])
        self.vals[(node.name, 0)] = out
        return True

    def _lower_softmax(self, node: Node):
        x = self._in(node, 0)
        if len(x.shape) != 2:
            return self._lower_glue(node)
        R, C = x.shape
        xin = self._as_bf16(x, node.name)
        topk = None
        for c in self.cons.get(node.name, []):
            cn = self.graph[c]
            if cn.op == "TopKV2":
                kv = self._get(cn.inputs[1])
                if kv is not None and kv.is_const:
                    topk = (cn, int(kv.const.item()))
        probs = self._new((R, C))
        k = topk[1] if topk else 1
        vals = self._new((R, k), torch.float32)
        idxs = self._new((R, k), torch.int32)

        def run(xin=xin, probs=probs, vals=vals, idxs=idxs):
            K.softmax_topk(_view(xin), k, want_probs=True, vals=vals.buf, idxs=idxs.buf, probs=probs.buf)

        self._emit(node.name, "softmax_topk", run, [xin], [probs, vals, idxs])
        self.vals[(node.name, 0)] = probs
        if topk is not None:
            self._fused.add(topk[0].name)
            self.vals[(topk[0].name, 0)] = vals
            self.vals[(topk[0].name, 1)] = idxs

    def _lower_reshape(self, node: Node):
        x = self._in(node, 0)
        sv = self._get(node.inputs[1])
        if sv is None or not sv.is_const or (x.phys_c and (x.is_const or x.rows is not None or x.buf_shape)):
            return self._lower_glue(node)
        shape = [int(v) for v in sv.const.reshape(-1).tolist()]
        if x.rows is not None:
            return self._reshape_rows(node, x, shape)
        if x.phys_c:
            # a channel-padded conv output (an SSD head of 3 x 4 = 12 or 3 x 91 = 273 channels):
            # compact the logical columns first, as the StridedSlice copy does, then alias
            packed = self._new(x.shape, x.dtype)
            packed.qscale = x.qscale

            def run(x=x, packed=packed):
                packed.buf.copy_(_view(x))

            self._emit(node.name, "copy", run, [x], [packed])
            x = packed
        n = int(np.prod(x.shape))
        if -1 in shape:
            i = shape.index(-1)
            rest = int(np.prod([s for j, s in enumerate(shape) if j != i]))
            shape[i] = n // max(rest, 1)
        out = Val(tuple(shape), x.dtype, alias_of=x)
        self.vals[(node.name, 0)] = out

    def _lower_concat(self, node: Node):
        ins = [self._in(node, i) for i in range(len(node.inputs) - 1)]
        av = self._get(node.inputs[-1])
        if av is None or not av.is_const:
            return self._lower_glue(node)
        axis = int(av.const.item()) % len(ins[0].shape)
        shape = list(ins[0].shape)
        shape[axis] = sum(v.shape[axis] for v in ins)
        fp8 = all(v.qscale is not None for v in ins) and self._qscale(node.name) is not None
        out = self._new(tuple(shape), torch.uint8 if fp8 else torch.bfloat16)
        if fp8:
            out.qscale = self._qscale(node.name)
        # one storage format per buffer: all fp8 at the concat's scale, or all bf16 (an fp8
        # plan's resize or depthwise branch next to fp8 convs is joined by the bf16 copy below)
        stride_write = (axis == len(shape) - 1 and len(shape) in (4, 5)
                        and (fp8 or not any(v.qscale is not None for v in ins))
                        and all(self._concat_writable(v, node.inputs[i][0], node.name) for i, v in enumerate(ins)))
        if stride_write:
            off = 0
            for v in ins:
                v.concat_slot = (out, off)
                off += v.shape[-1]
            self.vals[(node.name, 0)] = out
            out.concat_children = ins
            return
        if fp8 or any(v.qscale is not None for v in ins):  # mixed scales: concatenate in bf16
            out = self._new(tuple(shape))
            ins = [self._as_bf16(v, f"{node.name}/in{i}") for i, v in enumerate(ins)]

        def run(ins=ins, out=out, axis=axis):
            torch.cat([_view(v) for v in ins], dim=axis, out=out.buf)

        self._emit(node.name, "concat", run, ins, [out])
        self.vals[(node.name, 0)] = out

    def _concat_writable(self, v: Val, src_node: str, concat_node: str) -> bool:
        # produced by exactly one conv/pool/resize/deconv/conv3d/pool3d/instnorm/pad step (which can write at a channel offset),
        # consumed by nothing but this concat, and not fetched
        prods = [s for s in self.steps if any(o is v for o in s.outputs)]
        if len(prods) != 1 or prods[0].kind not in ("conv", "pool", "conv_fp8", "pool_fp8", "resize", "deconv",
                                                        "conv3d", "pool3d", "instnorm", "pad") \
                or v.concat_slot is not None \
                or (len(prods[0].outputs) != 1 and not prods[0].meta.get("multi_out")):
            return False
        if v.alias_of is not None or v.phys_c:
            return False
        # every graph node that maps to this value must feed only the concat
        # (a fused reader is a member of the producer's own chain, except the members of a matched norm
        # group: those read the value as the group's input, and its kernel reads a buffer of its own)
        readers = self._readers(v)
        if readers is None or any(c != concat_node and (c not in self._fused or self._norm_group_reads(c, v))
                                  for c in readers):
            return False
        if v.qscale is not None:
            return v.shape[-1] % 16 == 0 and src_node in self.cons
        return v.shape[-1] % 8 == 0 and v.dtype == torch.bfloat16 and src_node in self.cons

    def _norm_group_reads(self, name: str, v: Val) -> bool:
        """Graph node ``name`` belongs to a matched ``ln`` group whose input is the value ``v``."""
        grp = self._groups.get(name)
        return grp is not None and grp["kind"] == "ln" and self.vals.get(grp["x"]) is v

    def _lower_glue(self, node: Node, host_consts=()):
        """``node`` as a captured interpreter op.  ``host_consts``: the inputs whose constants stay on
        the host (a shape operand the op reads into Python ints, which a capture does not allow of a
        device tensor)."""
        if any(self.vals.get(s) is not None and self.vals[s].rows is not None for s in node.inputs):
            raise CompileError(f"{node.op} {node.name} reads token-packed rows; no packed lowering")
        if self.strict:
            raise CompileError(f"op {node.op} ({node.name}) has no CDNA4 lowering (strict mode)")
        self.glue_ops.append(node.op)
        LOG.info("glue op %s (%s) runs as a captured PyTorch op", node.op, node.name)
        ins = [self.vals.get((s, k)) for s, k in node.inputs]
        if any(v is None for v in ins):
            raise CompileError(f"inputs of {node.name} not available")
        fn = lookup(node.op)
        # infer output shapes with a meta/CPU dry run on zeros
        ctx = OpContext(self._const_sess, torch.device("cpu"))
        probe = [v.const if v.is_const else torch.zeros(v.shape, dtype=torch.float32 if v.dtype == torch.bfloat16
                                                          else v.dtype) for v in ins]
        outs = fn(ctx, node, *probe)
        outv = [self._new(o.shape, torch.bfloat16 if o.dtype == torch.float32 else o.dtype) for o in outs]
        dev_consts = [None if not v.is_const else
                      (v.const.to(self.device) if isinstance(v.const, torch.Tensor) and i not in host_consts else v.const)
                      for i, v in enumerate(ins)]
        dctx = OpContext(self._const_sess, self.device)

        def run(node=node, ins=ins, outv=outv, dev_consts=dev_consts):
            args = []
            for v, dc in zip(ins, dev_consts):
                if dc is not None:
                    args.append(dc)
                else:
                    b = _view(v)
                    args.append(b.float() if b.dtype == torch.bfloat16 else b)
            res = fn(dctx, node, *args)
            for o, r in zip(outv, res):
                o.buf.copy_(r.reshape(o.buf.shape))

        self._emit(node.name, "glue", run, [v for v in ins if not v.is_const], outv)
        for k, o in enumerate(outv):
            self.vals[(node.name, k)] = o

    def param_bytes(self) -> int:
        return sum(p.numel() * p.element_size() for p in self.params)

    def summary(self) -> dict:
        kinds: dict[str, int] = {}
        for s in self.steps:
            kinds[s.kind] = kinds.get(s.kind, 0) + 1
        return {"steps": len(self.steps), "kinds": kinds, "glue_ops": sorted(set(self.glue_ops)),
                "hip_graph": self._graph_obj is not None, "precision": self.precision,
                "fp8_layers": self.fp8_layers,
                **self.stats,  # every counter of _STATS (a misspelt one would show up as a new key)
                "activation_bytes": self.activation_bytes,
                "param_bytes": self.param_bytes(),
                **({"token_capacity": self.token_cap, "first_token_only_nodes": len(self._cls_nodes)}
                   if self._pack is not None else {})}


def compile_signature(session, feeds: dict[str, tuple[tuple, Any]], fetches: list[str], use_graph=True,
                      strict=False, precision: str = "bf16", calibration: dict | None = None) -> CompiledFunction:
    """Compiles ``session``'s graph for the given feed shapes on the session's GPU."""
    return CompiledFunction(session.graph, feeds, fetches, session.device, session.variables, use_graph, strict,
                            precision=precision, calibration=calibration)
