"""C3D video classifier as a frozen TF GraphDef (random-init weights; no network access): the
video family (action recognition, event detection over camera streams), whose layers are
``Conv3D`` and ``MaxPool3D``.  A sliding window of frames becomes one clip record.

The graph is the one TF exports for the classic architecture (Tran et al., 2015):

    clips [B, T, H, W, 3] uint8 -> Cast -> Mul(1 / 255)
    -> conv1 (base)          -> MaxPool3D 1x2x2
    -> conv2 (2 base)        -> MaxPool3D 2x2x2
    -> conv3a, conv3b (4 base) -> MaxPool3D 2x2x2
    -> conv4a, conv4b (8 base) -> MaxPool3D 2x2x2
    -> conv5a, conv5b (8 base) -> MaxPool3D 2x2x2 SAME (odd extents are covered)
    -> Reshape (flatten) -> fc6, fc7 (MatMul + BiasAdd + Relu) -> logits -> Softmax -> TopKV2

with every conv a ``3x3x3`` SAME ``Conv3D + BiasAdd + Relu``.  A pool's window and stride are 1
on an axis the clip has already been reduced to one element on (short or small test clips).

The compiler lowers all of it (``graph/conv3d_lowering.py``): the ``Cast → Mul`` prefix folds
into conv1, whose ``pad_cin`` copy casts the uint8 frames; each conv chain is one ``conv3d`` step
and each pool one ``pool3d`` step on ``kernels/conv3d.hip``; the head is three GEMMs and the
softmax / top-k step.

Tensor names: ``clips`` (uint8 [N, T, H, W, 3]), ``logits``, ``probs``, ``top_k`` (``top_k:0``
values, ``top_k:1`` indices).
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from ...graph.builder import GraphBuilder
from ...graph.compiler import CompiledFunction
from ...proto.messages import GraphDef
from ...runtime.model_functions import BatchedGpuModel
from ...types.tensor_value import TensorValue
from ..core import GenericModel, GraphDefGraphLoader, GraphLoader

# (name, width multiplier of ``base``) per conv, and the pool behind it (window = stride, padding)
_C3D_LAYERS = (("conv1", 1, ((1, 2, 2), "VALID")), ("conv2", 2, ((2, 2, 2), "VALID")), ("conv3a", 4, None),
               ("conv3b", 4, ((2, 2, 2), "VALID")), ("conv4a", 8, None), ("conv4b", 8, ((2, 2, 2), "VALID")),
               ("conv5a", 8, None), ("conv5b", 8, ((2, 2, 2), "SAME")))


def c3d_layer_shapes(frames: int = 16, image_hw: tuple[int, int] = (112, 112), base: int = 64) -> list[dict]:
    """The conv and pool layers of ``c3d_graph_def`` in order: ``{"name", "kind" ("conv" | "pool"),
    "in" (D, H, W, C), "out" (D, H, W, C), "window"}``: what the probe and the tests walk."""
    ext, cin, out = (frames, *image_hw), 3, []
    for i, (name, mult, pool) in enumerate(_C3D_LAYERS):
        c = base * mult
        out.append({"name": name, "kind": "conv", "in": (*ext, cin), "out": (*ext, c), "window": (3, 3, 3)})
        cin = c
        if pool is not None:
            win = tuple(min(k, e) for k, e in zip(pool[0], ext))
            nxt = tuple(-(-e // k) if pool[1] == "SAME" else e // k for e, k in zip(ext, win))
            out.append({"name": f"pool{sum(1 for l in _C3D_LAYERS[:i + 1] if l[2])}", "kind": "pool", "in": (*ext, c),
                        "out": (*nxt, c), "window": win, "padding": pool[1]})
            ext = nxt
    return out


def c3d_graph_def(frames: int = 16, image_hw: tuple[int, int] = (112, 112), base: int = 64, num_classes: int = 101,
                  top_k: int = 5, fc: int = 4096, seed: int = 0, logits_scale: float = 4.0) -> GraphDef:
    """``base`` and ``fc`` shrink the model for tests.  ``logits_scale`` multiplies the init of
    the logits layer, as in ``unet_graph_def``: random features give nearly tied classes
    otherwise."""
    if frames < 1 or min(image_hw) < 1 or base < 1 or fc < 1 or num_classes < 1:
        raise ValueError("c3d_graph_def: frames, image_hw, base, fc and num_classes must be positive")
    rng = np.random.default_rng(seed)
    gb = GraphBuilder()
    clips = gb.placeholder("clips", "UINT8", [None, frames, image_hw[0], image_hw[1], 3])
    x = gb.cast(clips, "FLOAT", name="Cast")
    x = gb.mul(x, gb.constant("scale", np.float32(1.0 / 255.0)), name="scaled")
    for layer in c3d_layer_shapes(frames, image_hw, base):
        name = layer["name"]
        if layer["kind"] == "pool":
            x = gb.max_pool3d(x, layer["window"], layer["window"], layer["padding"], name=name)
            continue
        cin, c = layer["in"][3], layer["out"][3]
        with gb.name_scope(name):
            w = (rng.standard_normal((3, 3, 3, cin, c)) * np.sqrt(2.0 / (27 * cin))).astype(np.float32)
            y = gb.conv3d(x, gb.constant("weights", w), (1, 1, 1), "SAME", name="Conv3D")
            b = gb.constant("biases", (rng.standard_normal(c) * 0.05).astype(np.float32))
            x = gb.relu(gb.bias_add(y, b, name="BiasAdd"), name="Relu")
    d, h, w_, c = layer["out"]
    feat = d * h * w_ * c
    x = gb.reshape(x, [-1, feat], name="flatten")
    for name, n_in, n_out in (("fc6", feat, fc), ("fc7", fc, fc)):
        with gb.name_scope(name):
            w = (rng.standard_normal((n_in, n_out)) * np.sqrt(2.0 / n_in)).astype(np.float32)
            b = gb.constant("biases", (rng.standard_normal(n_out) * 0.05).astype(np.float32))
            x = gb.relu(gb.bias_add(gb.matmul(x, gb.constant("weights", w), name="MatMul"), b, name="BiasAdd"), name="Relu")
    w = (rng.standard_normal((fc, num_classes)) * np.sqrt(1.0 / fc) * logits_scale).astype(np.float32)
    bo = gb.constant("fc8/biases", (rng.standard_normal(num_classes) * 0.1).astype(np.float32))
    logits = gb.bias_add(gb.matmul(x, gb.constant("fc8/weights", w), name="fc8/MatMul"), bo, name="logits")
    probs = gb.softmax(logits, name="probs")
    gb.top_k(probs, min(top_k, num_classes), name="top_k")
    return gb.build_graph_def()


class VideoClassifierModel(GenericModel, BatchedGpuModel):
    """Clip records ``(T, H, W, 3)`` uint8 -> top-k ``(probability, label)`` pairs.  On a GPU
    subtask ``open()`` compiles one strict plan per batch bucket and compute lane and serves them
    through the pipelined runner; on a host subtask the graph runs in the interpreter.  The
    default buckets are small: a 16 x 112 x 112 clip is 600 KB."""

    _TRANSIENT = ("_graph", "_session", "_plans", "_runner", "_arena")

    def __init__(self, frames: int = 16, image_hw: tuple[int, int] = (112, 112), base: int = 64, num_classes: int = 101,
                 fc: int = 4096, buckets: Sequence[int] = (4, 16), top_k: int = 5, labels: Sequence[str] | None = None,
                 seed: int = 0, device=None, depth: int = 3, use_graph: bool = True, lanes: int = 2):
        super().__init__(device)
        self.frames, self.image_hw, self.base, self.fc = frames, tuple(image_hw), base, fc
        self.num_classes = num_classes
        self.buckets = tuple(sorted(buckets))
        self.top_k = min(top_k, num_classes)
        self.labels = list(labels) if labels is not None else None
        self.seed = seed
        self.depth = depth
        self.use_graph = use_graph
        self.lanes = max(1, int(lanes))
        self.feed = "clips:0"
        self.fetches = ["top_k:0", "top_k:1"]
        self._plans: dict | None = None
        self._runner = None
        self._arena = None

    def graph_def(self) -> GraphDef:
        return c3d_graph_def(self.frames, self.image_hw, self.base, self.num_classes, self.top_k, self.fc, self.seed)

    @property
    def graph_loader(self) -> GraphLoader:
        return GraphDefGraphLoader(self.graph_def())

    @property
    def clip_shape(self) -> tuple:
        return (self.frames, *self.image_hw, 3)

    # ------------------------------------------------------------------ lifecycle
    def open(self) -> None:
        super().open()
        dev = self._session.device
        if dev.type == "cuda":
            from ...batching.arena import DeviceArena
            from ...batching.engine import PipelinedGpuRunner
            from ...config import EngineConfig

            budget = EngineConfig().arena_bytes(dev) // self.lanes
            self._arena = [DeviceArena(dev, budget, name=f"{type(self).__name__}/lane{i}") for i in range(self.lanes)]
            shape = self.clip_shape
            lanes = [{b: CompiledFunction(self._graph, {self.feed: ((b, *shape), "UINT8")}, self.fetches, dev,
                                          use_graph=self.use_graph, strict=True, arena=arena)
                      for b in sorted(self.buckets, reverse=True)} for arena in self._arena]
            self._plans = lanes[0]
            self._runner = PipelinedGpuRunner(lanes, self.feed, lambda p: p.output_tensors(), shape, torch.uint8,
                                              depth=self.depth, device=dev)

    def close(self) -> None:
        if self._runner is not None:
            self._runner.drain()
        self._runner = None
        self._plans = None
        self._arena = None
        super().close()

    def plan_summary(self) -> dict | None:
        return next(iter(self._plans.values())).summary() if self._plans else None

    def label_of(self, i: int) -> str:
        return self.labels[i] if self.labels and i < len(self.labels) else f"class_{i}"

    # ------------------------------------------------------------------ records
    def _as_array(self, r) -> np.ndarray:
        if isinstance(r, TensorValue):
            r = r.to_numpy()
        elif isinstance(r, torch.Tensor):
            r = r.cpu().numpy()
        a = np.asarray(r)
        if a.shape != self.clip_shape or a.dtype != np.uint8:
            raise ValueError(f"{type(self).__name__}: record {a.shape} {a.dtype} is not uint8 {self.clip_shape}")
        return np.ascontiguousarray(a)

    def _pairs(self, vals, idxs) -> list:
        return [[(float(v), self.label_of(int(i))) for v, i in zip(vr, ir)] for vr, ir in zip(vals.tolist(), idxs.tolist())]

    def _results(self, br):
        return self._pairs(br.outputs[0][: br.n], br.outputs[1][: br.n]), br.tags, br.latencies

    # ------------------------------------------------------------------ synchronous API
    def classify(self, clips) -> list[list[tuple[float, str]]]:
        """Top-k ``(probability, label)`` per clip, best first."""
        arrs = [self._as_array(r) for r in clips]
        out = []
        cap = self.buckets[-1]
        for s in range(0, len(arrs), cap):
            chunk = np.stack(arrs[s:s + cap])
            n = len(chunk)
            if self._plans is not None:
                b = next(bk for bk in self.buckets if bk >= n)
                buf = np.zeros((b, *self.clip_shape), dtype=np.uint8)
                buf[:n] = chunk
                vals, idxs = self._plans[b]({self.feed: torch.from_numpy(buf).to(self.session().device)})
                out += self._pairs(vals[:n].cpu(), idxs[:n].cpu())
            else:
                vals, idxs = self.session().run(self.fetches, {self.feed: torch.from_numpy(chunk)})
                out += self._pairs(torch.as_tensor(vals), torch.as_tensor(idxs))
        return out

    # ------------------------------------------------------------------ batched GPU API
    def submit(self, records, ingest_ts, tags):
        if self._runner is None:  # host fallback: synchronous interpreter run
            import time

            return [(self.classify(records), tags, time.perf_counter() - np.asarray(ingest_ts))]
        arrs = [self._as_array(r) for r in records]
        out = []
        cap = self.buckets[-1]
        for s in range(0, len(arrs), cap):
            for br in self._runner.submit(arrs[s:s + cap], np.asarray(ingest_ts[s:s + cap]), list(tags[s:s + cap])):
                out.append(self._results(br))
        return out

    def poll(self):
        return [self._results(b) for b in self._runner.poll()] if self._runner is not None else []

    def drain(self):
        return [self._results(b) for b in self._runner.drain()] if self._runner is not None else []


def export_c3d_saved_model(export_dir: str, **graph_args) -> str:
    """C3D as a TF 1.x SavedModel with its weights as variables (signature ``serving_default``:
    ``clips`` -> ``probabilities``, ``scores``, ``classes``); ``graph_args`` are those of
    ``c3d_graph_def``."""
    from ...proto.messages import SignatureDef
    from ..export import graph_def_to_saved_model, tensor_info

    num_classes = graph_args.get("num_classes", 101)
    top_k = min(graph_args.get("top_k", 5), num_classes)
    frames = graph_args.get("frames", 16)
    ih, iw = graph_args.get("image_hw", (112, 112))
    sig = SignatureDef(inputs={"clips": tensor_info("clips:0", "UINT8", [-1, frames, ih, iw, 3])},
                       outputs={"probabilities": tensor_info("probs:0", "FLOAT", [-1, num_classes]),
                                "scores": tensor_info("top_k:0", "FLOAT", [-1, top_k]),
                                "classes": tensor_info("top_k:1", "INT32", [-1, top_k])},
                       method_name="tensorflow/serving/predict")
    return graph_def_to_saved_model(export_dir, c3d_graph_def(**graph_args), {"serving_default": sig})
