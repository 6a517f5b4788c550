"""LSTM sequence classifier as a frozen TF GraphDef (random-init weights; no network access).

The model that runs over event streams: a window of ``seq_len`` feature vectors per record
(sensor readings, click features, embedded log lines) goes through ``layers`` stacked LSTM
layers and the last hidden state is classified.  The graph is the one TF exports for
``LSTMBlockFusedCell`` behind a batch-major input:

    sequences [B, T, I] float -> Transpose([1, 0, 2]) -> BlockLSTM x layers (zero initial state)
    -> h[T - 1] (StridedSlice) -> MatMul + BiasAdd -> Softmax -> TopKV2

The compiler lowers every ``BlockLSTM`` to one projection GEMM plus one ``lstm`` step on
``kernels/lstm.hip`` and absorbs the transpose and the last-step slice, so a strict plan holds
the fed cast, ``gemm`` + ``lstm`` per layer, the head GEMM and the softmax / top-k step
(``graph/recurrent_lowering.py``).

Tensor names: ``sequences`` (float [N, T, I]), ``logits``, ``probs``, ``top_k`` (``top_k:0``
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


def lstm_classifier_graph_def(seq_len: int = 128, features: int = 64, hidden: int = 128, layers: int = 2,
                              num_classes: int = 10, batch: int | None = None, top_k: int = 3, seed: int = 0,
                              forget_bias: float = 1.0, cell_clip: float = 3.0) -> GraphDef:
    """``batch`` fixes the batch size of the zero initial-state constants (TF bakes the
    ``zero_state`` of a fixed-batch export the same way); one graph per bucket."""
    if batch is None or batch < 1:
        raise ValueError("lstm_classifier_graph_def: the zero initial state needs the batch size")
    rng = np.random.default_rng(seed)
    gb = GraphBuilder()
    x = gb.placeholder("sequences", "FLOAT", [batch, seq_len, features])
    x = gb.transpose(x, [1, 0, 2], name="time_major")
    zeros = gb.constant("zero_state", np.zeros((batch, hidden), dtype=np.float32))
    cin = features
    for layer in range(layers):
        with gb.name_scope(f"lstm_{layer}"):
            # Glorot-uniform kernel over [x, h] -> 4H, zero bias (the forget bias is the attr)
            lim = float(np.sqrt(6.0 / (cin + hidden + 4 * hidden)))
            w = gb.constant("kernel", rng.uniform(-lim, lim, (cin + hidden, 4 * hidden)).astype(np.float32))
            b = gb.constant("bias", np.zeros((4 * hidden,), dtype=np.float32))
            cell = gb.block_lstm(x, w, b, zeros, zeros, seq_len, hidden, forget_bias=forget_bias, cell_clip=cell_clip,
                                 name="BlockLSTM")
        x = f"{cell}:6"
        cin = hidden
    last = gb.strided_slice(x, [-1], [0], name="last_step", end_mask=1, shrink_axis_mask=1)
    lim = float(np.sqrt(6.0 / (hidden + num_classes)))
    wo = gb.constant("dense/kernel", rng.uniform(-lim, lim, (hidden, num_classes)).astype(np.float32))
    bo = gb.constant("dense/bias", rng.uniform(-0.1, 0.1, (num_classes,)).astype(np.float32))
    logits = gb.bias_add(gb.matmul(last, wo, name="dense/MatMul"), bo, name="logits")
    probs = gb.softmax(logits, name="probs")
    gb.top_k(probs, min(top_k, num_classes), name="top_k")
    return gb.build_graph_def()


class LSTMClassifierModel(GenericModel, BatchedGpuModel):
    """Sequence records ``(T, I)`` float32 -> top-k ``(probability, label)`` pairs.  On a GPU
    subtask ``open()`` compiles one strict plan per batch bucket and compute lane and serves them
    through the pipelined runner; on a host subtask the graph runs in the interpreter."""

    _TRANSIENT = ("_graph", "_session", "_plans", "_runner", "_arena", "_graphs")

    def __init__(self, seq_len: int = 128, features: int = 64, hidden: int = 128, layers: int = 2,
                 num_classes: int = 10, buckets: Sequence[int] = (64, 256), top_k: int = 3,
                 labels: Sequence[str] | None = None, seed: int = 0, device=None, depth: int = 3,
                 use_graph: bool = True, lanes: int = 2, cell_clip: float = 3.0):
        super().__init__(device)
        self.seq_len, self.features, self.hidden, self.layers = seq_len, features, hidden, layers
        self.num_classes = num_classes
        self.buckets = tuple(sorted(buckets))
        self.top_k = min(top_k, num_classes)
        self.labels = list(labels) if labels is not None else None
        self.seed = seed
        self.depth = depth
        self.use_graph = use_graph
        self.lanes = max(1, int(lanes))
        self.cell_clip = cell_clip
        self.feed = "sequences:0"
        self.fetches = ["top_k:0", "top_k:1"]
        self._plans: dict | None = None
        self._runner = None
        self._arena = None
        self._graphs: dict = {}

    def graph_def(self, batch: int) -> GraphDef:
        return lstm_classifier_graph_def(self.seq_len, self.features, self.hidden, self.layers, self.num_classes,
                                         batch=batch, top_k=self.top_k, seed=self.seed, cell_clip=self.cell_clip)

    @property
    def graph_loader(self) -> GraphLoader:
        return GraphDefGraphLoader(self.graph_def(self.buckets[0]))

    def _graph_for(self, batch: int):
        """The graph with ``batch``-row initial states (the weights are the same for every batch)."""
        g = self._graphs.get(batch)
        if g is None:
            g = self._graphs[batch] = GraphDefGraphLoader(self.graph_def(batch)).load()
        return g

    # ------------------------------------------------------------------ lifecycle
    def open(self) -> None:
        super().open()
        self._graphs = {}
        dev = self._session.device
        if dev.type == "cuda":
            from ...batching.arena import DeviceArena
            from ...batching.engine import PipelinedGpuRunner
            from ...config import EngineConfig

            budget = EngineConfig().arena_bytes(dev) // self.lanes
            self._arena = [DeviceArena(dev, budget, name=f"{type(self).__name__}/lane{i}") for i in range(self.lanes)]
            shape = (self.seq_len, self.features)
            lanes = [{b: CompiledFunction(self._graph_for(b), {self.feed: ((b, *shape), "FLOAT")}, self.fetches, dev,
                                          use_graph=self.use_graph, strict=True, arena=arena)
                      for b in sorted(self.buckets, reverse=True)} for arena in self._arena]
            self._plans = lanes[0]
            self._runner = PipelinedGpuRunner(lanes, self.feed, lambda p: p.output_tensors(), shape, torch.float32,
                                              depth=self.depth, device=dev)

    def close(self) -> None:
        if self._runner is not None:
            self._runner.drain()
        self._runner = None
        self._plans = None
        self._arena = None
        self._graphs = {}
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
        a = np.ascontiguousarray(np.asarray(r), dtype=np.float32)
        if a.shape != (self.seq_len, self.features):
            raise ValueError(f"{type(self).__name__}: record {a.shape} is not ({self.seq_len}, {self.features})")
        return a

    def _pairs(self, vals, idxs) -> list:
        return [[(float(v), self.label_of(int(i))) for v, i in zip(vr, ir)] for vr, ir in zip(vals.tolist(), idxs.tolist())]

    def _results(self, br):
        return self._pairs(br.outputs[0][: br.n], br.outputs[1][: br.n]), br.tags, br.latencies

    # ------------------------------------------------------------------ synchronous API
    def classify(self, sequences) -> list[list[tuple[float, str]]]:
        """Top-k ``(probability, label)`` per sequence, best first."""
        arrs = [self._as_array(r) for r in sequences]
        out = []
        cap = self.buckets[-1]
        for s in range(0, len(arrs), cap):
            chunk = np.stack(arrs[s:s + cap])
            n = len(chunk)
            if self._plans is not None:
                b = next(bk for bk in self.buckets if bk >= n)
                buf = np.zeros((b, self.seq_len, self.features), dtype=np.float32)
                buf[:n] = chunk
                vals, idxs = self._plans[b]({self.feed: torch.from_numpy(buf).to(self.session().device)})
                out += self._pairs(vals[:n].cpu(), idxs[:n].cpu())
            else:  # the interpreter: the initial-state constants fix the batch, so one graph per size
                from ...graph.session import Session

                sess = Session(self._graph_for(n), device=self.session().device)
                try:
                    vals, idxs = sess.run(self.fetches, {self.feed: torch.from_numpy(chunk)})
                finally:
                    sess.close()
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


def export_lstm_classifier_saved_model(export_dir: str, batch: int, seq_len: int = 128, features: int = 64,
                                       hidden: int = 128, layers: int = 2, num_classes: int = 10, top_k: int = 3,
                                       seed: int = 0) -> str:
    """The classifier as a TF 1.x SavedModel with its weights as variables (signature
    ``serving_default``: ``sequences`` -> ``probabilities``, ``scores``, ``classes``) for batches
    of exactly ``batch`` sequences."""
    from ...proto.messages import SignatureDef
    from ..export import graph_def_to_saved_model, tensor_info

    top_k = min(top_k, num_classes)
    gd = lstm_classifier_graph_def(seq_len, features, hidden, layers, num_classes, batch=batch, top_k=top_k, seed=seed)
    sig = SignatureDef(inputs={"sequences": tensor_info("sequences:0", "FLOAT", [batch, seq_len, features])},
                       outputs={"probabilities": tensor_info("probs:0", "FLOAT", [batch, num_classes]),
                                "scores": tensor_info("top_k:0", "FLOAT", [batch, top_k]),
                                "classes": tensor_info("top_k:1", "INT32", [batch, top_k])},
                       method_name="tensorflow/serving/predict")
    return graph_def_to_saved_model(export_dir, gd, {"serving_default": sig})
