"""Two-tower retrieval model as a frozen TF GraphDef (random-init weights; no network access).

The candidate-generation stage in front of a ranker (``wide_deep.py``): a small query tower turns
a record's dense features into an embedding ``u [B, D]``, its scores against a constant item
matrix ``[N, D]`` (the item tower's output, computed offline) go through ``TopKV2`` and only the
``k`` best item indices leave the GPU.  The graph, as TF exports it:

    features [B, F] float -> (MatMul + BiasAdd + Relu) x 2 -> MatMul + BiasAdd (projection to D)
    -> MatMul(u, items, transpose_b=True) -> BiasAdd(item_bias) -> TopKV2

The compiler lowers the three tower layers to ``gemm`` steps and the tail to one ``retrieve`` step
on ``kernels/retrieve.hip`` (``graph/retrieval_lowering.py``), so a strict plan holds the fed
cast, ``gemm`` 3 and ``retrieve`` 1 and never writes the ``[B, N]`` score matrix.  The tower takes
dense features only: embedding lookups (``GatherV2``) have no general lowering.

Tensor names: ``features`` (float [N, F]), ``user_embedding``, ``scores``, ``top_k`` (``top_k:0``
scores, ``top_k:1`` item indices).
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


def two_tower_graph_def(features: int = 64, hidden: Sequence[int] = (256, 128), dim: int = 64, num_items: int = 100_000,
                        top_k: int = 10, seed: int = 0, weights: dict | None = None) -> GraphDef:
    """``hidden`` are the widths of the two ReLU layers.  ``weights`` replaces the random
    initialisation: ``{"w0", "b0", "w1", "b1", "w2", "b2", "items" [N, D], "item_bias" [N]}``."""
    if len(hidden) != 2:
        raise ValueError("two_tower_graph_def: the query tower has two hidden layers")
    rng = np.random.default_rng(seed)
    widths = [features, *hidden, dim]
    w = dict(weights or {})
    for i in range(3):
        lim = float(np.sqrt(6.0 / (widths[i] + widths[i + 1])))
        w.setdefault(f"w{i}", rng.uniform(-lim, lim, (widths[i], widths[i + 1])))
        w.setdefault(f"b{i}", rng.uniform(-0.1, 0.1, (widths[i + 1],)))
    w.setdefault("items", rng.standard_normal((num_items, dim)) / np.sqrt(dim))
    w.setdefault("item_bias", rng.uniform(-0.5, 0.5, (num_items,)))  # e.g. the log popularity of an item
    w = {n: np.asarray(v, dtype=np.float32) for n, v in w.items()}
    gb = GraphBuilder()
    x = gb.placeholder("features", "FLOAT", [-1, features])
    for i in range(3):
        with gb.name_scope(f"query_tower/dense_{i}"):
            x = gb.bias_add(gb.matmul(x, gb.constant("kernel", w[f"w{i}"]), name="MatMul"),
                            gb.constant("bias", w[f"b{i}"]), name="BiasAdd")
            if i < 2:
                x = gb.relu(x, name="Relu")
    u = gb.op("Identity", [x], name="user_embedding")
    s = gb.matmul(u, gb.constant("items", w["items"]), transpose_b=True, name="scores/MatMul")
    s = gb.bias_add(s, gb.constant("item_bias", w["item_bias"]), name="scores")
    gb.top_k(s, min(top_k, w["items"].shape[0]), name="top_k")
    return gb.build_graph_def()


class RetrievalModel(GenericModel, BatchedGpuModel):
    """Feature records ``(F,)`` float32 -> the ``k`` best ``(score, item_id)`` pairs, best first.
    ``item_ids`` is an optional host-side table that maps an item's row to its id.  On a GPU
    subtask ``open()`` compiles one strict plan per batch bucket and compute lane and serves them
    through the pipelined runner; on a host subtask the graph runs in the interpreter."""

    _TRANSIENT = ("_graph", "_session", "_plans", "_runner", "_arena")

    def __init__(self, features: int = 64, hidden: Sequence[int] = (256, 128), dim: int = 64, num_items: int = 100_000,
                 top_k: int = 10, buckets: Sequence[int] = (32, 256), item_ids: Sequence | None = None, seed: int = 0,
                 weights: dict | None = None, device=None, depth: int = 3, use_graph: bool = True, lanes: int = 2):
        super().__init__(device)
        self.features, self.hidden, self.dim, self.num_items = features, tuple(hidden), dim, num_items
        self.top_k = top_k
        self.buckets = tuple(sorted(buckets))
        self.item_ids = list(item_ids) if item_ids is not None else None
        self.seed, self.weights = seed, weights
        self.depth = depth
        self.use_graph = use_graph
        self.lanes = max(1, int(lanes))
        self.feed = "features:0"
        self.fetches = ["top_k:0", "top_k:1"]
        self._plans: dict | None = None
        self._runner = None
        self._arena = None

    def graph_def(self) -> GraphDef:
        return two_tower_graph_def(self.features, self.hidden, self.dim, self.num_items, self.top_k, self.seed,
                                   self.weights)

    @property
    def graph_loader(self) -> GraphLoader:
        return GraphDefGraphLoader(self.graph_def())

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
            graph = self._session.graph
            lanes = [{b: CompiledFunction(graph, {self.feed: ((b, self.features), "FLOAT")}, self.fetches, dev,
                                          use_graph=self.use_graph, strict=True, arena=arena)
                      for b in sorted(self.buckets, reverse=True)} for arena in self._arena]
            self._plans = lanes[0]
            self._runner = PipelinedGpuRunner(lanes, self.feed, lambda p: p.output_tensors(), (self.features,),
                                              torch.float32, depth=self.depth, device=dev)

    def close(self) -> None:
        if self._runner is not None:
            self._runner.drain()
        self._runner = None
        self._plans = None
        self._arena = None
        super().close()

    def plan_summary(self) -> dict | None:
        return next(iter(self._plans.values())).summary() if self._plans else None

    def item_id(self, i: int):
        return self.item_ids[i] if self.item_ids is not None else i

    # ------------------------------------------------------------------ records
    def _as_array(self, r) -> np.ndarray:
        if isinstance(r, TensorValue):
            r = r.to_numpy()
        elif isinstance(r, torch.Tensor):
            r = r.cpu().numpy()
        a = np.ascontiguousarray(np.asarray(r), dtype=np.float32)
        if a.shape != (self.features,):
            raise ValueError(f"{type(self).__name__}: record {a.shape} is not ({self.features},)")
        return a

    def _pairs(self, vals, idxs) -> list:
        return [[(float(v), self.item_id(int(i))) for v, i in zip(vr, ir)] for vr, ir in zip(vals.tolist(), idxs.tolist())]

    def _results(self, br):
        return self._pairs(br.outputs[0][: br.n], br.outputs[1][: br.n]), br.tags, br.latencies

    # ------------------------------------------------------------------ synchronous API
    def retrieve(self, features) -> list[list[tuple]]:
        """The ``k`` best ``(score, item_id)`` per record, best first."""
        arrs = [self._as_array(r) for r in features]
        out = []
        cap = self.buckets[-1]
        for s in range(0, len(arrs), cap):
            chunk = np.stack(arrs[s:s + cap])
            n = len(chunk)
            if self._plans is not None:
                b = next(bk for bk in self.buckets if bk >= n)
                buf = np.zeros((b, self.features), dtype=np.float32)
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

            return [(self.retrieve(records), tags, time.perf_counter() - np.asarray(ingest_ts))]
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


def export_two_tower_saved_model(export_dir: str, **graph_args) -> str:
    """The two-tower model as a TF 1.x SavedModel with its weights as variables (signature
    ``serving_default``: ``features`` -> ``scores``, ``items``); ``graph_args`` are those of
    ``two_tower_graph_def``."""
    from ...proto.messages import SignatureDef
    from ..export import graph_def_to_saved_model, tensor_info

    gd = two_tower_graph_def(**graph_args)
    items = (graph_args.get("weights") or {}).get("items")
    k = min(graph_args.get("top_k", 10), graph_args.get("num_items", 100_000) if items is None else len(items))
    sig = SignatureDef(inputs={"features": tensor_info("features:0", "FLOAT", [-1, graph_args.get("features", 64)])},
                       outputs={"scores": tensor_info("top_k:0", "FLOAT", [-1, k]),
                                "items": tensor_info("top_k:1", "INT32", [-1, k])},
                       method_name="tensorflow/serving/predict")
    return graph_def_to_saved_model(export_dir, gd, {"serving_default": sig})
