"""DLRM ranking model as a frozen TF GraphDef (random-init weights; no network access).

The ranking stage behind retrieval (``two_tower.py``): a bottom MLP turns a record's dense
features into a vector ``x [B, D]``, every categorical field looks its id up in its own embedding
table, the ``F + 1`` vectors interact by pairwise dot products and a top MLP turns ``[x, dots]``
into a click probability.  The graph, as TF exports it:

    dense [B, 16] float -> (MatMul + BiasAdd + Relu) x 3                        bottom MLP -> x [B, D]
    ids [B, F] int32 -> Unpack(axis=1) -> GatherV2(table_f, ids_f) x F          embedding lookups
    Pack([x, e_0 .. e_F-1], axis=1) -> BatchMatMul(T, T, adj_y) -> Reshape -> GatherV2(lower triangle)
    -> ConcatV2([x, tri]) -> (MatMul + BiasAdd + Relu) x 4 -> MatMul + BiasAdd (logit) -> Sigmoid

The compiler lowers the lookups and the interaction to one ``interact`` step on
``kernels/interact.hip`` (``graph/ranking_lowering.py``) and every layer to a ``gemm`` step, the
first top layer reading the interact step's padded row in place (``D + (F + 1) F / 2`` columns:
479 at the defaults).  The dense placeholder is as wide as the dense features rounded up to a
multiple of 8 (13 -> 16): the serving graph takes them zero-padded, since a plain ``MatMul``
operand of ``K % 8 != 0`` columns has no GEMM lowering; ``DLRMModel`` pads its records.

Tensor names: ``dense`` (float [N, 16]), ``ids`` (int32 [N, F]), ``logit``, ``probability`` ([N, 1]).
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from ...graph.builder import GraphBuilder
from ...graph.compiler import CompiledFunction
from ...proto.messages import GraphDef
from ...runtime.model_functions import BatchedGpuModel
from ..core import GenericModel, GraphDefGraphLoader, GraphLoader
from ..export import export_dlrm_saved_model  # noqa: F401  (the zoo exports it from here)


def dlrm_dense_width(dense_features: int) -> int:
    return -(-dense_features // 8) * 8


def dlrm_graph_def(dense_features: int = 13, vocab_sizes: Sequence[int] = (1000,) * 26, dim: int = 128,
                   bottom: Sequence[int] = (512, 256, 128), top: Sequence[int] = (1024, 1024, 512, 256, 1), seed: int = 0,
                   weights: dict | None = None) -> GraphDef:
    """``vocab_sizes`` has one entry per categorical field; ``bottom[-1]`` must be ``dim`` and
    ``top[-1]`` 1.  ``weights`` replaces the random initialisation: ``{"bw{i}", "bb{i}"}`` (bottom
    layer ``i``, ``bw0`` with ``dlrm_dense_width`` rows), ``{"tw{i}", "tb{i}"}`` (top) and
    ``{"emb{f}"}`` ``[V_f, dim]``."""
    if bottom[-1] != dim or top[-1] != 1:
        raise ValueError("dlrm_graph_def: the bottom MLP ends in dim columns and the top MLP in one")
    rng = np.random.default_rng(seed)
    F = len(vocab_sizes)
    w = dict(weights or {})
    bw = [dlrm_dense_width(dense_features), *bottom]
    tw = [dim + (F + 1) * F // 2, *top]
    for key, widths in (("b", bw), ("t", tw)):
        for i in range(len(widths) - 1):
            lim = float(np.sqrt(6.0 / (widths[i] + widths[i + 1])))
            w.setdefault(f"{key}w{i}", rng.uniform(-lim, lim, (widths[i], widths[i + 1])))
            w.setdefault(f"{key}b{i}", rng.uniform(-0.1, 0.1, (widths[i + 1],)))
    for f, V in enumerate(vocab_sizes):
        w.setdefault(f"emb{f}", rng.uniform(-1.0, 1.0, (V, dim)) / np.sqrt(dim))
    w = {n: np.asarray(v, dtype=np.float32) for n, v in w.items()}
    gb = GraphBuilder()
    x = gb.placeholder("dense", "FLOAT", [-1, bw[0]])
    ids = gb.placeholder("ids", "INT32", [-1, F])

    def mlp(x, key, n, scope, last_relu):
        for i in range(n):
            with gb.name_scope(f"{scope}/dense_{i}"):
                x = gb.bias_add(gb.matmul(x, gb.constant("kernel", w[f"{key}w{i}"]), name="MatMul"),
                                gb.constant("bias", w[f"{key}b{i}"]), name="BiasAdd")
                if i < n - 1 or last_relu:
                    x = gb.relu(x, name="Relu")
        return x

    x = mlp(x, "b", len(bottom), "bottom_mlp", True)
    cols = gb.op("Unpack", [ids], name="ids/unstack", num=F, axis=1, T=gb._dtype_of(ids)).split(":")[0]
    emb = [gb.embedding_lookup(gb.constant(f"embedding_{f}/table", w[f"emb{f}"]), f"{cols}:{f}", name=f"embedding_{f}/lookup")
           for f in range(F)]
    z = gb.dot_interaction([x, *emb], concat_with=x)
    z = mlp(z, "t", len(top), "top_mlp", False)
    gb.sigmoid(gb.identity(z, name="logit"), name="probability")
    return gb.build_graph_def()


class DLRMModel(GenericModel, BatchedGpuModel):
    """Records ``(dense float32 [dense_features], ids int32 [F])`` -> the click probability.  On a
    GPU subtask ``open()`` compiles one strict plan per batch bucket; on a host subtask the graph
    runs in the interpreter.  ``submit`` ranks its records through those plans before it returns:
    the pipelined runner stages one feed per record, this model has two, so ``poll`` and ``drain``
    have nothing left to hand out."""

    _TRANSIENT = ("_graph", "_session", "_plans", "_arena")

    def __init__(self, dense_features: int = 13, vocab_sizes: Sequence[int] = (1000,) * 26, dim: int = 128,
                 bottom: Sequence[int] = (512, 256, 128), top: Sequence[int] = (1024, 1024, 512, 256, 1),
                 buckets: Sequence[int] = (32, 256), seed: int = 0, weights: dict | None = None, device=None,
                 use_graph: bool = True, table_precision: str = "bf16"):
        super().__init__(device)
        if table_precision not in ("bf16", "fp8"):
            raise ValueError(f"table_precision must be bf16 or fp8, not {table_precision!r}")
        self.table_precision = table_precision  # "fp8": the plans keep the embedding tables as e4m3 codes + row exponents
        self.dense_features, self.vocab_sizes, self.dim = dense_features, tuple(vocab_sizes), dim
        self.bottom, self.top = tuple(bottom), tuple(top)
        self.buckets = tuple(sorted(buckets))
        self.seed, self.weights = seed, weights
        self.use_graph = use_graph
        self.fetches = ["probability:0"]
        self._plans: dict | None = None
        self._arena = None

    def graph_def(self) -> GraphDef:
        return dlrm_graph_def(self.dense_features, self.vocab_sizes, self.dim, self.bottom, self.top, self.seed, self.weights)

    @property
    def graph_loader(self) -> GraphLoader:
        return GraphDefGraphLoader(self.graph_def())

    def open(self) -> None:
        super().open()
        dev = self._session.device
        if dev.type == "cuda":
            from ...batching.arena import DeviceArena
            from ...config import EngineConfig

            self._arena = DeviceArena(dev, EngineConfig().arena_bytes(dev), name=type(self).__name__)
            W, F = dlrm_dense_width(self.dense_features), len(self.vocab_sizes)
            self._plans = {b: CompiledFunction(self._session.graph, {"dense:0": ((b, W), "FLOAT"), "ids:0": ((b, F), "INT32")},
                                               self.fetches, dev, use_graph=self.use_graph, strict=True, arena=self._arena,
                                               table_precision=self.table_precision)
                           for b in sorted(self.buckets, reverse=True)}

    def close(self) -> None:
        self._plans = None
        self._arena = None
        super().close()

    def plan_summary(self) -> dict | None:
        return next(iter(self._plans.values())).summary() if self._plans else None

    def _arrays(self, dense, ids):
        d = np.asarray([np.asarray(r, dtype=np.float32) for r in dense], dtype=np.float32)
        i = np.asarray([np.asarray(r) for r in ids], dtype=np.int32)
        F = len(self.vocab_sizes)
        if d.ndim != 2 or d.shape[1] != self.dense_features or i.shape != (len(d), F):
            raise ValueError(f"{type(self).__name__}: records {d.shape} / {i.shape} are not "
                             f"[N, {self.dense_features}] / [N, {F}]")
        return np.pad(d, ((0, 0), (0, dlrm_dense_width(self.dense_features) - self.dense_features))), i

    def rank(self, dense, ids) -> list[float]:
        """One click probability per record."""
        d, i = self._arrays(dense, ids)
        out, cap = [], self.buckets[-1]
        for s in range(0, len(d), cap):
            dc, ic = d[s:s + cap], i[s:s + cap]
            n = len(dc)
            if self._plans is not None:
                b = next(bk for bk in self.buckets if bk >= n)
                dev = self.session().device
                db, ib = np.zeros((b, d.shape[1]), dtype=np.float32), np.zeros((b, i.shape[1]), dtype=np.int32)
                db[:n], ib[:n] = dc, ic
                (p,) = self._plans[b]({"dense:0": torch.from_numpy(db).to(dev), "ids:0": torch.from_numpy(ib).to(dev)})
                out += p[:n].float().cpu().reshape(-1).tolist()
            else:
                (p,) = self.session().run(self.fetches, {"dense:0": torch.from_numpy(dc), "ids:0": torch.from_numpy(ic)})
                out += torch.as_tensor(p).float().reshape(-1).tolist()
        return out

    # ------------------------------------------------------------------ batched API
    def submit(self, records, ingest_ts, tags):
        import time

        probs = self.rank([r[0] for r in records], [r[1] for r in records])
        return [(probs, tags, time.perf_counter() - np.asarray(ingest_ts))]

    def poll(self):
        return []

    def drain(self):
        return []
