"""Next-item recommender (SASRec-style causal transformer) as a frozen TF GraphDef (random-init
weights; no network access).

A record is a session: the ids of the items a user touched, oldest first.  Each event may only
see the events before it, the hidden state of the last event is the query, and its scores against
the item embedding table go through ``TopKV2`` — the session-encoded query of a retrieval stage
(``two_tower.py`` encodes a feature vector instead).  The graph, as TF exports it (node patterns
of ``bert_graph.py``):

    item_ids [B, S] int32, left-padded with 0, the most recent S events
    -> GatherV2(item_embeddings) + position rows -> layer_norm
    -> L post-LN blocks whose attention adder is (1 - NotEqual(ids, 0)[:, None, None, :] * tril) * -10000
    -> StridedSlice of the last position -> MatMul(h_last, item_embeddings, transpose_b)
    -> BiasAdd(item_bias) -> TopKV2

The compiler lowers it to ``embed_ln`` 1, per block the fused QKV ``gemm`` + one
``causal_attention`` step (``kernels/attention_causal.hip``) + 3 ``gemm`` + 2 ``layernorm``, a
``copy`` of the last position and one ``retrieve`` step, so a strict plan holds no glue and never
writes a ``[B, H, S, S]`` or ``[B, N]`` score tensor.  The output table is the input embedding
table; ``item_bias[0]`` is a large negative constant so the pad id is never recommended.  The
hidden size is one of 64, 128, 192, 256 (``retrieve``'s ``D <= 256``) and equals ``head_dim * heads``
with 32-, 64- (the default) or 128-wide heads: SASRec / BERT4Rec sizes such as hidden 64 with 2 heads.

``NextItemConfig.window = W`` makes the attention local: the mask constant is the band ``i - W < j
<= i`` of the tril, each block's attention lowers to one ``window_attention`` step
(``kernels/attention_window.hip``) whose cost grows with ``S * W`` instead of ``S * S``, and the
history may be up to 8192 events long (2048 without a window).  ``W >= seq_len`` is the causal model.

``NextItemModel(pack_tokens=True)`` serves the same graph padding-free (``graph/packed.py`` with
``pack_causal=True``): ``pack_tokens`` + ``packed_rows`` + ``embed_ln`` at each event's own position,
every block on the real events only (``packed_causal_attention``), and the last block after its QKV
projection on one row per session (``last_attention``, then projections and LayerNorms on B rows).
With a window, ``packed_rows`` writes the windowed starts and ``last_attention`` reads the last W events.

Tensor names: ``item_ids`` (int32 [N, S]), ``scores``, ``top_k`` (``top_k:0`` scores, ``top_k:1``
item ids).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import numpy as np
import torch

from ...graph.builder import GraphBuilder
from ...graph.compiler import CompiledFunction
from ...proto.messages import GraphDef
from ...runtime.model_functions import BatchedGpuModel
from ...types.dtypes import DataType
from ..core import GenericModel, GraphDefGraphLoader, GraphLoader
from .bert_graph import _c, encoder_layers, layer_norm

PAD_BIAS = -1e4  # item_bias[0]: the pad id never reaches the top k


@dataclass
class NextItemConfig:
    num_items: int = 50_000  # ids 1 .. num_items - 1; 0 is padding
    hidden: int = 128
    heads: int = 2
    layers: int = 2
    intermediate: int = 512
    eps: float = 1e-12
    head_dim: int = 64       # 32, 64 or 128: the widths the attention kernels are built for
    window: int | None = None  # W: each event sees its last W events only (itself included); None: all before it

    def __post_init__(self):
        if self.window is not None and self.window < 1:
            raise ValueError("NextItemConfig: window must be >= 1")
        if self.head_dim not in (32, 64, 128):
            raise ValueError("NextItemConfig: head_dim must be 32, 64 or 128")
        if self.hidden not in (64, 128, 192, 256) or self.hidden != self.head_dim * self.heads:
            raise ValueError(f"NextItemConfig: hidden must be {self.head_dim} * heads, one of 64, 128, 192, 256")


def init_next_item_weights(cfg: NextItemConfig, seq_len: int, seed: int = 0) -> dict[str, torch.Tensor]:
    """Random-init fp32 host weights, named like the graph's variables."""
    g = torch.Generator().manual_seed(seed)
    H, I = cfg.hidden, cfg.intermediate

    def n(*shape):
        return torch.randn(*shape, generator=g) * 0.05

    w = {"next_item/embeddings/item_embeddings": n(cfg.num_items, H),
         "next_item/embeddings/position_embeddings": n(seq_len, H),
         "next_item/embeddings/LayerNorm/gamma": 1 + n(H), "next_item/embeddings/LayerNorm/beta": n(H),
         "next_item/item_bias": n(cfg.num_items)}
    w["next_item/item_bias"][0] = PAD_BIAS
    for l in range(cfg.layers):
        p = f"next_item/encoder/layer_{l}/"
        for nm, (i, o) in {"attention/self/query": (H, H), "attention/self/key": (H, H), "attention/self/value": (H, H),
                           "attention/output/dense": (H, H), "intermediate/dense": (H, I),
                           "output/dense": (I, H)}.items():
            w[p + nm + "/kernel"], w[p + nm + "/bias"] = n(i, o), n(o)
        for nm in ("attention/output/LayerNorm", "output/LayerNorm"):
            w[p + nm + "/gamma"], w[p + nm + "/beta"] = 1 + n(H), n(H)
    return w


def next_item_graph_def(cfg: NextItemConfig | None = None, seq_len: int = 64, k: int = 10, seed: int = 0,
                        weights: dict | None = None, causal_const: np.ndarray | None = None,
                        query_pos: int | None = None, band_part: bool = False) -> GraphDef:
    """The frozen graph on ``[B, seq_len]`` ids (B dynamic) with ``k`` recommendations per record.
    ``weights`` replaces ``init_next_item_weights(cfg, seq_len, seed)``; ``causal_const`` replaces
    the ``[1, 1, S, S]`` lower-triangular ones constant of the attention mask (with ``cfg.window``:
    its band), ``query_pos`` the position ``S - 1`` whose hidden state is the query; ``band_part``
    writes that constant as a ``MatrixBandPart`` node over ones instead."""
    cfg = cfg or NextItemConfig()
    w = weights if weights is not None else init_next_item_weights(cfg, seq_len, seed)
    S, H = seq_len, cfg.hidden
    b = GraphBuilder()

    def W(name):
        return b.constant(name, w[name].float().numpy())

    ids = b.placeholder("item_ids", "INT32", [None, S])
    mask = b.op("NotEqual", [ids, _c(b, "next_item/NotEqual/y", np.int32(0))], name="next_item/NotEqual",
                T=DataType.INT32, incompatible_shape_error=True)
    items = W("next_item/embeddings/item_embeddings")
    emb = b.op("GatherV2", [items, ids, _c(b, "next_item/embeddings/GatherV2/axis", np.int32(0))],
               name="next_item/embeddings/GatherV2", Tparams=DataType.FLOAT, Tindices=DataType.INT32,
               Taxis=DataType.INT32, batch_dims=0)
    pos = b.reshape(W("next_item/embeddings/position_embeddings"), [1, S, H], name="next_item/embeddings/Reshape")
    x = b.add(emb, pos, name="next_item/embeddings/add")
    x = layer_norm(b, x, W("next_item/embeddings/LayerNorm/gamma"), W("next_item/embeddings/LayerNorm/beta"), cfg.eps,
                   "next_item/embeddings/LayerNorm")
    # ---- attention mask [B, 1, S, S] = key mask [B, 1, 1, S] * tril [1, 1, S, S], then the adder
    mf = b.cast(mask, "FLOAT", name="next_item/encoder/Cast")
    m4 = b.op("ExpandDims", [b.op("ExpandDims", [mf, _c(b, "next_item/encoder/ExpandDims/dim", np.int32(1))],
                                  name="next_item/encoder/ExpandDims", T=DataType.FLOAT, Tdim=DataType.INT32),
                             _c(b, "next_item/encoder/ExpandDims_1/dim", np.int32(1))],
              name="next_item/encoder/ExpandDims_1", T=DataType.FLOAT, Tdim=DataType.INT32)
    tril = np.tril(np.ones((S, S), np.float32))
    if cfg.window is not None:  # the band i - W < j <= i; W >= S leaves the tril
        tril = np.triu(tril, -(cfg.window - 1))
    tril = tril[None, None] if causal_const is None else causal_const
    if band_part:  # the mask as tf.linalg.band_part(ones, W - 1, 0) leaves it in a frozen graph (-1: the tril)
        lower = -1 if cfg.window is None else cfg.window - 1
        cm = b.op("MatrixBandPart", [_c(b, "next_item/encoder/ones", np.ones((1, 1, S, S), np.float32)),
                                     _c(b, "next_item/encoder/band_part/num_lower", np.int64(lower)),
                                     _c(b, "next_item/encoder/band_part/num_upper", np.int64(0))],
                  name="next_item/encoder/causal_mask", T=DataType.FLOAT, Tindex=DataType.INT64)
    else:
        cm = _c(b, "next_item/encoder/causal_mask", np.asarray(tril, np.float32))
    m4 = b.mul(m4, cm, name="next_item/encoder/mul")
    one_minus = b.sub(_c(b, "next_item/encoder/sub/x", np.float32(1.0)), m4, name="next_item/encoder/sub")
    adder = b.mul(one_minus, _c(b, "next_item/encoder/mul_1/y", np.float32(-10000.0)), name="next_item/encoder/mul_1")
    x2 = b.reshape(x, [-1, H], name="next_item/encoder/Reshape")
    x2 = encoder_layers(b, W, x2, adder, S, H, cfg.heads, cfg.layers, cfg.eps, scope="next_item/encoder/")
    seq = b.reshape(x2, [-1, S, H], name="next_item/encoder/Reshape_out")
    qp = S - 1 if query_pos is None else query_pos
    last = b.op("StridedSlice", [seq, _c(b, "next_item/last/stack", np.asarray([0, qp, 0], np.int32)),
                                 _c(b, "next_item/last/stack_1", np.asarray([0, qp + 1, 0], np.int32)),
                                 _c(b, "next_item/last/stack_2", np.asarray([1, 1, 1], np.int32))],
                name="next_item/last", T=DataType.FLOAT, Index=DataType.INT32, begin_mask=5, end_mask=5,
                ellipsis_mask=0, new_axis_mask=0, shrink_axis_mask=2)
    s = b.matmul(last, items, transpose_b=True, name="scores/MatMul")
    s = b.bias_add(s, W("next_item/item_bias"), name="scores")
    b.top_k(s, min(k, cfg.num_items), name="top_k")
    return b.build_graph_def()


class NextItemModel(GenericModel, BatchedGpuModel):
    """Sessions (variable-length lists of item ids, oldest first) -> the ``k`` best
    ``(score, item_id)`` pairs, best first.  The host keeps the most recent ``seq_len`` events and
    left-pads with 0.  On a GPU subtask ``open()`` compiles one strict plan per batch bucket and
    compute lane and serves them through the pipelined runner; on a host subtask the graph runs in
    the interpreter.  ``pack_tokens=True``: each bucket is a padding-free ``PackedFunction`` with
    ``PACK_CAPACITIES`` token capacities (the host counts a batch's events and picks the smallest
    that holds them)."""

    # token capacities per bucket of a packed model: evenly spaced multiples of 64 (the packed causal
    # kernel's row tile).  ``default_granule`` is BERT-sized (2048-token steps: one capacity at 32 x 64).
    # Four keeps compile time and captured graphs at 4 x the padded model's per bucket and bounds
    # the padding at a quarter of the bucket; the count is a choice, not a measured optimum.
    PACK_CAPACITIES = 4

    _TRANSIENT = ("_graph", "_session", "_plans", "_runner", "_arena")

    def __init__(self, cfg: NextItemConfig | None = None, seq_len: int = 64, top_k: int = 10,
                 buckets: Sequence[int] = (32, 256), seed: int = 0, weights: dict | None = None, device=None,
                 depth: int = 3, use_graph: bool = True, lanes: int = 2, pack_tokens: bool = False):
        super().__init__(device)
        self.cfg = cfg or NextItemConfig()
        self.seq_len, self.top_k = seq_len, top_k
        self.buckets = tuple(sorted(buckets))
        self.seed, self.weights = seed, weights
        self.depth = depth
        self.use_graph = use_graph
        self.lanes = max(1, int(lanes))
        self.pack_tokens = pack_tokens
        self.feed = "item_ids:0"
        self.fetches = ["top_k:0", "top_k:1"]
        self._plans: dict | None = None
        self._runner = None
        self._arena = None

    def graph_def(self) -> GraphDef:
        return next_item_graph_def(self.cfg, self.seq_len, self.top_k, self.seed, self.weights)

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
            lanes = [{b: self._compile(graph, b, dev, arena) for b in sorted(self.buckets, reverse=True)}
                     for arena in self._arena]
            self._plans = lanes[0]
            self._runner = PipelinedGpuRunner(lanes, self.feed, lambda p: p.output_tensors(), (self.seq_len,),
                                              torch.int32, depth=self.depth, device=dev)

    def _compile(self, graph, b: int, dev, arena):
        feeds = {self.feed: ((b, self.seq_len), "INT32")}
        if not self.pack_tokens:
            return CompiledFunction(graph, feeds, self.fetches, dev, use_graph=self.use_graph, strict=True, arena=arena)
        from ...graph.packed import PackedFunction

        full, n = b * self.seq_len, self.PACK_CAPACITIES
        caps = sorted({min(full, -(-full * i // (n * 64)) * 64) for i in range(1, n + 1)})
        return PackedFunction(graph, feeds, self.fetches, dev, use_graph=self.use_graph, strict=True, arena=arena,
                              capacities=caps, pack_causal=True)

    def close(self) -> None:
        if self._runner is not None:
            self._runner.drain()
        self._runner = None
        self._plans = None
        self._arena = None
        super().close()

    def plan_summary(self) -> dict | None:
        return next(iter(self._plans.values())).summary() if self._plans else None

    # ------------------------------------------------------------------ records
    def _as_row(self, r) -> np.ndarray:
        """The last ``seq_len`` events of a session, left-padded with 0."""
        a = np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r).reshape(-1)
        if a.size == 0:
            raise ValueError(f"{type(self).__name__}: a record with no events has no next item")
        if a.min() < 1 or a.max() >= self.cfg.num_items:
            raise ValueError(f"{type(self).__name__}: item ids must lie in [1, {self.cfg.num_items})")
        a = a[-self.seq_len:].astype(np.int32)
        row = np.zeros(self.seq_len, dtype=np.int32)
        row[self.seq_len - a.size:] = a
        return row

    @staticmethod
    def _pairs(vals, idxs) -> list:
        return [[(float(v), int(i)) for v, i in zip(vr, ir)] for vr, ir in zip(vals.tolist(), idxs.tolist())]

    def _results(self, br):
        return self._pairs(br.outputs[0][: br.n], br.outputs[1][: br.n]), br.tags, br.latencies

    # ------------------------------------------------------------------ synchronous API
    def recommend(self, sequences) -> list[list[tuple]]:
        """The ``k`` best ``(score, item_id)`` per session, best first."""
        rows = [self._as_row(r) for r in sequences]
        out = []
        cap = self.buckets[-1]
        for s in range(0, len(rows), cap):
            chunk = np.stack(rows[s:s + cap])
            n = len(chunk)
            if self._plans is not None:
                b = next(bk for bk in self.buckets if bk >= n)
                buf = np.zeros((b, self.seq_len), dtype=np.int32)  # all-pad filler rows: zero context, dropped
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

            return [(self.recommend(records), tags, time.perf_counter() - np.asarray(ingest_ts))]
        rows = [self._as_row(r) for r in records]
        out = []
        cap = self.buckets[-1]
        for s in range(0, len(rows), cap):
            for br in self._runner.submit(rows[s:s + cap], np.asarray(ingest_ts[s:s + cap]), list(tags[s:s + cap])):
                out.append(self._results(br))
        return out

    def poll(self):
        return [self._results(b) for b in self._runner.poll()] if self._runner is not None else []

    def drain(self):
        return [self._results(b) for b in self._runner.drain()] if self._runner is not None else []
