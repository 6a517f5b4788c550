"""Lowering of retrieval heads (a mixin of ``CompiledFunction``): the candidate-generation tail
of a two-tower model, ``MatMul(u, items) -> [BiasAdd | Add(item_bias)] -> TopKV2``, to one
``retrieve`` step on ``kernels/retrieve.hip``.  The ``[B, N]`` score matrix is never written: the
kernel streams the item matrix once per query tile and only ``k`` values and indices per query
leave it.

The pattern lowers when the ``MatMul``'s first operand is a 2-D activation (not transposed), its
second a 2-D constant (either ``transpose_b``), the optional bias a constant ``[N]``, ``k`` a
constant, ``sorted`` true, every link is read only by the next and is not fetched, and
``K.retrieve_eligible`` passes (``D % 32 == 0``, ``32 <= D <= 256``, ``k <= 128``, ``k <= N <
2^31``).  The items go to the device once as bf16 ``[N, D]`` and the bias as fp32, both interned
as weights are; the scratch of sorted per-chunk keys comes from the plan's slab.  In an fp8 plan
the step runs bf16 (a quantised query is dequantised first).

Everything else keeps the path it had: scores with a second reader or fetched, a fed ``k``,
``k > 128``, ``D`` outside the envelope, ``sorted=False`` or a ``TopKV2`` of anything but such a
``MatMul`` is a ``gemm`` step plus a glue ``TopKV2`` (``CompileError`` under ``strict``).
``Softmax -> TopKV2`` is the softmax kernel's (``_lower_softmax``).
"""
from __future__ import annotations

import torch

from ..ops import kernels as K
from .plan import _view


class RetrievalLowering:
    """Mixin of ``CompiledFunction`` (uses its graph, ``vals``, ``_single_consumer`` and emitters)."""

    def _lower_retrieval(self, node) -> bool:
        """``node`` is a ``MatMul``: emits the ``retrieve`` step and returns True when the pattern matches."""
        a, b = self._in(node, 0), self._in(node, 1)
        if a.is_const or not b.is_const or node.attr("transpose_a", False) or len(a.shape) != 2 or a.rows is not None \
                or a.phys_c or b.const.dim() != 2:
            return False
        nxt = self._single_consumer(node.name)
        bias_node = bias = None
        if nxt is not None and nxt.op in ("BiasAdd", "Add", "AddV2"):
            other = [i for i, (s, _) in enumerate(nxt.inputs) if s != node.name]
            ov = self._get(nxt.inputs[other[0]]) if len(other) == 1 else None
            if ov is None or not ov.is_const or ov.const.dim() != 1:
                return False
            bias_node, bias = nxt, ov.const.float()
            nxt = self._single_consumer(nxt.name)
        if nxt is None or nxt.op != "TopKV2" or not nxt.attr("sorted", True) or len(nxt.inputs) != 2 \
                or nxt.inputs[0] != ((bias_node or node).name, 0):
            return False
        kv = self._get(nxt.inputs[1])
        if kv is None or not kv.is_const:
            return False
        k = int(kv.const.reshape(-1)[0])
        w = b.const.float()
        items = w if node.attr("transpose_b", False) else w.t()
        N, D = items.shape
        B = a.shape[0]
        if a.shape[1] != D or (bias is not None and bias.numel() != N) or not K.retrieve_eligible(B, N, D, k):
            return False
        xin = self._as_bf16(a, node.name)
        items_dev = self._dev(items, torch.bfloat16)
        bias_dev = self._dev(bias, torch.float32) if bias is not None else None
        self.params += [items_dev] + ([bias_dev] if bias_dev is not None else [])
        chunk = K.retrieve_chunk(B, N, D, k)
        vals, idxs = self._new((B, k), torch.float32), self._new((B, k), torch.int32)
        scratch = self._new((K.retrieve_scratch_numel(B, N, k, chunk),), torch.int64)

        def run(xin=xin, vals=vals, idxs=idxs, scratch=scratch):
            K.retrieve_topk(_view(xin), items_dev, k, bias_dev, chunk=chunk, out=(vals.buf, idxs.buf), scratch=scratch.buf)

        self._emit(node.name, "retrieve", run, [xin], [vals, idxs, scratch],
                   {"N": N, "k": k, "chunks": -(-N // chunk), "bias": bias is not None})
        for n in ([bias_node] if bias_node is not None else []) + [nxt]:
            self._fused.add(n.name)
        self.vals[(nxt.name, 0)] = vals
        self.vals[(nxt.name, 1)] = idxs
        return True
