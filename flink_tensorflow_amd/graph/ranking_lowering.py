"""Lowering of ranking (CTR) graphs (a mixin of ``CompiledFunction``): embedding lookups by
categorical id and DLRM's pairwise dot interaction, on ``kernels/interact.hip``.

The interaction subgraph, node for node as ``GraphBuilder.dot_interaction`` emits it and TF
exports it (``vectors`` are ``M`` tensors ``[B, D]``, at most one of them not a lookup):

    e_f  = GatherV2(table_f [V_f, D] const, ids[:, c_f], axis 0)    GraphBuilder.embedding_lookup
    T    = Pack(vectors, axis=1)                                    [B, M, D]
           (or Reshape(ConcatV2(vectors, axis 1), [B, M, D]))
    Z    = BatchMatMul(T, T, adj_y=True)                            [B, M, M]
    flat = Reshape(Z, [-1, M * M])
    tri  = GatherV2(flat, const index vector, axis 1)               any entries of Z, any order
    out  = ConcatV2([x, tri], axis 1)                               optional, x the activation vector

It lowers to one ``interact`` step (``K.dot_interact``: ids and rows are read, the top MLP's input
row is written, nothing between reaches HBM) when every packed vector but at most one is such a
lookup of a constant 2-D table, the id columns are ``Unpack(axis=1)`` outputs or shrink-axis
``StridedSlice`` columns of one int32 ``[B, F]`` feed or activation, the remaining vector is a 2-D
activation, all tables share ``D``, the index vector names no entry of ``Z`` twice once mirrored
(``Z`` is symmetric), every link is read only by the next and none is fetched, and
``K.dot_interact_eligible`` passes (``M <= 64``, ``D % 16 == 0``, ``16 <= D <= 256``).  The tables
go to the device once as one bf16 ``[sum V_f, D]`` buffer, the per-vector (base, id column, V) as
int64 and the selection table as int16, all interned as weights are.  The step's value has the
logical shape ``[B, Wlog]`` over a buffer of ``Wout = roundup(Wlog, 8)`` columns (``phys_c``), the
pad columns zero: the ``MatMul`` behind it reads the buffer in place against weight rows
zero-padded to ``Wout`` (``_lower_matmul``), which is the only way a ``K % 8 != 0`` MatMul lowers.
An id outside ``[0, V_f)`` gives a zero vector.  In an fp8 plan the step runs bf16.

A lone ``GatherV2(const [V, D] table, int32 ids, axis 0)`` with ``D % 8 == 0`` is one ``embed``
step (``K.embed_rows``); when its only reader is a ``ConcatV2`` of such lookups on the last axis, the
rows are written into the concat's slice in place.

``CompiledFunction(..., table_precision="fp8")`` stores the tables of both steps as 8-bit tables
(``K.quantize_table_fp8``: e4m3 codes and one power-of-two exponent per row, half the bytes) and the
steps run ``kernels/interact_fp8.hip``; their meta carries ``"tables": "fp8"``.  A lone lookup with
``D % 16 != 0`` keeps its bf16 table.  The option is independent of ``precision``.

What stays glue (``CompileError`` under ``strict``): a fed or variable table, ``axis != 0``, int64
ids; id columns of different feeds inside an interaction (the ``BatchMatMul`` stays glue, and so do
the column ops); ``M > 64``, ``D`` outside the envelope, two activation vectors; ``Z`` or ``T`` with
a second reader or fetched; a duplicate index;
multi-hot bags (``SparseSegmentSum``, ``embedding_lookup_sparse``).
"""
from __future__ import annotations

import torch

from ..ops import kernels as K
from .plan import _coff, _target, _view

_BMM = ("BatchMatMul", "BatchMatMulV2", "BatchMatMulV3")
_GATHER = ("GatherV2", "Gather")


class RankingLowering:
    """Mixin of ``CompiledFunction`` (uses its graph, ``vals``, ``cons``, ``_fused`` and emitters)."""

    # ------------------------------------------------------------------ matching
    def _prematch_ranking(self):
        """Finds the interaction groups.  A group's nodes but its last are marked fused, so the
        scheduler skips them; the last one lowers the group once the id tensor and the activation
        vector exist (``_interact_ready``), or gives the nodes back to the op-by-op lowering."""
        self._interact: dict[str, dict] = {}
        for name in self.order:
            if self.graph[name].op in _BMM and name not in self._groups:
                grp = self._match_interaction(self.graph[name])
                if grp is not None:
                    self._interact[grp["last"]] = grp
                    self._fused |= grp["members"] - {grp["last"]}

    def _rank_reader(self, name: str, ops) -> "Node | None":
        readers = set(self.cons.get(name, []))
        if len(readers) != 1 or self._fetched(name):
            return None
        n = self.graph[next(iter(readers))]
        return n if n.op in ops else None

    def _const_node(self, src) -> bool:
        n = self.graph.nodes.get(src[0])
        while n is not None and n.op == "Identity":
            n = self.graph.nodes.get(n.inputs[0][0])
        return n is not None and n.op == "Const"

    def _id_column(self, src):
        """``src`` as a column of a 2-D id tensor: ``(tensor source, column, column node)`` or None."""
        n = self.graph.nodes.get(src[0])
        if n is None:
            return None
        if n.op == "Unpack" and int(n.attr("axis", 0)) == 1:
            return n.inputs[0], src[1], n
        if n.op == "StridedSlice" and n.attr("shrink_axis_mask", 0) == 2 and n.attr("begin_mask", 0) & 1 \
                and n.attr("end_mask", 0) & 1 and not n.attr("ellipsis_mask", 0) and not n.attr("new_axis_mask", 0):
            b, s = (self._const_val(i) for i in (n.inputs[1], n.inputs[3]))
            if b is None or s is None or b.const.numel() != 2 or s.const.reshape(-1).tolist() != [1, 1]:
                return None
            return n.inputs[0], int(b.const.reshape(-1)[1]), n
        return None

    def _match_interaction(self, bmm):
        g = self.graph
        if len(bmm.inputs) != 2 or bmm.inputs[0] != bmm.inputs[1] or not bmm.attr("adj_y", False) or bmm.attr("adj_x", False):
            return None
        pack = g.nodes.get(bmm.inputs[0][0])
        if pack is None or self._rank_reader(pack.name, _BMM) is None:
            return None
        packed, joined, width = list(pack.inputs), None, None
        if pack.op == "Reshape":  # ConcatV2(vectors, axis 1) + Reshape to [B, M, D] in place of Pack(axis=1)
            joined, shp = g.nodes.get(pack.inputs[0][0]), self._const_val(pack.inputs[1])
            if joined is None or joined.op != "ConcatV2" or self._rank_reader(joined.name, ("Reshape",)) is None or shp is None:
                return None
            ax, packed = self._const_val(joined.inputs[-1]), list(joined.inputs[:-1])
            if ax is None or int(ax.const.reshape(-1)[0]) not in (1, -1) or shp.const.numel() != 3 \
                    or int(shp.const.reshape(-1)[1]) != len(packed):
                return None
            width = int(shp.const.reshape(-1)[2])
        elif pack.op != "Pack" or int(pack.attr("axis", 0)) != 1:
            return None
        flat = self._rank_reader(bmm.name, ("Reshape",))
        tri = self._rank_reader(flat.name, _GATHER) if flat is not None else None
        if tri is None or tri.inputs[0][0] != flat.name or len(tri.inputs) != 3:
            return None
        idx, axis = self._const_val(tri.inputs[1]), self._const_val(tri.inputs[2])
        if idx is None or axis is None or idx.const.dim() != 1 or int(axis.const.reshape(-1)[0]) != 1:
            return None
        members, vectors, dense, id_src = {pack.name, bmm.name, flat.name, tri.name}, [], None, None
        if joined is not None:
            members.add(joined.name)
        for src in packed:
            n = g.nodes.get(src[0])
            col = None
            if n is not None and n.op in _GATHER and len(n.inputs) == 3 and self._const_node(n.inputs[0]) \
                    and self._rank_reader(n.name, ("Pack", "ConcatV2")) is not None:
                ax = self._const_val(n.inputs[2])
                col = self._id_column(n.inputs[1]) if ax is not None and int(ax.const.reshape(-1)[0]) == 0 else None
            if col is None:
                if dense is not None:
                    return None  # two activation vectors
                dense = src
                vectors.append(None)
                continue
            if id_src is not None and col[0] != id_src:
                return None  # id columns of different tensors
            id_src = col[0]
            members |= {n.name, col[2].name}
            vectors.append((n.inputs[0], col[1]))
        if id_src is None:
            return None
        for m in list(members):  # a column op read from outside the group has to run on its own
            if g[m].op in ("Unpack", "StridedSlice") and (self._fetched(m) or not set(self.cons.get(m, [])) <= members):
                return None
        last, copy = tri, False
        cat = self._rank_reader(tri.name, ("ConcatV2",))
        if cat is not None and dense is not None and len(cat.inputs) == 3 and cat.inputs[0] == dense \
                and cat.inputs[1] == (tri.name, 0):
            ax = self._const_val(cat.inputs[2])
            if ax is not None and int(ax.const.reshape(-1)[0]) in (1, -1):
                last, copy = cat, True
                members.add(cat.name)
        M = len(vectors)
        pairs = [(int(k) // M, int(k) % M) for k in idx.const.reshape(-1).tolist()]
        if any(not 0 <= k < M * M for k in idx.const.reshape(-1).tolist()) or not 1 <= M <= K.INTERACT_MAX_VECTORS:
            return None
        try:
            K.dot_interact_lut(M, pairs, 0)
        except ValueError:
            return None  # an entry of Z selected twice
        return {"members": members, "last": last.name, "vectors": vectors, "dense": dense, "ids": id_src, "pairs": pairs,
                "copy": copy, "width": width}

    def _interact_ready(self, name: str) -> bool | None:
        """None: ``name`` does not end a group; else whether the group's computed inputs are lowered."""
        grp = self._interact.get(name)
        if grp is None:
            return None
        return all(s in self.vals for s in (grp["ids"], grp["dense"]) if s is not None)

    # ------------------------------------------------------------------ lowering
    def _table(self, table: torch.Tensor):
        """The device form of a float ``[rows, D]`` table, interned as weights are: ``(bf16 table, None)``, or
        under ``table_precision="fp8"`` and ``D % 16 == 0`` ``(e4m3 codes, row exponents)``.  A table with an
        inf or NaN entry has no 8-bit form and stays bf16, as it lowers today."""
        if self.table_precision == "fp8" and table.shape[1] % 16 == 0 and bool(torch.isfinite(table).all()):
            stored = [self._dev(t) for t in K.quantize_table_fp8(table)]
        else:
            stored = [self._dev(table, torch.bfloat16), None]
        self.params += [t for t in stored if t is not None]
        return stored

    def _lower_interaction(self, node) -> bool:
        """``node`` ends a matched group: emits its ``interact`` step.  When the operands do not
        validate the members are lowered op by op, in order, and False lets ``node`` follow."""
        grp = self._interact.pop(node.name)
        if self._emit_interact(node, grp):
            self._fused.add(node.name)
            return True
        self._fused -= grp["members"]
        for m in self.order:
            if m in grp["members"] and m != node.name:
                for src in self.graph[m].inputs:
                    self._const_val(src)  # fold the constant operands the scheduler has not reached yet
                self._lower(self.graph[m])
        return False

    def _emit_interact(self, node, grp) -> bool:
        ids = self._get(grp["ids"])
        dense = self._get(grp["dense"]) if grp["dense"] is not None else None
        if ids is None or ids.is_const or ids.dtype != torch.int32 or len(ids.shape) != 2 or ids.phys_c or ids.rows is not None:
            return False
        B, F = ids.shape
        tables, meta, base, known = [], [], 0, {}
        for v in grp["vectors"]:
            if v is None:
                meta.append((0, -1, 0))
                continue
            src, col = v
            t = self._const_val(src)
            if t is None or not isinstance(t.const, torch.Tensor) or t.const.dim() != 2 or not 0 <= col < F:
                return False
            if src not in known:  # a table shared by two fields is stored once
                known[src] = base
                tables.append(t.const.float())
                base += t.const.shape[0]
            meta.append((known[src], col, t.const.shape[0]))
        D = tables[0].shape[1]
        M, copy = len(meta), grp["copy"]
        wlog = (D if copy else 0) + len(grp["pairs"])
        if any(t.shape[1] != D for t in tables) or grp["width"] not in (None, D) or not K.dot_interact_eligible(M, D, wlog):
            return False
        if dense is not None and (dense.is_const or tuple(dense.shape) != (B, D) or dense.rows is not None
                                  or dense.dtype not in (torch.bfloat16, torch.float32, torch.uint8)):
            return False
        xin = self._as_bf16(dense, node.name) if dense is not None else None
        table_dev, exp_dev = self._table(torch.cat(tables))
        meta_dev = self._dev(torch.tensor(meta, dtype=torch.int64).t().contiguous())
        lut_dev = self._dev(K.dot_interact_lut(M, grp["pairs"], D if copy else 0))
        self.params += [meta_dev, lut_dev]
        wout = -(-wlog // 8) * 8
        out = self._new((B, wlog), phys_c=wout if wout != wlog else None)
        if wout != wlog:
            out.buf_shape = (B, wout)

        def run(ids=ids, xin=xin, out=out):
            K.dot_interact(table_dev, _view(ids), meta_dev, lut_dev, wlog, _view(xin) if xin is not None else None, copy,
                           out=out.buf, table_exp=exp_dev)

        self._emit(node.name, "interact", run, [ids] + ([xin] if xin is not None else []), [out],
                   {"M": M, "D": D, "width": wlog, "fields": M - (dense is not None),
                    **({"tables": "fp8"} if exp_dev is not None else {})})
        self.vals[(node.name, 0)] = out
        return True

    def _lower_embedding(self, node) -> bool:
        """A lone ``GatherV2(const [V, D] table, int32 ids, axis 0)`` as one ``embed`` step."""
        if len(node.inputs) != 3 or not self._const_node(node.inputs[0]):
            return False
        t, ax, ids = self._const_val(node.inputs[0]), self._const_val(node.inputs[2]), self._get(node.inputs[1])
        if t is None or ax is None or ids is None or ids.is_const or int(ax.const.reshape(-1)[0]) != 0:
            return False
        if not isinstance(t.const, torch.Tensor) or t.const.dim() != 2 or t.const.shape[1] % 8 or ids.dtype != torch.int32 \
                or ids.phys_c or ids.rows is not None or not ids.shape or min(ids.shape) < 1:
            return False
        V, D = t.const.shape
        table_dev, exp_dev = self._table(t.const.float())
        out = self._new((*ids.shape, D))

        def run(ids=ids, out=out):  # a sole ConcatV2 reader: the rows go straight into its slice (``_lower_concat``)
            tgt, off = _target(out), _coff(out)
            K.embed_rows(table_dev, _view(ids).reshape(-1), 0, V, out=tgt.view(-1, tgt.shape[-1])[:, off:off + D],
                         table_exp=exp_dev)

        self._emit(node.name, "embed", run, [ids], [out], {"V": V, "D": D, **({"tables": "fp8"} if exp_dev is not None else {})})
        self.vals[(node.name, 0)] = out
        return True
