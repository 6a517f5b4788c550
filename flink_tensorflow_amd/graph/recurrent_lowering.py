"""Lowering of recurrent layers (a mixin of ``CompiledFunction``): ``BlockLSTM`` to one
``gemm`` step (the input projection, on the existing GEMM launchers) plus one ``lstm`` step on
``kernels/lstm.hip``, with the layout ops around it absorbed.

**The op.**  ``BlockLSTM`` (TF's fused cell, gate columns i, ci, f, o) lowers when

* ``w``, ``b``, the three peephole vectors and ``seq_len_max`` are constants;
* ``x`` is a 3-D activation or a fed tensor (a fed fp32 ``x`` goes through the plan's cast);
* ``cs_prev`` / ``h_prev`` are constants, or ``[B, H]`` activations or feeds (a caller that
  carries the state from window to window feeds them and fetches the last states);
* the shape is inside ``K.lstm_eligible`` (``H`` a multiple of 16 up to 512, ``I`` a multiple of 8);
* only the outputs ``h`` (6) and ``cs`` (1) are read or fetched: ``i, f, o, ci, co`` exist for
  the training graph.

Anything else keeps the op as glue (the interpreter's routine, one captured PyTorch op per
gate and step), which is a ``CompileError`` under ``strict``.

The projection ``x . w[:I] + b`` (``forget_bias`` added on the ``f`` columns) runs once over
all ``T * B`` rows with the bias epilogue and a single rounding to bf16; the ``lstm`` step adds
``h_{t-1} . w[I:]`` per step from weights packed at compile time (``K.lstm_pack_weights``).
Both run bf16 in an fp8 plan, like ``dwconv`` and ``resize``.

**Absorbed layout ops** (no step, no buffer):

* ``Transpose(perm=[1, 0, 2])`` in front, batch-major ``[B, T, I]`` to time-major, read by the
  ``BlockLSTM`` alone: the projection is row-wise, so it runs on the ``B * T`` rows as they
  lie, and the ``lstm`` step reads ``xproj`` with swapped strides (``Val.tm_of``).
* the same ``Transpose`` behind ``h``, when nothing else reads ``h``: the step writes
  batch-major ``[B, T, H]``.
* ``StridedSlice`` of the last time step of ``h`` or ``cs`` (``h[T - 1]`` or ``h[-1]`` with the
  shrink-axis bit of axis 0, the other axes whole), when the ``[T, B, H]`` value has no other
  reader, is not fetched and ``seq_len_max >= T``: the step stores only ``h_{T-1}`` (``[B, H]``
  bf16) or the final cell state (``[B, H]`` fp32).
* stacked layers need nothing: layer 2's ``x`` is layer 1's time-major bf16 ``h``.

A ``[1, 0, 2]`` transpose next to a ``BlockLSTM`` that cannot be absorbed (a second reader, a
fetched ``h``) is a ``copy`` step; other transposes stay what they were.
"""
from __future__ import annotations

import torch

from ..ops import kernels as K
from .plan import Val, _view


class RecurrentLowering:
    """Mixin of ``CompiledFunction`` (uses its graph, ``cons``, ``vals``, ``_fetched`` and emitters,
    and the graph helper ``_const_of`` of the ``TransformerLowering`` mixin)."""

    # ------------------------------------------------------------------ graph helpers
    def _is_tb_transpose(self, node) -> bool:
        if node is None or node.op != "Transpose" or len(node.inputs) != 2:
            return False
        perm = self._const_of(node.inputs[1])
        return perm is not None and [int(v) for v in perm.reshape(-1).tolist()] == [1, 0, 2]

    def _out_readers(self, name: str, k: int) -> list:
        """The (node, input position) pairs of the pruned graph that read output ``k`` of ``name``."""
        out = []
        for c in dict.fromkeys(self.cons.get(name, [])):
            node = self.graph[c]
            out += [(node, i) for i, src in enumerate(node.inputs) if src == (name, k)]
        return out

    def _out_fetched(self, name: str, k: int) -> bool:
        return f"{name}:{k}" in self.fetch_names  # they are normalised to ``node:index``

    def _is_last_step_slice(self, node, shape) -> bool:
        """``x[T - 1]`` / ``x[-1]`` of a ``[T, B, H]`` value as a StridedSlice: axis 0 shrunk,
        every other axis whole."""
        if node.op != "StridedSlice" or len(shape) != 3:
            return False
        b, e, s = (self._const_of(node.inputs[i]) for i in (1, 2, 3))
        if b is None or e is None or s is None or not 1 <= b.numel() <= 3:
            return False
        if node.attr("ellipsis_mask", 0) or node.attr("new_axis_mask", 0) or node.attr("shrink_axis_mask", 0) != 1:
            return False
        b, e, s = (t.reshape(-1).tolist() for t in (b, e, s))
        bm, em = node.attr("begin_mask", 0), node.attr("end_mask", 0)
        if any(v != 1 for v in s) or bm & 1 or b[0] not in (shape[0] - 1, -1):
            return False
        return all((bm >> d & 1 or b[d] == 0) and (em >> d & 1 or e[d] >= shape[d]) for d in range(1, len(b)))

    # ------------------------------------------------------------------ the transposes
    def _lower_tb_transpose(self, node) -> bool:
        """``Transpose(perm=[1, 0, 2])`` next to a ``BlockLSTM``: absorbed in front of it when it
        feeds nothing else, else a ``copy`` step.  False: not ours (no BlockLSTM on either side)."""
        if not self._is_tb_transpose(node):
            return False
        x = self._get(node.inputs[0])
        if x is None or x.is_const or len(x.shape) != 3 or x.rows is not None or x.phys_c or x.qscale is not None \
                or x.tm_of is not None or x.dtype not in (torch.bfloat16, torch.float32):
            return False
        readers = [self.graph[c] for c in self.cons.get(node.name, [])]
        feeds_lstm = any(c.op == "BlockLSTM" for c in readers)
        src = self.graph.nodes.get(node.inputs[0][0])
        if not feeds_lstm and (src is None or src.op != "BlockLSTM"):
            return False
        B, T, C = x.shape
        out = self._new((T, B, C), x.dtype)
        if len(readers) == 1 and readers[0].op == "BlockLSTM" and not self._fetched(node.name) \
                and [i for i, s in enumerate(readers[0].inputs) if s[0] == node.name] == [1]:
            out.tm_of = x  # no step: the BlockLSTM reads the batch-major rows in place
        else:
            def run(x=x, out=out):
                out.buf.copy_(_view(x).permute(1, 0, 2))

            self._emit(node.name, "copy", run, [x], [out])
        self.vals[(node.name, 0)] = out
        return True

    def _lstm_glue(self, node):
        """The op stays glue: a time-major view without a buffer gets one first."""
        x = self.vals.get(node.inputs[1])
        if x is not None and x.tm_of is not None and not self.strict:
            src, x.tm_of = x.tm_of, None

            def run(src=src, x=x):
                x.buf.copy_(_view(src).permute(1, 0, 2))

            self._emit(node.name + "/time_major", "copy", run, [src], [x])
        return self._lower_glue(node)

    # ------------------------------------------------------------------ BlockLSTM
    def _lstm_state(self, src, B, H, name, dtype):
        """``cs_prev`` / ``h_prev`` as (Val or None, device constant or None); None: refuse."""
        v = self._get(src)
        if v is None or tuple(v.shape) != (B, H):
            return None
        if v.is_const:
            t = self._dev(v.const.float().reshape(B, H), dtype)
            self.params.append(t)
            return None, t
        if v.rows is not None or v.phys_c or v.tm_of is not None or (v.qscale is None and v.dtype not in (
                torch.bfloat16, torch.float32)):
            return None
        if v.qscale is not None or (dtype == torch.bfloat16 and v.dtype != torch.bfloat16):
            v = self._as_bf16(v, name)
        return v, None

    def _lower_block_lstm(self, node):
        if len(node.inputs) != 9:
            return self._lstm_glue(node)
        slm, w, wci, wcf, wco, b = (self._const_of(node.inputs[i]) for i in (0, 4, 5, 6, 7, 8))
        x = self._get(node.inputs[1])
        if any(t is None for t in (slm, w, wci, wcf, wco, b)) or x is None or x.is_const or len(x.shape) != 3 \
                or x.rows is not None or x.phys_c or w.dim() != 2:
            return self._lstm_glue(node)
        T, B, I = x.shape
        H = w.shape[1] // 4
        peep = bool(node.attr("use_peephole", False))
        if tuple(w.shape) != (I + H, 4 * H) or b.numel() != 4 * H or not K.lstm_eligible(T, B, I, H) \
                or (peep and any(t.numel() != H for t in (wci, wcf, wco))):
            return self._lstm_glue(node)
        used = {k for k in range(7) if self._out_readers(node.name, k) or self._out_fetched(node.name, k)}
        if used - {1, 6}:
            return self._lstm_glue(node)  # gate outputs are read: the training graph's form
        src = x.tm_of if x.tm_of is not None else x
        if src.qscale is None and src.dtype not in (torch.bfloat16, torch.float32):
            return self._lstm_glue(node)
        c0 = self._lstm_state(node.inputs[2], B, H, node.name + "/cs_prev", torch.float32)
        h0 = self._lstm_state(node.inputs[3], B, H, node.name + "/h_prev", torch.bfloat16)
        if c0 is None or h0 is None:
            return self._lstm_glue(node)
        steps = max(0, min(T, int(slm.reshape(-1)[0])))
        batch_major = x.tm_of is not None

        # ---- the projection: one GEMM over the T * B rows as they lie
        xin = self._as_bf16(src, node.name + "/x")
        rows = Val((T * B, I), torch.bfloat16, alias_of=xin)
        wf, bias = w.float(), b.float().reshape(-1).clone()
        bias[2 * H:3 * H] += float(node.attr("forget_bias", 1.0))
        w_dev = self._dev(wf[:I].t().contiguous(), torch.bfloat16)
        b_dev = self._dev(bias, torch.float32)
        wpk = self._dev(K.lstm_pack_weights(wf[I:].to(torch.bfloat16), H))
        pw = [self._dev(t.float().reshape(H), torch.float32) for t in (wci, wcf, wco)] if peep else [None] * 3
        self.params += [w_dev, b_dev, wpk] + [t for t in pw if t is not None]
        xproj = self._new((T * B, 4 * H))
        if self.device.type == "cuda" and I % 64 == 0:
            splits = K.gemm_pp_splits(T * B, 4 * H, I)
            ws = torch.empty(splits * T * B * 4 * H, dtype=torch.float32, device=self.device) if splits > 1 else None

            def run_proj(rows=rows, xproj=xproj, w_dev=w_dev, b_dev=b_dev, splits=splits, ws=ws):
                K.gemm_pp(_view(rows), w_dev, b_dev, None, K.ACT_NONE, out=xproj.buf, splits=splits, ws=ws)

            meta = {"impl": "gemm_pp", "splits": splits}
        else:
            def run_proj(rows=rows, xproj=xproj, w_dev=w_dev, b_dev=b_dev):
                K.gemm(_view(rows), w_dev, b_dev, None, K.ACT_NONE, out=xproj.buf)

            meta = {}
        self._emit(node.name + "/xproj", "gemm", run_proj, [xin], [xproj], meta)

        # ---- what the step writes
        def sole_reader(k):
            rd = self._out_readers(node.name, k)
            return rd[0][0] if len(rd) == 1 and rd[0][1] == 0 and not self._out_fetched(node.name, k) else None

        h_mode, hv = "all", None
        nxt = sole_reader(6)
        if nxt is not None and self._is_tb_transpose(nxt):
            h_mode, hv = "batch_major", self._new((B, T, H))
            self.vals[(nxt.name, 0)] = hv
            self._fused.add(nxt.name)
        elif nxt is not None and steps == T and self._is_last_step_slice(nxt, (T, B, H)):
            h_mode, hv = "last", self._new((B, H))
            self.vals[(nxt.name, 0)] = hv
            self._fused.add(nxt.name)
        else:
            hv = self._new((T, B, H))
            self.vals[(node.name, 6)] = hv
        csv = clv = None
        if 1 in used:
            nxt = sole_reader(1)
            if nxt is not None and steps == T and self._is_last_step_slice(nxt, (T, B, H)):
                clv = self._new((B, H), torch.float32)
                self.vals[(nxt.name, 0)] = clv
                self._fused.add(nxt.name)
            else:
                csv = self._new((T, B, H))
                self.vals[(node.name, 1)] = csv
        clip = float(node.attr("cell_clip", 3.0))

        def run(xproj=xproj, hv=hv, csv=csv, clv=clv, h0=h0, c0=c0, wpk=wpk, pw=pw):
            xp = xproj.buf.view(B, T, 4 * H).transpose(0, 1) if batch_major else xproj.buf.view(T, B, 4 * H)
            K.lstm_seq(xp, wpk, _view(h0[0]) if h0[0] is not None else h0[1],
                       _view(c0[0]) if c0[0] is not None else c0[1], wci=pw[0], wcf=pw[1], wco=pw[2], cell_clip=clip,
                       steps=steps, h_out=hv.buf.transpose(0, 1) if h_mode == "batch_major" else hv.buf,
                       cs_out=csv.buf if csv is not None else None, c_last=clv.buf if clv is not None else None,
                       last_only=h_mode == "last")

        self._emit(node.name, "lstm", run, [xproj] + [s[0] for s in (h0, c0) if s[0] is not None],
                   [v for v in (hv, csv, clv) if v is not None],
                   {"impl": K.lstm_impl(H), "T": T, "B": B, "I": I, "H": H, "steps": steps, "peephole": peep,
                    "x": "batch_major" if batch_major else "time_major", "h": h_mode,
                    "cs": "last" if clv is not None else ("all" if csv is not None else None)})
