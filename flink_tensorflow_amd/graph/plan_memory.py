"""Memory planning of a compiled plan (the ``PlanMemory`` mixin of ``CompiledFunction``): buffers
for feeds and fetches, one liveness-planned activation slab, and the batch-slice chain."""
from __future__ import annotations

import logging

import torch

from ..batching.arena import plan_offsets
from .plan import Chain, Val, _buf_shape, _cfg, _nbytes, _root

LOG = logging.getLogger("flink_tensorflow_amd.compiler")


class PlanMemory:
    def _plan_memory_and_bind(self):
        """Feeds and fetched values get persistent buffers (arena blocks); every other produced value lives
        at a planned offset of one activation slab — lifetimes [producing step, last reading step] never
        overlap in memory (native liveness planner, ``batching/arena.py``).  With a subtask arena the slab is
        shared by all of the subtask's plans (they replay serially on one stream)."""
        for f in self.feed_names:
            v = self._val_of(f)
            v.buf = self._persistent(v.shape, v.dtype)
            self._input_bufs[f] = v.buf
        fetch_vals = [self._val_of(f) for f in self.fetch_names]
        for i, s in enumerate(self.steps):
            for v in s.inputs:
                _root(v).last_use = max(_root(v).last_use, i)
        keep = {id(_root(v)) for v in fetch_vals}
        chain = self._find_chain(keep)
        internal = chain.internal if chain else {}
        owners: dict[int, Val] = {}   # buffer-owning values in order of first production
        born: dict[int, int] = {}
        for i, s in enumerate(self.steps):
            for o in s.outputs:
                r = _root(o)
                if r.buf is not None:
                    continue
                tgt = r.concat_slot[0] if r.concat_slot else r  # branches write into their concat
                if tgt.buf is None and id(tgt) not in owners:
                    owners[id(tgt)] = tgt
                    born[id(tgt)] = i
        for t in owners.values():
            t.last_use = max([t.last_use] + [c.last_use for c in t.concat_children or []])
        transient = []
        for k, t in owners.items():
            if k in internal:
                continue  # slice-sized buffer in the chain's own slab (below)
            if k in keep:
                t.buf = self._persistent(_buf_shape(t), t.dtype)
            else:
                transient.append(t)
        sizes = [_nbytes(_buf_shape(t), t.dtype) for t in transient]
        first = [born[id(t)] for t in transient]
        last = [max(born[id(t)], t.last_use) for t in transient]
        if chain:
            # a tensor the chain writes is written by its first slice pass and one it reads is
            # read by its last: both live across the whole chain
            i0, i1 = chain.range
            for j, t in enumerate(transient):
                if id(t) in chain.touched:
                    if i0 <= first[j] < i1:
                        first[j] = i0
                    if last[j] >= i0:
                        last[j] = max(last[j], i1 - 1)
            # the slice-sized internals form one region of the same slab, live across the chain
            chain_layout = self._plan_chain(chain, born)
            sizes.append(max(chain_layout[1], 1))
            first.append(i0)
            last.append(i1 - 1)
        offs, total = plan_offsets(sizes, first, last)
        self.activation_bytes = total
        slab = self.arena.shared_slab(total) if self.arena is not None else \
            torch.empty(max(total, 1), dtype=torch.uint8, device=self.device)
        for t, off, nb, lu in zip(transient, offs, sizes, last):
            t.buf = slab[off:off + nb].view(t.dtype).view(tuple(_buf_shape(t)))
            self._poison_after.setdefault(lu, []).append(t.buf)
        if chain:
            self._bind_chain(chain, chain_layout, slab, offs[-1])
        for v in self.vals.values():
            if v.alias_of is not None:
                r = _root(v)
                if r.buf is not None:
                    shape = v.shape if id(r) not in internal else (chain.batch, *v.shape[1:])
                    v.buf = r.buf.view(shape) if r.buf.is_contiguous() else r.buf.reshape(shape)
        if chain:
            chain.external = [v for v in chain.vals if id(_root(v)) not in internal]
            chain.bound = [v for v in chain.vals if id(_root(v)) in internal and v.buf is not None]
            self._chain = chain
        self._outputs = [fv.const if fv.is_const else fv for fv in fetch_vals]

    # ================================================================== batch-slice chain
    _CHAIN_KINDS = ("conv", "gemm", "pool", "elementwise", "conv_fp8", "pool_fp8")
    # persistent kernels that load a resident weight bank per launch
    _PERSISTENT_IMPLS = ("conv3x3c64", "bottleneck_tail", "bottleneck_chain", "pw_res")

    def _find_chain(self, keep: set) -> Chain | None:
        """The leading run of memory-bound layers that executes once per slice of ``EngineConfig.chain_batch``
        images instead of once over the batch (None when off or nothing qualifies).

        Every step of the run is per-image (convs, pools, element-wise) and every tensor it touches is NHWC
        with at least ``chain_min_hw`` pixels per image — ResNet-50's stem and 56x56 stage 1, where each
        tensor is 100-400 MB per 256-image batch and every layer streams it from HBM.  Per slice those tensors
        are 13-51 MB: the values made and consumed inside the run ("internal") get slice-sized buffers reused
        by every slice, so a layer reads what the previous one just wrote from the Infinity Cache (256 MiB)
        and a dead intermediate is overwritten there before it is written back.  Values entering or leaving
        the run keep their full buffers and are sliced."""
        cfg = _cfg()
        bs = int(cfg.chain_batch or 0)
        auto = bs < 0
        if auto:
            bs = 32
        if bs == 0 or self._pack is not None or not self.steps or not self.feed_names:
            return None
        shape = self._val_of(self.feed_names[0]).shape
        N = shape[0] if shape else 0
        if not N or -(-N // bs) < 2:
            return None

        def val_ok(v):
            if v is None or v.is_const:
                return True
            r = _root(v)
            if v.rows is not None or v.concat_slot is not None or r.concat_slot is not None or r.is_const:
                return False
            return len(v.shape) == 4 and v.shape[0] == N and _buf_shape(r)[0] == N

        def step_ok(st):
            vs = [v for v in list(st.inputs) + list(st.outputs) if v is not None and not v.is_const]
            if st.kind not in self._CHAIN_KINDS or not vs or not all(val_ok(v) for v in vs):
                return False
            if auto and st.meta.get("impl") in self._PERSISTENT_IMPLS:
                return False  # its per-launch weight prologue outweighs the cache residency (r04_d)
            big = [v.shape[1] * v.shape[2] >= cfg.chain_min_hw for v in vs]
            # chain_edge: a layer reading the large resolution into a smaller one (the next
            # stage's stride-2 conv / projection) joins too, so its large input stays internal
            return any(big) if cfg.chain_edge else all(big)

        start = 1 if self.steps[0].kind == "preprocess" else 0  # the head runs per H2D piece
        best, i = None, start
        while i < len(self.steps):
            if not step_ok(self.steps[i]):
                i += 1
                continue
            j = i
            while j < len(self.steps) and step_ok(self.steps[j]):
                j += 1
            if j - i >= 2 and (best is None or j - i > best[1] - best[0]):
                best = (i, j)
            i = j
        if best is None:
            return None
        i0, i1 = best
        vals, touched = [], set()
        for st in self.steps[i0:i1]:
            for v in list(st.inputs) + list(st.outputs):
                while v is not None and not v.is_const:
                    if all(v is not u for u in vals):
                        vals.append(v)
                    touched.add(id(_root(v)))
                    v = v.alias_of
        produced = {id(_root(o)) for st in self.steps[i0:i1] for o in st.outputs}
        used_outside = {id(_root(v)) for k, st in enumerate(self.steps) if not i0 <= k < i1
                        for v in list(st.inputs) + list(st.outputs) if v is not None and not v.is_const}
        feeds = {id(_root(self._val_of(f))) for f in self.feed_names}
        internal = {}
        for v in vals:
            r = _root(v)
            k = id(r)
            if k in produced and k not in used_outside and k not in keep and k not in feeds and r.buf is None:
                internal[k] = r
        return Chain(range=(i0, i1), batch=bs, parts=-(-N // bs), n=N, vals=vals, touched=touched, internal=internal)

    def _plan_chain(self, chain: Chain, born: dict) -> tuple:
        """Layout of the chain's slice-sized internal values, planned by the same liveness
        planner over the chain's own step range (one slice's lifetime): (offsets, total)."""
        i0, i1 = chain.range
        ts = list(chain.internal.values())
        shapes = [(chain.batch, *_buf_shape(t)[1:]) for t in ts]
        sizes = [_nbytes(s, t.dtype) for s, t in zip(shapes, ts)]
        first = [born[id(t)] - i0 for t in ts]
        last = [max(born[id(t)], min(t.last_use, i1 - 1)) - i0 for t in ts]
        return plan_offsets(sizes, first, last)

    def _bind_chain(self, chain: Chain, layout: tuple, slab: torch.Tensor, base: int):
        """Binds the chain's internal values into their region ``[base, base + total)`` of
        the activation slab (the subtask arena's shared slab when there is one)."""
        i0, i1 = chain.range
        offs, total = layout
        for t, off in zip(chain.internal.values(), offs):
            s = (chain.batch, *_buf_shape(t)[1:])
            nb = _nbytes(s, t.dtype)
            t.buf = slab[base + off:base + off + nb].view(t.dtype).view(s)
        self.chain_bytes = total
        self.chain_layers = i1 - i0
        LOG.info("batch-slice chain: steps %d-%d (%s .. %s) x %d slices of %d, %d internal values in %.1f MB", i0,
                 i1 - 1, self.steps[i0].name, self.steps[i1 - 1].name, chain.parts, chain.batch, len(offs), total / 1e6)

    def _persistent(self, shape, dtype) -> torch.Tensor:
        """A buffer outside the shared slab (plan inputs, fetched outputs)."""
        if self.arena is not None:
            return self.arena.alloc(tuple(shape), dtype)
        return torch.empty(tuple(shape), dtype=dtype, device=self.device)

    def _dev(self, t: torch.Tensor, dtype=None) -> torch.Tensor:
        """A baked-in weight on the device; identical weights of a subtask's bucket plans
        are stored once in its arena."""
        t = t.to(dtype) if dtype is not None else t
        if self.arena is not None:
            return self.arena.intern(t.contiguous())
        return t.to(self.device).contiguous()
