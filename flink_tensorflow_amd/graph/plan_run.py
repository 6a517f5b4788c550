"""Running a compiled plan (the ``PlanRunner`` mixin of ``CompiledFunction``): eager launches
with the batch-slice chain once per slice, profiling, fp8 calibration, hipGraph capture and
replay, and the pipelined runner's head bypass."""
from __future__ import annotations

import torch

from ..ops import fp8 as F8
from ..types.dtypes import DataType
from ..types.names import TensorName
from ..types.tensor import StringTensor
from ..utils import tracing
from .plan import CompileError, Val, _eff_scale, _root, _view


class PlanRunner:
    # ------------------------------------------------------------------ calibration
    def synthetic_feeds(self, seed: int = 0) -> dict:
        g = torch.Generator().manual_seed(seed)
        out = {}
        for f in self.feed_names:
            shape, dt = self.feed_specs[f]
            dt = DataType.of(dt).torch
            if dt == torch.uint8:
                out[f] = torch.randint(0, 256, tuple(shape), generator=g, dtype=torch.uint8)
            elif dt.is_floating_point:
                out[f] = torch.randn(tuple(shape), generator=g).to(dt)
            else:
                out[f] = torch.randint(0, 100, tuple(shape), generator=g).to(dt)
        return out

    @torch.no_grad()
    def calibrate(self, feeds: dict | None = None) -> dict[str, float]:
        """Runs the plan step by step on ``feeds`` (synthetic when None) and returns the
        absolute maximum of every computed value, keyed by graph node name."""
        for k, v in (feeds or self.synthetic_feeds()).items():
            self.input_buffer(k).copy_(v)
        by_id: dict[int, float] = {}

        def each(s):  # a batch-slice chain step runs once per slice: max over the slices
            s.fn()
            for o in s.outputs:
                t = _view(o)
                if t.is_floating_point() and t.numel():
                    k = id(_root(o))
                    by_id[k] = max(by_id.get(k, 0.0), float(t.float().abs().max()))

        self._run_range(0, len(self.steps), each)
        for v in self.vals.values():  # concat targets: max over their stride-written children
            if v.concat_children:
                by_id[id(v)] = max(by_id.get(id(_root(c)), 0.0) for c in v.concat_children)
        return {n: by_id[id(_root(v))] for (n, _), v in self.vals.items() if id(_root(v)) in by_id}

    # ------------------------------------------------------------------ execution
    def _run_range(self, lo: int, hi: int, each=None):
        """Launches steps[lo:hi] (``each(step)`` instead of ``step.fn()`` if given), the batch-slice chain once
        per slice: the chain's external values are rebound to the slice's rows while its steps launch (eager,
        or into a capture) and restored after.  A plan is driven by one thread at a time (one lane = one stream)."""
        each = each or (lambda st: st.fn())
        ch = self._chain
        c0, c1 = ch.range if ch is not None else (0, 0)
        if c0 < lo < c1 or c0 < hi < c1:
            raise CompileError(f"steps [{lo}, {hi}) cut the batch-slice chain [{c0}, {c1})")
        i = lo
        while i < hi:
            if ch is not None and i == c0 and c1 <= hi:
                for p in range(ch.parts):
                    self._run_chain_slice(p, each)
                i = c1
                continue
            each(self.steps[i])
            i += 1

    def _run_chain_slice(self, p: int, each):
        """The chain's steps for slice ``p`` (images [p*bs, (p+1)*bs)), its external values
        rebound to the slice's rows while they launch."""
        ch = self._chain
        i0, i1 = ch.range
        lo, hi = p * ch.batch, min(ch.n, (p + 1) * ch.batch)
        full = [(v, v.buf, True) for v in ch.external if v.buf is not None]
        if hi - lo < ch.batch:  # the short last slice: the slice-sized internals' leading rows
            full += [(v, v.buf, False) for v in ch.bound]
        try:
            for v, b, external in full:
                v.buf = b[lo:hi] if external else b[:hi - lo]
            for st in self.steps[i0:i1]:
                each(st)
        finally:
            for v, b, _ in full:
                v.buf = b

    def _run_steps(self):
        if not (self._debug_sync or self._poison_after and tracing.debug_poison()):
            self._run_range(0, len(self.steps))
            return
        poison = tracing.debug_poison()
        index = {id(s): i for i, s in enumerate(self.steps)}
        c0, c1 = self._chain.range if self._chain is not None else (0, 0)

        def each(s):
            i = index[id(s)]
            s.fn()
            if self._debug_sync and self.device.type == "cuda":
                try:
                    torch.cuda.synchronize(self.device)
                except RuntimeError as e:
                    raise RuntimeError(f"step {i} ({s.kind} {s.name}) failed: {e}") from e
            if poison and not c0 <= i < c1:  # chain buffers: live per slice
                for b in self._poison_after.get(i, ()):
                    b.view(-1).view(torch.uint8).fill_(0xFF)  # NaN in bf16/fp32, 0xFF in e4m3 = NaN

        self._run_range(0, len(self.steps), each)

    def profile(self, feeds: dict | None = None):
        """One eager run with a HIP event pair around every launch: a ``RunMetadata``
        whose ``NodeExecStats`` carry the per-step device time (``timeline_label`` = kind)
        — the compiled counterpart of ``Session.run(run_metadata=True)``."""
        from ..proto.messages import DeviceStepStats, NodeExecStats, RunMetadata, StepStats

        for k, v in (feeds or {}).items():
            self.input_buffer(k).copy_(v)
        stats = []
        index = {id(s): i for i, s in enumerate(self.steps)}
        if self.device.type == "cuda":
            evs = [[] for _ in self.steps]  # a chain step launches once per batch slice

            def each(s):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                s.fn()
                e1.record()
                evs[index[id(s)]].append((e0, e1))

            self._run_range(0, len(self.steps), each)
            torch.cuda.synchronize(self.device)
            times = [sum(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev) for ev in evs]
        else:
            import time

            times = [0.0] * len(self.steps)

            def each(s):
                t0 = time.perf_counter()
                s.fn()
                times[index[id(s)]] += (time.perf_counter() - t0) * 1e6

            self._run_range(0, len(self.steps), each)
        t = 0
        for s, us in zip(self.steps, times):
            stats.append(NodeExecStats(node_name=s.name, all_start_micros=int(t), op_end_rel_micros=int(us),
                                       all_end_rel_micros=int(us), timeline_label=s.kind))
            t += us
        return RunMetadata(step_stats=StepStats(dev_stats=[DeviceStepStats(device=str(self.device),
                                                                           node_stats=stats)]))

    def _capture(self):
        with tracing.capture_lock():  # warm-up + device sync + capture: no sibling capture in between
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s):
                for _ in range(2):
                    self._run_steps()
            torch.cuda.current_stream(self.device).wait_stream(s)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with tracing.graph_capture(g):
                self._run_steps()
            self._graph_obj = g
            self._head = self._head_feed_step()
            if self._head is not None:
                # the two graphs of a plan never replay concurrently (one lane = one stream):
                # the tail graph shares the full graph's private memory pool
                gt = torch.cuda.CUDAGraph()
                with tracing.graph_capture(gt, pool=g.pool()):
                    self._run_range(1, len(self.steps))
                self._graph_tail = gt

    def _head_feed_step(self):
        """``(feed, step)`` when the first step is the plan's head (the preprocess kernel, or the stem conv it
        folded into) with a ``head`` launcher and its input is a feed buffer no other step and no fetch reads."""
        st = self.steps[0] if self.steps else None
        if st is None or st.kind != "preprocess" or st.head is None or len(st.inputs) != 1 or st.inputs[0].buf is None:
            return None
        x = st.inputs[0]
        feeds = [k for k, b in self._input_bufs.items() if b.data_ptr() == x.buf.data_ptr()]
        if len(feeds) != 1:
            return None
        # compare alias roots (a Reshape of the feed is an alias Val sharing its buffer) and
        # buffer addresses: any other reader of the raw feed needs the input_buffer copy
        rx, ptr = _root(x), x.buf.data_ptr()

        def reads_feed(v):
            return v is not None and (_root(v) is rx or (v.buf is not None and v.buf.data_ptr() == ptr))

        if any(reads_feed(i) for t in self.steps[1:] for i in t.inputs) or any(reads_feed(o) for o in self._outputs):
            return None
        return feeds[0], st

    def input_buffer(self, feed: str) -> torch.Tensor:
        return self._input_bufs[str(TensorName.parse(feed))]

    def replay(self):
        """Runs the plan on the current input buffers (no host synchronisation)."""
        if self._graph_obj is not None:
            self._graph_obj.replay()
        else:
            self._run_steps()

    def replay_from(self, feed: str, src: torch.Tensor):
        """``input_buffer(feed).copy_(src); replay()`` without the copy when it can (``head_pieces_ok``):
        the head kernel is launched, outside the graph, straight on ``src`` — e.g. the runner's H2D staging
        slot — and the graph of the remaining steps is replayed.  Saves one D2D pass over the raw uint8
        batch (50 MB for ResNet-50 at B=256) per micro-batch."""
        if not self.replay_from_chunks(feed, src, [(0, None)], lambda i: None):  # the whole batch as one piece
            self.input_buffer(feed).copy_(src, non_blocking=True)
            self.replay()

    def replay_from_chunks(self, feed: str, src: torch.Tensor, chunks, wait) -> bool:
        """``replay_from`` for a batch that reaches the device in pieces: the head kernel runs per piece
        ``chunks[i] = (lo, hi)`` right after ``wait(i)`` (the current stream waits for that piece's H2D), so
        the GPU starts on the first records while the rest are still being gathered / copied; then the graph
        of the remaining steps.  False (nothing launched) when the plan has no such head."""
        if not self.head_pieces_ok(feed, src):
            return False
        for i, (lo, hi) in enumerate(chunks):
            wait(i)
            self.launch_head_piece(src, lo, hi)
        self.replay_tail()
        return True

    def head_pieces_ok(self, feed: str, src: torch.Tensor) -> bool:
        """The plan starts with a head kernel on ``feed`` that can run per piece of ``src``
        (``launch_head_piece``), the rest of the plan being one captured graph (``replay_tail``): the pipelined
        runner launches each piece's head right after its H2D, interleaved with the host gather of the next."""
        h = self._head
        buf = self.input_buffer(feed)
        return not (h is None or self._graph_tail is None or h[0] != str(TensorName.parse(feed))
                    or src.shape != buf.shape or src.dtype != buf.dtype or src.device != buf.device
                    or not src.is_contiguous())

    def launch_head_piece(self, src: torch.Tensor, lo: int, hi: int) -> None:
        st = self._head[1]
        st.head(src[lo:hi], _root(st.outputs[0]).buf[lo:hi])

    def replay_tail(self) -> None:
        self._graph_tail.replay()

    def __call__(self, feeds: dict | None = None, copy_outputs: bool = True, cast_outputs: bool = True):
        for k, v in (feeds or {}).items():
            buf = self.input_buffer(k)
            if isinstance(v, StringTensor):
                raise CompileError("STRING feeds are not supported in compiled plans")
            buf.copy_(v, non_blocking=True)
        self.replay()
        outs = []
        for o in self._outputs:
            if isinstance(o, Val):
                b = _view(o)
                if o.qscale is not None:
                    b = F8.from_fp8_bytes(b) * _eff_scale(o)
                elif cast_outputs and b.dtype == torch.bfloat16:
                    b = b.float()
                elif copy_outputs:
                    b = b.clone()
                outs.append(b)
            else:
                outs.append(o)
        return outs

    def output_tensors(self) -> list:
        """The static device tensors holding the fetched values (valid after replay)."""
        return [_view(o) if isinstance(o, Val) else o for o in self._outputs]
