"""The plan vocabulary shared by the graph compiler and its lowering mixins: symbolic
values (``Val``), launch steps (``Step``), the batch-slice chain record (``Chain``),
``CompileError`` and the helpers that map a value to its physical buffer.  A leaf module: it
imports nothing from the compiler."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Callable

import numpy as np
import torch


def _cfg():
    from ..config import current

    return current()


class CompileError(RuntimeError):
    pass


@dataclass
class Val:
    """A symbolic value in the plan."""

    shape: tuple
    dtype: torch.dtype
    const: Any = None          # folded constant (host tensor / StringTensor)
    buf: torch.Tensor | None = None
    phys_c: int | None = None  # physical channel count when padded (stem input)
    alias_of: "Val | None" = None
    last_use: int = -1
    concat_slot: tuple | None = None  # (target Val, channel offset) for concat-by-stride-write
    concat_children: list | None = None  # on that target: the branch Vals written into its slices
    qscale: float | None = None  # fp8 e4m3 storage (uint8 buffer) with this per-tensor scale
    # token-packed plans (``token_capacity``): "packed" = one row per real token (the plan's
    # token capacity T rows), "cls" = one row per sequence (its first token); ``shape`` is
    # then the physical [rows, D] and ``lshape`` the graph's logical shape ([B*S, D] or
    # [B, S, D]) that Reshape / StridedSlice reason about
    rows: str | None = None
    lshape: tuple | None = None
    # physical buffer shape when it is not ``shape`` / ``phys_c``: the preprocess output
    # (channels padded to 8, or space-to-depth packed for the stem), a decimated block-tail
    # output, a GEMM output with padded columns
    buf_shape: tuple | None = None
    # the fused preprocess kernel's output only: ``pre_cfg`` its mutable launch switches
    # ({"s2d": bool}, set by the stem conv that reads it), ``pre_chain`` the names of the
    # graph nodes it absorbed, ``pre_params`` what a stem conv needs to absorb the kernel
    pre_cfg: dict | None = None
    pre_chain: set | None = None
    pre_params: dict | None = None
    # detection heads (``detection_lowering.py``): values without a step or a buffer that only
    # a ``CombinedNonMaxSuppression`` reads.  ``decode_of`` = (encodings Val, anchors fp32
    # [N, 4], four reciprocal scales): the boxes of a matched ``decode_boxes`` subgraph, decoded
    # inside the ``nms`` step.  ``slice_of`` = (source Val, first column): a last-axis slice of
    # the scores, read in place through a pitch and a class offset.
    decode_of: tuple | None = None
    slice_of: tuple | None = None
    # recurrent layers (``recurrent_lowering.py``): the time-major ``[T, B, I]`` result of an
    # absorbed ``Transpose`` that only a ``BlockLSTM`` reads, without a step or a buffer;
    # ``tm_of`` is the batch-major ``[B, T, I]`` source Val, read in place through strides
    tm_of: "Val | None" = None
    # dense prediction heads: a ``ResizeBilinear`` result without a step or a buffer, read only by an
    # ``ArgMax`` that interpolates on the fly: (source Val, align_corners, half_pixel_centers)
    resize_of: tuple | None = None
    # video models (``conv3d_lowering.py``): the float value of an absorbed ``Cast → Mul | RealDiv`` of a
    # uint8 clip feed, without a step or a buffer, read only by one ``Conv3D``: (feed Val, scalar factor)
    u8_of: tuple | None = None

    @property
    def is_const(self):
        return self.const is not None


@dataclass
class Step:
    name: str
    kind: str
    fn: Callable[[], None]
    inputs: list = field(default_factory=list)
    outputs: list = field(default_factory=list)
    meta: dict = field(default_factory=dict)
    # launches this step reading ``src`` and writing ``dst`` instead of its bound buffers: the plan's head only
    head: Callable[[torch.Tensor, torch.Tensor], None] | None = None


@dataclass
class Chain:
    """The batch-slice chain of a plan (``PlanMemory._find_chain``): steps ``range`` run once
    per slice of ``batch`` images, ``parts`` times over the ``n`` images of the batch."""

    range: tuple    # (first step, end step)
    batch: int      # images per slice
    parts: int      # number of slices; a short last one when ``batch`` does not divide ``n`` (dynamic batch buckets)
    n: int          # images in the batch
    vals: list      # every value (alias Vals included) the chain's steps read or write
    touched: set    # ids of the roots of ``vals``: they live across the whole chain
    internal: dict  # id -> root Val made and consumed inside the chain: one slice-sized buffer
    # filled at bind time, rebound per slice by ``PlanRunner._run_chain_slice``:
    external: list = field(default_factory=list)  # the values on full-batch buffers, sliced ``[lo:hi]``
    bound: list = field(default_factory=list)     # the bound internal values, narrowed for a short last slice


def _buf_shape(r: Val) -> tuple:
    """Physical buffer shape of a value (channel-padded / space-to-depth stem inputs,
    decimated block-tail outputs)."""
    if r.buf_shape:
        return tuple(r.buf_shape)
    if r.phys_c:
        return (*r.shape[:-1], r.phys_c)
    return tuple(r.shape)


def _nbytes(shape, dtype) -> int:
    return int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()


def _root(v: Val) -> Val:
    while v.alias_of is not None:
        v = v.alias_of
    return v


def _view(v: Val) -> torch.Tensor:
    r = _root(v)
    if r.concat_slot is not None and r.buf is None:
        tgt, off = r.concat_slot
        return tgt.buf[..., off:off + r.shape[-1]]
    b = r.buf
    if r.phys_c and b.shape[-1] != r.shape[-1] and v is r:
        if tuple(b.shape[:-1]) == tuple(r.shape[:-1]):
            return b[..., :r.shape[-1]]  # channel-padded buffer: the logical columns
        return b  # space-to-depth packed stem input
    if v is not r:
        return b.reshape(v.shape)
    return b


def _target(v: Val) -> torch.Tensor:
    r = _root(v)
    if r.concat_slot is not None:
        return r.concat_slot[0].buf
    return r.buf


def _eff_scale(v: Val) -> float | None:
    """Storage scale of an fp8 value: a concat branch is stored with its buffer's scale."""
    r = _root(v)
    if r.concat_slot is not None and r.concat_slot[0].qscale is not None:
        return r.concat_slot[0].qscale
    return r.qscale


def _coff(v: Val) -> int:
    r = _root(v)
    return r.concat_slot[1] if r.concat_slot is not None else 0


def _host(t):
    if isinstance(t, torch.Tensor):
        return t.detach().to("cpu")
    return t
