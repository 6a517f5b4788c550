"""Lowering of the audio front end (a mixin of ``CompiledFunction``): ``AudioSpectrogram`` and
``Mfcc`` to one step on ``kernels/audio.hip``, with the layout and scaling ops around them
absorbed.

**The pair.**  ``AudioSpectrogram(magnitude_squared=True) → Mfcc`` becomes one ``mfcc`` step
(PCM in, coefficients out, nothing in memory in between) when

* only the ``Mfcc`` reads the spectrogram, and the spectrogram is not fetched;
* ``sample_rate`` is a constant;
* the input is a 2-D ``[samples, clips]`` feed or activation, fp32 (or int16, below);
* the shapes pass ``K.mfcc_eligible`` (FFT length 256..2048, ``D <= C <= 128``, every mel
  channel non-empty).

The result is bf16 ``[clips, frames, D]`` (fp32 when the ``Mfcc`` is fetched).

**Absorbed** (no step, no buffer), as the recurrent lowering absorbs its transposes:

* ``Transpose(perm=[1, 0])`` in front, read by the op alone: batched records arrive ``[B, S]``
  and the op wants ``[S, B]``; the step reads through swapped strides.
* ``Cast(INT16 → FLOAT) → [Mul | RealDiv by a scalar constant]`` in front of that, each read by
  the next alone: DecodeWav's scaling when the stream carries raw PCM.  The kernel reads the
  int16 samples and multiplies by the scale (``1 / c`` for a division), which halves the H2D copy.
* ``Reshape`` of the coefficients to ``[B, F, D, 1]`` read by one ``Conv2D`` alone: the step
  writes the conv's channel-padded input (``phys_c = 8``, channels 1..7 zero) with one 16-byte
  store per coefficient, so the conv lowering finds it padded and emits no ``pad_cin`` copy.

**A lone ``AudioSpectrogram``** (fetched, read by something else, or not squared) becomes a
``spectrogram`` step with an fp32 ``[clips, frames, N/2 + 1]`` value.

**What stays glue** (a ``CompileError`` under ``strict``): an ``Mfcc`` of anything but such a
spectrogram, a fed ``sample_rate`` (the spectrogram still lowers; the ``Mfcc`` does not, and
since the glue path sizes its outputs by a dry run on zeros, where a zero sample rate is no
filter bank, such a graph has no non-strict plan either and runs on the interpreter), shapes
outside the envelope, a transpose with a second reader.

The pattern is matched forward from its first node (the ``Cast``, the ``Transpose`` or the
``AudioSpectrogram``), where the source value is already known and everything else is a
constant; the nodes behind it are marked fused.  In an fp8 plan these steps run as they do in a
bf16 plan, like ``dwconv`` and ``resize``.
"""
from __future__ import annotations

import torch

from ..ops import kernels as K
from ..types.dtypes import DataType
from .plan import _view


class AudioLowering:
    """Mixin of ``CompiledFunction`` (uses its graph, ``cons``, ``vals``, ``_fetched`` and emitters,
    and the graph helper ``_const_of`` of the ``TransformerLowering`` mixin)."""

    def _sole_reader(self, node, op=None):
        """The only reader of ``node`` (not fetched, read once), of type ``op`` if given."""
        nxt = self._single_consumer(node.name)
        if nxt is None or (op is not None and nxt.op not in op):
            return None
        return nxt if [s[0] for s in nxt.inputs].count(node.name) == 1 else None

    def _scalar_const(self, src):
        c = self._const_of(src)
        if not isinstance(c, torch.Tensor) or c.numel() != 1 or not c.dtype.is_floating_point:
            return None
        return float(c.reshape(-1)[0])

    def _lower_audio_from(self, node) -> bool:
        """Tries the audio pattern that starts at ``node``; False: not ours, nothing emitted."""
        src = self.vals.get(node.inputs[0])  # a computed value or a feed: constants were folded before
        if src is None or src.is_const or len(src.shape) != 2 or src.rows is not None or src.phys_c \
                or src.qscale is not None or src.tm_of is not None:
            return False
        absorbed, scale, cur = [], 1.0, node
        if cur.op == "Cast":
            if src.dtype != torch.int16 or DataType.of(cur.attr("DstT")).torch != torch.float32:
                return False
            absorbed.append(cur)
            cur = self._sole_reader(cur, ("Mul", "RealDiv", "Transpose", "AudioSpectrogram"))
            if cur is not None and cur.op in ("Mul", "RealDiv"):
                ci = 1 if cur.inputs[0][0] == absorbed[-1].name else 0
                c = self._scalar_const(cur.inputs[ci])
                if c is None or (cur.op == "RealDiv" and (ci != 1 or c == 0.0)):
                    return False
                scale = c if cur.op == "Mul" else 1.0 / c
                absorbed.append(cur)
                cur = self._sole_reader(cur, ("Transpose", "AudioSpectrogram"))
            if cur is None:
                return False
        elif src.dtype != torch.float32:
            return False
        transposed = False
        if cur.op == "Transpose":
            perm = self._const_of(cur.inputs[1]) if len(cur.inputs) == 2 else None
            if perm is None or [int(v) for v in perm.reshape(-1).tolist()] != [1, 0]:
                return False
            transposed = True
            absorbed.append(cur)
            cur = self._sole_reader(cur, ("AudioSpectrogram",))
            if cur is None:
                return False
        if cur.op != "AudioSpectrogram" or cur.inputs[0][0] != (absorbed[-1].name if absorbed else node.inputs[0][0]):
            return False
        if not self._emit_audio(cur, src, transposed, scale):
            return False
        for n in absorbed + [cur]:
            if n is not node:
                self._fused.add(n.name)
        return True

    def _emit_audio(self, spec, src, transposed: bool, scale: float) -> bool:
        B, S = src.shape if transposed else src.shape[::-1]
        window, stride = int(spec.attr("window_size", 0)), int(spec.attr("stride", 0))
        squared = bool(spec.attr("magnitude_squared", False))
        if not K.mfcc_eligible(S, window, stride):
            return False
        F_, N = K.audio_frames(S, window, stride), K.audio_fft_length(window)
        meta = {"impl": "audio_frontend", "input": "int16" if src.dtype == torch.int16 else "fp32", "scale": scale,
                "layout": "clip_major" if transposed else "sample_major", "S": S, "B": B, "F": F_, "window": window,
                "stride": stride, "fft": N}

        def intern(tables):
            dev = {k: self._dev(v) if isinstance(v, torch.Tensor) else v for k, v in tables.items()}
            self.params += [v for v in dev.values() if isinstance(v, torch.Tensor)]
            return dev

        mf = self._sole_reader(spec, ("Mfcc",)) if squared else None
        rate = self._const_of(mf.inputs[1]) if mf is not None and mf.inputs[0][0] == spec.name else None
        if rate is not None and isinstance(rate, torch.Tensor) and rate.numel() == 1:
            rate = int(rate.reshape(-1)[0])
            lo, hi = float(mf.attr("lower_frequency_limit", 20.0)), float(mf.attr("upper_frequency_limit", 4000.0))
            C, D = int(mf.attr("filterbank_channel_count", 40)), int(mf.attr("dct_coefficient_count", 13))
            if not K.mfcc_eligible(S, window, stride, C, D, rate, lo, hi):
                return False  # the pair stays glue: an Mfcc of a lowered spectrogram would too
            tables = intern(K.mfcc_tables(window, rate, lo, hi, C, D))
            rs = self._sole_reader(mf, ("Reshape",))
            conv = self._sole_reader(rs, ("Conv2D",)) if rs is not None else None
            shape = self._const_of(rs.inputs[1]) if conv is not None and conv.inputs[0][0] == rs.name else None
            pad8 = False
            if shape is not None:
                shape = [int(v) for v in shape.reshape(-1).tolist()]
                if shape.count(-1) == 1:
                    rest = -1
                    for v in shape:
                        rest *= v
                    shape[shape.index(-1)] = B * F_ * D // max(rest, 1)
                pad8 = shape == [B, F_, D, 1]
            if pad8:
                out = self._new((B, F_, D, 1), phys_c=8)
                self.vals[(rs.name, 0)] = out
                self._fused.update((mf.name, rs.name))
            else:
                out = self._new((B, F_, D), torch.float32 if self._fetched(mf.name) else torch.bfloat16)
                self.vals[(mf.name, 0)] = out
                self._fused.add(mf.name)

            def run(src=src, out=out, tables=tables):
                x = _view(src)
                K.audio_mfcc(x.t() if transposed else x, tables, stride, scale, out=out.buf, out_dtype=out.dtype,
                             pad8=pad8)

            self._emit(mf.name, "mfcc", run, [src], [out],
                       {**meta, "C": C, "D": D, "sample_rate": rate,
                        "out": "padded8" if pad8 else ("fp32" if out.dtype == torch.float32 else "bf16")})
            return True
        tables = intern(K.mfcc_tables(window))
        out = self._new((B, F_, N // 2 + 1), torch.float32)

        def run(src=src, out=out, tables=tables):
            x = _view(src)
            K.audio_spectrogram(x.t() if transposed else x, tables, stride, squared, scale, out=out.buf)

        self._emit(spec.name, "spectrogram", run, [src], [out], {**meta, "squared": squared})
        self.vals[(spec.name, 0)] = out
        return True
