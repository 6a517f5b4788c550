"""Keyword spotter (TF's speech_commands ``conv`` architecture) as a frozen TF GraphDef
(random-init weights; no network access).

The model that runs over microphone or telephony streams: one-second clips go through the MFCC
front end and a small convolutional classifier.

    clips [B, S] (FLOAT, or INT16 -> Cast -> Mul 1/32768) -> Transpose([1, 0])
    -> AudioSpectrogram(480, 160, squared) -> Mfcc(16000, C = 40, D = 40, 20-4000 Hz)
    -> Reshape [B, 98, 40, 1] -> Conv2D 20x8x1x64 SAME + bias + ReLU -> MaxPool 2x2/2 SAME
    -> Conv2D 10x4x64x64 SAME + bias + ReLU -> Reshape [B, 62720] -> MatMul + bias (12 classes)
    -> Softmax -> TopKV2

The compiler lowers everything in front of the first convolution to one ``mfcc`` step on
``kernels/audio.hip`` that reads the raw PCM and writes the conv's channel-padded input
(``graph/audio_lowering.py``), so a strict plan holds ``mfcc``, two ``conv`` steps, the pool,
the head GEMM and the softmax / top-k step.

Tensor names: ``clips`` ([N, S] float or int16), ``fingerprint`` (the reshaped MFCCs),
``logits``, ``probs``, ``top_k`` (``top_k:0`` values, ``top_k:1`` indices).
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from ...graph.builder import GraphBuilder
from ...graph.compiler import CompiledFunction
from ...graph.ops_nn import decode_wav, spectrogram_frames
from ...proto.messages import GraphDef
from ...runtime.model_functions import BatchedGpuModel
from ...types.tensor_value import TensorValue
from ..core import GenericModel, GraphDefGraphLoader, GraphLoader

SPEECH_COMMANDS_LABELS = ("_silence_", "_unknown_", "yes", "no", "up", "down", "left", "right", "on", "off", "stop", "go")


def speech_commands_graph_def(clip_samples: int = 16000, sample_rate: int = 16000, window_size: int = 480,
                              stride: int = 160, channels: int = 40, dct_count: int = 40, lower: float = 20.0,
                              upper: float = 4000.0, conv1=(20, 8, 64), conv2=(10, 4, 64), num_classes: int = 12,
                              pcm: str = "float32", batch: int | None = None, top_k: int = 3,
                              seed: int = 0) -> GraphDef:
    """``pcm = "int16"`` feeds raw PCM and keeps DecodeWav's scaling (``/ 32768``) in the graph.
    ``batch`` fixes the leading dimension of the two reshapes (None: ``-1``).  ``conv1`` /
    ``conv2`` are ``(height over frames, width over coefficients, filters)``."""
    if pcm not in ("float32", "int16"):
        raise ValueError(f"speech_commands_graph_def: pcm is float32 or int16, not {pcm!r}")
    frames = spectrogram_frames(clip_samples, window_size, stride)
    if frames < 1:
        raise ValueError(f"speech_commands_graph_def: {clip_samples} samples hold no window of {window_size}")
    rng = np.random.default_rng(seed)
    gb = GraphBuilder()
    b = -1 if batch is None else int(batch)
    x = gb.placeholder("clips", "INT16" if pcm == "int16" else "FLOAT", [batch, clip_samples])
    if pcm == "int16":
        x = gb.cast(x, "FLOAT", name="pcm_float")
        x = gb.mul(x, gb.constant("pcm_scale", np.float32(1.0 / 32768.0)), name="pcm_scaled")
    x = gb.transpose(x, [1, 0], name="samples_major")
    x = gb.audio_spectrogram(x, window_size, stride, magnitude_squared=True, name="spectrogram")
    x = gb.mfcc(x, sample_rate, upper, lower, channels, dct_count, name="mfcc")
    x = gb.reshape(x, [b, frames, dct_count, 1], name="fingerprint")

    def conv(x, name, kh, kw, cin, cout):
        w = gb.constant(f"{name}/kernel", (rng.standard_normal((kh, kw, cin, cout)) * np.sqrt(2.0 / (kh * kw * cin)))
                        .astype(np.float32))
        bias = gb.constant(f"{name}/bias", rng.uniform(-0.05, 0.05, (cout,)).astype(np.float32))
        return gb.relu(gb.bias_add(gb.conv2d(x, w, padding="SAME", name=f"{name}/Conv2D"), bias, name=f"{name}/BiasAdd"),
                       name=f"{name}/Relu")

    x = conv(x, "conv1", conv1[0], conv1[1], 1, conv1[2])
    x = gb.max_pool(x, (2, 2), (2, 2), padding="SAME", name="pool1")
    x = conv(x, "conv2", conv2[0], conv2[1], conv1[2], conv2[2])
    flat = -(-frames // 2) * -(-dct_count // 2) * conv2[2]
    x = gb.reshape(x, [b, flat], name="flatten")
    lim = float(np.sqrt(6.0 / (flat + num_classes)))
    wo = gb.constant("dense/kernel", rng.uniform(-lim, lim, (flat, num_classes)).astype(np.float32))
    bo = gb.constant("dense/bias", rng.uniform(-0.1, 0.1, (num_classes,)).astype(np.float32))
    logits = gb.bias_add(gb.matmul(x, wo, name="dense/MatMul"), bo, name="logits")
    probs = gb.softmax(logits, name="probs")
    gb.top_k(probs, min(top_k, num_classes), name="top_k")
    return gb.build_graph_def()


class KeywordSpotterModel(GenericModel, BatchedGpuModel):
    """Audio clips -> top-k ``(probability, label)`` pairs.  A record is a float32 (``[-1, 1)``)
    or int16 array of ``clip_samples`` samples, or the bytes of a mono 16-bit WAV file (parsed
    on the host, cut or zero-padded to the clip length).  With ``pcm = "int16"`` (the default)
    the plan's feed is raw PCM, half the host-to-device bytes of float32.  On a GPU subtask
    ``open()`` compiles one strict plan per batch bucket and compute lane and serves them through
    the pipelined runner; on a host subtask the graph runs in the interpreter."""

    _TRANSIENT = ("_graph", "_session", "_plans", "_runner", "_arena")

    def __init__(self, clip_samples: int = 16000, sample_rate: int = 16000, window_size: int = 480, stride: int = 160,
                 channels: int = 40, dct_count: int = 40, lower: float = 20.0, upper: float = 4000.0,
                 conv1=(20, 8, 64), conv2=(10, 4, 64), num_classes: int = 12, pcm: str = "int16",
                 buckets: Sequence[int] = (64, 256), top_k: int = 3, labels: Sequence[str] | None = SPEECH_COMMANDS_LABELS,
                 seed: int = 0, device=None, depth: int = 3, use_graph: bool = True, lanes: int = 2):
        super().__init__(device)
        self.cfg = dict(clip_samples=clip_samples, sample_rate=sample_rate, window_size=window_size, stride=stride,
                        channels=channels, dct_count=dct_count, lower=lower, upper=upper, conv1=tuple(conv1),
                        conv2=tuple(conv2), num_classes=num_classes, pcm=pcm, seed=seed)
        self.clip_samples, self.sample_rate, self.pcm = clip_samples, sample_rate, pcm
        self.num_classes = num_classes
        self.buckets = tuple(sorted(buckets))
        self.top_k = min(top_k, num_classes)
        self.labels = list(labels) if labels is not None else None
        self.depth = depth
        self.use_graph = use_graph
        self.lanes = max(1, int(lanes))
        self.feed = "clips:0"
        self.fetches = ["top_k:0", "top_k:1"]
        self._np_dtype = np.int16 if pcm == "int16" else np.float32
        self._plans: dict | None = None
        self._runner = None
        self._arena = None

    def graph_def(self) -> GraphDef:
        return speech_commands_graph_def(top_k=self.top_k, **self.cfg)

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
            dt = "INT16" if self.pcm == "int16" else "FLOAT"
            lanes = [{b: CompiledFunction(self._graph, {self.feed: ((b, self.clip_samples), dt)}, self.fetches, dev,
                                          use_graph=self.use_graph, strict=True, arena=arena)
                      for b in sorted(self.buckets, reverse=True)} for arena in self._arena]
            self._plans = lanes[0]
            self._runner = PipelinedGpuRunner(lanes, self.feed, lambda p: p.output_tensors(), (self.clip_samples,),
                                              torch.int16 if self.pcm == "int16" else torch.float32, depth=self.depth,
                                              device=dev)

    def close(self) -> None:
        if self._runner is not None:
            self._runner.drain()
        self._runner = None
        self._plans = None
        self._arena = None
        super().close()

    def plan_summary(self) -> dict | None:
        return next(iter(self._plans.values())).summary() if self._plans else None

    def label_of(self, i: int) -> str:
        return self.labels[i] if self.labels and i < len(self.labels) else f"class_{i}"

    # ------------------------------------------------------------------ records
    def _as_array(self, r) -> np.ndarray:
        """A record as the feed's sample type: float32 in ``[-1, 1)`` or int16 PCM (``float * 32768``,
        rounded and clipped, and ``int16 / 32768`` the other way)."""
        if isinstance(r, (bytes, bytearray, memoryview)):
            audio, rate = decode_wav(bytes(r), desired_channels=1, desired_samples=self.clip_samples)
            if rate != self.sample_rate:
                raise ValueError(f"{type(self).__name__}: WAV sample rate {rate}, the model takes {self.sample_rate}")
            r = np.rint(audio.numpy()[:, 0] * 32768.0).astype(np.int16)  # exact: decode_wav divided by 32768
        elif isinstance(r, TensorValue):
            r = r.to_numpy()
        elif isinstance(r, torch.Tensor):
            r = r.cpu().numpy()
        a = np.asarray(r)
        if a.shape != (self.clip_samples,):
            raise ValueError(f"{type(self).__name__}: record {a.shape} is not ({self.clip_samples},)")
        if a.dtype == np.int16:
            return a if self.pcm == "int16" else a.astype(np.float32) / np.float32(32768.0)
        if not np.issubdtype(a.dtype, np.floating):
            raise TypeError(f"{type(self).__name__}: records are float32, int16 or WAV bytes, not {a.dtype}")
        a = a.astype(np.float32)
        return np.clip(np.rint(a * 32768.0), -32768, 32767).astype(np.int16) if self.pcm == "int16" else a

    def _pairs(self, vals, idxs) -> list:
        return [[(float(v), self.label_of(int(i))) for v, i in zip(vr, ir)] for vr, ir in zip(vals.tolist(), idxs.tolist())]

    def _results(self, br):
        return self._pairs(br.outputs[0][: br.n], br.outputs[1][: br.n]), br.tags, br.latencies

    # ------------------------------------------------------------------ synchronous API
    def spot(self, clips) -> list[list[tuple[float, str]]]:
        """Top-k ``(probability, label)`` per clip, best first."""
        arrs = [self._as_array(r) for r in clips]
        out = []
        cap = self.buckets[-1]
        for s in range(0, len(arrs), cap):
            chunk = np.stack(arrs[s:s + cap])
            n = len(chunk)
            if self._plans is not None:
                b = next(bk for bk in self.buckets if bk >= n)
                buf = np.zeros((b, self.clip_samples), dtype=self._np_dtype)
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

            return [(self.spot(records), tags, time.perf_counter() - np.asarray(ingest_ts))]
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


def export_keyword_spotter_saved_model(export_dir: str, pcm: str = "float32", top_k: int = 3, **graph_args) -> str:
    """The spotter as a TF 1.x SavedModel with its weights as variables (signature
    ``serving_default``: ``clips`` -> ``probabilities``, ``scores``, ``classes``); ``graph_args``
    are those of ``speech_commands_graph_def``."""
    from ...proto.messages import SignatureDef
    from ..export import graph_def_to_saved_model, tensor_info

    num_classes = graph_args.get("num_classes", 12)
    samples = graph_args.get("clip_samples", 16000)
    top_k = min(top_k, num_classes)
    gd = speech_commands_graph_def(pcm=pcm, top_k=top_k, **graph_args)
    sig = SignatureDef(inputs={"clips": tensor_info("clips:0", "INT16" if pcm == "int16" else "FLOAT", [-1, samples])},
                       outputs={"probabilities": tensor_info("probs:0", "FLOAT", [-1, num_classes]),
                                "scores": tensor_info("top_k:0", "FLOAT", [-1, top_k]),
                                "classes": tensor_info("top_k:1", "INT32", [-1, top_k])},
                       method_name="tensorflow/serving/predict")
    return graph_def_to_saved_model(export_dir, gd, {"serving_default": sig})
