"""The Johnson et al. / CycleGAN generator as a frozen TF GraphDef (random-init weights; no network
access): the generator half of the image-to-image family (fast style transfer, CycleGAN / pix2pix
generators, Magenta's stylisation nets).  In TF 1.x these are built from four things: convs,
``Conv2DBackpropInput``, ``tf.contrib.layers.instance_norm`` and ``MirrorPad`` in front of ``VALID``
convs (no border artefacts), and they return an RGB image.

The graph is the one TF exports:

* uint8 ``images`` through ``Cast → Sub(127.5) → Div(127.5)`` (``normalized``, in [-1, 1]);
* ``MirrorPad(3)``, ``7x7 VALID`` conv to ``base`` channels, instance norm, ``Relu``;
* two ``3x3/2 SAME`` convs to ``2 base`` and ``4 base`` channels, each with instance norm + ``Relu``;
* ``blocks`` residual blocks at ``4 base``: ``MirrorPad(1)``, ``3x3 VALID`` conv, instance norm, ``Relu``,
  ``MirrorPad(1)``, ``3x3 VALID`` conv, instance norm, ``Add`` of the block input;
* two ``3x3/2`` ``Conv2DBackpropInput`` + ``BiasAdd`` + instance norm + ``Relu`` back to ``base``;
* ``MirrorPad(3)``, ``7x7 VALID`` conv to 3 channels + ``BiasAdd`` (``rgb``);
* ``Tanh → Mul(127.5) → Add(127.5) → ClipByValue(0, 255) → Cast(UINT8)`` (``stylized``).

Instance norm is ``GraphBuilder.instance_norm``: the ten nodes of ``nn.moments(x, [1, 2],
keep_dims=True)`` + ``nn.batch_normalization``.  The convs in front of a norm have no bias (the norm
removes it), as in the published generators.

The compiler lowers all of it (``graph/generator_lowering.py``).  The step kinds of the plan, for any
``base`` that is a multiple of 8:

    preprocess 1, pad 2 + 2 blocks, conv 4 + 2 blocks, instnorm 5 + 2 blocks, elementwise blocks,
    deconv 2, image_out 1

(``expected_step_kinds``): each norm with its ``Relu`` is one ``instnorm`` step, each block's ``Add`` one
``elementwise`` step, and the five output nodes behind ``rgb`` one ``image_out`` step that stores bytes.

Tensor names: ``images`` (uint8 [N, H, W, 3]), ``normalized``, ``rgb`` ([N, H, W, 3] pre-activation),
``stylized`` (uint8 [N, H, W, 3]); ``image_hw`` must be a multiple of 4.
"""
from __future__ import annotations

import numpy as np

from ...graph.builder import GraphBuilder
from ...proto.messages import GraphDef
from .image_classifier import ImageClassifierModel
from .resnet import _Init


def expected_step_kinds(blocks: int = 5) -> dict:
    """Step kinds of the strict plan of ``style_transfer_graph_def(blocks=blocks)``."""
    return {"preprocess": 1, "pad": 2 + 2 * blocks, "conv": 4 + 2 * blocks, "instnorm": 5 + 2 * blocks,
            "elementwise": blocks, "deconv": 2, "image_out": 1}


def _instance_norm(gb: GraphBuilder, init: _Init, x: str, c: int, name: str, eps: float) -> str:
    g = gb.constant(f"{name}/gamma", init.rng.uniform(0.8, 1.2, c).astype(np.float32))
    b = gb.constant(f"{name}/beta", (init.rng.standard_normal(c) * 0.1).astype(np.float32))
    return gb.instance_norm(x, g, b, eps, name=name)


def style_transfer_graph_def(base: int = 32, blocks: int = 5, image_hw: tuple[int, int] = (256, 256),
                             pad_mode: str = "REFLECT", seed: int = 0, eps: float = 1e-5,
                             out_scale: float = 1.0) -> GraphDef:
    """``out_scale`` multiplies the He-style init of the last conv (the spread of ``rgb``, so how
    much of the image ``Tanh`` saturates)."""
    H, W = image_hw
    if base < 8 or base % 8 or blocks < 0 or H % 4 or W % 4 or min(H, W) < 8:
        raise ValueError(f"style_transfer: base {base} must be a multiple of 8 and image_hw {tuple(image_hw)} a "
                         "multiple of 4 (at least 8)")
    gb = GraphBuilder()
    init = _Init(seed)
    sp = lambda p: [[0, 0], [p, p], [p, p], [0, 0]]  # noqa: E731
    images = gb.placeholder("images", "UINT8", [None, H, W, 3])
    x = gb.cast(images, "FLOAT", name="Cast")
    x = gb.sub(x, gb.constant("mean", np.float32(127.5)), name="Sub")
    x = gb.div(x, gb.constant("std", np.float32(127.5)), name="normalized")

    def conv_in_relu(x, k, cin, cout, stride, padding, name):
        with gb.name_scope(name):
            y = gb.conv2d(x, gb.constant("weights", init.conv(k, k, cin, cout)), (stride, stride), padding, name="Conv2D")
            y = _instance_norm(gb, init, y, cout, "InstanceNorm", eps)
            return gb.relu(y, name="Relu")

    with gb.name_scope("encode"):
        x = gb.mirror_pad(x, sp(3), pad_mode, name="MirrorPad")
        x = conv_in_relu(x, 7, 3, base, 1, "VALID", "conv1")
        x = conv_in_relu(x, 3, base, 2 * base, 2, "SAME", "conv2")
        x = conv_in_relu(x, 3, 2 * base, 4 * base, 2, "SAME", "conv3")
    c = 4 * base
    for i in range(blocks):
        with gb.name_scope(f"residual{i}"):
            y = gb.mirror_pad(x, sp(1), pad_mode, name="MirrorPad")
            y = conv_in_relu(y, 3, c, c, 1, "VALID", "conv1")
            y = gb.mirror_pad(y, sp(1), pad_mode, name="MirrorPad_1")
            with gb.name_scope("conv2"):
                y = gb.conv2d(y, gb.constant("weights", init.conv(3, 3, c, c)), (1, 1), "VALID", name="Conv2D")
                y = _instance_norm(gb, init, y, c, "InstanceNorm", eps)
            x = gb.add(x, y, name="add")
    hw = (H // 4, W // 4)
    for i, cout in enumerate((2 * base, base)):
        with gb.name_scope(f"decode/deconv{i + 1}"):
            hw = (hw[0] * 2, hw[1] * 2)
            w = (init.rng.standard_normal((3, 3, cout, c)) * np.sqrt(2.0 * 4 / (9 * c))).astype(np.float32)
            y = gb.conv2d_transpose(x, gb.constant("weights", w), hw, (2, 2), "SAME", name="conv2d_transpose")
            y = gb.bias_add(y, gb.constant("biases", (init.rng.standard_normal(cout) * 0.05).astype(np.float32)),
                            name="BiasAdd")
            y = _instance_norm(gb, init, y, cout, "InstanceNorm", eps)
            x = gb.relu(y, name="Relu")
            c = cout
    with gb.name_scope("decode"):
        x = gb.mirror_pad(x, sp(3), pad_mode, name="MirrorPad")
        y = gb.conv2d(x, gb.constant("conv_out/weights", init.conv(7, 7, c, 3) * np.float32(out_scale)), (1, 1), "VALID",
                      name="conv_out/Conv2D")
        b = gb.constant("conv_out/biases", (init.rng.standard_normal(3) * 0.1).astype(np.float32))
    rgb = gb.bias_add(y, b, name="rgb")
    y = gb.tanh(rgb, name="Tanh")
    y = gb.mul(y, gb.constant("scale", np.float32(127.5)), name="Mul")
    y = gb.add(y, gb.constant("offset", np.float32(127.5)), name="Add")
    y = gb.clip_by_value(y, 0.0, 255.0, name="clip_by_value")
    gb.cast(y, "UINT8", name="stylized")
    return gb.build_graph_def()


def export_style_transfer_saved_model(export_dir: str, **graph_args) -> str:
    """The generator as a TF 1.x SavedModel with its weights as variables (signature
    ``serving_default``: ``images`` -> ``stylized``); ``graph_args`` are those of
    ``style_transfer_graph_def``."""
    from ...proto.messages import SignatureDef
    from ..export import graph_def_to_saved_model, tensor_info

    H, W = graph_args.get("image_hw", (256, 256))
    sig = SignatureDef(inputs={"images": tensor_info("images:0", "UINT8", [-1, H, W, 3])},
                       outputs={"stylized": tensor_info("stylized:0", "UINT8", [-1, H, W, 3])},
                       method_name="tensorflow/serving/predict")
    return graph_def_to_saved_model(export_dir, style_transfer_graph_def(**graph_args), {"serving_default": sig})


class StyleTransferModel(ImageClassifierModel):
    """The style-transfer generator (random-init frozen graph): generator networks.  The plan is
    strict: every ``MirrorPad`` one ``pad`` step, every instance norm with its ``Relu`` one
    ``instnorm`` step (``kernels/instnorm.hip``), the up-convs on the transposed-conv kernel and the
    ``Tanh → Mul → Add → ClipByValue → Cast`` output stage one ``image_out`` step that stores bytes
    (``kernels/pad.hip``).  Results are ``[H, W, 3]`` uint8 images, one per record, from ``stylize``
    and from the batched ``submit`` / ``poll`` / ``drain`` path alike."""

    def __init__(self, image_hw=(256, 256), buckets=(8, 32), seed: int = 0, device=None, base: int = 32,
                 blocks: int = 5, pad_mode: str = "REFLECT", fetches=("stylized:0",), **kw):
        self.seed = seed
        self.base_channels = base
        self.blocks = blocks
        self.pad_mode = pad_mode
        ImageClassifierModel.__init__(self, self._make_graph, image_hw, buckets, 1, device=device, fetches=fetches, **kw)

    def _make_graph(self) -> GraphDef:
        return style_transfer_graph_def(base=self.base_channels, blocks=self.blocks, image_hw=self.image_hw,
                                        pad_mode=self.pad_mode, seed=self.seed)

    def stylize(self, images) -> list[np.ndarray]:
        """One ``[H, W, 3]`` uint8 image per input image (synchronous)."""
        return list(self._run_sync(images)[0].numpy())

    def _sync_results(self, records):
        return self.stylize(records)

    def _results(self, br):
        return list(br.outputs[0][: br.n].numpy()), br.tags, br.latencies
