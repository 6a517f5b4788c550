"""U-Net as a frozen TF GraphDef (random-init weights; no network access): the image-to-image
family (segmentation, autoencoders, super-resolution, generators), whose learned upsample is
``Conv2DBackpropInput`` (``tf.nn.conv2d_transpose``, Keras ``Conv2DTranspose``).

The graph is the one TF exports for the classic architecture, behind the image front end of
``deeplab.py`` (``Cast → ResizeBilinear(crop) → Sub → Div``):

* encoder: per level two ``3x3 Conv2D + FusedBatchNorm + Relu`` (``base * 2^level`` channels),
  then ``MaxPool 2x2/2``;
* a bottleneck of two such convs at ``base * 2^depth`` channels;
* decoder: per level ``Conv2DBackpropInput 2x2/2 + BiasAdd`` halving the channels,
  ``ConcatV2([skip, up])``, two 3x3 convs;
* the head: a 1x1 conv to ``num_classes`` + ``BiasAdd`` (``logits``), ``ArgMax`` over the
  channels (``labels``) and a ``Cast`` to uint8 (``label_map``).

The compiler lowers all of it: each up-conv chain to one ``deconv`` step
(``kernels/deconv.hip``), the concat of a skip (which the pool reads too) and an up-conv as one
copy step, ``labels → label_map`` to one ArgMax launch that stores bytes.

Tensor names: ``images`` (uint8 [N,H,W,3]), ``normalized``, ``logits`` ([N,h,w,classes]),
``labels`` (int32 [N,h,w]), ``label_map`` (uint8 [N,h,w]); ``crop_hw`` must be a multiple of
``2^depth``.
"""
from __future__ import annotations

import numpy as np

from ...graph.builder import GraphBuilder
from ...proto.messages import GraphDef
from .deeplab import _conv_bn_relu
from .resnet import IMAGENET_MEAN, IMAGENET_STD, _Init


def unet_graph_def(base: int = 64, depth: int = 4, num_classes: int = 21, image_hw: tuple[int, int] | None = None,
                   crop_hw: tuple[int, int] = (256, 256), seed: int = 0, logits_scale: float = 4.0,
                   mean=IMAGENET_MEAN, std=IMAGENET_STD) -> GraphDef:
    """``logits_scale`` multiplies the He-style init of the logits layer, as in
    ``deeplab_v3_graph_def``: random features give nearly tied classes otherwise."""
    if depth < 1 or any(s % (1 << depth) for s in crop_hw):
        raise ValueError(f"crop_hw {tuple(crop_hw)} must be a multiple of 2^depth = {1 << depth}")
    gb = GraphBuilder()
    init = _Init(seed)
    shape = [None, image_hw[0], image_hw[1], 3] if image_hw else [None, None, None, 3]
    images = gb.placeholder("images", "UINT8", shape)
    x = gb.cast(images, "FLOAT", name="Cast")
    x = gb.resize_bilinear(x, gb.constant("size", np.asarray(crop_hw, dtype=np.int32)), name="ResizeBilinear")
    x = gb.sub(x, gb.constant("mean", np.asarray(mean, dtype=np.float32)), name="Sub")
    x = gb.div(x, gb.constant("std", np.asarray(std, dtype=np.float32)), name="normalized")
    cin, hw, skips = 3, list(crop_hw), []
    for lv in range(depth):
        c = base << lv
        x = _conv_bn_relu(gb, init, x, 3, cin, c, f"down{lv}/conv1")
        x = _conv_bn_relu(gb, init, x, 3, c, c, f"down{lv}/conv2")
        skips.append((x, c, tuple(hw)))
        x = gb.max_pool(x, (2, 2), (2, 2), "VALID", name=f"down{lv}/pool")
        hw = [s // 2 for s in hw]
        cin = c
    c = base << depth
    x = _conv_bn_relu(gb, init, x, 3, cin, c, "bottleneck/conv1")
    x = _conv_bn_relu(gb, init, x, 3, c, c, "bottleneck/conv2")
    cin = c
    for lv in reversed(range(depth)):
        skip, c, shw = skips[lv]
        with gb.name_scope(f"up{lv}"):
            # [KH, KW, Cout, Cin]; each output pixel sums one tap over Cin
            w = (init.rng.standard_normal((2, 2, c, cin)) * np.sqrt(2.0 / cin)).astype(np.float32)
            y = gb.conv2d_transpose(x, gb.constant("upconv/weights", w), shw, (2, 2), "SAME", name="upconv")
            b = gb.constant("upconv/biases", (init.rng.standard_normal(c) * 0.05).astype(np.float32))
            y = gb.bias_add(y, b, name="upconv/BiasAdd")
            x = gb.concat([skip, y], 3, name="concat")
        x = _conv_bn_relu(gb, init, x, 3, 2 * c, c, f"up{lv}/conv1")
        x = _conv_bn_relu(gb, init, x, 3, c, c, f"up{lv}/conv2")
        cin = c
    with gb.name_scope("logits_layer"):
        w = init.rng.standard_normal((1, 1, cin, num_classes)) * np.sqrt(1.0 / cin) * logits_scale
        y = gb.conv2d(x, gb.constant("weights", w.astype(np.float32)), (1, 1), "SAME", name="Conv2D")
        b = gb.constant("biases", (init.rng.standard_normal(num_classes) * 0.1).astype(np.float32))
    logits = gb.bias_add(y, b, name="logits")
    labels = gb.argmax(logits, 3, output_type="INT32", name="labels")
    gb.cast(labels, "UINT8", name="label_map")
    return gb.build_graph_def()


def export_unet_saved_model(export_dir: str, **graph_args) -> str:
    """The U-Net as a TF 1.x SavedModel with its weights as variables (signature
    ``serving_default``: ``images`` -> ``logits``, ``label_map``); ``graph_args`` are those of
    ``unet_graph_def``."""
    from ...proto.messages import SignatureDef
    from ..export import graph_def_to_saved_model, tensor_info

    num_classes = graph_args.get("num_classes", 21)
    ih, iw = graph_args.get("image_hw") or (-1, -1)
    ch, cw = graph_args.get("crop_hw", (256, 256))
    sig = SignatureDef(inputs={"images": tensor_info("images:0", "UINT8", [-1, ih, iw, 3])},
                       outputs={"logits": tensor_info("logits:0", "FLOAT", [-1, ch, cw, num_classes]),
                                "label_map": tensor_info("label_map:0", "UINT8", [-1, ch, cw])},
                       method_name="tensorflow/serving/predict")
    return graph_def_to_saved_model(export_dir, unet_graph_def(**graph_args), {"serving_default": sig})
