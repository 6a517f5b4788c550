"""DeepLab-v3 on the MobileNet-V1 backbone as a frozen TF GraphDef (random-init weights; no
network access): semantic segmentation, the dense-prediction model users serve from the
depthwise-separable family.

The graph is the one TF's DeepLab export emits, behind the image front end of ``mobilenet.py``
(``Cast → ResizeBilinear(crop) → Sub → Div``):

* the MobileNet-V1 feature extractor (``mobilenet.MOBILENET_V1_BLOCKS``) with TF-slim's
  ``output_stride`` rule: once the running stride reaches ``output_stride`` a stride-2 depthwise
  layer runs at stride 1 and every later depthwise layer is dilated by the stride it gave up;
* ASPP: a 1x1 conv, one atrous 3x3 conv per rate and the image-pooling branch
  ``Mean(keep_dims) → 1x1 conv → BN → Relu → ResizeBilinear(align_corners)``, joined by
  ``ConcatV2`` and projected by a 1x1 conv;
* the head: a 1x1 conv to ``num_classes`` + ``BiasAdd`` (``logits``), ``ResizeBilinear`` back to
  the crop with ``align_corners`` (``upsampled``), ``ArgMax`` over the channels (``labels``) and a
  ``Cast`` to uint8 (``label_map``).

The compiler lowers all of it: the atrous convs to the implicit GEMM (its K walk takes the
dilation), the dilated depthwise layers to the generic depthwise kernel, the pooled branch's
broadcast to the resize kernel writing its concat slot, the ``num_classes``-channel conv with its
filters zero-padded to a multiple of 8, and ``upsampled → labels → label_map`` to one fused
resize + ArgMax launch (``kernels/resize.hip``) that stores bytes.

Tensor names: ``images`` (uint8 [N,H,W,3]), ``normalized``, ``logits`` ([N,h,w,classes]),
``upsampled``, ``labels`` (int32 [N,H,W]), ``label_map`` (uint8 [N,H,W]).
"""
from __future__ import annotations

import numpy as np

from ...graph.builder import GraphBuilder
from ...proto.messages import GraphDef
from .mobilenet import MOBILENET_V1_BLOCKS, _bn_relu6, _width
from .resnet import IMAGENET_MEAN, IMAGENET_STD, _Init


def _conv_bn_relu(gb: GraphBuilder, init: _Init, x, k, cin, cout, name, rate=1):
    with gb.name_scope(name):
        y = gb.conv2d(x, gb.constant("weights", init.conv(k, k, cin, cout)), (1, 1), "SAME", name="Conv2D",
                      dilations=(rate, rate))
        g, b, m, v = init.bn(cout)
        y = gb.fused_batch_norm(y, gb.constant("gamma", g), gb.constant("beta", b), gb.constant("moving_mean", m),
                                gb.constant("moving_variance", v), 1e-3, name="BatchNorm")
        return gb.relu(y, name="Relu")


def deeplab_v3_graph_def(alpha: float = 1.0, num_classes: int = 21, image_hw: tuple[int, int] | None = None,
                         crop_hw: tuple[int, int] = (513, 513), output_stride: int = 16,
                         atrous_rates: tuple[int, ...] = (6, 12, 18), seed: int = 0, aspp_channels: int = 256,
                         logits_scale: float = 4.0, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> GraphDef:
    """``logits_scale`` multiplies the He-style init of the logits layer: random features give
    nearly tied classes otherwise, and a label map of ties says little."""
    if output_stride not in (8, 16, 32):
        raise ValueError(f"output_stride must be 8, 16 or 32, not {output_stride}")
    gb = GraphBuilder()
    init = _Init(seed)
    shape = [None, image_hw[0], image_hw[1], 3] if image_hw else [None, None, None, 3]
    images = gb.placeholder("images", "UINT8", shape)
    x = gb.cast(images, "FLOAT", name="Cast")
    x = gb.resize_bilinear(x, gb.constant("size", np.asarray(crop_hw, dtype=np.int32)), name="ResizeBilinear")
    x = gb.sub(x, gb.constant("mean", np.asarray(mean, dtype=np.float32)), name="Sub")
    x = gb.div(x, gb.constant("std", np.asarray(std, dtype=np.float32)), name="normalized")
    cin = _width(32, alpha)
    with gb.name_scope("MobilenetV1"):
        with gb.name_scope("Conv2d_0"):
            y = gb.conv2d(x, gb.constant("weights", init.conv(3, 3, 3, cin)), (2, 2), "SAME", name="Conv2D")
            x = _bn_relu6(gb, init, y, cin)
        hw = [-(-s // 2) for s in crop_hw]  # SAME: ceil(size / stride)
        cur, rate = 2, 1
        for i, (c, stride) in enumerate(MOBILENET_V1_BLOCKS, 1):
            cout = _width(c, alpha)
            if cur == output_stride:  # keep the resolution: dilate what follows instead
                s, r = 1, rate
                rate *= stride
            else:
                s, r = stride, 1
                cur *= stride
                hw = [-(-v // stride) for v in hw]
            with gb.name_scope(f"Conv2d_{i}_depthwise"):
                w = (init.rng.standard_normal((3, 3, cin, 1)) * np.sqrt(2.0 / 9)).astype(np.float32)
                y = gb.depthwise_conv2d(x, gb.constant("depthwise_weights", w), (s, s), "SAME", name="depthwise",
                                        dilations=(r, r))
                x = _bn_relu6(gb, init, y, cin)
            with gb.name_scope(f"Conv2d_{i}_pointwise"):
                y = gb.conv2d(x, gb.constant("weights", init.conv(1, 1, cin, cout)), (1, 1), "SAME", name="Conv2D")
                x = _bn_relu6(gb, init, y, cout)
            cin = cout
    depth = _width(aspp_channels, alpha)
    with gb.name_scope("image_pooling_branch"):
        pooled = gb.mean(x, [1, 2], keep_dims=True, name="Mean")
    pooled = _conv_bn_relu(gb, init, pooled, 1, cin, depth, "image_pooling")
    branches = [gb.resize_bilinear(pooled, gb.constant("image_pooling/size", np.asarray(hw, dtype=np.int32)),
                                   name="image_pooling/ResizeBilinear", align_corners=True)]
    branches.append(_conv_bn_relu(gb, init, x, 1, cin, depth, "aspp0"))
    for j, r in enumerate(atrous_rates, 1):
        branches.append(_conv_bn_relu(gb, init, x, 3, cin, depth, f"aspp{j}", rate=r))
    x = gb.concat(branches, 3, name="concat")
    x = _conv_bn_relu(gb, init, x, 1, depth * len(branches), depth, "concat_projection")
    with gb.name_scope("logits_layer"):
        w = init.rng.standard_normal((1, 1, depth, num_classes)) * np.sqrt(1.0 / depth) * logits_scale
        y = gb.conv2d(x, gb.constant("weights", w.astype(np.float32)), (1, 1), "SAME", name="Conv2D")
        b = gb.constant("biases", (init.rng.standard_normal(num_classes) * 0.1).astype(np.float32))
    logits = gb.bias_add(y, b, name="logits")
    up = gb.resize_bilinear(logits, gb.constant("upsampled/size", np.asarray(crop_hw, dtype=np.int32)),
                            name="upsampled", align_corners=True)
    labels = gb.argmax(up, 3, output_type="INT32", name="labels")
    gb.cast(labels, "UINT8", name="label_map")
    return gb.build_graph_def()
