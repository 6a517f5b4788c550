"""MobileNet-V1 as a frozen TF GraphDef (random-init weights; no network access).

The depthwise-separable family is what users serve from TF SavedModels on small budgets.  The
model is emitted as a real TF graph — ``Conv2D`` / ``DepthwiseConv2dNative`` /
``FusedBatchNormV3`` / ``Relu6`` / ``Mean`` / ``MatMul`` / ``BiasAdd`` / ``Softmax`` /
``TopKV2`` — behind the same image normalization front end as ``resnet.py``: a 3x3/s2 stem,
13 depthwise-separable blocks (3x3 depthwise, then 1x1 pointwise, each followed by
BatchNorm and Relu6) and a global-average-pool + fully-connected head.  The compiler folds
every BatchNorm into its conv, runs the depthwise layers on ``kernels/dwconv.hip`` and the
stem and pointwise layers on the implicit GEMM with its Relu6 epilogue.

Channel counts are ``alpha``-scaled and rounded to multiples of 8.  TF-slim's 1001-way
1x1-conv classifier is replaced by ``Mean → MatMul``, as newer exports do (a conv whose output
channels are no multiple of 8 lowers too: the compiler zero-pads its filters to the next
multiple and the consumers read the logical columns).

Tensor names: ``images`` (uint8 [N,H,W,3]), ``normalized``, ``logits``, ``probs``, ``top_k``
(``top_k:0`` values, ``top_k:1`` indices).
"""
from __future__ import annotations

import numpy as np

from ...graph.builder import GraphBuilder
from ...proto.messages import GraphDef
from .resnet import IMAGENET_MEAN, IMAGENET_STD, _Init

# (pointwise output channels at alpha = 1, depthwise stride) of the 13 separable blocks
MOBILENET_V1_BLOCKS = ((64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2), (512, 1), (512, 1), (512, 1),
                       (512, 1), (512, 1), (1024, 2), (1024, 1))


def _width(c: int, alpha: float) -> int:
    return max(8, int(c * alpha + 4) // 8 * 8)


def _bn_relu6(gb: GraphBuilder, init: _Init, y, c):
    g, b, m, v = init.bn(c)
    y = gb.fused_batch_norm(y, gb.constant("gamma", g), gb.constant("beta", b), gb.constant("moving_mean", m),
                            gb.constant("moving_variance", v), 1e-3, name="BatchNorm")
    return gb.relu6(y, name="Relu6")


def mobilenet_v1_graph_def(alpha: float = 1.0, num_classes: int = 1000, seed: int = 0,
                           image_hw: tuple[int, int] | None = None, out_hw: tuple[int, int] = (224, 224),
                           top_k: int = 5, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> GraphDef:
    gb = GraphBuilder()
    init = _Init(seed)
    shape = [None, image_hw[0], image_hw[1], 3] if image_hw else [None, None, None, 3]
    images = gb.placeholder("images", "UINT8", shape)
    x = gb.cast(images, "FLOAT", name="Cast")
    x = gb.resize_bilinear(x, gb.constant("size", np.asarray(out_hw, dtype=np.int32)), name="ResizeBilinear")
    x = gb.sub(x, gb.constant("mean", np.asarray(mean, dtype=np.float32)), name="Sub")
    x = gb.div(x, gb.constant("std", np.asarray(std, dtype=np.float32)), name="normalized")
    cin = _width(32, alpha)
    with gb.name_scope("Conv2d_0"):
        y = gb.conv2d(x, gb.constant("weights", init.conv(3, 3, 3, cin)), (2, 2), "SAME", name="Conv2D")
        x = _bn_relu6(gb, init, y, cin)
    for i, (c, stride) in enumerate(MOBILENET_V1_BLOCKS, 1):
        cout = _width(c, alpha)
        with gb.name_scope(f"Conv2d_{i}_depthwise"):
            # He init over the 9 taps of one channel
            w = (init.rng.standard_normal((3, 3, cin, 1)) * np.sqrt(2.0 / 9)).astype(np.float32)
            y = gb.depthwise_conv2d(x, gb.constant("depthwise_weights", w), (stride, stride), "SAME", name="depthwise")
            x = _bn_relu6(gb, init, y, cin)
        with gb.name_scope(f"Conv2d_{i}_pointwise"):
            y = gb.conv2d(x, gb.constant("weights", init.conv(1, 1, cin, cout)), (1, 1), "SAME", name="Conv2D")
            x = _bn_relu6(gb, init, y, cout)
        cin = cout
    x = gb.mean(x, [1, 2], name="avg_pool")
    w = gb.constant("fc/weights", (init.rng.standard_normal((cin, num_classes)) * np.sqrt(1.0 / cin)).astype(np.float32))
    b = gb.constant("fc/biases", np.zeros(num_classes, dtype=np.float32))
    logits = gb.bias_add(gb.matmul(x, w, name="fc/MatMul"), b, name="logits")
    probs = gb.softmax(logits, name="probs")
    gb.top_k(probs, top_k, name="top_k")
    return gb.build_graph_def()
