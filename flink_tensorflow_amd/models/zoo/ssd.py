"""SSD-MobileNet-V1 as a frozen TF GraphDef (random-init weights; no network access): object
detection, the third model family of an image pipeline next to classification and
segmentation.

The graph, behind the image front end of ``mobilenet.py`` (``Cast → ResizeBilinear → Sub →
Div``):

* the MobileNet-V1 feature extractor (``mobilenet.MOBILENET_V1_BLOCKS``); feature maps are taken
  after block 11 (stride 16) and block 13 (stride 32), followed by four extra ``1x1 → 3x3 / 2``
  layers (Conv2D + BatchNorm + Relu6).  At 300 x 300 the six grids are 19, 10, 5, 3, 2, 1;
* per feature map a 1x1 conv box predictor (``anchors * 4`` channels) and a 1x1 conv class
  predictor (``anchors * (num_classes + 1)`` channels, column 0 the background), each
  ``BiasAdd → Reshape`` to ``[B, cells * anchors, ·]`` and joined by ``ConcatV2(axis=1)``:
  ``box_encodings`` and the class logits.  3 anchors per cell on the first map and 6 on the
  others: N = 1917 at 300 x 300;
* anchors by the SSD scale rule (``ssd_anchors``), computed in numpy and stored as a constant;
* the head: ``Sigmoid``, a last-axis slice that drops the background column
  (``class_scores``), ``GraphBuilder.decode_boxes`` and ``CombinedNonMaxSuppression``.

The compiler lowers all of it: the backbone as MobileNet-V1, the narrow predictor convs with
zero-padded filters (12 → 16 channels) and a ``copy`` that compacts them at the ``Reshape``,
the axis-1 concats as ``concat`` steps, and decode + slice + NMS as one ``nms`` step
(``kernels/detection.hip``).  ``Sigmoid`` is an elementwise step over ``B * N * (C + 1)`` values,
which must be a multiple of 8 (``ssd_batch_ok``): with the default N = 1917 and C + 1 = 91, both
odd, the batch itself must be a multiple of 8.

Tensor names: ``images`` (uint8 [B,H,W,3]), ``normalized``, ``box_encodings`` [B,N,4],
``class_scores`` [B,N,C], ``detection_boxes`` [B,T,4], ``detection_scores`` [B,T],
``detection_classes`` [B,T] (fp32, background-free: class 0 is the first real class),
``num_detections`` [B] int32.
"""
from __future__ import annotations

import numpy as np

from ...graph.builder import GraphBuilder
from ...proto.messages import GraphDef
from .mobilenet import MOBILENET_V1_BLOCKS, _bn_relu6, _width
from .resnet import IMAGENET_MEAN, IMAGENET_STD, _Init

# (1x1 depth, 3x3 / 2 depth) of the four extra feature layers at alpha = 1
SSD_EXTRA_LAYERS = ((256, 512), (128, 256), (128, 256), (64, 128))
BOX_CODER_SCALES = (10.0, 10.0, 5.0, 5.0)


def ssd_anchors(grids, min_scale: float = 0.2, max_scale: float = 0.95) -> tuple[np.ndarray, list[int]]:
    """The anchor table ``[N, 4]`` = (yc, xc, h, w), fp32, in normalised image coordinates, and
    the anchors per cell of every feature map.  Map ``k`` of ``m`` has the scale ``s_k =
    min_scale + (max_scale - min_scale) * k / (m - 1)`` (``s_m = 1``).  The first map has three
    anchors, (0.1, 1), (s_0, 2), (s_0, 1/2) as (scale, aspect ratio); every other one the ratios
    1, 2, 1/2, 3, 1/3 at ``s_k`` and ratio 1 at ``sqrt(s_k * s_(k+1))``.  An anchor is ``h = s /
    sqrt(ratio)``, ``w = s * sqrt(ratio)`` around the cell centre ``((i + 0.5) / rows, (j + 0.5)
    / cols)``; the order is row, column, anchor, map after map."""
    m = len(grids)
    scales = [min_scale + (max_scale - min_scale) * k / max(m - 1, 1) for k in range(m)] + [1.0]
    rows, per_cell = [], []
    for k, (gh, gw) in enumerate(grids):
        if k == 0:
            spec = [(0.1, 1.0), (scales[0], 2.0), (scales[0], 0.5)]
        else:
            spec = [(scales[k], r) for r in (1.0, 2.0, 0.5, 3.0, 1.0 / 3.0)]
            spec.append((float(np.sqrt(scales[k] * scales[k + 1])), 1.0))
        per_cell.append(len(spec))
        for i in range(gh):
            for j in range(gw):
                for s, r in spec:
                    rows.append(((i + 0.5) / gh, (j + 0.5) / gw, s / np.sqrt(r), s * np.sqrt(r)))
    return np.asarray(rows, dtype=np.float32), per_cell


def ssd_feature_grids(hw: tuple[int, int]) -> list[tuple[int, int]]:
    """Grid sizes of the six feature maps for a network input of ``hw`` (SAME padding: every
    stride-2 layer halves rounding up): strides 16 and 32, then four more halvings."""
    def down(v, times):
        for _ in range(times):
            v = -(-v // 2)
        return v

    return [(down(hw[0], t), down(hw[1], t)) for t in (4, 5, 6, 7, 8, 9)]


def ssd_batch_ok(batch: int, hw: tuple[int, int], num_classes: int) -> bool:
    """True when a strict plan of the graph compiles for ``batch`` images resized to ``hw``: the
    ``Sigmoid`` over the class logits is an elementwise step and takes 8 values at a time."""
    grids = ssd_feature_grids(hw)
    n = sum(gh * gw * a for (gh, gw), a in zip(grids, [3] + [6] * (len(grids) - 1)))
    return batch * n * (num_classes + 1) % 8 == 0


def ssd_mobilenet_v1_graph_def(num_classes: int = 90, image_hw: tuple[int, int] | None = (300, 300), alpha: float = 1.0,
                               seed: int = 0, max_per_class: int = 100, max_total: int = 100,
                               iou_threshold: float = 0.6, score_threshold: float = 1e-8, scores_scale: float = 4.0,
                               input_hw: tuple[int, int] | None = None, mean=IMAGENET_MEAN,
                               std=IMAGENET_STD) -> GraphDef:
    """``image_hw`` is the size of the fed images (None: any), ``input_hw`` the size they are
    resized to (``image_hw``, or 300 x 300).  ``scores_scale`` multiplies the He-style init of the
    class predictors: random features give nearly equal scores otherwise, and a detection list
    of ties says little."""
    gb = GraphBuilder()
    init = _Init(seed)
    net_hw = tuple(input_hw or image_hw or (300, 300))
    shape = [None, image_hw[0], image_hw[1], 3] if image_hw else [None, None, None, 3]
    images = gb.placeholder("images", "UINT8", shape)
    x = gb.cast(images, "FLOAT", name="Cast")
    x = gb.resize_bilinear(x, gb.constant("size", np.asarray(net_hw, dtype=np.int32)), name="ResizeBilinear")
    x = gb.sub(x, gb.constant("mean", np.asarray(mean, dtype=np.float32)), name="Sub")
    x = gb.div(x, gb.constant("std", np.asarray(std, dtype=np.float32)), name="normalized")
    cin = _width(32, alpha)
    maps = []  # (tensor, channels)
    with gb.name_scope("FeatureExtractor/MobilenetV1"):
        with gb.name_scope("Conv2d_0"):
            y = gb.conv2d(x, gb.constant("weights", init.conv(3, 3, 3, cin)), (2, 2), "SAME", name="Conv2D")
            x = _bn_relu6(gb, init, y, cin)
        for i, (c, stride) in enumerate(MOBILENET_V1_BLOCKS, 1):
            cout = _width(c, alpha)
            with gb.name_scope(f"Conv2d_{i}_depthwise"):
                w = (init.rng.standard_normal((3, 3, cin, 1)) * np.sqrt(2.0 / 9)).astype(np.float32)
                y = gb.depthwise_conv2d(x, gb.constant("depthwise_weights", w), (stride, stride), "SAME", name="depthwise")
                x = _bn_relu6(gb, init, y, cin)
            with gb.name_scope(f"Conv2d_{i}_pointwise"):
                y = gb.conv2d(x, gb.constant("weights", init.conv(1, 1, cin, cout)), (1, 1), "SAME", name="Conv2D")
                x = _bn_relu6(gb, init, y, cout)
            cin = cout
            if i in (11, 13):
                maps.append((x, cin))
        for j, (d1, d2) in enumerate(SSD_EXTRA_LAYERS, 14):
            c1, c2 = _width(d1, alpha), _width(d2, alpha)
            with gb.name_scope(f"Conv2d_{j}_1_1x1"):
                y = gb.conv2d(x, gb.constant("weights", init.conv(1, 1, cin, c1)), (1, 1), "SAME", name="Conv2D")
                x = _bn_relu6(gb, init, y, c1)
            with gb.name_scope(f"Conv2d_{j}_2_3x3_s2"):
                y = gb.conv2d(x, gb.constant("weights", init.conv(3, 3, c1, c2)), (2, 2), "SAME", name="Conv2D")
                x = _bn_relu6(gb, init, y, c2)
            cin = c2
            maps.append((x, cin))
    grids = ssd_feature_grids(net_hw)
    anchors, per_cell = ssd_anchors(grids)
    encs, logits = [], []
    for k, ((feat, c), (gh, gw), a) in enumerate(zip(maps, grids, per_cell)):
        with gb.name_scope(f"BoxPredictor_{k}"):
            w = gb.constant("BoxEncodingPredictor/weights", init.conv(1, 1, c, a * 4))
            b = gb.constant("BoxEncodingPredictor/biases", (init.rng.standard_normal(a * 4) * 0.1).astype(np.float32))
            y = gb.bias_add(gb.conv2d(feat, w, (1, 1), "SAME", name="BoxEncodingPredictor/Conv2D"), b,
                            name="BoxEncodingPredictor/BiasAdd")
            encs.append(gb.reshape(y, [-1, gh * gw * a, 4], name="box_encodings"))
            w = gb.constant("ClassPredictor/weights", init.conv(1, 1, c, a * (num_classes + 1)) * np.float32(scores_scale))
            b = gb.constant("ClassPredictor/biases",
                            (init.rng.standard_normal(a * (num_classes + 1)) * 0.1).astype(np.float32))
            y = gb.bias_add(gb.conv2d(feat, w, (1, 1), "SAME", name="ClassPredictor/Conv2D"), b,
                            name="ClassPredictor/BiasAdd")
            logits.append(gb.reshape(y, [-1, gh * gw * a, num_classes + 1], name="class_logits"))
    enc = gb.concat(encs, 1, name="box_encodings")
    probs = gb.sigmoid(gb.concat(logits, 1, name="class_logits"), name="class_probabilities")
    scores = gb.last_axis_slice(probs, 1, num_classes + 1, name="class_scores")
    boxes = gb.decode_boxes(enc, anchors, BOX_CODER_SCALES, name="decode_boxes")
    nms = gb.combined_nms(boxes, scores, max_per_class, max_total, iou_threshold, score_threshold,
                          name="CombinedNonMaxSuppression").split(":")[0]
    for i, name in enumerate(("detection_boxes", "detection_scores", "detection_classes", "num_detections")):
        gb.identity(f"{nms}:{i}", name=name)
    return gb.build_graph_def()
