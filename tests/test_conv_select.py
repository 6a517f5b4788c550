"""Which kernel a Conv2D site runs on (``graph/conv_lowering.py``): the choice is a pure
function of a ``ConvSite``, so it is checked here without a plan and without a GPU."""
import dataclasses

import pytest
import torch

from flink_tensorflow_amd.graph.conv_lowering import ConvSite, select_conv_fp8_kernel, select_conv_kernel
from flink_tensorflow_amd.ops import kernels as K

RELU, NONE = K.ACT_RELU, K.ACT_NONE
SAME3 = (1, 1, 1, 1)     # 3x3, stride 1, SAME
SAME3_S2 = (0, 1, 0, 1)  # 3x3, stride 2, SAME on an even size
B = 256

# The single-conv steps of ResNet-50 v1.5 at 224x224, B=256, bf16, on an MI355X, as planned by
# the parent of the commit that split conv_lowering.py out of the compiler (aaff264, "Prune
# diagnostic and dead entry points from the HIP kernel library").  Recorded from a listing of
#   CompiledFunction(Graph.from_graph_def(resnet50_graph_def(image_hw=(224, 224), top_k=5, seed=0)),
#                    {"images:0": ((256, 224, 224, 3), "UINT8")}, ["top_k:0", "top_k:1"], "cuda:0",
#                    use_graph=False, strict=True)
# that printed, per step, its name, kind, meta["impl"], the shapes of its inputs and outputs
# and the name of the launch closure (that plan records no impl for dconv, conv_lite and
# igemm steps: run_d is the dconv closure, the closure holding a ConvPP the conv_lite one).
# Not in the table, because a graph-structural fusion takes them before the kernel choice:
# stage 1's expand convs (bottleneck_tail / bottleneck_chain, with the reduce conv that
# follows) and the expand + projection-shortcut pairs that open stages 2-4 (conv1x1_dual /
# conv_lite_dual).  block2/unit1/conv1 (the stage-2 K=256 reduce) is its own step only with
# fuse_block_tails off: its row is from the same listing under override(fuse_block_tails=False).
# columns: name, input NHWC, Cout, (KH, KW), stride, pads, act, residual, impl
RESNET50 = [
    ("block1/unit1/conv1", (B, 56, 56, 64), 64, (1, 1), 1, (0, 0, 0, 0), RELU, None, "igemm"),
    ("block1/unit*/conv2", (B, 56, 56, 64), 64, (3, 3), 1, SAME3, RELU, None, "conv3x3c64"),
    ("block2/unit1/conv1 (fuse_block_tails off)", (B, 56, 56, 256), 128, (1, 1), 1, (0, 0, 0, 0), RELU, None, "igemm"),
    ("block2/unit1/conv2", (B, 56, 56, 128), 128, (3, 3), 2, SAME3_S2, RELU, None, "conv_lite"),
    ("block2/unit2-4/conv1", (B, 28, 28, 512), 128, (1, 1), 1, (0, 0, 0, 0), RELU, None, "igemm"),
    ("block2/unit2-4/conv2", (B, 28, 28, 128), 128, (3, 3), 1, SAME3, RELU, None, "conv_lite"),
    ("block2/unit2-4/conv3", (B, 28, 28, 128), 512, (1, 1), 1, (0, 0, 0, 0), RELU, "plain", "pw_res"),
    ("block3/unit1/conv1", (B, 28, 28, 512), 256, (1, 1), 1, (0, 0, 0, 0), RELU, None, "gemm_pp"),
    ("block3/unit1/conv2", (B, 28, 28, 256), 256, (3, 3), 2, SAME3_S2, RELU, None, "conv_lite"),
    ("block3/unit2-6/conv1", (B, 14, 14, 1024), 256, (1, 1), 1, (0, 0, 0, 0), RELU, None, "gemm_pp"),
    ("block3/unit2-6/conv2", (B, 14, 14, 256), 256, (3, 3), 1, SAME3, RELU, None, "conv_lite"),
    ("block3/unit2-6/conv3", (B, 14, 14, 256), 1024, (1, 1), 1, (0, 0, 0, 0), RELU, "plain", "pw_res"),
    ("block4/unit1/conv1", (B, 14, 14, 1024), 512, (1, 1), 1, (0, 0, 0, 0), RELU, None, "gemm_pp"),
    ("block4/unit1/conv2", (B, 14, 14, 512), 512, (3, 3), 2, SAME3_S2, RELU, None, "conv_lite"),
    ("block4/unit2-3/conv1", (B, 7, 7, 2048), 512, (1, 1), 1, (0, 0, 0, 0), RELU, None, "gemm_pp"),
    ("block4/unit2-3/conv2", (B, 7, 7, 512), 512, (3, 3), 1, SAME3, RELU, None, "conv_lite"),
    ("block4/unit2-3/conv3", (B, 7, 7, 512), 2048, (1, 1), 1, (0, 0, 0, 0), RELU, "plain", "igemm"),
]
# choices that do not depend on the device today; every other one falls to igemm on the host
UNGATED = ("conv3x3c64", "pw_res")


def _site(x_shape, cout, kernel, stride, pads, act, residual, on_gpu=True, **kw):
    return ConvSite(on_gpu=on_gpu, x_shape=x_shape, cin=x_shape[-1], cin_phys=x_shape[-1], cout=cout, kernel=kernel,
                    stride=(stride, stride), pads=pads, act=act, residual=residual is not None,
                    res_plain=residual == "plain", res_alias=residual == "alias", **kw)


# the stem: 7x7 / stride 2 over RGB, lowered as a 4x4 / stride 1 conv over the space-to-depth
# preprocess output (16 channels; block pads of SAME on 224: (1, 2, 1, 2)), ReLU -> dconv
STEM = ConvSite(on_gpu=True, x_shape=(B, 224, 224, 3), cin=3, cin_phys=16, cout=64, kernel=(4, 4), stride=(1, 1),
                pads=(1, 2, 1, 2), act=RELU, s2d=True)


def _rows(table):
    return [pytest.param(*r[1:], id=r[0]) for r in table]


def test_resnet50_stem():
    assert select_conv_kernel(STEM) == "dconv"
    assert select_conv_kernel(dataclasses.replace(STEM, on_gpu=False)) == "igemm"


@pytest.mark.parametrize("x_shape, cout, kernel, stride, pads, act, residual, impl", _rows(RESNET50))
def test_resnet50_table(x_shape, cout, kernel, stride, pads, act, residual, impl):
    assert select_conv_kernel(_site(x_shape, cout, kernel, stride, pads, act, residual)) == impl
    host = select_conv_kernel(_site(x_shape, cout, kernel, stride, pads, act, residual, on_gpu=False))
    assert host == (impl if impl in UNGATED else "igemm")


def test_table_covers_every_kernel():
    assert {r[-1] for r in RESNET50} | {"dconv"} == {"dconv", "conv3x3c64", "gemm_pp", "pw_res", "conv_lite", "igemm"}


# Inception-v3 fp8 sites at 299x299.  The first four from the same kind of listing of the
# parent's B=64 fp8 plan on the MI355X (inception_v3_graph_def(image_hw=(299, 299), top_k=5,
# seed=0), precision="fp8").  There the stem folds the preprocess kernel and emits e4m3, so
# no layer reads bf16; the host plan of the same graph (B=2) keeps a bf16 stem, and its
# Conv2d_2a_3x3 is the register-staged layer of the last row.
# columns: name, input NHWC, input is fp8, Cout, (KH, KW), pads, impl on the GPU, impl on the host
INCEPTION_FP8 = [
    ("Conv2d_2a_3x3", (64, 149, 149, 32), True, 32, (3, 3), (0, 0, 0, 0), "dconv", "conv_lite_fp8"),
    ("Conv2d_2b_3x3", (64, 147, 147, 32), True, 64, (3, 3), SAME3, "dconv", "conv_lite_fp8"),
    ("Conv2d_3b_1x1", (64, 73, 73, 64), True, 80, (1, 1), (0, 0, 0, 0), "conv_lite_fp8", "conv_lite_fp8"),
    ("Conv2d_4a_3x3 (192 channels out)", (64, 73, 73, 80), True, 192, (3, 3), (0, 0, 0, 0), "conv_lite_fp8",
     "conv_lite_fp8"),
    ("Conv2d_2a_3x3 after a bf16 stem", (2, 149, 149, 32), False, 32, (3, 3), (0, 0, 0, 0), "igemm_fp8", "igemm_fp8"),
]


@pytest.mark.parametrize("x_shape, x_fp8, cout, kernel, pads, gpu_impl, host_impl", _rows(INCEPTION_FP8))
def test_inception_fp8_table(x_shape, x_fp8, cout, kernel, pads, gpu_impl, host_impl):
    site = _site(x_shape, cout, kernel, 1, pads, RELU, None, x_fp8=x_fp8,
                 x_dtype=torch.uint8 if x_fp8 else torch.bfloat16, out_dtype=torch.uint8, out_fp8=True)
    assert select_conv_fp8_kernel(site) == gpu_impl
    assert select_conv_fp8_kernel(dataclasses.replace(site, on_gpu=False)) == host_impl


# ---- toggles and edge conditions
STAGE1_3X3 = _site((B, 56, 56, 64), 64, (3, 3), 1, SAME3, RELU, None)
IDENTITY_EXPAND = _site((B, 28, 28, 128), 512, (1, 1), 1, (0, 0, 0, 0), RELU, "plain")
LITE = _site((B, 28, 28, 128), 128, (3, 3), 1, SAME3, RELU, None)


def test_toggles():
    assert select_conv_kernel(STAGE1_3X3) == "conv3x3c64"
    assert select_conv_kernel(dataclasses.replace(STAGE1_3X3, conv3x3c64_kernel=False)) == "conv_lite"
    assert select_conv_kernel(IDENTITY_EXPAND) == "pw_res"
    assert select_conv_kernel(dataclasses.replace(IDENTITY_EXPAND, pw_res_kernel=False)) == "igemm"


@pytest.mark.parametrize("change", [
    dict(out_coff=4),
    dict(x_shape=(B, 28, 28, 96), cin=96, cin_phys=96),
    dict(pads=(1024, 1, 1, 1)),
    dict(pads=(1, 1, 1, 1024)),
    dict(residual=True, res_plain=True, res_alias=True),
    dict(residual=True, res_plain=False),
], ids=["out-offset-4", "cin-96", "pad-1024-rows", "pad-1024-cols", "aliased-residual", "residual-of-another-shape"])
def test_conv_lite_edges_fall_to_igemm(change):
    assert select_conv_kernel(LITE) == "conv_lite"
    assert select_conv_kernel(dataclasses.replace(LITE, **change)) == "igemm"


def test_conv_lite_takes_a_plain_residual():
    assert select_conv_kernel(dataclasses.replace(LITE, residual=True, res_plain=True)) == "conv_lite"
