"""Sliding-window causal attention (query i sees key j iff ``i - W < j <= i`` and key j is no
padding): ``kernels/attention_window.hip``, the windowed ``packed_rows`` / ``last_attention`` paths and
the ``window_attention`` lowering, against plain float64 masked-softmax attention."""
import dataclasses
import functools
import itertools

import numpy as np
import pytest
import torch

from flink_tensorflow_amd.graph.compiler import CompiledFunction
from flink_tensorflow_amd.graph.graph import Graph
from flink_tensorflow_amd.graph.packed import PackedFunction
from flink_tensorflow_amd.graph.plan import CompileError
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.models.zoo.next_item import NextItemConfig, next_item_graph_def
from flink_tensorflow_amd.ops import kernels as K

F64, BF = torch.float64, torch.bfloat16
CFG = NextItemConfig(num_items=64, hidden=64, heads=1, layers=2, intermediate=128)  # test_causal_attention's
CU = torch.tensor([0, *itertools.accumulate([5, 70, 0, 130, 33])], dtype=torch.int32)  # ragged, one empty


def attention_f64(qkv, ok, H):
    """Plain float64 attention of [B, S, 3*H*Dh] under the boolean mask ``ok`` [B, S, S] (query, key);
    a query with no admissible key gives a zero row.  -> [B*S, H*Dh]."""
    B, S = qkv.shape[:2]
    Dh = qkv.shape[2] // (3 * H)
    q, k, v = qkv.to(F64).reshape(B, S, 3, H, Dh).permute(2, 0, 3, 1, 4)
    s = ((q @ k.transpose(-1, -2)) / Dh ** 0.5).masked_fill(~ok[:, None], float("-inf"))
    return (torch.softmax(s, -1).nan_to_num(0.0) @ v).permute(0, 2, 1, 3).reshape(B * S, H * Dh)


def band(S, W):
    d = torch.arange(S)[:, None] - torch.arange(S)[None, :]
    return (d >= 0) & (d < W)


def _holes(B, S, g):
    valid = torch.rand(B, S, generator=g) >= 0.3
    valid[1, 0] = False
    return valid


# ----------------------------------------------------------------------------- kernel: exact edges
@functools.lru_cache(maxsize=None)
def edge_case(Dh, S, direction, B=2, H=2):
    """Q = 256 everywhere and key j = s_j in every column (s_j = S - j: the OLDEST admissible key
    wins, s_j = j + 1: the NEWEST), so adjacent logits differ by 256 sqrt(Dh) >= 1448, every float64
    softmax weight but one is exactly 0 and the output row is the V row (integers, |v| <= 32) of that
    key: admitting key i - W fails ``oldest``; admitting i + 1 or dropping the diagonal fails ``newest``."""
    g = torch.Generator().manual_seed(S)
    j = torch.arange(S, dtype=F64)
    sj = (S - j) if direction == "oldest" else (j + 1)
    q = torch.full((B, S, H * Dh), 256.0, dtype=F64)
    k = sj[None, :, None].expand(B, S, H * Dh)
    v = torch.randint(-32, 33, (B, S, H * Dh), generator=g).to(F64)
    valid = _holes(B, S, g)
    valid[0, :S // 2] = False  # a sequence whose first half is padding
    return torch.cat([q, k, v], -1), valid


@pytest.mark.gpu
@pytest.mark.parametrize("direction", ["oldest", "newest"])
@pytest.mark.parametrize("W", [1, 2, 16, 17, 33, 64, 65, 100, "S+3"])
@pytest.mark.parametrize("S", [1, 17, 65, 130, 200])
@pytest.mark.parametrize("Dh", [32, 64, 128])
def test_exact_edges(Dh, S, W, direction):
    dev, B, H = torch.device("cuda", 0), 2, 2
    qkv, valid = edge_case(Dh, S, direction)
    w = S + 3 if W == "S+3" else W
    want = attention_f64(qkv, valid[:, None, :] & band(S, w), H)
    dq, ids = qkv.reshape(B * S, -1).to(BF).to(dev), valid.reshape(-1).to(torch.int32).to(dev)
    got = K.attention(dq, ids, B, S, H, causal=True, window=w)
    assert torch.equal(got.cpu().to(F64), want)
    if W == "S+3":  # the window holds every key: the causal kernel's result, bit for bit
        assert torch.equal(got, K.attention(dq, ids, B, S, H, causal=True))


# ----------------------------------------------------------------------------- kernel: continuous data
@pytest.mark.gpu
@pytest.mark.parametrize("S,W", [(192, 65), (2100, 100)])
def test_continuous_data(S, W):
    """The data and the bound of ``test_causal_attention.test_continuous_data`` (P is rounded to bf16
    before PV and the output once, at most 2^-9 max|V| each); S = 2100 lies above the causal cap."""
    B, H, D = 2, 2, 64
    g = torch.Generator().manual_seed(S)
    x = torch.randn(B * S, 3, H, D, generator=g, dtype=F64)
    x[:, :2] *= 3
    qkv = x.reshape(B, S, 3 * H * D).to(BF).to(F64)
    valid = _holes(B, S, g)
    valid[0, :5] = False
    dev = torch.device("cuda", 0)
    got = K.attention(qkv.reshape(B * S, -1).to(BF).to(dev), (valid.reshape(-1).to(torch.int32) * 7).to(dev), B, S, H,
                      causal=True, window=W).cpu().to(F64)
    ref = attention_f64(qkv, valid[:, None, :] & band(S, W), H)
    err, bound = float((got - ref).abs().max()), 1.05 * 2.0 ** -8 * float(qkv[..., 2 * H * D:].abs().max())
    print(f"S={S} W={W}: max abs error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ----------------------------------------------------------------------------- packed and last-event paths
@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 17, 64])
def test_packed_and_last(W):
    dev, H, D, B, T = torch.device("cuda", 0), 2, 64, len(CU) - 1, 256
    n = int(CU[-1])
    x = torch.randn(T, 3, H, D, generator=torch.Generator().manual_seed(W), dtype=F64)
    x[:, :2] *= 3
    qkv = x.reshape(T, 3 * H * D).to(BF).to(F64)
    t = torch.arange(T)
    seq = torch.bucketize(t, CU[1:].long(), right=True).clamp(max=B - 1)
    want = torch.where(t < n, torch.maximum(CU[seq].long(), t - W + 1), t).to(torch.int32)  # the host formula
    start, last = torch.empty(T, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    K.packed_rows(CU.to(dev), B, T, start, last, window=W)
    assert torch.equal(start.cpu(), want)
    host = torch.empty(T, dtype=torch.int32)
    K.packed_rows(CU, B, T, host, torch.empty(B, dtype=torch.int32), window=W)
    assert torch.equal(host, want)
    # one stream of T rows as one "sequence": same sequence, causal, inside the window
    ok = (seq[:, None] == seq[None, :]) & band(T, W) & (t < n)[None, :]
    ref = attention_f64(qkv[None], ok[None], H)
    bound = 1.05 * 2.0 ** -8 * float(qkv[:, 2 * H * D:].abs().max())
    dq = qkv.to(BF).to(dev)
    got = K.packed_causal_attention(dq, CU.to(dev), start, B, H).cpu().to(F64)
    got_last = K.last_attention(dq, CU.to(dev), B, 130, H, window=W).cpu().to(F64)
    ends = CU[1:].long() - 1
    want_last = torch.where((CU[1:] > CU[:-1])[:, None], ref[ends.clamp(min=0)], torch.zeros(1, dtype=F64))
    for name, a, b in (("packed", got[:n], ref[:n]), ("last", got_last, want_last)):
        err = float((a - b).abs().max())
        print(f"W={W} {name}: max abs error {err:.3e}, bound {bound:.3e}")
        assert err <= bound


# ----------------------------------------------------------------------------- lowering, model
WCFG = dataclasses.replace(CFG, window=5)


def _check_model(device, cfg, S, **graph_args):
    """``test_causal_attention._check_model`` for a windowed graph: a strict plan with two
    ``window_attention`` steps and no glue, and the top-k scores of the fp32 interpreter."""
    g = Graph.from_graph_def(next_item_graph_def(cfg, S, 4, seed=1, **graph_args))
    ids = torch.randint(1, cfg.num_items, (3, S), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    ids[0, :S // 3] = 0      # left pads: some, all but one event, none
    ids[1, :S - 1] = 0
    plan = CompiledFunction(g, {"item_ids:0": ((3, S), "INT32")}, ["top_k:0", "top_k:1"], device, strict=True)
    s = plan.summary()
    assert s["kinds"]["window_attention"] == 2 and s["kinds"]["retrieve"] == 1 and s["glue_ops"] == [], s
    vals, idxs = (t.cpu() for t in plan({"item_ids:0": ids.to(device)}))
    ref_scores, ref_vals = Session(g).run(["scores:0", "top_k:0"], {"item_ids:0": ids})
    torch.testing.assert_close(vals.float(), ref_vals, atol=2e-3, rtol=2e-2)
    torch.testing.assert_close(vals.float(), ref_scores.gather(1, idxs.long()), atol=2e-3, rtol=2e-2)
    return g, ids, ref_vals


@pytest.mark.parametrize("band_part", [False, True], ids=["constant", "MatrixBandPart"])
def test_windowed_model_lowers_strict_and_matches_interpreter(band_part):
    g, ids, ref_vals = _check_model("cpu", WCFG, 16, band_part=band_part)
    plan = PackedFunction(g, {"item_ids:0": ((3, 16), "INT32")}, ["top_k:0", "top_k:1"], "cpu", strict=True,
                          pack_causal=True, capacities=[16, 32, 48])
    s = plan.summary()
    assert s["glue_ops"] == [] and (s["kinds"]["packed_causal_attention"], s["kinds"]["last_attention"]) == (1, 1), s
    torch.testing.assert_close(plan({"item_ids:0": ids})[0].float(), ref_vals, atol=2e-3, rtol=2e-2)


def _hole(S):
    c = np.triu(np.tril(np.ones((S, S), np.float32)), -4)
    c[S // 2, S // 2 - 2] = 0.0
    return c


@pytest.mark.parametrize("const", [_hole, lambda S: np.triu(np.tril(np.ones((S, S), np.float32), -1), -5)],
                         ids=["hole", "off_diagonal"])
def test_wrong_bands_do_not_match(const):
    g = Graph.from_graph_def(next_item_graph_def(CFG, 16, 4, seed=1, causal_const=const(16)[None, None]))
    with pytest.raises(CompileError):
        CompiledFunction(g, {"item_ids:0": ((3, 16), "INT32")}, ["top_k:0"], "cpu", strict=True)


def test_window_arguments():
    qkv, ids = torch.zeros(4, 192, dtype=BF), torch.ones(4, dtype=torch.int32)
    for bad in (dict(window=2), dict(causal=True, window=0)):
        with pytest.raises(ValueError):
            K.attention(qkv, ids, 1, 4, 1, **bad)


@pytest.mark.gpu
def test_windowed_model_on_device():
    _check_model(torch.device("cuda", 0), dataclasses.replace(CFG, window=20), 80)
