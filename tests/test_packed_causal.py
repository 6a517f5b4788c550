"""Padding-free causal transformers: ``kernels/attention_causal_packed.hip`` (packed causal
attention, row bookkeeping) and ``last_attention`` on the GPU against plain float64 attention per
sequence, the ``pack_causal`` lowering on the host and the packed next-item model on the GPU.

Bound of the attention tests (as in ``test_causal_attention.py``, the same arithmetic): P is rounded
to bf16 before PV and the output once, at most 2^-9 max|V| each; the fp32 terms are of order
S 2^-22.  ``last_attention`` keeps P in fp32 and stays inside the same bound."""
import itertools

import pytest
import torch

from flink_tensorflow_amd.graph.graph import Graph
from flink_tensorflow_amd.graph.packed import PackedFunction
from flink_tensorflow_amd.graph.plan import CompileError
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.models.zoo.next_item import NextItemConfig, NextItemModel, next_item_graph_def
from flink_tensorflow_amd.ops import kernels as K

F64, BF, T_CAP = torch.float64, torch.bfloat16, 320
CFG = NextItemConfig(num_items=64, hidden=64, heads=1, layers=2, intermediate=128)  # test_causal_attention's
LAYOUTS = {"short": [1, 2, 15, 16, 17, 0, 33],  # sequences share a tile, one is empty, idle tiles behind
           "straddle": [40, 50, 70],            # starts mid-tile, crosses tile borders
           "long": [5, 200, 100]}               # four tiles from an unaligned start, partial last tile
SHAPES = [(dh, h) for dh in (32, 64, 128) for h in (1, 3)]  # odd H: the half pair at 32


def _cu(layout):
    return torch.tensor([0, *itertools.accumulate(LAYOUTS[layout])], dtype=torch.int32)


def attention_f64(qkv, cu, H, last=False):
    """Plain causal attention per sequence in float64: every row [T, H*Dh] (rows past cu[B]: zeros), or
    with ``last`` each sequence's last row [B, H*Dh] (an empty sequence: zeros)."""
    Dh = qkv.shape[1] // (3 * H)
    out = torch.zeros(len(cu) - 1 if last else qkv.shape[0], H * Dh, dtype=F64)
    for b, (a, e) in enumerate(zip(cu[:-1].tolist(), cu[1:].tolist())):
        if e > a:
            q, k, v = qkv[a:e].to(F64).reshape(e - a, 3, H, Dh).permute(1, 2, 0, 3)
            s = (q @ k.transpose(-1, -2)) / Dh ** 0.5
            s = s.masked_fill(~torch.ones(e - a, e - a, dtype=torch.bool).tril(), float("-inf"))
            o = (torch.softmax(s, -1) @ v).permute(1, 0, 2).reshape(e - a, H * Dh)
            out[b if last else slice(a, e)] = o[-1] if last else o
    return out


def _peaked(Dh, H, seed):
    """Continuous data with peaked logits (standard deviation ~9), bf16-exact; all T_CAP rows finite."""
    x = torch.randn(T_CAP, 3, H, Dh, generator=torch.Generator().manual_seed(seed), dtype=F64)
    x[:, :2] *= 3
    return x.reshape(T_CAP, 3 * H * Dh).to(BF).to(F64)


def _bait(Dh, H, cu, seed):
    """q = a u_s + noise, k = -a u_s + noise with a +-1 code u_s per sequence (the idle rows past
    cu[B] have one too): own keys score about -a^2 Dh scale, foreign keys about 0, so a foreign key
    out-scores every own key by a^2 sqrt(Dh) = 30 and a missing lower bound moves rows by O(max|V|)."""
    g = torch.Generator().manual_seed(seed)
    seq = torch.bucketize(torch.arange(T_CAP), cu[1:].long(), right=True)  # the idle rows: index B
    u = (torch.randint(0, 2, (len(cu), H * Dh), generator=g) * 2 - 1).to(F64)[seq]
    a = (30 / Dh ** 0.5) ** 0.5
    q, k, v = (torch.randn(T_CAP, H * Dh, generator=g, dtype=F64) for _ in range(3))
    return torch.cat([a * u + q, -a * u + k, v], 1).to(BF).to(F64)


def _check_packed(qkv, cu, H):
    """qkv as a view into a NaN-filled buffer, ctx pre-filled with a sentinel: the error bound on
    rows < cu[B], the sentinel on the rest."""
    dev = torch.device("cuda", 0)
    B, n = len(cu) - 1, int(cu[-1])
    buf = torch.full((T_CAP + 128, qkv.shape[1]), float("nan"), dtype=BF, device=dev)
    buf[64:64 + T_CAP] = qkv.to(BF)
    start, last = (torch.empty(m, dtype=torch.int32, device=dev) for m in (T_CAP, B))
    K.packed_rows(cu.to(dev), B, T_CAP, start, last)
    ctx = torch.full((T_CAP, qkv.shape[1] // 3), 77.0, dtype=BF, device=dev)
    K.packed_causal_attention(buf[64:64 + T_CAP], cu.to(dev), start, B, H, out=ctx)
    got = ctx.cpu().to(F64)
    err = float((got[:n] - attention_f64(qkv, cu, H)[:n]).abs().max())
    bound = 1.05 * 2.0 ** -8 * float(qkv[:, qkv.shape[1] // 3 * 2:].abs().max())
    print(f"max abs error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert torch.all(got[n:] == 77.0)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("Dh,H", SHAPES)
def test_packed_causal_kernel(Dh, H, layout):
    _check_packed(_peaked(Dh, H, Dh + H), _cu(layout), H)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["straddle", "short"])
@pytest.mark.parametrize("Dh,H", SHAPES)
def test_foreign_keys_are_masked(Dh, H, layout):
    _check_packed(_bait(Dh, H, _cu(layout), Dh + H), _cu(layout), H)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["short", "long"])
@pytest.mark.parametrize("Dh,H", SHAPES)
def test_last_attention(Dh, H, layout):
    dev = torch.device("cuda", 0)
    qkv, cu = _peaked(Dh, H, Dh + H), _cu(layout)
    B = len(cu) - 1
    out = torch.full((B, H * Dh), 77.0, dtype=BF, device=dev)
    K.last_attention(qkv.to(BF).to(dev), cu.to(dev), B, 256, H, out=out)
    got, ref = out.cpu().to(F64), attention_f64(qkv, cu, H, last=True)
    err, bound = float((got - ref).abs().max()), 1.05 * 2.0 ** -8 * float(qkv[:, 2 * H * Dh:].abs().max())
    print(f"max abs error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    empty = [b for b, n in enumerate(LAYOUTS[layout]) if n == 0]
    assert torch.all(got[empty] == 0)
    with pytest.raises(ValueError):
        K.last_attention(qkv.to(BF).to(dev), cu.to(dev), B, 513, H)


def _rows_host(layout):
    cu = _cu(layout)
    start, last = torch.empty(T_CAP, dtype=torch.int32), torch.empty(len(cu) - 1, dtype=torch.int32)
    K.packed_rows(cu, len(cu) - 1, T_CAP, start, last)
    return cu, start, last


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_packed_rows_host(layout):
    cu, start, last = _rows_host(layout)
    want = list(range(T_CAP))
    for a, e in zip(cu[:-1].tolist(), cu[1:].tolist()):
        want[a:e] = [a] * (e - a)
    assert start.tolist() == want
    assert last.tolist() == [max(e - 1, 0) for e in cu[1:].tolist()]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_packed_rows_device(layout):
    dev = torch.device("cuda", 0)
    cu, start, last = _rows_host(layout)
    dstart, dlast = torch.empty_like(start, device=dev), torch.empty_like(last, device=dev)
    K.packed_rows(cu.to(dev), len(cu) - 1, T_CAP, dstart, dlast)
    assert torch.equal(dstart.cpu(), start) and torch.equal(dlast.cpu(), last)


# ----------------------------------------------------------------------------- lowering, model
SPEC, FETCH = {"item_ids:0": ((3, 16), "INT32")}, ["top_k:0", "top_k:1"]


def _ids(S):
    ids = torch.randint(1, CFG.num_items, (3, S), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    ids[0, :S // 3] = 0      # left pads: some, all but one event, none
    ids[1, :S - 1] = 0
    return ids


def test_packed_plan_lowers_strict_and_matches_interpreter():
    g = Graph.from_graph_def(next_item_graph_def(CFG, 16, 4, seed=1))
    plan = PackedFunction(g, SPEC, FETCH, "cpu", strict=True, pack_causal=True, capacities=[16, 32, 48])
    s = plan.summary()
    assert s["glue_ops"] == [] and s["kinds"]["packed_rows"] == 1, s
    assert (s["kinds"]["packed_causal_attention"], s["kinds"]["last_attention"], s["kinds"]["retrieve"]) == (1, 1, 1), s
    vals, idxs = plan({"item_ids:0": _ids(16)})
    assert plan.current.token_cap == 32  # 10 + 1 + 16 events
    ref_scores, ref_vals = Session(g).run(["scores:0", "top_k:0"], {"item_ids:0": _ids(16)})
    torch.testing.assert_close(vals.float(), ref_vals, atol=2e-3, rtol=2e-2)
    torch.testing.assert_close(vals.float(), ref_scores.gather(1, idxs.long()), atol=2e-3, rtol=2e-2)


def test_causal_packing_is_opt_in_and_other_positions_are_refused():
    g = Graph.from_graph_def(next_item_graph_def(CFG, 16, 4, seed=1))
    with pytest.raises(CompileError):
        PackedFunction(g, SPEC, FETCH, "cpu", strict=True, capacities=[16, 32, 48])
    g3 = Graph.from_graph_def(next_item_graph_def(CFG, 16, 4, seed=1, query_pos=3))
    with pytest.raises(CompileError):
        PackedFunction(g3, SPEC, FETCH, "cpu", strict=True, pack_causal=True, capacities=[16, 32, 48])


@pytest.mark.gpu
def test_packed_model_matches_padded_model():
    sessions = [r[r != 0].tolist() for r in _ids(80)]  # a sequence crosses a tile
    got = []
    for pack in (False, True):
        m = NextItemModel(CFG, seq_len=80, top_k=4, buckets=(4,), seed=1, device="cuda:0", lanes=1, pack_tokens=pack)
        m.open()
        try:
            got.append(torch.tensor([[s for s, _ in row] for row in m.recommend(sessions)]))
        finally:
            m.close()
    torch.testing.assert_close(got[1], got[0], atol=2e-3, rtol=2e-2)
