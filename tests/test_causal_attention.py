"""Causal attention: the ``causal_attention`` lowering and the next-item model on the host, and
``kernels/attention_causal.hip`` on the GPU against plain float64 attention — exact selection data
(every output row is one chosen V row, integers) and continuous data with a derived bound."""
import functools

import numpy as np
import pytest
import torch

from flink_tensorflow_amd.graph.compiler import CompiledFunction
from flink_tensorflow_amd.graph.graph import Graph
from flink_tensorflow_amd.graph.plan import CompileError
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.models.zoo.next_item import NextItemConfig, next_item_graph_def
from flink_tensorflow_amd.ops import kernels as K

F64, BF, D = torch.float64, torch.bfloat16, 64
CFG = NextItemConfig(num_items=64, hidden=64, heads=1, layers=2, intermediate=128)


# ----------------------------------------------------------------------------- lowering, model
def _check_model(device, S):
    """Strict plan of the tiny model: two causal_attention steps, one retrieve, no glue, and the
    top-k scores of the fp32 interpreter (indices may swap between near-equal scores)."""
    g = Graph.from_graph_def(next_item_graph_def(CFG, S, 4, seed=1))
    ids = torch.randint(1, CFG.num_items, (3, S), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    ids[0, :S // 3] = 0      # left pads: some, all but one event, none
    ids[1, :S - 1] = 0
    plan = CompiledFunction(g, {"item_ids:0": ((3, S), "INT32")}, ["top_k:0", "top_k:1"], device, strict=True)
    s = plan.summary()
    assert s["kinds"]["causal_attention"] == 2 and s["kinds"]["retrieve"] == 1 and s["glue_ops"] == [], s
    vals, idxs = (t.cpu() for t in plan({"item_ids:0": ids.to(device)}))
    ref_scores, ref_vals = Session(g).run(["scores:0", "top_k:0"], {"item_ids:0": ids})
    torch.testing.assert_close(vals.float(), ref_vals, atol=2e-3, rtol=2e-2)
    torch.testing.assert_close(vals.float(), ref_scores.gather(1, idxs.long()), atol=2e-3, rtol=2e-2)


def test_tiny_model_lowers_strict_and_matches_interpreter():
    _check_model("cpu", 16)


@pytest.mark.gpu
def test_model_on_device_two_key_blocks():
    _check_model(torch.device("cuda", 0), 80)


def _flipped(S):
    t = np.tril(np.ones((S, S), np.float32))
    t[S // 2, 1] = 0.0
    return t


@pytest.mark.parametrize("const", [lambda S: np.triu(np.ones((S, S), np.float32)),
                                   lambda S: np.tril(np.ones((S, S), np.float32), -1), _flipped],
                         ids=["upper", "strict_lower", "flipped_entry"])
def test_wrong_constants_do_not_match(const):
    g = Graph.from_graph_def(next_item_graph_def(CFG, 16, 4, seed=1, causal_const=const(16)[None, None]))
    spec = {"item_ids:0": ((3, 16), "INT32")}
    with pytest.raises(CompileError):
        CompiledFunction(g, spec, ["top_k:0"], "cpu", strict=True)
    assert "causal_attention" not in CompiledFunction(g, spec, ["top_k:0"], "cpu").summary()["kinds"]


def test_packing_is_declined():
    from flink_tensorflow_amd.graph.packed import try_packed

    g = Graph.from_graph_def(next_item_graph_def(CFG, 16, 4, seed=1))
    assert try_packed(g, {"item_ids:0": ((3, 16), "INT32")}, ["top_k:0"], "cpu", strict=True) is None
    with pytest.raises(ValueError):
        K.attention(torch.zeros(4, 192, dtype=BF), None, 1, 4, 1, cu_seqlens=torch.tensor([0, 4], dtype=torch.int32),
                    causal=True)


# ----------------------------------------------------------------------------- kernel
def attention_f64(qkv, valid, B, S, H):
    """Plain causal attention in float64: key j of a sequence is admissible for query i iff
    ``j <= i`` and ``valid[b, j]``; a query with no admissible key gives a zero row."""
    q, k, v = qkv.to(F64).reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
    ok = valid[:, None, None, :] & torch.ones(S, S, dtype=torch.bool).tril()
    s = ((q @ k.transpose(-1, -2)) * 0.125).masked_fill(~ok, float("-inf"))
    return (torch.softmax(s, -1).nan_to_num(0.0) @ v).permute(0, 2, 1, 3).reshape(B * S, H * D)


def _valid(S, pattern, g, B=2):
    valid = torch.ones(B, S, dtype=torch.bool)
    if pattern == "right":
        valid[0, S - S // 3:] = False
        valid[1, (S + 1) // 2:] = False
    elif pattern == "left":      # the leading queries of both sequences have no admissible key
        valid[0, :max(1, S // 3)] = False
        valid[1, :S // 2] = False
    elif pattern == "holes":
        valid = torch.rand(B, S, generator=g) >= 0.3
        valid[1, 0] = False
    return valid


def _codes(idx, h):
    """[..., 64] in {+-1}: the 8 bits of ``idx ^ 0x55 h`` eight times; distinct ids differ in >= 8 places."""
    bits = (((idx ^ (0x55 * h))[..., None] >> torch.arange(8)) & 1) * 2 - 1
    return bits.repeat_interleave(8, -1).to(F64)


@functools.lru_cache(maxsize=None)
def exact_case(S, pattern, B=2, H=2):
    """Keys carry +-1 codes, query i is 512 x the code of its target t(i), an admissible key; the
    logit gap to any other code is >= 1024, so every other float64 softmax weight is exactly 0 and
    the output row is V[t(i)] (integers, |v| <= 32).  Among a sequence's n valid keys (by rank) the
    first h = n // 2 + 1 have fresh codes and rank r >= h repeats the code of rank r - h: a decoy
    for every query before it, and every other query targets the rank whose repeat is the very next
    valid key.  Pad keys repeat codes of valid keys too.  Decoys have V rows of their own."""
    g = torch.Generator().manual_seed(1000 * S + len(pattern))
    valid = _valid(S, pattern, g, B)
    v = torch.randint(-32, 33, (B, S, H * D), generator=g).to(F64)
    kidx = torch.zeros(B, S, dtype=torch.long)
    qidx = torch.zeros(B, S, dtype=torch.long)
    want = torch.zeros(B, S, H * D, dtype=F64)
    for b in range(B):
        pos = valid[b].nonzero().flatten()
        n = pos.numel()
        h = n // 2 + 1
        kidx[b] = torch.arange(S) % h                        # pad keys (overwritten for valid ones)
        kidx[b, pos] = torch.arange(n) % h
        for i in range(S):
            a = int((pos <= i).sum())                         # admissible keys of query i
            if a == 0:
                continue
            lo, hi = max(0, a - h), min(a - 1, h - 1)         # ranks whose code has one admissible key
            t = lo if i % 2 else int(torch.randint(lo, hi + 1, (1,), generator=g))
            qidx[b, i] = t
            want[b, i] = v[b, pos[t]]
    q = torch.cat([512 * _codes(qidx, h) for h in range(H)], -1)
    k = torch.cat([_codes(kidx, h) for h in range(H)], -1)
    ids = torch.where(valid, torch.randint(1, 30000, (B, S), generator=g), torch.zeros(B, S, dtype=torch.long))
    return dict(qkv=torch.cat([q, k, v], -1).reshape(B * S, 3 * H * D), ids=ids.reshape(-1).to(torch.int32),
                valid=valid, want=want.reshape(B * S, H * D), B=B, S=S, H=H)


def _run(d, dev):
    out = K.attention(d["qkv"].to(BF).to(dev), d["ids"].to(dev), d["B"], d["S"], d["H"], causal=True)
    return out.cpu().to(F64)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["none", "right", "left", "holes"])
@pytest.mark.parametrize("S", [1, 16, 17, 63, 64, 65, 129, 200])
def test_exact_selection(S, pattern):
    d = exact_case(S, pattern)
    assert torch.equal(attention_f64(d["qkv"], d["valid"], d["B"], S, d["H"]), d["want"])
    assert torch.equal(_run(d, torch.device("cuda", 0)), d["want"])


@pytest.mark.gpu
@pytest.mark.parametrize("S", [65, 192])
def test_continuous_data(S):
    """Peaked logits (standard deviation ~9).  P is rounded to bf16 before PV and the output once:
    each step contributes at most 2^-9 max|V|; the fp32 accumulation terms are of order S 2^-22."""
    B, H = 2, 2
    g = torch.Generator().manual_seed(S)
    x = torch.randn(B * S, 3, H, D, generator=g, dtype=F64)
    x[:, :2] *= 3
    qkv = x.reshape(B * S, 3 * H * D).to(BF).to(F64)
    valid = _valid(S, "holes", g, B)
    valid[0, :5] = False
    ids = valid.reshape(-1).to(torch.int32) * 7
    ref = attention_f64(qkv, valid, B, S, H)
    got = _run(dict(qkv=qkv, ids=ids, B=B, S=S, H=H), torch.device("cuda", 0))
    err, bound = float((got - ref).abs().max()), 1.05 * 2.0 ** -8 * float(qkv[:, 2 * H * D:].abs().max())
    print(f"S={S}: max abs error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
