"""Attention with 32- and 128-wide heads: the lowering and the zoo model on the host, and the
encoder, causal and first-token kernels on the GPU against plain float64 attention (exact selection
data in NaN-guarded buffers, continuous data with the project's ``1.05 * 2^-8 * max|V|`` bound)."""
import functools

import pytest
import torch

from flink_tensorflow_amd.graph.compiler import CompiledFunction
from flink_tensorflow_amd.graph.graph import Graph
from flink_tensorflow_amd.graph.packed import PackedFunction
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.models.zoo.bert import BertConfig, reference_forward
from flink_tensorflow_amd.models.zoo.bert_graph import bert_graph_def
from flink_tensorflow_amd.models.zoo.next_item import NextItemConfig, next_item_graph_def
from flink_tensorflow_amd.ops import kernels as K

F64, BF = torch.float64, torch.bfloat16
TOL = dict(atol=2e-3, rtol=2e-2)  # test_tiny_model_lowers_strict_and_matches_interpreter's, for the 64-wide model
DH = [(32, 1), (32, 2), (32, 3), (128, 2)]  # (head dim, heads); an odd H at 32 leaves the last pair one head
GUARD = 64  # NaN elements on either side of qkv and of out


# ----------------------------------------------------------------------------- host: lowering, model
@pytest.mark.parametrize("hidden,heads,head_dim", [(64, 2, 32), (128, 1, 128)])
def test_next_item_model_lowers_strict(hidden, heads, head_dim):
    cfg = NextItemConfig(num_items=64, hidden=hidden, heads=heads, head_dim=head_dim, layers=2, intermediate=128)
    g = Graph.from_graph_def(next_item_graph_def(cfg, 16, 4, seed=1))
    ids = torch.randint(1, cfg.num_items, (3, 16), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    ids[0, :5] = 0
    ids[1, :15] = 0
    plan = CompiledFunction(g, {"item_ids:0": ((3, 16), "INT32")}, ["top_k:0", "top_k:1"], "cpu", strict=True)
    s = plan.summary()
    assert s["kinds"]["causal_attention"] == 2 and s["glue_ops"] == [], s
    vals, idxs = plan({"item_ids:0": ids})
    ref_scores, ref_vals = Session(g).run(["scores:0", "top_k:0"], {"item_ids:0": ids})
    torch.testing.assert_close(vals.float(), ref_vals, **TOL)
    torch.testing.assert_close(vals.float(), ref_scores.gather(1, idxs.long()), **TOL)


def test_packed_encoder_with_32_wide_heads():
    cfg = BertConfig.tiny(heads=4)  # hidden 128: 32-wide heads
    gd, w = bert_graph_def(cfg, 16, seed=3, mask_from_ids=True)
    pf = PackedFunction(Graph.from_graph_def(gd), {"input_ids:0": ((4, 16), "INT32")}, ["logits:0"], "cpu",
                        strict=True, granule=16)
    s = pf.plans[64].summary()
    assert s["glue_ops"] == [] and s["kinds"]["attention"] == 1 and s["kinds"]["cls_attention"] == 1, s
    ids = torch.randint(1, cfg.vocab_size, (4, 16), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    for b in range(4):
        ids[b, 6 + 3 * b:] = 0
    torch.testing.assert_close(pf({"input_ids:0": ids})[0], reference_forward(w, cfg, ids), **TOL)


def test_other_widths_stay_on_the_host_and_config_rule():
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(8, 3 * 2 * 48, generator=g).to(BF)  # Dh = 48
    cu = torch.tensor([0, 5, 8], dtype=torch.int32)
    ctx = K.attention(qkv, None, 2, 5, 2, cu_seqlens=cu)
    first = K.cls_attention(qkv, cu, 2, 5, 2)
    assert ctx.shape == (8, 96) and torch.equal(first, ctx[[0, 5]])
    with pytest.raises(ValueError):
        NextItemConfig(hidden=96, heads=3, head_dim=32)


@pytest.mark.gpu
def test_other_widths_are_refused_on_the_gpu():
    dev = torch.device("cuda", 0)
    qkv, cu = torch.zeros(8, 3 * 2 * 48, dtype=BF, device=dev), torch.tensor([0, 5, 8], dtype=torch.int32, device=dev)
    for call in (lambda: K.attention(qkv, None, 2, 5, 2, cu_seqlens=cu), lambda: K.cls_attention(qkv, cu, 2, 5, 2),
                 lambda: K.attention(qkv, torch.ones(8, dtype=torch.int32, device=dev), 2, 4, 2, causal=True)):
        with pytest.raises(ValueError, match="32, 64, 128"):
            call()


# ----------------------------------------------------------------------------- float64 reference
def attention_f64(qkv, valid, H, D, causal, first_only=False):
    """Plain attention of ONE sequence in float64: ``qkv`` [n, 3 H D], key j admissible iff
    ``valid[j]`` (and ``j <= i`` when causal); no admissible key gives a zero row."""
    n = qkv.shape[0]
    q, k, v = qkv.to(F64).reshape(n, 3, H, D).permute(1, 2, 0, 3)
    ok = valid[None, :].expand(n, n) & (torch.ones(n, n, dtype=torch.bool).tril() if causal else True)
    s = ((q @ k.transpose(-1, -2)) / D ** 0.5).masked_fill(~ok, float("-inf"))
    o = (torch.softmax(s, -1).nan_to_num(0.0) @ v).permute(1, 0, 2).reshape(n, H * D)
    return o[:1] if first_only else o


def _valid(S, pattern, g):
    if pattern == "left":  # the leading queries of both sequences have no admissible key
        v = torch.ones(2, S, dtype=torch.bool)
        v[0, :max(1, S // 3)] = False
        v[1, :S // 2] = False
        return list(v)
    v = torch.rand(2, S, generator=g) >= 0.3  # holes
    v[1, 0] = False
    return list(v)


def _codes(idx, h, D):
    """[..., D] in {+-1}: the 8 bits of ``idx ^ 0x55 h``, each D / 8 times; distinct ids differ in >= D / 8 places."""
    bits = (((idx ^ (0x55 * h))[..., None] >> torch.arange(8)) & 1) * 2 - 1
    return bits.repeat_interleave(D // 8, -1).to(F64)


def _sequence(valid, H, D, causal, g, first_only=False):
    """``exact_case`` of test_causal_attention.py for one sequence and any D: keys carry +-1 codes,
    query i is (1024 at D = 32, 512 at D = 128) x the code of its target, an admissible key, so the
    logit gap is ~1448 and every output row is the target's V row (integers, |v| <= 32).  Causal:
    the first h = n // 2 + 1 valid keys have fresh codes and rank r >= h repeats rank r - h, a decoy
    for every query before it.  Not causal: every key is admissible to every query, so all n <= 255
    codes are fresh; ``first_only`` (up to 512 keys) gives the first query's target code 255 and
    lets the other keys share the rest."""
    S = valid.numel()
    pos = valid.nonzero().flatten()
    n = pos.numel()
    h = n // 2 + 1 if causal else max(n, 1)
    v = torch.randint(-32, 33, (S, H * D), generator=g).to(F64)
    kidx, qidx, want = torch.arange(S) % h, torch.zeros(S, dtype=torch.long), torch.zeros(S, H * D, dtype=F64)
    kidx[pos] = torch.arange(n) % h
    if first_only and S:
        t = int(torch.randint(0, S, (1,), generator=g))
        kidx, qidx[0], want[0] = torch.arange(S) % 255, 255, v[t]
        kidx[t] = 255
    for i in range(0 if first_only else S):
        a = int((pos <= i).sum()) if causal else n  # admissible keys of query i
        if a:
            lo, hi = max(0, a - h), min(a - 1, h - 1)  # ranks whose code has one admissible key
            qidx[i] = lo if i % 2 else int(torch.randint(lo, hi + 1, (1,), generator=g))
            want[i] = v[pos[qidx[i]]]
    mult = {32: 1024, 128: 512}[D]
    q = torch.cat([mult * _codes(qidx, hh, D) for hh in range(H)], -1)
    k = torch.cat([_codes(kidx, hh, D) for hh in range(H)], -1)
    return torch.cat([q, k, v], -1), (want[:1] if first_only else want)


@functools.lru_cache(maxsize=None)
def exact_case(D, H, S, pattern, kind):
    """Sequences, their valid masks, qkv rows and expected rows; the float64 reference must give them."""
    g = torch.Generator().manual_seed(1000 * S + 10 * D + H)
    if kind == "packed":
        valids = [torch.ones(n, dtype=torch.bool) for n in (S, 0, 1, S // 2 + 1)]
    elif kind == "cls":
        valids = [torch.ones(n, dtype=torch.bool) for n in (1, 0, 64, 65, 512)]
    else:
        valids = _valid(S, pattern, g)
    seqs = [_sequence(v, H, D, kind == "causal", g, kind == "cls") for v in valids]
    for v, (x, want) in zip(valids, seqs):
        if v.numel():
            assert torch.equal(attention_f64(x, v, H, D, kind == "causal", kind == "cls"), want)
    empty = torch.zeros(int(kind == "cls"), H * D, dtype=F64)  # cls: a zero row; packed: no row at all
    return valids, torch.cat([x for x, _ in seqs]), torch.cat([w if v.numel() else empty for v, (_, w) in zip(valids, seqs)])


def _guarded(rows, cols, dev, fill=None):
    """A [rows, cols] bf16 view inside a NaN-filled buffer (a read or write of a head that does not exist shows)."""
    buf = torch.full((rows * cols + 2 * GUARD,), float("nan"), dtype=BF, device=dev)
    view = buf[GUARD:GUARD + rows * cols].view(rows, cols)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _run(D, H, S, valids, qkv, kind):
    dev = torch.device("cuda", 0)
    _, x = _guarded(qkv.shape[0], 3 * H * D, dev, qkv.to(BF))
    cu = torch.tensor([0] + [v.numel() for v in valids], dtype=torch.int32).cumsum(0).to(torch.int32).to(dev)
    buf, out = _guarded(len(valids) if kind == "cls" else qkv.shape[0], H * D, dev)
    if kind == "cls":
        K.cls_attention(x, cu, len(valids), 512, H, out=out)
    elif kind == "packed":
        K.attention(x, None, len(valids), S, H, out=out, cu_seqlens=cu)
    else:
        ids = (torch.cat(valids).to(torch.int32) * 7).to(dev)
        K.attention(x, ids, len(valids), S, H, out=out, causal=kind == "causal")
    torch.cuda.synchronize()
    assert buf[:GUARD].isnan().all() and buf[-GUARD:].isnan().all()
    return out.cpu().to(F64)


# ----------------------------------------------------------------------------- GPU: kernels
@pytest.mark.gpu
@pytest.mark.parametrize("kind,pattern", [("causal", "left"), ("causal", "holes"), ("encoder", "left"),
                                          ("encoder", "holes"), ("packed", "-")])
@pytest.mark.parametrize("S", [1, 17, 64, 65, 129, 200])
@pytest.mark.parametrize("D,H", DH)
def test_exact_selection(D, H, S, kind, pattern):
    valids, qkv, want = exact_case(D, H, S, pattern, kind)
    assert torch.equal(_run(D, H, S, valids, qkv, kind), want)


@pytest.mark.gpu
@pytest.mark.parametrize("D,H", [(32, 1), (32, 3), (128, 1), (128, 3)])
def test_cls_attention_exact(D, H):
    """Lengths 1, 0, 64, 65 and 512 in one packed batch; the empty sequence gives a zero row."""
    valids, qkv, want = exact_case(D, H, 512, "-", "cls")
    assert not want[1].any() and torch.equal(_run(D, H, 512, valids, qkv, "cls"), want)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "encoder"])
@pytest.mark.parametrize("S", [65, 192])
@pytest.mark.parametrize("D,H", DH)
def test_continuous_data(D, H, S, causal):
    """Peaked logits (standard deviation ~9).  P is rounded to bf16 before PV and the output once:
    each step contributes at most 2^-9 max|V|, whatever D; the fp32 accumulation terms are of order S 2^-22."""
    g = torch.Generator().manual_seed(S + D + H)
    x = torch.randn(2 * S, 3, H, D, generator=g, dtype=F64)
    x[:, :2] *= 3
    qkv = x.reshape(2 * S, 3 * H * D).to(BF).to(F64)
    valids = _valid(S, "holes", g)
    valids[0][:5] = False
    ref = torch.cat([attention_f64(qkv[b * S:(b + 1) * S], valids[b], H, D, causal) for b in range(2)])
    got = _run(D, H, S, valids, qkv, "causal" if causal else "encoder")
    err, bound = float((got - ref).abs().max()), 1.05 * 2.0 ** -8 * float(qkv[:, 2 * H * D:].abs().max())
    print(f"D={D} H={H} S={S} causal={causal}: max abs error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
