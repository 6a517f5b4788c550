"""Ranking on 8-bit tables (kernels/interact_fp8.hip, ``K.quantize_table_fp8``, ``table_precision="fp8"``).

A row is e4m3 codes times ``2^k``, ``-32 <= k <= 31``: every value is exactly a bf16, so nothing here has a
tolerance.  The geometry tests use the exact data of ``test_ranking.py`` (entries in {-1, 0, 1}, here as the codes
0xB8 / 0x00 / 0x38 under row exponents in -2..2, so ``Z = 2^(k_i + k_j) n`` with ``|n| <= 256`` is exact) and its
float64 mirror; guard rows hold the NaN code 0x7F and guard exponents 127.
"""
import numpy as np
import pytest
import torch

from flink_tensorflow_amd.graph.builder import GraphBuilder
from flink_tensorflow_amd.graph.compiler import CompiledFunction
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.models.core import GraphDefGraphLoader
from flink_tensorflow_amd.models.zoo import DLRMModel, dlrm_graph_def
from flink_tensorflow_amd.ops import kernels as K
from test_ranking import BF, DIM, HID, NAN, VOCAB, _data, _mirror, _model, _operands, _pairs

FINITE = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)  # the 254 codes that are numbers


def _values(codes, exps):
    """float64, from the definition."""
    return torch.ldexp(codes.cpu().view(torch.float8_e4m3fn).double(), exps.cpu().long()[:, None])


def test_quantiser():
    codes = FINITE[torch.arange(64 * 16) % 254].reshape(64, 16).clone()
    codes[:, 0] = 0x7E  # 448: the row's exponent is the smallest one that holds it
    exps = torch.arange(-32, 32, dtype=torch.int8)
    table = torch.cat([_values(codes, exps), torch.zeros(1, 16, dtype=torch.float64),
                       torch.tensor([[448.0 * 2.0 ** 40, -2.0 ** 80] + [1.0] * 14], dtype=torch.float64)])
    qc, qe = K.quantize_table_fp8(table)
    assert qc.dtype == torch.uint8 and qe.dtype == torch.int8
    assert torch.equal(qc[:64], codes) and torch.equal(qe[:64], exps)
    assert int(qe[64]) == 0 and not bool(qc[64].any())
    assert int(qe[65]) == 31 and qc[65, :2].tolist() == [0x7E, 0xFE]  # saturated
    assert bool(((qc & 0x7F) != 0x7F).all())
    assert torch.equal(K.dequantize_table_fp8(qc[:64], qe[:64]).double(), table[:64])


@pytest.mark.gpu
def test_every_code():
    """Record ``b`` selects the rows whose column 0 holds code ``b`` (field 0) and ``253 - b`` (field 1)."""
    dev = torch.device("cuda", 0)
    codes = torch.zeros((508, 16), dtype=torch.uint8)
    codes[:, 0] = FINITE.repeat(2)
    exps = ((torch.arange(508) * 7) % 64 - 32).to(torch.int8)
    ids = torch.stack([torch.arange(254), 253 - torch.arange(254)], 1).to(torch.int32)
    meta = torch.tensor([(0, -1, 0), (0, 0, 254), (254, 1, 254)], dtype=torch.int64).t().contiguous()
    dense = torch.zeros((254, 16), dtype=BF)
    dense[:, 0] = 1.0
    got = K.dot_interact(codes.to(dev), ids.to(dev), meta.to(dev), K.dot_interact_lut(3, [(1, 0), (2, 0)]).to(dev), 2,
                         dense.to(dev), table_exp=exps.to(dev)).cpu()
    vals = _values(codes, exps)[:, 0]
    want = torch.stack([vals[:254], vals[254:].flip(0)], 1)
    assert not bool(torch.isnan(got).any()) and torch.equal(got[:, :2].double(), want) and not bool(got[:, 2:].any())


# D: the 8-byte tail alone (16), one load + tail and an odd step count (48), the full line (128), the maximum (256);
# M: one and two row groups; B > 4 with one workgroup: a wave takes a second and a third record, with and without
# the row prefetch (<4, 2> and <16, 2> have none); the activation vector first, last and absent
@pytest.mark.gpu
@pytest.mark.parametrize("B,M,D,workgroups,dense_row,copy,bad_ids", [
    (1, 2, 16, None, 0, True, False), (5, 27, 128, 1, 0, True, False), (9, 33, 48, 1, 32, False, False),
    (9, 64, 256, 1, 0, True, False), (9, 27, 256, 1, None, False, False), (5, 33, 128, 1, 0, False, False),
    (9, 64, 48, None, 63, True, True)])
def test_geometry(B, M, D, workgroups, dense_row, copy, bad_ids):
    """``test_ranking._check_interact`` on an 8-bit table with the same rows, guards and slot."""
    dev = torch.device("cuda", 0)
    tables, ids, cols, dense = _data(B, M, D, dense_row, seed=B + M + D, bad_ids=bad_ids)
    pairs = _pairs(M, "lower")
    table, ids_d, meta, lut, dense_d = _operands(tables, ids, cols, dense, dense_row, pairs, copy, dev)
    t = table.cpu().float()
    guard = torch.isnan(t[:, 0])
    codes = torch.where(torch.isnan(t), 0x7F, torch.where(t > 0, 0x38, torch.where(t < 0, 0xB8, 0))).to(torch.uint8)
    exps = torch.from_numpy(np.random.default_rng(M).integers(-2, 3, len(t))).to(torch.int8)
    exps[guard] = 127
    bases = [int(b) for b, c in zip(meta[0].tolist(), meta[1].tolist()) if c >= 0]
    scaled = [tb * 2.0 ** exps[b:b + len(tb)].double().numpy()[:, None] for tb, b in zip(tables, bases)]
    want = _mirror(scaled, ids, cols, dense, dense_row, pairs, copy)
    wlog = want.shape[1]
    wout = -(-wlog // 8) * 8
    runs = []
    for _ in range(2):
        buf = torch.full((B + 2, wout + 24), NAN, dtype=BF, device=dev)
        K.dot_interact(codes.to(dev), ids_d, meta, lut, wlog, dense_d, copy, out=buf[1:-1, 16:16 + wout], workgroups=workgroups,
                       table_exp=exps.to(dev))
        runs.append(buf.cpu())
    got = runs[0][1:-1, 16:16 + wout]
    assert torch.equal(got[:, :wlog], want) and bool((got[:, wlog:] == 0).all())
    outside = runs[0].clone()
    outside[1:-1, 16:16 + wout] = NAN
    assert bool(torch.isnan(outside).all())
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16))


def _random_table(rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    return FINITE[torch.randint(0, 254, (rows, D), generator=g)], torch.randint(-32, 32, (rows,), generator=g).to(torch.int8)


@pytest.mark.gpu
@pytest.mark.parametrize("B,M,D,data", [(9, 27, 128, "random"), (6, 40, 80, "random"), (6, 40, 80, "cancel"), (6, 27, 48, "cancel"),
                                        (6, 27, 112, "cancel")])
def test_equals_bf16_kernel(B, M, D, data):
    """fp32 rounds once per MFMA, so the bits are those of ``interact.hip`` only if every step sums the columns that
    kernel's step sums.  ``cancel`` makes that show: columns 0 and D / 2, both in its step 0, hold +-448 and all others
    stay below 0.25 under exponents 0..2.  Where the two large products cancel inside one step the small ones survive;
    split over two steps they are first rounded away next to 2^17.  ``random``: all codes, all exponents."""
    dev = torch.device("cuda", 0)
    F, V = M - 1, 5
    codes, exps = _random_table(F * V, D, M)
    g = torch.Generator().manual_seed(D)
    ids = torch.randint(0, V, (B, F), generator=g).to(torch.int32).to(dev)
    dense = torch.randn((B, D), generator=g)
    if data == "cancel":
        small = FINITE[(FINITE & 0x7F) < 0x28]
        codes, exps = small[torch.randint(0, len(small), codes.shape, generator=g)], torch.randint(0, 3, exps.shape, generator=g).to(torch.int8)
        codes[:, 0], codes[:, D // 2] = 0x7E, FINITE[126 + 127 * torch.randint(0, 2, (F * V,), generator=g)]  # 448, +-448
        dense = dense * 0.1
        dense[:, 0], dense[:, D // 2] = 448.0, -448.0
    dense = dense.to(BF).to(dev)
    meta = torch.tensor([(0, -1, 0)] + [(f * V, f, V) for f in range(F)], dtype=torch.int64).t().contiguous().to(dev)
    pairs = _pairs(M, "lower")
    args = (ids, meta, K.dot_interact_lut(M, pairs, D).to(dev), D + len(pairs), dense, True)
    got = K.dot_interact(codes.to(dev), *args, workgroups=1, table_exp=exps.to(dev))
    want = K.dot_interact(K.dequantize_table_fp8(codes, exps).to(dev), *args, workgroups=1)
    assert not bool(torch.isnan(got).any()) and torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 144])
def test_embed_rows(D):
    dev = torch.device("cuda", 0)
    V, R = 17, 37
    codes = torch.full((V + 4, D), 0x7F, dtype=torch.uint8)
    codes[2:2 + V] = FINITE[torch.arange(V * D) % 254].reshape(V, D)
    exps = torch.full((V + 4,), 127, dtype=torch.int8)
    exps[2:2 + V] = ((torch.arange(V) * 7) % 64 - 32).to(torch.int8)
    ids = torch.from_numpy(np.random.default_rng(D).integers(0, V, R).astype(np.int32))
    ids[[0, 5, 36]] = torch.tensor([-1, V, 2 ** 31 - 1], dtype=torch.int32)
    buf = torch.full((R + 2, D + 24), NAN, dtype=BF, device=dev)
    K.embed_rows(codes.to(dev), ids.to(dev), base=2, vocab=V, out=buf[1:-1, 16:16 + D], table_exp=exps.to(dev))
    ok = (ids >= 0) & (ids < V)
    want = torch.where(ok[:, None], K.dequantize_table_fp8(codes[2:2 + V], exps[2:2 + V])[ids.clamp(0, V - 1).long()], 0.0)
    got = buf.cpu()
    assert torch.equal(got[1:-1, 16:16 + D].view(torch.int16), want.to(BF).view(torch.int16))
    got[1:-1, 16:16 + D] = NAN
    assert bool(torch.isnan(got).all())


# ------------------------------------------------------------------ plans and the model
def _plan(w, B, device, **kw):
    g = GraphDefGraphLoader(dlrm_graph_def(13, VOCAB, DIM, (DIM,), (HID, 1), weights=w)).load()
    feeds = {"dense:0": ((B, 16), "FLOAT"), "ids:0": ((B, 3), "INT32")}
    return g, CompiledFunction(g, feeds, ["logit:0"], device, strict=True, **kw)


def _check_plan_and_model(device):
    B = 9
    w, dense, ids = _model(B)
    fed = {"dense:0": torch.from_numpy(dense), "ids:0": torch.from_numpy(ids)}
    on = {k: v.to(device) for k, v in fed.items()}
    g, plan = _plan(w, B, device, table_precision="fp8")  # +-1 entries quantise exactly: the interpreter's logits
    assert plan.summary()["kinds"] == _plan(w, B, device)[1].summary()["kinds"]
    assert [s.meta.get("tables") for s in plan.steps if s.kind == "interact"] == ["fp8"]
    ref = torch.as_tensor(Session(g, device=torch.device("cpu")).run(["logit:0"], fed)[0])
    assert torch.equal(plan(on)[0].cpu().float(), ref)
    # normally distributed tables: the bf16 plan of the dequantised quantisation, bit for bit
    rng = np.random.default_rng(7)
    wn = {**w, **{f"emb{f}": rng.normal(0.0, 0.3, (V, DIM)).astype(np.float32) for f, V in enumerate(VOCAB)}}
    wq = {**wn, **{f"emb{f}": K.dequantize_table_fp8(*K.quantize_table_fp8(torch.from_numpy(wn[f"emb{f}"]))).float().numpy()
                   for f in range(len(VOCAB))}}
    assert any(not np.array_equal(wn[f"emb{f}"], wq[f"emb{f}"]) for f in range(len(VOCAB)))
    got, want = _plan(wn, B, device, table_precision="fp8")[1](on)[0], _plan(wq, B, device)[1](on)[0]
    assert torch.equal(got.cpu().view(torch.int16), want.cpu().view(torch.int16))
    m = DLRMModel(13, VOCAB, DIM, (DIM,), (HID, 1), buckets=(4, 16), weights=w, device=device, table_precision="fp8")
    m.open()
    try:
        probs = torch.tensor(m.rank(dense[:, :13], ids), dtype=torch.float64)
        assert float((probs - torch.sigmoid(ref.double()).reshape(-1)).abs().max()) <= 2.0 ** -8
        assert all(any(s.meta.get("tables") == "fp8" for s in p.steps) for p in (m._plans or {}).values())
    finally:
        m.close()


def _check_lone_lookups(device):
    """A ``D = 16`` lookup becomes an 8-bit ``embed`` step, a ``D = 8`` one keeps its bf16 table."""
    gb = GraphBuilder()
    rng = np.random.default_rng(5)
    ta, tb = rng.integers(-1, 2, (6, 8)).astype(np.float32), rng.integers(-1, 2, (6, 16)).astype(np.float32)
    ids_t = gb.placeholder("ids", "INT32", [4, 3])
    gb.concat([gb.embedding_lookup(gb.constant("ta", ta), ids_t, name="a"), gb.embedding_lookup(gb.constant("tb", tb), ids_t, name="b")],
              -1, name="both")
    plan = CompiledFunction(GraphDefGraphLoader(gb.build_graph_def()).load(), {"ids:0": ((4, 3), "INT32")}, ["both:0"], device,
                            strict=True, table_precision="fp8")
    ids = torch.tensor([[0, 5, 6], [-1, 2, 3], [1, 1, 4], [5, 0, 2]], dtype=torch.int32)
    ok = ((ids >= 0) & (ids < 6))[..., None]
    want = torch.cat([torch.from_numpy(ta)[ids.clamp(0, 5).long()] * ok, torch.from_numpy(tb)[ids.clamp(0, 5).long()] * ok], -1)
    assert {s.meta["D"]: s.meta.get("tables") for s in plan.steps} == {8: None, 16: "fp8"}
    assert torch.equal(plan({"ids:0": ids.to(device)})[0].cpu().float(), want)


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("check", [_check_plan_and_model, _check_lone_lookups])
def test_plans(check, device):
    """On the host too: fails before ``table_precision`` existed."""
    check(device)


@pytest.mark.parametrize("case", ["precision", "no_exp", "exp_length", "exp_dtype", "exp_range", "D24", "exp_with_bf16"])
def test_refusals(case):
    codes, exps = _random_table(4, 24 if case == "D24" else 16, 0)
    exps = {"no_exp": None, "exp_length": exps[:3], "exp_dtype": exps.to(torch.int32), "exp_range": exps * 0 + 32}.get(case, exps)
    ids, meta = torch.zeros((2, 1), dtype=torch.int32), torch.tensor([[0], [0], [4]])
    with pytest.raises(ValueError):
        if case == "precision":
            _plan(_model(1)[0], 4, "cpu", table_precision="int8")
        elif case == "exp_with_bf16":
            K.embed_rows(torch.zeros((4, 16), dtype=BF), ids.reshape(-1), table_exp=exps)
        else:
            K.dot_interact(codes, ids, meta, K.dot_interact_lut(1, [(0, 0)]), 1, table_exp=exps)
    if case not in ("precision", "exp_with_bf16"):
        with pytest.raises(ValueError):
            K.embed_rows(codes, ids.reshape(-1), table_exp=exps)
