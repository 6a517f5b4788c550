"""Retrieval (kernels/retrieve.hip, graph/retrieval_lowering.py, models/zoo/two_tower.py).

Every kernel test uses exact data: operands are integers of magnitude <= 3 (exact in bf16), the
bias is multiples of 0.25, so every dot product and every score is exact in fp32 (|score| < 2^22
here) and the comparison with the float64 mirror is ``torch.equal``, values and indices.  Such
data is full of ties.

The plan's tower: features in {0, 1}, each tower column has 4 weights of +-1 and an integer bias of
magnitude <= 1, so |h0| <= 5, |h1| <= 4 * 5 + 1 = 21 and |u| <= 4 * 21 + 1 = 85: integers below
256, exact in bf16 through every layer.
"""
import numpy as np
import pytest
import torch

from flink_tensorflow_amd.graph.builder import GraphBuilder
from flink_tensorflow_amd.graph.compiler import CompiledFunction, CompileError
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.models.core import GraphDefGraphLoader
from flink_tensorflow_amd.models.zoo import RetrievalModel, two_tower_graph_def
from flink_tensorflow_amd.ops import kernels as K

IT = K.RETRIEVE_ITEM_TILE
BF = torch.bfloat16
N5 = 5 * IT + 3  # six chunks of IT, the last one partial
PLACEMENTS = ("tail", "one_chunk", "ascending", "descending", "equal", "negative")


def _data(B, N, D, placement=None, bias=True, tower=None, seed=0):
    """Exact operands ``(q, items, bias)`` as float32 arrays; ``placement`` shapes the bias (and,
    for ``equal``, the query) so that the winners lie as the name says for every query (|dot| <=
    9 D < 1024 = the step of the slopes).  ``tower = (F, H)``: the model's weights instead, ``q``
    being the 0 / 1 features."""
    rng = np.random.default_rng(seed)
    ints = lambda *s: rng.integers(-3, 4, s).astype(np.float32)  # noqa: E731
    q, items = ints(B, D), ints(N, D)
    b = rng.integers(-8, 9, N).astype(np.float32) * 0.25
    n = np.arange(N, dtype=np.float32)
    if placement == "tail":  # the last k = 10 items: the partial tile and the end of the one before
        b[N - 10:] += 4096.0
    elif placement == "one_chunk":
        b[2 * IT:3 * IT] += 4096.0
    elif placement in ("ascending", "descending"):
        b += 1024.0 * n * (1.0 if placement == "ascending" else -1.0)
    elif placement == "equal":
        q[:], b[:] = 0.0, 0.25
    elif placement == "negative":
        b -= 4096.0
    if tower is None:
        return q, items, (b if bias else None)
    F, H = tower
    w = {"items": items, "item_bias": b}
    for i, (fi, fo) in enumerate(((F, H), (H, H), (H, D))):
        w[f"w{i}"] = np.zeros((fi, fo), dtype=np.float32)
        for c in range(fo):
            w[f"w{i}"][rng.choice(fi, 4, replace=False), c] = rng.choice([-1.0, 1.0], 4)
        w[f"b{i}"] = rng.integers(-1, 2, fo).astype(np.float32)
    return rng.integers(0, 2, (B, F)).astype(np.float32), w


def _mirror(q, items, bias, k, tower=None):
    """float64: ``scores = q @ items.T + bias``, ordered by (score descending, index ascending)."""
    x = q.astype(np.float64)
    if tower is not None:
        for i in range(3):
            x = x @ tower[f"w{i}"].astype(np.float64) + tower[f"b{i}"]
            x = np.maximum(x, 0.0) if i < 2 else x
    s = x @ items.astype(np.float64).T + (0.0 if bias is None else bias.astype(np.float64))
    idx = np.stack([np.lexsort((np.arange(s.shape[1]), -row))[:k] for row in s])
    return torch.from_numpy(np.take_along_axis(s, idx, 1).astype(np.float32)), torch.from_numpy(idx.astype(np.int32))


def _graph(variant="plain", B=5, N=200, D=32, k=10):
    """``features [B, D] -> MatMul(items^T) -> BiasAdd -> TopKV2`` and its refused variants:
    ``(graph, feeds, fetches)``."""
    _, items, b = _data(B, N, D)
    gb = GraphBuilder()
    x = gb.placeholder("features", "FLOAT", [B, D])
    s = gb.bias_add(gb.matmul(x, gb.constant("items", items), transpose_b=True, name="mm"), gb.constant("b", b), name="scores")
    feeds, fetches = {"features:0": ((B, D), "FLOAT")}, ["top_k:0", "top_k:1"]
    kk = gb.constant("k", np.asarray(k, dtype=np.int32))
    if variant == "fed_k":
        kk = gb.placeholder("kfed", "INT32", [])
        feeds["kfed:0"] = ((), "INT32")
    elif variant == "fetched":
        fetches.append("scores:0")
    elif variant == "second_reader":
        gb.relu(s, name="other")
        fetches.append("other:0")
    gb.op("TopKV2", [s, kk], name="top_k", sorted=variant != "unsorted")
    return GraphDefGraphLoader(gb.build_graph_def()).load(), feeds, fetches


def _run_gpu(q, items, bias, k, chunk=None):
    dev = torch.device("cuda", 0)
    v, i = K.retrieve_topk(torch.from_numpy(q).to(dev, BF), torch.from_numpy(items).to(dev, BF), k,
                           None if bias is None else torch.from_numpy(bias).to(dev), chunk=chunk)
    return v.cpu(), i.cpu()


# N in {k, IT - 1, IT + 1, 5 IT + 3}; B in {1, 17, 65}; D in {32, 96, 256}; k in {1, 10, 100, 128} and 33 / 64
# (the 17..64 buffer class); chunk = IT: six one-tile chunks; chunk None at 5 IT + 3: chunks of 4 + 2 tiles
GEOMETRY = [(1, 1, 32, 1, None), (17, 10, 96, 10, None), (17, 100, 32, 100, None), (17, 128, 256, 128, None),
            (65, IT - 1, 32, 10, None), (17, IT + 1, 256, 1, None), (65, IT + 1, 256, 64, None),
            (65, N5, 96, 10, IT), (17, N5, 32, 100, IT), (65, N5, 256, 128, IT), (1, N5, 96, 128, IT),
            (17, N5, 96, 33, IT), (65, N5, 96, 10, None), (17, N5, 256, 100, None), (1, N5, 32, 1, IT)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,D,k,chunk", GEOMETRY)
def test_geometry(B, N, D, k, chunk):
    q, items, bias = _data(B, N, D, seed=B + N + D + k)
    v, i = _run_gpu(q, items, bias, k, chunk)
    rv, ri = _mirror(q, items, bias, k)
    assert torch.equal(i, ri) and torch.equal(v, rv)


@pytest.mark.gpu
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_placement(placement):
    """N = 5 IT + 3, chunk = IT, k = 10, B = 17.  ``tail``: the partial last tile holds 3 items, so
    the winners are the last 10 items (that tile and the end of the one before)."""
    q, items, bias = _data(17, N5, 32, placement, seed=3)
    v, i = _run_gpu(q, items, bias, 10, IT)
    rv, ri = _mirror(q, items, bias, 10)
    assert torch.equal(i, ri) and torch.equal(v, rv)
    if placement == "equal":
        assert torch.equal(i, torch.arange(10, dtype=torch.int32).expand(17, 10))
    if placement == "negative":
        assert bool((v < 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [True, False])
def test_bias_and_masking(masked):
    q, items, bias = _data(17, N5, 96, bias=masked, seed=5)
    if masked:
        bias[::3] = -np.inf
    v, i = _run_gpu(q, items, bias, 100, IT)
    rv, ri = _mirror(q, items, bias, 100)
    assert torch.equal(i, ri) and torch.equal(v, rv)
    assert not masked or (bool((i % 3 != 0).all()) and bool(torch.isfinite(v).all()))


@pytest.mark.gpu
def test_guards_and_determinism():
    """Operands between NaN bands, outputs and scratch between sentinel bands; two launches, same bits."""
    dev, G = torch.device("cuda", 0), 64
    B, N, D, k = 17, N5, 96, 10
    q, items, bias = _data(B, N, D, seed=7)

    def banded(t, fill):
        buf = torch.full((t.numel() + 2 * G,), fill, dtype=t.dtype, device=dev)
        buf[G:G + t.numel()] = t.reshape(-1).to(dev)
        return buf, buf[G:G + t.numel()].view(t.shape)

    qb, qd = banded(torch.from_numpy(q).to(BF), float("nan"))
    ib, idv = banded(torch.from_numpy(items).to(BF), float("nan"))
    need = K.retrieve_scratch_numel(B, N, k, IT)
    vb, vd = banded(torch.zeros(B, k), -7.0)
    xb, xd = banded(torch.zeros(B, k, dtype=torch.int32), -7)
    sb, sd = banded(torch.zeros(need, dtype=torch.int64), -7)
    runs = []
    for _ in range(2):
        K.retrieve_topk(qd, idv, k, torch.from_numpy(bias).to(dev), chunk=IT, out=(vd, xd), scratch=sd)
        torch.cuda.synchronize()
        runs.append((vd.cpu().clone(), xd.cpu().clone(), sd.cpu().clone()))
    for buf, fill in ((vb, -7.0), (xb, -7), (sb, -7)):
        assert bool((buf[:G] == fill).all()) and bool((buf[-G:] == fill).all())
    for buf in (qb, ib):
        assert bool(torch.isnan(buf[:G].float()).all()) and bool(torch.isnan(buf[-G:].float()).all())
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    rv, ri = _mirror(q, items, bias, k)
    assert torch.equal(runs[0][1], ri) and torch.equal(runs[0][0], rv)


def _check_plan(device):
    B, F, H, D, k = 17, 64, 64, 32, 10
    x, w = _data(B, N5, D, tower=(F, H), seed=11)
    g = GraphDefGraphLoader(two_tower_graph_def(F, (H, H), D, N5, k, weights=w)).load()
    plan = CompiledFunction(g, {"features:0": ((B, F), "FLOAT")}, ["top_k:0", "top_k:1"], device, strict=True)
    kinds = plan.summary()["kinds"]
    assert kinds["gemm"] == 3 and kinds["retrieve"] == 1 and plan.summary()["glue_ops"] == []
    v, i = plan({"features:0": torch.from_numpy(x).to(device)})
    rv, ri = _mirror(x, w["items"], w["item_bias"], k, tower=w)
    assert torch.equal(i.cpu(), ri) and torch.equal(v.cpu().float(), rv)
    return x, w, g, rv, ri


@pytest.mark.gpu
def test_plan_and_model_gpu():
    x, w, _, rv, ri = _check_plan(torch.device("cuda", 0))
    ids = [f"item_{n}" for n in range(N5)]
    m = RetrievalModel(64, (64, 64), 32, N5, 10, buckets=(8, 32), item_ids=ids, weights=w, device="cuda:0")
    m.open()
    try:
        want = [[(float(s), ids[n]) for s, n in zip(vr, ir)] for vr, ir in zip(rv.tolist(), ri.tolist())]
        assert m.retrieve(list(x)) == want
        done = m.submit(list(x), np.zeros(len(x)), list(range(len(x)))) + m.drain()
        got = {t: p for pairs, tags, _ in done for p, t in zip(pairs, tags)}
        assert [got[t] for t in range(len(x))] == want
    finally:
        m.close()


def test_plan_host():
    """Fails before the ``retrieve`` step existed: the bare ``TopKV2`` is a ``CompileError`` under ``strict``."""
    x, _, g, rv, ri = _check_plan("cpu")
    sv, si = Session(g, device=torch.device("cpu")).run(["top_k:0", "top_k:1"], {"features:0": torch.from_numpy(x)})
    assert torch.equal(torch.as_tensor(si), ri) and torch.equal(torch.as_tensor(sv).float(), rv)


@pytest.mark.parametrize("variant,kw", [("fetched", {}), ("second_reader", {}), ("fed_k", {}), ("plain", {"k": 129}),
                                        ("plain", {"D": 48}), ("unsorted", {})])
def test_refusals(variant, kw):
    g, feeds, fetches = _graph(variant, **kw)
    with pytest.raises(CompileError):
        CompiledFunction(g, feeds, fetches, "cpu", strict=True)
    assert "retrieve" not in CompiledFunction(g, feeds, fetches, "cpu").summary()["kinds"]
    g, feeds, fetches = _graph("plain")  # the same graph without the variation lowers
    assert CompiledFunction(g, feeds, fetches, "cpu", strict=True).summary()["kinds"]["retrieve"] == 1


def test_interpreter_topk_ties():
    gb = GraphBuilder()
    gb.top_k(gb.placeholder("x", "FLOAT", [1, 8]), 5, name="top_k")
    row = torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0, 1.0, 3.0, 1.0]])
    v, i = Session(gb.build(), device=torch.device("cpu")).run(["top_k:0", "top_k:1"], {"x:0": row})
    assert torch.as_tensor(i).tolist() == [[1, 2, 4, 6, 0]] and torch.as_tensor(v).tolist() == [[3.0, 3.0, 3.0, 3.0, 1.0]]
