"""Ranking (kernels/interact.hip, graph/ranking_lowering.py, models/zoo/dlrm.py).

Every kernel test uses exact data: table entries and the activation vector are integers in
{-1, 0, 1}, so every dot product is an integer of magnitude <= D <= 256, exact in fp32 in any
summation order and exact in bf16, and the comparison with the float64 mirror is ``torch.equal``.
Field ``f`` has its own vocabulary size (1 among them) and its ids sit in column ``F - 1 - f``, so a
wrong base, field or column shows.

The plan's MLPs (the retrieval test's tower trick): dense features in {0, 1}, every column has 4
weights of +-1 and an integer bias of magnitude <= 1, embedding rows have two entries of +-1.  So
the activation vector is at most 5, a dot at most 10, the top hidden layer at most 4 * 10 + 1 = 41
and the logit at most 4 * 41 + 1 = 165: integers below 256, exact in bf16 through every layer.
"""
import numpy as np
import pytest
import torch

from flink_tensorflow_amd.graph.builder import GraphBuilder
from flink_tensorflow_amd.graph.compiler import CompiledFunction, CompileError
from flink_tensorflow_amd.graph.session import Session
from flink_tensorflow_amd.models.core import GraphDefGraphLoader
from flink_tensorflow_amd.models.zoo import DLRMModel, dlrm_graph_def
from flink_tensorflow_amd.ops import kernels as K

BF = torch.bfloat16
NAN = float("nan")
FORMS = ("lower", "lower_diag", "upper", "shuffled")


def _data(B, M, D, dense_row, seed=0, bad_ids=False):
    """``(tables, ids [B, F], cols, dense [B, D])`` as numpy arrays; ``bad_ids`` plants -1 and ``V_f``."""
    rng = np.random.default_rng(seed)
    F = M - (dense_row is not None)
    tables = [rng.integers(-1, 2, (1 + (3 * f) % 5, D)).astype(np.float32) for f in range(F)]  # V_f = 1, 4, 2, 5, 3, ...
    cols = [F - 1 - f for f in range(F)]
    ids = np.zeros((B, max(F, 1)), dtype=np.int32)
    for f in range(F):
        ids[:, cols[f]] = rng.integers(0, len(tables[f]), B)
    if bad_ids:
        ids[0, :] = -1
        ids[-1, :] = [len(tables[F - 1 - c]) for c in range(F)]
        ids[B // 2, 0] = 2 ** 31 - 1
    return tables, ids, cols, rng.integers(-1, 2, (B, D)).astype(np.float32)


def _pairs(M, form):
    if form == "lower_diag":
        return [(i, j) for i in range(M) for j in range(i + 1)]
    if form == "upper":
        return [(i, j) for i in range(M) for j in range(i + 1, M)]
    lower = [(i, j) for i in range(M) for j in range(i)]
    if form == "shuffled":  # any order, either orientation
        rng = np.random.default_rng(M)
        lower = [lower[k] if k % 3 else lower[k][::-1] for k in rng.permutation(len(lower))]
    return lower


def _mirror(tables, ids, cols, dense, dense_row, pairs, copy):
    """float64, from the definition: gather, ``T @ T.T``, index by the pair list, concat."""
    T, f = [], 0
    for m in range(len(tables) + (dense_row is not None)):
        if m == dense_row:
            T.append(dense)
            continue
        i = ids[:, cols[f]].astype(np.int64)
        ok = (i >= 0) & (i < len(tables[f]))
        T.append(np.where(ok[:, None], tables[f][np.clip(i, 0, len(tables[f]) - 1)], 0.0))
        f += 1
    T = np.stack(T, 1).astype(np.float64)
    Z = T @ T.transpose(0, 2, 1)
    row = np.stack([Z[:, i, j] for i, j in pairs], 1)
    return torch.from_numpy(np.concatenate([dense, row], 1) if copy else row).to(BF)


def _operands(tables, ids, cols, dense, dense_row, pairs, copy, dev):
    """Device operands of ``K.dot_interact``: the tables in one buffer with two NaN rows around each, the
    activation inside a wider NaN buffer, ``meta`` and the LUT."""
    D = dense.shape[1]
    guard = np.full((2, D), NAN, dtype=np.float32)
    rows, bases, at = [guard], [], 2
    for t in tables:
        bases.append(at)
        rows += [t, guard]
        at += len(t) + 2
    table = torch.from_numpy(np.concatenate(rows)).to(dev, BF)
    meta, f = [], 0
    for m in range(len(tables) + (dense_row is not None)):
        meta.append((0, -1, 0) if m == dense_row else (bases[f], cols[f], len(tables[f])))
        f += m != dense_row
    meta = torch.tensor(meta, dtype=torch.int64).t().contiguous().to(dev)
    wide = torch.full((len(dense) + 2, D + 16), NAN, dtype=BF, device=dev)
    wide[1:-1, 8:8 + D] = torch.from_numpy(dense).to(dev, BF)
    lut = K.dot_interact_lut(meta.shape[1], pairs, D if copy else 0).to(dev)
    return table, torch.from_numpy(ids).to(dev), meta, lut, (wide[1:-1, 8:8 + D] if dense_row is not None or copy else None)


def _check_interact(B, M, D, dense_row, form, copy, workgroups=None, bad_ids=False, extra=0):
    """Runs the kernel twice into a slot of a NaN-filled buffer: the logical columns equal the mirror, the
    pad columns are zero, nothing outside the slot is touched and both launches give the same bits."""
    dev = torch.device("cuda", 0)
    tables, ids, cols, dense = _data(B, M, D, dense_row, seed=B + M + D, bad_ids=bad_ids)
    pairs = _pairs(M, form)
    want = _mirror(tables, ids, cols, dense, dense_row, pairs, copy)
    wlog = want.shape[1]
    wout = -(-(wlog + extra) // 8) * 8  # ``extra`` columns no pair selects: zeros, like the pad
    table, ids_d, meta, lut, dense_d = _operands(tables, ids, cols, dense, dense_row, pairs, copy, dev)
    runs = []
    for _ in range(2):
        buf = torch.full((B + 2, wout + 24), NAN, dtype=BF, device=dev)
        K.dot_interact(table, ids_d, meta, lut, wlog + extra, dense_d, copy, out=buf[1:-1, 16:16 + wout], workgroups=workgroups)
        runs.append(buf.cpu())
    got = runs[0][1:-1, 16:16 + wout]
    assert torch.equal(got[:, :wlog], want)
    assert bool((got[:, wlog:] == 0).all())
    outside = runs[0].clone()
    outside[1:-1, 16:16 + wout] = NAN
    assert bool(torch.isnan(outside).all())
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16))


# B in {1, 5, 9} (with one or two workgroups a wave takes a second and a third record); M in {2, 27, 32, 33, 64};
# D in {16, 48, 128, 256}: one MFMA step, an odd step count, the full line, the maximum
GEOMETRY = [(1, 2, 16, None), (5, 27, 128, 1), (9, 32, 48, 1), (9, 33, 16, 2), (5, 64, 256, None), (1, 64, 128, None),
            (9, 27, 256, 1), (5, 32, 16, None), (1, 33, 48, None), (9, 64, 48, 1), (5, 2, 256, 1), (9, 33, 128, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,M,D,workgroups", GEOMETRY)
def test_geometry(B, M, D, workgroups):
    _check_interact(B, M, D, 0, "lower", True, workgroups)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [27, 33])
@pytest.mark.parametrize("dense_row,copy", [(0, True), (0, False), ("last", True), ("last", False), (None, False)])
@pytest.mark.parametrize("form", FORMS)
def test_selection(form, dense_row, copy, M):
    _check_interact(5, M, 48, M - 1 if dense_row == "last" else dense_row, form, copy, workgroups=1)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [27, 64])
def test_out_of_range_ids(M):
    """Ids -1, ``V_f`` and 2^31 - 1 give zero vectors (the NaN rows next to every table stay unread)."""
    _check_interact(9, M, 128, 0, "lower_diag", True, bad_ids=True)


@pytest.mark.gpu
@pytest.mark.parametrize("M,dense_row", [(27, None), (33, 0)])
def test_unselected_columns_and_unpacked_copy(M, dense_row):
    """Eleven columns that no pair selects come out zero on a wave's second and third record too, and the copy of the
    activation vector does not depend on the vector being packed."""
    _check_interact(9, M, 48, dense_row, "upper", True, workgroups=1, extra=11)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [8, 136])
def test_embed_rows(D):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(D)
    V, R = 7, 37
    t = rng.integers(-1, 2, (V, D)).astype(np.float32)
    ids = rng.integers(0, V, R).astype(np.int32)
    ids[[0, 5, 36]] = [-1, V, 2 ** 31 - 1]
    table = torch.full((V + 4, D), NAN, dtype=BF, device=dev)
    table[2:2 + V] = torch.from_numpy(t).to(dev, BF)
    buf = torch.full((R + 2, D + 24), NAN, dtype=BF, device=dev)
    K.embed_rows(table, torch.from_numpy(ids).to(dev), base=2, vocab=V, out=buf[1:-1, 16:16 + D])
    ok = (ids >= 0) & (ids < V)
    want = torch.from_numpy(np.where(ok[:, None], t[np.clip(ids, 0, V - 1)], 0.0)).to(BF)
    got = buf.cpu()
    assert torch.equal(got[1:-1, 16:16 + D], want)
    got[1:-1, 16:16 + D] = NAN
    assert bool(torch.isnan(got).all())


# ------------------------------------------------------------------ plans and the model
VOCAB, DIM, HID = (5, 1, 7), 16, 32


def _model(B, seed=1):
    """Exact-integer weights of a small DLRM (F = 3, D = 16) and ``B`` records: ``(weights, dense [B, 16], ids [B, 3])``."""
    rng = np.random.default_rng(seed)
    w = {}
    for key, (fi, fo) in (("bw0", (16, DIM)), ("tw0", (DIM + 6, HID)), ("tw1", (HID, 1))):
        w[key] = np.zeros((fi, fo), dtype=np.float32)
        for c in range(fo):
            w[key][rng.choice(fi, 4, replace=False), c] = rng.choice([-1.0, 1.0], 4)
        w[key.replace("w", "b")] = rng.integers(-1, 2, fo).astype(np.float32)
    for f, V in enumerate(VOCAB):
        w[f"emb{f}"] = np.zeros((V, DIM), dtype=np.float32)
        for v in range(V):
            w[f"emb{f}"][v, rng.choice(DIM, 2, replace=False)] = rng.choice([-1.0, 1.0], 2)
    dense = rng.integers(0, 2, (B, 16)).astype(np.float32)
    dense[:, 13:] = 0.0  # the model pads 13 features to 16
    return w, dense, np.stack([rng.integers(0, V, B) for V in VOCAB], 1).astype(np.int32)


def _check_plan(device):
    B = 9
    w, dense, ids = _model(B)
    g = GraphDefGraphLoader(dlrm_graph_def(13, VOCAB, DIM, (DIM,), (HID, 1), weights=w)).load()
    feeds = {"dense:0": ((B, 16), "FLOAT"), "ids:0": ((B, 3), "INT32")}
    plan = CompiledFunction(g, feeds, ["logit:0", "probability:0"], device, strict=True)
    kinds = plan.summary()["kinds"]
    assert (kinds["gemm"], kinds["interact"], kinds["elementwise"]) == (3, 1, 1) and plan.summary()["glue_ops"] == []
    fed = {"dense:0": torch.from_numpy(dense), "ids:0": torch.from_numpy(ids)}
    logit, prob = plan({k: v.to(device) for k, v in fed.items()})
    ref = torch.as_tensor(Session(g, device=torch.device("cpu")).run(["logit:0"], fed)[0])
    assert bool((ref.abs() < 256).all()) and torch.equal(logit.cpu().float(), ref)
    assert float((prob.cpu().double() - torch.sigmoid(ref.double())).abs().max()) <= 2.0 ** -8
    return w, dense, ids, torch.sigmoid(ref.double()).reshape(-1)


def test_plan_host():
    """Fails before the ``interact`` step existed: a ``CompileError`` at the first ``GatherV2``."""
    _check_plan("cpu")


def _check_model(device):
    w, dense, ids, want = _check_plan(device)
    m = DLRMModel(13, VOCAB, DIM, (DIM,), (HID, 1), buckets=(4, 16), weights=w, device=device)
    m.open()
    try:
        got = m.rank(dense[:, :13], ids)
        done = m.submit(list(zip(dense[:, :13], ids)), np.zeros(len(ids)), list(range(len(ids)))) + m.drain()
        assert [p for probs, _, _ in done for p in probs] == got
        assert [t for _, tags, _ in done for t in tags] == list(range(len(ids)))
        assert float((torch.tensor(got, dtype=torch.float64) - want).abs().max()) <= 2.0 ** -8
    finally:
        m.close()


def test_model_host():
    _check_model("cpu")


@pytest.mark.gpu
def test_plan_and_model_gpu():
    _check_model("cuda:0")


def _graph(variant, B=5, D=16):
    """The builder's interaction of an activation vector and three lookups, its other lowered forms and its
    refused variants: ``(graph, feeds, fetches, fed tensors, variables)``."""
    rng = np.random.default_rng(3)
    B = 16 if variant == "axis1" else B  # a column gather of a [16, V] table gives [16, B]: packs only when B = D
    ints = lambda *s: rng.integers(-1, 2, s).astype(np.float32)  # noqa: E731
    D = 24 if variant == "D24" else D
    F = 65 if variant == "M66" else 3
    gb = GraphBuilder()
    x = gb.placeholder("x", "FLOAT", [B, D])
    idt = "INT64" if variant == "int64_ids" else "INT32"
    ids = gb.placeholder("ids", idt, [B, F])
    feeds = {"x:0": ((B, D), "FLOAT"), "ids:0": ((B, F), idt)}
    fed = {"x:0": torch.from_numpy(ints(B, D)),
           "ids:0": torch.from_numpy(rng.integers(0, 2, (B, F))).to(torch.int64 if idt == "INT64" else torch.int32)}
    cols = gb.op("Unpack", [ids], name="unstack", num=F, axis=1).split(":")[0]
    tables = [gb.constant(f"table_{f}", ints(2 + f % 3, D)) for f in range(F)]
    if variant == "fed_table":
        tables[1] = gb.placeholder("fed", "FLOAT", [3, D])
        feeds["fed:0"], fed["fed:0"] = ((3, D), "FLOAT"), torch.from_numpy(ints(3, D))
    idcols = [f"{cols}:{f}" for f in range(F)]
    variables = {}
    if variant == "variable_table":
        variables["var"] = torch.from_numpy(ints(3, D))
        tables[1] = gb.identity(gb.variable("var", "FLOAT", [3, D]), name="var/read")
    if variant == "slice_columns":
        idcols = [gb.strided_slice(ids, [0, f], [0, f + 1], name=f"col_{f}", begin_mask=1, end_mask=1, shrink_axis_mask=2)
                  for f in range(F)]
    if variant == "two_feeds":
        other = gb.placeholder("ids2", "INT32", [B, 1])
        feeds["ids2:0"], fed["ids2:0"] = ((B, 1), "INT32"), torch.zeros((B, 1), dtype=torch.int32)
        idcols[2] = gb.op("Unpack", [other], name="unstack2", num=1, axis=1)
    vec = [x] + [gb.embedding_lookup(t, c, name=f"lookup_{f}") for f, (t, c) in enumerate(zip(tables, idcols))]
    if variant == "axis1":  # GatherV2(table [D, V], ids, axis 1) -> [D, B]
        vec[2] = gb.op("GatherV2", [gb.constant("wide", ints(D, 3)), idcols[1], gb.constant("one", np.asarray(1, np.int32))],
                       name="columns")
    if variant == "two_dense":
        vec.append(gb.relu(x, name="second"))
    if variant == "bag":  # a multi-hot field: two ids per record, summed
        bag = gb.placeholder("bag", "INT32", [2 * B])
        feeds["bag:0"], fed["bag:0"] = ((2 * B,), "INT32"), torch.from_numpy(rng.integers(0, 4, 2 * B).astype(np.int32))
        vec.append(gb.op("SparseSegmentSum", [gb.constant("bag_table", ints(4, D)), bag,
                                              gb.constant("segments", np.repeat(np.arange(B, dtype=np.int32), 2))], name="bag_sum"))
    fetches = ["interaction/concat:0"]
    M = len(vec)
    if variant == "concat_reshape":
        T = gb.reshape(gb.concat(vec, 1, name="joined"), [-1, M, D], name="interaction/stack")
        flat = gb.reshape(gb.op("BatchMatMulV2", [T, T], name="interaction/MatMul", adj_x=False, adj_y=True), [-1, M * M])
        tri = gb.op("GatherV2", [flat, gb.constant("tri", np.asarray([i * M + j for i in range(M) for j in range(i)], np.int32)),
                                 gb.constant("ax", np.asarray(1, np.int32))], name="triangle")
        gb.concat([x, tri], 1, name="interaction/concat")
    elif variant == "duplicate":  # Z[1, 0] and its mirror Z[0, 1]
        T = gb.op("Pack", vec, name="interaction/stack", N=M, axis=1)
        flat = gb.reshape(gb.op("BatchMatMulV2", [T, T], name="interaction/MatMul", adj_x=False, adj_y=True), [-1, M * M])
        gb.op("GatherV2", [flat, gb.constant("dup", np.asarray([M, 1], np.int32)), gb.constant("ax", np.asarray(1, np.int32))],
              name="interaction/concat")
    else:
        gb.dot_interaction(vec, concat_with=x)
    if variant == "z_second_reader":
        gb.relu("interaction/MatMul:0", name="other")
        fetches.append("other:0")
    if variant == "t_fetched":
        fetches.append("interaction/stack:0")
    return GraphDefGraphLoader(gb.build_graph_def()).load(), feeds, fetches, fed, variables


def _interpreted(g, fetches, fed, variables):
    sess = Session(g, device=torch.device("cpu"))
    sess.variables.update(variables)
    return [torch.as_tensor(t).float() for t in sess.run(fetches, fed)]


@pytest.mark.parametrize("variant", ["fed_table", "variable_table", "axis1", "int64_ids", "two_feeds", "M66", "D24", "two_dense",
                                     "z_second_reader", "t_fetched", "duplicate", "bag"])
def test_refusals(variant):
    g, feeds, fetches, fed, variables = _graph(variant)
    with pytest.raises(CompileError):
        CompiledFunction(g, feeds, fetches, "cpu", variables, strict=True)
    plan = CompiledFunction(g, feeds, fetches, "cpu", variables)
    assert "interact" not in plan.summary()["kinds"]
    assert all(torch.equal(a.float(), b) for a, b in zip(plan(fed), _interpreted(g, fetches, fed, variables)))


@pytest.mark.parametrize("variant", ["plain", "concat_reshape", "slice_columns"])
def test_lowered_forms(variant):
    """The same graph without a refused variation, with ``ConcatV2 + Reshape`` for ``Pack`` and with sliced id columns."""
    g, feeds, fetches, fed, _ = _graph(variant)
    plan = CompiledFunction(g, feeds, fetches, "cpu", strict=True)
    assert plan.summary()["kinds"]["interact"] == 1 and plan.summary()["glue_ops"] == []
    assert torch.equal(plan(fed)[0].float(), _interpreted(g, fetches, fed, {})[0])


def _check_lone_lookups(device):
    """Two lone lookups (D = 8 and 16) of one id tensor and their ``ConcatV2``: two ``embed`` steps that write the
    concat's slices in place, no copy step; out-of-range ids give zero rows."""
    gb = GraphBuilder()
    rng = np.random.default_rng(5)
    ta, tb = rng.integers(-1, 2, (6, 8)).astype(np.float32), rng.integers(-1, 2, (6, 16)).astype(np.float32)
    ids_t = gb.placeholder("ids", "INT32", [4, 3])
    gb.concat([gb.embedding_lookup(gb.constant("ta", ta), ids_t, name="a"), gb.embedding_lookup(gb.constant("tb", tb), ids_t, name="b")],
              -1, name="both")
    plan = CompiledFunction(GraphDefGraphLoader(gb.build_graph_def()).load(), {"ids:0": ((4, 3), "INT32")}, ["both:0"], device,
                            strict=True)
    ids = torch.tensor([[0, 5, 6], [-1, 2, 3], [1, 1, 4], [5, 0, 2]], dtype=torch.int32)
    ok = ((ids >= 0) & (ids < 6))[..., None]
    want = torch.cat([torch.from_numpy(ta)[ids.clamp(0, 5).long()] * ok, torch.from_numpy(tb)[ids.clamp(0, 5).long()] * ok], -1)
    assert plan.summary()["kinds"] == {"embed": 2} and torch.equal(plan({"ids:0": ids.to(device)})[0].cpu().float(), want)


def test_lone_lookups_host():
    _check_lone_lookups("cpu")


@pytest.mark.gpu
def test_lone_lookups_gpu():
    _check_lone_lookups("cuda:0")
