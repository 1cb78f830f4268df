"""CPU: the restatement tests/graph_numpy.py -- its CSR propagation against the dense product, the adjointness of the two
sides, the Horner backward against a finite difference -- then the host-side refusals of ``ctr_graph_propagate`` and its
workspace call, and what ``ops`` and ``LightGCN`` decide before a device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import graph_numpy as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ELIMIT, EALIGN = 0, -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


def _user_csr(graph):
    num_users, _, users, items = graph
    indptr = np.zeros(num_users + 1, dtype=np.int64)
    np.cumsum(np.bincount(users, minlength=num_users), out=indptr[1:])
    return indptr, items.astype(np.int32)


# ---- the restatement
@pytest.mark.parametrize("name", sorted(gn.GRAPHS))
def test_csr_propagation_equals_the_dense_product(name):
    graph = gn.model_graph(name)
    num_users, num_items = graph[:2]
    indptr, indices = _user_csr(graph)
    assert indptr[-1] == gn.GRAPHS[name][2] == len(set(zip(graph[2], graph[3])))      # distinct pairs, all of them
    rs = np.random.RandomState(1)
    x, s_in, s_out = rs.normal(0, 1, (num_items, 16)), rs.uniform(0.05, 1, num_items), rs.uniform(0.05, 1, num_users)
    got, mag = gn.propagate64(x, indptr, indices, s_in, s_out)
    want = s_out[:, None] * (gn.dense_adjacency(indptr, indices, num_items) @ (s_in[:, None] * x))
    assert np.abs(got - want).max() <= 1e-12
    assert (mag >= np.abs(got) - 1e-12).all()
    rows = rs.permutation(num_users)[:11]
    assert np.array_equal(gn.propagate64(x, indptr, indices, s_in, s_out, rows=rows)[0], got[rows])
    ones, _ = gn.propagate64(x, indptr, indices)
    assert np.abs(ones - gn.dense_adjacency(indptr, indices, num_items) @ x).max() <= 1e-12


@pytest.mark.parametrize("name", sorted(gn.GRAPHS))
def test_user_and_item_side_are_adjoint(name):
    graph = gn.model_graph(name)
    num_users, num_items = graph[:2]
    indptr, indices = _user_csr(graph)
    t_indptr, t_indices = gn.transpose_csr(indptr, indices, num_items)
    assert np.array_equal(gn.dense_adjacency(t_indptr, t_indices, num_users),
                          gn.dense_adjacency(indptr, indices, num_items).T)
    rs = np.random.RandomState(2)
    s_u, s_i = rs.uniform(0.05, 1, num_users), rs.uniform(0.05, 1, num_items)
    x, y = rs.normal(0, 1, (num_items, 16)), rs.normal(0, 1, (num_users, 16))
    prop_u, _ = gn.propagate64(x, indptr, indices, s_i, s_u)            # (U, k) from the item table
    prop_i, _ = gn.propagate64(y, t_indptr, t_indices, s_u, s_i)        # (I, k) from the user table
    lhs, rhs = (prop_u * y).sum(), (x * prop_i).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


@pytest.mark.parametrize("layers", [0, 1, 3])
def test_horner_backward_is_the_gradient_of_the_mean_of_layers(layers):
    graph = gn.model_graph("small")
    num_users, num_items = graph[:2]
    adj = gn.normalised_adjacency(*graph)
    assert np.array_equal(adj, adj.T)
    assert not adj[:num_users, :num_users].any() and not adj[num_users:, num_users:].any()
    rs = np.random.RandomState(3)
    e0, gf = rs.normal(0, 1, (num_users + num_items, 4)), rs.normal(0, 1, (num_users + num_items, 4))

    def objective(e):      # the unrolled mean of layers, then a fixed linear functional
        total, layer = e.copy(), e
        for _ in range(layers):
            layer = adj @ layer
            total = total + layer
        return (gf * total / (layers + 1)).sum()
    got = gn.horner_backward(adj, layers, gf)
    for _ in range(40):
        r, c = rs.randint(num_users + num_items), rs.randint(4)
        step = np.zeros_like(e0)
        step[r, c] = 1e-3
        fd = (objective(e0 + step) - objective(e0 - step)) / 2e-3      # the objective is linear: exact up to roundoff
        assert abs(fd - got[r, c]) <= 1e-9 * max(1.0, abs(fd))
    assert np.abs(got - gn.mean_of_layers(adj, layers).T @ gf).max() <= 1e-12


def test_model_restatement_gradient_against_a_finite_difference():
    graph = gn.model_graph("small")
    rs = np.random.RandomState(4)
    w_u, w_i = rs.normal(0, 0.3, (graph[0], 4)), rs.normal(0, 0.3, (graph[1], 4))
    users, items, weights = gn.model_batch(graph)
    _, g_u, g_i = gn.model64(w_u, w_i, graph, 3, users, items, weights)
    for _ in range(10):
        r, c = rs.randint(graph[0]), rs.randint(4)
        step = np.zeros_like(w_u)
        step[r, c] = 1e-5
        hi = (weights * gn.model64(w_u + step, w_i, graph, 3, users, items, weights)[0]).sum()
        lo = (weights * gn.model64(w_u - step, w_i, graph, 3, users, items, weights)[0]).sum()
        assert abs((hi - lo) / 2e-5 - g_u[r, c]) <= 1e-7 * max(1.0, abs(g_u[r, c]))
    assert g_i.shape == w_i.shape


def test_case_builders():
    lengths = gn.list_lengths()
    for n in (0, 1, 2, 3, 63, 64, 65, 511, 512, 513, 1024, 1025, 15, 16, 17, 4, 5, 6, 19, 20, 21, 5 * 512 + 7):
        assert n in lengths
    assert [gn.entries_per_instruction(k) for k in gn.KS] == [16, 5, 4, 1]
    indptr, indices = gn.parity_csr()
    assert sorted(np.diff(indptr)) == sorted(lengths) and indices.max() < gn.X_ROWS - gn.X_UNNAMED
    _, _, users, items = gn.model_graph("large")
    degree_u, degree_i = np.bincount(users, minlength=300), np.bincount(items, minlength=200)
    assert degree_u[5] == degree_u[17] == 0 and (degree_u > 0).sum() == 298 and degree_i[0] == 298


# ---- the header and the C entries: every refusal below is decided on the host, before a launch
def test_header_declares_the_entries_and_the_constants(lib):
    from deeplearningrecommendationsystem_amd import ops
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    assert int(re.search(r"#define\s+CTR_GRAPH_MAX_DIM\s+(\d+)", text).group(1)) == lib.CTR_GRAPH_MAX_DIM == 256
    segment = int(re.search(r"#define\s+CTR_GRAPH_SEGMENT\s+(\d+)", text).group(1))
    assert segment == lib.CTR_GRAPH_SEGMENT == ops.GRAPH_SEGMENT == gn.SEGMENT
    handle = lib.load()
    for name in ("ctr_graph_propagate_workspace_bytes", "ctr_graph_propagate"):
        assert name in text and name in lib.SIGNATURES and hasattr(handle, name)
    source = open(os.path.join(ROOT, "deeplearningrecommendationsystem_amd", "csrc", "graph_prop.hip")).read()
    assert "atomicAdd" not in source and "atomic_add" not in source and "fadd" not in source      # no float atomics
    assert [k for k in range(0, 300) if ops.graph_supported(k)] == list(range(16, 257, 16))
    assert not ops.graph_supported(16.0) and not ops.graph_supported(True)


def _call(h, p, **over):
    a = dict(x=p, x_rows=10, ldx=64, k=64, indptr=p, indices=p, num_rows=5, nnz=20, s_in=None, s_out=None, rows=None,
             count=5, work=None, nwork=0, merge=None, nmerge=0, out=p, ldo=64, workspace=None, workspace_bytes=0,
             err_flag=None, stream=None)
    a.update(over)
    return h.ctr_graph_propagate(*a.values())


def test_c_entries_refuse_before_a_launch(lib):
    h = lib.load()
    buf = (ctypes.c_float * 64)()            # host memory, never dereferenced: nothing below reaches a launch
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    nbytes = ctypes.c_int64(-1)
    assert h.ctr_graph_propagate_workspace_bytes(7, 64, ctypes.byref(nbytes)) == OK and nbytes.value == 7 * 64 * 4
    assert h.ctr_graph_propagate_workspace_bytes(0, 64, ctypes.byref(nbytes)) == OK and nbytes.value == 0
    assert h.ctr_graph_propagate_workspace_bytes(7, 64, None) == EINVAL
    assert h.ctr_graph_propagate_workspace_bytes(-1, 64, ctypes.byref(nbytes)) == EINVAL
    assert h.ctr_graph_propagate_workspace_bytes(7, 0, ctypes.byref(nbytes)) == EINVAL
    assert h.ctr_graph_propagate_workspace_bytes(1 << 31, 64, ctypes.byref(nbytes)) == ELIMIT
    for k in (8, 24, 272, 250):
        assert h.ctr_graph_propagate_workspace_bytes(7, k, ctypes.byref(nbytes)) == ELIMIT
        assert _call(h, p, k=k, ldx=k + (-k) % 4, ldo=k + (-k) % 4) == ELIMIT
    # count == 0: CTR_OK, nothing enqueued, whatever the pointers are
    assert _call(h, p, x=None, indptr=None, indices=None, out=None, count=0) == OK
    for over in (dict(x=None), dict(indptr=None), dict(out=None), dict(indices=None), dict(count=-1), dict(x_rows=0),
                 dict(num_rows=0), dict(k=0), dict(nnz=-1), dict(ldx=60), dict(ldo=63), dict(nwork=3), dict(work=p),
                 dict(nmerge=2), dict(merge=p), dict(workspace_bytes=-1),
                 dict(work=p, nwork=1, merge=p, nmerge=1),                       # a merge list without a workspace
                 dict(merge=p, nmerge=1, workspace=p, workspace_bytes=1024)):    # ... or without work items
        assert _call(h, p, **over) == EINVAL, over
    assert _call(h, p, indices=None, nnz=0, x_rows=1 << 31) == ELIMIT           # a CSR without a pair is no EINVAL
    for over in (dict(count=1 << 31), dict(x_rows=1 << 31), dict(num_rows=1 << 31), dict(nnz=1 << 31),
                 dict(work=p, nwork=1 << 31), dict(work=p, nwork=1, merge=p, nmerge=1 << 31, workspace=p)):
        assert _call(h, p, **over) == ELIMIT, over
    for over in (dict(x=p + 4), dict(out=p + 8), dict(ldx=66), dict(ldo=70), dict(indptr=p + 4), dict(indices=p + 2),
                 dict(s_in=p + 2), dict(s_out=p + 1), dict(rows=p + 4), dict(err_flag=p + 2),
                 dict(work=p + 8, nwork=1), dict(work=p, nwork=1, merge=p + 4, nmerge=1, workspace=p),
                 dict(work=p, nwork=1, merge=p, nmerge=1, workspace=p + 4)):
        assert _call(h, p, **over) == EALIGN, over
    assert _call(h, p, k=24, x=p + 4) == ELIMIT and _call(h, p, x=None, ldx=66) == EINVAL      # the header's order


# ---- ops and the model, without a device
def test_ops_refuse_bad_arguments_and_have_no_cpu_fallback(lib):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    indptr, indices = torch.tensor([0, 2, 3]), torch.tensor([0, 1, 1], dtype=torch.int32)
    x = torch.zeros(5, 16)
    for k in (8, 24, 272):
        with pytest.raises(ValueError):
            ops.graph_propagate(torch.zeros(5, k), indptr, indices)
    bad = [dict(x=x.double()), dict(x=torch.zeros(5)), dict(x=torch.zeros(0, 16)), dict(x=torch.zeros(16, 5).t()),
           dict(x=torch.zeros(5, 18)[:, :16]), dict(indptr=indptr.int()), dict(indptr=torch.tensor([0])),
           dict(indptr=indptr.view(1, 3)), dict(indices=indices.long()), dict(indices=indices.view(3, 1)),
           dict(scale_in=torch.ones(4)), dict(scale_in=torch.ones(5, dtype=torch.float64)),
           dict(scale_out=torch.ones(3)), dict(rows=torch.tensor([0], dtype=torch.int32)),
           dict(rows=torch.zeros(1, 1, dtype=torch.int64)), dict(out=torch.zeros(3, 16)),
           dict(out=torch.zeros(2, 16, dtype=torch.float64)), dict(out=torch.zeros(2, 18)[:, :16]),
           dict(err_flag=torch.zeros(2, dtype=torch.int32)), dict(err_flag=torch.zeros(1)), dict(plan=object())]
    for over in bad:
        args = dict(x=x, indptr=indptr, indices=indices)
        args.update(over)
        with pytest.raises(ValueError):
            ops.graph_propagate(**args)
    plan = ops.GraphPlan(indptr, 2, None, None, 0)
    with pytest.raises(ValueError):
        ops.graph_propagate(x, indptr, indices, rows=torch.tensor([0]), plan=plan)      # a plan covers all rows
    with pytest.raises(ValueError):
        ops.graph_propagate(x, torch.tensor([0, 2, 3]), indices, plan=plan)             # another CSR's plan
    with pytest.raises(ValueError):
        ops.graph_plan(torch.tensor([0, 1], dtype=torch.int32))
    with pytest.raises(CtrHipError):
        ops.graph_plan(indptr)
    with pytest.raises(CtrHipError):
        ops.graph_propagate(x, indptr, indices)                                          # well formed, but no device
    with pytest.raises(CtrHipError):
        ops.graph_propagate(x, indptr, indices, out=torch.zeros(2, 20)[:, :16])          # ldo > k is well formed too


def test_model_argument_errors_need_no_device(lib):
    from deeplearningrecommendationsystem_amd import model as zoo
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    from deeplearningrecommendationsystem_amd.data import ObservedPairs
    from deeplearningrecommendationsystem_amd.model import lightgcn
    assert "LightGCN" in zoo.__all__ and zoo.LightGCN is lightgcn.LightGCN
    for kwargs in (dict(num_layers=-1), dict(num_layers=1.0), dict(embedding_size=24), dict(embedding_size=8),
                   dict(embedding_size=272)):
        with pytest.raises(ValueError):
            zoo.LightGCN(5, 6, **{"embedding_size": 16, **kwargs})
    assert zoo.LightGCN(5, 6, 24, num_layers=0).user_embeddings.weight.shape == (5, 24)      # MF takes any width
    torch.manual_seed(3)
    model = zoo.LightGCN(5, 6, 16)
    torch.manual_seed(3)
    twin = zoo.MatrixFactorization(5, 6, 16)
    assert model.num_layers == 3 and sorted(model.state_dict()) == sorted(twin.state_dict())
    for name, value in model.state_dict().items():
        assert torch.equal(value, twin.state_dict()[name])                                     # xavier_normal_ as MF
    users, items = torch.tensor([0, 1]), torch.tensor([2, 3])
    with pytest.raises(RuntimeError):
        model(users, items)
    with pytest.raises(RuntimeError):
        model.propagate()
    with pytest.raises(ValueError):
        model.set_graph(ObservedPairs(torch.tensor([0]), torch.tensor([2]), 5, 7))
    with pytest.raises(TypeError):
        model.set_graph((users, items))
    with pytest.raises(CtrHipError):
        model.set_graph(ObservedPairs(users, items, 5, 6))                                     # no device: no fallback
    assert lightgcn.grid_path(64) == "grid" and lightgcn.grid_path(20) == "forward"
