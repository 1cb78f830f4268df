"""CPU: which NeuralCF shapes the grid kernel admits (a function of shapes alone), and the host-side argument checks of
``ctr_ncf_grid_scores``, which run before anything is enqueued and so need no device."""
import ctypes

import pytest
import torch

PINNED = (64, [128, 64, 32, 16, 8])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


def _shapes(num_users, num_items, mf_dim, layers, bias=True, device="meta"):
    """(tables, hidden, proj) of NeuralCF(num_users, num_items, mf_dim, layers) as storage-free tensors"""
    from deeplearningrecommendationsystem_amd.ops import ACT_RELU, Layer
    e = lambda *shape: torch.empty(*shape, device=device)   # noqa: E731
    half = layers[0] // 2
    tables = (e(num_users, mf_dim), e(num_items, mf_dim), e(num_users, half), e(num_items, half))
    hidden = [Layer(e(b, a), e(b) if bias or k else None, ACT_RELU) for k, (a, b) in enumerate(zip(layers[:-1], layers[1:]))]
    return tables, hidden, (e(mf_dim, layers[-1]), e(mf_dim))


@pytest.mark.parametrize("nu,ni", [(1, 1), (943, 1682), (200_000, 30_000)])
def test_pinned_shape_is_admitted_at_any_table_size(lib, nu, ni):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import neuralcf
    shapes = _shapes(nu, ni, *PINNED)
    assert ops.ncf_grid_supported(*shapes)
    assert neuralcf.grid_path(*shapes) == "grid"


def test_cpu_tensors_will_do(lib):
    from deeplearningrecommendationsystem_amd.model import NeuralCF, neuralcf
    p = NeuralCF(5, 7, *PINNED)._params()
    assert neuralcf.grid_path(p.tables, p.hidden, p.proj) == "grid"
    p = NeuralCF(5, 7, 8, [16, 8, 4])._params()
    assert neuralcf.grid_path(p.tables, p.hidden, p.proj) == "forward"


@pytest.mark.parametrize("mf_dim,layers,bias", [
    (32, [128, 64, 32, 16, 8], True),            # mf_dim 32
    (64, [128, 64, 32, 16], True),               # a shorter tower
    (64, [128, 64, 32, 16, 8], False),           # a layer without bias
    (256, [512, 256, 128, 64, 32], True),        # the reference script's model
], ids=["mf32", "short-tower", "no-bias", "reference-script"])
def test_other_shapes_are_refused(lib, mf_dim, layers, bias):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import neuralcf
    shapes = _shapes(943, 1682, mf_dim, layers, bias=bias)
    assert not ops.ncf_grid_supported(*shapes)
    assert neuralcf.grid_path(*shapes) == "forward"


# ---- the C entry: every refusal below is decided on the host, before a launch
class _Call:
    """arguments of ctr_ncf_grid_scores over host buffers (never dereferenced: nothing below reaches a launch)"""

    def __init__(self, lib, nu=5, ni=7):
        self.lib = lib
        self.keep = [(ctypes.c_float * 64)() for _ in range(8)]        # 16-byte aligned stand-ins for device memory
        addr = [ctypes.addressof(b) + (-ctypes.addressof(b)) % 16 for b in self.keep]
        self.layers = (lib.MlpLayer * 3)()
        for e, (k, n) in zip(self.layers, ((64, 32), (32, 16), (16, 8))):
            e.w, e.b, e.n, e.k, e.act = addr[4], addr[5], n, k, lib.ACT_RELU
        self.a = dict(p_user=addr[0], p_item=addr[1], gmf_user=addr[2], gmf_item=addr[3], num_users=nu, num_items=ni,
                      mf_dim=64, width=64, layers=self.layers, nlayers=3, wfold=addr[6], cfold=addr[7], fold_k=8,
                      users=None, user0=0, rows=nu, act=lib.ACT_SIGMOID, out=addr[6], ldo=ni, stream=None)

    def __call__(self, **changed):
        a = dict(self.a, **changed)
        return self.lib.load().ctr_ncf_grid_scores(*a.values())


OK, EINVAL, ELIMIT = 0, -1, -2


def test_bad_arguments_are_einval(lib):
    call = _Call(lib)
    assert call(ldo=6) == EINVAL                                      # ldo < num_items
    for table in ("p_user", "p_item", "gmf_user", "gmf_item"):
        assert call(**{table: None}) == EINVAL, table
    assert call(layers=None) == EINVAL and call(wfold=None) == EINVAL and call(cfold=None) == EINVAL
    assert call(rows=-1) == EINVAL
    assert call(num_items=-1, ldo=0) == EINVAL and call(num_users=-1) == EINVAL
    assert call(out=None) == EINVAL
    assert call(user0=3, rows=3) == EINVAL                            # users 3 .. 5 of a table of five
    assert call(act=7) == EINVAL


def test_unpinned_shapes_are_elimit(lib):
    call = _Call(lib)
    assert call(mf_dim=32) == ELIMIT and call(width=128) == ELIMIT and call(fold_k=4) == ELIMIT
    assert call(nlayers=2) == ELIMIT
    call.layers[1].n = 32                                             # 32 -> 32 instead of 32 -> 16
    assert call() == ELIMIT
    call.layers[1].n = 16
    call.layers[2].b = None                                           # a layer without bias
    assert call() == ELIMIT
    assert _Call(lib)(num_users=1 << 31, rows=0) == ELIMIT


def test_empty_grid_is_a_no_op(lib):
    call = _Call(lib)
    assert call(rows=0) == OK and call(rows=0, out=None) == OK
    assert call(num_items=0, ldo=0) == OK
    assert call(num_users=0, rows=0) == OK
