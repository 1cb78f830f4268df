"""CPU: the float64 restatement tests/softmax_full_numpy.py against torch's float64 autograd of
``F.cross_entropy(X @ Q.T, t, reduction="none")`` under a random upstream gradient, the host-side refusals of the three
``ctr_softmax_full_*`` entries in contract order (they run before anything is enqueued, so they need no device), and
what ``ops`` and ``MatrixFactorization.softmax_nll`` decide before a device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import softmax_full_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ELIMIT, EALIGN = 0, -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


# ---- the restatement
@pytest.mark.parametrize("shape", [(1, 1, 1), (17, 65, 3), (40, 130, 20)])
@pytest.mark.parametrize("scale", [0.1, 1.0, 8.0])
def test_restatement_against_torch_float64_autograd(shape, scale):
    b, n, k = shape
    rng = np.random.default_rng(b + n + k)
    X, Q = rng.normal(0, scale, (b, k)), rng.normal(0, scale, (n, k))
    t, g = rng.integers(0, n, b), rng.random(b)
    t[0] = n - 1
    x, q = torch.tensor(X, requires_grad=True), torch.tensor(Q, requires_grad=True)
    z = x @ q.T
    nll = torch.nn.functional.cross_entropy(z, torch.tensor(t), reduction="none")
    nll.backward(torch.tensor(g))
    got_nll, got_lse, dX, dQ = sn.nll_grads(X, Q, t, g)
    np.testing.assert_allclose(got_nll, nll.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got_lse, torch.logsumexp(z, 1).detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dX, x.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dQ, q.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_one_item_is_exactly_zero():
    rng = np.random.default_rng(0)
    nll, lse, dX, dQ = sn.nll_grads(rng.normal(size=(5, 3)), rng.normal(size=(1, 3)), np.zeros(5, dtype=np.int64),
                                    rng.random(5))
    assert not nll.any() and not dX.any() and not dQ.any()


def test_bounds_have_the_shapes_of_the_outputs():
    rng = np.random.default_rng(1)
    X, Q, t, g = rng.normal(size=(6, 4)), rng.normal(size=(9, 4)), rng.integers(0, 9, 6), rng.random(6)
    lse, nll, dX, dQ = sn.bounds(X, Q, t, g)
    assert lse.shape == nll.shape == (6,) and dX.shape == X.shape and dQ.shape == Q.shape
    assert (lse > 0).all() and (nll >= lse).all() and (dX > 0).all() and (dQ > 0).all()


# ---- the header
def test_header_declares_the_entries_and_the_limit(lib):
    from deeplearningrecommendationsystem_amd import ops
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    define = int(re.search(r"#define\s+CTR_SOFTMAX_FULL_MAX_DIM\s+(\d+)", text).group(1))
    assert lib.CTR_SOFTMAX_FULL_MAX_DIM == define == ops.SOFTMAX_FULL_MAX_DIM == 256
    handle = lib.load()
    for name in ("ctr_softmax_full_workspace_bytes", "ctr_softmax_full_rows", "ctr_softmax_full_cols"):
        assert name in text and name in lib.SIGNATURES and hasattr(handle, name)


# ---- the C entries: every refusal below is decided on the host, before a launch
class _Call:
    """arguments of one entry over host buffers (never dereferenced: nothing below reaches a launch)"""

    ORDER = {
        "ctr_softmax_full_rows": ("x", "q", "batch", "num_items", "k", "target", "nll", "lse", "grad_x", "splits",
                                  "workspace", "workspace_bytes", "err_flag", "stream"),
        "ctr_softmax_full_cols": ("x", "q", "batch", "num_items", "k", "target", "lse", "nll", "gout", "grad_q", "splits",
                                  "workspace", "workspace_bytes", "stream"),
    }

    def __init__(self, lib, entry, **scalars):
        self.lib, self.entry = lib, entry
        names = [n for n in self.ORDER[entry] if n not in scalars]
        self.keep = [(ctypes.c_float * 64)() for _ in names]              # 16-byte aligned stand-ins for device memory
        addr = [ctypes.addressof(b) + (-ctypes.addressof(b)) % 16 for b in self.keep]
        self.a = {n: scalars[n] if n in scalars else addr[names.index(n)] for n in self.ORDER[entry]}

    def __call__(self, **changed):
        a = dict(self.a, **changed)
        return getattr(self.lib.load(), self.entry)(*a.values())


def _rows(lib):
    return _Call(lib, "ctr_softmax_full_rows", batch=5, num_items=7, k=16, splits=1, workspace_bytes=0, stream=None)


def _cols(lib):
    return _Call(lib, "ctr_softmax_full_cols", batch=5, num_items=7, k=16, splits=1, workspace_bytes=0, stream=None)


FLOATS = {"ctr_softmax_full_rows": ("x", "q", "nll", "lse", "grad_x"),
          "ctr_softmax_full_cols": ("x", "q", "lse", "nll", "gout", "grad_q")}


@pytest.mark.parametrize("make", [_rows, _cols], ids=["rows", "cols"])
def test_an_empty_batch_is_ok_whatever_the_pointers_are(lib, make):
    call = make(lib)
    assert call(batch=0) == OK
    assert call(batch=0, x=None, q=None, target=None, lse=None, workspace=None) == OK
    assert call(batch=0, k=300) == OK and call(batch=0, splits=0) == OK


@pytest.mark.parametrize("make", [_rows, _cols], ids=["rows", "cols"])
def test_bad_counts_are_refused(lib, make):
    call = make(lib)
    assert call(batch=-1) == EINVAL and call(num_items=0) == EINVAL and call(num_items=-3) == EINVAL
    assert call(k=0) == EINVAL and call(k=-16) == EINVAL and call(splits=-1) == EINVAL
    assert call(batch=0, num_items=0) == EINVAL and call(batch=0, k=0) == EINVAL     # counts come before emptiness


def test_null_pointers_are_refused(lib):
    call = _rows(lib)
    for name in ("x", "q", "target", "nll", "lse"):
        assert call(**{name: None}) == EINVAL, name
        assert call(**{name: None}, k=300) == EINVAL, name                           # EINVAL comes before ELIMIT
    # grad_x, err_flag and (one part) the workspace are optional: the refusal that follows is another one
    assert call(grad_x=None, err_flag=None, workspace=None, k=300) == ELIMIT
    call = _cols(lib)
    for name in ("x", "q", "target", "lse", "gout", "grad_q"):
        assert call(**{name: None}) == EINVAL, name
        assert call(**{name: None}, num_items=1 << 31) == EINVAL, name
    assert call(nll=None, workspace=None, k=300) == ELIMIT                           # optional, as above


@pytest.mark.parametrize("make", [_rows, _cols], ids=["rows", "cols"])
def test_shapes_beyond_the_limits_are_refused(lib, make):
    call = make(lib)
    assert call(k=257) == ELIMIT and call(k=4096) == ELIMIT
    assert call(batch=1 << 31) == ELIMIT and call(num_items=1 << 31) == ELIMIT and call(splits=65) == ELIMIT
    x = call.a["x"]
    assert call(k=257, x=x + 2) == ELIMIT                                            # ELIMIT comes before EALIGN


@pytest.mark.parametrize("make", [_rows, _cols], ids=["rows", "cols"])
def test_a_missing_workspace_is_refused_when_the_pass_is_split(lib, make):
    call = make(lib)
    need = ctypes.c_int64(-1)
    assert lib.load().ctr_softmax_full_workspace_bytes(100, 100, 16, 2, 2, ctypes.byref(need)) == OK
    assert need.value == 2 * 100 * (16 + 4) * 4                                       # rows: (m, l, z_t, -) and acc
    assert call(batch=100, num_items=100, splits=2, workspace=None) == EINVAL
    assert call(batch=100, num_items=100, splits=2, workspace_bytes=need.value // 2 - 4) == EINVAL


@pytest.mark.parametrize("make", [_rows, _cols], ids=["rows", "cols"])
def test_misaligned_pointers_are_refused(lib, make):
    call = make(lib)
    for name in FLOATS[call.entry]:
        assert call(**{name: call.a[name] + 2}) == EALIGN, name
    assert call(target=call.a["target"] + 4) == EALIGN


def test_workspace_bytes(lib):
    fn = lib.load().ctr_softmax_full_workspace_bytes
    need = ctypes.c_int64(-1)
    assert fn(8, 8, 4, 0, 0, None) == EINVAL and fn(-1, 8, 4, 0, 0, ctypes.byref(need)) == EINVAL
    assert fn(8, 0, 4, 0, 0, ctypes.byref(need)) == EINVAL and fn(8, 8, 0, 0, 0, ctypes.byref(need)) == EINVAL
    assert fn(8, 8, 4, -1, 0, ctypes.byref(need)) == EINVAL
    assert fn(8, 8, 257, 0, 0, ctypes.byref(need)) == ELIMIT and fn(8, 1 << 31, 4, 0, 0, ctypes.byref(need)) == ELIMIT
    assert fn(0, 8, 4, 0, 0, ctypes.byref(need)) == OK and need.value == 0
    assert fn(4096, 26744, 64, 1, 1, ctypes.byref(need)) == OK and need.value == 0   # one part needs none
    # the automatic choice is a function of the shape: the same answer twice, more parts for fewer owners
    a, b = ctypes.c_int64(), ctypes.c_int64()
    assert fn(4096, 26744, 64, 0, 1, ctypes.byref(a)) == OK and fn(4096, 26744, 64, 0, 1, ctypes.byref(b)) == OK
    assert a.value == b.value == 8 * 4096 * 68 * 4                                    # 64 workgroups on 512 slots
    assert fn(65536, 26744, 64, 0, 1, ctypes.byref(a)) == OK and a.value == 0        # the batch alone fills the device
    assert fn(65536, 1682, 64, 1, 0, ctypes.byref(a)) == OK and a.value == 16 * 1682 * 64 * 4
    assert fn(16, 17, 4, 3, 1, ctypes.byref(a)) == OK and a.value == 2 * 16 * 8 * 4   # two tiles: two parts at most


# ---- the Python layer: what is decided before a device is needed
def test_the_model_has_the_method_and_refuses_cpu_tensors(lib):
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    from deeplearningrecommendationsystem_amd.model import MatrixFactorization
    model = MatrixFactorization(5, 6, 4)
    with pytest.raises(CtrHipError):
        model.softmax_nll(torch.tensor([1]), torch.tensor([2]))


def test_the_ops_wrappers_refuse_cpu_tensors(lib):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    x, q, t = torch.zeros(3, 4), torch.zeros(5, 4), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(CtrHipError):
        ops.softmax_full_rows(x, q, t)
    with pytest.raises(CtrHipError):
        ops.softmax_full_cols(x, q, t, torch.zeros(3), torch.zeros(3))
