"""CPU: the numpy restatement tests/gdcf_numpy.py against the fixture recorded from the reference's GDCF_Final.py
(dev/make_gdcf_golden.py), in float64 (the reference's arithmetic: pins the pre-step evaluation, the divisor and the
no-exclusion rule) and in float32 (the package's arithmetic: its gap calibrates the GPU training test's tolerance);
and the C-ABI declarations of the GDCF entry points."""
import os
import re

import numpy as np
import pytest

import gdcf_numpy as gn
from golden_util import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# float32 against the float64 reference over the fixture's ten epochs (the GPU training test uses the same bounds):
# relative loss gap, absolute gap of recall / precision / F1, relative gap of the final P / Q samples and checksums.
# The float32 restatement shows 3e-8, 0 and 3.6e-5; the bounds leave room for the kernels' other summation order.
F32_LOSS_RTOL = 1e-5
F32_METRIC_ATOL = 5e-4
F32_PARAM_RTOL = 2e-4


def load_fixture():
    z = np.load(os.path.join(GOLDEN_DIR, "gdcf", "gdcf_ml100k.npz"), allow_pickle=False)
    m, n = int(z["num_users"]), int(z["num_items"])
    Y = np.unpackbits(z["bitmap"])[:m * n].reshape(m, n)
    rs = np.random.RandomState(int(z["seed"]))
    k = int(z["k"])
    P0, Q0 = rs.rand(m, k), rs.rand(n, k)
    return z, Y, P0, Q0


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def _run(fixture, dtype):
    z, Y, P0, Q0 = fixture
    return gn.train(P0, Q0, Y, z["test_users"].astype(np.int64), z["test_items"].astype(np.int64),
                    epochs=int(z["epochs"]), lr=float(z["lr"]), dtype=dtype)


def _metrics(z):
    return np.stack([z["recalls"], z["precisions"], z["f1s"]], 1)


def test_float64_restatement_reproduces_the_reference(fixture):
    z = fixture[0]
    losses, metrics, P, Q = _run(fixture, np.float64)
    np.testing.assert_allclose(losses, z["losses"], rtol=1e-12)
    np.testing.assert_allclose(metrics, _metrics(z), rtol=0, atol=1e-12)
    np.testing.assert_allclose(P[z["rows_p"]], z["p_rows"], rtol=1e-10)
    np.testing.assert_allclose(Q[z["rows_q"]], z["q_rows"], rtol=1e-10)
    np.testing.assert_allclose([P.sum(), Q.sum()], [z["p_sum"], z["q_sum"]], rtol=1e-12)


def test_float32_restatement_within_the_documented_tolerance(fixture):
    z = fixture[0]
    losses, metrics, P, Q = _run(fixture, np.float32)
    np.testing.assert_allclose(losses, z["losses"], rtol=F32_LOSS_RTOL)
    np.testing.assert_allclose(metrics, _metrics(z), rtol=0, atol=F32_METRIC_ATOL)
    np.testing.assert_allclose(P[z["rows_p"]], z["p_rows"], rtol=F32_PARAM_RTOL)
    np.testing.assert_allclose(Q[z["rows_q"]], z["q_rows"], rtol=F32_PARAM_RTOL)
    np.testing.assert_allclose([P.sum(dtype=np.float64), Q.sum(dtype=np.float64)], [z["p_sum"], z["q_sum"]],
                               rtol=F32_PARAM_RTOL)


def test_restated_gradients_match_finite_differences():
    rng = np.random.default_rng(0)
    P, Q = rng.normal(0, 0.5, (5, 3)), rng.normal(0, 0.5, (7, 3))
    Y = (rng.random((5, 7)) < 0.3).astype(np.uint8)
    _, dP, dQ = gn.loss_grads(P, Q, Y)
    h = 1e-6
    for X, dX, which in ((P, dP, 0), (Q, dQ, 1)):
        for idx in [(0, 0), (2, 1), (X.shape[0] - 1, 2)]:
            Xp, Xm = X.copy(), X.copy()
            Xp[idx] += h
            Xm[idx] -= h
            args_p = (Xp, Q) if which == 0 else (P, Xp)
            args_m = (Xm, Q) if which == 0 else (P, Xm)
            fd = (gn.loss_grads(*args_p, Y)[0] - gn.loss_grads(*args_m, Y)[0]) / (2 * h)
            assert abs(fd - dX[idx]) < 1e-8


def test_header_declares_the_gdcf_entry_points():
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    for name in ("ctr_gdcf_workspace_bytes", "ctr_gdcf_rows", "ctr_gdcf_cols"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    define = int(re.search(r"#define\s+CTR_GDCF_MAX_DIM\s+(\d+)", text).group(1))
    from deeplearningrecommendationsystem_amd import _lib, ops
    assert _lib.CTR_GDCF_MAX_DIM == define == ops.GDCF_MAX_DIM
    assert _lib.ABI_VERSION == 36
    for name in ("ctr_gdcf_workspace_bytes", "ctr_gdcf_rows", "ctr_gdcf_cols"):
        assert name in _lib.SIGNATURES


def test_gdcf_is_exported_and_refuses_bad_shapes_without_a_gpu():
    import deeplearningrecommendationsystem_amd as pkg
    from deeplearningrecommendationsystem_amd import ops
    assert pkg.GDCF is not None
    with pytest.raises(ValueError):
        pkg.GDCF(4, 5, k=ops.GDCF_MAX_DIM + 1, device="cpu")
    with pytest.raises(ValueError):
        pkg.GDCF(4, 5, k=0, device="cpu")
