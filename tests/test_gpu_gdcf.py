"""GPU: the fused GDCF passes (csrc/gdcf.hip) against the float64 restatement tests/gdcf_numpy.py -- loss, dP, dQ over
tile edges, densities, saturated logits and m n > 2^31 -- their determinism, gradient switches and memory, a ten-epoch
run against the fixture recorded from the reference's GDCF_Final.py, recommend() and the script."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gdcf_numpy as gn
from test_gdcf_cpu import F32_LOSS_RTOL, F32_METRIC_ATOL, F32_PARAM_RTOL, load_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg():
    import deeplearningrecommendationsystem_amd as pkg
    from deeplearningrecommendationsystem_amd import ops
    return pkg, ops


def _matrix(Y):
    u, i = np.nonzero(Y)
    return _pkg()[0].implicit_matrix(u, i, Y.shape[0], Y.shape[1])


def _run_passes(P, Q, mat):
    _, ops = _pkg()
    p, q = torch.from_numpy(P).float().cuda(), torch.from_numpy(Q).float().cuda()
    loss, dp = ops.gdcf_rows(p, q, mat.data)
    dq = ops.gdcf_cols(p, q, mat.transposed(), torch.ones((), device="cuda"))
    return loss.item(), dp.cpu().numpy(), dq.cpu().numpy()


def _check(P, Q, Y, rel=1e-4):
    """loss to 1e-5 relative; each gradient element within ``rel`` of the sum of the magnitudes it adds up (with the
    fp32 error of the scores it depends on)"""
    P32, Q32 = P.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)
    loss, dP, dQ = _run_passes(P, Q, _matrix(Y))
    ref_loss, ref_dP, ref_dQ = gn.loss_grads(P32, Q32, Y)
    assert np.isfinite(loss) and np.isfinite(dP).all() and np.isfinite(dQ).all()
    np.testing.assert_allclose(loss, ref_loss, rtol=1e-5, atol=1e-30)
    S = P32 @ Q32.T
    g_abs = np.abs(1 / (1 + np.exp(-np.clip(S, -700, 700))) - Y) + 1e-6 * (np.abs(P32) @ np.abs(Q32).T)
    inv = 1.0 / Y.size
    for got, ref, bound in ((dP, ref_dP, g_abs @ np.abs(Q32)), (dQ, ref_dQ, g_abs.T @ np.abs(P32))):
        bad = np.abs(got - ref) > rel * bound * inv + 1e-30
        assert not bad.any(), (got[bad][:5], ref[bad][:5], (bound * inv)[bad][:5])


def _init(kind, m, n, k, rng):
    if kind == "normal":
        return rng.normal(0, 0.1, (m, k)), rng.normal(0, 0.1, (n, k))
    return rng.random((m, k)), rng.random((n, k))


def _ratings(m, n, density, rng):
    Y = (rng.random((m, n)) < density).astype(np.uint8)
    Y[::3] = 0      # users with no positives
    return Y


@pytest.mark.parametrize("shape", [(1, 1, 1), (17, 65, 3), (129, 200, 100), (943, 1682, 100), (64, 4096, 7),
                                   (70, 130, 256), (65, 63, 17)])
@pytest.mark.parametrize("init", ["normal", "uniform"])
def test_loss_and_gradients_against_float64(shape, init):
    m, n, k = shape
    rng = np.random.default_rng(m * 7 + n + k)
    P, Q = _init(init, m, n, k, rng)
    _check(P, Q, _ratings(m, n, 0.05, rng))


@pytest.mark.parametrize("density", [0.0, 1.0])
@pytest.mark.parametrize("init", ["normal", "uniform"])
def test_empty_and_full_matrices(density, init):
    rng = np.random.default_rng(5)
    P, Q = _init(init, 129, 200, 100, rng)
    _check(P, Q, np.full((129, 200), int(density), dtype=np.uint8))


def test_padding_columns_are_excluded():
    """num_items = 70 -> 58 padding columns per row; ones written into them must change nothing"""
    rng = np.random.default_rng(9)
    P, Q = _init("normal", 40, 70, 12, rng)
    Y = _ratings(40, 70, 0.2, rng)
    mat = _matrix(Y)
    clean = _run_passes(P, Q, mat)
    mat.data[:, 70:] = 1
    mat._t = None
    dirty = _run_passes(P, Q, mat)
    assert clean[0] == dirty[0]
    assert np.array_equal(clean[1], dirty[1]) and np.array_equal(clean[2], dirty[2])


def test_saturated_logits():
    rng = np.random.default_rng(1)
    m, n, k = 50, 90, 4
    P = rng.choice([-1.0, 1.0], (m, k)) * np.sqrt(20.0)
    Q = rng.choice([-1.0, 1.0], (n, k)) * np.sqrt(20.0)    # scores in {0, +-40, +-80}
    Y = _ratings(m, n, 0.5, rng)
    _check(P, Q, Y)


def test_bitwise_deterministic():
    rng = np.random.default_rng(2)
    P, Q = _init("uniform", 943, 1682, 100, rng)
    mat = _matrix(_ratings(943, 1682, 0.05, rng))
    a, b = _run_passes(P, Q, mat), _run_passes(P, Q, mat)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_gradient_switches():
    pkg, _ = _pkg()
    rng = np.random.default_rng(4)
    mat = _matrix(_ratings(300, 500, 0.05, rng))
    model = pkg.GDCF(300, 500, k=32, seed=3)
    loss = model(mat)
    loss.backward()
    full_p, full_q = model.P.grad.clone(), model.Q.grad.clone()
    with torch.no_grad():
        loss_ng = model(mat)
    assert loss_ng.item() == loss.item() and loss_ng.requires_grad is False
    model.zero_grad()
    model.P.requires_grad_(False)
    model(mat).backward()
    assert model.P.grad is None
    assert torch.equal(model.Q.grad, full_q)
    model.P.requires_grad_(True)
    model.Q.requires_grad_(False)
    model.zero_grad()
    model(mat).backward()
    assert model.Q.grad is None and torch.equal(model.P.grad, full_p)
    # the upstream gradient scales both
    model.Q.requires_grad_(True)
    model.zero_grad()
    (model(mat) * 3.0).backward()
    torch.testing.assert_close(model.P.grad, full_p * 3.0, rtol=1e-6, atol=0)
    torch.testing.assert_close(model.Q.grad, full_q * 3.0, rtol=1e-6, atol=0)


def test_beyond_2_31_entries():
    """70 000 x 40 000 (2.8e9 entries), k = 16: sampled dP / dQ rows (the last ones included) against float64 on the
    host, the loss against a chunked float64 evaluation"""
    _, ops = _pkg()
    m, n, k = 70_000, 40_000, 16
    g = torch.Generator(device="cuda").manual_seed(0)
    p = (torch.randn(m, k, device="cuda", generator=g) * 0.3).contiguous()
    q = (torch.randn(n, k, device="cuda", generator=g) * 0.3).contiguous()
    nnz = 3_000_000
    u = torch.randint(0, m, (nnz,), device="cuda", generator=g)
    i = torch.randint(0, n, (nnz,), device="cuda", generator=g)
    u = torch.cat([u, torch.tensor([m - 1], device="cuda")])
    i = torch.cat([i, torch.tensor([n - 1], device="cuda")])
    mat = _pkg()[0].implicit_matrix(u, i, m, n)
    loss, dp = ops.gdcf_rows(p, q, mat.data)
    dq = ops.gdcf_cols(p, q, mat.transposed(), torch.ones((), device="cuda"))
    inv = 1.0 / (m * n)
    P64, Q64 = p.double().cpu().numpy(), q.double().cpu().numpy()
    for rows, X, Z, grad, ys in (
            ([0, 1, 31_337, m - 2, m - 1], P64, Q64, dp, lambda r: mat.data[r, :n]),
            ([0, 5, 20_000, n - 2, n - 1], Q64, P64, dq, lambda r: mat.data[:, r].t())):
        Y = ys(torch.tensor(rows, device="cuda")).double().cpu().numpy()
        S = X[rows] @ Z.T
        G = 1 / (1 + np.exp(-S)) - Y
        ref = G @ Z * inv
        bound = (np.abs(G) + 1e-6) @ np.abs(Z) * inv
        got = grad[rows].double().cpu().numpy()
        assert (np.abs(got - ref) <= 1e-4 * bound).all()
    total = torch.zeros((), dtype=torch.float64, device="cuda")
    pd_, qd = p.double(), q.double()
    for a in range(0, m, 4096):
        s = pd_[a:a + 4096] @ qd.T
        y = mat.data[a:a + 4096, :n].double()
        total += ((s.clamp_min(0) - y * s) + torch.log1p(torch.exp(-s.abs()))).sum()
    np.testing.assert_allclose(loss.item(), total.item() * inv, rtol=1e-5)


def test_epoch_memory_stays_far_below_the_score_matrix():
    pkg, _ = _pkg()
    m, n, k = 20_000, 16_000, 64          # an fp32 m x n matrix would be 1.28 GB
    rng = np.random.default_rng(6)
    u, i = rng.integers(0, m, 400_000), rng.integers(0, n, 400_000)
    mat = pkg.implicit_matrix(u, i, m, n)
    model = pkg.GDCF(m, n, k=k, seed=1)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)

    def epoch():
        loss = model(mat)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss

    epoch()       # optimizer state and the transposed matrix exist from here on
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    epoch()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 64 << 20


def test_ten_epochs_against_the_reference_fixture():
    pkg, _ = _pkg()
    from deeplearningrecommendationsystem_amd import optim
    z, Y, P0, Q0 = load_fixture()
    m, n = Y.shape
    mat = _matrix(Y)
    model = pkg.GDCF(m, n, k=int(z["k"]), seed=int(z["seed"]))
    np.testing.assert_array_equal(model.P.detach().cpu().numpy(), P0.astype(np.float32))
    opt = optim.Adam(model.parameters(), lr=float(z["lr"]))
    losses, metrics = [], []
    for _ in range(int(z["epochs"])):
        loss = model(mat)
        loss.backward()
        recs = model.recommend(n=50)     # the scores before this epoch's step, all items
        opt.step()
        opt.zero_grad()
        losses.append(loss.item())
        metrics.append(pkg.recall_precision_f1(recs, z["test_users"], z["test_items"]))
    np.testing.assert_allclose(losses, z["losses"], rtol=F32_LOSS_RTOL)
    np.testing.assert_allclose(metrics, np.stack([z["recalls"], z["precisions"], z["f1s"]], 1), rtol=0,
                               atol=F32_METRIC_ATOL)
    P, Q = model.P.detach().double().cpu().numpy(), model.Q.detach().double().cpu().numpy()
    np.testing.assert_allclose(P[z["rows_p"]], z["p_rows"], rtol=F32_PARAM_RTOL)
    np.testing.assert_allclose(Q[z["rows_q"]], z["q_rows"], rtol=F32_PARAM_RTOL)
    np.testing.assert_allclose([P.sum(), Q.sum()], [z["p_sum"], z["q_sum"]], rtol=F32_PARAM_RTOL)


def test_torch_adam_trains_too():
    pkg, _ = _pkg()
    rng = np.random.default_rng(8)
    mat = _matrix(_ratings(200, 300, 0.1, rng))
    model = pkg.GDCF(200, 300, k=16, seed=0)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    losses = []
    for _ in range(5):
        loss = model(mat)
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(loss.item())
    assert all(b < a for a, b in zip(losses, losses[1:]))


@pytest.mark.parametrize("exclude", [False, True])
def test_recommend_matches_numpy_ranking(exclude):
    pkg, _ = _pkg()
    rng = np.random.default_rng(12)
    m, n, k = 70, 150, 5
    Y = _ratings(m, n, 0.3, rng)
    Y[5, :] = 1                     # a user with nothing left to recommend
    mat = _matrix(Y)
    model = pkg.GDCF(m, n, k=k, seed=0)
    P = rng.integers(-2, 3, (m, k)).astype(np.float32)   # exact integer scores: many ties
    Q = rng.integers(-2, 3, (n, k)).astype(np.float32)
    with torch.no_grad():
        model.P.copy_(torch.from_numpy(P))
        model.Q.copy_(torch.from_numpy(Q))
        model(mat)
    S = P.astype(np.float64) @ Q.T.astype(np.float64)
    if exclude:
        S[Y != 0] = -np.inf
    want = gn.top(S, 60)
    if exclude:
        want = np.where(np.take_along_axis(S, want, 1) == -np.inf, -1, want)
    users = [0, 5, 69, 33]
    got = model.recommend(users, n=60, exclude_rated=exclude).cpu().numpy()
    np.testing.assert_array_equal(got, want[users])
    np.testing.assert_array_equal(model.recommend(n=60, exclude_rated=exclude).cpu().numpy(), want)


def test_refusals():
    pkg, ops = _pkg()
    Y = np.zeros((10, 20), dtype=np.uint8)
    Y[1, 2] = 1
    mat = _matrix(Y)
    p, q = torch.rand(10, 8, device="cuda"), torch.rand(20, 8, device="cuda")
    big = ops.GDCF_MAX_DIM + 1
    with pytest.raises(ValueError, match="k = "):
        ops.gdcf_rows(torch.rand(10, big, device="cuda"), torch.rand(20, big, device="cuda"), mat.data)
    with pytest.raises(ValueError):
        ops.gdcf_rows(p, torch.rand(20, 9, device="cuda"), mat.data)                  # k differs
    with pytest.raises(ValueError):
        ops.gdcf_rows(p.double(), q.double(), mat.data)                                # dtype
    with pytest.raises(ValueError):
        ops.gdcf_rows(torch.rand(8, 10, device="cuda").t(), q, mat.data)                # not contiguous
    with pytest.raises(ValueError):
        ops.gdcf_rows(torch.rand(11, 8, device="cuda"), q, mat.data)                    # rows differ from the matrix
    with pytest.raises(ValueError):
        ops.gdcf_rows(p, torch.rand(65, 8, device="cuda"), mat.data)                    # more items than columns
    with pytest.raises(ValueError):
        ops.gdcf_cols(p, q, mat.data, torch.ones((), device="cuda"))                    # not the transposed matrix
    with pytest.raises(ValueError):
        pkg.GDCF(11, 20, k=4)(mat)
    with pytest.raises(ValueError):
        pkg.GDCF(10, 20, k=big)


def test_script_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gdcf.py")], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("epoch")]
    assert len(lines) == 10, out.stdout[-2000:]
    losses = [float(ln.split("loss")[1].split()[0]) for ln in lines]
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert "recall" in lines[-1] and "precision" in lines[-1] and "F1" in lines[-1]
