"""GPU: the full softmax over the catalogue (csrc/softmax_full.hip) against the float64 restatement
tests/softmax_full_numpy.py -- nll, lse, dX and dQ over tile edges, both inits and every split of both passes -- its edge
cases (one item, one shared target, duplicate rows, saturated and huge logits, one-hot rows, bad targets), determinism
and locality, ``MatrixFactorization.softmax_nll`` against float64 autograd, its switches, memory and training, and the
script.

Worst error / bound ratios seen on the MI355X are quoted in DESIGN.md section 4r; every check prints its own."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import softmax_full_numpy as sn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (17, 65, 3), (129, 200, 100), (64, 4096, 7), (70, 130, 256), (65, 63, 17), (300, 1682, 64)]
SPLITS = [0, 1, 2, 3]


def _pkg():
    import deeplearningrecommendationsystem_amd as pkg
    from deeplearningrecommendationsystem_amd import ops
    return pkg, ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(X, Q, t, g, splits=0, grad=True, with_nll=True):
    """(nll, lse, dX, dQ) of the two passes as numpy; dX = g * the row pass's unit gradient and the column pass is
    handed nll, as the model does both"""
    _, ops = _pkg()
    x, q, tt, gg = _dev(X), _dev(Q), _dev(t), _dev(g)
    nll, lse, gx = ops.softmax_full_rows(x, q, tt, grad=grad, splits=splits)
    dq = ops.softmax_full_cols(x, q, tt, lse, gg, splits=splits, nll=nll if with_nll else None)
    dx = (gx * gg.unsqueeze(1)).cpu().numpy() if grad else None
    return nll.cpu().numpy(), lse.cpu().numpy(), dx, dq.cpu().numpy()


def _reference(X, Q, t, g):
    """the float64 reference of the fp32-rounded inputs and its four bounds"""
    X64, Q64, g64 = X.astype(np.float64), Q.astype(np.float64), g.astype(np.float64)
    return sn.nll_grads(X64, Q64, t, g64), sn.bounds(X64, Q64, t, g64)


def _compare(got, ref, bounds, what, gradients=True):
    nll, lse, dx, dq = got
    ref_nll, ref_lse, ref_dx, ref_dq = ref
    b_lse, b_nll, b_dx, b_dq = bounds
    pairs = [("lse", lse, ref_lse, b_lse), ("nll", nll, ref_nll, b_nll)]
    if gradients:
        pairs += [("dX", dx, ref_dx, b_dx), ("dQ", dq, ref_dq, b_dq)]
    ratios = {}
    for name, a, r, bound in pairs:
        assert np.isfinite(a).all(), (what, name)
        ratios[name] = float((np.abs(a - r) / (bound + 1e-300)).max())
    print(f"softmax_full {what}: worst error / bound " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for name, a, r, bound in pairs:
        bad = np.abs(a - r) > bound + 1e-30
        assert not bad.any(), (what, name, ratios[name], a[bad][:5], r[bad][:5], bound[bad][:5])


def _init(kind, b, n, k, rng):
    if kind == "normal":
        return rng.normal(0, 0.1, (b, k)).astype(np.float32), rng.normal(0, 0.1, (n, k)).astype(np.float32)
    return rng.random((b, k)).astype(np.float32), rng.random((n, k)).astype(np.float32)


def _targets(b, n, rng):
    t = rng.integers(0, n, b)
    t[0] = n - 1
    t[b // 2] = 0
    return t.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _case(shape, init):
    """inputs and float64 reference of one parity case, computed once and shared by the splits"""
    b, n, k = shape
    rng = np.random.default_rng(b * 7 + n + k)
    X, Q = _init(init, b, n, k, rng)
    t = _targets(b, n, rng)
    g = (rng.random(b) / b).astype(np.float32)
    return (X, Q, t, g) + _reference(X, Q, t, g)


# ---- parity
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("init", ["normal", "uniform"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_passes_against_float64(shape, init, splits):
    X, Q, t, g, ref, bounds = _case(shape, init)
    _compare(_run(X, Q, t, g, splits), ref, bounds, f"{shape} {init} splits={splits}")


@pytest.mark.parametrize("splits", [0, 2])
def test_column_pass_from_lse_alone(splits):
    """without nll a target's entry is g (exp(z_t - lse) - 1): the same bounds away from one-hot rows"""
    X, Q, t, g, ref, bounds = _case((129, 200, 100), "normal")
    _compare(_run(X, Q, t, g, splits, with_nll=False), ref, bounds, f"lse alone splits={splits}")


# ---- edge cases
@pytest.mark.parametrize("splits", SPLITS)
def test_one_item_gives_exact_zeros(splits):
    rng = np.random.default_rng(3)
    X, Q = _init("uniform", 70, 1, 20, rng)
    nll, lse, dx, dq = _run(X, Q, np.zeros(70, dtype=np.int64), rng.random(70).astype(np.float32), splits)
    assert not nll.any() and not dx.any() and not dq.any()
    np.testing.assert_allclose(lse, X.astype(np.float64) @ Q[0].astype(np.float64), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("splits", [0, 2])
def test_all_rows_share_one_target(splits):
    rng = np.random.default_rng(4)
    X, Q = _init("normal", 150, 90, 24, rng)
    t = np.full(150, 37, dtype=np.int64)                  # one dQ row collects 150 indicator terms
    g = (rng.random(150) / 150).astype(np.float32)
    _compare(_run(X, Q, t, g, splits), *_reference(X, Q, t, g), f"shared target splits={splits}")


def test_duplicate_batch_rows():
    rng = np.random.default_rng(5)
    X, Q = _init("uniform", 40, 130, 12, rng)
    rows = np.repeat(np.arange(40), 3)[:100]
    X, t = X[rows], np.repeat(_targets(40, 130, rng), 3)[:100]
    g = (rng.random(100) / 100).astype(np.float32)
    got = _run(X, Q, t, g, 1)
    _compare(got, *_reference(X, Q, t, g), "duplicate rows")
    unit = _run(X, Q, t, np.ones(100, dtype=np.float32), 1)
    for a in (unit[0], unit[1], unit[2]):                  # the copies of a row agree bitwise
        assert np.array_equal(a[0::3][:33], a[1::3][:33]) and np.array_equal(a[0::3][:33], a[2::3][:33])


@pytest.mark.parametrize("target", ["random", "argmax"])
@pytest.mark.parametrize("splits", [0, 2])
def test_saturated_scores(target, splits):
    rng = np.random.default_rng(1)
    b, n, k = 50, 90, 4
    X = (rng.choice([-1.0, 1.0], (b, k)) * np.sqrt(20.0)).astype(np.float32)
    Q = (rng.choice([-1.0, 1.0], (n, k)) * np.sqrt(20.0)).astype(np.float32)     # scores in {0, +-40, +-80}
    t = _targets(b, n, rng) if target == "random" else (X.astype(np.float64) @ Q.T.astype(np.float64)).argmax(1)
    g = (rng.random(b) / b).astype(np.float32)
    _compare(_run(X, Q, t, g, splits), *_reference(X, Q, t, g), f"saturated {target} splits={splits}")


@pytest.mark.parametrize("splits", [0, 3])
def test_one_hot_rows(splits):
    rng = np.random.default_rng(6)
    b, n, k = 70, 130, 16
    X, Q = _init("normal", b, n, k, rng)
    Q[:b] += 300 * X                                       # the target's probability is 1 to fp32 precision
    t = np.arange(b, dtype=np.int64)
    g = (rng.random(b) / b).astype(np.float32)
    assert np.abs(X.astype(np.float64) @ Q.T.astype(np.float64)).max() < 100
    _compare(_run(X, Q, t, g, splits), *_reference(X, Q, t, g), f"one-hot splits={splits}")


@pytest.mark.parametrize("splits", [0, 2])
def test_huge_logits_stay_finite(splits):
    """|z| up to about 2000: exp of a positive argument would overflow.  The gradient bounds assume score errors below
    1e-4, so only nll and lse are compared here; the gradients must be finite."""
    rng = np.random.default_rng(7)
    b, n, k = 65, 200, 64
    X, Q = rng.normal(0, 8, (b, k)).astype(np.float32), rng.normal(0, 8, (n, k)).astype(np.float32)
    t = _targets(b, n, rng)
    g = (rng.random(b) / b).astype(np.float32)
    got = _run(X, Q, t, g, splits)
    assert np.isfinite(got[2]).all() and np.isfinite(got[3]).all()
    _compare(got, *_reference(X, Q, t, g), f"huge logits splits={splits}", gradients=False)


def test_a_target_outside_the_catalogue_is_flagged_and_never_read():
    _, ops = _pkg()
    rng = np.random.default_rng(8)
    X, Q = _init("normal", 40, 70, 8, rng)
    t = _targets(40, 70, rng)
    bad = t.copy()
    bad[3], bad[4] = 70, -1
    g = np.full(40, 1.0, dtype=np.float32)
    x, q, gg = _dev(X), _dev(Q), _dev(g)
    for splits in (1, 2):
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        clean = ops.softmax_full_rows(x, q, _dev(t), splits=splits, err_flag=flag)
        assert flag.item() == 0
        nll, lse, gx = ops.softmax_full_rows(x, q, _dev(bad), splits=splits, err_flag=flag)
        assert flag.item() == 1
        keep = np.ones(40, dtype=bool)
        keep[[3, 4]] = False
        keep = torch.from_numpy(keep).cuda()
        assert torch.equal(nll[keep], clean[0][keep]) and torch.equal(lse, clean[1]) and torch.equal(gx[keep], clean[2][keep])
        assert torch.equal(nll[~keep], lse[~keep])                             # no target term
        # no indicator: the rows' columns are their softmax alone, so dQ sums to the sum of g x over the other rows'
        dq = ops.softmax_full_cols(x, q, _dev(bad), lse, gg, splits=splits).double().cpu().numpy()
        z, ref_lse, _ = sn.forward(X.astype(np.float64), Q.astype(np.float64), t)
        G = np.exp(z - ref_lse[:, None])
        for b in range(40):
            if b not in (3, 4):
                G[b, t[b]] -= 1.0
        ref = G.T @ X.astype(np.float64)
        assert np.abs(dq - ref).max() < 1e-4 * (np.abs(G).T @ np.abs(X)).max()


# ---- determinism and locality
@pytest.mark.parametrize("splits", [0, 1, 3])
def test_bitwise_deterministic(splits):
    X, Q, t, g, _, _ = _case((300, 1682, 64), "uniform")
    a, b = _run(X, Q, t, g, splits), _run(X, Q, t, g, splits)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("splits", [1, 2])
def test_a_row_does_not_depend_on_its_batch(splits):
    X, Q, t, g, _, _ = _case((129, 200, 100), "normal")
    full = _run(X, Q, t, g, splits)
    perm = np.random.default_rng(9).permutation(129)
    moved = _run(X[perm], Q, t[perm], g[perm], splits)
    part = _run(X[37:101], Q, t[37:101], g[37:101], splits)
    for a, b, c in zip(full[:3], moved[:3], part[:3]):                         # nll, lse, dX
        assert np.array_equal(a[perm], b) and np.array_equal(a[37:101], c)


def test_no_grad_rows_are_the_same_bits():
    X, Q, t, g, _, _ = _case((300, 1682, 64), "normal")
    for splits in (0, 2):
        a, b = _run(X, Q, t, g, splits), _run(X, Q, t, g, splits, grad=False)
        assert b[2] is None and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])


def test_refusals():
    _, ops = _pkg()
    x, q = torch.rand(10, 8, device="cuda"), torch.rand(20, 8, device="cuda")
    t = torch.zeros(10, dtype=torch.int64, device="cuda")
    lse, g = torch.zeros(10, device="cuda"), torch.ones(10, device="cuda")
    big = ops.SOFTMAX_FULL_MAX_DIM + 1
    with pytest.raises(ValueError, match="k = "):
        ops.softmax_full_rows(torch.rand(10, big, device="cuda"), torch.rand(20, big, device="cuda"), t)
    with pytest.raises(ValueError, match="columns"):
        ops.softmax_full_rows(x, torch.rand(20, 9, device="cuda"), t)           # k differs
    with pytest.raises(ValueError):
        ops.softmax_full_rows(x.double(), q.double(), t)                        # dtype
    with pytest.raises(ValueError):
        ops.softmax_full_rows(torch.rand(8, 10, device="cuda").t(), q, t)       # not contiguous
    with pytest.raises(ValueError, match="targets"):
        ops.softmax_full_rows(x, q, t[:9])                                      # length
    with pytest.raises(ValueError, match="targets"):
        ops.softmax_full_rows(x, q, t.int())                                    # dtype
    with pytest.raises(ValueError, match="splits"):
        ops.softmax_full_rows(x, q, t, splits=-1)
    with pytest.raises(ValueError, match="lse"):
        ops.softmax_full_cols(x, q, t, lse[:9], g)
    with pytest.raises(ValueError, match="upstream"):
        ops.softmax_full_cols(x, q, t, lse, g.double())
    with pytest.raises(ValueError):
        ops.softmax_full_rows(x, torch.rand(0, 8, device="cuda"), t)            # an empty catalogue
    nll, lse0, gx = ops.softmax_full_rows(x[:0], q, t[:0])                      # an empty batch is not an error
    assert nll.shape == (0,) and gx.shape == (0, 8)
    assert not ops.softmax_full_cols(x[:0], q, t[:0], lse0, g[:0]).any()


# ---- the model
def _model(nu=50, ni=130, k=20, seed=0):
    from deeplearningrecommendationsystem_amd.model import MatrixFactorization
    torch.manual_seed(seed)
    model = MatrixFactorization(nu, ni, k)
    with torch.no_grad():                                   # xavier rows of 180 are tiny: make the softmax uneven
        model.user_embeddings.weight.mul_(8.0)
        model.item_embeddings.weight.mul_(8.0)
    return model.cuda()


def _batch(nu, ni, b, seed):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, nu, b)
    u[: b // 4] = u[b // 4: 2 * (b // 4)]                   # repeated users
    i = _targets(b, ni, rng)
    return torch.from_numpy(u).cuda(), torch.from_numpy(i).cuda()


def test_model_against_float64_autograd():
    nu, ni, k, b = 50, 130, 20, 96
    model = _model(nu, ni, k)
    u, i = _batch(nu, ni, b, 11)
    nll = model.softmax_nll(u, i)
    assert nll.shape == (b,) and nll.dtype == torch.float32 and nll.requires_grad
    nll.mean().backward()
    P = model.user_embeddings.weight.detach().double().cpu().requires_grad_(True)
    Q = model.item_embeddings.weight.detach().double().cpu().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(P[u.cpu()] @ Q.T, i.cpu(), reduction="none")
    ref.mean().backward()
    un, inn = u.cpu().numpy(), i.cpu().numpy()
    X, g = P.detach().numpy()[un], np.full(b, 1.0 / b)
    b_lse, b_nll, b_dx, b_dq = sn.bounds(X, Q.detach().numpy(), inn, g)
    b_du = np.zeros((nu, k))
    np.add.at(b_du, un, b_dx)                               # a user's row adds up its samples' dX
    err = {"nll": np.abs(nll.detach().double().cpu().numpy() - ref.detach().numpy()) / b_nll,
           "dU": np.abs(model.user_embeddings.weight.grad.double().cpu().numpy() - P.grad.numpy()) / (b_du + 1e-300),
           "dQ": np.abs(model.item_embeddings.weight.grad.double().cpu().numpy() - Q.grad.numpy()) / b_dq}
    print("softmax_nll model: worst error / bound " + "  ".join(f"{k_} {v.max():.3f}" for k_, v in err.items()))
    untouched = np.setdiff1d(np.arange(nu), un)
    assert not model.user_embeddings.weight.grad[torch.from_numpy(untouched).cuda()].any()
    for name, v in err.items():
        assert (v <= 1.0).all(), (name, v.max())


def _sum_floors(model, u, i, scale):
    """(user, item) table floors for comparing two evaluations of the same gradient sums: the fp32 products and adds of
    a sum may round (and, for a repeated user's rows, be ordered) differently, each by at most a few ulps of the
    magnitudes added up -- 8 eps sum |terms|, the sums being those of ``sn.bounds`` (its 1e-4 taken out)"""
    un, inn = u.cpu().numpy(), i.cpu().numpy()
    P = model.user_embeddings.weight.detach().double().cpu().numpy()
    Q = model.item_embeddings.weight.detach().double().cpu().numpy()
    _, _, b_dx, b_dq = sn.bounds(P[un], Q, inn, np.full(un.shape[0], scale))
    b_du = np.zeros_like(P)
    np.add.at(b_du, un, b_dx)
    eps8 = 8 * np.finfo(np.float32).eps / 1e-4
    return b_du * eps8, b_dq * eps8


def _same_sums(got, want, floor):
    got, want = got.double().cpu().numpy(), want.double().cpu().numpy()
    assert (np.abs(got - want) <= 1e-6 * np.abs(want) + floor).all(), np.abs(got - want).max()


def test_model_gradient_switches():
    model = _model()
    u, i = _batch(50, 130, 96, 12)
    wu, wi = model.user_embeddings.weight, model.item_embeddings.weight
    floor_u, floor_i = _sum_floors(model, u, i, 1.0 / 96)
    before = model(u, i).detach().clone()
    loss = model.softmax_nll(u, i)
    loss.mean().backward()
    full_u, full_i = wu.grad.clone(), wi.grad.clone()
    with torch.no_grad():
        held_out = model.softmax_nll(u, i)
    assert torch.equal(held_out, loss.detach()) and held_out.requires_grad is False
    model.zero_grad()
    wu.requires_grad_(False)
    model.softmax_nll(u, i).mean().backward()
    assert wu.grad is None and torch.equal(wi.grad, full_i)
    wu.requires_grad_(True)
    wi.requires_grad_(False)
    model.zero_grad()
    model.softmax_nll(u, i).mean().backward()
    assert wi.grad is None
    _same_sums(wu.grad, full_u, floor_u)                                        # a repeated user's adds may reorder
    wu.requires_grad_(False)
    frozen = model.softmax_nll(u, i)
    assert frozen.requires_grad is False and torch.equal(frozen, held_out)
    # the upstream gradient scales both (to rtol 1e-6 of each element, beside the rounding of the sums themselves:
    # the upstream gradient multiplies every term ahead of its sum, so 3 g rounds each term anew)
    wu.requires_grad_(True)
    wi.requires_grad_(True)
    model.zero_grad()
    (model.softmax_nll(u, i).mean() * 3.0).backward()
    _same_sums(wu.grad, full_u * 3.0, 3 * floor_u)
    _same_sums(wi.grad, full_i * 3.0, 3 * floor_i)
    model.zero_grad()
    assert torch.equal(model(u, i), before)                                     # forward is what it was


def test_model_raises_index_error_for_ids_outside_the_tables():
    model = _model()
    model.check_index = True
    u, i = _batch(50, 130, 32, 13)
    for bad_u, bad_i in ((50, None), (-1, None), (None, 130), (None, -1)):
        uu, ii = u.clone(), i.clone()
        if bad_u is not None:
            uu[5] = bad_u
        if bad_i is not None:
            ii[5] = bad_i
        with pytest.raises(IndexError):
            model.softmax_nll(uu, ii)
    model.softmax_nll(u, i)                                                     # the flag was cleared
    with pytest.raises(ValueError):
        model.softmax_nll(u, i[:-1])
    with pytest.raises(ValueError):
        model.softmax_nll(u.int(), i)


def test_a_bad_user_id_adds_to_no_row_in_backward():
    model = _model()
    u, i = _batch(50, 130, 32, 14)
    keep = torch.ones(32, dtype=torch.bool, device="cuda")
    keep[5] = False
    model.softmax_nll(u[keep], i[keep]).sum().backward()
    want = model.user_embeddings.weight.grad.clone()
    model.zero_grad()
    u[5] = 50
    model.softmax_nll(u, i).sum().backward()
    with pytest.raises(IndexError):
        model.check_bad_index()
    _same_sums(model.user_embeddings.weight.grad, want, _sum_floors(model, u.clamp(max=49), i, 1.0)[0])


def test_step_memory_stays_far_below_the_logits():
    from deeplearningrecommendationsystem_amd.model import MatrixFactorization
    nu, ni, k, b = 1000, 32_768, 64, 8192                  # fp32 logits would be 1 GiB, their gradient another
    torch.manual_seed(0)
    model = MatrixFactorization(nu, ni, k).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    u, i = _batch(nu, ni, b, 15)

    def step():
        loss = model.softmax_nll(u, i).mean()
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=False)                   # gradients stay allocated: they are part of the base
        return loss

    step()       # optimizer state and gradients exist from here on
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 64 << 20


def test_five_adam_steps_lower_the_nll_every_time():
    model = _model(200, 300, 16, seed=1)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    u, i = _batch(200, 300, 2048, 16)
    losses = []
    for _ in range(5):
        loss = model.softmax_nll(u, i).mean()
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(loss.item())
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


def test_script_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "mf_softmax.py"), "--epochs", "2"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("epoch")]
    assert len(lines) == 2, out.stdout[-2000:]
    losses = [float(ln.split("train nll")[1].split()[0]) for ln in lines]
    assert losses[1] < losses[0], losses
    assert "precision@50" in lines[-1] and "recall@50" in lines[-1] and "NDCG@50" in lines[-1] and "MRR" in lines[-1]
