"""Score-level evaluation on the device: ctr_gauc_groups and ctr_score_counts (csrc/score_eval.hip), evaluator.score,
DeviceLoader.user_ids and Trainer.score_epoch.

Reference: score_numpy, a numpy restatement written from the definitions in the kernel file's header comment and pinned
to sklearn's roc_auc_score in test_score_cpu.py.  The per-user counts are integers and compared for exact equality.
The chunk sums of p, (p - y)^2 and y are float64 sums of the same float64 terms in another order: two orders of m
non-negative terms differ by at most m 2^-52 relative (each (m - 1) 2^-53 from the exact sum).  The BCE term is formed
in fp32 on the device and in float64 in the restatement: rtol 1e-5, atol 1e-6 on the mean, what test_gpu_ops.py holds
bce_fwd_kernel's expressions to."""
import math

import numpy as np
import pytest
import torch

import score_numpy as sn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the shared inputs are read-only


def _plan(users):
    from deeplearningrecommendationsystem_amd.evaluator import UserGroups
    return UserGroups(_dev(np.asarray(users, dtype=np.int64)))


def _run_groups(groups, p, y, u2=None, order=None):
    """one ctr_gauc_groups call -> (pos, neg, u2, err) as numpy / int; pos and neg start from a sentinel"""
    from deeplearningrecommendationsystem_amd import ops
    g = groups.num_groups
    pos, neg = (torch.full((g,), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    u2 = torch.zeros(g, dtype=torch.int64, device=DEV) if u2 is None else u2
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.gauc_groups(_dev(p), _dev(y), groups.order if order is None else order, groups.offsets, groups.small_groups,
                    groups.slab_group, groups.slab_first, pos, neg, u2, err)
    return pos.cpu().numpy(), neg.cpu().numpy(), u2.cpu().numpy(), int(err.item())


# ---------------------------------------------------------------------------------------------------------------
# 1. ctr_gauc_groups
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recipe():
    """the mixed input (score_numpy.recipe), plain and with special scores sprinkled in, the plan and the restated
    counts of both"""
    users, y, p = sn.recipe()
    special = sn.with_specials(p, 3)
    plan = sn.user_groups(users)
    want = {name: sn.group_counts(q, y, plan["order"], plan["offsets"]) for name, q in (("plain", p), ("special", special))}
    for t in (users, y, p, special):
        t.setflags(write=False)
    return dict(users=users, y=y, plain=p, special=special, plan=plan, want=want, groups=_plan(users))


@pytest.mark.parametrize("scores", ["plain", "special"])
def test_gauc_groups_equal_the_restatement_on_the_recipe(recipe, scores):
    groups, p, y = recipe["groups"], recipe[scores], recipe["y"]
    for name in ("order", "offsets", "small_groups", "slab_group", "slab_first"):
        assert np.array_equal(getattr(groups, name).cpu().numpy(), recipe["plan"][name]), name
    wpos, wneg, wu2, _ = recipe["want"][scores]
    assert (wu2 > 0).sum() >= 150
    pos, neg, u2, err = _run_groups(groups, p, y)
    assert err == 0
    assert np.array_equal(pos, wpos) and np.array_equal(neg, wneg) and np.array_equal(u2, wu2)
    again = _run_groups(groups, p, y)
    assert all(np.array_equal(a, b) for a, b in zip(again[:3], (pos, neg, u2)))       # run twice: identical
    start = torch.arange(groups.num_groups, dtype=torch.int64, device=DEV) * 3 + (1 << 40)
    _, _, added, _ = _run_groups(groups, p, y, u2=start.clone())
    assert np.array_equal(added, start.cpu().numpy() + wu2)                            # u2_out is added to


@pytest.mark.parametrize("size", [1, 2, 64, 65, 1024, 1025, 2049, 4097])
def test_gauc_groups_single_group(size):
    gen = np.random.default_rng(size)
    y = (gen.random(size) < 0.4).astype(np.float32)
    p = sn.with_specials(np.round(gen.random(size, dtype=np.float32) * 64) / np.float32(64), size + 1, every=5)
    if size >= 2:
        y[:2] = [1, 0]
    groups = _plan(np.full(size, 12345))
    assert groups.num_groups == 1 and groups.max_group == size
    assert groups.small_groups.numel() == (1 if size <= 64 else 0)
    assert groups.slab_first.tolist() == ([] if size <= 64 else list(range(0, size, 1024)))
    wpos, wneg, wu2, _ = sn.group_counts(p, y, np.arange(size), np.array([0, size]))
    pos, neg, u2, err = _run_groups(groups, p, y)
    assert err == 0 and (pos[0], neg[0], u2[0]) == (wpos[0], wneg[0], wu2[0])
    assert pos[0] + neg[0] == size
    again = _run_groups(groups, p, y)
    assert (again[0][0], again[1][0], again[2][0]) == (pos[0], neg[0], u2[0])


@pytest.mark.parametrize("bad", [-1, "n"])
def test_gauc_groups_flag_a_bad_order_entry_and_score_the_rest(recipe, bad):
    groups, p, y, plan = recipe["groups"], recipe["special"], recipe["y"], recipe["plan"]
    n = p.shape[0]
    order = plan["order"].copy()
    sizes = plan["sizes"]
    hit = [int(np.flatnonzero(sizes == s)[0]) for s in (3, 2049)]                      # one small group, one in slabs
    for g in hit:
        order[plan["offsets"][g] + 1] = n if bad == "n" else bad
    wpos, wneg, wu2, werr = sn.group_counts(p, y, order, plan["offsets"])
    assert werr == 1
    pos, neg, u2, err = _run_groups(groups, p, y, order=_dev(order))
    assert err == 1
    assert np.array_equal(pos, wpos) and np.array_equal(neg, wneg) and np.array_equal(u2, wu2)
    clean = recipe["want"]["special"]
    others = np.setdiff1d(np.arange(groups.num_groups), hit)
    assert all(np.array_equal(a[others], b[others]) for a, b in zip((pos, neg, u2), clean[:3]))
    assert all(pos[g] + neg[g] == sizes[g] - 1 for g in hit)


def test_gauc_wrapper_validates():
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    groups = _plan([3, 1, 3, 1, 1])
    p, y = torch.rand(5, device=DEV), torch.zeros(5, device=DEV)
    pos, neg = (torch.zeros(2, dtype=torch.int32, device=DEV) for _ in range(2))
    u2, err = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    args = [p, y, groups.order, groups.offsets, groups.small_groups, groups.slab_group, groups.slab_first, pos, neg, u2, err]
    ops.gauc_groups(*args)
    assert neg.tolist() == [3, 2] and pos.tolist() == [0, 0] and u2.tolist() == [0, 0]
    for k, wrong in ((0, p.double()), (1, y[:4]), (2, groups.order.long()), (7, pos.long()), (9, u2[:1]), (5, groups.offsets)):
        with pytest.raises(ValueError):
            ops.gauc_groups(*(args[:k] + [wrong] + args[k + 1:]))
    with pytest.raises(CtrHipError):
        ops.gauc_groups(*([p.cpu()] + args[1:]))


# ---------------------------------------------------------------------------------------------------------------
# 2. ctr_score_counts
# ---------------------------------------------------------------------------------------------------------------
def _score_input(n, with_nan=True):
    gen = np.random.default_rng(n)
    y = (gen.random(n) < 0.3).astype(np.float32)
    p = gen.random(n, dtype=np.float32)
    p[0] = 0.0
    if n > 1:
        p[1], y[1] = 1.0, 0.0                       # a certain miss: the -100 floor
    if n > 200:
        p[n // 2], p[n // 3] = np.nan if with_nan else 0.125, 1.5
        p[7], y[7] = 0.0, 1.0                       # the floor on the other logarithm
        p[11] = 0.5                                 # on the threshold: hard
    return p, y


def _run_score(p, y):
    from deeplearningrecommendationsystem_amd import ops
    n = p.shape[0]
    counts = torch.zeros(8, dtype=torch.int64, device=DEV)
    sums = torch.full((-(-n // sn.CHUNK), 4), -1.0, dtype=torch.float64, device=DEV)
    ops.score_counts(p, y, counts, sums)
    return counts.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("with_nan", [True, False])     # without: the sums of p and (p - y)^2 are finite everywhere
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65_535, 65_536, 65_537, 200_001])
def test_score_counts_equal_the_restatement(n, with_nan):
    p, y = _score_input(n, with_nan)
    dp, dy = _dev(p), _dev(y)
    counts, rows = _run_score(dp, dy)
    want_counts, want_rows = sn.counts(p, y), sn.chunk_sums(p, y)
    assert np.array_equal(counts, want_counts), (counts, want_counts)
    assert counts[0] + counts[1] == n and counts[2:6].sum() == n and counts[6] == ((1 + with_nan) if n > 200 else 0)
    assert rows.shape == want_rows.shape
    # sum p, sum (p - y)^2, sum y: per chunk row, and the totals added in chunk order (a NaN score makes both sides NaN)
    for c in range(rows.shape[0]):
        m = min(n, (c + 1) * sn.CHUNK) - c * sn.CHUNK
        for k in (1, 2, 3):
            got, want = rows[c, k], want_rows[c, k]
            print(f"n={n} chunk {c} sum {k}: {got!r} vs {want!r}")
            assert (math.isnan(got) and math.isnan(want)) or abs(got - want) <= m * 2.0 ** -52 * abs(want)
    for k in (1, 2, 3):
        got, want = float(np.cumsum(rows[:, k])[-1]), float(np.cumsum(want_rows[:, k])[-1])
        assert (math.isnan(got) and math.isnan(want)) or abs(got - want) <= n * 2.0 ** -52 * abs(want)
    assert not math.isnan(float(rows[:, 3].sum())) and float(rows[:, 3].sum()) == float(sn.positive(y).sum())
    got, want = float(np.cumsum(rows[:, 0])[-1]) / n, float(np.cumsum(want_rows[:, 0])[-1]) / n
    print(f"n={n} log-loss {got!r} vs {want!r}")
    assert math.isfinite(want) and abs(got - want) <= 1e-6 + 1e-5 * abs(want)
    # two runs are bit-identical; counts are added to
    counts2, rows2 = _run_score(dp, dy)
    assert np.array_equal(counts2, counts) and rows2.tobytes() == rows.tobytes()
    # a row depends on its chunk's data only
    for c in range(rows.shape[0]):
        lo, hi = c * sn.CHUNK, min(n, (c + 1) * sn.CHUNK)
        _, alone = _run_score(dp[lo:hi], dy[lo:hi])
        assert alone.shape == (1, 4) and alone[0].tobytes() == rows[c].tobytes(), c


def test_score_counts_wrapper_validates_and_adds_to_counts():
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    p, y = torch.rand(300, device=DEV), (torch.rand(300, device=DEV) < 0.5).float()
    counts = torch.full((8,), 5, dtype=torch.int64, device=DEV)
    sums = torch.empty((1, 4), dtype=torch.float64, device=DEV)
    ops.score_counts(p, y, counts, sums)
    assert counts.cpu().numpy().tolist() == (sn.counts(p.cpu().numpy(), y.cpu().numpy()) + 5).tolist()
    for args in ((p.double(), y, counts, sums), (p, y[:299], counts, sums), (p, y, counts[:7], sums),
                 (p, y, counts, sums.float()), (p, y, counts, torch.empty((2, 4), dtype=torch.float64, device=DEV)),
                 (p.view(-1, 1), y, counts, sums)):
        with pytest.raises(ValueError):
            ops.score_counts(*args)
    with pytest.raises(CtrHipError):
        ops.score_counts(p.cpu(), y, counts, sums)
    empty = torch.empty(0, device=DEV)
    ops.score_counts(empty, empty, counts, torch.empty((0, 4), dtype=torch.float64, device=DEV))   # a no-op


# ---------------------------------------------------------------------------------------------------------------
# 3. score_metrics
# ---------------------------------------------------------------------------------------------------------------
def test_score_metrics_agree_with_the_evaluator_and_the_restatement(recipe):
    from deeplearningrecommendationsystem_amd.evaluator import (Evaluator, ScoreMetrics, UserGroups, gauc_from_counts,
                                                                score_metrics, user_auc_counts)
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    users, y = recipe["users"], recipe["y"]
    p = np.nan_to_num(recipe["plain"], nan=0.75)          # the evaluator's numbers need finite scores
    dy, dp, groups = _dev(y).view(-1, 1), _dev(p).view(-1, 1), recipe["groups"]
    got = score_metrics(dy, dp, groups)
    assert isinstance(got, ScoreMetrics) and got.samples == users.shape[0] and got.bad == 0
    assert got.positives == int(sn.positive(y).sum())
    shared = Evaluator.eval(dy, dp)
    for name, want in zip(("accuracy", "precision", "recall", "f1", "balanced_accuracy"), shared):
        assert abs(getattr(got, name) - want) <= 1e-6, name
    assert got.auc == Evaluator.score_auc(dy, dp)
    rows = sn.chunk_sums(p, y)
    n = users.shape[0]
    assert abs(got.logloss - rows[:, 0].sum() / n) <= 1e-6 + 1e-5 * rows[:, 0].sum() / n
    assert abs(got.calibration - rows[:, 1].sum() / rows[:, 3].sum()) <= 1e-12
    assert abs(got.rmse - math.sqrt(rows[:, 2].sum() / n)) <= 1e-12
    pos, neg, u2, _ = sn.group_counts(p, y, recipe["plan"]["order"], recipe["plan"]["offsets"])
    want = sn.gauc(pos, neg, u2)
    assert abs(got.gauc - want[0]) <= 1e-12 and abs(got.user_auc_mean - want[1]) <= 1e-12
    assert (got.users_scored, got.samples_scored) == want[2:] and got.users_scored >= 190
    counts = user_auc_counts(groups, dy.view(-1), dp.view(-1))
    assert all(t.is_cuda for t in counts) and np.array_equal(counts[2].cpu().numpy(), u2)
    assert gauc_from_counts(*counts) == got[-4:]
    text = got.report()
    assert "GAUC" in text and "LogLoss" in text and str(got.gauc) in text
    plain = score_metrics(dy.view(-1), dp.view(-1))                                   # (N,) inputs, no groups
    assert plain[:12] == got[:12] and plain.gauc is None and plain.users_scored is None
    assert "GAUC" not in plain.report()
    with pytest.raises(ValueError):
        score_metrics(dy, dp, UserGroups(_dev(users[:-1])))                           # the plan of another set
    with pytest.raises(ValueError):
        score_metrics(dy, dp[:-1])
    with pytest.raises(ValueError):
        score_metrics(dy.view(1, -1), dp.view(1, -1))
    with pytest.raises(ValueError):
        score_metrics(dy.double(), dp)
    with pytest.raises(CtrHipError):
        score_metrics(dy.cpu(), dp.cpu())


def test_score_metrics_count_bad_predictions_and_a_missing_class():
    from deeplearningrecommendationsystem_amd.evaluator import score_metrics
    p = torch.tensor([0.2, float("nan"), 1.5, -0.5, 0.9], device=DEV)
    got = score_metrics(torch.zeros(5, device=DEV), p, _plan([1, 1, 2, 2, 2]))
    assert got.bad == 3 and got.positives == 0 and math.isnan(got.gauc) and got.users_scored == 0
    assert math.isnan(got.balanced_accuracy) and math.isnan(got.calibration) and got.recall == 0.0


# ---------------------------------------------------------------------------------------------------------------
# 4. DeviceLoader.user_ids and Trainer.score_epoch
# ---------------------------------------------------------------------------------------------------------------
NU, NI = 50, 40


@pytest.fixture(scope="module")
def tiny():
    """50 users x 40 items, 5..20 observed items per user, about half of them rated 1"""
    from deeplearningrecommendationsystem_amd.data import ObservedPairs
    gen = np.random.default_rng(23)
    rows = [sorted(gen.choice(NI, int(gen.integers(5, 21)), replace=False).tolist()) for _ in range(NU)]
    pu = np.repeat(np.arange(NU), [len(r) for r in rows])
    pi = np.array([x for r in rows for x in r], dtype=np.int64)
    mix = gen.permutation(pu.shape[0])                     # the users interleave
    users, items = _dev(pu[mix]), _dev(pi[mix])
    ratings = _dev((gen.random(pu.shape[0]) < 0.5).astype(np.float32))
    return dict(users=users, items=items, ratings=ratings, observed=ObservedPairs(users, items, NU, NI))


def _trainer():
    from deeplearningrecommendationsystem_amd.model import MatrixFactorization
    from deeplearningrecommendationsystem_amd.trainer import Trainer
    torch.manual_seed(0)
    model = MatrixFactorization(NU, NI, 8).to(DEV)
    return Trainer(model, torch.nn.BCELoss(), torch.optim.Adam(model.parameters(), lr=0.01))


@pytest.mark.parametrize("negatives", [0, 2])
def test_score_epoch_is_score_metrics_on_its_predictions(tiny, negatives):
    from deeplearningrecommendationsystem_amd.data import DeviceLoader
    from deeplearningrecommendationsystem_amd.evaluator import UserGroups, score_metrics
    extra = dict(negatives=2, observed=tiny["observed"]) if negatives else {}
    ratings = torch.ones_like(tiny["ratings"]) if negatives else tiny["ratings"]
    loader = DeviceLoader.pairs(tiny["users"], tiny["items"], ratings, 64, seed=5, **extra)
    ids = loader.user_ids()
    assert ids.dtype == torch.int64 and ids.shape == (loader.num_samples,)
    assert torch.equal(ids, tiny["users"].repeat_interleave(1 + negatives))
    seen = torch.cat([args[0].clone() for args, _ in loader.epoch(0, shuffle=False)])
    assert torch.equal(seen, ids)                                                      # the users the batches show
    groups = UserGroups(ids)
    assert groups.num_samples == loader.num_samples and groups.num_groups == NU
    trainer = _trainer()
    trainer.train_epoch(loader, 0)
    got = trainer.score_epoch(loader, groups)
    assert got is trainer.score_metrics and trainer.predictions_score.shape[0] == loader.num_samples
    assert trainer.score_rating.shape[0] == loader.num_samples and trainer.score_loss is not None
    assert got == score_metrics(trainer.score_rating, trainer.predictions_score, groups)
    assert got.samples == loader.num_samples and got.users_scored > NU // 2 and 0.0 <= got.gauc <= 1.0
    y, p = trainer.score_rating.cpu().numpy().reshape(-1), trainer.predictions_score.cpu().numpy().reshape(-1)
    plan = sn.user_groups(ids.cpu().numpy())
    want = sn.gauc(*sn.group_counts(p, y, plan["order"], plan["offsets"])[:3])
    assert abs(got.gauc - want[0]) <= 1e-12 and got.users_scored == want[2]
    without = trainer.score_epoch(loader)
    assert without.gauc is None and without[:12] == got[:12]
    with pytest.raises(ValueError):
        trainer.score_epoch(loader, UserGroups(ids[:-1]))
    split = DeviceLoader.pairs(tiny["users"], tiny["items"], ratings, 64, seed=5, rank=0, world=2, **extra)
    with pytest.raises(ValueError):
        trainer.score_epoch(split, groups)
