"""GPU: NeuralCF over the user x item grid -- ``ctr_ncf_grid_scores`` (csrc/ncf_grid.hip) behind ``score_rows``,
``score_grid`` and ``recommend`` -- against the float64 oracle, against the per-sample forward, and against its own
geometry: a pair's score may not depend on which rows, which order or which tile it was computed in.

Parameters.  A freshly initialised NeuralCF scores every pair within 0.01 of 0.5, where the tolerance below is a
hundred times looser than any honest error and a third of the adjacent scores tie.  So the four tables are
``randn * 2``, every bias is ``rand - 0.5`` (seeded), the weights keep their default init; every test that has more
than one pair asserts that its float64 scores spread (standard deviation >= 0.2), so that it cannot go soft.

Shapes: the smallest at which the tiling can go wrong -- one pair, 15 / 16 / 17 items (a wave's tile), 63 / 65 (a
workgroup's four tiles), several item workgroups (130), and 129 / 130 users: one more than the kernel's user tile
(kUT = 128, csrc/ncf_grid.hip)."""
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
from grid_cases import ATOL, DEV, RTOL, observed as _observed, rank64 as _rank64
from oracle import ctr_oracle as orc

pytestmark = pytest.mark.gpu
PINNED = (64, [128, 64, 32, 16, 8])
USER_TILE = 128
SHAPES = [(1, 1), (5, 15), (5, 16), (5, 17), (3, 63), (3, 65), (33, 130), (130, 37), (USER_TILE + 1, 20)]


def _neuralcf():
    from deeplearningrecommendationsystem_amd.model import neuralcf
    return neuralcf


def _build(nu, ni, mf_dim, layers, seed):
    """a NeuralCF on the CPU with the parameters of the module docstring"""
    torch.manual_seed(seed)
    model = _neuralcf().NeuralCF(nu, ni, mf_dim, layers)
    gen = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for emb in (model.GMF_Embedding_User, model.GMF_Embedding_Item, model.MLP_Embedding_User, model.MLP_Embedding_Item):
            emb.weight.copy_(torch.randn(emb.weight.shape, generator=gen) * 2.0)
        for lin in list(model.dnn_network) + [model.linear, model.linear2]:
            lin.bias.copy_(torch.rand(lin.bias.shape, generator=gen) - 0.5)
    return model


def _scores64(model, nu, ni):
    """(ranking, scores) of the float64 oracle over the whole grid, as numpy"""
    p64 = {k: v.detach().double() for k, v in model.state_dict().items()}
    topk, scores = orc.recommend_ids("neuralcf", p64, nu, ni)
    return topk.numpy(), scores.numpy()


@functools.lru_cache(maxsize=None)
def _case(nu, ni, mf_dim=PINNED[0], layers=tuple(PINNED[1]), seed=5):
    """(model on the device, float64 scores, float64 ranking), made once and shared: no test changes it"""
    model = _build(nu, ni, mf_dim, list(layers), seed + 31 * nu + ni)
    topk, scores = _scores64(model, nu, ni)
    if scores.size > 1:
        assert scores.std() >= 0.2, f"soft parameters: the scores' standard deviation is {scores.std():.3f}"
    return model.to(DEV).eval(), scores, topk


def _path(model):
    p = model._params()
    return _neuralcf().grid_path(p.tables, p.hidden, p.proj)


# ------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("nu,ni", SHAPES)
def test_score_grid_matches_the_float64_oracle(nu, ni):
    model, scores64, _ = _case(nu, ni)
    assert _path(model) == "grid"
    got = model.score_grid()
    assert got.shape == (nu, ni) and got.dtype == torch.float32 and got.is_contiguous()
    err = np.abs(got.cpu().numpy().astype(np.float64) - scores64)
    print(f"({nu}, {ni}): max |error| {err.max():.3e}, max error / (atol + rtol |ref|) "
          f"{(err / (ATOL + RTOL * np.abs(scores64))).max():.3f}")
    torch.testing.assert_close(got.cpu().double(), torch.from_numpy(scores64), rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ 2. geometry independence, bitwise
@pytest.mark.parametrize("nu,ni", [(33, 130), (130, 37)])
def test_a_score_does_not_depend_on_the_rows_asked_for(nu, ni):
    model, _, _ = _case(nu, ni)
    full = model.score_grid()
    assert torch.equal(model.score_grid(), full)                             # run to run
    assert torch.equal(model.score_grid([3, 1, 3, 0]), full[[3, 1, 3, 0]])
    assert torch.equal(model.score_grid(torch.arange(nu - 1, -1, -1)), full.flip(0))
    ranges = [(0, nu), (0, 1), (2, 2), (nu - 1, nu), (5, 20)]
    if nu > USER_TILE:
        ranges += [(USER_TILE - 1, USER_TILE + 1), (USER_TILE, nu), (1, USER_TILE + 1), (USER_TILE - 8, nu)]
    for s, e in ranges:
        rows = model.score_rows(s, e)
        assert rows.shape == (e - s, ni) and rows.is_contiguous()
        assert torch.equal(rows, full[s:e]), (s, e)


def test_a_score_does_not_depend_on_the_items_position():
    nu, ni = 33, 130
    model_a, _, _ = _case(nu, ni)
    perm = torch.randperm(ni, generator=torch.Generator().manual_seed(2))
    model_b = _build(nu, ni, *PINNED, seed=0)
    model_b.load_state_dict(model_a.state_dict())
    model_b = model_b.to(DEV).eval()
    with torch.no_grad():
        for name in ("GMF_Embedding_Item", "MLP_Embedding_Item"):
            getattr(model_b, name).weight.copy_(getattr(model_a, name).weight[perm.to(DEV)])
    assert torch.equal(model_b.score_grid(), model_a.score_grid()[:, perm.to(DEV)])


@pytest.mark.parametrize("nu,ni", [(5, 17), (130, 37)])
def test_columns_past_the_items_are_left_alone(nu, ni):
    from deeplearningrecommendationsystem_amd import ops
    model, _, _ = _case(nu, ni)
    sc = _neuralcf()._GridScorer(model)._shared()
    sentinel = -12345.5
    buf = torch.full((nu, ni + 3), sentinel, dtype=torch.float32, device=DEV)
    out = ops.ncf_grid_scores(sc.p_u, sc.p_i, sc.tables[0], sc.tables[1], sc.layers, sc.wfold, sc.cfold, out=buf[:, :ni])
    assert out.data_ptr() == buf.data_ptr() and out.stride(0) == ni + 3
    assert torch.equal(buf[:, :ni], model.score_grid())
    assert bool((buf[:, ni:] == sentinel).all())


# ------------------------------------------------------------------ 3. against the per-sample forward
@pytest.mark.parametrize("nu,ni", [(33, 130), (130, 37), (5, 17)])
def test_score_grid_matches_the_per_sample_forward(nu, ni):
    neuralcf = _neuralcf()
    model, _, _ = _case(nu, ni)
    users = torch.arange(nu, device=DEV).repeat_interleave(ni)
    items = torch.arange(ni, device=DEV).repeat(nu)
    p = model._params()
    path = neuralcf.choose_path(p.tables, p.hidden, p.proj, users.numel(), True)
    with torch.no_grad():
        want = model(users, items).view(nu, ni)
    got = model.score_grid()
    print(f"({nu}, {ni}): forward path {path}, bitwise equal: {bool(torch.equal(got, want))}, "
          f"{int((got != want).sum())} of {got.numel()} scores differ, max |difference| {float((got - want).abs().max()):.3e}")
    torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ 4. recommend
def _own_ranking(model, users, n, observed):
    """topk_rows of the kernel's own scores after rank_mask, -1 where the survivors run out"""
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.topn import excluded_rows
    ni = model.GMF_Embedding_Item.weight.shape[0]
    scores = model.score_grid(users)
    left = torch.full((scores.shape[0],), ni, dtype=torch.int64, device=DEV)
    if observed is not None:
        off, ids = excluded_rows(observed, users)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.rank_mask(scores, off, ids, err)
        assert int(err.item()) == 0
        left -= off.diff()
    take = min(n, ni)
    want = torch.full((scores.shape[0], n), -1, dtype=torch.int64, device=DEV)
    want[:, :take] = ops.topk_rows(scores, take)
    want[torch.arange(n, device=DEV)[None, :] >= left[:, None]] = -1
    return want


@pytest.mark.parametrize("excluded", [False, True], ids=["all-items", "observed-left-out"])
def test_recommend_is_the_ranking_of_the_kernels_scores(excluded):
    nu, ni = 33, 130
    model, scores64, _ = _case(nu, ni)
    observed, seen = _observed(nu, ni) if excluded else (None, np.zeros((nu, ni), dtype=bool))
    want64 = _rank64(scores64, ~seen)
    left = (~seen).sum(axis=1)
    for n in (1, 5, ni, ni + 3):
        got = model.recommend(n=n, exclude=observed)
        assert got.shape == (nu, n) and got.dtype == torch.int64
        assert torch.equal(got, _own_ranking(model, torch.arange(nu, device=DEV), n, observed)), n
        got = got.cpu().numpy()
        for u in range(nu):                     # every user: the columns the row fills, then nothing but -1
            m = min(n, int(left[u]))
            assert (got[u, m:] == -1).all() and (got[u, :m] >= 0).all(), (n, u)
            assert not seen[u, got[u, :m]].any(), f"n = {n}, user {u}: an excluded item is recommended"
            gu.assert_same_ranking(got[u:u + 1, :m], want64[u:u + 1, :m], scores64[u:u + 1], tol=1e-5)
        if excluded:
            assert (got[0] == -1).all() and set(got[1, :min(n, 2)]) <= {2, ni - 1}


def test_recommend_for_a_user_list_in_chunks(monkeypatch):
    nu, ni = 130, 37
    model, scores64, _ = _case(nu, ni)
    observed, seen = _observed(nu, ni, seed=9)
    users = torch.tensor([129, 0, 7, 7, 128, 1, 64] + list(range(100, 120)))
    whole = model.recommend(users, n=6, exclude=observed)
    assert torch.equal(whole, model.recommend(n=6, exclude=observed)[users.to(DEV)])
    from deeplearningrecommendationsystem_amd import topn
    monkeypatch.setattr(topn, "SCORE_CHUNK_FLOATS", 5 * ni)                  # five users at a time
    assert torch.equal(model.recommend(users, n=6, exclude=observed), whole)
    assert torch.equal(model.recommend(users.tolist(), n=6, exclude=None), model.recommend(users, n=6))


def test_recommend_deeper_than_the_topk_kernel():
    from deeplearningrecommendationsystem_amd import ops
    nu, ni = 2, ops.TOPK_MAX_K + 5
    model, scores64, _ = _case(nu, ni)
    got = model.recommend(n=ni + 2).cpu().numpy()
    assert (got[:, ni:] == -1).all()
    gu.assert_same_ranking(got[:, :ni], _rank64(scores64), scores64, tol=1e-5)


# ------------------------------------------------------------------ 5. the fallback path
def test_other_shapes_take_the_forward_path(monkeypatch):
    nu, ni = 50, 60
    model, scores64, topk64 = _case(nu, ni, 12, (24, 12, 6))
    assert _path(model) == "forward"
    got = model.score_grid()
    torch.testing.assert_close(got.cpu().double(), torch.from_numpy(scores64), rtol=RTOL, atol=ATOL)
    gu.assert_same_ranking(model.recommend(n=20).cpu().numpy(), topk64[:, :20], scores64, tol=1e-5)
    monkeypatch.setattr(_neuralcf(), "_FORWARD_CHUNK", 1000)                 # chunks that end inside a row
    assert torch.equal(model.score_grid(), got)
    assert torch.equal(model.score_rows(7, 31), got[7:31])
    assert torch.equal(model.score_grid([3, 1, 3, 0]), got[[3, 1, 3, 0]])
    observed, seen = _observed(nu, ni)
    rec = model.recommend(n=ni + 3, exclude=observed)
    assert torch.equal(rec, _own_ranking(model, torch.arange(nu, device=DEV), ni + 3, observed))
    assert (rec[0] == -1).all()


def test_the_forward_path_reproduces_the_reference_fixture():
    g = gu.load_rec("rec_neuralcf")
    model = _neuralcf().NeuralCF(*g["meta"]["args"])
    model.load_state_dict(g["params"], strict=True)
    model = model.to(DEV).eval()
    assert _path(model) == "forward"
    nu, ni = g["num_users"], g["num_items"]
    got = model.score_grid()
    assert got.shape == (nu, ni)
    torch.testing.assert_close(got.cpu(), torch.from_numpy(g["scores"]).float(), rtol=RTOL, atol=ATOL)
    gu.assert_same_ranking(model.recommend(n=20).cpu().numpy(), g["topk"], g["scores"], tol=1e-5)


# ------------------------------------------------------------------ 6. ranking_metrics, and nothing is left behind
def test_ranking_metrics_over_score_rows_and_the_model_is_untouched():
    from deeplearningrecommendationsystem_amd.evaluator import ranking
    nu, ni = 33, 130
    model, _, _ = _case(nu, ni)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    training = model.training
    gen = torch.Generator().manual_seed(11)
    kind = torch.rand((nu, ni), generator=gen)
    train = tuple(t.to(DEV) for t in (kind < 0.3).nonzero(as_tuple=True))
    held = kind > 0.9
    held[torch.arange(nu), kind.argmax(dim=1)] = True                             # no empty actual row
    real = tuple(t.to(DEV) for t in held.nonzero(as_tuple=True))
    grid = model.score_grid()
    keep = grid.clone()
    a = ranking.ranking_metrics(model.score_rows, real, 10, exclude=(train,), num_users=nu, chunk=7)
    b = ranking.ranking_metrics(grid, real, 10, exclude=(train,), num_users=nu, chunk=7)
    assert np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True), (a, b)
    assert 0.0 < a.precision <= 1.0
    assert torch.equal(grid, keep)
    observed, _ = _observed(nu, ni)
    model.recommend(n=5, exclude=observed)
    model.score_rows(3, 9)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed"
    assert model.training == training
    assert all(p.grad is None for p in model.parameters())


# ------------------------------------------------------------------ 7. errors
def test_errors():
    from deeplearningrecommendationsystem_amd.data import ObservedPairs
    nu, ni = 5, 17
    model, _, _ = _case(nu, ni)
    for bad in ([nu], [-1], [0, 1, nu + 3]):
        with pytest.raises(IndexError):
            model.score_grid(bad)
        with pytest.raises(IndexError):
            model.recommend(bad, n=3)
    for s, e in ((-1, 2), (2, nu + 1), (3, 2)):
        with pytest.raises(IndexError):
            model.score_rows(s, e)
    with pytest.raises(ValueError):
        model.recommend(n=0)
    pairs = torch.zeros(1, dtype=torch.int64, device=DEV)
    for shape in ((nu + 1, ni), (nu, ni - 1)):
        with pytest.raises(ValueError):
            model.recommend(n=3, exclude=ObservedPairs(pairs, pairs, *shape))
    assert model.score_grid([]).shape == (0, ni) and model.recommend([], n=3).shape == (0, 3)
    assert model.score_rows(2, 2).shape == (0, ni)
