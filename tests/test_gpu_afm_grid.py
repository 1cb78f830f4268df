"""GPU: AFM over the user x item grid -- ``ctr_afm_grid_scores`` (csrc/afm_grid.hip) behind ``AFM.catalogue_scorer``:
against the float64 oracle, against the per-sample forward, and against its own geometry: a pair's score may not depend
on which rows, which order, which tile or which launch grid it came from.

Parameters.  A default-initialised AFM is soft: its tables are ``xavier_normal_``, so the pair products are about 1e-3,
every attention logit is ``h . relu(b_att)`` and the softmax is uniform; a broken kernel would pass.  Every case is built
on the CPU, seeded: the five embedding tables are ``randn * t`` (t = 0.7 at E = 16, 0.5 at E = 48, 0.4 at E = 128),
``attention_W`` is ``randn * 1.0 / 0.8 / 0.6``, ``attention_b`` ``randn * 0.5``, ``attention_h`` ``randn * 0.25``,
``output_layer.weight`` ``randn * 1.5 / 1.2 / 1.0``, and the weights of ``user``, ``item`` and ``linear`` ``randn *
0.3``.  Features: age ``rand``, gender and occupation one-hot, genres Bernoulli(0.09); item 1 has no genre (an all-zero
movie vector).  Every case with at least 64 pairs asserts on its float64 reference that the scores spread (std >=
0.15), that the eight cross products hold between 0.3 and 0.8 of the softmax mass on average, that the largest of the 15
weights averages between 0.2 and 0.7, that the hidden units of the user x item product are positive for 30-70 % of the
(pair, unit) entries, and that the cross part ``sum_c w_c t_c`` -- doubly centred over users and items -- has at least
0.25 of the logit's standard deviation: so that neither the attention map, nor the softmax merge, nor the output dot
can go soft.

Shapes (IT = ops.AFM_GRID_ITEM_TILE items a workgroup, UT = ops.AFM_GRID_USER_TILE users a tile): one pair, 15 / 16 / 17
items (a wave's tile), IT - 1 / IT + 1 (a workgroup's eight tiles), several item workgroups, and one or two users more
than one and two user tiles; ``row_blocks`` = 1 and 2 are the only way the tile loop and its restaging barrier run at
these sizes.

Measured on an MI355X, max error / (atol + rtol |ref|) against float64 over the cases of section 1 (the lines this
file prints under ``pytest -s``): 0.39 at E = 16 (at (3, 127); 0.16 at (33, 258)), 0.37 at E = 128 (at (33, 258)), 0.07
at E = 48; the per-sample forward on the same pairs reaches 0.22 and 0.34 at (33, 258).  The side tables of section 1
stay below 0.03 of ``linear_fwd``'s tolerance.  Large logits ((18, 37), ``attention_h`` times 8, max |s| 123.9): the
grid's worst error is 1.7e-6 (0.37 of the project tolerance), the per-sample forward's 2.2e-6."""
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
from grid_cases import (ATOL, DEV, RTOL, error_and_frac as _frac, features as _features, frame as _frame,
                        observed as _observed, rank64 as _rank64)
from oracle import ctr_oracle as orc

pytestmark = pytest.mark.gpu
IT, UT = 128, 16             # asserted against ops.AFM_GRID_ITEM_TILE / ops.AFM_GRID_USER_TILE below
ATT = 64
SHAPES_16 = [(1, 1), (5, 15), (5, 16), (5, 17), (3, IT - 1), (3, IT + 1), (33, 2 * IT + 2), (UT + 2, 37), (UT + 1, 20),
             (2 * UT + 1, 20)]
SHAPES_128 = [(5, 16), (3, IT + 1), (33, 2 * IT + 2), (UT + 2, 37)]
CASES = [(nu, ni, 16) for nu, ni in SHAPES_16] + [(nu, ni, 128) for nu, ni in SHAPES_128] + [(5, 17, 48)]
TABLE_SCALE = {16: 0.7, 48: 0.5, 128: 0.4}
W_SCALE = {16: 1.0, 48: 0.8, 128: 0.6}
OUT_SCALE = {16: 1.5, 48: 1.2, 128: 1.0}
B_SCALE, H_SCALE, WIDE_SCALE = 0.5, 0.25, 0.3
SEEDS = {}                   # cases whose default seed (5) misses a condition of _assert_hard
TABLES = ("user_embedding", "item_embedding", "gender_embedding", "occupation_embedding", "movie_embedding")
PAIRS = [(i, j) for i in range(6) for j in range(i + 1, 6)]
USER_COLUMNS, ITEM_COLUMNS, CROSS_COLUMNS = (1, 2, 3, 9, 10, 12), (8,), (0, 4, 5, 6, 7, 11, 13, 14)
# linear_fwd's own tolerance (tests/linear_ref.py FWD_TOL: rtol 1e-5, atol 4e-6 at unit scale) as a relative error
SIDE_TOL = 1e-5 + 4e-6


def _afm():
    from deeplearningrecommendationsystem_amd.model import afm
    return afm


def test_the_tiles_are_the_ones_the_shapes_were_chosen_for():
    from deeplearningrecommendationsystem_amd import ops
    assert (ops.AFM_GRID_ITEM_TILE, ops.AFM_GRID_USER_TILE) == (IT, UT)
    afm = _afm()
    assert (tuple(afm._USER_PAIRS), tuple(afm._ITEM_PAIRS), tuple(afm._CROSS_PAIRS)) == (USER_COLUMNS, ITEM_COLUMNS,
                                                                                       CROSS_COLUMNS)


# ------------------------------------------------------------------ the cases: CPU only, float64 reference
def _parts64(p64, x64):
    """float64 pieces of the model over the frame: z (B, 15, 64) hidden pre-activations, s (B, 15) logits, w (B, 15)
    softmax weights, t (B, 15) output dots, wide (B,) the linear part, logit (B,)"""
    e = p64["user_embedding.weight"].shape[1]
    f = [p64["user_embedding.weight"][orc.ids_from_float(x64[:, orc.COL_USER])],
         p64["item_embedding.weight"][orc.ids_from_float(x64[:, orc.COL_ITEM])],
         x64[:, orc.COL_AGE].unsqueeze(1).expand(-1, e),
         orc.bag_pool(x64[:, orc.SL_GENDER], p64["gender_embedding.weight"]),
         orc.bag_pool(x64[:, orc.SL_OCC], p64["occupation_embedding.weight"]),
         orc.bag_pool(x64[:, orc.SL_GENRE], p64["movie_embedding.weight"])]
    pairs = torch.stack([f[i] * f[j] for i, j in PAIRS], dim=1)
    z = pairs @ p64["attention_W"] + p64["attention_b"]
    s = (torch.relu(z) @ p64["attention_h"]).squeeze(2)
    w = torch.softmax(s, dim=1)
    t = pairs @ p64["output_layer.weight"][0]
    uid, iid = orc.ids_from_float(x64[:, orc.COL_USER]), orc.ids_from_float(x64[:, orc.COL_ITEM])
    wide_u = p64["user.weight"][uid, 0] + x64[:, 2:26] @ p64["linear.weight"][0, :24]
    wide_i = (p64["item.weight"][iid, 0] + x64[:, 26:] @ p64["linear.weight"][0, 24:] + p64["linear.bias"][0]
              + p64["output_layer.bias"][0])
    logit = wide_u + wide_i + (w * t).sum(1)
    return dict(z=z, s=s, w=w, t=t, wide_u=wide_u, wide_i=wide_i, logit=logit)


def _build(nu, ni, dim, seed, h_times=1.0):
    """(AFM on the CPU with the parameters of the module docstring, user features, item features)"""
    torch.manual_seed(seed)
    model = _afm().AFM(nu, ni, dim, ATT)
    gen = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        def fill(t, scale):
            t.copy_(torch.randn(t.shape, generator=gen) * scale)
        for name in TABLES:
            fill(getattr(model, name).weight, TABLE_SCALE[dim])
        fill(model.attention_W, W_SCALE[dim])
        fill(model.attention_b, B_SCALE)
        fill(model.attention_h, H_SCALE * h_times)
        fill(model.output_layer.weight, OUT_SCALE[dim])
        for lin in (model.user, model.item, model.linear):
            fill(lin.weight, WIDE_SCALE)
        uf, itf = _features(nu, ni, gen)
    return model, uf, itf


def _p64(model):
    return {k: v.detach().double() for k, v in model.state_dict().items()}


def _reference(model, uf, itf):
    """float64 (scores (nu, ni), the pieces of ``_parts64``)"""
    nu, ni = uf.shape[0], itf.shape[0]
    p64, x64 = _p64(model), _frame(uf, itf).double()
    with torch.no_grad():
        scores = orc.afm_forward(p64, x64).view(nu, ni)
        parts = _parts64(p64, x64)
        assert torch.allclose(torch.sigmoid(parts["logit"]).view(nu, ni), scores, rtol=0, atol=1e-13)
    return scores.numpy(), parts


def _assert_hard(scores, parts, what):
    """the conditions of the module docstring: the case exercises the attention map, the softmax merge and the dots"""
    if scores.size < 64:
        return
    nu, ni = scores.shape
    w, t, z = parts["w"], parts["t"], parts["z"]
    cols = list(CROSS_COLUMNS)
    mass, top = float(w[:, cols].sum(1).mean()), float(w.max(1).values.mean())
    live = float((z[:, 0, :] > 0).double().mean())
    cross = (w[:, cols] * t[:, cols]).sum(1).view(nu, ni)
    cross = cross - cross.mean(0, keepdim=True) - cross.mean(1, keepdim=True) + cross.mean()
    ratio = float(cross.std()) / float(parts["logit"].std())
    print(f"{what}: std {scores.std():.3f}, cross mass {mass:.2f}, top weight {top:.2f}, live {live:.2f}, cross part "
          f"{ratio:.2f}, max |s| {float(parts['s'].abs().max()):.1f}")
    assert scores.std() >= 0.15, f"{what}: soft parameters, the scores' standard deviation is {scores.std():.3f}"
    assert 0.3 <= mass <= 0.8, f"{what}: the cross products hold {mass:.2f} of the softmax mass"
    assert 0.2 <= top <= 0.7, f"{what}: the largest weight averages {top:.2f}"
    assert 0.3 <= live <= 0.7, f"{what}: hidden units of user x item are positive for {live:.2f} of the entries"
    assert ratio >= 0.25, f"{what}: the centred cross part has {ratio:.3f} of the logit's standard deviation"


@functools.lru_cache(maxsize=None)
def _cpu_case(nu, ni, dim=16):
    """(model on the CPU, user features, item features, float64 scores, float64 parts), made once and shared: no test
    changes it"""
    model, uf, itf = _build(nu, ni, dim, SEEDS.get((nu, ni, dim), 5) + 31 * nu + ni + dim)
    scores, parts = _reference(model, uf, itf)
    _assert_hard(scores, parts, f"({nu}, {ni}) E = {dim}")
    return model, uf, itf, scores, parts


def _on_device(cpu, nu, ni, dim):
    model = _afm().AFM(nu, ni, dim, ATT)
    model.load_state_dict(cpu.state_dict())
    return model.to(DEV).eval()


def _scorer(model, uf, itf):
    from deeplearningrecommendationsystem_amd.data import FeatureAssembler
    return model.catalogue_scorer(FeatureAssembler(uf.to(DEV), itf.to(DEV)))


@functools.lru_cache(maxsize=None)
def _case(nu, ni, dim=16):
    """(model on the device, scorer, float64 scores)"""
    cpu, uf, itf, scores, _ = _cpu_case(nu, ni, dim)
    model = _on_device(cpu, nu, ni, dim)
    return model, _scorer(model, uf, itf), scores


def _forward_pairs(model, scorer, nu, ni):
    users = torch.arange(nu, device=DEV).repeat_interleave(ni)
    items = torch.arange(ni, device=DEV).repeat(nu)
    with torch.no_grad():
        return model(scorer.assembler.feature(users, items)).view(nu, ni)


# ------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("nu,ni,dim", CASES)
def test_score_grid_matches_the_float64_oracle(nu, ni, dim):
    model, scorer, scores64 = _case(nu, ni, dim)
    assert scorer.path == "grid" and type(scorer) is _afm()._GridScorer
    got = scorer.score_grid()
    assert got.shape == (nu, ni) and got.dtype == torch.float32 and got.is_contiguous()
    err, frac = _frac(got, scores64)
    print(f"({nu}, {ni}) E = {dim}: max |error| {err:.3e}, max error / (atol + rtol |ref|) {frac:.3f}")
    torch.testing.assert_close(got.cpu().double(), torch.from_numpy(scores64), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("nu,ni,dim", [(33, 2 * IT + 2, 16), (UT + 2, 37, 128)])
def test_the_side_tables_match_their_float64_values(nu, ni, dim):
    """locates a failure of the final comparison: a, b, the user's softmax summary and the item's (s, t), each table's
    worst error relative to its largest entry, within linear_fwd's own tolerance"""
    model, scorer, _ = _case(nu, ni, dim)
    parts = _cpu_case(nu, ni, dim)[4]
    with torch.no_grad():
        p, (su, fu), (si, fi) = scorer._shared()
    assert su.shape == (nu, 4) and si.shape == (ni, 3) and fu.shape == (nu, 4 * dim) and fi.shape == (ni, 2 * dim)
    view = lambda v: v.view(nu, ni, *v.shape[1:])  # noqa: E731
    s, t = view(parts["s"]), view(parts["t"])
    s_u, t_u = s[:, 0, list(USER_COLUMNS)], t[:, 0, list(USER_COLUMNS)]
    m_u = s_u.max(1).values
    e_u = torch.exp(s_u - m_u[:, None])
    want = {"a": view(parts["wide_u"])[:, 0], "mU": m_u, "dU": e_u.sum(1), "nU": (e_u * t_u).sum(1),
            "b": view(parts["wide_i"])[0], "sI": s[0, :, ITEM_COLUMNS[0]], "tI": t[0, :, ITEM_COLUMNS[0]]}
    got = {"a": su[:, 0], "mU": su[:, 1], "dU": su[:, 2], "nU": su[:, 3], "b": si[:, 0], "sI": si[:, 1], "tI": si[:, 2]}
    for name, ref in want.items():
        err = float((got[name].cpu().double() - ref).abs().max()) / float(ref.abs().max())
        print(f"({nu}, {ni}) E = {dim}: {name} relative error {err:.3e} ({err / SIDE_TOL:.3f} of linear_fwd's tolerance)")
        assert err <= SIDE_TOL, name


# ------------------------------------------------------------------ 2. geometry independence, bitwise
@pytest.mark.parametrize("nu,ni,dim", [(33, 2 * IT + 2, 16), (UT + 2, 37, 16), (2 * UT + 1, 20, 16), (UT + 2, 37, 128)])
def test_a_score_does_not_depend_on_the_rows_asked_for(nu, ni, dim):
    model, scorer, _ = _case(nu, ni, dim)
    full = scorer.score_grid()
    assert torch.equal(scorer.score_grid(), full)                             # run to run
    assert torch.equal(scorer.score_grid([3, 1, 3, 0]), full[[3, 1, 3, 0]])
    assert torch.equal(scorer.score_grid(torch.arange(nu - 1, -1, -1)), full.flip(0))
    ranges = [(0, nu), (0, 1), (2, 2), (nu - 1, nu), (1, nu - 1), (UT - 1, UT + 1), (UT, nu), (1, UT + 1), (UT - 5, nu)]
    for s, e in ranges:
        rows = scorer.score_rows(s, e)
        assert rows.shape == (e - s, ni) and rows.is_contiguous()
        assert torch.equal(rows, full[s:e]), (s, e)
        assert torch.equal(scorer(s, e), rows)


def test_a_score_does_not_depend_on_the_items_position():
    from deeplearningrecommendationsystem_amd.data import FeatureAssembler
    nu, ni = 33, 2 * IT + 2
    model_a, scorer_a, _ = _case(nu, ni)
    perm = torch.randperm(ni, generator=torch.Generator().manual_seed(2)).to(DEV)
    model_b = _on_device(_cpu_case(nu, ni)[0], nu, ni, 16)
    with torch.no_grad():
        model_b.item_embedding.weight.copy_(model_a.item_embedding.weight[perm])
        model_b.item.weight.copy_(model_a.item.weight[perm])
    asm = scorer_a.assembler
    scorer_b = model_b.catalogue_scorer(FeatureAssembler(asm.user_features, asm.item_features[perm]))
    assert torch.equal(scorer_b.score_grid(), scorer_a.score_grid()[:, perm])


@pytest.mark.parametrize("nu,ni,dim", [(2 * UT + 1, 20, 16), (UT + 2, 37, 16), (UT + 2, 37, 128)])
def test_a_score_does_not_depend_on_the_launch_geometry(nu, ni, dim):
    """row_blocks = 1: one workgroup per item tile walks every user tile (the tile loop and its restaging barrier);
    2: two workgroups share them; 0: the launch's own choice"""
    model, scorer, _ = _case(nu, ni, dim)
    own = scorer.score_grid()
    users = torch.arange(nu - 1, -1, -1)
    try:
        for blocks in (1, 2):
            scorer.row_blocks = blocks
            assert torch.equal(scorer.score_grid(), own), blocks
            assert torch.equal(scorer.score_rows(1, nu), own[1:]), blocks
            assert torch.equal(scorer.score_grid(users), own.flip(0)), blocks
    finally:
        scorer.__dict__.pop("row_blocks", None)


@pytest.mark.parametrize("nu,ni", [(5, 17), (UT + 2, 37)])
def test_columns_past_the_items_are_left_alone(nu, ni):
    from deeplearningrecommendationsystem_amd import ops
    model, scorer, _ = _case(nu, ni)
    with torch.no_grad():
        p, (su, fu), (si, fi) = scorer._shared()
        sentinel = -12345.5
        buf = torch.full((nu, ni + 3), sentinel, dtype=torch.float32, device=DEV)
        out = ops.afm_grid_scores(su, si, fu, fi, p.att_w, p.att_b, p.att_h, p.out_w, out=buf[:, :ni], row_blocks=1)
    assert out.data_ptr() == buf.data_ptr() and out.stride(0) == ni + 3
    assert torch.equal(buf[:, :ni], scorer.score_grid())
    assert bool((buf[:, ni:] == sentinel).all())


# ------------------------------------------------------------------ 3. against the per-sample forward
@pytest.mark.parametrize("nu,ni,dim", [(33, 2 * IT + 2, 16), (UT + 2, 37, 16), (5, 17, 16), (33, 2 * IT + 2, 128)])
def test_score_grid_matches_the_per_sample_forward(nu, ni, dim):
    model, scorer, scores64 = _case(nu, ni, dim)
    want = _forward_pairs(model, scorer, nu, ni)
    got = scorer.score_grid()
    print(f"({nu}, {ni}) E = {dim}: {int((got != want).sum())} of {got.numel()} scores differ bitwise, max |difference| "
          f"{float((got - want).abs().max()):.3e}; against float64: grid {_frac(got, scores64)[1]:.3f}, forward "
          f"{_frac(want, scores64)[1]:.3f} of the tolerance")
    torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ 4. large logits
def test_large_logits_do_not_overflow():
    """``attention_h`` times 8: logits beyond 90, where exp(s) without the running maximum overflows float32.  The
    project tolerance was not derived for logits of this size, so the bound is the larger of it and twice the
    per-sample forward's own worst error against float64 on these pairs (one more rounding in the merge)"""
    nu, ni, dim = UT + 2, 37, 16
    cpu, uf, itf = _build(nu, ni, dim, 5 + 31 * nu + ni + dim, h_times=8.0)
    scores64, parts = _reference(cpu, uf, itf)
    assert float(parts["s"].abs().max()) > 90.0
    model = _on_device(cpu, nu, ni, dim)
    scorer = _scorer(model, uf, itf)
    got = scorer.score_grid()
    assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    forward_err = _frac(_forward_pairs(model, scorer, nu, ni), scores64)[0]
    err = np.abs(got.cpu().numpy().astype(np.float64) - scores64)
    allowed = np.maximum(ATOL + RTOL * np.abs(scores64), 2.0 * forward_err)
    print(f"({nu}, {ni}) E = {dim}, max |s| {float(parts['s'].abs().max()):.1f}: grid max |error| {err.max():.3e} "
          f"({_frac(got, scores64)[1]:.3f} of the project tolerance), forward max |error| {forward_err:.3e}")
    assert (err <= allowed).all()


# ------------------------------------------------------------------ 5. recommend
def _own_ranking(scorer, users, n, observed):
    """topk_rows of the scorer's own scores after rank_mask, -1 where the survivors run out"""
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.topn import excluded_rows
    ni = scorer.num_items
    scores = scorer.score_grid(users)
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
    nu, ni = 33, 2 * IT + 2
    model, scorer, scores64 = _case(nu, ni)
    observed, seen = _observed(nu, ni) if excluded else (None, np.zeros((nu, ni), dtype=bool))
    want64 = _rank64(scores64, ~seen)
    left = (~seen).sum(axis=1)
    for n in (1, 5, ni, ni + 3):
        got = scorer.recommend(n=n, exclude=observed)
        assert got.shape == (nu, n) and got.dtype == torch.int64
        assert torch.equal(got, _own_ranking(scorer, torch.arange(nu, device=DEV), n, observed)), n
        got = got.cpu().numpy()
        for u in range(nu):                     # every user: the columns the row fills, then nothing but -1
            m = min(n, int(left[u]))
            assert (got[u, m:] == -1).all() and (got[u, :m] >= 0).all(), (n, u)
            assert not seen[u, got[u, :m]].any(), f"n = {n}, user {u}: an excluded item is recommended"
            gu.assert_same_ranking(got[u:u + 1, :m], want64[u:u + 1, :m], scores64[u:u + 1], tol=1e-5)
        if excluded:
            assert (got[0] == -1).all() and set(got[1, :min(n, 2)]) <= {2, ni - 1}


def test_recommend_for_a_user_list_in_chunks(monkeypatch):
    nu, ni = 2 * UT + 1, 20
    model, scorer, scores64 = _case(nu, ni)
    observed, seen = _observed(nu, ni, seed=9)
    users = torch.tensor([nu - 1, 0, 7, 7, UT, 1, UT - 1] + list(range(3, nu)))
    whole = scorer.recommend(users, n=6, exclude=observed)
    assert torch.equal(whole, scorer.recommend(n=6, exclude=observed)[users.to(DEV)])
    from deeplearningrecommendationsystem_amd import topn
    monkeypatch.setattr(topn, "SCORE_CHUNK_FLOATS", 5 * ni)                  # five users at a time
    assert torch.equal(scorer.recommend(users, n=6, exclude=observed), whole)
    assert torch.equal(scorer.recommend(users.tolist(), n=6, exclude=None), scorer.recommend(users, n=6))


# ------------------------------------------------------------------ 6. ranking_metrics, and nothing is left behind
def test_ranking_metrics_over_the_scorer_and_the_model_is_untouched():
    from deeplearningrecommendationsystem_amd.evaluator import ranking
    nu, ni = 33, 2 * IT + 2
    model, scorer, _ = _case(nu, ni)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    training = model.training
    gen = torch.Generator().manual_seed(11)
    kind = torch.rand((nu, ni), generator=gen)
    train = tuple(t.to(DEV) for t in (kind < 0.3).nonzero(as_tuple=True))
    held = kind > 0.9
    held[torch.arange(nu), kind.argmax(dim=1)] = True                             # no empty actual row
    real = tuple(t.to(DEV) for t in held.nonzero(as_tuple=True))
    grid = scorer.score_grid()
    keep = grid.clone()
    a = ranking.ranking_metrics(scorer, real, 10, exclude=(train,), num_users=nu, chunk=7)
    b = ranking.ranking_metrics(grid, real, 10, exclude=(train,), num_users=nu, chunk=7)
    assert np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True), (a, b)
    assert 0.0 < a.precision <= 1.0
    assert torch.equal(grid, keep)
    observed, _ = _observed(nu, ni)
    scorer.recommend(n=5, exclude=observed)
    scorer.score_rows(3, 9)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed"
    assert model.training == training
    assert all(p.grad is None for p in model.parameters())


# ------------------------------------------------------------------ 7. a scorer is never stale
def test_a_scorer_is_never_stale():
    """the weights are read at every call: a scorer made before a parameter changed scores the new parameters"""
    nu, ni = 5, 17
    cpu, uf, itf = _cpu_case(nu, ni)[:3]
    model = _on_device(cpu, nu, ni, 16)
    scorer = _scorer(model, uf, itf)
    last = scorer.score_grid()
    changes = (lambda: model.movie_embedding.weight[3].add_(0.5), lambda: model.attention_W[:, 5].add_(0.25),
               lambda: model.attention_h[7:40].add_(0.25), lambda: model.output_layer.bias.add_(0.25))
    for change in changes:
        with torch.no_grad():
            change()
        new = scorer.score_grid()
        assert not torch.equal(new, last)
        assert torch.equal(new, model.catalogue_scorer(scorer.assembler).score_grid())
        torch.testing.assert_close(new, _forward_pairs(model, scorer, nu, ni), rtol=RTOL, atol=ATOL)
        last = new


# ------------------------------------------------------------------ 8. errors
def test_errors():
    from deeplearningrecommendationsystem_amd.data import FeatureAssembler, ObservedPairs
    nu, ni = 5, 17
    model, scorer, _ = _case(nu, ni)
    assert scorer.path == "grid"
    for bad in ([nu], [-1], [0, 1, nu + 3]):
        with pytest.raises(IndexError):
            scorer.score_grid(bad)
        with pytest.raises(IndexError):
            scorer.recommend(bad, n=3)
    for s, e in ((-1, 2), (2, nu + 1), (3, 2)):
        with pytest.raises(IndexError):
            scorer.score_rows(s, e)
    with pytest.raises(ValueError):
        scorer.recommend(n=0)
    pairs = torch.zeros(1, dtype=torch.int64, device=DEV)
    for shape in ((nu + 1, ni), (nu, ni - 1)):
        with pytest.raises(ValueError):
            scorer.recommend(n=3, exclude=ObservedPairs(pairs, pairs, *shape))
    asm = scorer.assembler
    for users, items in ((asm.user_features[:-1], asm.item_features), (asm.user_features, asm.item_features[1:])):
        with pytest.raises(ValueError):
            model.catalogue_scorer(FeatureAssembler(users, items))
    assert scorer.score_grid([]).shape == (0, ni) and scorer.recommend([], n=3).shape == (0, 3)
    assert scorer.score_rows(2, 2).shape == (0, ni)
