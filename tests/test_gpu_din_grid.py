"""GPU: DIN over the history x item grid -- ``ctr_din_grid_pool`` (csrc/din_grid.hip) behind ``score_histories``,
``history_scorer`` and ``recommend`` -- against the float64 oracle, against the per-sample forward, and against its own
geometry: a pair's pooled row may not depend on which rows, which order or which tile it was computed in.

Parameters.  A freshly initialised DIN scores every pair within 0.005 of the others and attends uniformly: a kernel that
ignored the softmax would pass.  So the table is ``randn``, every ``Linear`` weight of ``attention`` and ``fc`` is its
default init times 3 and every bias is ``rand - 0.5`` (seeded); every case with more than one pair asserts, on the
float64 reference alone, that its scores spread (standard deviation >= 0.2) and, for L >= 4, that the attention is
peaked (mean over pairs of the largest weight >= 2 / L).

Shapes: the smallest at which the tiling can go wrong -- one pair, 15 / 16 / 17 items (a wave's tile), 63 / 65 (a
workgroup's four tiles), several item workgroups (130); L = 1, 2, 10, 33 and 100 (the kernel stages blocks of 32
history positions, csrc/din_grid.hip kPB); R = 1, 3, 5, 33 (its row tile is 4 rows, kRT).  In every case with two rows
or more the first history is one repeated id and the last one has id 0 inside it.

Error against float64 as a fraction of the tolerance, worst over the shapes below (every case prints its own): pooled
rows 0.15, scores on the grid path 0.22, scores of the per-sample forward on the same explicit pairs 0.19 (DESIGN.md
section 4j)."""
import functools
import os

import numpy as np
import pytest
import torch

import golden_util as gu
from grid_cases import (ATOL, DEV, RTOL, forward_pairs as _forward_pairs, frac_of_bound as _frac,
                        histories as _histories, observed as _observed, rank64 as _rank64)
from oracle import ctr_oracle as orc

pytestmark = pytest.mark.gpu
E = 64
POSITION_BLOCK, ROW_TILE = 32, 4
SHAPES = [(1, 1, 1), (3, 15, 2), (3, 16, 10), (3, 17, 2), (1, 17, 33), (5, 63, 10), (ROW_TILE + 1, 65, 10), (33, 130, 33),
          (2, 20, 3 * POSITION_BLOCK + 4), (3, 130, 1)]
POOL_ATOL = 1e-5             # pooled rows: the same rtol


def _grid():
    from deeplearningrecommendationsystem_amd.model import _grid
    return _grid


def _din():
    from deeplearningrecommendationsystem_amd.model import din
    return din


def _build(ni, embed, seed):
    """a DIN on the CPU with the parameters of the module docstring"""
    torch.manual_seed(seed)
    model = _din().DIN(ni, embed)
    gen = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        model.item_embedding.weight.copy_(torch.randn(model.item_embedding.weight.shape, generator=gen))
        for seq in (model.attention, model.fc):
            for lin in seq:
                if isinstance(lin, torch.nn.Linear):
                    lin.weight.mul_(3.0)
                    lin.bias.copy_(torch.rand(lin.bias.shape, generator=gen) - 0.5)
    return model


def _reference(rows, ni, length, embed, seed):
    """(model on the CPU, hist, float64 scores (R, I), float64 pooled (R, I, E), float64 ranking, the scores' standard
    deviation, the mean over pairs of the largest attention weight)"""
    model = _build(ni, embed, seed)
    hist = _histories(rows, ni, length, seed + 1)
    p64 = {k: v.detach().double() for k, v in model.state_dict().items()}
    topk, scores = orc.recommend_hist("din", p64, rows, ni, hist.tolist(), min(ni, 20))
    h, _, a = orc.din_attention(p64, "", hist.repeat_interleave(ni, 0), torch.arange(ni).repeat(rows))
    pooled = (h * a.unsqueeze(-1)).sum(dim=1).view(rows, ni, embed)
    scores = scores.numpy()
    return model, hist, scores, pooled.numpy(), topk.numpy(), float(scores.std()), float(a.max(dim=1).values.mean())


@functools.lru_cache(maxsize=None)
def _case(rows, ni, length, embed=E, seed=7):
    """(model on the device, hist on the device, float64 scores, float64 pooled, float64 ranking), made once and shared:
    no test changes it.  The spread of the scores depends on the draw (a single history row saturates easily), so the
    seed is the first of ``seed, seed + 1, ...`` whose FLOAT64 REFERENCE meets the bounds of the module docstring --
    nothing the code under test computes takes part in the choice -- and the bounds are asserted on what was chosen."""
    single = rows * ni == 1
    for s in range(seed, seed + 32):
        model, hist, scores, pooled, topk, std, peak = _reference(rows, ni, length, embed, s)
        if single or (std >= 0.2 and (length < 4 or peak >= 2.0 / length)):
            break
    if not single:
        assert std >= 0.2, f"soft parameters: the scores' standard deviation is {std:.3f}"
        assert length < 4 or peak >= 2.0 / length, f"soft parameters: mean largest attention weight {peak:.3f}, L = {length}"
    return model.to(DEV).eval(), hist.to(DEV), scores, pooled, topk


def _operands(model, hist, by_position=False):
    """the arguments of ``ops.din_grid_pool`` for the model and history rows"""
    from deeplearningrecommendationsystem_amd import ops
    sc = _din()._HistoryScorer(model)
    assert sc.path == "grid"
    if by_position:
        ah = ops.linear_fwd(sc.table[hist.reshape(-1)].contiguous(), sc.wf[0], None)
    else:
        ah = ops.linear_fwd(sc.table, sc.wf[0], None)
    return sc, (sc.table, sc.at, ah, sc.w2, sc.b2, sc.w3)


# ------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("rows,ni,length", SHAPES)
def test_pooled_rows_and_scores_match_the_float64_oracle(rows, ni, length):
    from deeplearningrecommendationsystem_amd import ops
    model, hist, scores64, pooled64, _ = _case(rows, ni, length)
    assert _din().grid_path(E) == "grid"
    for by_position in (False, True):
        _, args = _operands(model, hist, by_position)
        pooled = ops.din_grid_pool(*args, hist, ah_by_position=by_position)
        assert pooled.shape == (rows * ni, E) and pooled.dtype == torch.float32 and pooled.is_contiguous()
        got = pooled.view(rows, ni, E).cpu().numpy()
        print(f"({rows}, {ni}, {length}) pooled, AH by {'position' if by_position else 'id'}: "
              f"max error / (atol + rtol |ref|) {_frac(got, pooled64, POOL_ATOL):.3f}")
        torch.testing.assert_close(torch.from_numpy(got).double(), torch.from_numpy(pooled64), rtol=RTOL, atol=POOL_ATOL)
    got = model.score_histories(hist)
    assert got.shape == (rows, ni) and got.dtype == torch.float32 and got.is_contiguous()
    assert got.data_ptr() != model.score_histories(hist).data_ptr() or rows * ni == 0        # fresh
    fwd = _forward_pairs(model, hist, ni)
    print(f"({rows}, {ni}, {length}) scores: grid max error / (atol + rtol |ref|) {_frac(got.cpu(), scores64, ATOL):.3f}, "
          f"per-sample forward {_frac(fwd.cpu(), scores64, ATOL):.3f}")
    torch.testing.assert_close(got.cpu().double(), torch.from_numpy(scores64), rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ 2. geometry independence, bitwise
@pytest.mark.parametrize("rows,ni,length", [(33, 130, 33), (ROW_TILE + 1, 65, 10)])
def test_a_pooled_row_does_not_depend_on_the_rows_asked_for(rows, ni, length):
    from deeplearningrecommendationsystem_amd import ops
    model, hist, _, _, _ = _case(rows, ni, length)
    _, args = _operands(model, hist)
    full = ops.din_grid_pool(*args, hist).view(rows, ni, E)
    assert torch.equal(ops.din_grid_pool(*args, hist).view(rows, ni, E), full)               # run to run
    picks = [[3, 1, 3, 0], list(range(rows - 1, -1, -1)), [rows - 1], [2, 2, 2, 2, 2, 2], list(range(1, rows))]
    for pick in picks:
        sub = ops.din_grid_pool(*args, hist[pick].contiguous()).view(len(pick), ni, E)
        assert torch.equal(sub, full[pick]), pick


def test_a_pooled_row_does_not_depend_on_the_items_position():
    from deeplearningrecommendationsystem_amd import ops
    rows, ni, length = 33, 130, 33
    model, hist, _, _, _ = _case(rows, ni, length)
    _, (table, at, ah, w2, b2, w3) = _operands(model, hist)
    full = ops.din_grid_pool(table, at, ah, w2, b2, w3, hist).view(rows, ni, E)
    perm = torch.randperm(ni, generator=torch.Generator().manual_seed(2)).to(DEV)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(ni, device=DEV)                    # the new id of every old item
    moved = ops.din_grid_pool(table[perm].contiguous(), at[perm].contiguous(), ah[perm].contiguous(), w2, b2, w3,
                              inv[hist]).view(rows, ni, E)
    assert torch.equal(moved, full[:, perm])


@pytest.mark.parametrize("rows,ni,length", [(3, 17, 2), (ROW_TILE + 1, 65, 10)])
def test_columns_and_rows_past_the_pooled_block_are_left_alone(rows, ni, length):
    from deeplearningrecommendationsystem_amd import ops
    model, hist, _, _, _ = _case(rows, ni, length)
    _, args = _operands(model, hist)
    sentinel = -12345.5
    buf = torch.full((rows * ni + 2, 2 * E), sentinel, dtype=torch.float32, device=DEV)
    out = ops.din_grid_pool(*args, hist, out=buf[:rows * ni, :E])
    assert out.data_ptr() == buf.data_ptr() and out.stride(0) == 2 * E
    assert torch.equal(buf[:rows * ni, :E], ops.din_grid_pool(*args, hist))
    assert bool((buf[:, E:] == sentinel).all()) and bool((buf[rows * ni:] == sentinel).all())
    narrow = torch.full((rows * ni + 2, E + 4), sentinel, dtype=torch.float32, device=DEV)
    ops.din_grid_pool(*args, hist, out=narrow[:rows * ni, :E])
    assert torch.equal(narrow[:rows * ni, :E], buf[:rows * ni, :E])
    assert bool((narrow[:, E:] == sentinel).all()) and bool((narrow[rows * ni:] == sentinel).all())


# ------------------------------------------------------------------ 3. against the per-sample forward, and chunking
@pytest.mark.parametrize("rows,ni,length", [(33, 130, 33), (ROW_TILE + 1, 65, 10), (3, 17, 2)])
def test_score_histories_matches_the_per_sample_forward_in_any_chunking(rows, ni, length, monkeypatch):
    model, hist, _, _, _ = _case(rows, ni, length)
    want = _forward_pairs(model, hist, ni)
    got = model.score_histories(hist)
    print(f"({rows}, {ni}, {length}): {int((got != want).sum())} of {got.numel()} scores differ from the per-sample "
          f"forward, max |difference| {float((got - want).abs().max()):.3e}")
    torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL)
    for pairs in (ni, 2 * ni + 1):                 # one row per chunk; two rows: a chunk boundary inside the row list
        monkeypatch.setattr(_grid(), "PAIR_CHUNK", pairs)
        torch.testing.assert_close(model.score_histories(hist), got, rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ 4. recommend
def _own_ranking(model, hist, users, n, observed):
    """topk_rows of the model's own scores after rank_mask, -1 where the survivors run out"""
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.topn import excluded_rows
    ni = model.item_embedding.weight.shape[0]
    scores = model.score_histories(hist)
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
def test_recommend_is_the_ranking_of_its_own_scores(excluded):
    rows, ni, length = 33, 130, 33
    model, hist, scores64, _, _ = _case(rows, ni, length)
    observed, seen = _observed(rows, ni) if excluded else (None, np.zeros((rows, ni), dtype=bool))
    want64 = _rank64(scores64, ~seen)
    left = (~seen).sum(axis=1)
    for n in (1, 5, ni, ni + 3):
        got = model.recommend(hist, n=n, exclude=observed)
        assert got.shape == (rows, n) and got.dtype == torch.int64
        assert torch.equal(got, _own_ranking(model, hist, torch.arange(rows, device=DEV), n, observed)), n
        got = got.cpu().numpy()
        for u in range(rows):                     # every row: the columns it fills, then nothing but -1
            m = min(n, int(left[u]))
            assert (got[u, m:] == -1).all() and (got[u, :m] >= 0).all(), (n, u)
            assert not seen[u, got[u, :m]].any(), f"n = {n}, row {u}: an excluded item is recommended"
            gu.assert_same_ranking(got[u:u + 1, :m], want64[u:u + 1, :m], scores64[u:u + 1], tol=1e-5)
        if excluded:
            assert (got[0] == -1).all() and set(got[1, :min(n, 2)]) <= {2, ni - 1}


def test_recommend_for_shuffled_users_with_repeats_in_chunks(monkeypatch):
    rows, ni, length = 33, 130, 33
    model, hist, _, _, _ = _case(rows, ni, length)
    observed, _ = _observed(rows, ni, seed=9)
    users = torch.tensor([32, 0, 7, 7, 31, 1, 16] + list(range(10, 20)), device=DEV)
    per_user = model.recommend(hist, n=6, exclude=observed)
    whole = model.recommend(hist[users], n=6, exclude=observed, users=users)
    assert torch.equal(whole, per_user[users])
    from deeplearningrecommendationsystem_amd import topn
    monkeypatch.setattr(topn, "SCORE_CHUNK_FLOATS", 5 * ni)                  # five rows at a time
    assert torch.equal(model.recommend(hist[users], n=6, exclude=observed, users=users), whole)
    assert torch.equal(model.recommend(hist[users], n=6, users=users.tolist()), model.recommend(hist, n=6)[users])


# ------------------------------------------------------------------ 5. the fallback path
def test_other_embed_sizes_take_the_forward_path(monkeypatch):
    rows, ni, length = 9, 60, 5
    model, hist, scores64, _, topk64 = _case(rows, ni, length, embed=8)
    assert _din().grid_path(8) == "forward" and _din()._HistoryScorer(model).path == "forward"
    got = model.score_histories(hist)
    assert got.shape == (rows, ni) and got.is_contiguous()
    print(f"forward path: max error / (atol + rtol |ref|) {_frac(got.cpu(), scores64, ATOL):.3f}")
    torch.testing.assert_close(got.cpu().double(), torch.from_numpy(scores64), rtol=RTOL, atol=ATOL)
    gu.assert_same_ranking(model.recommend(hist, n=20).cpu().numpy(), topk64, scores64, tol=1e-5)
    monkeypatch.setattr(_grid(), "PAIR_CHUNK", 100)                          # chunks that end inside a row
    torch.testing.assert_close(model.score_histories(hist), got, rtol=RTOL, atol=ATOL)
    observed, _ = _observed(rows, ni)
    rec = model.recommend(hist, n=ni + 3, exclude=observed)
    assert torch.equal(rec, _own_ranking(model, hist, torch.arange(rows, device=DEV), ni + 3, observed))
    assert (rec[0] == -1).all()


def test_the_forward_path_reproduces_the_reference_fixture():
    g = gu.load_rec("rec_din")
    model = _din().DIN(*g["meta"]["args"])
    model.load_state_dict(g["params"], strict=True)
    model = model.to(DEV).eval()
    assert _din()._HistoryScorer(model).path == "forward"
    ni, k = g["num_items"], g["k"]
    by_len = {}
    for u, h in enumerate(g["hist_list"]):
        by_len.setdefault(len(h), []).append(u)
    assert len(by_len) > 1                                                   # ragged: several length groups
    for length, users in by_len.items():
        hist = torch.tensor([g["hist_list"][u] for u in users], dtype=torch.int64, device=DEV)
        got = model.score_histories(hist)
        assert got.shape == (len(users), ni)
        torch.testing.assert_close(got.cpu(), torch.from_numpy(g["scores"][users]).float(), rtol=RTOL, atol=ATOL)
        gu.assert_same_ranking(model.recommend(hist, n=k).cpu().numpy(), g["topk"][users], g["scores"][users], tol=1e-5)


# ------------------------------------------------------------------ 6. ranking_metrics, and nothing is left behind
def test_ranking_metrics_over_the_history_scorer_and_the_model_is_untouched():
    from deeplearningrecommendationsystem_amd.evaluator import ranking
    nu, ni, length = 33, 130, 33
    model, history, _, _, _ = _case(nu, ni, length)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    training = model.training
    gen = torch.Generator().manual_seed(11)
    kind = torch.rand((nu, ni), generator=gen)
    train = tuple(t.to(DEV) for t in (kind < 0.3).nonzero(as_tuple=True))
    held = kind > 0.9
    held[torch.arange(nu), kind.argmax(dim=1)] = True                             # no empty actual row
    real = tuple(t.to(DEV) for t in held.nonzero(as_tuple=True))
    grid = model.score_histories(history)
    keep = grid.clone()
    a = ranking.ranking_metrics(model.history_scorer(history), real, 10, exclude=(train,), num_users=nu, chunk=7)
    b = ranking.ranking_metrics(grid, real, 10, exclude=(train,), num_users=nu, chunk=7)
    assert np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True), (a, b)
    assert 0.0 < a.precision <= 1.0
    assert torch.equal(grid, keep)
    observed, _ = _observed(nu, ni)
    model.recommend(history, n=5, exclude=observed)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed"
    assert model.training == training
    assert all(p.grad is None for p in model.parameters())


# ------------------------------------------------------------------ 7. errors
@pytest.mark.parametrize("embed", [E, 8], ids=["grid", "forward"])
def test_errors(embed):
    from deeplearningrecommendationsystem_amd.data import ObservedPairs
    rows, ni, length = (3, 17, 2) if embed == E else (9, 60, 5)
    model, hist, _, _, _ = _case(rows, ni, length, embed=embed)
    for bad_id in (ni, -1, ni + 1000):
        bad = hist.clone()
        bad[rows - 1, length - 1] = bad_id
        with pytest.raises(IndexError):
            model.score_histories(bad)
        with pytest.raises(IndexError):
            model.recommend(bad, n=3)
    model.score_histories(hist)                                              # the flag does not outlive its error
    for bad in (hist.cpu(), hist[0], hist.int(), hist[:, :0]):
        with pytest.raises(ValueError):
            model.score_histories(bad)
        with pytest.raises(ValueError):
            model.recommend(bad, n=3)
    with pytest.raises(ValueError):
        model.recommend(hist, n=0)
    pairs = torch.zeros(1, dtype=torch.int64, device=DEV)
    for shape in ((rows + 1, ni), (rows, ni - 1)):
        with pytest.raises(ValueError):
            model.recommend(hist, n=3, exclude=ObservedPairs(pairs, pairs, *shape))
    observed = ObservedPairs(pairs, pairs, rows + 1, ni)
    for users in ([0] * (rows + 1), [0] * (rows - 1), [0] * (rows - 1) + [rows + 1], [-1] + [0] * (rows - 1)):
        with pytest.raises(ValueError):
            model.recommend(hist, n=3, exclude=observed, users=users)
    assert model.recommend(hist, n=3, exclude=observed, users=[rows] * rows).shape == (rows, 3)
    assert model.score_histories(hist[:0]).shape == (0, ni) and model.recommend(hist[:0], n=3).shape == (0, 3)
    scorer = model.history_scorer(hist)
    assert scorer(1, 1).shape == (0, ni)
    with pytest.raises(IndexError):
        scorer(0, rows + 1)


def test_sharded_models_are_refused():
    model, hist, _, _, _ = _case(3, 17, 2)
    model.sharded = True
    try:
        for call in (model.score_histories, model.history_scorer, model.recommend):
            with pytest.raises(ValueError, match="sharded"):
                call(hist)
    finally:
        model.sharded = False


# ------------------------------------------------------------------ 8. the script
def test_din_topk_script_runs(capsys, monkeypatch):
    import runpy
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.setattr(sys, "argv", ["din_topk.py", "--epochs", "2"])
    monkeypatch.syspath_prepend(os.path.join(root, "scripts"))
    runpy.run_path(os.path.join(root, "scripts", "din_topk.py"), run_name="__main__")
    out = capsys.readouterr().out
    assert "epoch 2:" in out and "Precision@50" in out and "Mean NDCG@50" in out and "MRR" in out
    assert "user 2:" in out
