"""GPU: ``ctr_lowrank_grid_scores`` (csrc/lowrank_grid.hip) alone, through ``ops.lowrank_grid_scores``: against float64
numpy, and against its own geometry -- a pair's score may not depend on which rows, which order, which tile, which
``ldo`` or which launch grid it came from.

Parameters.  ``cu`` and ``ci`` are ``randn * sqrt(1.5 / sqrt(K))``, ``a`` and ``b`` ``randn * 0.5``, seeded, on the CPU.
In float64 that gives a score std of about 0.28 and a doubly centred dot at 0.84 - 0.90 of the logit's std at K = 16, 64,
256; every case with at least 64 pairs asserts score std >= 0.15 and, where there is a dot (K > 0), centred dot >= 0.25
of the logit's std, so that neither the product nor the biases can go soft.  An fp32 chain restated in numpy stays at
0.03 / 0.06 / 0.11 of the project tolerance (grid_cases.RTOL / ATOL on the probability) at those ranks.

Shapes (IT = ops.LOWRANK_GRID_ITEM_TILE items a workgroup, UT = ops.LOWRANK_GRID_USER_TILE users a tile; a wave's
matrix-core tile is 32 users x 32 items): one pair, 15 / 16 / 17 and 31 / 32 / 33 items, IT - 1 / IT + 1 (a workgroup's
four tiles), several item workgroups, and one or two users more than one and two user tiles; ``row_blocks`` = 1 and 2 are
the only way the tile loop, its prefetch and its stage swap run at these sizes.

Measured on an MI355X, max error / (atol + rtol |ref|) against float64 (the lines this file prints under ``pytest -s``):
0.17 at K = 256 (at (33, 258)), at most 0.08 at every other rank, 0.01 at K = 0."""
import functools

import numpy as np
import pytest
import torch

from grid_cases import ATOL, DEV, RTOL, error_and_frac as _frac

pytestmark = pytest.mark.gpu
IT, UT = 128, 32             # asserted against ops.LOWRANK_GRID_ITEM_TILE / ops.LOWRANK_GRID_USER_TILE below
SHAPES_16 = [(1, 1), (5, 15), (5, 16), (5, 17), (5, 31), (5, 32), (5, 33), (3, IT - 1), (3, IT + 1), (33, 2 * IT + 2),
             (UT + 2, 37), (UT + 1, 20), (2 * UT + 1, 20)]
SHAPES_K = [(5, 16), (3, IT + 1), (33, 2 * IT + 2), (UT + 2, 37)]
CASES = ([(nu, ni, 16) for nu, ni in SHAPES_16] + [(nu, ni, k) for k in (0, 32, 64, 256) for nu, ni in SHAPES_K]
         + [(5, 17, 48)])
# cases whose default seed (5) misses a condition of _assert_hard: without a dot the logit is a + b alone, whose score
# std is 0.157 in expectation; these three drew 0.145, 0.143 and 0.149
SEEDS = {(5, 16, 0, "ab"): 8, (3, IT + 1, 0, "ab"): 7, (UT + 2, 37, 0, "ab"): 9}


def _ops():
    from deeplearningrecommendationsystem_amd import ops
    return ops


def test_the_tiles_are_the_ones_the_shapes_were_chosen_for():
    assert (_ops().LOWRANK_GRID_ITEM_TILE, _ops().LOWRANK_GRID_USER_TILE) == (IT, UT)


# ------------------------------------------------------------------ the cases: CPU only, float64 reference
def _reference(cu, ci, a, b):
    """float64 (scores, dot, logit) of float32 operands; a / b None: zeros"""
    nu, ni = (cu.shape[0], ci.shape[0]) if cu is not None else (a.shape[0], b.shape[0])
    dot = cu.double().numpy() @ ci.double().numpy().T if cu is not None and cu.shape[1] else np.zeros((nu, ni))
    bias = (a.double().numpy()[:, None] if a is not None else 0.0) + (b.double().numpy()[None, :] if b is not None else 0.0)
    logit = bias + dot
    return 1.0 / (1.0 + np.exp(-logit)), dot, logit


def _assert_hard(scores, dot, logit, rank, what):
    if scores.size < 64:
        return
    centred = dot - dot.mean(0, keepdims=True) - dot.mean(1, keepdims=True) + dot.mean()
    ratio = centred.std() / logit.std()
    print(f"{what}: score std {scores.std():.3f}, centred dot {ratio:.2f} of the logit's std")
    assert scores.std() >= 0.15, f"{what}: soft parameters, the scores' standard deviation is {scores.std():.3f}"
    if rank:
        assert ratio >= 0.25, f"{what}: the centred dot has {ratio:.3f} of the logit's standard deviation"


@functools.lru_cache(maxsize=None)
def _cpu_case(nu, ni, rank, biases="ab"):
    """(cu, ci, a, b on the CPU -- None where absent --, float64 scores), made once and shared: no test changes it"""
    gen = torch.Generator().manual_seed(SEEDS.get((nu, ni, rank, biases), 5) + 31 * nu + ni + rank)
    scale = (1.5 / max(rank, 1) ** 0.5) ** 0.5
    cu = torch.randn((nu, rank), generator=gen) * scale if rank else None
    ci = torch.randn((ni, rank), generator=gen) * scale if rank else None
    a = torch.randn(nu, generator=gen) * 0.5 if "a" in biases else None
    b = torch.randn(ni, generator=gen) * 0.5 if "b" in biases else None
    scores, dot, logit = _reference(cu, ci, a, b)
    _assert_hard(scores, dot, logit, rank, f"({nu}, {ni}) K = {rank} biases '{biases}'")
    return cu, ci, a, b, scores


@functools.lru_cache(maxsize=None)
def _case(nu, ni, rank, biases="ab"):
    """(the four operands on the device, float64 scores)"""
    *operands, scores = _cpu_case(nu, ni, rank, biases)
    return tuple(t.to(DEV) if t is not None else None for t in operands), scores


def _scores(operands, **kw):
    return _ops().lowrank_grid_scores(*operands, **kw)


# ------------------------------------------------------------------ 1. against float64
def _check(nu, ni, rank, biases="ab"):
    operands, scores64 = _case(nu, ni, rank, biases)
    got = _scores(operands)
    assert got.shape == (nu, ni) and got.dtype == torch.float32 and got.is_contiguous()
    err, frac = _frac(got, scores64)
    print(f"({nu}, {ni}) K = {rank} biases '{biases}': max |error| {err:.3e}, max error / (atol + rtol |ref|) {frac:.3f}")
    torch.testing.assert_close(got.cpu().double(), torch.from_numpy(scores64), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("nu,ni,rank", CASES)
def test_the_scores_match_float64(nu, ni, rank):
    assert _ops().lowrank_grid_supported(rank)
    _check(nu, ni, rank)


@pytest.mark.parametrize("biases", ["b", "a", ""], ids=["a-null", "b-null", "both-null"])
def test_a_null_bias_is_zeros(biases):
    _check(UT + 2, 37, 16, biases)


def test_every_admitted_rank_runs():
    """the ranks no other case reaches: one user tile and a partial wave tile each"""
    for rank in range(16, 257, 16):
        _check(5, 17, rank)


# ------------------------------------------------------------------ 2. geometry independence, bitwise
GEOMETRY = [(33, 2 * IT + 2, 16), (UT + 2, 37, 16), (2 * UT + 1, 20, 16), (UT + 2, 37, 0), (UT + 2, 37, 64),
            (UT + 2, 37, 256)]


@pytest.mark.parametrize("nu,ni,rank", GEOMETRY)
def test_a_score_does_not_depend_on_the_rows_asked_for(nu, ni, rank):
    operands, _ = _case(nu, ni, rank)
    full = _scores(operands)
    assert torch.equal(_scores(operands), full)                                # run to run
    users = lambda ids: torch.as_tensor(ids, dtype=torch.int64, device=DEV)   # noqa: E731
    assert torch.equal(_scores(operands, users=users([3, 1, 3, 0])), full[[3, 1, 3, 0]])
    assert torch.equal(_scores(operands, users=torch.arange(nu - 1, -1, -1, device=DEV)), full.flip(0))
    ranges = [(0, nu), (0, 1), (2, 2), (nu - 1, nu), (1, nu - 1), (UT - 1, UT + 1), (UT, nu), (1, UT + 1), (UT - 5, nu)]
    for s, e in ranges:
        rows = _scores(operands, user0=s, rows=e - s)
        assert rows.shape == (e - s, ni) and rows.is_contiguous()
        assert torch.equal(rows, full[s:e]), (s, e)
    assert torch.equal(_scores(operands, user0=3), full[3:])                   # rows None: up to the table's end


@pytest.mark.parametrize("rank", [0, 16, 64])
def test_a_score_does_not_depend_on_the_items_position(rank):
    nu, ni = 33, 2 * IT + 2
    (cu, ci, a, b), _ = _case(nu, ni, rank)
    perm = torch.randperm(ni, generator=torch.Generator().manual_seed(2)).to(DEV)
    moved = (cu, ci[perm] if ci is not None else None, a, b[perm])
    assert torch.equal(_scores(moved), _scores((cu, ci, a, b))[:, perm])


@pytest.mark.parametrize("nu,ni,rank", GEOMETRY)
def test_a_score_does_not_depend_on_the_launch_geometry(nu, ni, rank):
    """row_blocks = 1: one workgroup per item tile walks every user tile (the tile loop, its prefetch and its restaging
    barrier); 2: two workgroups share them; 0: the launch's own choice"""
    operands, _ = _case(nu, ni, rank)
    own = _scores(operands)
    for blocks in (1, 2):
        assert torch.equal(_scores(operands, row_blocks=blocks), own), blocks
        assert torch.equal(_scores(operands, user0=1, rows=nu - 1, row_blocks=blocks), own[1:]), blocks
        assert torch.equal(_scores(operands, users=torch.arange(nu - 1, -1, -1, device=DEV), row_blocks=blocks),
                           own.flip(0)), blocks


@pytest.mark.parametrize("nu,ni,rank", [(5, 17, 48), (UT + 2, 37, 16), (33, 2 * IT + 2, 16), (UT + 2, 37, 0)])
def test_columns_past_the_items_are_left_alone(nu, ni, rank):
    """``out`` a view of a wider buffer: the same bits for another ``ldo``, and nothing written past a row's scores"""
    operands, _ = _case(nu, ni, rank)
    sentinel = -12345.5
    for extra, blocks in ((3, 1), (1, 0), (64, 2)):
        buf = torch.full((nu, ni + extra), sentinel, dtype=torch.float32, device=DEV)
        out = _scores(operands, out=buf[:, :ni], row_blocks=blocks)
        assert out.data_ptr() == buf.data_ptr() and out.stride(0) == ni + extra
        assert torch.equal(buf[:, :ni], _scores(operands))
        assert bool((buf[:, ni:] == sentinel).all())


def test_an_empty_call_returns_an_empty_grid():
    operands, _ = _case(5, 17, 48)
    assert _scores(operands, user0=2, rows=0).shape == (0, 17)
    assert _scores(operands, users=torch.zeros(0, dtype=torch.int64, device=DEV)).shape == (0, 17)


def test_a_rank_the_kernel_is_not_built_for_raises():
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    for rank in (8, 24, 272):
        assert not _ops().lowrank_grid_supported(rank)
        with pytest.raises(CtrHipError):
            _scores((torch.zeros((3, rank), device=DEV), torch.zeros((4, rank), device=DEV), None, None))
