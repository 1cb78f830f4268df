"""CPU: which ranks the low-rank grid kernel admits and which Wide & Deep towers its sibling does (functions of shapes
alone), the host-side argument checks of ``ctr_lowrank_grid_scores`` and ``ctr_widedeep_grid_scores``, which run before
anything is enqueued and so need no device, ``grid_path`` of MatrixFactorization, FFM, LogisticRegression and WideDeep
on CPU and meta tensors, and the refusals of their scorers that are decided before a device is touched."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANKS = [0] + list(range(16, 257, 16))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


# ---- admission
def test_rank_zero_and_every_multiple_of_sixteen_up_to_256_is_admitted(lib):
    from deeplearningrecommendationsystem_amd import ops
    assert [k for k in range(-16, 301) if ops.lowrank_grid_supported(k)] == RANKS


@pytest.mark.parametrize("hidden,want", [([512, 256, 128, 1], True), ([64, 256, 128, 1], True), ([1, 256, 128, 1], True),
                                         ([512, 128, 128, 1], False), ([512, 256, 64, 1], False), ([512, 256, 128], False),
                                         ([512, 256, 128, 2], False), ([512, 256, 128, 1, 1], False), ([32, 16, 1], False)])
def test_the_pinned_tower_is_the_one_wide_and_deep_is_admitted_with(lib, hidden, want):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import widedeep
    assert ops.widedeep_grid_supported(hidden) is want
    assert widedeep.grid_path(hidden) == ("grid" if want else "forward")


def test_the_tile_constants_mirror_the_header(lib):
    from deeplearningrecommendationsystem_amd import ops
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define (CTR_[A-Z0-9_]+) (\d+)\b", text, flags=re.M)}
    for name in ("LOWRANK_GRID_ITEM_TILE", "LOWRANK_GRID_USER_TILE", "WIDEDEEP_GRID_ITEM_TILE", "WIDEDEEP_GRID_USER_TILE"):
        assert getattr(ops, name) == getattr(lib, "CTR_" + name) == defines["CTR_" + name], name
    assert ops.LOWRANK_GRID_ITEM_TILE % 32 == 0 and ops.LOWRANK_GRID_USER_TILE == 32      # 32 x 32 matrix-core tiles
    assert (ops.WIDEDEEP_GRID_ITEM_TILE, ops.WIDEDEEP_GRID_USER_TILE) == (ops.DEEPFM_GRID_ITEM_TILE,
                                                                         ops.DEEPFM_GRID_USER_TILE)   # one template


# ---- the C entries: every refusal below is decided on the host, before a launch
OK, EINVAL, ELIMIT, EALIGN = 0, -1, -2, -4


class _Call:
    """arguments of one entry over host buffers (never dereferenced: nothing below reaches a launch)"""

    def __init__(self, lib, entry, names, **scalars):
        self.lib, self.entry = lib, entry
        self.keep = [(ctypes.c_float * 64)() for _ in range(len(names) + 1)]   # 16-byte aligned stand-ins for device memory
        addr = [ctypes.addressof(b) + (-ctypes.addressof(b)) % 16 for b in self.keep]
        pointers = dict(zip(names, addr))
        self.users = addr[-1]
        self.a = {k: pointers.get(k, scalars.get(k)) for k in self.ORDER[entry]}

    ORDER = {
        "ctr_lowrank_grid_scores": ("cu", "ci", "a", "b", "num_users", "num_items", "rank", "users", "user0", "rows", "out",
                                    "ldo", "row_blocks", "stream"),
        "ctr_widedeep_grid_scores": ("zu", "zi", "a", "b", "num_users", "num_items", "n1", "n2", "w2", "b2", "w3", "b3",
                                     "out_w", "out_b", "users", "user0", "rows", "out", "ldo", "row_blocks", "stream"),
    }

    def __call__(self, **changed):
        a = dict(self.a, **changed)
        return getattr(self.lib.load(), self.entry)(*a.values())


def _lowrank(lib, nu=5, ni=7, rows=3, rank=16):
    return _Call(lib, "ctr_lowrank_grid_scores", ("cu", "ci", "a", "b", "out"), num_users=nu, num_items=ni, rank=rank,
                 users=None, user0=0, rows=rows, ldo=ni, row_blocks=0, stream=None)


def _widedeep(lib, nu=5, ni=7, rows=3):
    return _Call(lib, "ctr_widedeep_grid_scores", ("zu", "zi", "a", "b", "w2", "b2", "w3", "b3", "out_w", "out_b", "out"),
                 num_users=nu, num_items=ni, n1=256, n2=128, users=None, user0=0, rows=rows, ldo=ni, row_blocks=0,
                 stream=None)


def test_the_stand_in_calls_are_admitted_up_to_the_launch(lib):
    """the base arguments pass every check: with rows = 0 they return CTR_OK (so a refusal below has one cause)"""
    assert _lowrank(lib)(rows=0) == OK and _widedeep(lib)(rows=0) == OK


def test_null_pointers_are_refused(lib):
    call = _lowrank(lib)
    for name in ("cu", "ci", "out"):
        assert call(**{name: None}) == EINVAL, name
    assert call(cu=None, ci=None) == EINVAL                                    # rank 16 without its tables
    assert call(rank=0, cu=None, ci=None, a=None, b=None) == EINVAL            # rank 0 without a bias
    assert call(rank=8, cu=None) == EINVAL and call(rank=256, ci=None) == EINVAL   # EINVAL comes before ELIMIT
    call = _widedeep(lib)
    for name in ("zu", "zi", "a", "b", "w2", "b2", "w3", "b3", "out_w", "out_b", "out"):
        assert call(**{name: None}) == EINVAL, name


def test_null_biases_are_zeros(lib):
    call = _lowrank(lib)
    for rank in RANKS[1:]:
        assert call(rank=rank, rows=0, a=None) == OK and call(rank=rank, rows=0, b=None) == OK
        assert call(rank=rank, rows=0, a=None, b=None) == OK, rank
    assert call(rank=0, rows=0, cu=None, ci=None, a=None) == OK and call(rank=0, rows=0, cu=None, ci=None, b=None) == OK


@pytest.mark.parametrize("make", [_lowrank, _widedeep], ids=["lowrank", "widedeep"])
def test_bad_counts_are_refused(lib, make):
    call = make(lib)
    assert call(rows=-1) == EINVAL and call(row_blocks=-1) == EINVAL
    assert call(num_users=-1) == EINVAL and call(num_items=-1) == EINVAL
    assert call(ldo=6) == EINVAL and call(ldo=0) == EINVAL            # narrower than a row of scores
    assert call(rows=6) == EINVAL and call(user0=3, rows=3) == EINVAL and call(user0=-1) == EINVAL   # outside the table
    assert call(num_users=0, users=call.users) == EINVAL              # rows of an empty table


def test_shapes_not_admitted_are_refused(lib):
    call = _lowrank(lib)
    for rank in (8, 24, 272, -16, 1, 15, 17, 250, 4096):
        assert call(rank=rank) == ELIMIT, rank
    assert call(num_items=1 << 31, ldo=1 << 31) == ELIMIT and call(num_users=1 << 31) == ELIMIT
    assert call(rank=0, cu=None, ci=None, num_users=1 << 31) == ELIMIT
    call = _widedeep(lib)
    assert call(n1=128) == ELIMIT and call(n1=512) == ELIMIT and call(n2=64) == ELIMIT and call(n2=256) == ELIMIT
    assert call(n1=0) == ELIMIT and call(n2=0) == ELIMIT
    assert call(num_items=1 << 31, ldo=1 << 31) == ELIMIT and call(num_users=1 << 31) == ELIMIT


def test_misaligned_rows_are_refused(lib):
    call = _lowrank(lib)
    for name in ("cu", "ci"):
        assert call(**{name: call.a[name] + 4}) == EALIGN, name
        assert call(**{name: call.a[name] + 4}, rank=24) == ELIMIT, name        # ELIMIT comes before EALIGN
    assert call(a=call.a["a"] + 4, b=call.a["b"] + 4, rows=0) == OK             # the biases are read by the float
    call = _widedeep(lib)
    for name in ("zu", "zi", "w2"):
        assert call(**{name: call.a[name] + 4}) == EALIGN, name
        assert call(**{name: call.a[name] + 4}, n1=128) == ELIMIT, name


def test_an_empty_grid_is_a_no_op(lib):
    call = _lowrank(lib)
    for rank in RANKS:
        tables = {} if rank else dict(cu=None, ci=None)
        assert call(rows=0, rank=rank, **tables) == OK and call(rows=0, out=None, rank=rank, **tables) == OK, rank
        assert call(rows=0, users=call.users, rank=rank, **tables) == OK, rank
        assert call(num_items=0, ldo=0, rank=rank, **tables) == OK, rank
        assert call(num_items=0, ldo=0, out=None, rank=rank, **tables) == OK, rank
    call = _widedeep(lib)
    assert call(rows=0) == OK and call(rows=0, out=None) == OK and call(rows=0, users=call.users) == OK
    assert call(num_items=0, ldo=0) == OK and call(num_items=0, ldo=0, out=None) == OK


# ---- the Python layer: what is decided before a device is needed
def _stub_assembler(nu, ni, device="cpu"):
    return SimpleNamespace(user_features=torch.empty((nu, 24), device=device),
                           item_features=torch.empty((ni, 19), device=device))


def test_grid_path_is_a_function_of_shapes(lib):
    from deeplearningrecommendationsystem_amd.model import ffm, lr, mf, widedeep
    assert [k for k in range(-16, 301) if mf.grid_path(k) == "grid"] == RANKS[1:]
    assert [k for k in range(-16, 301) if ffm.grid_path(k) == "grid"] == RANKS[1:]
    assert mf.grid_path(64) == "grid" and mf.grid_path(20) == "forward" and mf.grid_path(8) == "forward"
    assert ffm.grid_path(32) == "grid" and ffm.grid_path(8) == "forward" and ffm.grid_path(272) == "forward"
    assert lr.grid_path() == "grid"
    assert widedeep.grid_path([512, 256, 128, 1]) == "grid" and widedeep.grid_path([512, 128, 128, 1]) == "forward"


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_cpu_models_and_meta_tensors_will_do(lib, device):
    from deeplearningrecommendationsystem_amd.model import (FFM, LogisticRegression, MatrixFactorization, WideDeep, _base,
                                                            _grid, ffm, lr, mf, widedeep)
    nu, ni = 7, 9
    asm = _stub_assembler(nu, ni, device)
    for k, want in ((8, "forward"), (16, "grid"), (32, "grid"), (64, "grid"), (20, "forward")):
        scorer = FFM(43, k, num_users=nu, num_items=ni).to(device).catalogue_scorer(asm)
        assert scorer.path == want == ffm.grid_path(k) and isinstance(scorer, _base.CatalogueScorer)
        assert (type(scorer) is ffm._GridScorer) == (want == "grid")
        assert (scorer.num_users, scorer.num_items) == (nu, ni)
        model = MatrixFactorization(nu, ni, k).to(device)
        scorer = mf._GridScorer(model)
        assert scorer.path == want == mf.grid_path(k) and isinstance(scorer, _grid.UserGridScorer)
        assert (scorer.num_users, scorer.num_items) == (nu, ni)
    for hidden, dim, want in (([512, 256, 128, 1], 16, "grid"), ([64, 256, 128, 1], 24, "grid"),
                              ([512, 128, 128, 1], 16, "forward"), ([32, 16, 1], 8, "forward")):
        scorer = WideDeep(nu, ni, hidden, dim).to(device).catalogue_scorer(asm)
        assert scorer.path == want == widedeep.grid_path(hidden) and isinstance(scorer, _base.CatalogueScorer)
        assert (type(scorer) is widedeep._GridScorer) == (want == "grid")
    scorer = LogisticRegression(nu, ni, 43).to(device).catalogue_scorer(asm)
    assert scorer.path == "grid" and type(scorer) is lr._GridScorer and isinstance(scorer, _base.CatalogueScorer)


def test_matrix_factorization_has_the_grid_interface(lib):
    from deeplearningrecommendationsystem_amd.model import MatrixFactorization
    nu, ni = 11, 13
    for k in (16, 20):
        model = MatrixFactorization(nu, ni, k)
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
        for shape in ((nu + 1, ni), (nu, ni - 1)):
            with pytest.raises(ValueError, match="exclude"):
                model.recommend(n=3, exclude=SimpleNamespace(num_users=shape[0], num_items=shape[1]))


def test_argument_errors_that_need_no_device(lib):
    from deeplearningrecommendationsystem_amd.model import FFM, LogisticRegression, WideDeep
    nu, ni = 11, 13
    models = [FFM(43, 32, num_users=nu, num_items=ni), FFM(43, 8, num_users=nu, num_items=ni),
              WideDeep(nu, ni, [512, 256, 128, 1], 16), WideDeep(nu, ni, [32, 16, 1], 8), LogisticRegression(nu, ni, 43)]
    for model in models:
        for bad in (_stub_assembler(nu + 1, ni), _stub_assembler(nu, ni - 1)):
            with pytest.raises(ValueError, match="built for"):
                model.catalogue_scorer(bad)
        wrong_width = SimpleNamespace(user_features=torch.empty((nu, 23)), item_features=torch.empty((ni, 19)))
        with pytest.raises(ValueError):
            model.catalogue_scorer(wrong_width)
        scorer = model.catalogue_scorer(_stub_assembler(nu, ni))
        with pytest.raises(ValueError):
            scorer.recommend(n=0)
        for shape in ((nu + 1, ni), (nu, ni - 1)):
            with pytest.raises(ValueError, match="exclude"):
                scorer.recommend(n=3, exclude=SimpleNamespace(num_users=shape[0], num_items=shape[1]))
        for bad in ([nu], [-1], [0, 1, nu + 3]):
            with pytest.raises(IndexError):
                scorer.score_grid(bad)
            with pytest.raises(IndexError):
                scorer.recommend(bad, n=3)
        for s, e in ((-1, 2), (2, nu + 1), (3, 2)):
            with pytest.raises(IndexError):
                scorer.score_rows(s, e)
            with pytest.raises(IndexError):
                scorer(s, e)


def test_a_sharded_ffm_is_refused(lib, monkeypatch):
    """the grid wants the whole id tables on one device: decided on the flag, before the assembler is looked at"""
    from deeplearningrecommendationsystem_amd.model import FFM
    model = FFM(43, 32, num_users=7, num_items=9)
    monkeypatch.setattr(model, "sharded", True)
    with pytest.raises(ValueError, match="sharded"):
        model.catalogue_scorer(_stub_assembler(7, 9))


def test_the_ffm_split_is_the_one_the_pairs_give(lib):
    """six dots on the user's side, one on the item's, and the eight that cross are a full 4 x 2 product"""
    from deeplearningrecommendationsystem_amd.model import ffm
    name = lambda pairs: sorted((ffm.VECTORS[i], ffm.VECTORS[j]) for i, j in pairs)  # noqa: E731
    assert len(ffm._USER_PAIRS) == 6 and name(ffm._ITEM_PAIRS) == [("movie_item", "itemid_item")]
    assert [ffm.VECTORS[i] for i in ffm._CROSS_USER] == ["age_item", "gender_item", "occupation_item", "userid_item"]
    assert [ffm.VECTORS[j] for j in ffm._CROSS_ITEM] == ["movie_user", "itemid_user"]
    assert sorted(ffm._CROSS_PAIRS) == sorted((i, j) for i in ffm._CROSS_USER for j in ffm._CROSS_ITEM)
    assert sorted(ffm._USER_PAIRS + ffm._ITEM_PAIRS + tuple(tuple(sorted(p)) for p in ffm._CROSS_PAIRS)) == sorted(
        tuple(sorted(p)) for p in ffm.PAIRS)


def test_the_ops_wrappers_refuse_what_they_cannot_size(lib):
    from deeplearningrecommendationsystem_amd import ops
    with pytest.raises(ValueError, match="together"):
        ops.lowrank_grid_scores(torch.zeros(3, 16), None, None, None)
    with pytest.raises(ValueError, match="rank 0"):
        ops.lowrank_grid_scores(None, None, torch.zeros(3), None)
