"""CPU: which PNN shapes the user x item grid kernel admits (a function of shapes alone), the host-side argument
checks of ``ctr_pnn_grid_scores``, which run before anything is enqueued and so need no device, and the argument
errors of ``catalogue_scorer`` and its scorer that are decided before a device is touched."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOWER = [256, 128, 64, 32]
ADMITTED = list(range(16, 257, 16))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


# ---- admission
@pytest.mark.parametrize("embed", [16, 256])
def test_the_pinned_tower_is_admitted_at_both_embedding_sizes(lib, embed):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import pnn
    assert ops.pnn_grid_supported(TOWER, embed) and ops.pnn_grid_supported(tuple(TOWER), embed, "in")
    assert pnn.grid_path(TOWER, embed) == "grid" and pnn.grid_path(TOWER, embed, "in") == "grid"


def test_every_multiple_of_sixteen_up_to_256_is_admitted(lib):
    from deeplearningrecommendationsystem_amd import ops
    assert [e for e in range(1, 301) if ops.pnn_grid_supported(TOWER, e)] == ADMITTED


@pytest.mark.parametrize("hidden", [[256, 128, 64], [128, 128, 64, 32], [256, 128, 64, 32, 16], [32, 16, 8]])
@pytest.mark.parametrize("embed", [16, 256])
def test_other_towers_take_the_forward_path(lib, hidden, embed):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import pnn
    assert not ops.pnn_grid_supported(hidden, embed)
    assert pnn.grid_path(hidden, embed) == "forward"


@pytest.mark.parametrize("embed", [16, 256])
def test_the_outer_mode_takes_the_forward_path(lib, embed):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import pnn
    assert not ops.pnn_grid_supported(TOWER, embed, "out")
    assert pnn.grid_path(TOWER, embed, model="out") == "forward"


def test_the_pair_columns_are_the_ones_of_allpairs(lib):
    from deeplearningrecommendationsystem_amd.model import _base, pnn
    assert (_base._USER_FIELDS, _base._ITEM_FIELDS) == ((0, 2, 3, 4), (1, 5))
    assert pnn._USER_PAIRS == [1, 2, 3, 9, 10, 12] and pnn._ITEM_PAIRS == [8]
    assert pnn._CROSS_PAIRS == [0, 4, 5, 6, 7, 11, 13, 14]
    pairs = [(i, j) for i in range(6) for j in range(i + 1, 6)]
    assert [pairs[c] for c in pnn._CROSS_PAIRS] == [(0, 1), (0, 5), (1, 2), (1, 3), (1, 4), (2, 5), (3, 5), (4, 5)]


def _stub_assembler(nu, ni, device="cpu"):
    return SimpleNamespace(user_features=torch.empty((nu, 24), device=device),
                           item_features=torch.empty((ni, 19), device=device))


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_cpu_models_and_meta_tensors_will_do(lib, device):
    from deeplearningrecommendationsystem_amd.model import PNN, _base, pnn
    for hidden, embed, mode, want in ((TOWER, 16, "in", "grid"), (TOWER, 256, "in", "grid"), (TOWER, 16, "out", "forward"),
                                      ([32, 16, 8], 8, "in", "forward"), (TOWER, 8, "in", "forward")):
        model = PNN(embed, hidden, mode, num_users=7, num_items=9).to(device)
        scorer = model.catalogue_scorer(_stub_assembler(7, 9, device))
        assert scorer.path == want and isinstance(scorer, _base.CatalogueScorer)
        assert (type(scorer) is pnn._GridScorer) == (want == "grid")
        assert (type(scorer) is _base.CatalogueScorer) == (want == "forward")
        assert (scorer.num_users, scorer.num_items) == (7, 9)
        if want == "grid":
            assert scorer.row_blocks == 0


def test_the_tile_constants_mirror_the_header(lib):
    from deeplearningrecommendationsystem_amd import ops
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define (CTR_[A-Z0-9_]+) (\d+)\b", text, flags=re.M)}
    assert ops.PNN_GRID_ITEM_TILE == lib.CTR_PNN_GRID_ITEM_TILE == defines["CTR_PNN_GRID_ITEM_TILE"]
    assert ops.PNN_GRID_USER_TILE == lib.CTR_PNN_GRID_USER_TILE == defines["CTR_PNN_GRID_USER_TILE"]
    assert ops.PNN_GRID_ITEM_TILE % 16 == 0 and ops.PNN_GRID_USER_TILE >= 1
    assert re.search(r"\bint\s+ctr_pnn_grid_scores\s*\(", text) and "ctr_pnn_grid_scores" in lib.SIGNATURES


# ---- the C entry: every refusal below is decided on the host, before a launch
POINTERS = ("zu", "zi", "fu", "fi", "g", "d2_w", "d2_b", "d3_w", "d3_b", "out_w", "out_b")


class _Call:
    """arguments of ctr_pnn_grid_scores over host buffers (never dereferenced: nothing below reaches a launch)"""

    def __init__(self, lib, nu=5, ni=7, rows=3):
        self.lib = lib
        self.keep = [(ctypes.c_float * 64)() for _ in range(len(POINTERS) + 2)]   # 16-byte aligned stand-ins for device memory
        addr = [ctypes.addressof(b) + (-ctypes.addressof(b)) % 16 for b in self.keep]
        at = dict(zip(POINTERS, addr))
        self.a = dict(zu=at["zu"], zi=at["zi"], fu=at["fu"], fi=at["fi"], g=at["g"], num_users=nu, num_items=ni,
                      embed=16, n1=128, n2=64, n3=32, d2_w=at["d2_w"], d2_b=at["d2_b"], d3_w=at["d3_w"],
                      d3_b=at["d3_b"], out_w=at["out_w"], out_b=at["out_b"], users=None, user0=0, rows=rows,
                      out=addr[-1], ldo=ni, row_blocks=0, stream=None)
        self.users = addr[-2]

    def __call__(self, **changed):
        a = dict(self.a, **changed)
        return self.lib.load().ctr_pnn_grid_scores(*a.values())


OK, EINVAL, ELIMIT, EALIGN = 0, -1, -2, -4


def test_null_pointers_are_refused(lib):
    call = _Call(lib)
    for name in POINTERS + ("out",):
        assert call(**{name: None}) == EINVAL, name


def test_bad_counts_are_refused(lib):
    call = _Call(lib)
    assert call(rows=-1) == EINVAL and call(row_blocks=-1) == EINVAL
    assert call(num_users=-1) == EINVAL and call(num_items=-1) == EINVAL
    assert call(ldo=6) == EINVAL and call(ldo=0) == EINVAL            # narrower than a row of scores
    assert call(rows=6) == EINVAL and call(user0=3, rows=3) == EINVAL and call(user0=-1) == EINVAL   # outside the table
    assert call(user0=6, rows=0) == EINVAL
    assert call(num_users=0, users=call.users) == EINVAL              # rows of an empty table


def test_shapes_not_admitted_are_refused(lib):
    call = _Call(lib)
    for embed in (0, 8, 24, 100, 250, 272, 512, -16):
        assert call(embed=embed) == ELIMIT, embed
    assert call(n1=256) == ELIMIT and call(n1=64) == ELIMIT
    assert call(n2=128) == ELIMIT and call(n2=32) == ELIMIT
    assert call(n3=64) == ELIMIT and call(n3=16) == ELIMIT and call(n3=1) == ELIMIT
    assert call(num_items=1 << 31, ldo=1 << 31) == ELIMIT
    assert call(num_users=1 << 31) == ELIMIT


def test_misaligned_rows_are_refused(lib):
    call = _Call(lib)
    for name in ("zu", "zi", "fu", "fi", "d2_w", "d3_w"):
        assert call(**{name: call.a[name] + 4}) == EALIGN, name


def test_a_refusal_for_the_arguments_comes_before_one_for_the_shape(lib):
    """CTR_EINVAL, then CTR_ELIMIT, then CTR_EALIGN, as ctr_deepfm_grid_scores orders them"""
    call = _Call(lib)
    assert call(zu=None, embed=8) == EINVAL
    assert call(embed=8, zi=call.a["zi"] + 4) == ELIMIT


def test_an_empty_grid_is_a_no_op(lib):
    call = _Call(lib)
    assert call(rows=0) == OK and call(rows=0, out=None) == OK and call(rows=0, users=call.users) == OK
    assert call(user0=5, rows=0) == OK                                # the empty range at the table's end
    assert call(num_items=0, ldo=0) == OK and call(num_items=0, ldo=0, out=None) == OK
    for embed in ADMITTED:
        assert call(rows=0, embed=embed) == OK, embed
        assert call(num_items=0, ldo=0, embed=embed) == OK, embed


# ---- the Python layer: what is refused before a device is needed
def test_argument_errors_that_need_no_device(lib):
    from deeplearningrecommendationsystem_amd.model import PNN
    nu, ni = 11, 13
    with pytest.raises(ValueError, match="num_fields"):
        PNN(16, TOWER, num_fields=4, vocab=10).catalogue_scorer(_stub_assembler(10, 10))
    models = [PNN(16, TOWER, num_users=nu, num_items=ni), PNN(256, TOWER, num_users=nu, num_items=ni),
              PNN(16, TOWER, "out", num_users=nu, num_items=ni), PNN(8, [32, 16, 8], num_users=nu, num_items=ni)]
    for model, path in zip(models, ("grid", "grid", "forward", "forward")):
        for bad in (_stub_assembler(nu + 1, ni), _stub_assembler(nu, ni - 1)):
            with pytest.raises(ValueError, match="built for"):
                model.catalogue_scorer(bad)
        wrong_width = SimpleNamespace(user_features=torch.empty((nu, 23)), item_features=torch.empty((ni, 19)))
        with pytest.raises(ValueError):
            model.catalogue_scorer(wrong_width)
        scorer = model.catalogue_scorer(_stub_assembler(nu, ni))
        assert scorer.path == path
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
