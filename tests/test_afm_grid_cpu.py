"""CPU: which AFM shapes the user x item grid kernel admits (a function of shapes alone), the host-side argument
checks of ``ctr_afm_grid_scores``, which run before anything is enqueued and so need no device, and the argument
errors of ``catalogue_scorer`` and its scorer that are decided before a device is touched."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATT = 64
ADMITTED = list(range(16, 129, 16))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


# ---- admission
def test_exactly_the_multiples_of_sixteen_up_to_128_are_admitted(lib):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import afm
    assert [e for e in range(1, 301) if ops.afm_grid_supported(e, ATT)] == ADMITTED
    assert [e for e in range(1, 301) if afm.grid_path(e, ATT) == "grid"] == ADMITTED
    assert (ops.AFM_GRID_ATTENTION, ops.AFM_GRID_MAX_EMBED, ops.AFM_GRID_CROSS) == (ATT, 128, 8)


@pytest.mark.parametrize("attention", [32, 63, 65, 128])
def test_other_attention_widths_take_the_forward_path(lib, attention):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import afm
    for embed in ADMITTED:
        assert not ops.afm_grid_supported(embed, attention)
        assert afm.grid_path(embed, attention) == "forward"


@pytest.mark.parametrize("embed", [8, 144])
def test_embedding_widths_outside_the_range_take_the_forward_path(lib, embed):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import afm
    assert not ops.afm_grid_supported(embed, ATT)
    assert afm.grid_path(embed, ATT) == "forward"


def test_the_pair_columns_are_pnns(lib):
    from deeplearningrecommendationsystem_amd.model import _base, afm, pnn
    assert (_base._USER_FIELDS, _base._ITEM_FIELDS) == ((0, 2, 3, 4), (1, 5))
    assert afm._CROSS_PAIRS is pnn._CROSS_PAIRS and afm._CROSS_PAIRS == [0, 4, 5, 6, 7, 11, 13, 14]
    assert afm._USER_PAIRS == [1, 2, 3, 9, 10, 12] and afm._ITEM_PAIRS == [8]
    assert (afm.NVEC, afm.NPAIRS) == (6, 15) == (6, len(afm._USER_PAIRS + afm._ITEM_PAIRS + afm._CROSS_PAIRS))


def _stub_assembler(nu, ni, device="cpu"):
    return SimpleNamespace(user_features=torch.empty((nu, 24), device=device),
                           item_features=torch.empty((ni, 19), device=device))


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_cpu_models_and_meta_tensors_will_do(lib, device):
    from deeplearningrecommendationsystem_amd.model import AFM, _base, afm
    for embed, attention, want in ((16, 64, "grid"), (128, 64, "grid"), (48, 64, "grid"), (16, 32, "forward"),
                                   (8, 64, "forward"), (144, 64, "forward"), (128, 128, "forward")):
        model = AFM(7, 9, embed, attention).to(device)
        scorer = model.catalogue_scorer(_stub_assembler(7, 9, device))
        assert scorer.path == want and isinstance(scorer, _base.CatalogueScorer)
        assert (type(scorer) is afm._GridScorer) == (want == "grid")
        assert (type(scorer) is _base.CatalogueScorer) == (want == "forward")
        assert (scorer.num_users, scorer.num_items) == (7, 9)
        if want == "grid":
            assert isinstance(scorer, _base.SixFieldGridScorer) and scorer.row_blocks == 0


def test_the_field_specs_hook_defaults_to_the_six_tables(lib):
    """DeepFM's and PNN's scorers read the embedding stage's field list through the hook AFM overrides"""
    from deeplearningrecommendationsystem_amd.model import PNN, _base, afm
    assert afm._GridScorer._field_specs is not _base.SixFieldGridScorer._field_specs
    model = PNN(16, [256, 128, 64, 32], num_users=7, num_items=9)
    scorer = model.catalogue_scorer(_stub_assembler(7, 9))
    assert type(scorer)._field_specs is _base.SixFieldGridScorer._field_specs
    p = model._params()
    got = scorer._field_specs(p, 16, torch.device("cpu"))
    want = _base.six_field_specs([t.detach() for t in p.tables], 16)
    assert len(got) == len(want) == 6
    for a, b in zip(got, want):
        assert (a.kind, a.width, a.out_col, a.src_col, a.bag_size) == (b.kind, b.width, b.out_col, b.src_col, b.bag_size)
        assert a.table.data_ptr() == b.table.data_ptr()


def test_the_tile_constants_mirror_the_header(lib):
    from deeplearningrecommendationsystem_amd import ops
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define (CTR_[A-Z0-9_]+) (\d+)\b", text, flags=re.M)}
    assert ops.AFM_GRID_ITEM_TILE == lib.CTR_AFM_GRID_ITEM_TILE == defines["CTR_AFM_GRID_ITEM_TILE"]
    assert ops.AFM_GRID_USER_TILE == lib.CTR_AFM_GRID_USER_TILE == defines["CTR_AFM_GRID_USER_TILE"]
    assert ops.AFM_GRID_ITEM_TILE % 16 == 0 and ops.AFM_GRID_USER_TILE >= 1
    assert re.search(r"\bint\s+ctr_afm_grid_scores\s*\(", text) and "ctr_afm_grid_scores" in lib.SIGNATURES


# ---- the C entry: every refusal below is decided on the host, before a launch
POINTERS = ("su", "si", "fu", "fi", "att_w", "att_b", "att_h", "out_w")


class _Call:
    """arguments of ctr_afm_grid_scores over host buffers (never dereferenced: nothing below reaches a launch)"""

    def __init__(self, lib, nu=5, ni=7, rows=3):
        self.lib = lib
        self.keep = [(ctypes.c_float * 64)() for _ in range(len(POINTERS) + 2)]   # 16-byte aligned stand-ins for device memory
        addr = [ctypes.addressof(b) + (-ctypes.addressof(b)) % 16 for b in self.keep]
        at = dict(zip(POINTERS, addr))
        self.a = dict(su=at["su"], si=at["si"], fu=at["fu"], fi=at["fi"], num_users=nu, num_items=ni, embed=16,
                      attention=ATT, att_w=at["att_w"], att_b=at["att_b"], att_h=at["att_h"], out_w=at["out_w"],
                      users=None, user0=0, rows=rows, out=addr[-1], ldo=ni, row_blocks=0, stream=None)
        self.users = addr[-2]

    def __call__(self, **changed):
        a = dict(self.a, **changed)
        return self.lib.load().ctr_afm_grid_scores(*a.values())


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
    for embed in (0, 8, 24, 100, 144, 256, -16):
        assert call(embed=embed) == ELIMIT, embed
    for attention in (0, 32, 63, 65, 128):
        assert call(attention=attention) == ELIMIT, attention
        assert call(attention=attention, embed=128) == ELIMIT, attention
    assert call(num_items=1 << 31, ldo=1 << 31) == ELIMIT
    assert call(num_users=1 << 31) == ELIMIT


def test_misaligned_rows_are_refused(lib):
    """the pointers the kernel reads in 16-byte pieces: the users' scalars, both sides' field vectors, attention_W"""
    call = _Call(lib)
    for name in ("su", "fu", "fi", "att_w"):
        assert call(**{name: call.a[name] + 4}) == EALIGN, name
    for name in ("si", "att_b", "att_h", "out_w"):                    # read one float at a time
        assert call(rows=0, **{name: call.a[name] + 4}) == OK, name


def test_a_refusal_for_the_arguments_comes_before_one_for_the_shape(lib):
    """CTR_EINVAL, then CTR_ELIMIT, then CTR_EALIGN, as ctr_pnn_grid_scores orders them"""
    call = _Call(lib)
    assert call(su=None, embed=8) == EINVAL
    assert call(rows=-1, attention=32, fu=call.a["fu"] + 4) == EINVAL
    assert call(embed=8, fi=call.a["fi"] + 4) == ELIMIT
    assert call(attention=32, su=call.a["su"] + 4) == ELIMIT
    assert call(num_users=1 << 31, fu=call.a["fu"] + 4) == ELIMIT


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
    from deeplearningrecommendationsystem_amd.model import AFM
    nu, ni = 11, 13
    models = [AFM(nu, ni, 16, 64), AFM(nu, ni, 128, 64), AFM(nu, ni, 16, 32), AFM(nu, ni, 8, 64)]
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
