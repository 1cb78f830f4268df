"""CPU: which DeepFM shapes the user x item grid kernel admits (a function of shapes alone), the host-side argument
checks of ``ctr_deepfm_grid_scores``, which run before anything is enqueued and so need no device, and the argument
errors of ``catalogue_scorer`` and its scorer that are decided before a device is touched."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


# ---- admission
@pytest.mark.parametrize("embed", [16, 128])
@pytest.mark.parametrize("hidden", [[512, 256, 128, 1], [64, 256, 128, 1]])
def test_the_pinned_tower_is_admitted_at_both_embedding_sizes(lib, hidden, embed):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import deepfm
    assert ops.deepfm_grid_supported(hidden, embed)
    assert deepfm.grid_path(hidden, embed) == "grid"


@pytest.mark.parametrize("hidden,embed", [([512, 256, 128], 16), ([512, 128, 128, 1], 16), ([32, 16, 1], 16),
                                          ([512, 256, 128, 1], 8), ([512, 256, 128, 1], 24), ([512, 256, 128, 1], 144),
                                          ([512, 256, 128, 1, 1], 16), ([512, 256, 128, 2], 128)])
def test_other_shapes_take_the_forward_path(lib, hidden, embed):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import deepfm
    assert not ops.deepfm_grid_supported(hidden, embed)
    assert deepfm.grid_path(hidden, embed) == "forward"


def test_every_multiple_of_sixteen_up_to_128_is_admitted(lib):
    from deeplearningrecommendationsystem_amd import ops
    assert [e for e in range(1, 200) if ops.deepfm_grid_supported([512, 256, 128, 1], e)] == list(range(16, 129, 16))


def _stub_assembler(nu, ni, device="cpu"):
    return SimpleNamespace(user_features=torch.empty((nu, 24), device=device),
                           item_features=torch.empty((ni, 19), device=device))


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_cpu_models_and_meta_tensors_will_do(lib, device):
    from deeplearningrecommendationsystem_amd.model import DeepFM, _base, deepfm
    for hidden, embed, want in (([512, 256, 128, 1], 16, "grid"), ([64, 256, 128, 1], 128, "grid"),
                                ([32, 16, 1], 8, "forward"), ([512, 256, 128, 1], 8, "forward")):
        model = DeepFM(7, 9, hidden, embed).to(device)
        widths = [model.linear.out_features] + [lin.out_features for lin in model.dnn_network]
        assert deepfm.grid_path(widths, model.user_embedding.embedding_dim) == want
        scorer = model.catalogue_scorer(_stub_assembler(7, 9, device))
        assert scorer.path == want and isinstance(scorer, _base.CatalogueScorer)
        assert (scorer.num_users, scorer.num_items) == (7, 9)


def test_the_tile_constants_mirror_the_header(lib):
    from deeplearningrecommendationsystem_amd import ops
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define (CTR_[A-Z0-9_]+) (\d+)\b", text, flags=re.M)}
    assert ops.DEEPFM_GRID_ITEM_TILE == lib.CTR_DEEPFM_GRID_ITEM_TILE == defines["CTR_DEEPFM_GRID_ITEM_TILE"]
    assert ops.DEEPFM_GRID_USER_TILE == lib.CTR_DEEPFM_GRID_USER_TILE == defines["CTR_DEEPFM_GRID_USER_TILE"]
    assert ops.DEEPFM_GRID_ITEM_TILE % 16 == 0 and ops.DEEPFM_GRID_USER_TILE >= 1


# ---- the C entry: every refusal below is decided on the host, before a launch
class _Call:
    """arguments of ctr_deepfm_grid_scores over host buffers (never dereferenced: nothing below reaches a launch)"""

    def __init__(self, lib, nu=5, ni=7, rows=3):
        self.lib = lib
        self.keep = [(ctypes.c_float * 64)() for _ in range(14)]       # 16-byte aligned stand-ins for device memory
        addr = [ctypes.addressof(b) + (-ctypes.addressof(b)) % 16 for b in self.keep]
        self.a = dict(zu=addr[0], zi=addr[1], su=addr[2], si=addr[3], a=addr[4], b=addr[5], num_users=nu, num_items=ni,
                      embed=16, n1=256, n2=128, w2=addr[6], b2=addr[7], w3=addr[8], b3=addr[9], out_w=addr[10],
                      out_b=addr[11], users=None, user0=0, rows=rows, out=addr[13], ldo=ni, row_blocks=0, stream=None)
        self.users = addr[12]

    def __call__(self, **changed):
        a = dict(self.a, **changed)
        return self.lib.load().ctr_deepfm_grid_scores(*a.values())


OK, EINVAL, ELIMIT, EALIGN = 0, -1, -2, -4


def test_null_pointers_are_refused(lib):
    call = _Call(lib)
    for name in ("zu", "zi", "su", "si", "a", "b", "w2", "b2", "w3", "b3", "out_w", "out_b", "out"):
        assert call(**{name: None}) == EINVAL, name


def test_bad_counts_are_refused(lib):
    call = _Call(lib)
    assert call(rows=-1) == EINVAL and call(row_blocks=-1) == EINVAL
    assert call(num_users=-1) == EINVAL and call(num_items=-1) == EINVAL
    assert call(ldo=6) == EINVAL and call(ldo=0) == EINVAL            # narrower than a row of scores
    assert call(rows=6) == EINVAL and call(user0=3, rows=3) == EINVAL and call(user0=-1) == EINVAL   # outside the table
    assert call(num_users=0, users=call.users) == EINVAL              # rows of an empty table


def test_shapes_not_admitted_are_refused(lib):
    call = _Call(lib)
    for embed in (0, 8, 24, 100, 144, 256, -16):
        assert call(embed=embed) == ELIMIT, embed
    assert call(n1=128) == ELIMIT and call(n1=512) == ELIMIT and call(n2=64) == ELIMIT and call(n2=256) == ELIMIT
    assert call(num_items=1 << 31, ldo=1 << 31) == ELIMIT
    assert call(num_users=1 << 31) == ELIMIT


def test_misaligned_rows_are_refused(lib):
    call = _Call(lib)
    for name in ("zu", "zi", "su", "si", "w2"):
        assert call(**{name: call.a[name] + 4}) == EALIGN, name


def test_an_empty_grid_is_a_no_op(lib):
    call = _Call(lib)
    assert call(rows=0) == OK and call(rows=0, out=None) == OK and call(rows=0, users=call.users) == OK
    assert call(num_items=0, ldo=0) == OK and call(num_items=0, ldo=0, out=None) == OK
    for embed in range(16, 129, 16):
        assert call(rows=0, embed=embed) == OK, embed


# ---- the Python layer: what is refused before a device is needed
def test_argument_errors_that_need_no_device(lib):
    from deeplearningrecommendationsystem_amd.model import PNN, DeepFM, LogisticRegression
    nu, ni = 11, 13
    with pytest.raises(ValueError, match="num_fields"):
        DeepFM(None, None, [512, 256, 128, 1], 16, num_fields=4, vocab=10).catalogue_scorer(_stub_assembler(10, 10))
    with pytest.raises(ValueError, match="num_fields"):
        PNN(8, [32, 16, 8], num_fields=4, vocab=10).catalogue_scorer(_stub_assembler(10, 10))
    models = [DeepFM(nu, ni, [512, 256, 128, 1], 16), DeepFM(nu, ni, [32, 16, 1], 8),
              PNN(8, [32, 16, 8], num_users=nu, num_items=ni), LogisticRegression(nu, ni, 43)]
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
