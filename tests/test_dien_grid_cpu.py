"""CPU: which DIEN shapes the history x item grid kernel admits (a function of shapes alone), the host-side argument
checks of ``ctr_dien_grid_hidden``, which run before anything is enqueued and so need no device, and the argument
errors of ``DIEN.score_histories`` / ``history_scorer`` / ``recommend`` that are decided before a device is touched."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


def _attention_dims(embed, device="meta"):
    """the attention weights' shapes of DIEN(., embed) read off storage-free tensors"""
    return [tuple(torch.empty(n, k, device=device).shape) for n, k in ((64, 3 * embed), (32, 64), (1, 32))]


@pytest.mark.parametrize("num_items", [1, 1682, 26744, 10_000_000])
def test_embed_16_is_admitted_at_any_table_size(lib, num_items):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import dien
    table = torch.empty(num_items, 16, device="meta")
    assert ops.dien_grid_supported(table.shape[1], _attention_dims(16))
    assert dien.grid_path(table.shape[1]) == "grid"


@pytest.mark.parametrize("embed", [8, 32, 64])
def test_other_embed_sizes_are_refused(lib, embed):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import dien
    assert not ops.dien_grid_supported(embed, _attention_dims(embed))
    assert dien.grid_path(embed) == "forward"


def test_other_attention_widths_are_refused(lib):
    from deeplearningrecommendationsystem_amd import ops
    assert not ops.dien_grid_supported(16, [(32, 48), (32, 32), (1, 32)])
    assert not ops.dien_grid_supported(16, [(64, 48), (16, 64), (1, 16)])
    assert not ops.dien_grid_supported(16, [(128, 48), (64, 128), (1, 64)])      # DIN's widths
    assert not ops.dien_grid_supported(16, [(64, 48), (32, 64)])


def test_cpu_models_will_do(lib):
    from deeplearningrecommendationsystem_amd.model import DIEN, dien
    for embed, want in ((16, "grid"), (8, "forward")):
        p = DIEN(7, embed)._params()
        assert dien.grid_path(p.table.shape[1], [tuple(layer.weight.shape) for layer in p.att]) == want


def test_the_kept_scores_length_is_mirrored(lib):
    from deeplearningrecommendationsystem_amd import ops
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    assert ops.DIEN_GRID_KEEP == int(re.search(r"^#define CTR_DIEN_GRID_KEEP (\d+)\b", text, flags=re.M).group(1))
    assert ops.DIEN_GRID_KEEP >= 100          # the benchmark's and the scripts' history length stays in LDS


# ---- the C entry: every refusal below is decided on the host, before a launch
class _Call:
    """arguments of ctr_dien_grid_hidden over host buffers (never dereferenced: nothing below reaches a launch)"""

    def __init__(self, lib, ni=7, rows=3, length=5):
        self.lib = lib
        self.keep = [(ctypes.c_float * 64)() for _ in range(11)]       # 16-byte aligned stand-ins for device memory
        addr = [ctypes.addressof(b) + (-ctypes.addressof(b)) % 16 for b in self.keep]
        self.a = dict(at=addr[0], hp=addr[1], hp_by_position=0, num_items=ni, embed=16, w2=addr[2], b2=addr[3],
                      w3=addr[4], n1=64, n2=32, b_ih=addr[5], w_hh=addr[6], b_hh=addr[7], hist=addr[8], rows=rows,
                      len=length, out=addr[9], ldo=32, err_flag=addr[10], stream=None)

    def __call__(self, **changed):
        a = dict(self.a, **changed)
        return self.lib.load().ctr_dien_grid_hidden(*a.values())


OK, EINVAL, ELIMIT, EALIGN = 0, -1, -2, -4


def test_null_pointers_are_refused(lib):
    call = _Call(lib)
    for name in ("at", "hp", "w2", "b2", "w3", "b_ih", "w_hh", "b_hh", "hist", "out"):
        assert call(**{name: None}) == EINVAL, name


def test_shapes_not_admitted_are_refused(lib):
    call = _Call(lib)
    for embed in (8, 32, 64):
        assert call(embed=embed) == ELIMIT, embed
    assert call(n1=128) == ELIMIT and call(n2=64) == ELIMIT and call(n1=32) == ELIMIT and call(n2=16) == ELIMIT
    assert call(num_items=1 << 31) == ELIMIT
    assert call(len=0) == EINVAL and call(len=-3) == EINVAL
    assert call(ldo=15) == EINVAL and call(ldo=12) == EINVAL and call(ldo=0) == EINVAL   # narrower than a state
    assert call(rows=-1) == EINVAL and call(num_items=-1) == EINVAL
    assert call(ldo=18) == EALIGN and call(ldo=33) == EALIGN           # rows that are not 16-byte aligned
    for name in ("at", "hp", "w2", "out"):
        assert call(**{name: call.a[name] + 4}) == EALIGN, name         # a misaligned matrix
    assert call(ldo=16, rows=0) == OK and call(ldo=20, rows=0) == OK   # (the no-op return sits behind every check)


def test_an_empty_grid_is_a_no_op(lib):
    call = _Call(lib)
    assert call(rows=0) == OK and call(rows=0, hist=None, out=None) == OK
    assert call(num_items=0) == OK and call(num_items=0, out=None) == OK
    assert call(rows=0, err_flag=None) == OK


# ---- the Python layer: what is refused before a device is needed
def test_argument_errors_that_need_no_device(lib):
    from deeplearningrecommendationsystem_amd.model import DIEN
    model = DIEN(11, 16)
    good = torch.zeros((2, 3), dtype=torch.int64)                     # right shape and type, but on the host
    for bad in (good, good[0], good.int(), torch.zeros((2, 0), dtype=torch.int64), [[1, 2]]):
        with pytest.raises(ValueError):
            model.score_histories(bad)
        with pytest.raises(ValueError):
            model.history_scorer(bad)
        with pytest.raises(ValueError):
            model.recommend(bad, n=3)
    with pytest.raises(ValueError):
        model.recommend(good, n=0)
    model.sharded = True                                              # (what DIEN(..., sharded=True) sets)
    for call in (model.score_histories, model.history_scorer, model.recommend):
        with pytest.raises(ValueError, match="sharded"):
            call(good)
