"""CPU: which DIN shapes the history x item grid kernel admits (a function of shapes alone), the host-side argument
checks of ``ctr_din_grid_pool``, which run before anything is enqueued and so need no device, and the argument errors
of ``DIN.score_histories`` / ``history_scorer`` / ``recommend`` that are decided before a device is touched."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib


def _attention_dims(embed, device="meta"):
    """the attention weights' shapes of DIN(., embed) read off storage-free tensors"""
    return [tuple(torch.empty(n, k, device=device).shape) for n, k in ((128, 3 * embed), (64, 128), (1, 64))]


@pytest.mark.parametrize("num_items", [1, 1682, 26744, 10_000_000])
def test_embed_64_is_admitted_at_any_table_size(lib, num_items):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import din
    table = torch.empty(num_items, 64, device="meta")
    assert ops.din_grid_supported(table.shape[1], _attention_dims(64))
    assert din.grid_path(table.shape[1]) == "grid"


@pytest.mark.parametrize("embed", [8, 128])
def test_other_embed_sizes_are_refused(lib, embed):
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import din
    assert not ops.din_grid_supported(embed, _attention_dims(embed))
    assert din.grid_path(embed) == "forward"


def test_other_attention_widths_are_refused(lib):
    from deeplearningrecommendationsystem_amd import ops
    assert not ops.din_grid_supported(64, [(64, 192), (64, 64), (1, 64)])
    assert not ops.din_grid_supported(64, [(128, 192), (32, 128), (1, 32)])
    assert not ops.din_grid_supported(64, [(128, 192), (64, 128)])


def test_cpu_models_will_do(lib):
    from deeplearningrecommendationsystem_amd.model import DIN, din
    for embed, want in ((64, "grid"), (8, "forward")):
        p = DIN(7, embed)._params()
        assert din.grid_path(p.table.shape[1], [tuple(layer.weight.shape) for layer in p.att]) == want


# ---- the C entry: every refusal below is decided on the host, before a launch
class _Call:
    """arguments of ctr_din_grid_pool over host buffers (never dereferenced: nothing below reaches a launch)"""

    def __init__(self, lib, ni=7, rows=3, length=5):
        self.lib = lib
        self.keep = [(ctypes.c_float * 64)() for _ in range(9)]        # 16-byte aligned stand-ins for device memory
        addr = [ctypes.addressof(b) + (-ctypes.addressof(b)) % 16 for b in self.keep]
        self.a = dict(table=addr[0], num_items=ni, embed=64, at=addr[1], ah=addr[2], ah_by_position=0, w2=addr[3],
                      b2=addr[4], w3=addr[5], n1=128, n2=64, hist=addr[6], rows=rows, len=length, out=addr[7], ldo=128,
                      err_flag=addr[8], stream=None)

    def __call__(self, **changed):
        a = dict(self.a, **changed)
        return self.lib.load().ctr_din_grid_pool(*a.values())


OK, EINVAL = 0, -1


def test_null_pointers_are_refused(lib):
    call = _Call(lib)
    for name in ("table", "at", "ah", "w2", "b2", "w3", "hist", "out"):
        assert call(**{name: None}) == EINVAL, name


def test_shapes_not_admitted_are_refused(lib):
    call = _Call(lib)
    for embed in (8, 16, 32, 128):
        assert call(embed=embed) == EINVAL, embed
    assert call(n1=64) == EINVAL and call(n2=32) == EINVAL and call(n1=256) == EINVAL
    assert call(len=0) == EINVAL and call(len=-3) == EINVAL
    assert call(ldo=63) == EINVAL and call(ldo=0) == EINVAL          # narrower than a pooled row
    assert call(ldo=66) == EINVAL                                     # rows that are not 16-byte aligned
    assert call(rows=-1) == EINVAL and call(num_items=-1) == EINVAL
    assert call(num_items=1 << 31) == EINVAL
    assert call(table=call.a["table"] + 4) == EINVAL                  # a misaligned table


def test_an_empty_grid_is_a_no_op(lib):
    call = _Call(lib)
    assert call(rows=0) == OK and call(rows=0, hist=None, out=None) == OK
    assert call(num_items=0) == OK and call(num_items=0, out=None) == OK
    assert call(rows=0, err_flag=None) == OK


# ---- the Python layer: what is refused before a device is needed
def test_argument_errors_that_need_no_device(lib):
    from deeplearningrecommendationsystem_amd.model import DIN
    model = DIN(11, 64)
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
    model.sharded = True                                              # (what DIN(..., sharded=True) sets)
    for call in (model.score_histories, model.history_scorer, model.recommend):
        with pytest.raises(ValueError, match="sharded"):
            call(good)
