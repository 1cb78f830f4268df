"""CPU: the host-side pieces of ``topn.py`` -- the chunk rule, the user-list check, the CSR rows ``rank_mask`` takes and
the flat walk over the row x item grid -- on CPU tensors.  ``top_n`` itself ranks on the device: tests/test_gpu_topn.py."""
import numpy as np
import pytest
import torch


def _topn():
    from deeplearningrecommendationsystem_amd import topn
    return topn


def test_chunk_rows_default_rule():
    topn = _topn()
    assert (topn.SCORE_CHUNK_FLOATS, topn.MAX_ROWS) == (1 << 27, 65535)
    assert topn.chunk_rows(1) == 65535                       # the row bound
    assert topn.chunk_rows(26_744) == (1 << 27) // 26_744 == 5018
    assert topn.chunk_rows(2 ** 27 + 1) == 1                 # a row longer than the chunk still goes, alone


def test_chunk_rows_reads_lowered_constants(monkeypatch):
    topn = _topn()
    monkeypatch.setattr(topn, "SCORE_CHUNK_FLOATS", 4 * 7)
    assert topn.chunk_rows(7) == 4 and topn.chunk_rows(29) == 1
    monkeypatch.setattr(topn, "MAX_ROWS", 3)
    assert topn.chunk_rows(7) == 3 and topn.chunk_rows(1) == 3


def test_users_tensor():
    users_tensor = _topn().users_tensor
    assert torch.equal(users_tensor(None, 5, "cpu"), torch.arange(5))
    for users in ([4, 0, 0, 2], torch.tensor([4, 0, 0, 2], dtype=torch.int32), np.array([[4, 0], [0, 2]])):
        got = users_tensor(users, 5, "cpu")
        assert got.dtype == torch.int64 and got.tolist() == [4, 0, 0, 2]
    empty = users_tensor([], 5, "cpu")
    assert empty.shape == (0,) and empty.dtype == torch.int64
    for bad in ([0, -1], [5], torch.tensor([2, 5])):
        with pytest.raises(IndexError, match="outside"):
            users_tensor(bad, 5, "cpu")


def test_excluded_rows_are_each_users_sorted_distinct_items():
    from deeplearningrecommendationsystem_amd.data import ObservedPairs
    nu, ni = 6, 9
    gen = torch.Generator().manual_seed(4)
    u = torch.randint(0, nu - 1, (40,), generator=gen)
    u[u == 3] = 5                                            # user 3 is left without a pair, user 5 has some
    i = torch.randint(0, ni, (40,), generator=gen)
    observed = ObservedPairs(u, i, nu, ni)
    users = torch.tensor([5, 3, 0, 0, 2])
    off, ids = _topn().excluded_rows(observed, users)
    assert off.dtype == ids.dtype == torch.int64 and off.shape == (6,) and off[0] == 0 and off[-1] == ids.numel()
    for r, user in enumerate(users.tolist()):
        assert ids[off[r]:off[r + 1]].tolist() == sorted(set(i[u == user].tolist())), (r, user)
    assert off[2] == off[1] and off[1] > 0 and 40 > ids.numel() > 0


def test_forward_grid_fills_every_cell_from_its_pair():
    calls = []

    def forward(r, i):
        assert r.dtype == i.dtype == torch.int64 and r.dim() == i.dim() == 1
        calls.append(r.numel())
        return (100 * r + i).to(torch.float32).view(-1, 1)   # a model's forward returns a column

    out = torch.full((5, 7), -1.0)
    assert _topn().forward_grid(out, 4, forward) is None
    assert calls == [4] * 8 + [3]
    assert torch.equal(out, (100 * torch.arange(5)[:, None] + torch.arange(7)[None, :]).float())
    calls.clear()
    _topn().forward_grid(torch.empty((0, 7)), 4, forward)
    assert calls == []
