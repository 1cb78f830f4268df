"""CPU: the user-grid frame of ``model/_grid.py`` on a stub scorer (score = 100 * user + item) -- which rows reach
``_scores``, that ``_shared()`` runs once per public call and reaches every chunk, and that every argument error is
raised before ``_shared()`` runs.  CPU tensors, no library call; ``recommend``'s ranking runs on the device:
tests/test_gpu_grid_scorer.py."""
from types import SimpleNamespace

import pytest
import torch

NU, NI = 7, 5


def _stub():
    from deeplearningrecommendationsystem_amd.model._grid import UserGridScorer

    class Stub(UserGridScorer):
        def __init__(self):
            super().__init__(NU, NI, "cpu")
            self.shared_calls, self.score_calls = 0, []

        def _shared(self):
            self.shared_calls += 1
            return ("shared", self.shared_calls)

        def _scores(self, users, start, stop, shared):
            self.score_calls.append(shared)
            u = users if users is not None else torch.arange(start, stop)
            return (100 * u[:, None] + torch.arange(NI)[None, :]).to(torch.float32)

    return Stub()


def _want(users):
    return (100 * torch.as_tensor(users, dtype=torch.int64).reshape(-1, 1) + torch.arange(NI)[None, :]).float()


def test_score_rows_and_score_grid_return_the_rows_asked_for():
    sc = _stub()
    for s, e in ((0, NU), (2, 5), (NU - 1, NU)):
        assert torch.equal(sc.score_rows(s, e), _want(range(s, e)))
        assert torch.equal(sc(s, e), _want(range(s, e)))                     # the ranking_metrics callable
    assert sc.score_rows(3, 3).shape == (0, NI)
    assert torch.equal(sc.score_grid([3, 1, 3, 0]), _want([3, 1, 3, 0]))     # a list with repeats
    assert torch.equal(sc.score_grid(torch.tensor([6, 6])), _want([6, 6]))
    assert torch.equal(sc.score_grid(None), _want(range(NU)))
    got = sc.score_grid([])
    assert got.shape == (0, NI) and got.dtype == torch.float32


def test_shared_runs_once_per_public_call_and_reaches_scores():
    sc = _stub()
    calls = [lambda: sc.score_rows(1, 4), lambda: sc(0, 2), lambda: sc.score_grid([2, 2]), lambda: sc.score_grid()]
    for k, call in enumerate(calls, start=1):
        call()
        assert sc.shared_calls == k and sc.score_calls == [("shared", j) for j in range(1, k + 1)]


def test_range_and_id_errors_come_before_shared():
    sc = _stub()
    for s, e in ((-1, 2), (2, NU + 1), (3, 2)):
        with pytest.raises(IndexError, match="are outside"):
            sc.score_rows(s, e)
    for bad in ([NU], [-1], [0, 1, NU + 3]):
        with pytest.raises(IndexError, match="outside"):
            sc.score_grid(bad)
        with pytest.raises(IndexError, match="outside"):
            sc.recommend(bad, n=3)
    assert sc.shared_calls == 0 and sc.score_calls == []


def test_recommend_argument_errors_come_before_shared():
    sc = _stub()
    with pytest.raises(ValueError, match="n must be at least 1"):
        sc.recommend(n=0)
    for shape in ((NU + 1, NI), (NU, NI - 1)):
        with pytest.raises(ValueError, match="exclude was built for"):
            sc.recommend(n=3, exclude=SimpleNamespace(num_users=shape[0], num_items=shape[1]))
    with pytest.raises(ValueError, match="n must be at least 1"):            # n is checked first
        sc.recommend(n=0, exclude=SimpleNamespace(num_users=NU + 1, num_items=NI))
    assert sc.shared_calls == 0 and sc.score_calls == []
