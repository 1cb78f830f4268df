"""CPU: the score-level evaluation as restated in score_numpy.py (the GPU tests compare the kernels of
csrc/score_eval.hip with it): the per-user AUC of the restatement pinned to sklearn's roc_auc_score, the UserGroups
plan on CPU tensors, the host-side argument checks of the two entry points through the loaded library, the mirrors of
the header's limits, and gauc_from_counts on hand-made counts."""
import math
import os
import re

import numpy as np
import pytest
import torch

import score_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recipe():
    users, y, p = sn.recipe()
    for t in (users, y, p):
        t.setflags(write=False)
    return users, y, p


def test_recipe_is_the_stated_one(recipe):
    users, y, p = recipe
    plan = sn.user_groups(users)
    assert users.shape[0] == 12697 and plan["sizes"].shape[0] == 213
    assert sorted(plan["sizes"].tolist())[-9:] == sn.FIXED_SIZES[4:]
    assert int(np.isnan(p).sum()) == 5


def test_restated_user_auc_is_sklearn_roc_auc(recipe):
    """every group that has both classes and finite scores: u2 / (2 pos neg) is roc_auc_score within 1e-12"""
    from sklearn.metrics import roc_auc_score
    users, y, p = recipe
    plan = sn.user_groups(users)
    pos, neg, u2, err = sn.group_counts(p, y, plan["order"], plan["offsets"])
    assert err == 0 and int(pos.sum()) == int(sn.positive(y).sum()) and int((pos + neg).sum()) == users.shape[0]
    compared, worst = 0, 0.0
    for g in range(pos.shape[0]):
        members = plan["order"][plan["offsets"][g]:plan["offsets"][g + 1]]
        assert (users[members] == plan["group_users"][g]).all()
        if pos[g] == 0 or neg[g] == 0 or not np.isfinite(p[members]).all():
            continue
        want = roc_auc_score(y[members], p[members])
        worst = max(worst, abs(u2[g] / (2.0 * pos[g] * neg[g]) - want))
        compared += 1
    print(f"compared {compared} groups, worst difference {worst:.3g}")
    assert compared >= 190, "fewer groups compared than the recipe holds"
    assert worst <= 1e-12
    sizes = plan["sizes"]
    constant = int(np.flatnonzero(sizes == 1025)[0])
    assert u2[constant] == pos[constant] * neg[constant]            # all ties: AUC 0.5 exactly
    assert ((pos[sizes == 63] == 0) & (neg[sizes == 63] == 63)).all()
    pairs = np.flatnonzero(sizes == 2)
    assert sorted(zip(pos[pairs].tolist(), neg[pairs].tolist()))[-1] == (2, 0)
    value, mean, scored, samples = sn.gauc(pos, neg, u2)
    assert 0.4 < value < 0.6 and 0.4 < mean < 0.6 and scored >= 190 and samples <= users.shape[0]


def test_restated_pairs_treat_nan_and_signed_zero_as_ieee_does():
    p = np.array([0.0, -0.0, np.nan, 0.5, np.nan, 0.5, 0.25], dtype=np.float32)
    y = np.array([1, 0, 0, 1, 1, 0, np.nan], dtype=np.float32)      # the NaN target is a negative
    pos, neg, u2, err = sn.group_counts(p, y, np.arange(7), np.array([0, 7]))
    # positives 0.0, 0.5, NaN; negatives -0.0, NaN, 0.5, 0.25: (0.0: tie with -0.0) + (0.5: beats -0.0, 0.25, ties 0.5)
    assert (pos[0], neg[0], u2[0], err) == (3, 4, 1 + 2 + 2 + 1, 0)


def test_user_groups_on_cpu_tensors(recipe):
    from deeplearningrecommendationsystem_amd.evaluator import UserGroups
    users = recipe[0]
    groups = UserGroups(torch.from_numpy(users.copy()))
    n = users.shape[0]
    assert groups.num_samples == n and groups.num_groups == 213 and groups.max_group == 3000
    assert groups.order.dtype == torch.int32 and groups.offsets.dtype == torch.int64
    assert groups.group_users.dtype == torch.int64
    assert all(t.dtype == torch.int32 for t in (groups.small_groups, groups.slab_group, groups.slab_first))
    order, offsets = groups.order.numpy(), groups.offsets.numpy()
    assert sorted(order.tolist()) == list(range(n))                                   # a permutation
    assert offsets[0] == 0 and offsets[-1] == n and (np.diff(offsets) > 0).all()
    group_users = groups.group_users.numpy()
    assert len(set(group_users.tolist())) == groups.num_groups                         # every user one group
    for g in range(groups.num_groups):
        members = order[offsets[g]:offsets[g + 1]]
        assert (users[members] == group_users[g]).all()                                # every group one user
        assert (np.diff(members) > 0).all()                                            # in sample order
    sizes = np.diff(offsets)
    small, slab_group, slab_first = (t.numpy() for t in (groups.small_groups, groups.slab_group, groups.slab_first))
    assert sorted(small.tolist()) == np.flatnonzero(sizes <= 64).tolist()
    covered = sorted(small.tolist() + sorted(set(slab_group.tolist())))
    assert covered == list(range(groups.num_groups))                                   # every group exactly once
    for g in set(slab_group.tolist()):
        firsts = slab_first[slab_group == g].tolist()
        assert firsts == list(range(0, int(sizes[g]), 1024))                           # 0, 1024, .. below the size
    by_size = {int(s): int(g) for g, s in enumerate(sizes) if s >= 63}
    assert by_size[64] in small and by_size[65] not in small
    assert (slab_group == by_size[65]).sum() == 1 and (slab_group == by_size[1024]).sum() == 1
    assert (slab_group == by_size[1025]).sum() == 2 and (slab_group == by_size[2049]).sum() == 3
    assert groups.pair_evaluations() == int((sizes * np.where(sizes <= 64, sizes, -(-sizes // 1024) * 1024)).sum())
    # the restated plan is the same plan
    want = sn.user_groups(users)
    for name in ("order", "offsets", "group_users", "small_groups", "slab_group", "slab_first"):
        assert np.array_equal(getattr(groups, name).numpy(), want[name]), name


def test_user_groups_edge_inputs():
    from deeplearningrecommendationsystem_amd.evaluator import UserGroups
    empty = UserGroups(torch.zeros(0, dtype=torch.int64))
    assert empty.num_samples == 0 and empty.num_groups == 0 and empty.max_group == 0
    assert empty.offsets.tolist() == [0] and empty.small_groups.numel() == 0 and empty.slab_group.numel() == 0
    one = UserGroups(torch.tensor([1 << 40, -5, 1 << 40, 7]))                          # sparse, large, interleaved
    assert one.group_users.tolist() == [-5, 7, 1 << 40] and one.order.tolist() == [1, 3, 0, 2]
    assert one.offsets.tolist() == [0, 1, 2, 4] and one.small_groups.tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        UserGroups(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        UserGroups(torch.zeros((4, 1), dtype=torch.int64))
    with pytest.raises(ValueError):
        UserGroups(torch.zeros(1, dtype=torch.int64).expand(1 << 31))                  # N >= 2^31: refused unread


@pytest.fixture(scope="module")
def handle():
    import __graft_entry__ as g
    g.build()
    from deeplearningrecommendationsystem_amd import _lib
    return _lib.load()


def test_score_entry_points_validate_without_gpu(handle):
    one = 8   # any non-null address: the checks return before anything is read or launched
    assert handle.ctr_score_counts(None, None, 4, None, None, None) == -1
    assert handle.ctr_score_counts(None, one, 4, one, one, None) == -1
    assert handle.ctr_score_counts(one, one, 4, one, None, None) == -1
    assert handle.ctr_score_counts(one, one, -1, one, one, None) == -1
    assert handle.ctr_score_counts(None, None, 0, None, None, None) == 0              # n = 0: a no-op

    def gauc(prob=one, target=one, n=4, order=one, offsets=one, groups=1, small=one, num_small=1, slab_group=one,
             slab_first=one, num_slabs=1, pos=one, neg=one, u2=one):
        return handle.ctr_gauc_groups(prob, target, n, order, offsets, groups, small, num_small, slab_group, slab_first,
                                      num_slabs, pos, neg, u2, None, None)
    assert handle.ctr_gauc_groups(None, None, 4, None, None, 1, None, 1, None, None, 0, None, None, None, None, None) == -1
    for name in ("prob", "target", "order", "offsets", "small", "slab_group", "slab_first", "pos", "neg", "u2"):
        assert gauc(**{name: None}) == -1, name
    assert gauc(n=-1) == -1 and gauc(groups=-1) == -1 and gauc(num_small=-1) == -1 and gauc(num_slabs=-1) == -1
    assert gauc(n=1 << 31) == -2 and gauc(groups=1 << 31) == -2                       # CTR_ELIMIT
    assert handle.ctr_gauc_groups(None, None, 0, None, None, 0, None, 0, None, None, 0, None, None, None, None, None) == 0
    assert gauc(groups=0) == 0                                                        # no group: a no-op


def test_python_mirrors_of_the_score_limits_match_the_header(handle):
    from deeplearningrecommendationsystem_amd import _lib
    text = open(os.path.join(ROOT, "include", "ctrhip.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define (CTR_[A-Z0-9_]+)\s+(\d+)\b", text, flags=re.M)}
    for name, value in (("CTR_SCORE_CHUNK", 65536), ("CTR_GAUC_SMALL", 64), ("CTR_GAUC_SLAB", 1024)):
        assert defines[name] == value and getattr(_lib, name) == value, name
    assert (sn.CHUNK, sn.SMALL, sn.SLAB) == (_lib.CTR_SCORE_CHUNK, _lib.CTR_GAUC_SMALL, _lib.CTR_GAUC_SLAB)


def test_gauc_from_counts_on_hand_made_counts():
    from deeplearningrecommendationsystem_amd.evaluator import gauc_from_counts
    pos = np.array([1, 2, 0, 3, 1], dtype=np.int32)
    neg = np.array([1, 2, 5, 0, 3], dtype=np.int32)
    u2 = np.array([2, 4, 0, 0, 3], dtype=np.int64)       # AUCs 1.0, 0.5, -, -, 0.5 with weights 2, 4, -, -, 4
    got = gauc_from_counts(pos, neg, u2)
    assert got.users_scored == 3 and got.samples_scored == 10
    assert abs(got.gauc - (2 * 1.0 + 4 * 0.5 + 4 * 0.5) / 10) <= 1e-15
    assert abs(got.user_auc_mean - (1.0 + 0.5 + 0.5) / 3) <= 1e-15
    same = gauc_from_counts(torch.from_numpy(pos), torch.from_numpy(neg), torch.from_numpy(u2))
    assert same == got
    assert got == sn.gauc(pos, neg, u2)
    big = gauc_from_counts([1 << 30], [1 << 30], [1 << 61])                            # u2 = 2 pos neg: AUC 1
    assert big.gauc == 1.0 and big.samples_scored == 1 << 31
    none = gauc_from_counts(pos[2:4], neg[2:4], u2[2:4])                               # no group has both classes
    assert math.isnan(none.gauc) and math.isnan(none.user_auc_mean) and none.users_scored == 0
    assert none.samples_scored == 0
    empty = gauc_from_counts([], [], [])
    assert math.isnan(empty.gauc) and empty.users_scored == 0
    with pytest.raises(ValueError):
        gauc_from_counts(pos, neg[:3], u2)


def test_score_metrics_refuses_cpu_tensors_and_wrong_shapes():
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    from deeplearningrecommendationsystem_amd.evaluator import score_metrics
    y, p = torch.zeros(6), torch.full((6,), 0.5)
    with pytest.raises(CtrHipError):
        score_metrics(y, p)
    with pytest.raises(ValueError):
        score_metrics(y.double(), p)
    with pytest.raises(ValueError):
        score_metrics(y.view(3, 2), p.view(3, 2))
