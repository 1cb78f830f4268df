"""GPU: the four models whose user x item grid splits into per-user and per-item tables with no tower of their own --
MatrixFactorization, FFM and LogisticRegression over ``ctr_lowrank_grid_scores`` (csrc/lowrank_grid.hip), Wide & Deep
over ``ctr_widedeep_grid_scores`` (csrc/deepfm_grid.hip) -- through their public interface (``MatrixFactorization.
score_rows / score_grid / recommend``, ``catalogue_scorer`` of the others): against the float64 oracle, against the
per-sample forward, and against their own geometry: a pair's score may not depend on which rows, which order, which tile
or which launch grid it came from.

Parameters.  Default-initialised models are soft (``xavier_normal_`` tables: every dot is about 1e-3, Wide & Deep's h3 is
zero for every pair), so a broken kernel would pass.  Every case is built on the CPU, seeded, and every case with at least
64 pairs asserts on its float64 reference:
  MF    tables ``randn * sqrt(1.5 / sqrt(K))``; score std >= 0.15, doubly centred dot >= 0.25 of the logit's std.
  LR    ``user`` / ``item`` ``randn``, ``linear.weight`` ``randn * 0.3``; score std >= 0.15.
  FFM   the twelve tables ``randn * t`` (t = 0.3 / 0.27 / 0.22 at k = 16 / 32 / 64), ``user`` / ``item`` ``randn * 0.5``,
        ``linear.weight`` ``randn * 0.3`` shifted so that its sum is 1.5 (the reference adds the second-order scalar to
        all 43 dense inputs, which scales it by that sum), bias ``rand - 0.5``; score std >= 0.15, median |logit| <= 3,
        the doubly centred cross part and the user's own part each >= 0.25 of the logit's std.
  W&D   tests/test_gpu_deepfm_grid.py's recipe: tables ``randn * t`` (t = 0.25 / 0.15 / 0.1 at E = 16 / 48 / 128),
        ``user`` / ``item`` ``randn``, biases ``rand - 0.5``, ``linear`` and ``dnn_network`` weights times 3,
        ``output.weight = [[1, 1]]``, the last deep layer calibrated in float64 (scaled by 2 / std(z3), the median taken
        off the bias); score std >= 0.15, h3 > 0 for 40 - 60 % of the pairs, std(h3) >= 0.5, doubly centred h3 std >= 0.3.
Features: age ``rand``, gender and occupation one-hot, genres Bernoulli(0.09); item 1 has no genre.

Shapes (IT items a workgroup, UT users a tile: 128 / 32 for the low-rank kernel, 128 / 16 for Wide & Deep): one pair,
15 / 16 / 17 items, IT - 1 / IT + 1, several item workgroups, one or two users more than one and two user tiles, at every
model's smallest rank; four of them at the script shape (MF 64, FFM 32, Wide & Deep E = 128).  ``row_blocks`` = 1 and 2
are the only way the tile loop and its restaging barrier run at these sizes.

Tolerance: against float64 the project's (grid_cases.RTOL / ATOL on the probability), for the grid and for the
per-sample forward on the same pairs; section 1 prints both as fractions of the bound.  Measured on an MI355X over the
cases of section 1: MF 0.06, FFM 0.08, LR 0.02, Wide & Deep 0.25 (E = 128, (33, 258)) for the grid, 0.03 / 0.05 / 0.02 /
0.39 for the per-sample forward: the forward stays inside the bound everywhere, so the large-logit rule of
tests/test_gpu_afm_grid.py is not used.  The side tables stay below 0.03 of ``linear_fwd``'s tolerance."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
from grid_cases import (ATOL, DEV, RTOL, error_and_frac as _frac, features as _features, frame as _frame,
                        observed as _observed, rank64 as _rank64)
from oracle import ctr_oracle as orc

pytestmark = pytest.mark.gpu
IT = 128
TILE_USERS = {"mf": 32, "ffm": 32, "lr": 32, "wd": 16}    # asserted against the ops constants below
SMALL = {"mf": 16, "ffm": 16, "lr": 0, "wd": 16}          # a model's smallest rank / E (LR has none)
SCRIPT = {"mf": 64, "ffm": 32, "wd": 128}                 # the shapes scripts/*.py run
WD_HIDDEN = (512, 256, 128, 1)
FFM_SCALE = {8: 0.35, 16: 0.3, 32: 0.27, 64: 0.22}
WD_SCALE = {8: 0.35, 16: 0.25, 48: 0.15, 128: 0.1}
# linear_fwd's own tolerance (tests/linear_ref.py FWD_TOL: rtol 1e-5, atol 4e-6 at unit scale) as a relative error
SIDE_TOL = 1e-5 + 4e-6
SEEDS = {}                   # (kind, nu, ni, size): cases whose default seed (5) misses a condition of _assert_hard


def _shapes(kind):
    ut = TILE_USERS[kind]
    return [(1, 1), (5, 15), (5, 16), (5, 17), (3, IT - 1), (3, IT + 1), (33, 2 * IT + 2), (ut + 2, 37), (ut + 1, 20),
            (2 * ut + 1, 20)]


def _script_shapes(kind):
    return [(5, 16), (3, IT + 1), (33, 2 * IT + 2), (TILE_USERS[kind] + 2, 37)]


CASES = [(kind, nu, ni, SMALL[kind]) for kind in ("mf", "ffm", "lr", "wd") for nu, ni in _shapes(kind)]
CASES += [(kind, nu, ni, SCRIPT[kind]) for kind in ("mf", "ffm", "wd") for nu, ni in _script_shapes(kind)]
CASES += [("ffm", 5, 17, 64), ("wd", 5, 17, 48), ("mf", 5, 17, 48)]
KINDS = ("mf", "ffm", "lr", "wd")


def _mod(kind):
    from deeplearningrecommendationsystem_amd.model import ffm, lr, mf, widedeep
    return {"mf": mf, "ffm": ffm, "lr": lr, "wd": widedeep}[kind]


def test_the_tiles_are_the_ones_the_shapes_were_chosen_for():
    from deeplearningrecommendationsystem_amd import ops
    assert ops.LOWRANK_GRID_ITEM_TILE == ops.WIDEDEEP_GRID_ITEM_TILE == IT
    assert ops.LOWRANK_GRID_USER_TILE == TILE_USERS["mf"] == TILE_USERS["ffm"] == TILE_USERS["lr"]
    assert ops.WIDEDEEP_GRID_USER_TILE == TILE_USERS["wd"]


# ------------------------------------------------------------------ the cases: CPU only, float64 reference
def _new(kind, nu, ni, size):
    m = _mod(kind)
    if kind == "mf":
        return m.MatrixFactorization(nu, ni, size)
    if kind == "ffm":
        return m.FFM(43, size, num_users=nu, num_items=ni)
    if kind == "lr":
        return m.LogisticRegression(nu, ni, 43)
    return m.WideDeep(nu, ni, list(size[1]) if isinstance(size, tuple) else list(WD_HIDDEN),
                      size[0] if isinstance(size, tuple) else size)


def _p64(model):
    return {k: v.detach().double() for k, v in model.state_dict().items()}


def _wd_z3(p64, x64):
    """float64 pre-activation of Wide & Deep's last deep layer over the frame"""
    h = F.linear(orc.stack_5e1(p64, x64), p64["linear.weight"], p64["linear.bias"])
    layers = sum(1 for k in p64 if k.startswith("dnn_network.") and k.endswith(".weight"))
    for k in range(layers - 1):
        h = torch.relu(F.linear(h, p64[f"dnn_network.{k}.weight"], p64[f"dnn_network.{k}.bias"]))
    return F.linear(h, p64[f"dnn_network.{layers - 1}.weight"], p64[f"dnn_network.{layers - 1}.bias"]).view(-1)


def _build(kind, nu, ni, size, seed):
    """(model on the CPU with the parameters of the module docstring, user features, item features)"""
    torch.manual_seed(seed)
    model = _new(kind, nu, ni, size)
    gen = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        def fill(t, scale):
            t.copy_(torch.randn(t.shape, generator=gen) * scale)
        if kind == "mf":
            for emb in (model.user_embeddings, model.item_embeddings):
                fill(emb.weight, (1.5 / size ** 0.5) ** 0.5)
        elif kind == "lr":
            fill(model.user.weight, 1.0)
            fill(model.item.weight, 1.0)
            fill(model.linear.weight, 0.3)
        elif kind == "ffm":
            for name in _mod(kind).VECTORS:
                fill(getattr(model, name).weight, FFM_SCALE[size])
            fill(model.user.weight, 0.5)
            fill(model.item.weight, 0.5)
            fill(model.linear.weight, 0.3)
            model.linear.weight.add_((1.5 - float(model.linear.weight.double().sum())) / model.linear.weight.numel())
            model.linear.bias.copy_(torch.rand(model.linear.bias.shape, generator=gen) - 0.5)
        else:
            dim = model.user_embedding.embedding_dim
            for emb in (model.user_embedding, model.item_embedding, model.gender_embedding, model.occupation_embedding,
                        model.movie_embedding):
                fill(emb.weight, WD_SCALE[dim])
            fill(model.user.weight, 1.0)
            fill(model.item.weight, 1.0)
            for lin in [model.linear, model.wide, model.output] + list(model.dnn_network):
                lin.bias.copy_(torch.rand(lin.bias.shape, generator=gen) - 0.5)
            for lin in [model.linear] + list(model.dnn_network):
                lin.weight.mul_(3.0)
            model.output.weight.copy_(torch.tensor([[1.0, 1.0]]))
        uf, itf = _features(nu, ni, gen)
        if kind == "wd":
            # the last deep layer, calibrated in float64 over the case's own grid
            x64 = _frame(uf, itf).double()
            last = model.dnn_network[len(model.dnn_network) - 1]
            z3 = _wd_z3(_p64(model), x64)
            scale = 2.0 / float(z3.std()) if z3.numel() > 1 and float(z3.std()) > 0 else 1.0
            last.weight.mul_(scale)
            last.bias.mul_(scale)
            last.bias.sub_(float(_wd_z3(_p64(model), x64).median()))
    return model, uf, itf


def _centred(m):
    return m - m.mean(0, keepdim=True) - m.mean(1, keepdim=True) + m.mean()


def _reference(kind, model, uf, itf):
    """float64 (scores (nu, ni) numpy, the pieces the conditions and the side tables are checked on)"""
    nu, ni = uf.shape[0], itf.shape[0]
    p64, x64 = _p64(model), _frame(uf, itf).double()
    uid, iid = orc.ids_from_float(x64[:, orc.COL_USER]), orc.ids_from_float(x64[:, orc.COL_ITEM])
    grid = lambda v: v.view(nu, ni, *v.shape[1:])  # noqa: E731
    parts = {}
    with torch.no_grad():
        if kind == "mf":
            scores = orc.mf_forward(p64, uid, iid).view(nu, ni)
            parts["dot"] = p64["user_embeddings.weight"] @ p64["item_embeddings.weight"].T
            parts["logit"] = parts["dot"]
        elif kind == "lr":
            scores = orc.lr_forward(p64, x64).view(nu, ni)
            w = p64["linear.weight"][0]
            parts["a"] = grid(p64["user.weight"][uid, 0] + x64[:, 2:26] @ w[:24] + p64["linear.bias"][0])[:, 0]
            parts["b"] = grid(p64["item.weight"][iid, 0] + x64[:, 26:] @ w[24:])[0]
            parts["logit"] = parts["a"][:, None] + parts["b"][None, :]
        elif kind == "ffm":
            scores = orc.ffm_forward(p64, x64).view(nu, ni)
            v = orc.ffm_vectors(p64, x64)
            w = p64["linear.weight"][0]
            sw = w.sum()
            dot = lambda a, b: (v[a] * v[b]).sum(1)  # noqa: E731
            own_u = sum(dot(a, b) for a, b in orc.FFM_PAIRS if "movie" not in a + b and "itemid" not in a + b)
            own_i = dot("movie_item", "itemid_item")
            A = v["age_item"] + v["gender_item"] + v["occupation_item"] + v["userid_item"]
            B = v["movie_user"] + v["itemid_user"]
            parts["cu"], parts["ci"] = grid(sw * A)[:, 0], grid(B)[0]
            parts["a"] = grid(p64["user.weight"][uid, 0] + x64[:, 2:26] @ w[:24] + p64["linear.bias"][0] + sw * own_u)[:, 0]
            parts["b"] = grid(p64["item.weight"][iid, 0] + x64[:, 26:] @ w[24:] + sw * own_i)[0]
            parts["cross"] = parts["cu"] @ parts["ci"].T
            parts["own_u"] = grid(sw * own_u)[:, 0]
            parts["logit"] = parts["a"][:, None] + parts["b"][None, :] + parts["cross"]
        else:
            scores = orc.widedeep_forward(p64, x64).view(nu, ni)
            e = p64["user_embedding.weight"].shape[1]
            stack = orc.stack_5e1(p64, x64)
            user_cols = torch.zeros(5 * e + 1, dtype=torch.bool)
            user_cols[:e] = True
            user_cols[2 * e:4 * e + 1] = True
            w0, b0 = p64["linear.weight"], p64["linear.bias"]
            w1, b1 = p64["dnn_network.0.weight"], p64["dnn_network.0.bias"]
            parts["zu"] = grid(F.linear(F.linear(stack * user_cols, w0), w1))[:, 0]
            parts["zi"] = grid(F.linear(F.linear(stack * ~user_cols, w0, b0), w1, b1))[0]
            w = p64["wide.weight"][0]
            parts["a"] = grid(p64["user.weight"][uid, 0] + x64[:, 2:26] @ w[:24])[:, 0]
            parts["b"] = grid(p64["item.weight"][iid, 0] + x64[:, 26:] @ w[24:] + p64["wide.bias"][0])[0]
            parts["h3"] = torch.relu(_wd_z3(p64, x64)).view(nu, ni)
            out_w, out_b = p64["output.weight"][0], p64["output.bias"][0]
            parts["logit"] = out_w[0] * (parts["a"][:, None] + parts["b"][None, :]) + out_w[1] * parts["h3"] + out_b
        # the split the scorers are built on, restated in float64: it must be the oracle's model
        assert torch.allclose(torch.sigmoid(parts["logit"]), scores, rtol=0, atol=1e-12), kind
    return scores.numpy(), parts


def _assert_hard(kind, scores, parts, what):
    """the conditions of the module docstring"""
    if scores.size < 64:
        return
    logit_std = float(parts["logit"].std())
    assert scores.std() >= 0.15, f"{what}: soft parameters, the scores' standard deviation is {scores.std():.3f}"
    if kind == "mf":
        ratio = float(_centred(parts["dot"]).std()) / logit_std
        print(f"{what}: score std {scores.std():.3f}, centred dot {ratio:.2f} of the logit's std")
        assert ratio >= 0.25, f"{what}: the centred dot has {ratio:.3f} of the logit's standard deviation"
    elif kind == "ffm":
        median = float(parts["logit"].abs().median())
        cross, own = float(_centred(parts["cross"]).std()) / logit_std, float(parts["own_u"].std()) / logit_std
        print(f"{what}: score std {scores.std():.3f}, median |logit| {median:.2f}, cross share {cross:.2f}, own share "
              f"{own:.2f}")
        assert median <= 3.0, f"{what}: the median |logit| is {median:.2f}"
        assert cross >= 0.25, f"{what}: the centred cross part has {cross:.3f} of the logit's standard deviation"
        assert own >= 0.25, f"{what}: the user's own part has {own:.3f} of the logit's standard deviation"
    elif kind == "wd":
        h3 = parts["h3"]
        live, centred = float((h3 > 0).double().mean()), float(_centred(h3).std())
        print(f"{what}: score std {scores.std():.3f}, h3 > 0 at {live:.2f}, std(h3) {float(h3.std()):.2f}, centred "
              f"{centred:.2f}")
        assert 0.4 <= live <= 0.6, f"{what}: h3 > 0 for {live:.2f} of the pairs"
        assert float(h3.std()) >= 0.5, f"{what}: std(h3) = {float(h3.std()):.3f}"
        assert centred >= 0.3, f"{what}: the doubly centred h3 has std {centred:.3f}"
    else:
        print(f"{what}: score std {scores.std():.3f}")


@functools.lru_cache(maxsize=None)
def _cpu_case(kind, nu, ni, size):
    """(model on the CPU, user features, item features, float64 scores, float64 parts), made once and shared: no test
    changes it"""
    model, uf, itf = _build(kind, nu, ni, size, SEEDS.get((kind, nu, ni, size), 5) + 31 * nu + ni + (
        size if isinstance(size, int) else size[0]))
    scores, parts = _reference(kind, model, uf, itf)
    _assert_hard(kind, scores, parts, f"{kind} ({nu}, {ni}) size {size}")
    return model, uf, itf, scores, parts


def _on_device(kind, cpu, nu, ni, size):
    model = _new(kind, nu, ni, size)
    model.load_state_dict(cpu.state_dict())
    return model.to(DEV).eval()


def _scorer(kind, model, uf, itf):
    """what scores the model: ``catalogue_scorer`` over the side features, or (MF) the scorer behind the model's methods"""
    from deeplearningrecommendationsystem_amd.data import FeatureAssembler
    if kind == "mf":
        return _mod(kind)._GridScorer(model)
    return model.catalogue_scorer(FeatureAssembler(uf.to(DEV), itf.to(DEV)))


@functools.lru_cache(maxsize=None)
def _case(kind, nu, ni, size):
    """(model on the device, scorer, float64 scores)"""
    cpu, uf, itf, scores, _ = _cpu_case(kind, nu, ni, size)
    model = _on_device(kind, cpu, nu, ni, size)
    return model, _scorer(kind, model, uf, itf), scores


def _forward_pairs(kind, model, scorer, nu, ni):
    users = torch.arange(nu, device=DEV).repeat_interleave(ni)
    items = torch.arange(ni, device=DEV).repeat(nu)
    with torch.no_grad():
        if kind == "mf":
            return model(users, items).view(nu, ni)
        return model(scorer.assembler.feature(users, items)).view(nu, ni)


def _geometry_cases():
    out = []
    for kind in KINDS:
        ut = TILE_USERS[kind]
        out += [(kind, 33, 2 * IT + 2, SMALL[kind]), (kind, ut + 2, 37, SMALL[kind]), (kind, 2 * ut + 1, 20, SMALL[kind])]
        if kind in SCRIPT:
            out.append((kind, ut + 2, 37, SCRIPT[kind]))
    return out


# ------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("kind,nu,ni,size", CASES)
def test_score_grid_matches_the_float64_oracle(kind, nu, ni, size):
    model, scorer, scores64 = _case(kind, nu, ni, size)
    assert scorer.path == "grid" and type(scorer) is _mod(kind)._GridScorer
    got = scorer.score_grid()
    assert got.shape == (nu, ni) and got.dtype == torch.float32 and got.is_contiguous()
    err, frac = _frac(got, scores64)
    forward = _frac(_forward_pairs(kind, model, scorer, nu, ni), scores64)[1]
    print(f"{kind} ({nu}, {ni}) size {size}: max |error| {err:.3e}, max error / (atol + rtol |ref|) {frac:.3f}; the "
          f"per-sample forward {forward:.3f}")
    torch.testing.assert_close(got.cpu().double(), torch.from_numpy(scores64), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("kind,nu,ni,size", [("ffm", 33, 2 * IT + 2, 16), ("ffm", 34, 37, 32), ("wd", 33, 2 * IT + 2, 16),
                                             ("wd", 18, 37, 128), ("lr", 33, 2 * IT + 2, 0)])
def test_the_side_tables_match_their_float64_values(kind, nu, ni, size):
    """locates a failure of the final comparison: each table's worst error relative to its largest entry, within
    linear_fwd's own tolerance"""
    model, scorer, _ = _case(kind, nu, ni, size)
    parts = _cpu_case(kind, nu, ni, size)[4]
    with torch.no_grad():
        shared = scorer._shared()
    if kind == "lr":
        got = dict(zip(("a", "b"), shared))
    elif kind == "ffm":
        _, (cu, a), (ci, b) = shared
        assert cu.shape == (nu, size) and ci.shape == (ni, size)
        got = {"cu": cu, "a": a, "ci": ci, "b": b}
    else:
        _, (zu, a), (zi, b) = shared
        assert zu.shape == (nu, 256) and zi.shape == (ni, 256)
        got = {"zu": zu, "a": a, "zi": zi, "b": b}
    for name, value in got.items():
        ref = parts[name]
        assert value.shape == ref.shape, name
        err = float((value.cpu().double() - ref).abs().max()) / float(ref.abs().max())
        print(f"{kind} ({nu}, {ni}) size {size}: {name} relative error {err:.3e} ({err / SIDE_TOL:.3f} of linear_fwd's "
              f"tolerance)")
        assert err <= SIDE_TOL, name


# ------------------------------------------------------------------ 2. geometry independence, bitwise
@pytest.mark.parametrize("kind,nu,ni,size", _geometry_cases())
def test_a_score_does_not_depend_on_the_rows_asked_for(kind, nu, ni, size):
    model, scorer, _ = _case(kind, nu, ni, size)
    ut = TILE_USERS[kind]
    full = scorer.score_grid()
    assert torch.equal(scorer.score_grid(), full)                             # run to run
    assert torch.equal(scorer.score_grid([3, 1, 3, 0]), full[[3, 1, 3, 0]])
    assert torch.equal(scorer.score_grid(torch.arange(nu - 1, -1, -1)), full.flip(0))
    ranges = [(0, nu), (0, 1), (2, 2), (nu - 1, nu), (1, nu - 1), (ut - 1, ut + 1), (ut, nu), (1, ut + 1), (ut - 5, nu)]
    for s, e in ranges:
        rows = scorer.score_rows(s, e)
        assert rows.shape == (e - s, ni) and rows.is_contiguous()
        assert torch.equal(rows, full[s:e]), (s, e)
        assert torch.equal(scorer(s, e), rows)


@pytest.mark.parametrize("kind", KINDS)
def test_a_score_does_not_depend_on_the_items_position(kind):
    from deeplearningrecommendationsystem_amd.data import FeatureAssembler
    nu, ni, size = 33, 2 * IT + 2, SMALL[kind]
    model_a, scorer_a, _ = _case(kind, nu, ni, size)
    perm = torch.randperm(ni, generator=torch.Generator().manual_seed(2)).to(DEV)
    model_b = _on_device(kind, _cpu_case(kind, nu, ni, size)[0], nu, ni, size)
    by_item = {"mf": ("item_embeddings",), "lr": ("item",), "wd": ("item_embedding", "item"),
               "ffm": ("itemid_user", "itemid_item", "item")}[kind]
    with torch.no_grad():
        for name in by_item:
            getattr(model_b, name).weight.copy_(getattr(model_a, name).weight[perm])
    if kind == "mf":
        scorer_b = _scorer(kind, model_b, None, None)
    else:
        asm = scorer_a.assembler
        scorer_b = model_b.catalogue_scorer(FeatureAssembler(asm.user_features, asm.item_features[perm]))
    assert torch.equal(scorer_b.score_grid(), scorer_a.score_grid()[:, perm])


@pytest.mark.parametrize("kind,nu,ni,size", [c for c in _geometry_cases() if c[2] != 2 * IT + 2])
def test_a_score_does_not_depend_on_the_launch_geometry(kind, nu, ni, size):
    """row_blocks = 1: one workgroup per item tile walks every user tile (the tile loop and its restaging barrier);
    2: two workgroups share them; 0: the launch's own choice"""
    model, scorer, _ = _case(kind, nu, ni, size)
    own = scorer.score_grid()
    users = torch.arange(nu - 1, -1, -1)
    try:
        for blocks in (1, 2):
            scorer.row_blocks = blocks
            assert torch.equal(scorer.score_grid(), own), blocks
            assert torch.equal(scorer.score_rows(1, nu), own[1:]), blocks
            assert torch.equal(scorer.score_grid(users), own.flip(0)), blocks
    finally:
        scorer.__dict__.pop("row_blocks", None)


# ------------------------------------------------------------------ 3. against the per-sample forward
@pytest.mark.parametrize("kind,nu,ni,size", [(k, 33, 2 * IT + 2, SMALL[k]) for k in KINDS]
                         + [(k, 5, 17, SMALL[k]) for k in KINDS] + [(k, 33, 2 * IT + 2, SCRIPT[k]) for k in SCRIPT])
def test_score_grid_matches_the_per_sample_forward(kind, nu, ni, size):
    model, scorer, scores64 = _case(kind, nu, ni, size)
    want = _forward_pairs(kind, model, scorer, nu, ni)
    got = scorer.score_grid()
    print(f"{kind} ({nu}, {ni}) size {size}: {int((got != want).sum())} of {got.numel()} scores differ bitwise, max "
          f"|difference| {float((got - want).abs().max()):.3e}; against float64: grid {_frac(got, scores64)[1]:.3f}, "
          f"forward {_frac(want, scores64)[1]:.3f} of the tolerance")
    torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL)


def test_matrix_factorization_scores_through_its_own_methods():
    """the public interface of the one model that owns its scorer: every call makes a fresh one"""
    nu, ni = 34, 37
    model, scorer, scores64 = _case("mf", nu, ni, 16)
    full = model.score_grid()
    assert torch.equal(full, scorer.score_grid())
    torch.testing.assert_close(full.cpu().double(), torch.from_numpy(scores64), rtol=RTOL, atol=ATOL)
    assert torch.equal(model.score_rows(3, 33), full[3:33]) and torch.equal(model.score_grid([4, 4, 0]), full[[4, 4, 0]])
    observed, _ = _observed(nu, ni)
    assert torch.equal(model.recommend(n=5, exclude=observed), scorer.recommend(n=5, exclude=observed))
    assert torch.equal(model.recommend([7, 2], n=3), scorer.recommend([7, 2], n=3))


# ------------------------------------------------------------------ 5. recommend
def _own_ranking(scorer, users, n, observed):
    """topk_rows of the scorer's own scores after rank_mask, -1 where the survivors run out"""
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.topn import excluded_rows
    ni = scorer.num_items
    scores = scorer.score_grid(users)
    left = torch.full((scores.shape[0],), ni, dtype=torch.int64, device=DEV)
    if observed is not None:
        off, ids = excluded_rows(observed, users)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.rank_mask(scores, off, ids, err)
        assert int(err.item()) == 0
        left -= off.diff()
    take = min(n, ni)
    want = torch.full((scores.shape[0], n), -1, dtype=torch.int64, device=DEV)
    want[:, :take] = ops.topk_rows(scores, take)
    want[torch.arange(n, device=DEV)[None, :] >= left[:, None]] = -1
    return want


@pytest.mark.parametrize("excluded", [False, True], ids=["all-items", "observed-left-out"])
@pytest.mark.parametrize("kind", KINDS)
def test_recommend_is_the_ranking_of_the_kernels_scores(kind, excluded):
    nu, ni = 33, 2 * IT + 2
    model, scorer, scores64 = _case(kind, nu, ni, SMALL[kind])
    observed, seen = _observed(nu, ni) if excluded else (None, np.zeros((nu, ni), dtype=bool))
    want64 = _rank64(scores64, ~seen)
    left = (~seen).sum(axis=1)
    for n in (1, 5, ni, ni + 3):
        got = scorer.recommend(n=n, exclude=observed)
        assert got.shape == (nu, n) and got.dtype == torch.int64
        assert torch.equal(got, _own_ranking(scorer, torch.arange(nu, device=DEV), n, observed)), n
        got = got.cpu().numpy()
        for u in range(nu):                     # every user: the columns the row fills, then nothing but -1
            m = min(n, int(left[u]))
            assert (got[u, m:] == -1).all() and (got[u, :m] >= 0).all(), (n, u)
            assert not seen[u, got[u, :m]].any(), f"n = {n}, user {u}: an excluded item is recommended"
            gu.assert_same_ranking(got[u:u + 1, :m], want64[u:u + 1, :m], scores64[u:u + 1], tol=1e-5)
        if excluded:
            assert (got[0] == -1).all() and set(got[1, :min(n, 2)]) <= {2, ni - 1}


@pytest.mark.parametrize("kind", KINDS)
def test_recommend_for_a_user_list_in_chunks(kind, monkeypatch):
    ut = TILE_USERS[kind]
    nu, ni = 2 * ut + 1, 20
    model, scorer, scores64 = _case(kind, nu, ni, SMALL[kind])
    observed, seen = _observed(nu, ni, seed=9)
    users = torch.tensor([nu - 1, 0, 7, 7, ut, 1, ut - 1] + list(range(3, nu)))
    whole = scorer.recommend(users, n=6, exclude=observed)
    assert torch.equal(whole, scorer.recommend(n=6, exclude=observed)[users.to(DEV)])
    from deeplearningrecommendationsystem_amd import topn
    monkeypatch.setattr(topn, "SCORE_CHUNK_FLOATS", 5 * ni)                  # five users at a time
    assert torch.equal(scorer.recommend(users, n=6, exclude=observed), whole)
    assert torch.equal(scorer.recommend(users.tolist(), n=6, exclude=None), scorer.recommend(users, n=6))


# ------------------------------------------------------------------ 6. ranking_metrics, and nothing is left behind
@pytest.mark.parametrize("kind", KINDS)
def test_ranking_metrics_over_the_scorer_and_the_model_is_untouched(kind):
    from deeplearningrecommendationsystem_amd.evaluator import ranking
    nu, ni = 33, 2 * IT + 2
    model, scorer, _ = _case(kind, nu, ni, SMALL[kind])
    before = {k: v.clone() for k, v in model.state_dict().items()}
    training = model.training
    gen = torch.Generator().manual_seed(11)
    pick = torch.rand((nu, ni), generator=gen)
    train = tuple(t.to(DEV) for t in (pick < 0.3).nonzero(as_tuple=True))
    held = pick > 0.9
    held[torch.arange(nu), pick.argmax(dim=1)] = True                             # no empty actual row
    real = tuple(t.to(DEV) for t in held.nonzero(as_tuple=True))
    grid = scorer.score_grid()
    keep = grid.clone()
    a = ranking.ranking_metrics(scorer if kind != "mf" else model.score_rows, real, 10, exclude=(train,), num_users=nu,
                                chunk=7)
    b = ranking.ranking_metrics(grid, real, 10, exclude=(train,), num_users=nu, chunk=7)
    assert np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True), (a, b)
    assert 0.0 < a.precision <= 1.0
    assert torch.equal(grid, keep)
    observed, _ = _observed(nu, ni)
    scorer.recommend(n=5, exclude=observed)
    scorer.score_rows(3, 9)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed"
    assert model.training == training
    assert all(p.grad is None for p in model.parameters())


# ------------------------------------------------------------------ 7. a scorer is never stale
@pytest.mark.parametrize("kind", KINDS)
def test_a_scorer_is_never_stale(kind):
    """the weights are read at every call: a scorer made before a parameter changed scores the new parameters -- a table
    row, a wide weight and (Wide & Deep) tower weights on either side of the split"""
    nu, ni, size = 5, 17, SMALL[kind]
    cpu, uf, itf = _cpu_case(kind, nu, ni, size)[:3]
    model = _on_device(kind, cpu, nu, ni, size)
    scorer = _scorer(kind, model, uf, itf)
    last = scorer.score_grid()
    changes = {
        "mf": (lambda: model.user_embeddings.weight[2].add_(0.5), lambda: model.item_embeddings.weight[16].add_(0.5)),
        "lr": (lambda: model.user.weight[2].add_(0.5), lambda: model.linear.weight[0, 0].add_(0.25),
               lambda: model.linear.bias.add_(0.25)),
        "ffm": (lambda: model.userid_item.weight[2].add_(0.5), lambda: model.gender_user.weight[:].add_(0.25),
                lambda: model.linear.weight[0, 0].add_(0.25), lambda: model.item.weight[16].add_(0.5)),
        "wd": (lambda: model.user_embedding.weight[2].add_(0.5), lambda: model.wide.weight[0, 0].add_(0.25),
               lambda: model.linear.weight[7:40].add_(0.25), lambda: model.dnn_network[1].weight[3:90].add_(0.05),
               lambda: model.dnn_network[2].weight.mul_(1.25), lambda: model.output.bias.add_(0.25)),
    }[kind]
    for change in changes:
        with torch.no_grad():
            change()
        new = scorer.score_grid()
        assert not torch.equal(new, last)
        assert torch.equal(new, _scorer(kind, model, uf, itf).score_grid())
        torch.testing.assert_close(new, _forward_pairs(kind, model, scorer, nu, ni), rtol=RTOL, atol=ATOL)
        last = new


def test_matrix_factorization_passes_its_tables_themselves():
    """no copy: the kernel reads the weight tables where they are"""
    model, scorer, _ = _case("mf", 5, 17, 16)
    cu, ci = scorer._shared()
    assert cu.data_ptr() == model.user_embeddings.weight.data_ptr()
    assert ci.data_ptr() == model.item_embeddings.weight.data_ptr()


# ------------------------------------------------------------------ 8. errors
@pytest.mark.parametrize("kind", KINDS)
def test_errors(kind):
    from deeplearningrecommendationsystem_amd.data import FeatureAssembler, ObservedPairs
    nu, ni = 5, 17
    model, scorer, _ = _case(kind, nu, ni, SMALL[kind])
    assert scorer.path == "grid"
    for bad in ([nu], [-1], [0, 1, nu + 3]):
        with pytest.raises(IndexError):
            scorer.score_grid(bad)
        with pytest.raises(IndexError):
            scorer.recommend(bad, n=3)
    for s, e in ((-1, 2), (2, nu + 1), (3, 2)):
        with pytest.raises(IndexError):
            scorer.score_rows(s, e)
    with pytest.raises(ValueError):
        scorer.recommend(n=0)
    pairs = torch.zeros(1, dtype=torch.int64, device=DEV)
    for shape in ((nu + 1, ni), (nu, ni - 1)):
        with pytest.raises(ValueError):
            scorer.recommend(n=3, exclude=ObservedPairs(pairs, pairs, *shape))
    if kind != "mf":
        asm = scorer.assembler
        for users, items in ((asm.user_features[:-1], asm.item_features), (asm.user_features, asm.item_features[1:])):
            with pytest.raises(ValueError):
                model.catalogue_scorer(FeatureAssembler(users, items))
    assert scorer.score_grid([]).shape == (0, ni) and scorer.recommend([], n=3).shape == (0, 3)
    assert scorer.score_rows(2, 2).shape == (0, ni)


# ------------------------------------------------------------------ 9. the forward path of the shapes the kernels refuse
@pytest.mark.parametrize("kind,size", [("mf", 20), ("ffm", 8), ("wd", (8, (512, 128, 128, 1)))])
def test_a_shape_without_a_grid_kernel_takes_the_forward_path(kind, size, monkeypatch):
    """the same contract from the per-sample forward, in chunks that do not divide the grid"""
    nu, ni = 18, 37
    model, scorer, scores64 = _case(kind, nu, ni, size)
    from deeplearningrecommendationsystem_amd.model import _base
    assert scorer.path == "forward" and (kind == "mf" or type(scorer) is _base.CatalogueScorer)
    monkeypatch.setattr(_base, "FORWARD_GRID_PAIRS", 100)
    monkeypatch.setattr(_mod("mf"), "_FORWARD_CHUNK", 100)
    got = scorer.score_grid()
    torch.testing.assert_close(got, _forward_pairs(kind, model, scorer, nu, ni), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(got.cpu().double(), torch.from_numpy(scores64), rtol=RTOL, atol=ATOL)
    assert torch.equal(scorer.score_rows(3, 17), got[3:17]) and torch.equal(scorer.score_grid([5, 5, 0]), got[[5, 5, 0]])
    observed, seen = _observed(nu, ni)
    rec = scorer.recommend(n=4, exclude=observed)
    assert torch.equal(rec, _own_ranking(scorer, torch.arange(nu, device=DEV), 4, observed))
