"""CPU only.  tests/mlp_ref.py against autograd, its plan() against the text of csrc/mlp_fused.hip, its case tables
against plan(), and its comparisons against small mutations of the reference: what tests/test_gpu_mlp_arms.py trusts,
checked without a GPU.

* the float64 references equal float64 autograd of linear + activation layers and a head on top;
* the constants plan() restates (kWaves, kMaxDim, kMaxLayers, kHeadMax, kSlack, the N / K / ACT arrays of the pinned
  shapes) are read out of the kernel source: if they move, this fails here and not on the GPU;
* every case is admitted by plan() and has the property it names; every arm class of REQUIRED_ARMS is claimed by some
  case (the table is printed), every refusal is planned with the code the table gives;
* the enumeration for the flush's single-copy arm: not reachable under the 160 KB cap and 16 tiles (printed);
* negative controls: every mutation, rounded to float32 like a kernel's output, is rejected by the comparison the GPU
  test applies, at EVERY case it changes anything at; the unmutated float32 image passes."""
import itertools
import os

import pytest
import torch

import mlp_ref as ref

TIGHT = dict(rtol=1e-11, atol=1e-12)
SOURCE = os.path.join(os.path.dirname(__file__), "..", "deeplearningrecommendationsystem_amd", "csrc", "mlp_fused.hip")
_cache = {}


def _case(c):
    """operands and the float64 results, computed once per case (one large case in memory at a time)"""
    if c.name not in _cache:
        _cache.clear()
        ops_ = ref.operands(c)
        _cache[c.name] = (ops_, ref.fwd_reference(c, ops_), ref.bwd_reference(c, ops_))
    return _cache[c.name]


def test_the_references_equal_autograd():
    c = ref.Case("autograd", [8, 24, 16, 5], [ref.R, ref.S, ref.N], 37, "", nobias=(1,), head_p=8, ldx_pad=8, xoff=4,
                 last_pad=1, last_off=1)
    ops_ = ref.operands(c)
    x = ref.get(ops_, "x").double().requires_grad_(True)
    ws = [ref.get(ops_, f"w{i}").double().requires_grad_(True) for i in range(3)]
    bs = [ref.get(ops_, f"b{i}").double().reshape(-1).requires_grad_(True) for i in range(3)]
    h, ys = x, []
    for i in range(3):
        z = torch.nn.functional.linear(h, ws[i], None if i in c.nobias else bs[i])
        h = [z, torch.relu(z), torch.sigmoid(z)][c.acts[i]]
        ys.append(h)
    hw = ref.get(ops_, "hw").double().reshape(-1)
    out = torch.sigmoid(torch.cat([ref.get(ops_, "xe").double(), h], 1) @ hw + ref.get(ops_, "hc").double().reshape(()))
    want = ref.fwd_reference(c, ops_)
    for a, b in zip(want["ys"], ys):
        torch.testing.assert_close(a, b.detach(), **TIGHT)
    torch.testing.assert_close(want["out"], out.detach().reshape(-1, 1), **TIGHT)
    # the backward reads the float32 image of y: give autograd the same saved outputs by comparing at float32 accuracy
    h.backward(ref.get(ops_, "gy").double())
    got = ref.bwd_reference(c, ops_)
    loose = dict(rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(got["gx"], x.grad, **loose)
    for i in range(3):
        torch.testing.assert_close(got["gw"][i] - ref.get(ops_, f"gw{i}").double(), ws[i].grad, **loose)
        if i not in c.nobias:
            torch.testing.assert_close(got["gb"][i] - ref.get(ops_, f"gb{i}").double().reshape(-1), bs[i].grad, **loose)


def test_the_plan_constants_are_those_of_the_kernel_source():
    with open(SOURCE) as f:
        k = ref.source_constants(f.read())
    assert (k["kWaves"], k["kMaxDim"], k["kMaxLayers"], k["kHeadMax"], k["kSlack"]) == (
        ref.K_WAVES, ref.K_MAX_DIM, ref.K_MAX_LAYERS, ref.K_HEAD_MAX, ref.K_SLACK)
    for shape, (n, kk, act, _) in ref.PINNED.items():
        assert k[shape] == (n, kk, act), shape
    assert ref.NCF[1:] == list(ref.PINNED["NcfShape"][0]) and ref.NCF[:-1] == list(ref.PINNED["NcfShape"][1])
    assert ref.NCF_TOWER[1:] == list(ref.PINNED["NcfTowerShape"][0]) and ref.DIEN_ATT[1:] == list(ref.PINNED["DienAttShape"][0])


def test_each_case_has_the_property_it_names():
    names = [c.name for c in ref.STACK_CASES + ref.HEAD_CASES] + [r.name for r in ref.REFUSALS]
    assert len(set(names)) == len(names)
    by = {c.name: c for c in ref.STACK_CASES + ref.HEAD_CASES}
    for c in by.values():
        assert c.plan(False).code == ref.CTR_OK and (c.head_p is not None or c.plan(True).code == ref.CTR_OK), c.name
        assert len(c.acts) == c.nl and c.ldy_pad % 4 == 0 and c.ldx_pad % 4 == 0 and c.xoff % 4 == 0, c.name
    a = by["A_m37"].plan(True)
    assert (a.maxt, a.acc_off, a.ntiles) == (8, [0, 1, 3, 5], 6)
    assert a.pair_roles == [{"A"}, {"A", "B"}, {"A", "B"}, {"B"}]        # every pair (s2, s2 + 1) holds two layers
    assert a.dx_rem == ["<=24", "0", "<=16", "<=8"] and by["A_m37"].plan(False).k_rem == [8, 24, 0, 16]
    for name in ("A_second_tile", "G_tower_second_tile", "H_dien_grid512", "head_A_p8_ldout3_second_tile"):
        assert by[name].plan(False).second_tile and by[name].m % 32, name
    b = by["B_one_tile_wide"].plan(True)
    assert b.maxt == 8 and b.two_rows_one_pair == [True, False] and b.dx_rem[1] == ">24"
    cf = by["C_stride34"].plan(False)
    assert (cf.sa, cf.sb) == (34, 20) and cf.odd_stride and not by["C_stride34"].plan(True).odd_stride
    assert by["D_maxt12"].plan(True).maxt == 12 and by["D_maxt12"].plan(True).pinned is None
    e = by["E_copies2"].plan(True)
    assert e.copies == [2, 4] and e.maxt == 16 and 0 <= ref.LDS_CAP - e.lds_bytes - ref.STACK_DESC_BYTES < 4096
    assert e.grid == 4 and by["E_copies2"].m > 3 * 128              # every wave of the first workgroups adds 3 tiles
    g = by["G_tower_second_tile"].plan(True)
    assert (g.pinned, g.maxt, g.cap, g.gvec) == ("NcfTowerShape", 12, 256, True)
    h = by["H_dien_grid512"].plan(True)
    assert (h.pinned, h.maxt, h.cap, h.grid, h.extent) == ("DienAttShape", 6, 512, 512, 512 * 4225)
    assert by["H_dien_m100"].plan(True).extent == 4225
    assert [by[n].plan(True).gvec for n in ("I_ncf_ldgy65", "I_ncf_gy_off1", "I_ncf_gvec")] == [False, False, True]
    assert by["J_maxt14"].plan(True).maxt == 14 and by["J_maxt16"].plan(True).maxt == 16
    assert by["J_maxt16"].plan(True).acc_off == [0, 8, 12, 14] and by["J_maxt16"].plan(True).ntiles == 16
    assert by["head_ncf_is_generic"].plan(False).pinned is None
    f, fb = ref.plan(ref.F_DIMS, ref.F_ACTS, False, ref.F_M), ref.plan(ref.F_DIMS, ref.F_ACTS, True, ref.F_M)
    assert f.code == ref.CTR_OK and fb.code == ref.CTR_ELIMIT and fb.ntiles == 18
    assert fb.lds_bytes + ref.STACK_DESC_BYTES <= ref.LDS_CAP       # refused for its tiles, not for its LDS
    n128 = ref.plan([128, 128, 8], [ref.R, ref.N], False, ref.F_M)
    assert n128.code == ref.CTR_ELIMIT and n128.lds_bytes > ref.LDS_CAP


def test_every_arm_class_has_a_case():
    arms = ref.arms_claimed()
    for arm in sorted(arms):
        print(f"{arm:40s} {', '.join(arms[arm])}")
    missing = [arm for arm in ref.REQUIRED_ARMS if arm not in arms]
    assert not missing, f"no case claims: {missing}"


@pytest.mark.parametrize("r", ref.REFUSALS, ids=lambda r: r.name)
def test_every_refusal_is_planned_with_its_code(r):
    assert r.plan().code == r.code
    # and the same stack without the defect is admitted (the defect is what is refused)
    if r.tweak and r.tweak != "ws_short":
        assert ref.plan(r.dims, r.acts(), r.entry == "bwd", r.m, head_p=r.head_p).code == ref.CTR_OK


def test_the_flush_never_runs_with_a_single_copy():
    """all admissible 1- to 3-layer stacks with widths in multiples of 8 up to 128"""
    widths = range(8, 129, 8)
    seen = {4: 0, 2: 0, 1: 0}
    example = {}
    for nl in (1, 2, 3):
        for dims in itertools.product(widths, repeat=nl + 1):
            p = ref.plan(list(dims), [ref.R] * nl, True, 1 << 20)
            if p.code != ref.CTR_OK:
                continue
            for cp in p.copies:
                seen[cp] += 1
                example.setdefault(cp, dims)
    print(f"layers flushed with 4 / 2 / 1 copies: {seen[4]} / {seen[2]} / {seen[1]}; first stack with 2: {example.get(2)}")
    assert seen[1] == 0 and seen[2] > 0 and seen[4] > 0


def _f32(t):
    return None if t is None else t.float()


@pytest.mark.parametrize("c", ref.FWD_CASES + ref.HEAD_CASES, ids=lambda c: c.name)
def test_the_forward_comparison_passes_the_reference_and_rejects_every_mutation(c):
    ops_, want, _ = _case(c)
    ref.check_fwd(c, ops_, [y.float() for y in want["ys"]], _f32(want["out"]), want)
    applied = 0
    for mutate in ref.FWD_MUTATIONS:
        li = ref.fwd_mutation_layer(c, mutate)
        if li is None:
            continue
        applied += 1
        if mutate == "ragged_row_written":               # row m of the last output: the row behind the ragged tile
            view = c.views()[f"y{li}"]
            buf = ref.blank(view)
            ref.check_gaps(buf, view, f"{c.name} y{li} buffer")
            buf[view.off + c.m * view.ld] = 0.0
            assert ref.rejects(ref.check_gaps, buf, view, "mutated"), f"{c.name}: '{mutate}' passed"
            continue
        ys, out = ref.fwd_mutated(c, ops_, want, mutate)
        assert ref.rejects(ref.check_fwd, c, ops_, ys, out, want), f"{c.name}: '{mutate}' passed the comparison"
    assert applied >= 2


@pytest.mark.parametrize("c", ref.BWD_CASES, ids=lambda c: c.name)
def test_the_backward_comparison_passes_the_reference_and_rejects_every_mutation(c):
    ops_, _, want = _case(c)
    f32 = lambda d: {"gx": _f32(d["gx"]), "gw": [t.float() for t in d["gw"]], "gb": [t.float() for t in d["gb"]]}  # noqa: E731
    ref.check_bwd(c, f32(want), want)
    applied = 0
    for mutate in ref.BWD_MUTATIONS:
        if ref.bwd_mutation_layer(c, mutate) is None:
            continue
        applied += 1
        if mutate == "gx_ragged_row_written":
            view, buf = ops_["gx"]
            buf = buf.clone()
            ref.check_gaps(buf, view, f"{c.name} gx buffer")
            buf[view.off + c.m * view.ld] = 0.0
            assert ref.rejects(ref.check_gaps, buf, view, "mutated"), f"{c.name}: '{mutate}' passed"
            continue
        wrong = f32(ref.bwd_reference(c, ops_, mutate))
        assert ref.rejects(ref.check_bwd, c, wrong, want), f"{c.name}: '{mutate}' passed the comparison"
    assert applied >= 4


def test_every_mutation_meets_a_case():
    for mutate in ref.FWD_MUTATIONS:
        assert any(ref.fwd_mutation_layer(c, mutate) is not None for c in ref.FWD_CASES + ref.HEAD_CASES), mutate
    for mutate in ref.BWD_MUTATIONS:
        assert any(ref.bwd_mutation_layer(c, mutate) is not None for c in ref.BWD_CASES), mutate
