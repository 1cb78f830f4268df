"""CPU: the float64 reference of the embedding stage (tests/embed_ref.py) against float64 autograd, the exactness guard
over every case of tests/embed_cases.py, and mutations of the reference that the exact comparison has to notice."""
import pytest
import torch

import embed_cases as cases
import embed_ref as ref


def _in_range(case):
    """the case's specs and x with every bad id folded into range (id mod vocab): the restatement below indexes"""
    mats = {k: m.clone() for k, m in case.mats.items()}
    x = None if case.x is None else case.x.clone()
    specs = []
    for s in case.specs:
        t = ref.Spec(**s.__dict__)
        if s.kind in (ref.ID_I64, ref.PROD_I64):
            m, c = s.ikey
            mats[m][:, c] %= s.table.shape[0]
            t.idx = mats[m][:, c]
        if s.kind == ref.PROD_I64:
            m, c = s.ikey2
            mats[m][:, c] %= s.table2.shape[0]
            t.idx2 = mats[m][:, c]
        if s.kind == ref.ID_F32:
            x[:, s.src_col] = (x[:, s.src_col].to(torch.int64) % s.table.shape[0]).float()
        specs.append(t)
    return specs, x


def _autograd(case, specs, x):
    """tab[idx], x @ tab, t1[i] * t2[j] written into a zero (batch, width) matrix; d(sum(out * gout)) / d(table)"""
    leaves = {k: t.double().requires_grad_() for k, t in case.tables.items()}
    out = torch.zeros(case.batch, case.width, dtype=torch.float64)
    for s in specs:
        cols = slice(s.out_col, s.out_col + s.width)
        if s.kind == ref.ID_I64:
            out[:, cols] = leaves[s.tkey][s.idx]
        elif s.kind == ref.ID_F32:
            out[:, cols] = leaves[s.tkey][x[:, s.src_col].long()]
        elif s.kind == ref.BAG:
            out[:, cols] = x[:, s.src_col:s.src_col + s.bag_size].double() @ leaves[s.tkey]
        elif s.kind == ref.DENSE:
            out[:, cols] = x[:, s.src_col:s.src_col + s.width].double()
        else:
            out[:, cols] = leaves[s.tkey][s.idx] * leaves[s.tkey2][s.idx2]
    (out * case.gout.double()).sum().backward()
    return out.detach(), {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in leaves.items()}


@pytest.mark.parametrize("name", cases.SMALL)
def test_reference_equals_float64_autograd_on_in_range_ids(name):
    case = cases.case(name)
    specs, x = _in_range(case)
    out, flag = ref.embed_ref(specs, x, case.batch)
    want_out, want_grads = _autograd(case, specs, x)
    assert flag == 0
    assert torch.equal(out.nan_to_num(nan=0.0), want_out), ref.first_diff(out.nan_to_num(nan=0.0), want_out)
    grads = ref.embed_bwd_ref(specs, x, case.gout)
    for key, want in want_grads.items():
        got = grads.get(key, torch.zeros_like(want))
        assert torch.equal(got, want), f"{key}: {ref.first_diff(got, want)}"


@pytest.mark.parametrize("name", cases.names())
def test_every_case_passes_the_exactness_guard_and_is_on_its_arm(name):
    case = cases.case(name)
    worst_b, worst_f = ref.exact_guard(case)
    print(f"{name}: backward at most {worst_b:.0f} units of 2^-6, forward {worst_f:.0f} of 2^-4 (limit {ref.LIMIT:.0f})")
    # the flag is raised exactly where the case says it has bad ids
    assert ref.embed_ref(case.specs, case.x, case.batch)[1] == int(case.has_bad)
    # the kernels the case names are the ones the entry point's selectors (restated in embed_cases.py) choose
    fwd, bwd = cases.forward_kernels(case), cases.backward_kernels(case)
    print(f"{name}: forward {sorted(fwd)}, backward {sorted(bwd)}; aimed at {case.arm}")
    assert cases.claimed_kernels(case.arm) == (fwd if case.family.startswith("fwd_") else bwd)


def test_the_guard_rejects_a_product_field_at_batch_140000():
    """64 units per sample are fine for the id field; a product term reaches 128: with every id equal the sum does
    not fit"""
    b = ref.Build("guard_rejects", "none", "none", 140000)
    m = b.ids([100, 100], "equal")
    b.prod(b.table(100, 4), m, 0, b.table(100, 4), m, 1)
    case = b.done()
    case.tables["t0"].fill_(2.0)
    case.tables["t1"].fill_(2.0)
    case.gout.fill_(1.0)
    with pytest.raises(AssertionError, match="units of 2\\^-6"):
        ref.exact_guard(case)


def _outputs(case, mutate=None):
    """forward output and every gradient as fp32, the form the device results are compared in; gout gets four more
    dyadic columns on the right so that a field shifted by four columns has something to read"""
    gen = torch.Generator().manual_seed(11)
    gout = torch.cat([case.gout, ref.sixteenths_nonzero((case.batch, 4), gen)], 1)
    out, _ = ref.embed_ref(case.specs, case.x, case.batch, mutate)
    if out.shape[1] == case.width:
        out = torch.cat([out, torch.full((case.batch, 4), float("nan"), dtype=torch.float64)], 1)
    grads = ref.embed_bwd_ref(case.specs, case.x, gout, mutate)
    return {"out": out.float(), **{k: (g + case.base[k].double()).float() for k, g in grads.items() if k not in case.frozen}}


def _changed(a, b):
    return [k for k in a if ref.first_diff(a[k], b[k]) is not None]


_SMALL = {}


def _small(name):
    if name not in _SMALL:
        case = cases.case(name)
        _SMALL[name] = (case, _outputs(case))
    return _SMALL[name]


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
@pytest.mark.parametrize("family", cases.families())
def test_a_mutated_reference_differs_in_every_family(family, mutation):
    """drop the last sample / double one sample of the hottest row / shift every out_col by four: every case changes.
    Swap the product partners: every case with a product.  Send bad ids to row 0 (what the sorted path did): every case
    with bad ids.  Skip row vocab - 1: at least one case of the family"""
    changed, applicable = 0, 0
    for name in cases.names(family):
        if name not in cases.SMALL:
            continue
        case, true = _small(name)
        has_prod = any(s.kind == ref.PROD_I64 for s in case.specs)
        has_grad = any(s.kind != ref.DENSE and (s.tkey not in case.frozen or (s.tkey2 and s.tkey2 not in case.frozen))
                       for s in case.specs)
        must = {"drop_last": True, "double_hot": has_grad, "shift_out_col": True, "swap_partners": has_prod,
                "bad_to_row0": case.has_bad, "skip_last_row": False}[mutation]
        diff = _changed(true, _outputs(case, mutation))
        print(f"{name} / {mutation}: {diff}")
        if must:
            assert diff, f"{name}: the mutation {mutation} changes no output bit"
        applicable += must or mutation == "skip_last_row"
        changed += bool(diff)
    na = (family, mutation) in {(f, "swap_partners") for f in ("fwd_ids", "fwd_bag", "bwd_fast", "bwd_hot", "bwd_bag")}
    assert (applicable == 0) == na, f"{family} / {mutation}: applicable to {applicable} cases"
    assert na or changed > 0


def test_each_family_has_small_cases_and_the_two_hot_rows_collide():
    for family in cases.families():
        assert [n for n in cases.names(family) if n in cases.SMALL], family
    a, b = ref.colliding_rows(9000)
    assert ref.hot_slot(0, a) == ref.hot_slot(1, b) and 0 < a < 9000 and 0 < b < 9000
    case = cases.case("bwd_hot_w4_collision")
    ids = case.mats["m0"]
    assert int((ids[:, 0] == a).sum()) > 20000 and int((ids[:, 1] == b).sum()) > 20000
    assert int((ids[:, 2] == 8999).sum()) == 2
    assert case.batch * 8 == 2048 * 256 + 24
