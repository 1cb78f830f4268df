"""CPU only.  tests/interact_ref.py against the oracle, and its comparisons against small mutations of the references:
what tests/test_gpu_interactions.py trusts, checked without a GPU.

* ffm_ref, fields_fm_ref and pairs_ref equal the float64 oracle (outputs, loss, every parameter gradient);
* negative controls: each mutation of a reference, cast to float32 like a kernel's output, must be rejected by the
  comparison the GPU test applies to that output, at every input the GPU test uses there; the unmutated reference
  must pass the same comparison."""
import pytest
import torch

import interact_ref as ref
from oracle import ctr_oracle as orc

FFM_NAMES = ("age_user", "age_item", "gender_user", "gender_item", "occupation_user", "occupation_item",
             "movie_user", "movie_item", "userid_user", "userid_item", "itemid_user", "itemid_item")
TIGHT = dict(rtol=1e-11, atol=1e-13)   # float64 against float64: different summation orders only


def test_the_pair_list_is_the_models():
    assert tuple((FFM_NAMES.index(a), FFM_NAMES.index(b)) for a, b in orc.FFM_PAIRS) == ref.FFM_PAIRS
    for (kind, col, rows), vocab in zip(ref.FFM_SOURCE, ref.FFM_VOCAB):
        assert kind == "bag" and rows == vocab


@pytest.mark.parametrize("dim", [8, 16, 64])
def test_ffm_ref_equals_the_oracle_step(dim):
    """probability, loss and the gradients of all 16 parameters; the table gradients formed from gemb with the float64
    bag and gather chain rule"""
    batch = 67
    x, tables, user1, item1, lin_w, lin_b, _ = ref.ffm_case(dim, batch, 900 + dim)
    y = (torch.rand(batch, 1, generator=torch.Generator().manual_seed(dim)) < 0.5).float()
    params = {f"{n}.weight": t for n, t in zip(FFM_NAMES, tables)}
    params.update({"user.weight": user1, "item.weight": item1, "linear.weight": lin_w, "linear.bias": lin_b})
    prob_o, loss_o, grads_o = orc.step("ffm", params, [x], y, dtype=torch.float64)
    fwd = ref.ffm_ref(x, tables, user1, item1, lin_w, lin_b)
    p, yd = fwd["prob"], y.double()
    torch.testing.assert_close(p, prob_o, **TIGHT)
    torch.testing.assert_close(orc.bce_loss(p, yd), loss_o, **TIGHT)
    gprob = (p - yd) / (p * (1 - p)) / batch                      # d mean-BCE / d prob
    out = ref.ffm_ref(x, tables, user1, item1, lin_w, lin_b, gprob=gprob)
    got = {f"{n}.weight": g for n, g in zip(FFM_NAMES, ref.ffm_table_grads(x, tables, out["gemb"]))}
    got.update({"user.weight": out["guser1"], "item.weight": out["gitem1"], "linear.weight": out["glin_w"],
                "linear.bias": out["glin_b"]})
    assert set(got) == set(grads_o) and len(got) == 16
    for k in got:
        torch.testing.assert_close(got[k], grads_o[k], **TIGHT, msg=lambda m, k=k: f"{k}: {m}")
    # the head alone on the float32 operand is the same function
    head = ref.ffm_head_ref(fwd["emb"], 12, dim, ref.FFM_PAIRS, x, user1, item1, lin_w, lin_b)
    torch.testing.assert_close(head["prob"], prob_o, **TIGHT)


def test_fields_fm_ref_plus_a_float64_mlp_equals_the_oracle_step():
    vocabs, dim, batch = [7, 50, 1000, 5, 31], 8, 129
    idx, tables, first, bias, _, _ = ref.fields_case(vocabs, dim, batch, 77)
    gen = torch.Generator().manual_seed(5)
    nf = len(vocabs)
    rnd = lambda *s: 0.3 * torch.randn(*s, generator=gen)  # noqa: E731
    mlp = {"linear.weight": rnd(16, nf * dim), "linear.bias": rnd(16), "dnn_network.0.weight": rnd(8, 16),
           "dnn_network.0.bias": rnd(8), "dnn_network.1.weight": rnd(1, 8), "dnn_network.1.bias": rnd(1),
           "output.weight": rnd(1, 2), "output.bias": rnd(1)}
    params = dict(mlp)
    params.update({f"embeddings.{f}.weight": tables[f] for f in range(nf)})
    params.update({f"first_order.{f}.weight": first[f] for f in range(nf)})
    params["first_order_bias"] = bias
    y = (torch.rand(batch, 1, generator=gen) < 0.5).float()
    prob_o, loss_o, grads_o = orc.step("deepfm_fields", params, [idx], y, dtype=torch.float64)

    fwd = ref.fields_fm_ref(idx, tables, first, bias)
    emb = fwd["emb"].clone().requires_grad_(True)
    fm = fwd["fm"].clone().requires_grad_(True)
    m = {k: v.double().clone().requires_grad_(True) for k, v in mlp.items()}
    lin = torch.nn.functional.linear
    h = lin(emb, m["linear.weight"], m["linear.bias"])
    for k in range(2):
        h = torch.relu(lin(h, m[f"dnn_network.{k}.weight"], m[f"dnn_network.{k}.bias"]))
    prob = torch.sigmoid(lin(torch.cat([fm, h], 1), m["output.weight"], m["output.bias"]))
    loss = orc.bce_loss(prob, y.double())
    loss.backward()
    torch.testing.assert_close(prob.detach(), prob_o, **TIGHT)
    torch.testing.assert_close(loss.detach(), loss_o, **TIGHT)
    out = ref.fields_fm_ref(idx, tables, first, bias, gdeep=emb.grad, gfm=fm.grad)
    got = {k: v.grad for k, v in m.items()}
    got.update({f"embeddings.{f}.weight": out["gtables"][f] for f in range(nf)})
    got.update({f"first_order.{f}.weight": out["gfirst"][f] for f in range(nf)})
    got["first_order_bias"] = out["gbias"]
    assert set(got) == set(grads_o)
    for k in got:
        torch.testing.assert_close(got[k], grads_o[k], **TIGHT, msg=lambda m_, k=k: f"{k}: {m_}")
    # the masses dominate the values they belong to, the counts are those of the ids
    assert bool((out["fm_mass"] >= out["fm"].abs() * (1 - 1e-12)).all())
    for f in range(nf):
        assert bool((out["gtables_mass"][f] >= out["gtables"][f].abs() * (1 - 1e-12)).all())
        assert torch.equal(out["gfirst_n"][f].view(-1), torch.bincount(idx[:, f], minlength=vocabs[f]).double())


@pytest.mark.parametrize("nvec,dim,batch", [(6, 16, 37), (9, 8, 5), (32, 12, 3)])
def test_pairs_ref_equals_the_oracle(nvec, dim, batch):
    gen = torch.Generator().manual_seed(nvec * dim)
    buf = torch.randn(batch, nvec * dim + 4, generator=gen)
    emb = buf[:, :nvec * dim]                                     # a strided view
    gp = torch.randn(batch, nvec * (nvec - 1) // 2, generator=gen)
    leaf = emb.double().clone().requires_grad_(True)
    prod = orc.pnn_inner_products([leaf[:, f * dim:(f + 1) * dim] for f in range(nvec)])
    prod.backward(gp.double())
    out = ref.pairs_ref(emb, nvec, dim, gp)
    torch.testing.assert_close(out["prod"], prod.detach(), **TIGHT)
    torch.testing.assert_close(out["gemb"], leaf.grad, **TIGHT)
    assert bool((out["prod_mass"] >= out["prod"].abs() * (1 - 1e-12)).all())
    assert bool((out["gemb_mass"] >= out["gemb"].abs() * (1 - 1e-12)).all())


def test_rows_sum_and_act_mask_refs():
    gen = torch.Generator().manual_seed(3)
    ta, tb = torch.randn(5, 12, generator=gen), torch.randn(7, 12, generator=gen)
    ids = torch.stack([torch.randint(0, 5, (9,), generator=gen), torch.randint(0, 7, (9,), generator=gen)], 1)
    for act, fn in ((ref.ACT_NONE, lambda z: z), (ref.ACT_RELU, torch.relu), (ref.ACT_SIGMOID, torch.sigmoid)):
        out = ref.rows_sum_act_ref(ta, ids[:, 0], tb, ids[:, 1], act)
        z = (ta.double()[ids[:, 0]] + tb.double()[ids[:, 1]]).requires_grad_(True)
        y = fn(z)
        torch.testing.assert_close(out["out"], y.detach(), **TIGHT)
        g = torch.randn(9, 12, generator=gen)
        y.backward(g.double())
        torch.testing.assert_close(ref.act_mask_ref(g, y.detach(), act)["out"], z.grad, **TIGHT)


# ---------------------------------------------------------------------------------------------------------------
# negative controls
# ---------------------------------------------------------------------------------------------------------------
def _f32(d):
    return {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


@pytest.mark.parametrize("dim,batch", ref.FFM_FUSED_CASES)
@pytest.mark.parametrize("mutate", ["drop_pair", "half_group", "no_cross", "swap_partners"])
def test_the_ffm_comparisons_reject_small_mutations(dim, batch, mutate):
    """one of the 15 pairs dropped, only LPR / 2 lanes of a group added, x without + cross: the probability comparison
    rejects each; two partner lists swapped: the gradient comparison rejects it"""
    x, tables, user1, item1, lin_w, lin_b, gprob = ref.ffm_case(dim, batch, ref.ffm_seed(dim, batch))
    want = ref.ffm_ref(x, tables, user1, item1, lin_w, lin_b, gprob=gprob)
    wrong = _f32(ref.ffm_ref(x, tables, user1, item1, lin_w, lin_b, gprob=gprob, mutate=mutate))
    keys = ("gemb", "guser1", "gitem1", "glin_w", "glin_b")
    good = _f32(want)
    ref.check_ffm_emb(good["emb"], want)
    ref.check_prob(good["prob"], want["prob"])
    ref.check_ffm_bwd({k: good[k] for k in keys}, want)
    if mutate == "swap_partners":
        assert ref.rejects(ref.check_ffm_bwd, {"gemb": wrong["gemb"]}, want), f"'{mutate}' passed the gradient comparison"
    else:
        assert ref.rejects(ref.check_prob, wrong["prob"], want["prob"]), f"'{mutate}' passed the probability comparison"
        assert ref.rejects(ref.check_ffm_bwd, {k: wrong[k] for k in keys}, want), f"'{mutate}' passed the gradient comparison"


@pytest.mark.parametrize("case", ref.FIELDS_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("mutate", ["no_last", "shift_first"])
def test_the_fields_fm_comparisons_reject_small_mutations(case, mutate):
    """the last field left out of S: fm and the table gradients are rejected; the first-order rule shifted by one field:
    fm is rejected (with one field there is no neighbour to shift to: left out)"""
    name, vocabs, dim, batch = case
    if mutate == "shift_first" and len(vocabs) == 1:
        return
    idx, tables, first, bias, gdeep, gfm = ref.fields_case(vocabs, dim, batch, ref.fields_seed(name))
    want = ref.fields_fm_ref(idx, tables, first, bias, gdeep, gfm)
    wrong = ref.fields_fm_ref(idx, tables, first, bias, gdeep, gfm, mutate=mutate)
    f32 = lambda ts: [t.float() for t in ts]  # noqa: E731
    ref.check_fields_fm_fwd(want["emb"].float(), want["fm"].float(), want)
    ref.check_fields_fm_bwd(f32(want["gtables"]), f32(want["gfirst"]), want["gbias"].float(), want)
    assert ref.rejects(ref.check_fields_fm_fwd, wrong["emb"].float(), wrong["fm"].float(), want), f"'{mutate}' passed (fm)"
    if mutate == "no_last":
        assert ref.rejects(ref.check_fields_fm_bwd, f32(wrong["gtables"]), None, None, want), f"'{mutate}' passed (gtables)"


@pytest.mark.parametrize("nvec,dim,batch", [c for c in ref.PAIRS_CASES if c[2] < 1000])
def test_the_pairs_comparison_rejects_a_dropped_element_and_a_shifted_pair(nvec, dim, batch):
    """a product that misses the vector's last element, and products written one slot later, are both rejected"""
    emb, gp = ref.pairs_case(nvec, dim, batch)
    want = ref.pairs_ref(emb, nvec, dim, gp)
    check = lambda got: ref.check_sum(got, want["prod"], want["prod_n"], want["prod_mass"], "prod")  # noqa: E731
    check(want["prod"].float())
    v = emb.double().view(batch, nvec, dim).clone()
    v[:, :, -1] = 0.0
    assert ref.rejects(check, ref.pairs_ref(v.view(batch, -1), nvec, dim)["prod"].float())
    assert ref.rejects(check, want["prod"].float().roll(1, 1))
    gcheck = lambda got: ref.check_sum(got, want["gemb"], want["gemb_n"], want["gemb_mass"], "gemb")  # noqa: E731
    gcheck(want["gemb"].float())
    gp2 = gp.clone()
    gp2[:, -1] = 0.0                                              # the last pair's coefficient never arrives
    assert ref.rejects(gcheck, ref.pairs_ref(emb, nvec, dim, gp2)["gemb"].float())


@pytest.mark.parametrize("act", [ref.ACT_NONE, ref.ACT_RELU, ref.ACT_SIGMOID])
def test_the_rows_sum_comparison_rejects_a_missing_row_and_one_ulp_too_many(act):
    table_a, table_b, ids = ref.rows_case(24, 333)
    want = ref.rows_sum_act_ref(table_a, ids[:, 0], table_b, ids[:, 1], act)
    ref.check_rows_sum_act(want["out"].float(), want, act)
    only_a = ref.rows_sum_act_ref(table_a, ids[:, 0], torch.zeros_like(table_b), ids[:, 1], act)
    assert ref.rejects(ref.check_rows_sum_act, only_a["out"].float(), want, act)
    other = ref.rows_sum_act_ref(table_a, ids[:, 0].roll(1), table_b, ids[:, 1], act)
    assert ref.rejects(ref.check_rows_sum_act, other["out"].float(), want, act)
