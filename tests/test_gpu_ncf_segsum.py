"""NeuralCF's table-row path (csrc/ncf_proj.hip): the segment sums over the buckets.  A lane group of sixteen owns
sixteen consecutive slots, a workgroup 256; a run of one row that ends inside its group is stored, a run that goes on
in a neighbouring group is parked in LDS and met there by the workgroup, and only a chain that is open at a
workgroup's first or last slot is added atomically.

* the launch alone: after a training forward, ncfp_bwd (phases = 1) and ncfp_segsum (phases = 2) through the C entry
  points on a workspace pre-filled with a sentinel, ST = [S | T] against float64 sums formed on the CPU from the kernel's
  own inputs (the gz0 rows, the slot records, the GMF tables), for id patterns that put the run boundaries where the
  kernel takes another path;
* whole steps against the CPU oracle for three of them.

The bound of the first is n_v * 2^-23 * sum |terms| per element, n_v the bucket's size: the error of an fp32 sum of n_v
terms in any order, (n_v - 1) 2^-24 sum |terms| to first order, plus one rounding per product, with a factor two to
spare -- not a tuned tolerance.  A row without a sample must be exactly zero.  The whole steps use the repository's
tolerances: prob / loss rtol 1e-5, atol 1e-6; gradients rtol 1e-4 with a floor of 1e-6 + 1e-5 max|ref|
(tests/test_gpu_ncf_bucket_plan.py, _check_grads)."""
import ctypes as C

import pytest
import torch

DEV = "cuda:0"
SENTINEL = -12345.5
# record fields that would address far outside every buffer if anything were fetched through them: as a float 3.4e38,
# as an index 2139062143; and the most negative index but one
POISON = (0x7F7F7F7F, -0x7FFFFFFF)

CASES = ["aligned", "one_off", "two_rows", "short_buckets", "ragged", "hot"]


def _check_grads(got, want):
    """the rule of tests/test_gpu_ncf_bucket_plan.py"""
    assert set(got) == set(want)
    for k in want:
        floor = 1e-6 + 1e-5 * float(want[k].abs().max())
        torch.testing.assert_close(got[k], want[k], rtol=1e-4, atol=floor, msg=lambda m, k=k: f"grad {k}: {m}")


def _ncf(nu, ni, seed):
    from deeplearningrecommendationsystem_amd.model import NeuralCF
    torch.manual_seed(seed)
    return NeuralCF(nu, ni, 64, [128, 64, 32, 16, 8])


def _case(name):
    """(nu, ni, user ids, item ids, poison the unused slots)"""
    from deeplearningrecommendationsystem_amd import synth
    gen = synth.generator(1000 + CASES.index(name))
    if name in ("aligned", "one_off"):
        # every user bucket is one workgroup's 256 slots, every item bucket one group's 16: no open run anywhere;
        # one_off: a user id outside the table takes one slot out, every later bucket straddles a boundary by one
        nu, ni, m = 16, 256, 4096
        b = torch.randperm(m, generator=gen)
        u, i = b % 16, (b // 16) % 256
        if name == "one_off":
            u[100] = nu
    elif name == "two_rows":
        # every group is a single run, open on both sides: chains through whole workgroups, atomics at both edges
        nu, ni, m = 1, 1, 4096
        u, i = torch.zeros(m, dtype=torch.int64), torch.zeros(m, dtype=torch.int64)
    elif name == "short_buckets":
        # several complete runs per group, rows without a sample, item buckets of ~170 slots
        nu, ni, m = 1000, 24, 4096
        u, i = synth.id_batch(m, nu, ni, gen)
    elif name == "ragged":
        # batch = 1 mod 16, an odd total (the four ids of the bucket-plan test outside their tables, and a fifth), the
        # last group and the last workgroup partly behind the total
        nu, ni, m = 301, 407, 4097
        u, i = synth.id_batch(m, nu, ni, gen)
        u[5], u[m - 1], i[7], i[m // 2] = nu, -1, ni + 9, -3
        u[11] = nu + 1
    else:
        assert name == "hot"
        # 90 % of the samples on one user: one bucket across ~29 workgroups, many adders on one row
        nu, ni, m = 301, 407, 8192
        u, i = synth.id_batch(m, nu, ni, gen)
        u[torch.rand(m, generator=gen) < 0.9] = 17
    y = synth.labels(m, True, gen)
    return nu, ni, u.contiguous(), i.contiguous(), y, name == "ragged"


def _segment_sums_alone(module, u, i, y, poison):
    """a training forward, then ncfp_bwd (phases = 1) and ncfp_segsum (phases = 2) through the C entry points, the way
    ops.NcfProj calls them, on a workspace pre-filled with a sentinel (`poison`: the slot records with POISON instead:
    what the slots at and behind the total still hold when the segment sums run).  Returns the bucket offsets and, from
    the workspace (layout: csrc/ncf_proj.hip, workspace_floats), the gz0 rows (m + 1, 64), the records (2 m + 1, 4) as
    int32 and ST (rows, 128)."""
    from deeplearningrecommendationsystem_amd import _lib, ops
    p = {k: v.detach() for k, v in module.named_parameters()}
    tables = (p["GMF_Embedding_User.weight"], p["GMF_Embedding_Item.weight"], p["MLP_Embedding_User.weight"],
              p["MLP_Embedding_Item.weight"])
    hidden = [ops.Layer(p[f"dnn_network.{k}.weight"], p[f"dnn_network.{k}.bias"], ops.ACT_RELU) for k in range(4)]
    proj, head = (p["linear.weight"], p["linear.bias"]), (p["linear2.weight"], p["linear2.bias"])
    m = u.numel()
    assert ops.NcfProj.supported(tables, hidden, proj, m)
    ud, idd, yd = u.to(DEV), i.to(DEV), y.to(DEV)
    run = ops.NcfProj(ud, idd, tables, hidden, proj, head, None, True)
    prob = run.forward()
    assert prob is not None
    pr = prob.reshape(-1)
    gprob = ((pr - yd.reshape(-1)) / (pr * (1.0 - pr)).clamp_min(1e-12) / m).contiguous()
    grads = {k: torch.zeros_like(v) for k, v in p.items()}
    d, g = run._desc(), _lib.NcfProjGrad()
    g.gprob, g.ldgprob = gprob.data_ptr(), 1
    for k in range(4):
        g.layers[k].gw, g.layers[k].gb = grads[f"dnn_network.{k}.weight"].data_ptr(), grads[f"dnn_network.{k}.bias"].data_ptr()
    g.g_gmf_user, g.g_gmf_item = grads["GMF_Embedding_User.weight"].data_ptr(), grads["GMF_Embedding_Item.weight"].data_ptr()
    g.g_mlp_user, g.g_mlp_item = grads["MLP_Embedding_User.weight"].data_ptr(), grads["MLP_Embedding_Item.weight"].data_ptr()
    g.g_proj_w, g.ld_g_proj_w, g.g_proj_b = (grads["linear.weight"].data_ptr(), grads["linear.weight"].stride(0),
                                             grads["linear.bias"].data_ptr())
    g.g_head_w, g.g_head_b = grads["linear2.weight"].data_ptr(), grads["linear2.bias"].data_ptr()
    need = C.c_int64(0)
    assert _lib.load().ctr_ncf_proj_workspace_floats(m, run.nu, run.ni, C.byref(need)) == 0
    rows = run.nu + run.ni
    ws = torch.full((need.value,), SENTINEL, dtype=torch.float32, device=DEV)
    r0, r1 = (m + 1) * 64, (m + 1) * 64 + (2 * m + 1) * 4
    if poison:
        rec = ws[r0:r1].view(torch.int32).view(-1, 4)
        rec[0::2] = POISON[0]
        rec[1::2] = POISON[1]
    g.workspace, g.workspace_floats = ws.data_ptr(), need.value
    g.zero_buf, g.zero_floats = None, 0
    for phase in (1, 2):
        g.phases = phase
        rc = _lib.load().ctr_ncf_proj_bwd(C.byref(d), C.byref(g), _lib.stream_ptr())
        _lib.check(rc, "ctr_ncf_proj_bwd")
    torch.cuda.synchronize()
    offsets = run.bucket_offsets().cpu().to(torch.int64)
    gz0 = ws[:r0].view(m + 1, 64).cpu()
    rec = ws[r0:r1].view(torch.int32).view(-1, 4).cpu()
    st = ws[r1:r1 + rows * 128].view(rows, 128).cpu()
    return offsets, gz0, rec, st, tables[0].cpu(), tables[1].cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_the_segment_sums_alone(name):
    """ST after ncfp_bwd and ncfp_segsum alone against float64 sums over the buckets, formed from the gz0 rows, the slot
    records and the GMF tables the launch itself read.  Bound per element: n_v 2^-23 sum |terms|; a row without a sample
    is exactly zero.  In `ragged` the record slots at and behind the total hold POISON."""
    nu, ni, u, i, y, poison = _case(name)
    m, rows = u.numel(), nu + ni
    offsets, gz0, rec, st, gmf_u, gmf_i = _segment_sums_alone(_ncf(nu, ni, 23).to(DEV), u, i, y, poison)
    good_u, good_i = (u >= 0) & (u < nu), (i >= 0) & (i < ni)
    counts = torch.cat([torch.bincount(u[good_u], minlength=nu), torch.bincount(i[good_i], minlength=ni)])
    assert torch.equal(offsets, torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]))
    total = int(offsets[rows])
    if name == "one_off":
        assert total == 8191
    if name == "ragged":
        assert total % 2 == 1 and m % 16 == 1
        behind = rec[total:2 * m].to(torch.int64)
        assert bool((behind[0::2] == POISON[total % 2]).all()) and bool((behind[1::2] == POISON[1 - total % 2]).all())
    # the bucket of row v is the slots [offsets[v], offsets[v + 1])
    slot_row = torch.repeat_interleave(torch.arange(rows), counts)
    used = rec[:total]
    assert torch.equal(used[:, 2].to(torch.int64), slot_row)
    gz = used[:, 0].contiguous().view(torch.float32).to(torch.float64)
    partner, sample = used[:, 1].to(torch.int64), used[:, 3].to(torch.int64)
    assert bool(((sample >= 0) & (sample < m)).all())
    user_slot = slot_row < nu
    assert bool((partner[user_slot] < ni).all()) and bool((partner[~user_slot] < nu).all()) and bool((partner >= 0).all())
    prow = torch.where(user_slot.unsqueeze(1), gmf_i.to(torch.float64)[partner.clamp(max=ni - 1)],
                       gmf_u.to(torch.float64)[partner.clamp(max=nu - 1)])
    terms = torch.cat([gz0.to(torch.float64)[sample], gz.unsqueeze(1) * prow], dim=1)           # (total, 128)
    want = torch.zeros(rows, 128, dtype=torch.float64).index_add_(0, slot_row, terms)
    mass = torch.zeros(rows, 128, dtype=torch.float64).index_add_(0, slot_row, terms.abs())
    bound = counts.to(torch.float64).unsqueeze(1) * 2.0 ** -23 * mass
    err = (st.to(torch.float64) - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: total {total}, max |err| {float(err.max()):.3e}, max |err| / bound {worst:.3f}")
    assert bool(torch.isfinite(st).all())
    empty = counts == 0
    assert bool((st[empty] == 0).all()), "a row without a sample is not exactly zero"
    assert bool((err <= bound).all()), f"max |err| / bound = {worst}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["aligned", "two_rows", "short_buckets"])
def test_a_whole_step_against_the_oracle(name):
    """the step as training runs it against the CPU oracle: runs that fill their group or workgroup exactly, two table
    rows that chain through every workgroup, and many short complete runs"""
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import neuralcf as ncf_mod
    from oracle import ctr_oracle as orc
    nu, ni, u, i, y, _ = _case(name)
    module = _ncf(nu, ni, 41)
    params = {k: v.detach().clone() for k, v in module.state_dict().items()}
    prob_ref, loss_ref, grads_ref = orc.step("neuralcf", params, [u, i], y)
    module = module.to(DEV)
    calls = []
    real = ops.NcfProj.backward
    ops.NcfProj.backward = lambda self, *a: (calls.append(1), real(self, *a))[1]
    try:
        assert ncf_mod.PROJECT_TABLES
        module.train()
        module.zero_grad()
        prob = module(u.to(DEV), i.to(DEV))
        loss = torch.nn.BCELoss()(prob, y.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.NcfProj.backward = real
    assert calls, "the table-row path did not run"
    torch.testing.assert_close(prob.detach().cpu(), prob_ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(loss.detach().cpu(), loss_ref, rtol=1e-5, atol=1e-6)
    _check_grads({k: p.grad.detach().cpu() for k, p in module.named_parameters()}, grads_ref)
