"""NeuralCF's table-row path (csrc/ncf_proj.hip): the bucket plan a training forward builds -- ranks from per-chunk LDS
histograms, per-row prefixes over the chunks, bucket offsets scanned once -- and the backward reads.

* the plan is a bucketing: after a training forward and the per-sample backward launch ALONE the slot records of every
  table row's bucket name exactly the samples that carry that id, every slot below the total is written once, a sample
  with an id outside its table owns no slot;
* whole steps against the CPU oracle for id patterns that stress the plan (sorted ids, one hot user, Zipf, chunks that
  miss most rows);
* a captured step replayed with OTHER ids in its static buffers: the plan is rebuilt inside the graph.

Tolerances are the repository's: prob / loss rtol 1e-5, atol 1e-6; gradients rtol 1e-4 with a floor of 1e-6 +
1e-5 max|ref| (test_gpu_models._check_grads)."""
import ctypes as C

import pytest
import torch

DEV = "cuda:0"
SENTINEL = -12345.5


def _check_grads(got, want):
    assert set(got) == set(want)
    for k in want:
        floor = 1e-6 + 1e-5 * float(want[k].abs().max())
        torch.testing.assert_close(got[k], want[k], rtol=1e-4, atol=floor, msg=lambda m, k=k: f"grad {k}: {m}")


def _ncf(nu, ni, seed):
    from deeplearningrecommendationsystem_amd.model import NeuralCF
    torch.manual_seed(seed)
    return NeuralCF(nu, ni, 64, [128, 64, 32, 16, 8])


def _oracle(module, u, i, y):
    from oracle import ctr_oracle as orc
    params = {k: v.detach().clone() for k, v in module.state_dict().items()}
    return orc.step("neuralcf", params, [u, i], y)


def _records_after_the_per_sample_launch(module, u, i, y):
    """a training forward and ncfp_bwd alone (phases = 1) through the C entry points, the way ops.NcfProj calls them, on
    a workspace pre-filled with a sentinel.  Returns the plan's bucket offsets (rows + 1) and the slot records'
    (row, sample) columns as int64 (2 batch + 1 slots; a slot nobody wrote keeps the sentinel's bits in both)."""
    from deeplearningrecommendationsystem_amd import _lib, ops
    p = {k: v.detach() for k, v in module.named_parameters()}
    tables = (p["GMF_Embedding_User.weight"], p["GMF_Embedding_Item.weight"], p["MLP_Embedding_User.weight"],
              p["MLP_Embedding_Item.weight"])
    hidden = [ops.Layer(p[f"dnn_network.{k}.weight"], p[f"dnn_network.{k}.bias"], ops.ACT_RELU) for k in range(4)]
    proj, head = (p["linear.weight"], p["linear.bias"]), (p["linear2.weight"], p["linear2.bias"])
    batch = u.numel()
    assert ops.NcfProj.supported(tables, hidden, proj, batch)
    ud, idd, yd = u.to(DEV), i.to(DEV), y.to(DEV)
    run = ops.NcfProj(ud, idd, tables, hidden, proj, head, None, True)
    prob = run.forward()
    assert prob is not None
    pr = prob.reshape(-1)
    gprob = ((pr - yd.reshape(-1)) / (pr * (1.0 - pr)).clamp_min(1e-12) / batch).contiguous()
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
    assert _lib.load().ctr_ncf_proj_workspace_floats(batch, run.nu, run.ni, C.byref(need)) == 0
    ws = torch.full((need.value,), SENTINEL, dtype=torch.float32, device=DEV)
    g.workspace, g.workspace_floats = ws.data_ptr(), need.value
    g.zero_buf, g.zero_floats = None, 0
    g.phases = 1
    rc = _lib.load().ctr_ncf_proj_bwd(C.byref(d), C.byref(g), _lib.stream_ptr())
    _lib.check(rc, "ctr_ncf_proj_bwd")
    torch.cuda.synchronize()
    offsets = run.bucket_offsets().cpu().to(torch.int64)
    # workspace: gz0 rows (batch + 1, 64) | slot records (2 batch + 1, 4) = {gz, partner id, row, sample}
    rec = ws[(batch + 1) * 64: (batch + 1) * 64 + (2 * batch + 1) * 4].view(torch.int32).view(-1, 4).cpu().to(torch.int64)
    return offsets, rec[:, 2], rec[:, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("nu,ni,batch", [(943, 1682, 65536), (301, 407, 4096), (301, 407, 64 * 256 + 1), (301, 407, 8193),
                                         (6000, 10384, 65536)],
                         ids=["benchmark", "batch4096", "last_chunk_of_one", "batch_1_mod_16", "max_rows"])
def test_the_plan_is_a_bucketing(nu, ni, batch):
    """the benchmark's shape; batch 4096 (sixteen chunks of one sample per thread); 64 x 256 + 1 samples (one more than
    64 chunks of 256 hold: chunks of 512, the 33rd holds one sample); a batch = 1 mod 16; 16384 table rows (the LDS
    histogram at its 64 KB, most rows missing from every chunk).  Every case carries a few ids outside their tables."""
    from deeplearningrecommendationsystem_amd import _lib, synth
    assert nu + ni <= _lib.CTR_NCF_PROJ_MAX_ROWS
    gen = synth.generator(batch + nu)
    u, i = synth.id_batch(batch, nu, ni, gen)
    u[0], i[0], u[1], i[1] = 0, 0, nu - 1, ni - 1
    u[5], u[batch - 1], i[7], i[batch // 2] = nu, -1, ni + 9, -3          # no slot in that table
    u[11], i[11] = nu + 1, -1                                             # no slot at all
    y = synth.labels(batch, True, gen)
    offsets, rec_row, rec_sample = _records_after_the_per_sample_launch(_ncf(nu, ni, 5).to(DEV), u, i, y)
    rows = nu + ni
    good_u, good_i = (u >= 0) & (u < nu), (i >= 0) & (i < ni)
    # offsets = exclusive scan of the per-row sample counts, user rows first
    counts = torch.cat([torch.bincount(u[good_u], minlength=nu), torch.bincount(i[good_i], minlength=ni)])
    want_off = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    assert torch.equal(offsets, want_off)
    total = int(want_off[rows])
    assert total == int(good_u.sum()) + int(good_i.sum())
    # every slot below the total holds the row its position says, slots behind it (but the spare one) were never written
    slot_row = torch.repeat_interleave(torch.arange(rows), counts)
    assert torch.equal(rec_row[:total], slot_row)
    sentinel = int(torch.tensor([SENTINEL]).view(torch.int32))
    assert bool((rec_row[total:2 * batch] == sentinel).all()) and bool((rec_sample[total:2 * batch] == sentinel).all())
    # a bucket names exactly the samples that carry its id: each table's half of the slots, sorted by (row, sample),
    # is the stable sort of that table's good samples by id -- every sample once, none without a slot's right
    nslot_u = int(want_off[nu])
    for lo, hi, ids, good, base in ((0, nslot_u, u, good_u, 0), (nslot_u, total, i, good_i, nu)):
        samples = torch.nonzero(good).reshape(-1)
        order = torch.argsort(ids[samples], stable=True)
        want_samples = samples[order]                                     # by id, then by sample
        got = rec_row[lo:hi] * (2 * batch) + rec_sample[lo:hi]
        assert torch.equal(torch.sort(got).values, (ids[want_samples] + base) * (2 * batch) + want_samples)


def _pattern(name, nu, ni, batch, gen):
    from deeplearningrecommendationsystem_amd import synth
    u, i = synth.id_batch(batch, nu, ni, gen)
    if name == "sorted_by_user":
        order = torch.argsort(u, stable=True)
        u, i = u[order], i[order]
    elif name == "sorted_by_item":
        order = torch.argsort(i, stable=True)
        u, i = u[order], i[order]
    elif name == "hot_user":                   # 90 % of the samples on one user
        u[torch.rand(batch, generator=gen) < 0.9] = 17
    elif name == "zipf":                       # P(id <= r) = log r / log V in both columns
        u = (torch.exp(torch.rand(batch, generator=gen) * torch.log(torch.tensor(float(nu)))).long() - 1).clamp_(0, nu - 1)
        i = (torch.exp(torch.rand(batch, generator=gen) * torch.log(torch.tensor(float(ni)))).long() - 1).clamp_(0, ni - 1)
    else:
        assert name == "uniform"
    return u, i


@pytest.mark.gpu
@pytest.mark.parametrize("name,nu,ni,batch", [("sorted_by_user", 943, 1682, 16384), ("sorted_by_item", 943, 1682, 16384),
                                              ("hot_user", 943, 1682, 16384), ("zipf", 943, 1682, 16384),
                                              ("uniform", 6000, 10384, 65536)],
                         ids=["sorted_by_user", "sorted_by_item", "hot_user", "zipf", "chunks_miss_most_rows"])
def test_a_whole_step_against_the_oracle_for_id_patterns_that_stress_the_plan(name, nu, ni, batch):
    """ids sorted by user / by item (a chunk's samples share a few rows: whole waves on one LDS counter, most rows of
    the histogram zero), 90 % of the samples on one user, Zipf ids, and 16384 table rows at the smallest batch the path
    admits for them (a chunk of 1024 samples misses most rows): the step as training runs it against the CPU oracle"""
    from deeplearningrecommendationsystem_amd import ops, synth
    from deeplearningrecommendationsystem_amd.model import neuralcf as ncf_mod
    module = _ncf(nu, ni, 41)
    gen = synth.generator(batch + len(name))
    u, i = _pattern(name, nu, ni, batch, gen)
    y = synth.labels(batch, True, gen)
    prob_ref, loss_ref, grads_ref = _oracle(module, u, i, y)
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


@pytest.mark.gpu
def test_graph_replay_rebuilds_the_plan_for_changed_ids():
    """a captured step (graph.GraphedStep) whose static id buffers get another batch -- other ids, sorted by user, so
    that no rank, prefix or offset of the captured batch fits -- replays to the gradients of an eager step on that
    batch; then the first batch again"""
    from deeplearningrecommendationsystem_amd import synth
    from deeplearningrecommendationsystem_amd.graph import GraphedStep
    from deeplearningrecommendationsystem_amd.loss import BCELoss
    nu, ni, batch = 943, 1682, 16384
    model = _ncf(nu, ni, 13).to(DEV)
    model.train()
    gen = synth.generator(99)
    batches = []
    for name in ("uniform", "sorted_by_user"):
        u, i = _pattern(name, nu, ni, batch, gen)
        batches.append((u.to(DEV), i.to(DEV), synth.labels(batch, True, gen).to(DEV)))

    def eager(u, i, y):
        model.zero_grad(set_to_none=True)
        loss = BCELoss()(model(u, i), y)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().cpu(), {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}

    want = [eager(*b) for b in batches]
    a = batches[0]
    graphed = GraphedStep(model, BCELoss(), [a[0].clone(), a[1].clone()], a[2].clone())
    for k in (0, 1, 0):
        u, i, y = batches[k]
        graphed.load([u, i], y)
        loss = graphed()
        torch.cuda.synchronize()
        torch.testing.assert_close(loss.detach().cpu().reshape(()), want[k][0].reshape(()), rtol=1e-5, atol=1e-6)
        _check_grads({n: p.grad.detach().cpu() for n, p in model.named_parameters()}, want[k][1])
