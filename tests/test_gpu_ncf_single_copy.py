"""NeuralCF's table-row path (csrc/ncf_proj.hip) after the layer-0 gradient rows moved to ONE copy in sample order and
ncfp_finish was split into parts: what the new workspace layout and the new grid can break and the model-level tests
(test_gpu_models.py) do not pin.

* the carve of the workspace: ctr_ncf_proj_bwd called with EXACTLY ctr_ncf_proj_workspace_floats floats, a sentinel
  behind them;
* the size itself, on the host (no GPU);
* the parts of ncfp_finish at the edges of the tables (a table smaller than a row block, ragged last blocks, a one-row
  table) and with gradient buffers the C call allows to be null.

Tolerances are the repository's (test_gpu_models._check_grads): rtol 1e-4, floor 1e-6 + 1e-5 max|ref| per gradient."""
import ctypes as C

import pytest
import torch

DEV = "cuda:0"
SENTINEL = -12345.5
GUARD = 1 << 16          # floats behind the workspace that must keep the sentinel


def _check_grads(got, want):
    assert set(got) == set(want)
    for k in want:
        floor = 1e-6 + 1e-5 * float(want[k].abs().max())
        torch.testing.assert_close(got[k], want[k], rtol=1e-4, atol=floor, msg=lambda m, k=k: f"grad {k}: {m}")


def _ncf(nu, ni, seed):
    from deeplearningrecommendationsystem_amd.model import NeuralCF
    torch.manual_seed(seed)
    return NeuralCF(nu, ni, 64, [128, 64, 32, 16, 8])


def _batch(nu, ni, batch, seed):
    from deeplearningrecommendationsystem_amd import synth
    gen = synth.generator(seed)
    u, i = synth.id_batch(batch, nu, ni, gen)
    u[0], i[0], u[1], i[1] = 0, 0, nu - 1, ni - 1
    return u, i, synth.labels(batch, True, gen)


def _oracle(module, u, i, y):
    from oracle import ctr_oracle as orc
    params = {k: v.detach().clone() for k, v in module.state_dict().items()}
    return orc.step("neuralcf", params, [u, i], y)


def _c_step(module, u, i, y, skip=()):
    """one training forward + backward through ctr_ncf_proj_fwd / ctr_ncf_proj_bwd, called the way ops.NcfProj calls
    them but with a workspace of exactly the size the library asks for (a sentinel behind it) and with the gradient
    buffers named in `skip` passed as null.  `module` lives on the device.  Returns prob, {parameter name: gradient}
    (names in `skip` left out) and the guard floats behind the workspace."""
    from deeplearningrecommendationsystem_amd import _lib, ops
    names = dict(module.named_parameters())
    p = {k: v.detach() for k, v in names.items()}
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
    # torch.nn.BCELoss(mean)'s gradient (ctr_bce_bwd's formula)
    pr = prob.reshape(-1)
    gprob = ((pr - yd.reshape(-1)) / (pr * (1.0 - pr)).clamp_min(1e-12) / batch).contiguous()
    grads = {k: torch.zeros_like(v) for k, v in p.items()}
    gp = {k: (None if k in skip else grads[k].data_ptr()) for k in grads}
    d, g = run._desc(), _lib.NcfProjGrad()
    g.gprob, g.ldgprob = gprob.data_ptr(), 1
    for k in range(4):
        g.layers[k].gw, g.layers[k].gb = gp[f"dnn_network.{k}.weight"], gp[f"dnn_network.{k}.bias"]
    g.g_gmf_user, g.g_gmf_item = gp["GMF_Embedding_User.weight"], gp["GMF_Embedding_Item.weight"]
    g.g_mlp_user, g.g_mlp_item = gp["MLP_Embedding_User.weight"], gp["MLP_Embedding_Item.weight"]
    g.g_proj_w, g.ld_g_proj_w, g.g_proj_b = gp["linear.weight"], grads["linear.weight"].stride(0), gp["linear.bias"]
    g.g_head_w, g.g_head_b = gp["linear2.weight"], gp["linear2.bias"]
    need = C.c_int64(0)
    assert _lib.load().ctr_ncf_proj_workspace_floats(batch, run.nu, run.ni, C.byref(need)) == 0
    ws = torch.full((need.value + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    g.workspace, g.workspace_floats = ws.data_ptr(), need.value
    g.zero_buf, g.zero_floats = None, 0
    rc = _lib.load().ctr_ncf_proj_bwd(C.byref(d), C.byref(g), _lib.stream_ptr())
    run._owns = False                       # (the call's last launch zeroed the counters: this holder dies with `run`)
    _lib.check(rc, "ctr_ncf_proj_bwd")
    torch.cuda.synchronize()
    return prob.detach().cpu(), {k: v.cpu() for k, v in grads.items() if k not in skip}, ws[need.value:].cpu()


def test_workspace_size_follows_the_single_copy_layout():
    """host only: one more sample costs 64 floats of gz0 row + 2 x 4 of slot records.  943 / 1682 rows; both batches are
    past the cap on the per-sample kernel's slabs, so the slab term cancels.  (Two bucket copies gave 136.)"""
    import __graft_entry__ as entry
    entry.build()
    from deeplearningrecommendationsystem_amd import _lib
    h = _lib.load()
    a, b = C.c_int64(0), C.c_int64(0)
    assert h.ctr_ncf_proj_workspace_floats(131072, 943, 1682, C.byref(a)) == 0
    assert h.ctr_ncf_proj_workspace_floats(65536, 943, 1682, C.byref(b)) == 0
    assert a.value - b.value == 65536 * 72


@pytest.mark.gpu
@pytest.mark.parametrize("nu,ni,batch", [(301, 407, 4096), (301, 407, 8193), (2, 3, 65536 + 5)])
def test_backward_stays_inside_a_workspace_of_exactly_the_asked_size(nu, ni, batch):
    """batch 4096 (the smallest NcfProj.supported() admits), a batch = 1 mod 16 (one live lane in the last group: its
    fifteen padding lanes write the spare row and the spare slot, the last things in their buffers), and 2 users x 3
    items at batch 65536 + 5 (every bucket spans many slot ranges and workgroups of the segment sum, every record of a
    range names a far-apart sample row): the floats behind the workspace keep their sentinel, prob and every gradient
    meet the CPU oracle"""
    module = _ncf(nu, ni, 5)
    u, i, y = _batch(nu, ni, batch, batch)
    prob_ref, _, grads_ref = _oracle(module, u, i, y)
    prob, grads, guard = _c_step(module.to(DEV), u, i, y)
    assert bool((guard == SENTINEL).all()), "ctr_ncf_proj_bwd wrote behind ctr_ncf_proj_workspace_floats floats"
    torch.testing.assert_close(prob.reshape(-1), prob_ref.reshape(-1), rtol=1e-5, atol=1e-6)
    _check_grads(grads, grads_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("nu,ni", [(5, 200), (70, 150), (128, 1), (1, 1000)])
def test_finish_parts_at_the_edges_of_the_tables(nu, ni):
    """ncfp_finish gives four row blocks of ONE table to a workgroup and every piece of their work to another part of
    the grid: a table smaller than one row block, tables whose last workgroups are ragged in different ways (70 = 64 +
    6 rows, 150 = 128 + 22), a table that fills its workgroups exactly beside a one-row table: the whole step (model
    level, as training runs it) against the CPU oracle"""
    from deeplearningrecommendationsystem_amd import ops
    from deeplearningrecommendationsystem_amd.model import neuralcf as ncf_mod
    batch = 4096 + 16 * 3 + 7
    module = _ncf(nu, ni, 29)
    u, i, y = _batch(nu, ni, batch, nu * 1000 + ni)
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


TABLES = ("GMF_Embedding_User.weight", "GMF_Embedding_Item.weight", "MLP_Embedding_User.weight", "MLP_Embedding_Item.weight")


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [TABLES, ("dnn_network.0.weight",), ("MLP_Embedding_User.weight", "GMF_Embedding_Item.weight")],
                         ids=["no_table_grads", "no_w0_grad", "one_table_of_each_kind"])
def test_finish_parts_skip_null_gradient_buffers(skip):
    """g_mlp_* / g_gmf_* / layers[0].gw are nullable in ctr_ncf_proj_grad_t: the part of ncfp_finish that owns a missing
    buffer skips it, every other gradient comes out as in the full call (same inputs; the sums through atomics differ
    by their order only, so the repository's gradient tolerance applies)"""
    nu, ni, batch = 70, 150, 4096 + 9
    module = _ncf(nu, ni, 31)
    u, i, y = _batch(nu, ni, batch, 77)
    module = module.to(DEV)
    prob_full, full, guard_full = _c_step(module, u, i, y)
    prob, part, guard = _c_step(module, u, i, y, skip=skip)
    assert bool((guard == SENTINEL).all()) and bool((guard_full == SENTINEL).all())
    torch.testing.assert_close(prob, prob_full, rtol=0, atol=0)
    assert set(part) == set(full) - set(skip)
    _check_grads(part, {k: full[k] for k in part})
