"""GPU: the loss-fused backward of NeuralCF's table-row path (``ctr_ncf_proj_bwd`` with a target: csrc/ncf_proj.hip,
``ncfp_bwd_kernel<true>`` and the loss output of ``slab_reduce_role``) through ``ops.NcfProj``, and the captured step
that uses it (``graph.GraphedStep`` with ``loss.BCELoss``).

Every fused call is set against the unfused call on the same weights and batch: ``ctr_bce_fwd`` (loss and the gradient
for an upstream of 1), then the backward with that gradient.  Each backward has a training forward of its own.

The loss is held to ``step_tail_ref.bce_reference`` on the device's own ``prob`` (float64), with that file's form of
bound, ``2^-24 * mean|term| * (20 + L)``.  L counts EVERY fp32 addition on the longest path of a term to the loss word
(trees included, so the 20 is left to the two logs and the arithmetic of a term, which is what it covers there):
    groups a wave walks, one addition each (a lane sums its samples' terms)        ceil(ceil(n / 16) / waves)
    row_sum16, the wave's sixteen samples                                          4
    the workgroup's four waves, (a + b) + (c + d)                                  2
    slab second pass: a part-lane's eight accumulators take every 64th workgroup,
      at most 256 / 64 = 4 each, then at most 7 left-over workgroups on one        4 + 7
    the accumulators' tree, the half-wave shuffle, the four waves                  3 + 1 + 2
with waves = 4 * min(ceil(ceil(n / 16) / 4), 256): L = groups per wave + 23.
"""
import ctypes as C
import math

import pytest
import torch

import step_tail_ref as ref

gpu = pytest.mark.gpu
DEV = "cuda:0"
NU, NI = 50, 60
BATCHES = (5, 16, 17, 4099, 16405)
# parameters whose gradients leave ncfp_bwd through the slabs and the fixed-order second pass: bitwise reproducible.
# (dnn_network.0 and linear2.weight[:, :64] come from the table rows, through atomics, like the tables themselves.)
BITWISE = ([f"dnn_network.{k}.{w}" for k in (1, 2, 3) for w in ("weight", "bias")] +
           ["linear.weight", "linear.bias", "linear2.bias"])


def chain_length(n):
    groups = -(-n // 16)
    waves = 4 * min(-(-groups // 4), 256)
    return -(-groups // waves) + 23


def _module(seed=5, head_bias=None):
    from deeplearningrecommendationsystem_amd.model import NeuralCF
    torch.manual_seed(seed)
    module = NeuralCF(NU, NI, 64, [128, 64, 32, 16, 8])
    if head_bias is not None:
        with torch.no_grad():
            module.linear2.bias.fill_(head_bias)
    return module.to(DEV)


def _ids(n, seed):
    from deeplearningrecommendationsystem_amd import synth
    u, i = synth.id_batch(n, NU, NI, synth.generator(seed))
    return u.contiguous(), i.contiguous()


def _target(n, kind, seed):
    """-> (the tensor handed over, on the device; its values in sample order, on the host)"""
    g = torch.Generator().manual_seed(seed)
    hard = (torch.rand(n, generator=g) < 0.5).float()
    soft = torch.rand(n, generator=g)
    if kind == "hard_2d":
        return hard.view(n, 1).to(DEV), hard
    if kind == "soft_1d":
        return soft.to(DEV), soft
    assert kind == "strided"
    wide = torch.rand(n, 3, generator=g)
    wide[:, 1] = torch.where(torch.arange(n) % 2 == 0, hard, soft)
    return wide.to(DEV)[:, 1], wide[:, 1].clone()


class _Case:
    """the parameters of a module by name, and one call of either kind on them"""

    def __init__(self, module, u, i):
        from deeplearningrecommendationsystem_amd import ops
        self.p = {k: v.detach() for k, v in module.named_parameters()}
        p = self.p
        self.tables = (p["GMF_Embedding_User.weight"], p["GMF_Embedding_Item.weight"], p["MLP_Embedding_User.weight"],
                       p["MLP_Embedding_Item.weight"])
        self.hidden = [ops.Layer(p[f"dnn_network.{k}.weight"], p[f"dnn_network.{k}.bias"], ops.ACT_RELU) for k in range(4)]
        self.proj, self.head = (p["linear.weight"], p["linear.bias"]), (p["linear2.weight"], p["linear2.bias"])
        self.u, self.i = u.to(DEV), i.to(DEV)
        self.flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def forward(self):
        from deeplearningrecommendationsystem_amd import ops
        self.flag.zero_()
        run = ops.NcfProj(self.u, self.i, self.tables, self.hidden, self.proj, self.head, self.flag, True)
        prob = run.forward()
        assert prob is not None
        return run, prob

    def _grads(self):
        grads = {k: torch.zeros_like(v) for k, v in self.p.items()}
        return grads, {id(self.p[k]): g for k, g in grads.items()}

    def unfused(self, y):
        """ctr_bce_fwd, then the backward with its gradient -> (prob, loss, grads, flag), on the host"""
        from deeplearningrecommendationsystem_amd import _lib
        run, prob = self.forward()
        n = prob.numel()
        yf = y.reshape(-1)
        loss = torch.empty((), dtype=torch.float32, device=DEV)
        ws = torch.empty(256, dtype=torch.float32, device=DEV)
        ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
        gp1 = torch.empty(n, dtype=torch.float32, device=DEV)
        rc = _lib.load().ctr_bce_fwd(prob.data_ptr(), 1, yf.data_ptr(), yf.stride(0) if n > 1 else 1, n, loss.data_ptr(),
                                     ws.data_ptr(), ws.numel(), ticket.data_ptr(), gp1.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "ctr_bce_fwd")
        grads, by_id = self._grads()
        run.backward(gp1, by_id, None)
        torch.cuda.synchronize()
        return prob.detach().cpu(), float(loss), {k: g.cpu() for k, g in grads.items()}, int(self.flag)

    def fused(self, y):
        """the backward with the target; the loss word holds NaN before the call"""
        run, prob = self.forward()
        loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
        grads, by_id = self._grads()
        run.backward(None, by_id, None, target=y.reshape(-1), loss=loss)
        torch.cuda.synchronize()
        return prob.detach().cpu(), loss.cpu(), {k: g.cpu() for k, g in grads.items()}, int(self.flag)


def _check(case, y_dev, y_host, n):
    prob_u, loss_u, grads_u, flag_u = case.unfused(y_dev)
    prob_f, loss_f, grads_f, flag_f = case.fused(y_dev)
    _, loss_f2, grads_f2, _ = case.fused(y_dev)
    assert torch.equal(prob_f, prob_u) and flag_f == flag_u
    # the loss: float64 from the device's own prob
    want, _, bound_there = ref.bce_reference(prob_f, y_host)
    mean_abs = bound_there / (ref.U * (20 + ref.bce_passes(n)))
    bound = ref.U * mean_abs * (20 + chain_length(n))
    got = float(loss_f)
    print(f"n {n}: loss {got!r} float64 {want!r} |diff| {abs(got - want):.3e} bound {bound:.3e} "
          f"(unfused launch {loss_u!r})")
    assert not math.isnan(got), "the poisoned loss word was not overwritten"
    assert abs(got - want) <= bound
    assert loss_f.view(torch.int32).item() == loss_f2.view(torch.int32).item(), "the loss differs between two runs"
    # the gradients: the unfused call on the same weights and batch
    assert set(grads_f) == set(grads_u)
    for k in BITWISE:
        assert torch.equal(grads_f[k], grads_u[k]), f"{k} is not bit-identical to the unfused call"
        assert torch.equal(grads_f[k], grads_f2[k]), f"{k} differs between two runs"
    assert torch.equal(grads_f["linear2.weight"][:, 64:], grads_u["linear2.weight"][:, 64:])
    for k in grads_u:
        floor = 1e-6 + 1e-5 * float(grads_u[k].abs().max())
        torch.testing.assert_close(grads_f[k], grads_u[k], rtol=1e-4, atol=floor, msg=lambda m, k=k: f"grad {k}: {m}")
    return prob_f, grads_f


@gpu
@pytest.mark.parametrize("kind", ["hard_2d", "soft_1d", "strided"])
@pytest.mark.parametrize("n", BATCHES)
def test_fused_backward_equals_bce_launch_then_backward(n, kind):
    """5: less than one group; 17, 4099: dead lanes in the last group; 16405: more than 256 workgroups x 4 waves x 16
    samples, some waves walk two groups.  Targets: hard (B, 1), soft (B,), a strided column of a (B, 3) tensor."""
    case = _Case(_module(), *_ids(n, 100 + n))
    y_dev, y_host = _target(n, kind, 200 + n)
    if kind == "strided":
        assert y_dev.stride(0) == 3
    _, grads = _check(case, y_dev, y_host, n)
    assert all(float(g.abs().max()) > 0 for g in grads.values()), "a gradient is all zero: the case checks nothing"


@gpu
@pytest.mark.parametrize("n", [17, 4099])
@pytest.mark.parametrize("bias,p_exact", [(200.0, 1.0), (-200.0, 0.0)])
def test_saturated_prob_against_both_labels(bias, p_exact, n):
    """the head bias puts every prob at exactly 1.0f / 0.0f; against y = 0 and y = 1 (hard labels, both present) the
    terms are 0 and 100 (the clamp), p (1 - p) is 0 (the 1e-12 floor) and the gradient (p - y) / 1e-12 / n"""
    case = _Case(_module(head_bias=bias), *_ids(n, 300 + n))
    y_dev, y_host = _target(n, "hard_2d", 400 + n)
    assert 0 < int(y_host.sum()) < n
    prob, _ = _check(case, y_dev, y_host, n)
    assert bool((prob == p_exact).all())


@gpu
def test_an_id_outside_its_table_counts_in_the_loss():
    """the sample has a prob (row 0 stands in) and the loss launch counts it: same flag, loss and gradients"""
    n = 4099
    u, i = _ids(n, 77)
    u[1234] = NU
    case = _Case(_module(), u, i)
    y_dev, y_host = _target(n, "hard_2d", 78)
    _check(case, y_dev, y_host, n)
    assert int(case.flag) == 1


@gpu
def test_loss_without_target_is_refused_before_anything_is_enqueued():
    from deeplearningrecommendationsystem_amd import _lib
    n = 4099
    case = _Case(_module(), *_ids(n, 9))
    run, prob = case.forward()
    grads, by_id = case._grads()
    d, g = run._desc(), _lib.NcfProjGrad()
    gprob = torch.zeros(n, dtype=torch.float32, device=DEV)
    g.gprob, g.ldgprob = gprob.data_ptr(), 1
    for k, layer in enumerate(case.hidden):
        g.layers[k].gw, g.layers[k].gb = by_id[id(layer.weight)].data_ptr(), by_id[id(layer.bias)].data_ptr()
    gmf_u, gmf_i, mlp_u, mlp_i = case.tables
    g.g_mlp_user, g.g_mlp_item, g.g_gmf_user, g.g_gmf_item = (by_id[id(t)].data_ptr() for t in (mlp_u, mlp_i, gmf_u, gmf_i))
    g.g_proj_w, g.ld_g_proj_w, g.g_proj_b = (by_id[id(case.proj[0])].data_ptr(), by_id[id(case.proj[0])].stride(0),
                                             by_id[id(case.proj[1])].data_ptr())
    g.g_head_w, g.g_head_b = by_id[id(case.head[0])].data_ptr(), by_id[id(case.head[1])].data_ptr()
    need = C.c_int64(0)
    assert _lib.load().ctr_ncf_proj_workspace_floats(n, NU, NI, C.byref(need)) == 0
    ws = torch.full((need.value,), -12345.5, dtype=torch.float32, device=DEV)
    g.workspace, g.workspace_floats = ws.data_ptr(), need.value
    loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
    g.loss = loss.data_ptr()
    assert _lib.load().ctr_ncf_proj_bwd(C.byref(d), C.byref(g), _lib.stream_ptr()) == -1     # CTR_EINVAL
    # a target without a stride, and neither a target nor a gradient
    y = torch.zeros(n, dtype=torch.float32, device=DEV)
    g.target, g.ldtarget = y.data_ptr(), 0
    assert _lib.load().ctr_ncf_proj_bwd(C.byref(d), C.byref(g), _lib.stream_ptr()) == -1
    g.target, g.loss, g.gprob = None, None, None
    assert _lib.load().ctr_ncf_proj_bwd(C.byref(d), C.byref(g), _lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((ws == -12345.5).all()), "a refused call wrote to the workspace"
    assert math.isnan(float(loss)) and all(float(v.abs().max()) == 0 for v in grads.values())


# ---------------------------------------------------------------------------------------------------------------
# the captured step
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def restore_toggles():
    """GraphedStep switches the AccumulateGrad stream-mismatch warning off for the process; torch's default is on"""
    yield
    torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(True)


def _batch(n, seed, two_d=True):
    from deeplearningrecommendationsystem_amd import synth
    gen = synth.generator(seed)
    u, i = synth.id_batch(n, gen=gen)
    return [u.to(DEV), i.to(DEV)], synth.labels(n, two_d, gen).to(DEV)


def _eager_step(twin, model, loss_fn, inputs, y):
    """an eager step on the twin with the model's current parameters (an eager zero_grad on the captured module would
    detach .grad from the graph's buffers)"""
    twin.load_state_dict(model.state_dict())
    twin.train()
    twin.zero_grad(set_to_none=True)
    prob = twin(*inputs)
    loss = loss_fn(prob, y)
    loss.backward()
    torch.cuda.synchronize()
    return prob.detach().cpu(), float(loss.detach()), {k: p.grad.detach().cpu() for k, p in twin.named_parameters()}


def _assert_replay(step, model, want, what):
    prob_e, loss_e, grads_e = want
    loss = float(step().detach())
    torch.cuda.synchronize()
    assert torch.equal(step.prob.detach().cpu(), prob_e), f"{what}: prob"
    # the bound tests/test_gpu_models.py and test_gpu_bench_shapes.py hold a replay to
    assert abs(loss - loss_e) <= 1e-6 * max(1.0, abs(loss_e)), (what, loss, loss_e)
    for k, p in model.named_parameters():
        floor = 1e-6 + 1e-5 * float(grads_e[k].abs().max())
        torch.testing.assert_close(p.grad.detach().cpu(), grads_e[k], rtol=1e-4, atol=floor,
                                   msg=lambda m, k=k: f"{what}: grad {k}: {m}")


def _replay_equals_eager(make, loss_fn, n, deferred, two_d=True):
    from deeplearningrecommendationsystem_amd.graph import GraphedStep
    torch.manual_seed(3)
    model = make().to(DEV)
    twin = make().to(DEV)
    a, b = _batch(n, 11, two_d), _batch(n, 12, two_d)
    assert not torch.equal(a[1], b[1])
    first = _eager_step(twin, model, loss_fn, *a)
    step = GraphedStep(model, loss_fn, [t.clone() for t in a[0]], a[1].clone())
    assert (type(step.loss.grad_fn).__name__ == "_DeferredBCEFunctionBackward") == deferred
    _assert_replay(step, model, first, "replay 1")
    _assert_replay(step, model, first, "replay 2")
    torch.optim.Adam(model.parameters(), lr=0.01).step()
    updated = _eager_step(twin, model, loss_fn, *a)
    assert abs(updated[1] - first[1]) > 1e-5 * max(1.0, abs(first[1])), "the optimizer step did not move the loss"
    _assert_replay(step, model, updated, "replay after the optimizer step")
    step.load(*b)
    _assert_replay(step, model, _eager_step(twin, model, loss_fn, *b), "replay of another batch and target")
    from deeplearningrecommendationsystem_amd import loss as loss_mod
    assert loss_mod._deferral is None


def _bench_model():
    from deeplearningrecommendationsystem_amd.model import NeuralCF
    return NeuralCF(943, 1682, 64, [128, 64, 32, 16, 8])


@gpu
@pytest.mark.parametrize("n", [4096, 8192 + 5, 10500, 10500 + 13, 16405])
def test_graphed_bce_step_equals_the_eager_step(n, restore_toggles):
    """the benchmark's model.  With its 2625 table rows the table-row kernel admits a batch from 4 x 2625 = 10500 on
    (ops.few_table_rows): 4096 and 8192 + 5 are captured with today's launches, 10500 (the threshold itself), 10513
    and 16405 (waves of two groups) with the loss deferred into the backward."""
    from deeplearningrecommendationsystem_amd.loss import BCELoss
    _replay_equals_eager(_bench_model, BCELoss(), n, deferred=n >= 10500)


@gpu
def test_graphed_bce_step_with_a_flat_target(restore_toggles):
    from deeplearningrecommendationsystem_amd.loss import BCELoss
    _replay_equals_eager(_bench_model, BCELoss(), 10500 + 13, deferred=True, two_d=False)


@gpu
def test_other_losses_models_and_dtypes_take_todays_path(restore_toggles):
    """BPRLoss on the deferring model, and BCELoss on NeuralCF at the reference script's shape (the composed table-row
    path): captured with the launches of an eager step.  A float64 target is refused by BCELoss today; the captured
    step refuses it the same way and leaves no deferral state behind."""
    from deeplearningrecommendationsystem_amd import loss as loss_mod
    from deeplearningrecommendationsystem_amd.graph import GraphedStep
    from deeplearningrecommendationsystem_amd.model import NeuralCF
    _replay_equals_eager(_bench_model, loss_mod.BPRLoss(4), 5 * 2101, deferred=False)
    _replay_equals_eager(lambda: NeuralCF(943, 1682, 256, [512, 256, 128, 64, 32]), loss_mod.BCELoss(), 10500 + 13,
                         deferred=False)
    torch.manual_seed(3)
    model = _bench_model().to(DEV)
    inputs, y = _batch(10500 + 13, 11)
    with pytest.raises(ValueError, match="float32"):
        loss_mod.BCELoss()(model(*inputs), y.double())
    with pytest.raises(ValueError, match="float32"):
        GraphedStep(model, loss_mod.BCELoss(), inputs, y.double())
    assert loss_mod._deferral is None
    # and the module still trains eagerly afterwards, with a loss that is valid at once
    prob = model(*inputs)
    loss = loss_mod.BCELoss()(prob, y)
    want, _, bound = ref.bce_reference(prob, y)
    assert abs(float(loss) - want) <= bound


@gpu
def test_a_deferred_loss_refuses_any_other_upstream_gradient():
    """the placeholder is never computed from: a root gradient other than unit_grad raises in the loss, a second
    consumer of prob (its gradient added to the placeholder) raises in the model's backward"""
    from deeplearningrecommendationsystem_amd import loss as loss_mod
    torch.manual_seed(3)
    model = _bench_model().to(DEV)
    inputs, y = _batch(10500 + 13, 11)
    model.train()
    with loss_mod.deferred_bce():
        loss = loss_mod.BCELoss()(model(*inputs), y)
        assert type(loss.grad_fn).__name__ == "_DeferredBCEFunctionBackward"
        with pytest.raises(RuntimeError, match="unit_grad"):
            loss.backward()
    with loss_mod.deferred_bce():
        prob = model(*inputs)
        loss = loss_mod.BCELoss()(prob, y)
        with pytest.raises(RuntimeError, match="that loss alone"):
            torch.autograd.backward([loss, prob.sum()], [loss_mod.unit_grad(prob.device), None])
    assert loss_mod._deferral is None
    torch.cuda.synchronize()
