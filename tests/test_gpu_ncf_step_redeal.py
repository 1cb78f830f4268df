"""GPU: NeuralCF's table-row path (csrc/ncf_proj.hip) at every number of sample groups a wave of the per-sample kernels
can walk, and the slab roles (tower dW / db second pass, head fold, fused loss) in the launch they ride with.

A wave of ``ncfp_fwd_kernel`` / ``ncfp_bwd_kernel`` requests the rows of its next group and the ids of the one after
while it computes; what it requests behind its LAST group is clamped and never used.  With 1024 waves (256
workgroups) the batches below give: one group in the whole launch (1, 15, 16), two (17), three on four waves (48: the
fourth wave of the workgroup has no group), every wave exactly one group -- no wave has a real next group (16384),
one wave with two (16400), two everywhere (32768), waves with two and three and padding lanes in the very last group
(32768 + 83), and three groups on every wave plus one with four (49153).

Every batch runs twice: with the loss fused into the backward (``ncfp_bwd_kernel<true>``: through a captured
``GraphedStep`` from the smallest batch the model sends down this path, through ``ops.NcfProj`` with a target below
it) and eagerly with the gradient of prob handed in (``<false>``).  Held to the float64 oracle
(``oracle/ctr_oracle.py``) with the tolerances of tests/test_gpu_ncf_store_policy.py: prob / loss rtol 1e-5, atol
1e-6; gradients rtol 1e-4 with a floor of 1e-6 + 1e-5 max|ref|.

``ops.NcfProj.supported`` is asserted where it can hold: it admits a batch only from ``ops.few_table_rows`` on
(at least 4096 samples and four per table row: 10500 for these tables), so below that the kernels are reached through
``ops.NcfProj`` directly (as the store-policy tests do) and the shape part of the admission is asserted with a batch
that passes.
"""
import functools

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"
NU, NI = 943, 1682
TABLES = ("GMF_Embedding_User.weight", "GMF_Embedding_Item.weight", "MLP_Embedding_User.weight", "MLP_Embedding_Item.weight")
BATCHES = [1, 15, 16, 17, 48, 16384, 16400, 32768, 32768 + 83, 49153]


def _module(seed=5):
    from deeplearningrecommendationsystem_amd.model import NeuralCF
    torch.manual_seed(seed)
    return NeuralCF(NU, NI, 64, [128, 64, 32, 16, 8])


def _batch(n, seed):
    from deeplearningrecommendationsystem_amd import synth
    gen = synth.generator(seed)
    u, i = synth.id_batch(n, NU, NI, gen)
    return u.contiguous(), i.contiguous(), synth.labels(n, True, gen)


def _oracle64(params, u, i, y):
    from oracle import ctr_oracle as orc
    prob, loss, grads = orc.step("neuralcf", {k: v.detach().cpu() for k, v in params.items()}, [u, i], y,
                                 dtype=torch.float64)
    return prob.reshape(-1), loss, grads


@functools.lru_cache(maxsize=None)
def _reference(n):
    """the module, the batch and the float64 step of a batch: computed once, shared by both ways, never changed"""
    module = _module()
    u, i, y = _batch(n, 2000 + n)
    return module, (u, i, y), _oracle64(module.state_dict(), u, i, y)


def _check(prob, loss, grads, want, what="", skip=()):
    prob_ref, loss_ref, grads_ref = want
    torch.testing.assert_close(prob.reshape(-1).double(), prob_ref, rtol=1e-5, atol=1e-6, msg=lambda m: f"{what}prob: {m}")
    if loss is not None:
        torch.testing.assert_close(loss.reshape(()).double(), loss_ref.reshape(()), rtol=1e-5, atol=1e-6,
                                   msg=lambda m: f"{what}loss: {m}")
    assert set(grads) == set(grads_ref)
    for k, ref in grads_ref.items():
        if k in skip:
            continue
        floor = 1e-6 + 1e-5 * float(ref.abs().max())
        torch.testing.assert_close(grads[k].double(), ref, rtol=1e-4, atol=floor, msg=lambda m, k=k: f"{what}grad {k}: {m}")


def _admitted(n):
    from deeplearningrecommendationsystem_amd import ops
    return ops.few_table_rows(NU + NI, n)


GUARD = 3          # rows behind every per-sample buffer that must keep their fill
FILL = -7.25


class _Call:
    """one training forward + backward through ops.NcfProj on a module's parameters.  The per-sample buffers the
    wrapper owns (saved activations, prob, ranks: m + 1 rows each) are replaced by views of longer ones whose rows
    behind the spare row hold FILL.  The workspace's per-sample parts (gz0 rows, slot records) lie in front of the
    segment sums and the slabs inside one allocation: a store past their spare rows lands in what the next launch
    sums, and shows in the gradients."""

    def __init__(self, module, u, i, y):
        from deeplearningrecommendationsystem_amd import ops
        self.p = {k: v.detach().to(DEV) for k, v in module.named_parameters()}
        p = self.p
        self.tables = tuple(p[k] for k in TABLES)
        self.hidden = [ops.Layer(p[f"dnn_network.{k}.weight"], p[f"dnn_network.{k}.bias"], ops.ACT_RELU) for k in range(4)]
        self.proj, self.head = (p["linear.weight"], p["linear.bias"]), (p["linear2.weight"], p["linear2.bias"])
        self.u, self.i, self.y = u.to(DEV), i.to(DEV), y.reshape(-1).to(DEV)
        self.flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        n = self.u.numel()
        assert ops.NcfProj.supported(self.tables, self.hidden, self.proj, n if ops.few_table_rows(NU + NI, n) else 16384)

    def grad_views(self, fill):
        sizes = {k: -(-v.numel() // 4) * 4 for k, v in self.p.items()}       # every view 16-byte aligned
        flat = torch.full((sum(sizes.values()),), fill, dtype=torch.float32, device=DEV)
        grads, at = {}, 0
        for k, v in self.p.items():
            grads[k] = flat[at:at + v.numel()].view(v.shape)
            at += sizes[k]
        return flat, grads

    def forward(self, y_stride=None):
        from deeplearningrecommendationsystem_amd import ops
        self.flag.zero_()
        run = ops.NcfProj(self.u, self.i, self.tables, self.hidden, self.proj, self.head, self.flag, True)
        m = run.batch
        self.guards = []
        for k in range(3):
            rows, width = run.ys[k].shape
            ld = width if y_stride is None or k == 2 else y_stride
            big = torch.full((rows + GUARD, width), FILL, dtype=torch.float32, device=DEV) if ld == width else None
            if big is None:                      # a wide stride: the rows are far apart, nothing lies behind the last
                run.ys[k] = torch.empty((rows, ld), dtype=torch.float32, device=DEV)[:, :width]
                assert run.ys[k].stride(0) == ld
            else:
                run.ys[k] = big[:rows]
                self.guards.append(big[rows:])
        big = torch.full((m + 1 + GUARD, 1), FILL, dtype=torch.float32, device=DEV)
        run.prob_buf, run.prob = big[:m + 1], big[:m]
        self.guards.append(big[m + 1:])
        big = torch.full((2 * (m + 1 + GUARD),), -12345, dtype=torch.int32, device=DEV)
        run.ranks = big[:2 * (m + 1)]
        self.rank_guard = big[2 * (m + 1):]
        prob = run.forward()
        assert prob is not None, "ctr_ncf_proj_fwd refused the shape"
        return run, prob

    def guards_kept(self):
        return all(bool((g == FILL).all()) for g in self.guards) and bool((self.rank_guard == -12345).all())

    def run(self, fused, y_stride=None):
        """-> prob, loss (None when not fused), {name: gradient}, error flag; on the host"""
        run, prob = self.forward(y_stride)
        flat, grads = self.grad_views(float("nan"))     # poisoned: the backward's first launch clears it
        by_id = {id(self.p[k]): g for k, g in grads.items()}
        if fused:
            loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
            run.backward(None, by_id, flat, target=self.y, loss=loss)
        else:
            loss = None
            pr = prob.detach().reshape(-1)
            gprob = (pr - self.y) / torch.clamp((1.0 - pr) * pr, min=1e-12) / pr.numel()
            run.backward(gprob, by_id, flat)
        torch.cuda.synchronize()
        assert self.guards_kept(), "a row behind the spare row of a per-sample buffer was written"
        return (prob.detach().cpu(), None if loss is None else loss.cpu(), {k: g.cpu() for k, g in grads.items()},
                int(self.flag))


@pytest.fixture
def restore_toggles():
    """GraphedStep switches the AccumulateGrad stream-mismatch warning off for the process; torch's default is on"""
    yield
    torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(True)


@gpu
@pytest.mark.parametrize("n", BATCHES)
def test_loss_fused_step(n, restore_toggles):
    """ncfp_bwd_kernel<true>.  From batch 16384 on: the captured step, replayed once after its capture."""
    module, (u, i, y), want = _reference(n)
    if not _admitted(n):
        prob, loss, grads, flag = _Call(module, u, i, y).run(fused=True)
        assert flag == 0
        _check(prob, loss, grads, want)
        return
    from deeplearningrecommendationsystem_amd.graph import GraphedStep
    from deeplearningrecommendationsystem_amd.loss import BCELoss
    _Call(module, u, i, y)                      # (asserts ops.NcfProj.supported for this batch)
    model = _module().to(DEV)
    step = GraphedStep(model, BCELoss(), [u.to(DEV), i.to(DEV)], y.to(DEV))
    assert type(step.loss.grad_fn).__name__ == "_DeferredBCEFunctionBackward", "the table-row path was not captured"
    loss = step().detach()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters()}
    _check(step.prob.detach().cpu(), loss.cpu(), grads, want)
    assert all(float(g.abs().max()) > 0 for g in grads.values()), "a gradient is all zero: the case checks nothing"


@gpu
@pytest.mark.parametrize("n", BATCHES)
def test_eager_step(n):
    """ncfp_bwd_kernel<false>: the gradient of prob is formed outside (the mean BCE's, in fp32) and handed in"""
    module, (u, i, y), want = _reference(n)
    prob, _, grads, flag = _Call(module, u, i, y).run(fused=False)
    assert flag == 0
    _check(prob, None, grads, want)


@gpu
def test_bad_id_in_a_waves_last_group():
    """batch 32768 + 83 = 2054 groups on 1024 waves, eagerly.  Sample 5 of group 2049 -- the third and last group of
    wave 1 -- carries a user id outside its table; sample 3 of group 1524 -- the second and last group of wave 500 --
    an item id.  No valid id names row 0, which stands in for a bad id in the forward (the
    float64 step runs on ids clamped the same way).  The flag is raised; prob and every gradient meet the float64 step
    except row 0 of the table whose id was bad: the sample owns no slot there, and the row stays exactly zero."""
    n = 32768 + 83
    module = _module()
    u, i, y = _batch(n, 77)
    u[u == 0] = 1
    i[i == 0] = 1
    bad_u, bad_i = u.clone(), i.clone()
    su, si = 2049 * 16 + 5, 1524 * 16 + 3
    bad_u[su], bad_i[si] = NU + 2, NI
    clamped_u, clamped_i = u.clone(), i.clone()
    clamped_u[su], clamped_i[si] = 0, 0
    want = _oracle64(module.state_dict(), clamped_u, clamped_i, y)
    prob, _, grads, flag = _Call(module, bad_u, bad_i, y).run(fused=False)
    assert flag == 1
    _check(prob, None, grads, want, skip=TABLES)
    for k in TABLES:
        got, ref = grads[k], want[2][k]
        assert bool(torch.isfinite(got).all()), k
        assert float(got[0].abs().max()) == 0.0, f"{k}: row 0 moved, and only a bad id names it"
        floor = 1e-6 + 1e-5 * float(ref.abs().max())
        torch.testing.assert_close(got[1:].double(), ref[1:], rtol=1e-4, atol=floor, msg=lambda m, k=k: f"grad {k}: {m}")


@gpu
def test_last_groups_with_plain_stores():
    """a row stride of 2^26 floats for y1 and y2: ncfp_fwd_kernel<false>, whose rows keep plain stores.  Batch 17: the
    first wave runs one group, the second a group of one sample and fifteen padding lanes; each is its wave's last.  (18 rows of 256 MB each are allocated twice, 18 x 128 and 18 x 64 bytes of them touched.)"""
    module, (u, i, y), want = _reference(17)
    prob, loss, grads, flag = _Call(module, u, i, y).run(fused=True, y_stride=1 << 26)
    torch.cuda.empty_cache()
    assert flag == 0
    _check(prob, loss, grads, want)


@gpu
@pytest.mark.parametrize("n", [17, 16400])
def test_slab_roles_run_with_the_last_launch(n, monkeypatch):
    """the slab reduction and the head fold belong to launch 4 of ``phases``.  The gradient buffers hold FILL and are
    not handed over for clearing.  After launches 1 | 2 alone every gradient buffer still holds FILL and the loss
    word its NaN: those launches write the workspace only.  The test then clears the buffers itself; after launch 4
    they and the loss meet the float64 step."""
    import ctypes as C
    from deeplearningrecommendationsystem_amd import _lib
    module, (u, i, y), want = _reference(n)
    call = _Call(module, u, i, y)
    run, prob = call.forward()
    flat, grads = call.grad_views(FILL)
    loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
    lib = _lib.load()
    real = lib.ctr_ncf_proj_bwd
    seen = {}

    def in_two_calls(dref, gref, stream):
        g = gref._obj
        g.phases = 3
        rc = real(dref, gref, stream)
        torch.cuda.synchronize()
        seen["kept"] = bool((flat == FILL).all())
        seen["loss_kept"] = bool(torch.isnan(loss))
        flat.zero_()
        g.phases = 4
        return rc or real(C.byref(dref._obj), C.byref(g), stream)

    monkeypatch.setattr(lib, "ctr_ncf_proj_bwd", in_two_calls)
    run.backward(None, {id(call.p[k]): g for k, g in grads.items()}, None, target=call.y, loss=loss)
    torch.cuda.synchronize()
    assert seen["kept"], "launches 1 | 2 wrote a gradient buffer"
    assert seen["loss_kept"], "launches 1 | 2 wrote the loss word"
    assert call.guards_kept()
    _check(prob.detach().cpu(), loss.cpu(), {k: g.cpu() for k, g in grads.items()}, want)
