"""The later zoo models (Deep & Cross, Wide & Deep, NFM, AFM, logistic regression, AutoRec) and hipGraph replay at
the shapes bench.py and the README report: batch 65536, embedding 128, stacked width 5 * 128 + 1 = 641, deep tower
[512, 256, 128, 1], AFM attention 64, AutoRec hidden 256 over 1682 / 943 columns.  The recorded fixtures of these
models stop at batch 64 / width 8; at the script shapes the host code picks other kernels (direct-to-LDS GEMMs with
tail-column launches for 641, padded weight and activation copies, the per-workgroup LDS sum of the (V, 1) gradients,
the sorted small-table scatter: all seen in a kernel trace of the Wide & Deep and Deep & Cross steps at batch 65573
with Zipf ids), and these tests check that the MODULES wire them correctly.

Reference everywhere: oracle/ctr_oracle.py in float64, cast to float32.  Tolerances are the project's own
(bench_shapes_util.assert_step_close): prob / loss rtol 1e-5, atol 1e-6; gradients rtol 1e-4 with the floor
1e-6 + 1e-5 * max|want|, no element excluded.  One thing is not decided by a tolerance: a relu whose float64
pre-activation is below float32's rounding (seen once: NFM, batch 4160, fourth step, z = -3.7e-8).  Gradients that
miss the oracle must then meet it, at the same tolerance in every element, with relu' taken on the other side at one
or two such named positions (bench_shapes_util.assert_step_matches_oracle), or the test fails.

Seeds.  With tables drawn N(0, 0.5) the reference's own initialisation can still leave a whole tower without a
gradient: Deep & Cross, Wide & Deep and NFM put a ReLU behind the 1-unit last deep layer (model/deepcross.py:21-31,
model/widedeep.py:56-58), and for about a third of the initialisation seeds that unit is negative for every sample,
at once or after a few Adam steps.  The seeds below were chosen on the float64 oracle alone: every parameter of every
model receives a gradient in every case and at every one of the five training steps (asserted where it is used,
assert_reference_is_live).

Every GPU test carries the ``gpu`` mark itself; the one unmarked test is the CPU proof that the comparison can fail."""
import functools

import numpy as np
import pytest
import torch

import bench_shapes_util as bs
import golden_util as gu
from oracle import ctr_oracle as orc

gpu = pytest.mark.gpu
DEV = "cuda:0"
MODEL_SEED, TABLE_SEED, INPUT_SEED = 5, 2, 3
MODEL_SEEDS = {"deepcross": 2}      # seed 5 leaves Deep & Cross without a live deep tower after the first Adam step
FEATURE = list(bs.FEATURE_MODELS)


def _loss_fn():
    from deeplearningrecommendationsystem_amd.loss import BCELoss
    return BCELoss()


def _grads(module):
    return {k: p.grad.detach().cpu() for k, p in module.named_parameters()}


def _eager_step(module, inputs, y):
    """one train-loop body on the device -> (prob, loss, grads) on the host"""
    module.train()
    module.zero_grad(set_to_none=True)
    prob = module(*inputs)
    loss = _loss_fn()(prob, y)
    loss.backward()
    torch.cuda.synchronize()
    return prob.detach().cpu(), loss.detach().cpu(), _grads(module)


def _feature_module(name):
    return bs.normal_tables(bs.feature_model(name, MODEL_SEEDS.get(name, MODEL_SEED)), TABLE_SEED)


def _initial_case(name, batch, dist):
    """(seeded parameters, x, y, the float64 oracle's step on them, in float64)"""
    params = bs.cpu_params(_feature_module(name))
    x, y = bs.feature_inputs(batch, dist, INPUT_SEED)
    return params, x, y, bs.oracle_step64(name, params, [x], y)


# the one case that recurs: the one-step test, the CPU mutation test and the first of the five training steps (both
# runs) all start from it.  The 65536-sample cases are each computed once and not kept
_case_4160 = functools.lru_cache(maxsize=None)(lambda name: _initial_case(name, 4160, "uniform"))


# ---------------------------------------------------------------------------------------------------------------
# 1. one train-loop body at the script shape
# ---------------------------------------------------------------------------------------------------------------
# 65536: the benchmark's batch; 65536 + 37: a ragged last tile in every kernel, also with every sample the same
# (user, item) pair (65573 terms into one table row) and with Zipf ids, so the hot-row and LDS-sum scatter paths run
# inside a model; 4160: just above the 4096 threshold of the direct-to-LDS dW, not a multiple of 128; 1.
# What each case can see of the id tables' gradients: the floor of 1e-6 is absolute, and with uniform ids at batch
# 65536 a row of a 128-wide id table receives 1e-6 - 2e-5, so there those gradients are held to the floor only (a
# 0.1 % error in one passes; tried).  The one-pair case (rows of 5e-3 and more) and batch 1 are where a relative error
# in a table gradient shows, the Zipf case for the (V, 1) tables; every dense weight is held relatively in every case
STEP_CASES = [(65536, "uniform"), (65536 + 37, "uniform"), (65536 + 37, "onepair"), (65536 + 37, "zipf"),
              (4160, "uniform"), (1, "uniform")]


@gpu
@pytest.mark.parametrize("batch,dist", STEP_CASES)
@pytest.mark.parametrize("name", FEATURE)
def test_feature_model_script_shape_step_against_the_float64_oracle(name, batch, dist):
    params, x, y, want64 = _case_4160(name) if (batch, dist) == (4160, "uniform") else _initial_case(name, batch, dist)
    bs.assert_reference_is_live(bs.to_float32(want64), batch)
    got = _eager_step(_feature_module(name).to(DEV), [x.to(DEV)], y.to(DEV))
    bs.assert_step_matches_oracle(name, params, [x], y, got, want64)


@gpu
@pytest.mark.parametrize("transpose", [False, True])
def test_autorec_script_shape_step_against_the_float64_oracle(transpose):
    """scripts/autorec.py: AutoRec(1682, 256) on the rows of the (943, 1682) matrix; scripts/i-autorec.py:
    AutoRec(943, 256) on its transpose -- the whole matrix as the batch.  1682 and 943 are not multiples of 4: every
    operand goes through the 16-byte aligned copies of AutoRec._rows4"""
    from deeplearningrecommendationsystem_amd.model import AutoRec
    gen = torch.Generator().manual_seed(INPUT_SEED)
    x = (torch.rand(943, 1682, generator=gen) < 0.5).float()
    y = (torch.rand(943, 1682, generator=gen) < 0.5).float()
    if transpose:
        x, y = x.t().contiguous(), y.t().contiguous()
    torch.manual_seed(MODEL_SEED)
    module = AutoRec(x.shape[1], 256)
    params = bs.cpu_params(module)
    got = _eager_step(module.to(DEV), [x.to(DEV)], y.to(DEV))
    want = bs.assert_step_matches_oracle("autorec", params, [x], y, got)
    bs.assert_reference_is_live(want, x.shape[0])


def _mutations(name, params, x, y):
    """(label, params, x, y) variants that a correct comparison must reject"""
    xa = x.clone()
    xa[:, orc.COL_AGE] = 0.0          # the one-float field that puts everything after it off 16-byte alignment
    yb = y.clone()
    yb[-1] = 1.0 - yb[-1]
    out = [("age column zeroed", params, xa, y), ("last label flipped", params, x, yb)]
    if name in ("deepcross", "widedeep"):
        pc = dict(params)
        pc["movie_embedding.weight"] = params["movie_embedding.weight"].clone()
        pc["movie_embedding.weight"][:, -1] = 0.0      # stacked column 640: the one the tail-column launch carries
        out.append(("last stacked column zeroed", pc, x, y))
    return out


@pytest.mark.parametrize("name", FEATURE)
def test_the_comparison_rejects_small_mutations_of_the_step(name):
    """CPU only.  assert_step_matches_oracle -- the comparison of every GPU test here -- must reject the float64
    oracle's own step when one input column, one label or one stacked column is changed.  At batch 4160: a single
    label at batch 65536 would slip under the loss tolerance."""
    params, x, y, want64 = _case_4160(name)
    bs.assert_reference_is_live(bs.to_float32(want64), 4160)
    bs.assert_step_matches_oracle(name, params, [x], y, bs.oracle_step(name, params, [x], y), want64)   # the step itself
    for label, p, xm, ym in _mutations(name, params, x, y):
        try:
            bs.assert_step_matches_oracle(name, params, [x], y, bs.oracle_step(name, p, [xm], ym), want64)
        except AssertionError:
            continue
        pytest.fail(f"{name}: '{label}' passed the comparison")


# ---------------------------------------------------------------------------------------------------------------
# 2. graph replay == eager step, for every benchmark workload
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def restore_toggles():
    """GraphedStep switches the AccumulateGrad stream-mismatch warning off for the process; torch's default is on,
    and no test of this suite sets it otherwise, so that is what is put back: test order does not matter"""
    yield
    torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(True)


def _workload(name):
    """(factory of the module at bench.py:make_model's shape, batch builder(seed) -> (inputs, y) on the host)"""
    from deeplearningrecommendationsystem_amd import model as zoo, synth
    batch = 8192 + 37

    def ids(two_d):
        def f(seed):
            gen = synth.generator(seed)
            u, i = synth.id_batch(batch, gen=gen)
            return [u, i], synth.labels(batch, two_d, gen)
        return f

    def feats(nu=943, ni=1682):
        def f(seed):
            x, y = bs.feature_inputs(batch, "uniform", seed, nu, ni)
            return [x], y
        return f

    def seq(seed):
        gen = synth.generator(seed)
        hist, target = synth.hist_batch(1024 + 5, 100, 100_000, gen)
        return [hist, target], synth.labels(1024 + 5, True, gen)

    if name in bs.FEATURE_MODELS:
        return (lambda: _feature_module(name)), feats()
    table = {
        "mf": (lambda: zoo.MatrixFactorization(943, 1682, 64), ids(False)),
        "neuralcf": (lambda: zoo.NeuralCF(943, 1682, 64, [128, 64, 32, 16, 8]), ids(True)),
        "ffm": (lambda: zoo.FFM(43, 32), feats()),
        "pnn": (lambda: zoo.PNN(16, [256, 128, 64, 32]), feats()),
        "deepcrossing": (lambda: zoo.DeepCrossing(943, 1682, 32, [256, 128, 64, 32]), feats()),
        # tables cut to 100 000 rows: the case is about the step, not about memory
        "deepfm": (lambda: zoo.DeepFM(100_000, 100_000, [512, 256, 128, 1], 16), feats(100_000, 100_000)),
        "din": (lambda: zoo.DIN(100_000, 64), seq),
        "dien": (lambda: zoo.DIEN(100_000, 16), seq),
    }
    make, inputs = table[name]

    def seeded():
        torch.manual_seed(MODEL_SEED)
        return make()
    return seeded, inputs


def _assert_replay_equals_eager(got, want, what):
    """as test_graphed_step_survives_pool_reallocation_between_replays: the same kernels on the same data, only the
    order of atomic additions differs -- loss within 1e-6 relative, gradients rtol 1e-4 with the scaled floor"""
    loss, grads = got
    loss_e, grads_e = want
    assert abs(loss - loss_e) <= 1e-6 * max(1.0, abs(loss_e)), (what, loss, loss_e)
    assert set(grads) == set(grads_e)
    for k in grads_e:
        floor = 1e-6 + 1e-5 * float(grads_e[k].abs().max())
        torch.testing.assert_close(grads[k], grads_e[k], rtol=1e-4, atol=floor, msg=lambda m, k=k: f"{what}: grad {k}: {m}")


@gpu
@pytest.mark.parametrize("name", ["mf", "neuralcf", "ffm", "pnn", "deepcrossing", "deepfm", "din", "dien",
                                  "deepcross", "widedeep", "nfm", "afm", "lr"])
def test_graph_replay_equals_the_eager_step(name, restore_toggles):
    """What bench.py times is a GraphedStep replay.  A replay must compute what an eager step computes, see weights
    the optimizer changed in place (the padded weight copies are made by a copy_ INSIDE the captured region), and
    after load() give the step of the new batch (nothing decided from id values at capture time may be frozen in).
    The eager steps run on a twin module that receives the model's parameters before each step, because an eager
    zero_grad(set_to_none=True) on the captured module would detach .grad from the graph's static buffers.  Eager
    and replay share the host code, so the replay after the optimizer step is also held to the float64 oracle."""
    from deeplearningrecommendationsystem_amd.graph import GraphedStep
    make, batch_of = _workload(name)
    model, twin = make().to(DEV), make().to(DEV)
    (in_a, y_a), (in_b, y_b) = batch_of(INPUT_SEED), batch_of(INPUT_SEED + 1)
    assert any(not torch.equal(a, b) for a, b in zip(in_a, in_b)) and not torch.equal(y_a, y_b)
    dev_a, dev_b = ([t.to(DEV) for t in in_a], y_a.to(DEV)), ([t.to(DEV) for t in in_b], y_b.to(DEV))

    def eager(batch):
        twin.load_state_dict(model.state_dict())
        _, loss, grads = _eager_step(twin, *batch)
        return float(loss), grads

    def replay():
        loss = float(step().detach())
        return loss, _grads(model)

    # 1, 2: the captured step, replayed twice, against an eager step on the same weights
    first = eager(dev_a)
    step = GraphedStep(model, _loss_fn(), [t.clone() for t in dev_a[0]], dev_a[1].clone())
    _assert_replay_equals_eager(replay(), first, "replay 1")
    _assert_replay_equals_eager(replay(), first, "replay 2")
    # 3: the optimizer changes the parameters in place; the replay must train on the new values
    torch.optim.Adam(model.parameters(), lr=0.01).step()
    updated = eager(dev_a)
    assert abs(updated[0] - first[0]) > 1e-5 * max(1.0, abs(first[0])), "the optimizer step did not move the loss"
    got = replay()
    _assert_replay_equals_eager(got, updated, "replay after the optimizer step")
    bs.assert_step_matches_oracle(name, bs.cpu_params(model), in_a, y_a,
                                  (step.prob.detach().cpu(), step.loss.detach().cpu(), got[1]))
    # 4: another batch of the same shape through load(), then the first one again
    step.load(*dev_b)
    _assert_replay_equals_eager(replay(), eager(dev_b), "replay of the second batch")
    step.load(*dev_a)
    _assert_replay_equals_eager(replay(), updated, "replay of the first batch loaded back")


# ---------------------------------------------------------------------------------------------------------------
# 3. five consecutive training steps, checked at every step
# ---------------------------------------------------------------------------------------------------------------
STEPS = 5


def _adam_settings(name):
    """the reference scripts' optimizer: Adam lr 0.001, weight decay 1e-5 (scripts/lr.py: lr 0.05, no decay)"""
    return dict(lr=0.05, weight_decay=0.0) if name == "lr" else dict(lr=0.001, weight_decay=1e-5)


@functools.lru_cache(maxsize=None)
def _oracle_losses(name):
    """the five losses of float64 orc.step + orc.adam_update from the seeded parameters (one trajectory serves the
    eager and the graphed run)"""
    params, x, y, _ = _case_4160(name)
    p = {k: v.double().clone() for k, v in params.items()}
    m, v = ({k: torch.zeros_like(t) for k, t in p.items()} for _ in range(2))
    losses = []
    for k in range(1, STEPS + 1):
        _, loss, grads = orc.step(name, p, [x], y, dtype=torch.float64)
        losses.append(float(loss))
        for key in p:
            orc.adam_update(p[key], grads[key], m[key], v[key], k, **_adam_settings(name))
    return losses


@gpu
@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
@pytest.mark.parametrize("name", FEATURE)
def test_five_training_steps_checked_at_every_step(name, graphed, restore_toggles):
    """State that survives a step is where module code goes stale: the padded weight copies, gradient buffers,
    counters.  Five steps of forward, BCELoss, backward and Adam, eagerly and as GraphedStep + optimizer (as
    bench.py --full runs them).  Teacher-forced: at step k the step's prob, loss and gradients are compared with
    the float64 oracle AT THE MODULE'S CURRENT PARAMETERS -- a stale copy of a weight, or a gradient buffer not
    cleared, fails at k = 2.  Free-running: the five losses against five float64 oracle steps with orc.adam_update.
    (The parameters after five Adam steps are not compared: Adam turns a gradient entry near zero into a step of a
    rounding-dependent fraction of lr -- the float32 oracle's own trajectory leaves the float64 one by 0.69 * lr in
    entries of Wide & Deep's dnn_network.0.weight.)  Nothing is compared only between the two runs: a copy left
    stale by host code would be equally stale in both."""
    from deeplearningrecommendationsystem_amd.graph import GraphedStep
    batch = 4160
    start, x, y, first = _case_4160(name)
    want_losses = _oracle_losses(name)
    model = _feature_module(name).to(DEV)
    xd, yd = x.to(DEV), y.to(DEV)
    step = GraphedStep(model, _loss_fn(), [xd], yd) if graphed else None
    opt = torch.optim.Adam(model.parameters(), **_adam_settings(name))
    losses = []
    for k in range(1, STEPS + 1):
        before = bs.cpu_params(model)
        assert k > 1 or all(torch.equal(before[key], start[key]) for key in start)
        if graphed:
            step()
            torch.cuda.synchronize()
            got = step.prob.detach().cpu(), step.loss.detach().cpu(), _grads(model)
        else:
            got = _eager_step(model, [xd], yd)
        try:
            want = bs.assert_step_matches_oracle(name, before, [x], y, got, first if k == 1 else None)
        except AssertionError as e:
            raise AssertionError(f"step {k}: {e}") from None
        bs.assert_reference_is_live(want, batch)
        losses.append(float(got[1]))
        opt.step()
        after = bs.cpu_params(model)
        for key, g in want[2].items():
            if float(g.abs().max()) > 0:
                assert float((after[key] - before[key]).abs().max()) > 0, f"step {k}: {key} did not move"
    print(f"{name} losses {losses} oracle {want_losses}")
    torch.testing.assert_close(torch.tensor(losses, dtype=torch.float64), torch.tensor(want_losses, dtype=torch.float64),
                               rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------
# 4. recommendation, index check, eval
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_autorec_recommendation_ranks_like_topk_of_the_oracle_scores():
    """recommendation (top-k along dim 1, scripts/autorec.py) and i_recommendation (along dim 0,
    scripts/i-autorec.py) of a (40, 70) matrix; a tie in the oracle's scores may fall either way"""
    from deeplearningrecommendationsystem_amd.model import AutoRec
    gen = torch.Generator().manual_seed(INPUT_SEED)
    x = torch.randint(0, 3, (40, 70), generator=gen).float() * 0.5      # 1 liked, 0 disliked, 0.5 unknown
    torch.manual_seed(MODEL_SEED)
    module = AutoRec(70, 16)
    with torch.no_grad():
        scores = orc.autorec_forward(bs.cpu_params(module), x)
    module = module.to(DEV).eval()
    k = 12
    got = module.recommendation(x.to(DEV), k)
    assert got.shape == (40, k)
    gu.assert_same_ranking(got, torch.topk(scores, k, dim=1).indices.numpy(), scores.numpy(), tol=1e-5)
    got = module.i_recommendation(x.to(DEV), k)
    assert got.shape == (k, 70)
    gu.assert_same_ranking(np.ascontiguousarray(got.T), torch.topk(scores, k, dim=0).indices.t().numpy(),
                           scores.t().numpy(), tol=1e-5)


@gpu
def test_feature_model_index_out_of_range_raises_and_the_next_call_works():
    """ids arrive as a float column: 943.0 (one past the table) and -1.0"""
    module = bs.feature_model("widedeep", MODEL_SEED).to(DEV)
    module.check_index = True
    x, _ = bs.feature_inputs(64, "uniform", INPUT_SEED)
    good = module(x.to(DEV)).detach().clone()
    for col, bad in ((0, 943.0), (0, -1.0), (1, 1682.0), (1, -1.0)):
        xb = x.clone()
        xb[17, col] = bad
        with pytest.raises(IndexError):
            module(xb.to(DEV))
        assert torch.equal(module(x.to(DEV)).detach(), good), "the call after a refused one"


@gpu
@pytest.mark.parametrize("name", FEATURE)
def test_eval_under_no_grad_is_bit_identical_to_the_train_forward(name):
    module = _feature_module(name).to(DEV)
    x, _ = bs.feature_inputs(4160, "uniform", INPUT_SEED)
    xd = x.to(DEV)
    module.train()
    a = module(xd).detach().clone()
    module.eval()
    with torch.no_grad():
        b = module(xd)
    assert a.shape == (4160, 1) and torch.equal(a, b)
