"""helpers of tests/test_gpu_bench_shapes.py: the benchmark's module shapes, inputs that make the comparison able
to fail, the float64 oracle step and assert_step_matches_oracle, THE comparison every test of that module goes through
(the CPU mutation test included, so that what it proves holds for the GPU tests)."""
import itertools
from unittest import mock

import torch

from oracle import ctr_oracle as orc

HIDDEN = [512, 256, 128, 1]
# name -> (class, constructor arguments): exactly what bench.py:make_model builds
FEATURE_MODELS = {
    "deepcross": ("DeepCross", (943, 1682, 3, HIDDEN, 128)),
    "widedeep": ("WideDeep", (943, 1682, HIDDEN, 128)),
    "nfm": ("NFM", (943, 1682, HIDDEN, 128)),
    "afm": ("AFM", (943, 1682, 128, 64)),
    "lr": ("LogisticRegression", (943, 1682, 43)),
}


def feature_model(name, seed=0):
    from deeplearningrecommendationsystem_amd import model as zoo
    cls, args = FEATURE_MODELS[name]
    torch.manual_seed(seed)
    return getattr(zoo, cls)(*args)


def normal_tables(module, seed, std=0.5):
    """every embedding table, the (V, 1) first-order ones included, drawn from N(0, std): with the default
    initialisation prob has a standard deviation of 0.012 - 0.04 around 0.5 and parts of the network barely reach
    the output, so a wrong row would hide inside the tolerance"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.Embedding):
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * std)
    return module


def zipf_ids(batch, fields, vocab, gen):
    """rank r of a Zipf(~1) law over the rows by inverse CDF on a log grid: P(rank <= r) = log r / log V"""
    u = torch.rand(batch, fields, generator=gen, dtype=torch.float64)
    return (float(vocab) ** u - 1.0).long().clamp_(0, vocab - 1)


def feature_inputs(batch, dist="uniform", seed=0, num_users=943, num_items=1682):
    """(x (B,45), y (B,1)); ``dist``: ids uniform, every sample the same (user, item) pair, or Zipf"""
    from deeplearningrecommendationsystem_amd import synth
    gen = synth.generator(seed)
    x = synth.feature_batch(batch, num_users, num_items, gen)
    y = synth.labels(batch, True, gen)
    if dist == "onepair":
        x[:, 0], x[:, 1] = float(num_users - 1), float(num_items - 1)
    elif dist == "zipf":
        x[:, 0] = zipf_ids(batch, 1, num_users, gen)[:, 0].float()
        x[:, 1] = zipf_ids(batch, 1, num_items, gen)[:, 0].float()
    else:
        assert dist == "uniform", dist
    return x, y


def cpu_params(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def oracle_step64(key, params, inputs, y, **kw):
    """orc.step in float64: a float32 oracle drops samples at relu knife edges (see
    test_sequence_models_config5_backward_against_oracle_on_a_slice).  Returns (prob, loss, grads), float64"""
    return orc.step(key, params, inputs, y, dtype=torch.float64, **kw)


def to_float32(step):
    prob, loss, grads = step
    return prob.float(), loss.float(), {k: v.float() for k, v in grads.items()}


def oracle_step(key, params, inputs, y, **kw):
    """the float64 oracle's step cast to float32"""
    return to_float32(oracle_step64(key, params, inputs, y, **kw))


def _assert_grads_close(grads, grads_ref):
    assert set(grads) == set(grads_ref), set(grads) ^ set(grads_ref)
    for k in grads_ref:
        floor = 1e-6 + 1e-5 * float(grads_ref[k].abs().max())
        torch.testing.assert_close(grads[k], grads_ref[k], rtol=1e-4, atol=floor, msg=lambda m, k=k: f"grad {k}: {m}")


def assert_step_close(got, want):
    """(prob, loss, grads) against the reference: prob / loss rtol 1e-5, atol 1e-6; every gradient rtol 1e-4 with
    the floor 1e-6 + 1e-5 * max|want| (test_gpu_models._check_grads).  No element is excluded."""
    prob, loss, grads = got
    prob_ref, loss_ref, grads_ref = want
    assert prob.shape == prob_ref.shape, (prob.shape, prob_ref.shape)
    torch.testing.assert_close(prob, prob_ref, rtol=1e-5, atol=1e-6, msg=lambda m: f"prob: {m}")
    torch.testing.assert_close(loss, loss_ref, rtol=1e-5, atol=1e-6, msg=lambda m: f"loss: {m}")
    _assert_grads_close(grads, grads_ref)


def assert_reference_is_live(want, batch):
    """the case can fail: the scores depend on the rows and every parameter receives a gradient"""
    prob_ref, _, grads_ref = want
    if batch > 1:
        assert float(prob_ref.std()) > 0.003, "degenerate case: the scores do not depend on the rows"
    dead = [k for k, g in grads_ref.items() if float(g.abs().max()) == 0.0]
    assert not dead, f"degenerate case: no gradient reaches {dead}"


# ---------------------------------------------------------------------------------------------------------------
# relu knife edges.  relu'(z) is 0 or 1 by the sign of z, and a float32 pre-activation cannot resolve a sign below its
# own rounding error.  Seen on the MI355X: NFM, batch 4160, fourth training step, dnn_network.1 unit 87, sample 4097
# has z = -3.7e-8 in float64; the kernel's float32 sum lands on the other side, keeps that sample in the unit's
# gradient row, and the row differs from the oracle's by exactly gz * h[sample] (residual 2e-11), 1.57e-6 where the
# floor allows 1.01e-6.  One sample's term is 1/batch of the gradient scale, so this shows at 4160 and not at 65536.
# Neither side is wrong, and the tolerance is not what gives: where the gradients miss the float64 oracle, they must
# instead meet, AT THE SAME TOLERANCE AND IN EVERY ELEMENT, the float64 oracle with relu' taken on the other side at
# one or two named (relu call, sample, unit) whose |z| is below RELU_EDGE -- the same reference evaluated on the
# other side of a tie float32 cannot see.  prob and loss are never explained this way.
# RELU_EDGE is measured: the largest difference between a float32 and a float64 pre-activation of the dense towers
# at these shapes and seeds is 1.41e-6 (NFM dnn_network.0; 8.5e-7 Deep & Cross, 5.0e-7 Wide & Deep; CPU float32).
# ---------------------------------------------------------------------------------------------------------------
RELU_EDGE = 1.5e-6
# every candidate costs one oracle step.  A batch of 4160 has ten to thirty; a batch of 65536 has hundreds, each a
# sixteenth of the size against the same floor, so none can explain a miss there: above this count the miss stands
MAX_RELU_EDGES = 48


class _Relu(torch.autograd.Function):
    """relu whose derivative is taken on the other side at the flat position ``flip``"""

    @staticmethod
    def forward(ctx, z, flip):
        mask = z > 0
        if flip is not None:
            mask.view(-1)[flip] = ~mask.view(-1)[flip]
        ctx.save_for_backward(mask)
        return z.clamp_min(0)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None


def _oracle_with_relu(key, params, inputs, y, on_relu, **kw):
    """oracle_step64 with ``on_relu(call number, z) -> flat position to flip or None`` asked at every relu"""
    calls = itertools.count()
    with mock.patch.object(torch, "relu", lambda z: _Relu.apply(z, on_relu(next(calls), z))):
        return oracle_step64(key, params, inputs, y, **kw)


def relu_edge_terms(key, params, inputs, y, **kw):
    """[((relu call, flat position, z), {gradient name: float64 change when relu' there is taken on the other
    side})] for every pre-activation with |z| < RELU_EDGE in the float64 oracle; None above MAX_RELU_EDGES"""
    edges = []

    def record(call, z):
        near = (z.detach().abs().reshape(-1) < RELU_EDGE).nonzero().flatten()
        edges.extend((call, int(i), float(z.detach().reshape(-1)[i])) for i in near)
    base = _oracle_with_relu(key, params, inputs, y, record, **kw)[2]
    if len(edges) > MAX_RELU_EDGES:
        return None
    terms = []
    for call, pos, z in edges:
        flipped = _oracle_with_relu(key, params, inputs, y, lambda c, _: pos if c == call else None, **kw)[2]
        terms.append(((call, pos, z), {k: flipped[k] - base[k] for k in base}))
    return terms


def assert_step_matches_oracle(key, params, inputs, y, got, want64=None, **kw):
    """``got`` (prob, loss, grads) of the device against the float64 oracle at ``params`` (``want64``: its float64
    step, where the caller already has it) through assert_step_close.  Gradients that miss it must meet the same
    bounds against the oracle with one or two relu knife edges (above) on the other side, or the miss stands.
    Returns the oracle's (prob, loss, grads) as float32"""
    want64 = want64 if want64 is not None else oracle_step64(key, params, inputs, y, **kw)
    want = to_float32(want64)
    try:
        assert_step_close(got, want)
    except AssertionError as plain:
        assert_step_close((got[0], got[1], want[2]), want)        # a miss in prob or loss is raised here
        terms = relu_edge_terms(key, params, inputs, y, **kw)
        if terms is None:
            raise
        for n in (1, 2):
            for subset in itertools.combinations(terms, n):
                ref = {k: (g + sum(t[k] for _, t in subset)).float() for k, g in want64[2].items()}
                try:
                    _assert_grads_close(got[2], ref)
                except AssertionError:
                    continue
                print(f"{key}: gradients meet the oracle with relu' on the other side at (call, position, z) "
                      f"{[e for e, _ in subset]}; against the plain oracle: {str(plain).splitlines()[0]}")
                return want
        raise AssertionError(f"{plain}\n(and no one or two of the {len(terms)} relu pre-activations below "
                             f"{RELU_EDGE} explain it)") from None
    return want
