"""Training on a group loss end to end: a grouped ``DeviceLoader``, ``loss.BPRLoss`` / ``loss.SampledSoftmaxLoss`` and
``Trainer.train_epoch`` with and without the one-graph replay of the full batches, then ``rank_epoch``.

200 users x 150 items; 3 000 positives (u, i) with u + i even, so that there is something to rank; k = 4 negatives per
positive, batch 320: 46 full batches and an eager tail of 56 groups per epoch.  Replay and eager run the same kernels on
the same batches; the criterion on their losses is test_gpu_loader's for exactly that situation (1e-6 relative)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NU, NI, N, K, BATCH, EPOCHS = 200, 150, 3000, 4, 320, 3


@pytest.fixture
def restore_toggles():
    """GraphedStep switches the AccumulateGrad stream-mismatch warning off for the process; torch's default is on"""
    yield
    torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(True)


@functools.lru_cache(maxsize=None)
def _split():
    """(train users, train items, test users, test items) on the device and the observed set over both"""
    from deeplearningrecommendationsystem_amd.data import ObservedPairs
    gen = torch.Generator().manual_seed(17)
    users = torch.arange(NU).repeat_interleave(NI // 2)
    items = torch.arange(NI // 2).repeat(NU) * 2 + users % 2          # every pair with u + i even, once
    pick = torch.randperm(users.shape[0], generator=gen)[:N + 200]
    users, items = users[pick].to(DEV), items[pick].to(DEV)
    observed = ObservedPairs(users, items, NU, NI)
    return users[:N], items[:N], users[N:], items[N:], observed


def _loader(grouped=True, negatives=K, shuffle=True, batch=BATCH):
    from deeplearningrecommendationsystem_amd.data import DeviceLoader
    users, items, _, _, observed = _split()
    ones = torch.ones(N, 1, device=DEV)
    return DeviceLoader.pairs(users, items, ones, batch, seed=3, shuffle=shuffle, negatives=negatives, observed=observed,
                              grouped=grouped)


def _model(name):
    from deeplearningrecommendationsystem_amd import model as zoo
    torch.manual_seed(5)
    module = zoo.NeuralCF(NU, NI, 8, [16, 8]) if name == "neuralcf" else zoo.MatrixFactorization(NU, NI, 8)
    return module.to(DEV)


def _loss(name):
    from deeplearningrecommendationsystem_amd.loss import BPRLoss, SampledSoftmaxLoss
    return BPRLoss(K) if name == "bpr" else SampledSoftmaxLoss(K)


def _run(model_name, loss_name, graph):
    from deeplearningrecommendationsystem_amd.trainer import Trainer
    module = _model(model_name)
    opt = torch.optim.Adam(module.parameters(), lr=0.001, weight_decay=1e-5)      # the reference scripts' optimizer
    trainer = Trainer(module, _loss(loss_name), opt, graph=graph)
    loader = _loader()
    assert loader.grouped and len(loader) == 47 and loader.ranges[-1][1] == 280
    losses = []
    for epoch in range(EPOCHS):
        trainer.train_epoch(loader, epoch)
        torch.cuda.synchronize()
        losses.append(float(trainer.train_loss))
        assert trainer.train_rating.shape[0] == 280, "the tail batch ran last, eagerly"
        assert (trainer._graphed is not None) == graph
    loader.check_bad_index()
    return trainer, losses


@pytest.mark.parametrize("loss_name", ["bpr", "softmax"])
@pytest.mark.parametrize("model_name", ["neuralcf", "mf"])
def test_replay_and_eager_train_alike_and_the_loss_falls(model_name, loss_name, restore_toggles):
    from deeplearningrecommendationsystem_amd.data import LeaveOneOut
    eager, losses_e = _run(model_name, loss_name, False)
    replay, losses = _run(model_name, loss_name, True)
    print(model_name, loss_name, "eager", losses_e, "replay", losses)
    for epoch, (got, want) in enumerate(zip(losses, losses_e)):
        assert abs(got - want) <= 1e-6 * max(1.0, abs(want)), (model_name, loss_name, epoch, got, want)
    assert losses_e[2] < losses_e[0] and losses[2] < losses[0], "the loss of epoch 3 is below that of epoch 1"
    # sampled leave-one-out evaluation afterwards: 200 held-out positives against 9 candidates each; groups of 10 are
    # whole groups of 5 for the loss of the pass
    _, _, test_u, test_i, observed = _split()
    held_out = LeaveOneOut(test_u, test_i, observed, negatives=9, seed=2)
    held_out.check()
    for trainer in (eager, replay):
        m = trainer.rank_epoch(held_out.pairs(BATCH), negatives=9, cutoffs=(5,))
        assert trainer.predictions_rank.shape[0] == 2000 and 0.0 <= m.hr[5] <= 1.0 and 0.0 < m.mrr <= 1.0
        assert bool(torch.isfinite(trainer.rank_loss))
    print("HR@5", m.hr[5], "MRR", m.mrr)


@pytest.mark.parametrize("family", ["features", "sequences"])
def test_the_other_families_connect(family):
    """one DeepFM and one DIN step on a grouped loader of their family: 64 positives, one batch of 320"""
    from deeplearningrecommendationsystem_amd import model as zoo, synth
    from deeplearningrecommendationsystem_amd.data import DeviceLoader, FeatureAssembler, ObservedPairs
    from deeplearningrecommendationsystem_amd.trainer import Trainer
    nu, ni = synth.NUM_USERS_ML100K, synth.NUM_ITEMS_ML100K
    gen = synth.generator(3)
    users, items = (t.to(DEV) for t in synth.id_batch(64, nu, ni, gen))
    observed = ObservedPairs(users, items, nu, ni)
    ones = torch.ones(64, 1, device=DEV)
    torch.manual_seed(5)
    if family == "features":
        asm = FeatureAssembler(synth.feature_batch(nu, gen=gen)[:, 2:26].contiguous().to(DEV),
                               synth.feature_batch(ni, gen=gen)[:, 26:45].contiguous().to(DEV))
        loader = DeviceLoader.features(asm, users, items, ones, BATCH, seed=3, negatives=K, observed=observed, grouped=True)
        module = zoo.DeepFM(nu, ni, [512, 256, 128, 1], 16).to(DEV)
    else:
        hist, _ = synth.hist_batch(nu, 10, ni, gen)
        loader = DeviceLoader.sequences(hist.to(DEV), users, items, ones, BATCH, seed=3, negatives=K, observed=observed,
                                        grouped=True)
        module = zoo.DIN(ni, 64).to(DEV)
    assert loader.ranges == [(0, 320)]
    before = {k: v.detach().clone() for k, v in module.named_parameters()}
    for loss_name in ("bpr", "softmax"):
        trainer = Trainer(module, _loss(loss_name), torch.optim.Adam(module.parameters(), lr=0.001))
        trainer.train_epoch(loader, 0)
        assert bool(torch.isfinite(trainer.train_loss)) and float(trainer.train_loss) > 0.0
        assert trainer.predictions_train.shape[0] == 320
    loader.check_bad_index()
    assert any(not torch.equal(v, before[k]) for k, v in module.named_parameters()), "the step moved nothing"


def test_train_epoch_refuses_a_loader_that_breaks_the_groups():
    from deeplearningrecommendationsystem_amd.loss import BCELoss
    from deeplearningrecommendationsystem_amd.trainer import Trainer
    module = _model("mf")
    opt = torch.optim.Adam(module.parameters(), lr=0.01)
    trainer = Trainer(module, _loss("bpr"), opt)
    with pytest.raises(ValueError, match="grouped"):
        trainer.train_epoch(_loader(grouped=False), 0)                 # shuffled and ungrouped
    with pytest.raises(ValueError, match="negatives"):
        trainer.train_epoch(_loader(negatives=3, batch=320), 0)        # groups of 4 under a loss over groups of 5
    with pytest.raises(ValueError, match="multiple"):
        trainer.train_epoch(_loader(grouped=False, shuffle=False, batch=321), 0)
    # an unshuffled ungrouped loader shows whole groups, and BCE takes any loader
    trainer.train_epoch(_loader(grouped=False, shuffle=False), 0)
    assert bool(torch.isfinite(trainer.train_loss))
    Trainer(module, BCELoss(), opt).train_epoch(_loader(grouped=False), 0)
