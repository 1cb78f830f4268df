"""The device-side mini-batch loader (csrc/loader.hip, data/loader.py) and the trainer methods that drive it.

References.  The shuffled index: loader_numpy.perm, a numpy restatement written from the definition in the kernel
file's header comment; integers, compared element for element.  A batch: plain host indexing of the sources with that
index (``users[idx]``, ``FeatureAssembler.feature(users[idx], items[idx])``, ``history[users[idx]]``); the loader only
copies, so every comparison is bit-equality.  An epoch of training: ``Trainer.train_loop`` called on those
host-indexed batches -- the same kernels on the same batches, so only the order of atomic additions may differ, and the
tolerances are those of test_gpu_bench_shapes._assert_replay_equals_eager for exactly that situation, unchanged:
loss within 1e-6 relative, tensors rtol 1e-4 with the floor 1e-6 + 1e-5 * max|want|."""
import os

import numpy as np
import pytest
import torch

import loader_numpy as ln

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NU, NI = 943, 1682
SEED = 20


@pytest.fixture
def restore_toggles():
    """GraphedStep switches the AccumulateGrad stream-mismatch warning off for the process; torch's default is on"""
    yield
    torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(True)


def _sources(n, hist_len=10, hist_rows=NU, seed=1):
    """host tensors of n samples: ids, a rating of each trailing shape, the assembler's tables, a (U, L) history"""
    from deeplearningrecommendationsystem_amd import synth
    gen = synth.generator(seed)
    users, items = synth.id_batch(n, min(NU, hist_rows), NI, gen)
    hist, _ = synth.hist_batch(hist_rows, hist_len, NI, gen)
    return dict(users=users, items=items, y1=synth.labels(n, False, gen), y2=synth.labels(n, True, gen),
                ufeat=synth.feature_batch(NU, gen=gen)[:, 2:26].contiguous(),
                ifeat=synth.feature_batch(NI, gen=gen)[:, 26:45].contiguous(), hist=hist)


def _loader(family, src, batch_size, **kw):
    """(loader, host reference: idx (numpy) -> (args, rating) on the host, bit for bit what the batch must hold)"""
    from deeplearningrecommendationsystem_amd.data import DeviceLoader, FeatureAssembler
    d = {k: v.to(DEV) for k, v in src.items()}
    if family == "mf":
        loader = DeviceLoader.pairs(d["users"], d["items"], d["y1"], batch_size, **kw)
        return loader, lambda idx: ((src["users"][idx], src["items"][idx]), src["y1"][idx])
    if family == "pairs":
        loader = DeviceLoader.pairs(d["users"], d["items"], d["y2"], batch_size, **kw)
        return loader, lambda idx: ((src["users"][idx], src["items"][idx]), src["y2"][idx])
    if family == "features":
        asm = FeatureAssembler(d["ufeat"], d["ifeat"])
        loader = DeviceLoader.features(asm, d["users"], d["items"], d["y2"], batch_size, **kw)
        return loader, lambda idx: ((asm.feature(d["users"][idx], d["items"][idx]).cpu(),), src["y2"][idx])
    assert family == "sequences"
    loader = DeviceLoader.sequences(d["hist"], d["users"], d["items"], d["y2"], batch_size, **kw)
    return loader, lambda idx: ((src["hist"][src["users"][idx]], src["items"][idx]), src["y2"][idx])


def _index(loader, epoch, first, count, shuffle=True):
    pos = np.arange(first, first + count)
    return ln.perm(loader.seed, epoch, pos, loader.num_samples) if shuffle else pos


# ---------------------------------------------------------------------------------------------------------------
# 1. the permutation on the device
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 65537, 2 ** 20 + 3])
def test_loader_indices_equal_the_numpy_restatement(n):
    src = _sources(n)
    loader, _ = _loader("mf", src, 1000, seed=SEED)
    for epoch in (0, 1, 5, 1 << 40):
        for first, count in ((0, n), (0, 1), (n - 1, 1), (n // 3, min(n - n // 3, 4099)), (5, 0)):
            got = loader.indices(epoch, first, count).cpu().numpy()
            assert np.array_equal(got, _index(loader, epoch, first, count)), (n, epoch, first, count)
    assert np.array_equal(loader.indices(3, 0, n, shuffle=False).cpu().numpy(), np.arange(n))
    other, _ = _loader("mf", src, 1000, seed=SEED + 1)
    assert not torch.equal(other.indices(0), loader.indices(0))


# ---------------------------------------------------------------------------------------------------------------
# 2. every batch of every family, bit for bit
# ---------------------------------------------------------------------------------------------------------------
def _assert_epoch_is_host_indexing(loader, ref, epoch, shuffle):
    """every batch of this rank equals host indexing with the restated permutation; returns the indices drawn"""
    seen = []
    static = loader.static_batch()
    ranges = ln.batch_ranges(loader.num_samples, loader.batch_size, loader.drop_last, loader.rank, loader.world)
    assert loader.ranges == ranges and len(loader) == len(ranges)
    batches = 0
    for (args, rating), (first, count) in zip(loader.epoch(epoch), ranges):
        idx = _index(loader, epoch, first, count, shuffle)
        want_args, want_rating = ref(torch.from_numpy(idx))
        assert rating.shape == want_rating.shape and torch.equal(rating.cpu(), want_rating), (epoch, first)
        assert len(args) == len(want_args)
        for got, want in zip(args, want_args):
            assert got.dtype == want.dtype and got.shape == want.shape and got.is_contiguous()
            assert torch.equal(got.cpu(), want), (epoch, first, count)
        if count == loader.batch_size and batches < (loader.num_samples // loader.batch_size) // loader.world:
            assert rating is static[1] and all(a is b for a, b in zip(args, static[0])), "full batches: static buffers"
        else:
            assert static is None or rating.data_ptr() != static[1].data_ptr(), "the tail has buffers of its own"
        seen.append(idx)
        batches += 1
    assert batches == len(ranges)
    return np.concatenate(seen) if seen else np.zeros(0, dtype=np.int64)


FAMILIES = ["mf", "pairs", "features", "sequences"]
# (n, batch_size, history length): several batches and a tail; batch_size >= n; one sample; one batch exactly
SHAPES = [(6921, 2048, 10), (37, 64, 1), (1, 8, 130), (4096, 1024, 130), (777, 100, 1), (5000, 333, 7)]


@pytest.mark.parametrize("n,batch_size,hist_len", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_every_batch_is_bit_equal_to_host_indexing(family, n, batch_size, hist_len):
    src = _sources(n, hist_len, hist_rows=NU if hist_len != 130 else 61)
    for shuffle in (True, False):
        loader, ref = _loader(family, src, batch_size, seed=SEED, shuffle=shuffle)
        for epoch in (0, 3):
            seen = _assert_epoch_is_host_indexing(loader, ref, epoch, shuffle)
            assert np.array_equal(np.sort(seen), np.arange(n)), "every sample exactly once per epoch"
            if not shuffle:
                assert np.array_equal(seen, np.arange(n))
        loader.check_bad_index()
    # the loader's setting can be overridden per pass (what an evaluation pass does)
    args, rating = next(iter(loader.epoch(0, shuffle=True)))
    count = min(n, batch_size)
    assert torch.equal(rating.cpu(), ref(torch.from_numpy(_index(loader, 0, 0, count)))[1])
    # drop_last: the full batches only
    loader, ref = _loader(family, src, batch_size, seed=SEED, drop_last=True)
    seen = _assert_epoch_is_host_indexing(loader, ref, 1, True)
    assert len(seen) == (n // batch_size) * batch_size and len(np.unique(seen)) == len(seen)


@pytest.mark.parametrize("family", ["pairs", "sequences"])
def test_ranks_partition_one_permutation(family):
    n, batch_size, world = 6921, 512, 3
    src = _sources(n)
    for drop_last in (False, True):
        seen = []
        for rank in range(world):
            loader, ref = _loader(family, src, batch_size, seed=SEED, drop_last=drop_last, rank=rank, world=world)
            assert loader.num_rank_samples == sum(c for _, c in loader.ranges)
            seen.append(_assert_epoch_is_host_indexing(loader, ref, 2, True))
        assert len({sum(1 for _, c in ln.batch_ranges(n, batch_size, drop_last, r, world) if c == batch_size)
                    for r in range(world)}) == 1
        every = np.concatenate(seen)
        assert len(np.unique(every)) == len(every)
        assert len(every) == ((n // batch_size) // world * world * batch_size if drop_last else n)


def test_a_bad_id_in_a_join_raises_and_the_next_epoch_works():
    n = 500
    for family, key, bad in (("features", "users", NU), ("features", "items", -1), ("features", "items", NI),
                             ("sequences", "users", -3), ("sequences", "users", NU)):
        src = _sources(n)
        src[key] = src[key].clone()
        src[key][123] = bad
        loader, _ = _loader(family, src, 128, seed=SEED)
        for _ in loader.epoch(0):
            pass
        with pytest.raises(IndexError):
            loader.check_bad_index()
        loader.check_bad_index()        # the flag was cleared
        # the bad row is clamped to row 0 of its table; the id columns of the feature matrix keep the id itself
        pos = int(np.nonzero(ln.perm(SEED, 0, np.arange(n), n) == 123)[0][0])
        batches = list(ln.batch_ranges(n, 128))
        k = next(j for j, (first, count) in enumerate(batches) if first <= pos < first + count)
        for j, (args, _) in enumerate(loader.epoch(0)):
            if j == k:
                row = args[0][pos - batches[k][0]].cpu()
        if family == "features":
            u, i = int(src["users"][123]), int(src["items"][123])
            want = torch.cat([torch.tensor([float(u), float(i)]), src["ufeat"][u if 0 <= u < NU else 0],
                              src["ifeat"][i if 0 <= i < NI else 0]])
        else:
            want = src["hist"][0]
        assert torch.equal(row, want), (family, key, bad)
        with pytest.raises(IndexError):
            loader.check_bad_index()


def test_cpu_tensors_are_refused():
    from deeplearningrecommendationsystem_amd._lib import CtrHipError
    from deeplearningrecommendationsystem_amd.data import DeviceLoader
    src = _sources(64)
    with pytest.raises(CtrHipError):
        DeviceLoader.pairs(src["users"].to(DEV), src["items"], src["y2"].to(DEV), 16)
    with pytest.raises(ValueError):
        DeviceLoader.pairs(src["users"].to(DEV), src["items"][:-1].to(DEV), src["y2"].to(DEV), 16)
    with pytest.raises(ValueError):
        DeviceLoader.pairs(src["users"].to(DEV).int(), src["items"].to(DEV), src["y2"].to(DEV), 16)


# ---------------------------------------------------------------------------------------------------------------
# 3. train_epoch against explicit steps
# ---------------------------------------------------------------------------------------------------------------
def _model(name):
    from deeplearningrecommendationsystem_amd import model as zoo
    torch.manual_seed(5)
    if name == "neuralcf":
        return zoo.NeuralCF(NU, NI, 64, [128, 64, 32, 16, 8]), "pairs"
    if name == "deepfm":
        return zoo.DeepFM(NU, NI, [512, 256, 128, 1], 16), "features"
    return zoo.DIN(NI, 64), "sequences"


def _trainer(module, graph=False):
    from deeplearningrecommendationsystem_amd.loss import BCELoss
    from deeplearningrecommendationsystem_amd.trainer import Trainer
    opt = torch.optim.Adam(module.parameters(), lr=0.001, weight_decay=1e-5)   # the reference scripts' optimizer
    return Trainer(module, BCELoss(), opt, graph=graph)


def _assert_close_as_replay_and_eager(loss, loss_e, tensors, tensors_e, what):
    """test_gpu_bench_shapes._assert_replay_equals_eager, applied to the parameters after an epoch"""
    assert abs(loss - loss_e) <= 1e-6 * max(1.0, abs(loss_e)), (what, loss, loss_e)
    assert set(tensors) == set(tensors_e)
    for k in tensors_e:
        floor = 1e-6 + 1e-5 * float(tensors_e[k].abs().max())
        torch.testing.assert_close(tensors[k], tensors_e[k], rtol=1e-4, atol=floor, msg=lambda m, k=k: f"{what}: {k}: {m}")


def _params(module):
    return {k: v.detach().cpu().clone() for k, v in module.named_parameters()}


EPOCHS, N_TRAIN, B_TRAIN = 3, 3 * 2048 + 777, 2048


def _explicit_epochs(name):
    """[(parameters after the epoch, sample-weighted mean loss)]: Trainer.train_loop on batches indexed on the host with
    the restated permutation"""
    module, family = _model(name)
    module = module.to(DEV)
    trainer = _trainer(module)
    src = _sources(N_TRAIN)
    loader, ref = _loader(family, src, B_TRAIN, seed=SEED)
    out = []
    for epoch in range(EPOCHS):
        total = 0.0
        for first, count in ln.batch_ranges(N_TRAIN, B_TRAIN):
            args, rating = ref(torch.from_numpy(ln.perm(SEED, epoch, np.arange(first, first + count), N_TRAIN)))
            trainer.train_loop(*[t.to(DEV) for t in args], train_rating=rating.to(DEV))
            total += float(trainer.train_loss) * count
        out.append((_params(module), total / N_TRAIN))
    return out


@pytest.mark.parametrize("name", ["neuralcf", "deepfm", "din"])
def test_train_epoch_equals_train_loop_on_host_indexed_batches(name, restore_toggles):
    want = _explicit_epochs(name)
    moved = max(float((want[-1][0][k] - want[0][0][k]).abs().max()) for k in want[0][0])
    assert moved > 1e-4, "the explicit run did not train"
    for graph in (False, True):
        module, family = _model(name)
        module = module.to(DEV)
        trainer = _trainer(module, graph=graph)
        loader, _ = _loader(family, _sources(N_TRAIN), B_TRAIN, seed=SEED)
        assert len(loader) == 4 and loader.ranges[-1][1] == 777
        captured = None
        for epoch in range(EPOCHS):
            trainer.train_epoch(loader, epoch)
            torch.cuda.synchronize()
            what = f"{name} {'graph' if graph else 'eager'} epoch {epoch}"
            print(what, "loss", float(trainer.train_loss), "explicit", want[epoch][1])
            _assert_close_as_replay_and_eager(float(trainer.train_loss), want[epoch][1], _params(module), want[epoch][0],
                                              what)
            assert trainer.predictions_train.shape[0] == 777 and trainer.train_rating.shape[0] == 777
            if graph:
                # one capture for all epochs: the eager tail step must not have replaced it
                assert trainer._graphed is not None
                captured = captured or (trainer._graphed, trainer._graphed.graph)
                assert trainer._graphed is captured[0] and trainer._graphed.graph is captured[1], what
            else:
                assert trainer._graphed is None
        loader.check_bad_index()


# ---------------------------------------------------------------------------------------------------------------
# 4. valid_epoch / test_epoch and the report
# ---------------------------------------------------------------------------------------------------------------
def _metric_lines(text):
    return [line for line in text.splitlines() if " - " in line and "Loss" not in line]


@pytest.mark.parametrize("name", ["neuralcf", "deepfm", "din"])
def test_valid_epoch_gathers_what_valid_loop_gives(name, capsys):
    n, batch_size = 5000, 1024
    module, family = _model(name)
    module = module.to(DEV)
    trainer, whole = _trainer(module), _trainer(module)
    src = _sources(n, seed=2)
    loader, ref = _loader(family, src, batch_size, seed=SEED)         # a shuffling loader: the pass must not shuffle
    trainer.valid_epoch(loader)
    trainer.test_epoch(loader)
    args, rating = ref(torch.arange(n))
    args, rating = [t.to(DEV) for t in args], rating.to(DEV)
    pieces = []
    for first, count in ln.batch_ranges(n, batch_size):
        whole.valid_loop(*[t[first:first + count] for t in args], valid_rating=rating[first:first + count])
        pieces.append(whole.predictions_valid.clone())
    assert trainer.predictions_valid.shape == (n, 1) and torch.equal(trainer.predictions_valid, torch.cat(pieces))
    assert torch.equal(trainer.valid_rating, rating) and torch.equal(trainer.predictions_test, trainer.predictions_valid)
    whole.valid_loop(*args, valid_rating=rating)
    whole.test_loop(*args, test_rating=rating)
    print("valid loss", float(trainer.valid_loss), "valid_loop on the whole set", float(whole.valid_loss))
    torch.testing.assert_close(trainer.valid_loss, whole.valid_loss, rtol=1e-5, atol=0.0)
    torch.testing.assert_close(trainer.test_loss, whole.test_loss, rtol=1e-5, atol=0.0)
    assert not module.training
    # the report: the same metrics from the gathered predictions as from valid_loop on the whole set
    for t in (trainer, whole):
        t.predictions_train, t.train_rating, t.train_loss = whole.predictions_valid, rating, whole.valid_loss
    capsys.readouterr()
    trainer.model_eval(0)
    got = capsys.readouterr().out
    whole.model_eval(0)
    want = capsys.readouterr().out
    assert len(_metric_lines(want)) == 15 and _metric_lines(got) == _metric_lines(want)


def test_minibatch_script_runs(monkeypatch, capsys):
    """scripts/minibatch.py on its default arguments: three models, several batches and a tail each"""
    import runpy
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.setattr(sys, "argv", ["minibatch.py"])
    monkeypatch.syspath_prepend(os.path.join(root, "scripts"))
    runpy.run_path(os.path.join(root, "scripts", "minibatch.py"), run_name="__main__")
    out = capsys.readouterr().out
    assert out.count("Epoch 3:") == 3 and "Training Loss" in out and "ROC AUC Score" in out
    for name in ("NeuralCF", "DeepFM", "DIN"):
        assert f"==== {name}:" in out
