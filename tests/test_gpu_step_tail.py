"""GPU: the three pieces that end every training step -- ``loss.BCELoss``, ``optim.Adam`` and, in sparse mode,
``sparse.mark`` / ``sparse.adam_rows`` / ``sparse.discard`` -- at the sizes and configurations the timed step runs
them, against the float64 references and bounds of step_tail_ref.py (test_step_tail_cpu.py holds torch's own fp32
and deliberately wrong rules against the same bounds).  Every ratio is printed before it is asserted."""
import pytest
import torch

import step_tail_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _adam(hyper):
    from deeplearningrecommendationsystem_amd.optim import Adam
    return lambda params: Adam(params, **hyper)


def _check_adam(what, params, opt, refs):
    torch.cuda.synchronize()
    rp, rm, rv = ref.adam_ratios(params, opt, refs)
    print(f"Adam {what}: p {rp:.3f} m {rm:.3f} v {rv:.3f} of the bound")
    assert rp <= 1 and rm <= 1 and rv <= 1


# ------------------------------------------------------------------------------------------------------------------
# dense Adam through optim.Adam
# ------------------------------------------------------------------------------------------------------------------
def test_adam_grid_stride_passes_and_tails():
    """1 .. 1025 elements, exactly one pass of the capped grid, one more, and two passes + a partial third + a
    scalar tail, in one optimizer"""
    hyper = ref.ADAM_SETS[0]
    refs = ref.adam_reference(ref.ADAM_BIG_SIZES, 21, 3, hyper)
    params, opt = ref.run_adam(_adam(hyper), DEV, ref.ADAM_BIG_SIZES, 21, 3)
    _check_adam("big sizes", params, opt, refs)


@pytest.mark.parametrize("count", ref.ADAM_COUNTS)
def test_adam_tensor_counts_across_the_pack_limit(count):
    hyper, sizes = ref.ADAM_SETS[0], ref.adam_count_sizes(count)
    refs = ref.adam_reference(sizes, 31 + count, 3, hyper)
    params, opt = ref.run_adam(_adam(hyper), DEV, sizes, 31 + count, 3)
    _check_adam(f"{count} tensors", params, opt, refs)


@pytest.mark.parametrize("which,scale", ref.ADAM_HYPER_CASES)
def test_adam_hyper_parameter_sets_and_late_steps(which, scale):
    hyper = ref.ADAM_SETS[which]
    refs = ref.adam_reference(ref.ADAM_HYPER_SIZES, 11 + which, 6, hyper, scale, ref.ADAM_JUMP)
    params, opt = ref.run_adam(_adam(hyper), DEV, ref.ADAM_HYPER_SIZES, 11 + which, 6, scale, ref.ADAM_JUMP)
    assert all(opt.state[p]["step"] == ref.ADAM_JUMP + 2 for p in params)
    _check_adam(f"set {which} scale {scale:g}", params, opt, refs)


def test_adam_zero_gradient_without_decay_changes_nothing():
    hyper = ref.ADAM_SETS[1]
    assert hyper["weight_decay"] == 0.0
    still, moving = (t.to(DEV).requires_grad_(True) for t in ref.adam_params((4099, 1025), 41))
    start = still.detach().clone()
    opt = _adam(hyper)([moving, still])
    for step in range(1, 4):
        still.grad = torch.zeros_like(still)
        moving.grad = ref.adam_grads((1025,), 41, step)[0].to(DEV)
        opt.step()
    assert torch.equal(still.detach(), start)
    assert not bool(opt.state[still]["exp_avg"].any()) and not bool(opt.state[still]["exp_avg_sq"].any())
    assert not torch.equal(moving.detach(), ref.adam_params((4099, 1025), 41)[1].to(DEV))


def test_adam_two_parameter_groups():
    sizes, seed = (1025, 77, 4099), 43
    hypers = [dict(ref.ADAM_SETS[0]), dict(ref.ADAM_SETS[0], lr=2e-2, weight_decay=1e-2)]
    params = [t.to(DEV).requires_grad_(True) for t in ref.adam_params(sizes, seed)]
    from deeplearningrecommendationsystem_amd.optim import Adam
    opt = Adam([dict(params=params[:2]), dict(params=params[2:], lr=2e-2, weight_decay=1e-2)], **ref.ADAM_SETS[0])
    refs = [ref.AdamRef(p) for p in ref.adam_params(sizes, seed)]
    for step in range(1, 4):
        grads = ref.adam_grads(sizes, seed, step)
        for k, (p, g) in enumerate(zip(params, grads)):
            p.grad = g.to(DEV)
            refs[k].step(g, step, **hypers[k // 2])
        opt.step()
    _check_adam("two groups", params, opt, refs)


def test_adam_skips_a_parameter_without_gradient():
    sizes, seed, hyper = (1025, 77, 5), 45, ref.ADAM_SETS[0]
    params = [t.to(DEV).requires_grad_(True) for t in ref.adam_params(sizes, seed)]
    start = params[1].detach().clone()
    opt = _adam(hyper)(params)
    refs = [ref.AdamRef(p) for p in ref.adam_params(sizes, seed)]
    for step in range(1, 4):
        for k, g in enumerate(ref.adam_grads(sizes, seed, step)):
            if k != 1:
                params[k].grad = g.to(DEV)
                refs[k].step(g, step, **hyper)
        opt.step()
    assert params[1].grad is None and torch.equal(params[1].detach(), start)
    assert params[1] not in opt.state or not opt.state[params[1]]
    _check_adam("grad None", [params[0], params[2]], opt, [refs[0], refs[2]])


def test_adam_steps_over_an_empty_parameter():
    """torch.optim.Adam steps over a parameter with zero elements; so must this one (its data pointer is null)"""
    sizes, hyper = (5, 0, 1025), ref.ADAM_SETS[0]
    refs = ref.adam_reference(sizes, 47, 3, hyper)
    params, opt = ref.run_adam(_adam(hyper), DEV, sizes, 47, 3)
    assert params[1].numel() == 0
    _check_adam("empty parameter", params, opt, refs)
    only = torch.empty(0, device=DEV, requires_grad=True)      # and an optimizer that holds nothing else
    only.grad = torch.empty(0, device=DEV)
    _adam(hyper)([only]).step()


# ------------------------------------------------------------------------------------------------------------------
# row-wise Adam, marking and discard, at op level
# ------------------------------------------------------------------------------------------------------------------
def _table(p):
    from deeplearningrecommendationsystem_amd import sparse
    p = p.to(DEV).clone()
    p._ctr_sparse = sparse.SparseRows(p)
    return p, p._ctr_sparse


def _is_clean(st):
    return not bool(torch.stack([st.grad.any(), st.flags.any(), st.count.any(), st.done.any()]).any())


def _untouched(vocab, rows):
    mask = torch.ones(vocab, dtype=torch.bool)
    mask[rows] = False
    return mask.to(DEV)


def _rows_ratios(what, p, m, v, r):
    got = (ref.ratio(p, r.p, r.tol_p), ref.ratio(m, r.m, r.tol_m), ref.ratio(v, r.v, r.tol_v))
    print(f"row-wise Adam {what}: p {got[0]:.3f} m {got[1]:.3f} v {got[2]:.3f} of the bound")
    assert got[0] <= 1 and got[1] <= 1 and got[2] <= 1


def _adam_rows(items, step, hyper=ref.ROWS_HYPER):
    from deeplearningrecommendationsystem_amd import sparse
    sparse.adam_rows(items, hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"], step)


@pytest.mark.parametrize("which", range(len(ref.ROWS_HYPERS)))
@pytest.mark.parametrize("dim", ref.ROWS_DIMS)
def test_rows_adam_lane_counts_and_global_step(dim, which):
    """dwordx4 rows of 1, 3, 4, 5 and 16 lanes and the one-lane-per-element path at dim 1 and 3; three steps whose
    row sets differ, rows 0 and vocab-1 sitting out the second"""
    from deeplearningrecommendationsystem_amd import sparse
    hyper = ref.ROWS_HYPERS[which]
    p0, m0, v0, batches = ref.rows_case(dim)
    (p, st), m, v = _table(p0), m0.to(DEV), v0.to(DEV)
    r = ref.AdamRef(p0, m0, v0)
    for step, (ids, vals) in enumerate(batches, 1):
        st.grad.index_add_(0, ids.to(DEV), vals.to(DEV))
        g = st.grad.to("cpu", copy=True)                                   # the fp32 sums as the device formed them
        sparse.mark([(p, ids.to(DEV))])
        rows = torch.unique(ids)
        assert torch.equal(st.pending()[0].cpu(), rows)
        before = [t.clone() for t in (p, m, v)]
        _adam_rows([(p, m, v)], step, hyper)
        r.step(g, step, rows=rows, **hyper)
        rest = _untouched(ref.ROWS_VOCAB, rows)
        for got, was in zip((p, m, v), before):
            assert torch.equal(got[rest], was[rest])
            assert not torch.equal(got[~rest], was[~rest])
        assert _is_clean(st)
    _rows_ratios(f"dim {dim} betas {hyper['betas']}", p, m, v, r)


@pytest.mark.parametrize("vocab,dim,distinct,nids", [(70000, 16, 40000, 40000), (150000, 1, 140000, 300000)])
def test_rows_adam_pending_list_longer_than_one_pass(vocab, dim, distinct, nids):
    """160 000 dwordx4 lanes and 140 000 scalar lanes against the launch's 131 072 threads; 300 000 ids against the
    262 144 one pass of the marking kernel covers"""
    from deeplearningrecommendationsystem_amd import sparse
    g = torch.Generator().manual_seed(vocab)
    p0 = torch.randn(vocab, dim, generator=g)
    rows = torch.randperm(vocab, generator=g)[:distinct]
    ids = torch.cat([rows, rows[torch.randint(0, distinct, (nids - distinct,), generator=g)]])
    vals = torch.randn(distinct, dim, generator=g)
    (p, st), m, v = _table(p0), torch.zeros(vocab, dim, device=DEV), torch.zeros(vocab, dim, device=DEV)
    st.grad.index_add_(0, rows.to(DEV), vals.to(DEV))
    grad = st.grad.to("cpu", copy=True)
    sparse.mark([(p, ids.to(DEV))])
    listed = st.pending()[0].cpu()
    assert listed.numel() == distinct and torch.equal(listed, torch.sort(rows).values)
    _adam_rows([(p, m, v)], 1)
    r = ref.AdamRef(p0)
    r.step(grad, 1, rows=listed, **ref.ROWS_HYPER)
    rest = _untouched(vocab, listed)
    assert torch.equal(p[rest], p0.to(DEV)[rest]) and not bool(m[rest].any()) and not bool(v[rest].any())
    assert _is_clean(st)
    _rows_ratios(f"vocab {vocab} dim {dim}", p, m, v, r)


def test_rows_mark_id_forms_list_each_valid_row_once():
    from deeplearningrecommendationsystem_amd import sparse
    vocab, batch = 997, 5000
    g = torch.Generator().manual_seed(51)
    p, st = _table(torch.zeros(vocab, 4))

    def draw():
        return torch.randint(0, vocab, (batch,), generator=g)

    def listed_is(*id_sets):
        ids = torch.cat([t.reshape(-1).long() for t in id_sets])
        want = torch.unique(ids[(ids >= 0) & (ids < vocab)])
        rows = st.pending()[0].cpu()
        assert rows.numel() == int(st.count.item()) == want.numel() and torch.equal(rows, want)
        flags = torch.zeros(vocab, dtype=torch.int32)
        flags[want] = 1
        assert torch.equal(st.flags.cpu(), flags)
        sparse.discard([p])
        assert _is_clean(st)

    ids = draw()                                                   # int64, contiguous
    sparse.mark([(p, ids.to(DEV))])
    listed_is(ids)
    mat = torch.randint(0, vocab, (batch, 5), generator=g)         # int64 column of a (B, 5) matrix
    col = mat.to(DEV)[:, 2]
    assert col.stride(0) == 5
    sparse.mark([(p, col)])
    listed_is(mat[:, 2])
    feat = torch.rand(batch, 45, generator=g) * 2000 - 500         # float32 column of a (B, 45) matrix
    feat[:, 1] = draw().float()
    sparse.mark([(p, feat.to(DEV)[:, 1])])
    listed_is(feat[:, 1])
    for as_float in (False, True):                                 # -1 and vocab mixed in: they mark nothing
        ids = draw()
        ids[::3], ids[1::7] = -1, vocab
        sparse.mark([(p, ids.float().to(DEV) if as_float else ids.to(DEV))])
        listed_is(ids)
    ids = draw()                                                   # one row is half of all ids
    ids[::2] = 123
    sparse.mark([(p, ids.to(DEV))])
    listed_is(ids)
    a, b = draw()[:700], draw()[:900]                              # two calls before one step, overlapping rows
    b[:300] = a[:300]
    sparse.mark([(p, a.to(DEV))])
    sparse.mark([(p, b.to(DEV))])
    listed_is(a, b)
    sparse.mark([(p, a.to(DEV)), (p, b.to(DEV))])                  # two jobs of one call name the same table
    listed_is(a, b)
    only = torch.tensor([-1, vocab, -5])                           # nothing valid at all
    sparse.mark([(p, only.to(DEV))])
    listed_is(only)


@pytest.mark.parametrize("count", [32, 33, 52, 65])
def test_rows_table_counts_across_the_job_limit(count):
    """one mark / adam_rows / discard call over more tables than one launch takes (32): half (V,16), half (V,1) as
    the 26-field models have them, distinct vocabularies and row sets"""
    from deeplearningrecommendationsystem_amd import sparse
    g = torch.Generator().manual_seed(count)
    tables = []
    for i in range(count):
        vocab, dim = 200 + 7 * i, 16 if i % 2 == 0 else 1
        p0 = torch.randn(vocab, dim, generator=g)
        p, st = _table(p0)
        tables.append(dict(vocab=vocab, dim=dim, p=p, st=st, m=torch.zeros_like(p), v=torch.zeros_like(p),
                           ref=ref.AdamRef(p0)))

    def scatter_and_mark():
        jobs = []
        for i, t in enumerate(tables):
            n = 150 + 3 * i
            ids = torch.randint(0, t["vocab"], (n,), generator=g)
            t["st"].grad.index_add_(0, ids.to(DEV), torch.randn(n, t["dim"], generator=g).to(DEV))
            t["ids"], t["g"] = ids, t["st"].grad.to("cpu", copy=True)
            jobs.append((t["p"], ids.to(DEV)))
        sparse.mark(jobs)
        for t in tables:
            assert torch.equal(t["st"].pending()[0].cpu(), torch.unique(t["ids"]))

    def step(number):
        before = [[x.clone() for x in (t["p"], t["m"], t["v"])] for t in tables]
        _adam_rows([(t["p"], t["m"], t["v"]) for t in tables], number)
        for t, was in zip(tables, before):
            rows = torch.unique(t["ids"])
            t["ref"].step(t["g"], number, rows=rows, **ref.ROWS_HYPER)
            rest = _untouched(t["vocab"], rows)
            for got, old in zip((t["p"], t["m"], t["v"]), was):
                assert torch.equal(got[rest], old[rest])
            assert _is_clean(t["st"])

    scatter_and_mark()
    step(1)
    scatter_and_mark()                                             # a batch that zero_grad drops
    before = [[x.clone() for x in (t["p"], t["m"], t["v"])] for t in tables]
    sparse.discard([t["p"] for t in tables])
    for t, was in zip(tables, before):
        assert all(torch.equal(got, old) for got, old in zip((t["p"], t["m"], t["v"]), was))
        assert _is_clean(t["st"])
    scatter_and_mark()                                             # the following step updates only its own rows
    step(2)
    worst = [0.0, 0.0, 0.0]
    for t in tables:
        r = t["ref"]
        got = (ref.ratio(t["p"], r.p, r.tol_p), ref.ratio(t["m"], r.m, r.tol_m), ref.ratio(t["v"], r.v, r.tol_v))
        worst = [w if w >= x else x for w, x in zip(worst, got)]
    print(f"row-wise Adam {count} tables: p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f} of the bound")
    assert worst[0] <= 1 and worst[1] <= 1 and worst[2] <= 1


# ------------------------------------------------------------------------------------------------------------------
# BCELoss
# ------------------------------------------------------------------------------------------------------------------
def _bce(prob, target, backward=None):
    """loss (a device scalar), with ``backward(loss)`` run if given"""
    from deeplearningrecommendationsystem_amd.loss import BCELoss
    loss = BCELoss()(prob, target)
    if backward is not None:
        backward(loss)
    return loss.detach()


@pytest.mark.parametrize("n", ref.BCE_SIZES)
def test_bce_loss_and_gradient_against_float64(n):
    from deeplearningrecommendationsystem_amd.loss import unit_grad
    p, y = ref.bce_inputs(n)
    want, grad, tol = ref.bce_reference(p, y)
    y_d = y.view(n, 1).to(DEV)
    a, b, c = (p.view(n, 1).to(DEV).requires_grad_(True) for _ in range(3))
    loss = _bce(a, y_d, lambda l: l.backward())                     # autograd's own ones: the scaling kernel
    rl, rg = abs(float(loss) - want) / tol, ref.bce_grad_ratio(a.grad, grad)
    print(f"BCELoss n {n}: loss {rl:.3f} of the bound, gradient {rg:.3f} ({8 * rg:.2f} * 2^-24)")
    assert rl <= 1 and rg <= 1
    assert a.grad.shape == (n, 1)
    unit = _bce(b, y_d, lambda l: l.backward(unit_grad(torch.device(DEV))))   # THE 1.0: the forward's own gradient
    assert torch.equal(unit, loss) and torch.equal(b.grad, a.grad)
    scaled = _bce(c, y_d, lambda l: (-2.5 * l).backward())
    rs = ref.bce_grad_ratio(c.grad, ref.bce_reference(p, y, gloss=-2.5)[1])
    print(f"BCELoss n {n}: gradient under -2.5 {rs:.3f}")
    assert torch.equal(scaled, loss) and rs <= 1
    assert torch.equal(_bce(p.view(n, 1).to(DEV), y_d), loss)       # no gradient wanted: the same loss bits


@pytest.mark.parametrize("n", [257, 262145])
def test_bce_columns_of_wider_buffers(n):
    """the probability as column 1 of an (n, 3) buffer, the target as column 0 of an (n, 2) buffer"""
    p, y = ref.bce_inputs(n)
    want, grad, tol = ref.bce_reference(p, y)
    wide_p = torch.full((n, 3), 7.0)           # a neighbour read by mistake gives log(negative) = nan
    wide_p[:, 1] = p
    wide_y = torch.full((n, 2), float("nan"))
    wide_y[:, 0] = y
    wide_p, wide_y = wide_p.to(DEV).requires_grad_(True), wide_y.to(DEV)
    prob, target = wide_p[:, 1:2], wide_y[:, 0:1]
    assert prob.stride(0) == 3 and target.stride(0) == 2
    assert prob.reshape(-1).stride(0) == 3 and target.reshape(-1).stride(0) == 2   # what the loss hands the kernel
    loss = _bce(prob, target, lambda l: l.backward())
    rl, rg = abs(float(loss) - want) / tol, ref.bce_grad_ratio(wide_p.grad[:, 1], grad)
    print(f"BCELoss columns n {n}: loss {rl:.3f} of the bound, gradient {rg:.3f}")
    assert rl <= 1 and rg <= 1
    assert not bool(wide_p.grad[:, 0].any()) and not bool(wide_p.grad[:, 2].any())
    flat = p.view(n, 1).to(DEV).requires_grad_(True)
    same = _bce(flat, y.view(n, 1).to(DEV), lambda l: l.backward())
    assert torch.equal(same, loss) and torch.equal(flat.grad[:, 0], wide_p.grad[:, 1])


def test_bce_ticket_rearms_across_changing_grids():
    """the fixed-order reduction is bitwise reproducible, whatever grids ran in between"""
    losses = {}
    for n in (600001, 37, 262145, 1, 600001):
        p, y = ref.bce_inputs(n)
        loss = _bce(p.view(n, 1).to(DEV), y.view(n, 1).to(DEV))
        want, _, tol = ref.bce_reference(p, y)
        assert abs(float(loss) - want) <= tol
        losses.setdefault(n, []).append(loss)
    assert torch.equal(*losses[600001])
