"""GPU: every dispatch arm of the feature-interaction kernels against the float64 references of tests/interact_ref.py.

csrc/ffm_fused.hip, csrc/fields.hip, csrc/rows_sum.hip and the LDS-tile kernels of csrc/interact.hip choose a template
instance or a code path from the embedding width, the field count, alignment and batch size.  Each case below is on
one of those arms; its comment shows the arithmetic (grid cap, samples per workgroup, LDS bytes, tile size) taken from
the entry point.  The tolerances and the inputs are those of tests/interact_ref.py, where tests/test_interact_ref_cpu.py
shows that they reject small mutations of the references.  Every comparison prints its worst |err| / bound."""
import ctypes as C

import pytest
import torch

import interact_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def ops():
    from deeplearningrecommendationsystem_amd import ops as o
    return o


def _lib():
    from deeplearningrecommendationsystem_amd import _lib as L
    return L


def _dev(t):
    if t is None:
        return None
    if isinstance(t, (list, tuple)):
        return [_dev(v) for v in t]
    return t.to(DEV)


def _filled(rows, cols, value=float("nan")):
    return torch.full((rows, cols), value, dtype=torch.float32, device=DEV)


def _flag():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------
# ctr_ffm_fused_fwd / ctr_ffm_fused_bwd
# ---------------------------------------------------------------------------------------------------------------
def _fused_step(ops, case, want_user=True, want_item=True):
    x, tables, user1, item1, lin_w, lin_b, gprob = case
    batch, dim = x.shape[0], tables[0].shape[1]
    xd, td, u1, i1, w, b, gp = _dev(x), _dev(tables), _dev(user1), _dev(item1), _dev(lin_w), _dev(lin_b), _dev(gprob)
    emb, prob, flag = _filled(batch, 12 * dim), _filled(batch, 1), _flag()
    ops.ffm_fused_fwd(xd, td, u1, i1, w, b, emb, prob, flag)
    gu = torch.zeros_like(u1) if want_user else None
    gi = torch.zeros_like(i1) if want_item else None
    gw, gb, gemb = torch.zeros_like(w), torch.zeros_like(b), _filled(batch, 12 * dim)
    ops.ffm_fused_bwd(xd, emb, user1.shape[0], item1.shape[0], w, prob, gp, gu, gi, gw, gb, gemb)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    grads = {"gemb": gemb, "glin_w": gw, "glin_b": gb}
    if want_user:
        grads["guser1"] = gu
    if want_item:
        grads["gitem1"] = gi
    return emb, prob, grads


def _check_fused(case, emb, prob, grads):
    x, tables, user1, item1, lin_w, lin_b, gprob = case
    want = ref.ffm_ref(x, tables, user1, item1, lin_w, lin_b, gprob=gprob)
    ref.check_ffm_emb(emb, want)
    ref.check_prob(prob, want["prob"])
    ref.check_ffm_bwd(grads, want)
    return want


# LPR = dim / 4 lanes own a sample, a wave covers 64 / LPR samples, a workgroup of 4 waves 256 / LPR:
#   dim  8: LPR  2, 32 per wave, 128 per workgroup; batch 37 = 32 + 5: wave 1 has 5 of its 32 slots live
#   dim 16: LPR  4, 16 per wave,  64 per workgroup; batch 67 = 64 + 3: workgroup 1, wave 0 has 3 of 16 live
#   dim 32: LPR  8,  8 per wave,  32 per workgroup; batch 1: one slot of one wave
#   dim 64: LPR 16,  4 per wave,  16 per workgroup; batch 19 = 16 + 3: workgroup 1, wave 0 has 3 of 4 live; the
#           backward holds PER = ceil(43 / 16) = 3 weight slots per lane and folds the 4 sample slots in two steps
@pytest.mark.parametrize("dim,batch", ref.FFM_FUSED_CASES)
def test_ffm_fused_every_width(ops, dim, batch):
    """sample 0 has no genre (its two multi-hot vectors are exactly zero), sample batch // 2 a non-trivial real age"""
    case = ref.ffm_case(dim, batch, ref.ffm_seed(dim, batch))
    x = case[0]
    assert float(x[0, 26:45].abs().sum()) == 0.0 and 0.0 < float(x[batch // 2, 2]) < 1.0
    emb, prob, grads = _fused_step(ops, case)
    _check_fused(case, emb, prob, grads)
    assert bool((emb[0, 6 * dim:8 * dim] == 0).all())


def test_ffm_fused_grid_stride_loops(ops):
    """dim 64 (16 samples per workgroup) at batch 32787 = 2048 * 16 + 16 + 3.  Forward: grid = min(ceil(32787 / 16),
    256 * 8) = 2048 workgroups cover 32768 samples, the second pass has workgroup 0 full and workgroup 1 with one wave
    of 3 live slots.  Backward: grid = min(2050, 1024) = 1024 workgroups x 16 = 16384 per pass: three passes, the
    weight / bias gradients from 1024 partials."""
    dim, batch = 64, 32787
    assert batch == 2048 * 16 + 16 + 3
    case = ref.ffm_case(dim, batch, 4242)
    emb, prob, grads = _fused_step(ops, case)
    _check_fused(case, emb, prob, grads)


def test_ffm_fused_strided_operands(ops):
    """x a column slice of a 48-wide buffer (ldx = 48 > 45), emb / gemb slices of wider 16-byte aligned buffers (lde =
    ldg = 12 * 16 + 8, first column 4), prob / gprob columns of (B, 2): the columns beside each output stay untouched"""
    dim, batch = 16, 67
    case = ref.ffm_case(dim, batch, 515)
    x, tables, user1, item1, lin_w, lin_b, gprob = case
    xbuf = _filled(batch, 48, SENTINEL)
    xbuf[:, 2:47] = x.to(DEV)
    xd = xbuf[:, 2:47]
    ebuf, gbuf = _filled(batch, 12 * dim + 8, SENTINEL), _filled(batch, 12 * dim + 8, SENTINEL)
    emb, gemb = ebuf[:, 4:4 + 12 * dim], gbuf[:, 4:4 + 12 * dim]
    assert emb.data_ptr() % 16 == 0 and emb.stride(0) % 4 == 0 and xd.stride(0) == 48
    pbuf = _filled(batch, 2, SENTINEL)
    pbuf[:, 1] = gprob.view(-1).to(DEV)
    prob, gp = pbuf[:, 0:1], pbuf[:, 1:2]
    td, u1, i1, w, b = _dev(tables), _dev(user1), _dev(item1), _dev(lin_w), _dev(lin_b)
    flag = _flag()
    ops.ffm_fused_fwd(xd, td, u1, i1, w, b, emb, prob, flag)
    gu, gi, gw, gb = torch.zeros_like(u1), torch.zeros_like(i1), torch.zeros_like(w), torch.zeros_like(b)
    ops.ffm_fused_bwd(xd, emb, user1.shape[0], item1.shape[0], w, prob, gp, gu, gi, gw, gb, gemb)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    _check_fused(case, emb, prob, {"gemb": gemb, "guser1": gu, "gitem1": gi, "glin_w": gw, "glin_b": gb})
    side = torch.full((batch, 4), SENTINEL)
    for buf in (ebuf, gbuf):
        assert torch.equal(buf[:, :4].cpu(), side) and torch.equal(buf[:, 4 + 12 * dim:].cpu(), side)
    assert torch.equal(pbuf[:, 1].cpu(), gprob.view(-1))
    assert torch.equal(xbuf[:, :2].cpu(), side[:, :2]) and torch.equal(xbuf[:, 47:].cpu(), side[:, :1])


@pytest.mark.parametrize("missing", ["guser1", "gitem1"])
def test_ffm_fused_bwd_without_one_first_order_gradient(ops, missing):
    """guser1 / gitem1 NULL: the other gradients are what they were"""
    case = ref.ffm_case(32, 45, 616)
    emb, prob, grads = _fused_step(ops, case, want_user=missing != "guser1", want_item=missing != "gitem1")
    assert missing not in grads and len(grads) == 4
    _check_fused(case, emb, prob, grads)


def test_ffm_fused_bwd_without_the_linear_gradients(ops):
    """glin_w / glin_b NULL, through the C entry point (ops always passes both): the one asked for is right, the
    other's buffer keeps its pre-fill"""
    L = _lib()
    dim, batch = 16, 67
    case = ref.ffm_case(dim, batch, 717)
    x, tables, user1, item1, lin_w, lin_b, gprob = case
    want = ref.ffm_ref(x, tables, user1, item1, lin_w, lin_b, gprob=gprob)
    xd, td, u1, i1, w, b, gp = _dev(x), _dev(tables), _dev(user1), _dev(item1), _dev(lin_w), _dev(lin_b), _dev(gprob)
    emb, prob = _filled(batch, 12 * dim), _filled(batch, 1)
    ops.ffm_fused_fwd(xd, td, u1, i1, w, b, emb, prob)
    for with_w, with_b in ((False, True), (True, False), (False, False)):
        gu, gi, gw, gb = torch.zeros_like(u1), torch.zeros_like(i1), torch.zeros_like(w), torch.zeros_like(b)
        gemb = _filled(batch, 12 * dim)
        ws = torch.full((1024 * 44,), SENTINEL, dtype=torch.float32, device=DEV)
        rc = L.load().ctr_ffm_fused_bwd(xd.data_ptr(), xd.stride(0), batch, dim, emb.data_ptr(), emb.stride(0),
                                        user1.shape[0], item1.shape[0], w.data_ptr(), prob.data_ptr(), 1, gp.data_ptr(), 1,
                                        gu.data_ptr(), gi.data_ptr(), gw.data_ptr() if with_w else None,
                                        gb.data_ptr() if with_b else None, gemb.data_ptr(), gemb.stride(0),
                                        ws.data_ptr(), ws.numel(), L.stream_ptr())
        L.check(rc, "ctr_ffm_fused_bwd")
        torch.cuda.synchronize()
        got = {"gemb": gemb, "guser1": gu, "gitem1": gi}
        if with_w:
            got["glin_w"] = gw
        else:
            assert bool((gw == 0).all())
        if with_b:
            got["glin_b"] = gb
        else:
            assert bool((gb == 0).all())
        ref.check_ffm_bwd(got, want)


def test_ffm_fused_fwd_bad_ids(ops):
    """one user id == num_users, one item id -1: the flag is set, those rows of emb are row 0 bit for bit, the rest of
    the batch is untouched by it; a second, clean call leaves a cleared flag cleared"""
    dim, batch, nu, ni = 16, 67, 50, 70
    x, tables, user1, item1, lin_w, lin_b, _ = ref.ffm_case(dim, batch, 818, nu, ni)
    bad = x.clone()
    bad[3, 0], bad[5, 1] = float(nu), -1.0
    td, u1, i1, w, b = _dev(tables), _dev(user1), _dev(item1), _dev(lin_w), _dev(lin_b)
    emb, prob, flag = _filled(batch, 12 * dim), _filled(batch, 1), _flag()
    ops.ffm_fused_fwd(_dev(bad), td, u1, i1, w, b, emb, prob, flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 1
    emb = emb.cpu()
    for f, row in ((8, 3), (9, 3), (10, 5), (11, 5)):
        assert torch.equal(emb[row, f * dim:(f + 1) * dim], tables[f][0])
    fixed = bad.clone()
    fixed[3, 0], fixed[5, 1] = 0.0, 0.0                            # what the clamp stands for
    want = ref.ffm_ref(fixed, tables, user1, item1, lin_w, lin_b)
    ref.check_ffm_emb(emb, want)
    ref.check_prob(prob, want["prob"])
    flag.zero_()
    emb2, prob2 = _filled(batch, 12 * dim), _filled(batch, 1)
    ops.ffm_fused_fwd(_dev(x), td, u1, i1, w, b, emb2, prob2, flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    ref.check_ffm_emb(emb2, ref.ffm_ref(x, tables, user1, item1, lin_w, lin_b))


def _ffm_specs(ops, tables, dim):
    """the embedding stage's description of the 12 vectors (model/ffm.py, FFM._specs)"""
    L = _lib()
    specs = []
    for f, ((kind, col, rows), t) in enumerate(zip(ref.FFM_SOURCE, tables)):
        if kind == "bag":
            specs.append(ops.FieldSpec(L.FIELD_BAG, dim, f * dim, table=t, src_col=col, bag_size=rows))
        else:
            specs.append(ops.FieldSpec(L.FIELD_ID_F32, dim, f * dim, table=t, src_col=col))
    return specs


def test_ffm_fused_and_two_launch_forward_agree_bit_for_bit_on_emb(ops):
    """csrc/ffm_fused.hip's header: skipping the zero-weight rows leaves the in-order FMA chain's bits as they are, so
    the fused kernel and embed_fwd write the same operand; ffm_head_fwd on it gives the fused probability within the
    probability tolerance"""
    dim, batch = 32, 67
    case = ref.ffm_case(dim, batch, 919)
    x, tables, user1, item1, lin_w, lin_b, gprob = case
    xd, td, u1, i1, w, b = _dev(x), _dev(tables), _dev(user1), _dev(item1), _dev(lin_w), _dev(lin_b)
    emb, prob = _filled(batch, 12 * dim), _filled(batch, 1)
    ops.ffm_fused_fwd(xd, td, u1, i1, w, b, emb, prob)
    emb2, prob2 = _filled(batch, 12 * dim), _filled(batch, 1)
    ops.embed_fwd(_ffm_specs(ops, td, dim), xd, batch, emb2)
    ops.ffm_head_fwd(emb2, 12, dim, ref.FFM_PAIRS, xd, u1, i1, w, b, prob2)
    torch.cuda.synchronize()
    assert torch.equal(emb.cpu(), emb2.cpu())
    want = ref.ffm_ref(x, tables, user1, item1, lin_w, lin_b)
    ref.check_prob(prob, want["prob"])
    ref.check_prob(prob2, want["prob"])


# ---------------------------------------------------------------------------------------------------------------
# ctr_ffm_head_fwd / ctr_ffm_head_bwd (LDS tiles)
# ---------------------------------------------------------------------------------------------------------------
def _head_case(nvec, dim, batch, seed, offset=0, pad=0):
    """an arbitrary (B, nvec * dim) operand N(0, 0.25^2) -- at column ``offset`` of a buffer ``pad`` columns wider --
    and FFM's feature matrix and head parameters"""
    x, _, user1, item1, lin_w, lin_b, gprob = ref.ffm_case(8, batch, seed)
    gen = torch.Generator().manual_seed(seed)
    buf = 0.25 * torch.randn(batch, nvec * dim + pad, generator=gen)
    return buf, offset, x, user1, item1, lin_w, lin_b, gprob


def _head_step(ops, case, nvec, dim, pairs):
    buf, offset, x, user1, item1, lin_w, lin_b, gprob = case
    batch = x.shape[0]
    emb = buf.to(DEV)[:, offset:offset + nvec * dim]
    xd, u1, i1, w, b, gp = _dev(x), _dev(user1), _dev(item1), _dev(lin_w), _dev(lin_b), _dev(gprob)
    prob, flag = _filled(batch, 1), _flag()
    ops.ffm_head_fwd(emb, nvec, dim, pairs, xd, u1, i1, w, b, prob, flag)
    gu, gi, gw, gb = torch.zeros_like(u1), torch.zeros_like(i1), torch.zeros_like(w), torch.zeros_like(b)
    gemb = _filled(batch, nvec * dim)
    ops.ffm_head_bwd(emb, nvec, dim, pairs, xd, u1, i1, w, b, prob, gp, gu, gi, gw, gb, gemb)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    want = ref.ffm_head_ref(buf[:, offset:offset + nvec * dim], nvec, dim, pairs, x, user1, item1, lin_w, lin_b, gprob)
    ref.check_prob(prob, want["prob"])
    got = {"gemb": gemb, "guser1": gu, "gitem1": gi, "glin_w": gw, "glin_b": gb}
    ref.check_ffm_bwd(got, want)
    return emb, got, want


# make_geometry: VEC = 4 when dim % 4 == 0, the base pointer is 16-byte aligned and lde % 4 == 0, else 1; a vector
# takes dim + VEC floats of LDS, a sample nvec of them plus `extra`; tile = min(64, 12288 / that).  Batch 131 = 2 * 64
# + 3: three tiles, the last of 3 samples.
#   dim  4: VEC 4, row 12 * 8 = 96, forward (96 + 15) -> 64 (capped), backward (96 + 60) -> 64
#   dim  5: VEC 1 (5 % 4 != 0), row 12 * 6 = 72 -> 64
#   dim 12: VEC 4, row 12 * 16 = 192, forward 12288 / 207 = 59, backward 12288 / 252 = 48: 131 = 2 * 59 + 13 = 2 * 48 + 35
#   dim 16 at column 1 of a wider buffer: the base pointer is 4 bytes off 16 -> VEC 1, row 12 * 17 = 204 -> 56 / 46
@pytest.mark.parametrize("dim,offset", [(4, 0), (5, 0), (12, 0), (16, 1)])
def test_ffm_head_widths_and_staging(ops, dim, offset):
    case = _head_case(12, dim, 131, 2000 + dim, offset, 4 if offset else 0)
    emb, _, _ = _head_step(ops, case, 12, dim, ref.FFM_PAIRS)
    aligned = emb.data_ptr() % 16 == 0 and emb.stride(0) % 4 == 0 and dim % 4 == 0
    assert aligned == (dim in (4, 12))


def test_ffm_head_wide_vectors_and_grid_stride(ops):
    """dim 128: a vector takes 132 floats, a sample 12 * 132 = 1584; forward 12288 / (1584 + 15) = 7 samples per tile,
    backward 12288 / (1584 + 15 + 2 + 43) = 7.  Batch 14346 = 2048 * 7 + 7 + 3 = 2050 tiles: the forward's 2048
    workgroups make two passes, the backward's 1024 (the cap with a workspace) three."""
    assert 12288 // (1584 + 15) == 7 and 12288 // (1584 + 60) == 7 and 14346 == 2048 * 7 + 7 + 3
    _head_step(ops, _head_case(12, 128, 14346, 2128), 12, 128, ref.FFM_PAIRS)


@pytest.mark.parametrize("nvec", [5, 6])
def test_ffm_head_another_pair_list(ops, nvec):
    """pairs [(0, 1), (0, 1), (3, 2), (4, 0)]: a repeated pair and a > b -- make_pairs' start / partner tables for a list
    that is not FFM's.  With nvec = 5 every vector has a partner; with nvec = 6 the last one has none, and its
    gradient is exactly zero."""
    pairs = [(0, 1), (0, 1), (3, 2), (4, 0)]
    _, got, _ = _head_step(ops, _head_case(nvec, 8, 70, 2300 + nvec), nvec, 8, pairs)
    if nvec == 6:
        assert bool((got["gemb"][:, 5 * 8:] == 0).all())


@pytest.mark.parametrize("pairs", [[(0, 1), (2, 2)], [(0, 1), (1, 5)], [(0, 1), (-1, 2)], [(0, 1)] * 65],
                         ids=["a_equals_b", "index_is_nvec", "negative_index", "65_pairs"])
def test_ffm_head_bad_pair_lists_are_refused(ops, pairs):
    """an error from both entry points, and nothing written"""
    L = _lib()
    nvec, dim, batch = 5, 8, 9
    buf, _, x, user1, item1, lin_w, lin_b, gprob = _head_case(nvec, dim, batch, 2400)
    emb, xd, u1, i1, w, b, gp = _dev(buf), _dev(x), _dev(user1), _dev(item1), _dev(lin_w), _dev(lin_b), _dev(gprob)
    prob = _filled(batch, 1, SENTINEL)
    with pytest.raises(L.CtrHipError):
        ops.ffm_head_fwd(emb, nvec, dim, pairs, xd, u1, i1, w, b, prob)
    outs = [torch.full_like(t, SENTINEL) for t in (u1, i1, w, b, emb)]
    good = torch.full((batch, 1), 0.5, device=DEV)
    with pytest.raises(L.CtrHipError):
        ops.ffm_head_bwd(emb, nvec, dim, pairs, xd, u1, i1, w, b, good, gp, *outs)
    torch.cuda.synchronize()
    for t in [prob] + outs:
        assert bool((t == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------
# ops.allpairs_fwd / allpairs_bwd: ctr_fields_pairs_fwd's strips, ctr_allpairs_*'s tiles
# ---------------------------------------------------------------------------------------------------------------
# forward, nvec > 8 and dim in {8, 16, 32, 64} (strip kernel): a sample takes stride = nvec * dim + pad floats with
# stride % 64 == 16, a wave 64 / (dim / 4) samples; two waves per workgroup while 2 * per_wave <= 56 KB.
# backward: ctr_fields_pairs_bwd refuses everything but 26 x 16, ctr_allpairs_bwd takes tiles of
# min(64, 12288 / (nvec * (dim + 4) + npairs)) samples.
#   (26, 64,    70): stride 1680, per_wave 4 * 1680 * 4 = 26880 B, two waves = 53760 B > 48 KB: the raised limit;
#                    backward tile 12288 / (26 * 68 + 325) = 5
#   (32, 64,    37): stride 2064, per_wave 33024 B, 2 * that > 56 KB: one wave; backward tile 12288 / (2176 + 496) = 4
#   (32, 64, 16389): the same, 4 samples per workgroup, grid min(4098, 4096): workgroups 0 and 1 make a second pass
#                    (16389 = 4096 * 4 + 5); backward 4098 tiles on 2048 workgroups: three passes
#   (32,  8,   100): LPR 2, 32 samples per wave, stride 272; backward tile 12288 / (384 + 496) = 13
#   ( 9, 16,    65): LPR 4, 16 per wave, 32 per workgroup: 65 = 2 * 32 + 1; backward tile 12288 / (180 + 36) = 56
#   (32, 256,    3): dim 256 is not a strip width: ctr_allpairs_fwd, 12288 / (32 * 260) = 1 sample per tile, backward
#                    12288 / (8320 + 496) = 1
@pytest.mark.parametrize("nvec,dim,batch", ref.PAIRS_CASES)
def test_allpairs_arms(ops, nvec, dim, batch):
    emb, gp = ref.pairs_case(nvec, dim, batch)
    want = ref.pairs_ref(emb, nvec, dim, gp)
    npairs = nvec * (nvec - 1) // 2
    ed = emb.to(DEV)
    out = _filled(batch, npairs)
    ops.allpairs_fwd(ed, nvec, dim, out=out)
    gemb = _filled(batch, nvec * dim)
    ops.allpairs_bwd(ed, nvec, dim, gp.to(DEV), gemb, accumulate=False)
    torch.cuda.synchronize()
    ref.check_sum(out, want["prod"], want["prod_n"], want["prod_mass"], "prod")
    ref.check_sum(gemb, want["gemb"], want["gemb_n"], want["gemb_mass"], "gemb")


@pytest.mark.parametrize("dim", [8, 12, 64])
@pytest.mark.parametrize("nvec", [8, 9, 32, 33, 64])
def test_allpairs_forward_and_backward_admit_the_same_shapes(ops, nvec, dim):
    """forward and backward either both succeed or both raise ValueError: up to 32 vectors both run, above (what only
    the strip forward could do) both refuse before anything is enqueued"""
    batch, npairs = 3, nvec * (nvec - 1) // 2
    emb, gp = ref.pairs_case(nvec, dim, batch)
    ed, out, gemb = emb.to(DEV), _filled(batch, npairs, SENTINEL), _filled(batch, nvec * dim, SENTINEL)
    outcome = []
    for call in (lambda: ops.allpairs_fwd(ed, nvec, dim, out=out),
                 lambda: ops.allpairs_bwd(ed, nvec, dim, gp.to(DEV), gemb, accumulate=False)):
        try:
            call()
            outcome.append("ok")
        except ValueError:
            outcome.append("refused")
    torch.cuda.synchronize()
    assert outcome[0] == outcome[1], outcome
    assert outcome[0] == ("ok" if nvec <= 32 else "refused")
    if outcome[0] == "ok":
        want = ref.pairs_ref(emb, nvec, dim, gp)
        ref.check_sum(out, want["prod"], want["prod_n"], want["prod_mass"], "prod")
        ref.check_sum(gemb, want["gemb"], want["gemb_n"], want["gemb_mass"], "gemb")
    else:
        assert bool((out == SENTINEL).all()) and bool((gemb == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------
# ctr_fields_fm_fwd / ctr_fields_fm_bwd
# ---------------------------------------------------------------------------------------------------------------
def _fields_fwd(ops, idx, tables, first, bias, emb=None, fm=None):
    batch, nf = idx.shape
    dim = tables[0].shape[1]
    emb = _filled(batch, nf * dim) if emb is None else emb
    fm = _filled(batch, 1) if fm is None else fm
    flag = _flag()
    ops.fields_fm_fwd(idx, _dev(tables), _dev(first), _dev(bias), emb, fm, flag)
    torch.cuda.synchronize()
    return emb, fm, int(flag.item())


def _fields_bwd(ops, idx, tables, emb, gdeep, gfm, want_first=True, want_bias=True, fill=0.0):
    dim = tables[0].shape[1]
    gtables = [torch.zeros_like(t, device=DEV) for t in tables]
    gfirst = [torch.full((t.shape[0], 1), fill, device=DEV) for t in tables] if want_first else None
    gbias = torch.full((1,), fill, device=DEV) if want_bias else None
    ops.fields_fm_bwd(idx, [t.shape[0] for t in tables], dim, emb, gdeep, gfm, gtables, gfirst, gbias)
    torch.cuda.synchronize()
    return gtables, gfirst, gbias


# forward: dim / 4 lanes own a sample, 256 / (dim / 4) samples per workgroup, fields in chunks of 8 with the next
# chunk's ids in flight; backward: dim lanes own a sample, 256 / dim per workgroup.  Width 16, batch 67 = 64 + 3
# (forward: workgroup 1 has 3 live samples; backward: 16 per workgroup, the fifth has 3):
#   1 field: every id lane past the first aliases field 0;  8: exactly one chunk;  9: one field in the second chunk;
#   16: two full chunks;  32: CTR_MAX_FIELDS, four chunks
#   2 fields x 64, batch 65555 = 4096 * 16 + 16 + 3: forward 16 per workgroup, grid min(4098, 256 * 16): two passes;
#       backward 4 per workgroup, grid min(16389, 2048): 9 passes (65555 = 8 * 8192 + 19), gbias from 2048 partials;
#       half the batch sits on one row of each table
#   5 fields at widths 8 and 32: LPR 2 (128 samples per workgroup, 129 = 128 + 1) and 8 (32 per workgroup, 35 = 32 + 3)
#   vocabularies [7, 50, 1000] with ids 6, 49, 999 in sample 0: the lanes of the chunk past field 2 carry id 999 into
#       field 0's vocabulary of 7 and must not raise the flag
@pytest.mark.parametrize("case", ref.FIELDS_CASES, ids=lambda c: c[0])
def test_fields_fm_field_counts_and_widths(ops, case):
    """forward and backward (gdeep and gfm together, every first-order table, the bias); duplicate samples and a hot
    row in every table, so the atomics accumulate"""
    name, vocabs, dim, batch = case
    idx, tables, first, bias, gdeep, gfm = ref.fields_case(vocabs, dim, batch, ref.fields_seed(name))
    assert torch.equal(idx[0], torch.tensor([v - 1 for v in vocabs]))
    want = ref.fields_fm_ref(idx, tables, first, bias, gdeep, gfm)
    idd = idx.to(DEV)
    emb, fm, flag = _fields_fwd(ops, idd, tables, first, bias)
    assert flag == 0
    ref.check_fields_fm_fwd(emb, fm, want)
    got = _fields_bwd(ops, idd, tables, emb, gdeep.to(DEV), gfm.to(DEV))
    ref.check_fields_fm_bwd(*got, want)


@pytest.mark.parametrize("first_mode,with_bias", [("some", True), ("none", True), ("all", False), ("none", False)])
def test_fields_fm_optional_first_order_and_bias(ops, first_mode, with_bias):
    """first with entries NULL (every third field), first NULL altogether, bias NULL: forward and backward (gfirst with
    the same entries NULL, gbias NULL)"""
    vocabs, dim, batch = [7 + 13 * f for f in range(9)], 16, 67
    idx, tables, first, bias, gdeep, gfm = ref.fields_case(vocabs, dim, batch, 7100)
    if first_mode == "some":
        first = [None if f % 3 == 1 else t for f, t in enumerate(first)]
    elif first_mode == "none":
        first = None
    bias = bias if with_bias else None
    want = ref.fields_fm_ref(idx, tables, first, bias, gdeep, gfm)
    idd = idx.to(DEV)
    emb, fm, flag = _fields_fwd(ops, idd, tables, first, bias)
    assert flag == 0
    ref.check_fields_fm_fwd(emb, fm, want)
    gtables = [torch.zeros_like(t, device=DEV) for t in tables]
    gfirst = None if first is None else [None if t is None else torch.zeros_like(t, device=DEV) for t in first]
    gbias = torch.zeros(1, device=DEV) if with_bias else None
    ops.fields_fm_bwd(idd, vocabs, dim, emb, gdeep.to(DEV), gfm.to(DEV), gtables, gfirst, gbias)
    torch.cuda.synchronize()
    ref.check_fields_fm_bwd(gtables, gfirst, gbias, want)


@pytest.mark.parametrize("which", ["gdeep", "gfm", "both"])
def test_fields_fm_bwd_with_one_incoming_gradient(ops, which):
    """gdeep only (gfm NULL): the first-order and bias gradients keep their pre-fill exactly; gfm only; both"""
    vocabs, dim, batch = [7 + 13 * f for f in range(9)], 16, 67
    idx, tables, first, bias, gdeep, gfm = ref.fields_case(vocabs, dim, batch, 7200)
    gdeep = gdeep if which != "gfm" else None
    gfm = gfm if which != "gdeep" else None
    want = ref.fields_fm_ref(idx, tables, first, bias, gdeep, gfm)
    idd = idx.to(DEV)
    emb, _, _ = _fields_fwd(ops, idd, tables, first, bias)
    fill = SENTINEL if which == "gdeep" else 0.0
    gtables, gfirst, gbias = _fields_bwd(ops, idd, tables, emb, _dev(gdeep), _dev(gfm), fill=fill)
    if which == "gdeep":
        assert all(bool((t == SENTINEL).all()) for t in gfirst) and float(gbias.item()) == SENTINEL
        ref.check_fields_fm_bwd(gtables, None, None, want)
    else:
        ref.check_fields_fm_bwd(gtables, gfirst, gbias, want)


def test_fields_fm_strided_operands(ops):
    """idx the columns 1..F of a (B, F + 2) matrix (ldidx = F + 2), emb / gdeep slices of wider buffers (lde = ldg =
    F * E + 8 at column 4), fm / gfm columns of (B, 2) (ldfm = 2): the neighbours stay untouched"""
    vocabs, dim, batch = [7 + 13 * f for f in range(9)], 16, 67
    nf = len(vocabs)
    idx, tables, first, bias, gdeep, gfm = ref.fields_case(vocabs, dim, batch, 7300)
    want = ref.fields_fm_ref(idx, tables, first, bias, gdeep, gfm)
    ibuf = torch.full((batch, nf + 2), 2 ** 40, dtype=torch.int64, device=DEV)   # no table has such a row
    ibuf[:, 1:nf + 1] = idx.to(DEV)
    idd = ibuf[:, 1:nf + 1]
    ebuf, gbuf, fbuf = _filled(batch, nf * dim + 8, SENTINEL), _filled(batch, nf * dim + 8, SENTINEL), _filled(batch, 2, SENTINEL)
    emb, gd = ebuf[:, 4:4 + nf * dim], gbuf[:, 4:4 + nf * dim]
    gd.copy_(gdeep)
    fbuf[:, 1] = gfm.view(-1).to(DEV)
    fm, gf = fbuf[:, 0:1], fbuf[:, 1:2]
    _, _, flag = _fields_fwd(ops, idd, tables, first, bias, emb, fm)
    assert flag == 0
    ref.check_fields_fm_fwd(emb, fm, want)
    got = _fields_bwd(ops, idd, tables, emb, gd, gf)
    ref.check_fields_fm_bwd(*got, want)
    side = torch.full((batch, 4), SENTINEL)
    assert torch.equal(ebuf[:, :4].cpu(), side) and torch.equal(ebuf[:, 4 + nf * dim:].cpu(), side)
    assert torch.equal(fbuf[:, 1].cpu(), gfm.view(-1))


def test_fields_fm_bad_id(ops):
    """an id == vocab in the last field of one sample and -1 in the first of another: the flag, row 0 in their place,
    no gradient from them"""
    vocabs, dim, batch = [7, 50, 1000], 16, 70
    idx, tables, first, bias, gdeep, gfm = ref.fields_case(vocabs, dim, batch, 7400)
    bad = idx.clone()
    bad[4, 2], bad[9, 0] = 1000, -1
    emb, fm, flag = _fields_fwd(ops, bad.to(DEV), tables, first, bias)
    assert flag == 1
    fixed = bad.clone()
    fixed[4, 2], fixed[9, 0] = 0, 0
    ref.check_fields_fm_fwd(emb, fm, ref.fields_fm_ref(fixed, tables, first, bias))


# ---------------------------------------------------------------------------------------------------------------
# ctr_rows_sum_act_fwd / ctr_act_mask_bwd
# ---------------------------------------------------------------------------------------------------------------
ACTS = [ref.ACT_NONE, ref.ACT_RELU, ref.ACT_SIGMOID]


def _rows_sum(ops, table_a, table_b, ids, act, pad=4):
    batch, width = ids.shape[0], table_a.shape[1]
    idd = ids.to(DEV)
    buf, flag = _filled(batch, width + pad, SENTINEL), _flag()
    out = buf[:, :width]
    ops.rows_sum_act_fwd(table_a.to(DEV), idd[:, 0], table_b.to(DEV), idd[:, 1], act, out, flag)
    torch.cuda.synchronize()
    assert torch.equal(buf[:, width:].cpu(), torch.full((batch, pad), SENTINEL)), "columns beside out were written"
    return out, int(flag.item())


# a lane group of lpr = width / 4 rounded up to a power of two (<= 64) lanes per sample, 16 bytes per lane and step:
#   width   4: lpr  1;   12: lpr  4, lane 3 idle;   24: lpr  8, lanes 6, 7 idle;   64: lpr 16;   256: lpr 64;
#   width 260: lpr 64, lane 0 makes a second step for columns 256..259;   512: lpr 64, two steps per lane
# the ids are the columns of a (B, 2) int64 matrix (stride 2), out the first columns of a buffer 4 wider; the last
# sample holds the largest valid id of both tables, and the lanes past the batch, clamped onto it, must not raise the flag
@pytest.mark.parametrize("batch", [1, 333])
@pytest.mark.parametrize("width", [4, 12, 24, 64, 256, 260, 512])
def test_rows_sum_act_widths(ops, width, batch):
    table_a, table_b, ids = ref.rows_case(width, batch)
    for act in ACTS:
        out, flag = _rows_sum(ops, table_a, table_b, ids, act)
        assert flag == 0
        ref.check_rows_sum_act(out, ref.rows_sum_act_ref(table_a, ids[:, 0], table_b, ids[:, 1], act), act, f"act {act}")


def test_rows_sum_act_grid_stride(ops):
    """width 256: lpr 64, 4 samples per workgroup, grid min(ceil(8197 / 4), 256 * 8) = 2048 workgroups cover 8192:
    batch 8197 = 2048 * 4 + 4 + 1 sends workgroups 0 and 1 through a second pass, the last with one live sample"""
    table_a, table_b, ids = ref.rows_case(256, 8197)
    out, flag = _rows_sum(ops, table_a, table_b, ids, ref.ACT_RELU)
    assert flag == 0
    ref.check_rows_sum_act(out, ref.rows_sum_act_ref(table_a, ids[:, 0], table_b, ids[:, 1], ref.ACT_RELU), ref.ACT_RELU)


def test_rows_sum_act_bad_id(ops):
    """an id == rows in one table, -1 in the other: the flag is set and row 0 stands in"""
    table_a, table_b, ids = ref.rows_case(24, 70)
    bad = ids.clone()
    bad[3, 0], bad[8, 1] = table_a.shape[0], -1
    out, flag = _rows_sum(ops, table_a, table_b, bad, ref.ACT_NONE)
    assert flag == 1
    fixed = bad.clone()
    fixed[3, 0], fixed[8, 1] = 0, 0
    ref.check_rows_sum_act(out, ref.rows_sum_act_ref(table_a, fixed[:, 0], table_b, fixed[:, 1], ref.ACT_NONE), ref.ACT_NONE)


@pytest.mark.parametrize("width,batch", [(4, 1), (24, 333), (260, 70)])
def test_act_mask_bwd(ops, width, batch):
    """in place on g (the first columns of a wider buffer); ACT_NONE leaves g bit-identical; ReLU at y == 0 gives 0"""
    gen = torch.Generator().manual_seed(width + batch)
    g = torch.randn(batch, width, generator=gen)
    for act in ACTS:
        y = torch.randn(batch, width, generator=gen)
        y = torch.relu(y) if act == ref.ACT_RELU else torch.sigmoid(y) if act == ref.ACT_SIGMOID else y
        if act == ref.ACT_RELU:
            y[0, 0] = 0.0
            assert bool((y == 0).any())
        buf = _filled(batch, width + 4, SENTINEL)
        gd = buf[:, :width]
        gd.copy_(g)
        ops.act_mask_bwd(gd, y.to(DEV), act)
        torch.cuda.synchronize()
        assert torch.equal(buf[:, width:].cpu(), torch.full((batch, 4), SENTINEL))
        want = ref.act_mask_ref(g, y, act)
        if act == ref.ACT_NONE:
            assert torch.equal(gd.cpu(), g)
        else:
            ref.check_sum(gd, want["out"], want["out_n"], want["out_mass"], f"act_mask {act}")
        if act == ref.ACT_RELU:
            assert bool((gd.cpu()[y == 0] == 0).all())
