"""float64 references of the feature-interaction kernels (csrc/ffm_fused.hip, csrc/fields.hip, csrc/rows_sum.hip and the
LDS-tile kernels of csrc/interact.hip), the comparisons that go with them and the inputs both sides share.  Plain
torch on the CPU: nothing here imports the HIP library, so tests/test_interact_ref_cpu.py can check every function --
and that every comparison rejects a slightly wrong kernel -- without a GPU.

Every reference takes the kernel's own operands (strided views included), returns a dict with every output in float64
and, when the incoming gradients are given, every gradient through autograd on float64 leaves.  Beside each sum it
returns ``<name>_mass`` = sum |terms| and ``<name>_n`` = the number of terms, which the bound below needs.

Tolerances (nothing here is tuned to what a kernel gives):

* copies (id gathers, one-hot bags, a one-row bag with a real weight -- one exactly rounded product) are bit-exact;
* an fp32 sum of n terms, in any order: |err| <= n 2^-23 sum |terms| per element (tests/test_gpu_ncf_segsum.py: the
  error of the sum is (n - 1) 2^-24 sum |terms| to first order, plus one rounding per product, with a factor two to
  spare).  Where a value is a sum of sums, the rule is applied at each level (fields_fm_ref);
* after a sigmoid, a logit error bound e gives e / 4 + 2^-23;
* a row summed atomically over its samples: the same rule with every sample's terms counted;
* through several stages (FFM's probability and its gradients): the repository's own tolerances, probability rtol 1e-5,
  atol 1e-6, gradients rtol 1e-4 with a floor of 1e-6 + 1e-5 max |ref|.
"""
import torch

ULP = 2.0 ** -23
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2

# the 12 field-aware vectors of FFM in buffer order: (kind, first source column, bag rows)
FFM_SOURCE = (("bag", 2, 1), ("bag", 2, 1), ("bag", 3, 2), ("bag", 3, 2), ("bag", 5, 21), ("bag", 5, 21),
              ("bag", 26, 19), ("bag", 26, 19), ("id", 0, 0), ("id", 0, 0), ("id", 1, 0), ("id", 1, 0))
FFM_VOCAB = (1, 1, 2, 2, 21, 21, 19, 19)   # rows of the eight bag tables
# the reference's 15 dot products as index pairs into that order (model/ffm.py:62-80)
FFM_PAIRS = ((0, 2), (0, 4), (1, 6), (0, 8), (1, 10), (2, 4), (3, 6), (2, 8), (3, 10), (5, 6), (4, 8), (5, 10), (6, 9),
             (7, 11), (9, 10))
NUM_COLS, NUM_DENSE = 45, 43


# ---------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------
def check_sum(got, want, n, mass, what, sigmoid=False):
    """|got - want| <= n 2^-23 mass per element (after a sigmoid: that / 4 + 2^-23); prints and returns the worst ratio"""
    n = n if torch.is_tensor(n) else torch.tensor(float(n), dtype=torch.float64)
    bound = n.to(torch.float64) * ULP * mass
    if sigmoid:
        bound = bound / 4 + ULP
    got = got.detach().cpu().to(torch.float64)
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    err = (got - want).abs()
    ratio = err / bound.clamp_min(1e-300)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{what}: max |err| {float(err.max()) if err.numel() else 0.0:.3e}, max |err| / bound {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: max |err| / bound = {worst}"
    return worst


def check_prob(got, want, what="prob"):
    torch.testing.assert_close(got.detach().cpu(), want.float(), rtol=1e-5, atol=1e-6, msg=lambda m: f"{what}: {m}")


def check_grads(got, want):
    """the rule of tests/test_gpu_ncf_bucket_plan.py (_check_grads)"""
    assert set(got) == set(want)
    for k in want:
        floor = 1e-6 + 1e-5 * float(want[k].abs().max())
        torch.testing.assert_close(got[k].detach().cpu(), want[k].float(), rtol=1e-4, atol=floor,
                                   msg=lambda m, k=k: f"grad {k}: {m}")


def rejects(check, *args, **kw):
    """True when ``check`` raises AssertionError"""
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------
# FFM (csrc/ffm_fused.hip, ffm_head_* of csrc/interact.hip)
# ---------------------------------------------------------------------------------------------------------------
def ffm_vectors_ref(x, tables12):
    """the (B, 12k) operand: bags are x[:, a:a+K] @ W, ids are x[:, c].long().  Returns emb, emb_mass, emb_n (B, 12k)"""
    xd = x.to(torch.float64)
    vecs, mass, cnt = [], [], []
    for (kind, col, rows), t in zip(FFM_SOURCE, tables12):
        td = t.detach().cpu().to(torch.float64)
        if kind == "bag":
            w = xd[:, col:col + rows]
            vecs.append(w @ td)
            mass.append(w.abs() @ td.abs())
            cnt.append((w != 0).sum(1, keepdim=True).expand(-1, td.shape[1]))
        else:
            ids = x[:, col].long()
            vecs.append(td[ids])
            mass.append(td[ids].abs())
            cnt.append(torch.ones(x.shape[0], td.shape[1], dtype=torch.int64))
    return torch.cat(vecs, 1), torch.cat(mass, 1), torch.cat(cnt, 1)


def ffm_head_ref(emb, nvec, dim, pairs, x, user1, item1, lin_w, lin_b, gprob=None, mutate=None):
    """prob = sigmoid(user1[u] + item1[i] + linear(x[:, 2:] + cross)), cross = sum over ``pairs`` of <v_a, v_b>, with the
    reference's quirk: the cross scalar is added to every dense column before the linear layer.  Given ``gprob``: gemb
    (with respect to the emb operand as a leaf: what the kernel writes), guser1, gitem1, glin_w, glin_b.

    ``mutate`` (negative controls): "drop_pair" leaves the last pair out, "half_group" adds only the first half of every
    vector's elements (LPR / 2 lanes of a lane group), "no_cross" takes x without + cross, "swap_partners" exchanges the
    gradients (the partner lists) of vectors 0 and 1."""
    batch = x.shape[0]
    leaf = lambda t: t.detach().cpu().to(torch.float64).clone().requires_grad_(gprob is not None)  # noqa: E731
    e, u1, i1, w, b = leaf(emb[:, :nvec * dim]), leaf(user1), leaf(item1), leaf(lin_w), leaf(lin_b)
    xd = x.detach().cpu().to(torch.float64)
    uid, iid = xd[:, 0].long(), xd[:, 1].long()
    v = e.reshape(batch, nvec, dim)
    use = pairs[:-1] if mutate == "drop_pair" else pairs
    keep = dim // 2 if mutate == "half_group" else dim
    cross = None
    for a, c in use:
        d = (v[:, a, :keep] * v[:, c, :keep]).sum(1)
        cross = d if cross is None else cross + d          # left to right, as model/ffm.py:82
    dense = xd[:, 2:NUM_COLS]
    if mutate != "no_cross":
        dense = dense + cross.unsqueeze(1)
    logit = u1[uid] + i1[iid] + dense @ w.t() + b
    prob = torch.sigmoid(logit)
    out = {"prob": prob.detach(), "cross": cross.detach(), "logit": logit.detach()}
    if gprob is not None:
        prob.backward(gprob.detach().cpu().to(torch.float64).reshape(batch, 1))
        grad = e.grad if e.grad is not None else torch.zeros_like(e)
        gemb = grad.clone()
        if mutate == "swap_partners":
            gemb[:, 0:dim], gemb[:, dim:2 * dim] = grad[:, dim:2 * dim], grad[:, 0:dim]
        out.update(gemb=gemb, guser1=u1.grad, gitem1=i1.grad, glin_w=w.grad, glin_b=b.grad)
    return out


def ffm_ref(x, tables12, user1, item1, lin_w, lin_b, pairs=FFM_PAIRS, gprob=None, mutate=None):
    """ctr_ffm_fused_fwd / _bwd: ffm_vectors_ref, then ffm_head_ref on that operand"""
    emb, mass, cnt = ffm_vectors_ref(x, tables12)
    dim = tables12[0].shape[1]
    out = ffm_head_ref(emb, 12, dim, pairs, x, user1, item1, lin_w, lin_b, gprob, mutate)
    out.update(emb=emb, emb_mass=mass, emb_n=cnt)
    return out


def ffm_table_grads(x, tables12, gemb):
    """the gradients of the 12 tables from gemb: the float64 bag and gather chain rule"""
    xd = x.detach().cpu().to(torch.float64)
    dim = tables12[0].shape[1]
    grads = []
    for f, ((kind, col, rows), t) in enumerate(zip(FFM_SOURCE, tables12)):
        g = gemb[:, f * dim:(f + 1) * dim].to(torch.float64)
        if kind == "bag":
            grads.append(xd[:, col:col + rows].t() @ g)
        else:
            grads.append(torch.zeros(t.shape[0], dim, dtype=torch.float64).index_add_(0, xd[:, col].long(), g))
    return grads


GENRE_COLS = slice(6, 8)    # vectors 6 and 7: the multi-hot bags, the only fp32 sums in the operand


def check_ffm_emb(got, ref):
    """the (B, 12k) operand: bit-exact but for the multi-hot bags (sums of <= 19 rows: the fp32 sum rule; a sample
    without a genre has n = 0 and must be exactly zero)"""
    dim = ref["emb"].shape[1] // 12
    got = got.detach().cpu()
    lo, hi = GENRE_COLS.start * dim, GENRE_COLS.stop * dim
    assert torch.equal(got[:, :lo], ref["emb"][:, :lo].float()), "emb: age / gender / occupation vectors are not bit-exact"
    assert torch.equal(got[:, hi:], ref["emb"][:, hi:].float()), "emb: id rows are not bit-exact"
    return check_sum(got[:, lo:hi], ref["emb"][:, lo:hi], ref["emb_n"][:, lo:hi], ref["emb_mass"][:, lo:hi], "emb genre bags")


def check_ffm_bwd(got, ref):
    check_grads(got, {k: ref[k] for k in got})


def ffm_case(dim, batch, seed, num_users=50, num_items=70):
    """x from synth.feature_batch with sample 0 without a genre and sample `batch // 2` with a non-trivial real age;
    tables N(0, 0.25^2), gprob N(0, 1)"""
    from deeplearningrecommendationsystem_amd import synth
    gen = synth.generator(seed)
    x = synth.feature_batch(batch, num_users, num_items, gen, zero_genre_rows=1)
    x[batch // 2, 2] = 0.6180339887
    if batch > 2:
        x[batch - 1, 26:45] = 0.0
        x[batch - 1, 26 + 3], x[batch - 1, 26 + 11], x[batch - 1, 26 + 18] = 1.0, 1.0, 1.0   # three genres for certain
    rnd = lambda *s: 0.25 * torch.randn(*s, generator=gen)  # noqa: E731
    tables = [rnd(v, dim) for v in FFM_VOCAB] + [rnd(num_users, dim), rnd(num_users, dim), rnd(num_items, dim),
                                                 rnd(num_items, dim)]
    user1, item1, lin_w, lin_b = rnd(num_users, 1), rnd(num_items, 1), rnd(1, NUM_DENSE), rnd(1)
    gprob = torch.randn(batch, 1, generator=gen)
    return x, tables, user1, item1, lin_w, lin_b, gprob


# ---------------------------------------------------------------------------------------------------------------
# N id fields + FM (ctr_fields_fm_fwd / _bwd)
# ---------------------------------------------------------------------------------------------------------------
def fields_fm_ref(idx, tables, first, bias, gdeep=None, gfm=None, mutate=None):
    """emb[b, f*E + e] = v_fe = tables[f][idx[b, f], e];
    fm[b] = sum_f first[f][idx[b, f]] + bias + 0.5 sum_e [(sum_f v_fe)^2 - sum_f v_fe^2]          (first / bias: may be None)
    The sum rule at both levels of the nest: S_e = sum_f v_fe has F terms, so S_e^2 is within 2 F 2^-23 A_e^2 (A_e = sum_f
    |v_fe|) and q_e = sum_f v_fe^2 within F 2^-23 q_e; the outer sum has 2 E + F + 1 terms (S_e^2, q_e, the first-order
    weights, the bias), each at most its own mass: fm_n = 3 F + 2 E + 1 on fm_mass = 0.5 sum_e (A_e^2 + q_e) + sum_f
    |first| + |bias|.
    Given gdeep (B, F*E) and/or gfm (B, 1): gtables, gfirst, gbias of  sum(emb * gdeep) + sum(fm * gfm), each with its
    mass and n.  A table row: every sample on it brings gdeep + g (sum_h v_h - v_f), F + 2 terms, and the row adds its
    c samples: n = c + F + 2 on the mass of all of them.

    ``mutate``: "no_last" leaves the last field out of S = sum_f v_f, "shift_first" fetches field f's first-order weight
    with the id of field f + 1 (the lane rule shifted by one field)."""
    idx = idx.detach().cpu()
    batch, nf = idx.shape
    dim = tables[0].shape[1]
    want_grad = gdeep is not None or gfm is not None
    leaf = lambda t: None if t is None else t.detach().cpu().to(torch.float64).clone().requires_grad_(want_grad)  # noqa: E731
    tl = [leaf(t) for t in tables]
    fl = [None] * nf if first is None else [leaf(t) for t in first]
    bl = leaf(bias)
    vs = [tl[f][idx[:, f]] for f in range(nf)]
    emb = torch.cat(vs, 1)
    stack = torch.stack(vs, 1)                                     # (B, F, E)
    s = (stack[:, :-1] if mutate == "no_last" else stack).sum(1)
    fm = 0.5 * ((s * s).sum(1) - (stack * stack).sum((1, 2)))
    mass = 0.5 * ((stack.detach().abs().sum(1) ** 2).sum(1) + (stack.detach() ** 2).sum((1, 2)))
    for f in range(nf):
        if fl[f] is not None:
            ids = idx[:, (f + 1) % nf] % fl[f].shape[0] if mutate == "shift_first" else idx[:, f]
            fm = fm + fl[f][ids, 0]
            mass = mass + fl[f].detach()[ids, 0].abs()
    if bl is not None:
        fm = fm + bl[0]
        mass = mass + bl.detach()[0].abs()
    out = {"emb": emb.detach(), "fm": fm.detach().unsqueeze(1), "fm_mass": mass.unsqueeze(1),
           "fm_n": 3 * nf + 2 * dim + 1}
    if not want_grad:
        return out
    gd = None if gdeep is None else gdeep.detach().cpu().to(torch.float64)[:, :nf * dim]
    g = None if gfm is None else gfm.detach().cpu().to(torch.float64).reshape(batch)
    loss = 0.0
    if gd is not None:
        loss = loss + (emb * gd).sum()
    if g is not None:
        loss = loss + (fm * g).sum()
    loss.backward()
    zero = lambda t: torch.zeros_like(t)  # noqa: E731
    out["gtables"] = [t.grad if t.grad is not None else zero(t) for t in tl]
    out["gfirst"] = [None if t is None else (t.grad if t.grad is not None else zero(t)) for t in fl]
    out["gbias"] = None if bl is None else (bl.grad if bl.grad is not None else zero(bl))
    # masses: |gdeep| + |g| (sum_h |v_h| + |v_f|) per sample on the row
    sd = stack.detach().abs()
    gabs = torch.zeros(batch, dtype=torch.float64) if g is None else g.abs()
    out["gtables_mass"], out["gtables_n"], out["gfirst_mass"], out["gfirst_n"] = [], [], [], []
    for f in range(nf):
        m = gabs.view(batch, 1) * (sd.sum(1) + sd[:, f])
        if gd is not None:
            m = m + gd[:, f * dim:(f + 1) * dim].abs()
        rows = tables[f].shape[0]
        cnt = torch.bincount(idx[:, f], minlength=rows).to(torch.float64).unsqueeze(1)
        out["gtables_mass"].append(torch.zeros(rows, dim, dtype=torch.float64).index_add_(0, idx[:, f], m))
        out["gtables_n"].append(cnt + (nf + 2))
        out["gfirst_mass"].append(torch.zeros(rows, 1, dtype=torch.float64).index_add_(0, idx[:, f], gabs.view(batch, 1)))
        out["gfirst_n"].append(cnt)
    out["gbias_mass"], out["gbias_n"] = gabs.sum().reshape(1), batch
    return out


def check_fields_fm_fwd(emb, fm, ref):
    assert torch.equal(emb.detach().cpu(), ref["emb"].float()), "emb: the gathered rows are not bit-exact"
    return check_sum(fm, ref["fm"], ref["fm_n"], ref["fm_mass"], "fm")


def check_fields_fm_bwd(gtables, gfirst, gbias, ref):
    """every gradient the caller asked for (None: not asked); returns the worst ratio"""
    worst = 0.0
    for f, g in enumerate(gtables):
        if g is not None:
            worst = max(worst, check_sum(g, ref["gtables"][f], ref["gtables_n"][f], ref["gtables_mass"][f], f"gtable {f}"))
    for f, g in enumerate(gfirst or []):
        if g is not None:
            worst = max(worst, check_sum(g, ref["gfirst"][f], ref["gfirst_n"][f], ref["gfirst_mass"][f], f"gfirst {f}"))
    if gbias is not None:
        worst = max(worst, check_sum(gbias, ref["gbias"], ref["gbias_n"], ref["gbias_mass"], "gbias"))
    return worst


def fields_case(vocabs, dim, batch, seed, hot=True):
    """ids with the largest id of every field present, duplicate samples, and (``hot``) half the batch on one id of
    every field so that the atomics accumulate; tables / first N(0, 0.25^2), bias, gdeep, gfm N(0, 1)"""
    gen = torch.Generator().manual_seed(seed)
    nf = len(vocabs)
    idx = torch.stack([torch.randint(0, v, (batch,), generator=gen) for v in vocabs], 1)
    if hot and batch >= 4:
        half = torch.randperm(batch, generator=gen)[:batch // 2]
        idx[half] = torch.tensor([v // 3 for v in vocabs])
    idx[0] = torch.tensor([v - 1 for v in vocabs])
    if batch >= 3:
        idx[batch - 1] = idx[1]                                     # a duplicate sample
    tables = [0.25 * torch.randn(v, dim, generator=gen) for v in vocabs]
    first = [0.25 * torch.randn(v, 1, generator=gen) for v in vocabs]
    bias = torch.randn(1, generator=gen)
    gdeep = torch.randn(batch, nf * dim, generator=gen)
    gfm = torch.randn(batch, 1, generator=gen)
    return idx, tables, first, bias, gdeep, gfm


# ---------------------------------------------------------------------------------------------------------------
# all-pairs inner products (ctr_fields_pairs_fwd, ctr_allpairs_fwd / _bwd)
# ---------------------------------------------------------------------------------------------------------------
def pairs_ref(emb, nvec, dim, gp=None):
    """prod[b, idx(i, j)] = <v_i, v_j>, i < j lexicographic, through the per-sample Gram matrices (no (B, npairs, dim)
    intermediate); given gp (B, npairs): gemb[b, i] = sum_{j != i} gp[b, idx(i, j)] v_j, through the symmetric
    coefficient matrices.  prod_n = dim, gemb_n = nvec - 1."""
    v = emb.detach().cpu()[:, :nvec * dim].to(torch.float64).reshape(-1, nvec, dim)
    iu = torch.triu_indices(nvec, nvec, 1)
    gram = torch.bmm(v, v.transpose(1, 2))
    out = {"prod": gram[:, iu[0], iu[1]], "prod_n": dim}
    out["prod_mass"] = torch.bmm(v.abs(), v.abs().transpose(1, 2))[:, iu[0], iu[1]]
    del gram
    if gp is not None:
        c = torch.zeros(v.shape[0], nvec, nvec, dtype=torch.float64)
        c[:, iu[0], iu[1]] = gp.detach().cpu().to(torch.float64)[:, :iu.shape[1]]
        c = c + c.transpose(1, 2)
        out["gemb"] = torch.bmm(c, v).reshape(v.shape[0], nvec * dim)
        out["gemb_mass"] = torch.bmm(c.abs(), v.abs()).reshape(v.shape[0], nvec * dim)
        out["gemb_n"] = nvec - 1
    return out


# ---------------------------------------------------------------------------------------------------------------
# NeuralCF's any-width table-row path (ctr_rows_sum_act_fwd, ctr_act_mask_bwd)
# ---------------------------------------------------------------------------------------------------------------
def _act(z, act):
    return torch.relu(z) if act == ACT_RELU else torch.sigmoid(z) if act == ACT_SIGMOID else z


def rows_sum_act_ref(table_a, idx_a, table_b, idx_b, act):
    """out[b] = act(table_a[idx_a[b]] + table_b[idx_b[b]]): two terms per element"""
    a = table_a.detach().cpu().to(torch.float64)[idx_a.detach().cpu()]
    b = table_b.detach().cpu().to(torch.float64)[idx_b.detach().cpu()]
    return {"out": _act(a + b, act), "out_mass": a.abs() + b.abs(), "out_n": 2}


def check_rows_sum_act(got, ref, act, what="rows_sum_act"):
    return check_sum(got, ref["out"], ref["out_n"], ref["out_mass"], what, sigmoid=act == ACT_SIGMOID)


def act_mask_ref(g, y, act):
    """g * act'(y) with the derivative through the OUTPUT y: 1, [y > 0], y (1 - y) = y - y^2 (two terms)"""
    g, y = g.detach().cpu().to(torch.float64), y.detach().cpu().to(torch.float64)
    if act == ACT_RELU:
        return {"out": g * (y > 0), "out_mass": g.abs(), "out_n": 1}
    if act == ACT_SIGMOID:
        return {"out": g * y * (1 - y), "out_mass": g.abs() * (y.abs() + y * y), "out_n": 2}
    return {"out": g, "out_mass": g.abs(), "out_n": 1}


def rows_case(width, batch, rows_a=37, rows_b=53):
    """two tables N(0, 1) and a (B, 2) int64 id matrix whose last sample holds the largest valid id of both"""
    gen = torch.Generator().manual_seed(width * 100003 + batch)
    table_a, table_b = torch.randn(rows_a, width, generator=gen), torch.randn(rows_b, width, generator=gen)
    ids = torch.stack([torch.randint(0, rows_a, (batch,), generator=gen), torch.randint(0, rows_b, (batch,), generator=gen)], 1)
    ids[batch - 1, 0], ids[batch - 1, 1] = rows_a - 1, rows_b - 1
    return table_a, table_b, ids


# ---------------------------------------------------------------------------------------------------------------
# the shapes tests/test_gpu_interactions.py runs (the arithmetic that puts each on its arm is in the comments there);
# tests/test_interact_ref_cpu.py applies its negative controls at the same inputs
# ---------------------------------------------------------------------------------------------------------------
FFM_FUSED_CASES = [(8, 37), (16, 67), (32, 1), (64, 19)]


def ffm_seed(dim, batch):
    return 4000 + 131 * dim + batch


def _vocabs(n):
    return [7 + 13 * f for f in range(n)]


FIELDS_CASES = [("f1", _vocabs(1), 16, 67), ("f8", _vocabs(8), 16, 67), ("f9", _vocabs(9), 16, 67),
                ("f16", _vocabs(16), 16, 67), ("f32", _vocabs(32), 16, 67), ("f2_w64_two_passes", [30, 1000], 64, 65555),
                ("f5_w8", _vocabs(5), 8, 129), ("f5_w32", _vocabs(5), 32, 35), ("vocab_7_50_1000", [7, 50, 1000], 16, 70)]


def fields_seed(name):
    return 7000 + [c[0] for c in FIELDS_CASES].index(name)


PAIRS_CASES = [(26, 64, 70), (32, 64, 37), (32, 64, 16389), (32, 8, 100), (9, 16, 65), (32, 256, 3)]


def pairs_case(nvec, dim, batch):
    gen = torch.Generator().manual_seed(nvec * 1009 + dim * 31 + batch)
    return torch.randn(batch, nvec * dim, generator=gen), torch.randn(batch, nvec * (nvec - 1) // 2, generator=gen)
