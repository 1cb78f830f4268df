"""float64 reference of the embedding stage (csrc/embed.hip, embed_sorted.hip, embed_bag.hip), inputs on which
every fp32 sum is exact, and the builder of the cases in tests/embed_cases.py (one per dispatch arm of ctr_embed_fwd /
ctr_embed_bwd).  CPU only.

The contract ("Bad ids in the embedding stage"): an id outside [0, vocab) reads row 0 in the forward and
raises the flag; in the backward that sample adds to no row -- for a product field, to no row of either factor.

Exact inputs.  gout is k / 16 with 1 <= |k| <= 16; tables, bag weights, dense columns and the gradients' start values
are k / 4 with |k| <= 8.  Every term of a gradient element (g, w * g, g * t) is then a multiple of 2^-6 of at most 128
units, and every forward term (t, w * t, t1 * t2) a multiple of 2^-4 of at most 64.  ``exact_guard`` sums |term| per
output element: while that stays below 2^24 units every partial sum, in ANY order and through any mix of LDS, register
and global atomics, is an fp32 number, so the kernels have one right answer and every comparison is ``torch.equal``.

tests/test_embed_ref_cpu.py holds the reference against float64 autograd, the guard over every case,
and mutations of the reference; tests/test_gpu_embed_arms.py runs the cases on the device."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

ID_I64, ID_F32, BAG, DENSE, PROD_I64 = range(5)      # ctr_field_kind (include/ctrhip.h)
GUARD_ROWS = 4          # rows before and after a gradient view (4 rows x width floats keeps 16-byte alignment)
GUARD_COLS = 4          # columns left of an output view (the right guard is whatever ldo leaves, >= 1)
SENTINEL = -12345.5
GRAD_UNIT, FWD_UNIT, LIMIT = 2.0 ** -6, 2.0 ** -4, 2.0 ** 24
MUTATIONS = ("drop_last", "double_hot", "shift_out_col", "swap_partners", "bad_to_row0", "skip_last_row")


@dataclass
class Spec:
    """mirror of ops.FieldSpec on CPU tensors; ``tkey`` / ``ikey`` name the table and the (id matrix, column)"""
    kind: int
    width: int
    out_col: int
    table: Optional[torch.Tensor] = None
    src_col: int = 0
    bag_size: int = 0
    idx: Optional[torch.Tensor] = None
    idx_stride: int = 1
    table2: Optional[torch.Tensor] = None
    idx2: Optional[torch.Tensor] = None
    tkey: Optional[str] = None
    tkey2: Optional[str] = None
    ikey: Optional[Tuple[str, int]] = None
    ikey2: Optional[Tuple[str, int]] = None


# ---------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------
def _rows(s: Spec, x, second=False):
    """(ids, in-range mask) of an id field; ID_F32 truncates toward zero like the kernels' (int64_t) cast"""
    if s.kind == ID_F32:
        ids, vocab = x[:, s.src_col].to(torch.int64), s.table.shape[0]
    elif second:
        ids, vocab = s.idx2, s.table2.shape[0]
    else:
        ids, vocab = s.idx, s.table.shape[0]
    return ids, (ids >= 0) & (ids < vocab)


def out_width(specs):
    return max(s.out_col + s.width for s in specs)


def embed_ref(specs, x, batch, mutate=None):
    """(float64 (batch, out_width) output with NaN where no field writes, flag).  ``mutate``: see MUTATIONS"""
    if mutate == "shift_out_col":
        specs = [_shifted(s) for s in specs]
    out = torch.full((batch, out_width(specs)), float("nan"), dtype=torch.float64)
    flag = 0
    live = batch - 1 if mutate == "drop_last" else batch
    for s in specs:
        cols = slice(s.out_col, s.out_col + s.width)
        if s.kind in (ID_I64, ID_F32):
            ids, ok = _rows(s, x)
            flag |= int((~ok).any())
            v = s.table.double()[torch.where(ok, ids, torch.zeros_like(ids))]
        elif s.kind == BAG:
            tab, v = s.table.double(), torch.zeros(batch, s.width, dtype=torch.float64)
            for j in range(s.bag_size):           # in row order, like the kernels' FMA chain
                v += x[:, s.src_col + j, None].double() * tab[j]
        elif s.kind == DENSE:
            v = x[:, s.src_col:s.src_col + s.width].double()
        else:
            (i1, ok1), (i2, ok2) = _rows(s, x), _rows(s, x, True)
            flag |= int((~ok1).any() or (~ok2).any())
            v = (s.table.double()[torch.where(ok1, i1, torch.zeros_like(i1))]
                 * s.table2.double()[torch.where(ok2, i2, torch.zeros_like(i2))])
        out[:live, cols] = v[:live]
    return out, flag


def _shifted(s: Spec) -> Spec:
    t = Spec(**s.__dict__)
    t.out_col = s.out_col + 4
    return t


def _hot_sample(specs, x):
    """a sample of the most frequent in-range row of the first id / product field (bags: the first sample with a
    non-zero weight)"""
    for s in specs:
        if s.kind in (ID_I64, ID_F32, PROD_I64):
            ids, ok = _rows(s, x)
            if s.kind == PROD_I64:
                ok = ok & _rows(s, x, True)[1]
            if ok.any():
                row = torch.bincount(ids[ok]).argmax()
                return int(torch.nonzero(ok & (ids == row))[0])
    for s in specs:
        if s.kind == BAG:
            return int(torch.nonzero(x[:, s.src_col:s.src_col + s.bag_size].abs().sum(1))[0])
    return 0


def embed_bwd_ref(specs, x, gout, mutate=None, absolute=False) -> Dict[str, torch.Tensor]:
    """float64 gradient per table key (zeros for a table nothing reaches).  ``gout`` is (batch, >= out_width).
    ``absolute``: every term replaced by its magnitude (the guard's sum)"""
    batch = gout.shape[0]
    g64 = gout.double()
    if mutate == "shift_out_col":
        specs = [_shifted(s) for s in specs]
    wgt = torch.ones(batch, 1, dtype=torch.float64)        # per-sample weight: 1 in the true reference
    if mutate == "drop_last":
        wgt[-1] = 0.0
    if mutate == "double_hot":
        wgt[_hot_sample(specs, x)] = 2.0
    mag = (lambda t: t.abs()) if absolute else (lambda t: t)
    grads: Dict[str, torch.Tensor] = {}

    def acc(key, table):
        if key not in grads:
            grads[key] = torch.zeros(table.shape, dtype=torch.float64)
        return grads[key]

    def add_rows(key, table, ids, ok, terms):
        g = acc(key, table)
        if mutate == "bad_to_row0":
            ids, ok = torch.where(ok, ids, torch.zeros_like(ids)), torch.ones_like(ok)
        if mutate == "skip_last_row":
            ok = ok & (ids != table.shape[0] - 1)
        g.index_add_(0, ids[ok], mag(terms[ok]))

    for s in specs:
        if s.kind == DENSE:
            continue
        gs = g64[:, s.out_col:s.out_col + s.width] * wgt
        if s.kind in (ID_I64, ID_F32):
            ids, ok = _rows(s, x)
            add_rows(s.tkey, s.table, ids, ok, gs)
        elif s.kind == BAG:
            g = acc(s.tkey, s.table)
            last = s.bag_size - (1 if mutate == "skip_last_row" else 0)
            for j in range(last):
                g[j] += mag(x[:, s.src_col + j, None].double() * gs).sum(0)
        else:
            (i1, ok1), (i2, ok2) = _rows(s, x), _rows(s, x, True)
            both = ok1 & ok2                                # a bad id in either factor: no gradient for both
            if mutate == "bad_to_row0":
                both = torch.ones_like(both)
            r1, r2 = torch.where(ok1, i1, torch.zeros_like(i1)), torch.where(ok2, i2, torch.zeros_like(i2))
            t1, t2 = s.table.double()[r1], s.table2.double()[r2]
            if mutate == "swap_partners":
                t1, t2 = t2, t1
            add_rows(s.tkey, s.table, r1, both, gs * t2)
            add_rows(s.tkey2, s.table2, r2, both, gs * t1)
    return grads


# ---------------------------------------------------------------------------------------------------------------
# exact inputs
# ---------------------------------------------------------------------------------------------------------------
def quarters(shape, gen):
    """k / 4, |k| <= 8"""
    return torch.randint(-8, 9, shape, generator=gen).float() / 4


def quarters_nonzero(shape, gen):
    """k / 4, 1 <= |k| <= 8: a gradient's start value (non-zero: the contract is to accumulate)"""
    k = torch.randint(1, 9, shape, generator=gen) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
    return k.float() / 4


def sixteenths_nonzero(shape, gen):
    """k / 16, 1 <= |k| <= 16 (gout: a dropped or doubled sample always changes a sum)"""
    k = torch.randint(1, 17, shape, generator=gen) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
    return k.float() / 16


def bag_weights(batch, rows, gen):
    """sample b: all-zero (b % 3 == 0), one-hot with weight 1 (b % 3 == 1), multi-hot k / 4 (b % 3 == 2)"""
    w = torch.zeros(batch, rows)
    b = torch.arange(batch)
    one = b % 3 == 1
    w[one, torch.randint(0, rows, (int(one.sum()),), generator=gen)] = 1.0
    multi = b % 3 == 2
    n = int(multi.sum())
    w[multi] = quarters((n, rows), gen) * (torch.rand(n, rows, generator=gen) < 0.6)
    return w


def make_ids(batch, vocab, pattern, gen):
    if pattern == "uniform":
        ids = torch.randint(0, vocab, (batch,), generator=gen)
    elif pattern == "zipf":                             # V ** u - 1: row 0 is the hottest
        u = torch.rand(batch, generator=gen, dtype=torch.float64)
        ids = (vocab ** u - 1).floor().to(torch.int64).clamp_(0, vocab - 1)
    elif pattern == "equal":
        ids = torch.full((batch,), min(3, vocab - 1), dtype=torch.int64)
    elif pattern == "sorted":
        ids = torch.randint(0, vocab, (batch,), generator=gen).sort().values
    elif pattern == "quarter0":                          # the behaviour sequences' padding row
        ids = torch.randint(0, vocab, (batch,), generator=gen)
        ids[torch.arange(batch) % 4 == 1] = 0
    elif pattern == "ends":                              # both ends of the range among uniform ids
        ids = torch.randint(0, vocab, (batch,), generator=gen)
        ids[torch.arange(batch) % 3 == 0] = 0
        ids[torch.arange(batch) % 3 == 1] = vocab - 1
    else:
        raise ValueError(pattern)
    return ids


def inject_bad(ids, vocab):
    """-3 at the first sample, vocab at the last, vocab + 7 in the middle of a run of nine equal ids"""
    batch = ids.shape[0]
    mid = batch // 2
    if batch >= 16:
        ids[mid - 4:mid + 5] = ids[mid].clone()
    if batch >= 3:
        ids[mid] = vocab + 7
        ids[-1] = vocab
    ids[0] = -3
    return ids


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    family: str
    arm: str
    batch: int
    specs: List[Spec]
    x: Optional[torch.Tensor]
    gout: torch.Tensor                      # (batch, width)
    tables: Dict[str, torch.Tensor]
    mats: Dict[str, torch.Tensor]           # id matrices (batch, L) int64
    base: Dict[str, torch.Tensor]           # start value of every gradient
    frozen: frozenset = frozenset()         # tables without a gradient buffer
    table_shift: frozenset = frozenset()    # tables placed one float off 16-byte alignment
    grad_shift: frozenset = frozenset()     # gradients placed one float off 16-byte alignment
    left: int = GUARD_COLS                  # first column of the out / gout view inside its buffer
    ldo: int = 0                            # leading dimension of that buffer
    ws: object = "ops"                      # "ops": ops.embed_bwd's scratch; None: NULL; int: that many floats (C entry)
    ws_written: Optional[bool] = None       # with an int workspace: whether the arm writes it
    has_bad: bool = False

    @property
    def width(self):
        return out_width(self.specs)


class Build:
    """collects tables, id matrices, x columns and fields of one case"""

    def __init__(self, name, family, arm, batch):
        self.name, self.family, self.arm, self.batch = name, family, arm, batch
        self.gen = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + batch)
        self.tables, self.mats, self.xcols, self.specs = {}, {}, [], []
        self.frozen, self.tshift, self.gshift = set(), set(), set()
        self.col, self.ldx, self.has_bad = 0, 0, False

    def table(self, vocab, width, frozen=False, shift=False, grad_shift=False):
        key = f"t{len(self.tables)}"
        self.tables[key] = quarters((vocab, width), self.gen)
        if frozen:
            self.frozen.add(key)
        if shift:
            self.tshift.add(key)
        if grad_shift:
            self.gshift.add(key)
        return key

    def ids(self, vocabs, pattern="uniform", bad=()):
        """an id matrix (batch, len(vocabs)); ``bad``: the columns that get the three bad ids"""
        key = f"m{len(self.mats)}"
        cols = [make_ids(self.batch, v, pattern, self.gen) for v in vocabs]
        for c in bad:
            inject_bad(cols[c], vocabs[c])
            self.has_bad = True
        self.mats[key] = torch.stack(cols, 1).contiguous()
        return key

    def _x(self, block):
        src = self.ldx
        self.xcols.append(block)
        self.ldx += block.shape[1]
        return src

    def pad_x(self, multiple=4):
        n = -self.ldx % multiple
        if n:
            self._x(torch.full((self.batch, n), SENTINEL))

    def _out(self, width, out_col):
        if out_col is None:
            out_col = self.col
        self.col = max(self.col, out_col + width)
        return out_col

    def id(self, t, m, col=0, out_col=None):
        tab, mat = self.tables[t], self.mats[m]
        self.specs.append(Spec(ID_I64, tab.shape[1], self._out(tab.shape[1], out_col), table=tab, idx=mat[:, col],
                               idx_stride=mat.shape[1], tkey=t, ikey=(m, col)))

    def idf(self, t, pattern="uniform", bad=False, out_col=None):
        tab = self.tables[t]
        ids = make_ids(self.batch, tab.shape[0], pattern, self.gen)
        if bad:
            inject_bad(ids, tab.shape[0])
            self.has_bad = True
        src = self._x(ids.float()[:, None])
        self.specs.append(Spec(ID_F32, tab.shape[1], self._out(tab.shape[1], out_col), table=tab, src_col=src, tkey=t))

    def bag(self, t, out_col=None):
        tab = self.tables[t]
        src = self._x(bag_weights(self.batch, tab.shape[0], self.gen))
        self.specs.append(Spec(BAG, tab.shape[1], self._out(tab.shape[1], out_col), table=tab, src_col=src,
                               bag_size=tab.shape[0], tkey=t))

    def dense(self, width, out_col=None):
        src = self._x(quarters((self.batch, width), self.gen))
        self.specs.append(Spec(DENSE, width, self._out(width, out_col), src_col=src))

    def prod(self, t1, m1, c1, t2, m2, c2, out_col=None):
        a, b = self.tables[t1], self.tables[t2]
        assert self.mats[m1].shape[1] == self.mats[m2].shape[1], "one idx_stride per field"
        self.specs.append(Spec(PROD_I64, a.shape[1], self._out(a.shape[1], out_col), table=a, idx=self.mats[m1][:, c1],
                               idx_stride=self.mats[m1].shape[1], table2=b, idx2=self.mats[m2][:, c2], tkey=t1, tkey2=t2,
                               ikey=(m1, c1), ikey2=(m2, c2)))

    def done(self, left=GUARD_COLS, ldo=None, ws="ops", ws_written=None):
        width = self.col
        if ldo is None:
            ldo = (left + width + 4 + 3) // 4 * 4
        assert ldo > left + width, "a guard column on the right"
        x = torch.cat(self.xcols, 1).contiguous() if self.xcols else None
        base = {k: quarters_nonzero(tuple(t.shape), self.gen) for k, t in self.tables.items() if k not in self.frozen}
        return Case(self.name, self.family, self.arm, self.batch, self.specs, x,
                    sixteenths_nonzero((self.batch, width), self.gen), self.tables, self.mats, base,
                    frozenset(self.frozen), frozenset(self.tshift), frozenset(self.gshift), left, ldo, ws, ws_written,
                    self.has_bad)


def exact_guard(case: Case):
    """every output element's sum of |term| (plus the gradient's start value) stays below 2^24 units: 2^-6 in the
    backward, 2^-4 in the forward.  Returns the two worst unit counts"""
    worst_b = 0.0
    mags = embed_bwd_ref(case.specs, case.x, case.gout, absolute=True)
    for key, g in mags.items():
        if key in case.frozen:
            continue
        units = float(((g + case.base[key].double().abs()) / GRAD_UNIT).max())
        assert units < LIMIT, f"{case.name}: gradient of {key} may need {units:.0f} units of 2^-6 (limit 2^24)"
        worst_b = max(worst_b, units)
    worst_f = 0.0
    for s in case.specs:
        if s.kind == BAG:
            xa = case.x[:, s.src_col:s.src_col + s.bag_size].double().abs()
            worst_f = max(worst_f, float((xa @ s.table.double().abs()).max() / FWD_UNIT))
    assert worst_f < LIMIT, f"{case.name}: a bag's forward sum may need {worst_f:.0f} units of 2^-4"
    for name, t in (("gout", case.gout), *case.tables.items(), *case.base.items()):
        assert bool((t * 16 == (t * 16).round()).all()) and float(t.abs().max()) <= 2.0, f"{case.name}: {name} not dyadic"
    if case.x is not None:
        for s in case.specs:
            if s.kind in (BAG, DENSE):
                n = s.bag_size if s.kind == BAG else s.width
                xs = case.x[:, s.src_col:s.src_col + n]
                assert bool((xs * 4 == (xs * 4).round()).all()) and float(xs.abs().max()) <= 2.0
    return worst_b, worst_f


def sorted_need(batch, jobs):
    """workspace floats the sorted path asks for (embed_sorted.hip): ``jobs`` is [(vocab, has companion column)].
    nblk = min(ceil(batch / 1024), 128), chunk = ceil(batch / nblk), nblk = ceil(batch / chunk); per job
    2 * ceil4(nblk * vocab) + ceil4(vocab) + (3 if companion else 2) * ceil4(batch)"""
    c4 = lambda v: (v + 3) // 4 * 4  # noqa: E731
    nblk = min(-(-batch // 1024), 128)
    chunk = -(-batch // nblk)
    nblk = -(-batch // chunk)
    return sum(2 * c4(nblk * v) + c4(v) + (3 if comp else 2) * c4(batch) for v, comp in jobs)


def hot_slot(field, row, slots_log2=11):
    """slot of a (field, row) key in embed_ids_hot_bwd_kernel's direct-mapped cache"""
    key = (field << 24) | row
    return ((key * 2654435761) & 0xFFFFFFFF) >> (32 - slots_log2)


def colliding_rows(vocab, field_a=0, field_b=1):
    """the first (row of field_a, row of field_b), both > 0, whose keys share a slot"""
    for a in range(1, vocab):
        for b in range(1, vocab):
            if hot_slot(field_a, a) == hot_slot(field_b, b):
                return a, b
    raise AssertionError("no colliding pair")


def first_diff(got: torch.Tensor, want: torch.Tensor):
    """None, or 'row r, column c: got g, want w' of the first element that differs (NaN equals NaN)"""
    same = (got == want) | (got.isnan() & want.isnan())
    if bool(same.all()):
        return None
    r, c = (int(v) for v in torch.nonzero(~same)[0])
    return f"row {r}, column {c}: got {float(got[r, c])!r}, want {float(want[r, c])!r} ({int((~same).sum())} differ)"
