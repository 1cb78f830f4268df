"""One case per dispatch arm of ctr_embed_fwd / ctr_embed_bwd (csrc/embed.hip, embed_sorted.hip, embed_bag.hip), on
the exact inputs of tests/embed_ref.py.  CPU only; tests/test_gpu_embed_arms.py runs every case forward and backward.

Each case names, as ``arm``, the kernel it is aimed at; the comment beside it holds the entry-point arithmetic that puts
it there.  Cases are registered by name and built on demand (``case(name)``): the largest holds 134 MB of gout."""
from __future__ import annotations

from typing import Callable, Dict, List, Tuple

import torch

import embed_ref as ref
from embed_ref import Build, Case, colliding_rows, sorted_need

_REG: Dict[str, Tuple[str, str, int, Callable, dict]] = {}


def _add(name, family, arm, batch, fill, **layout):
    assert name not in _REG
    _REG[name] = (family, arm, batch, fill, layout)


def names(family=None) -> List[str]:
    return [n for n, r in _REG.items() if family is None or r[0] == family]


def families() -> List[str]:
    return sorted({r[0] for r in _REG.values()})


def arm(name) -> str:
    return _REG[name][1]


def case(name) -> Case:
    family, arm_, batch, fill, layout = _REG[name]
    b = Build(name, family, arm_, batch)
    fill(b)
    return b.done(**layout)


def _idm(nf, width, vocab, pattern="uniform", bad=(), frozen=()):
    """nf id fields of one width, one table each, the columns of one (batch, nf) id matrix, packed left to right"""
    def fill(b):
        m = b.ids([vocab] * nf, pattern, bad)
        for f in range(nf):
            b.id(b.table(vocab, width, frozen=f in frozen), m, f)
    return fill


# ---------------------------------------------------------------------------------------------------------------
# forward, (B, F) id matrix
# ---------------------------------------------------------------------------------------------------------------
FAM, ARM = "fwd_ids", "embed_ids_fast_kernel"
# try_fast_ids: width % 4 == 0, lpr = width / 4 a power of two <= 64, out 16-byte aligned, ldo % 4 == 0, field i an
# ID_I64 at out_col i * width reading column i of one (B, F) matrix.  A workgroup pass takes per_block = (256 / lpr) * 2
# items; items = batch * F one short of and one past it:
#   width   4: lpr  1, per_block 512: 511 = 73 * 7,  513 = 171 * 3
#   width  16: lpr  4, per_block 128: 127 = 127 * 1, 129 = 43 * 3
#   width  64: lpr 16, per_block  32:  31 = 31 * 1,   33 = 11 * 3
#   width 256: lpr 64, per_block   8:   7 = 1 * 7,     9 = 3 * 3
for _w, _shapes in ((4, ((73, 7), (171, 3))), (16, ((127, 1), (43, 3))), (64, ((31, 1), (11, 3))), (256, ((1, 7), (3, 3)))):
    for _b, _nf in _shapes:
        _add(f"fwd_ids_w{_w}_items{_b * _nf}", FAM, ARM, _b, _idm(_nf, _w, 19, "ends"))
# batch 1: 5 items, one partly live pass
_add("fwd_ids_batch1", FAM, ARM, 1, _idm(5, 16, 11))
# bad ids in columns 0 and 2: row 0 is read, the flag raised
_add("fwd_ids_bad", FAM, ARM, 100, _idm(3, 16, 23, "zipf", bad=(0, 2)))
# refusals.  width 12: lpr 3 is no power of two; width 260 > 256: both fast paths refuse, 16-byte alignment holds
_add("fwd_ids_w12_refused", FAM, "embed_fwd_kernel<4>", 70, _idm(3, 12, 17, "ends"))
_add("fwd_ids_w260_refused", FAM, "embed_fwd_kernel<4>", 9, _idm(2, 260, 13))
# the out view one float off (first column 5 of a 16-byte aligned buffer) / ldo odd / a table one float off:
# ctr_aligned16(out), ldo % 4 == 0 or ctr_aligned16(table) fails in try_fast_ids, try_fast_rows and make_plan's vec4
_add("fwd_ids_out_shifted", FAM, "embed_fwd_kernel<1>", 70, _idm(3, 16, 17, bad=(1,)), left=5)
_add("fwd_ids_odd_ldo", FAM, "embed_fwd_kernel<1>", 70, _idm(3, 16, 17), ldo=4 + 48 + 5)


def _fill(b):
    m = b.ids([17, 17, 17])
    b.id(b.table(17, 16), m, 0)
    b.id(b.table(17, 16, shift=True), m, 1)
    b.id(b.table(17, 16), m, 2)


_add("fwd_ids_table_unaligned", FAM, "embed_fwd_kernel<1>", 70, _fill)

# ---------------------------------------------------------------------------------------------------------------
# forward, row fields from separate id columns
# ---------------------------------------------------------------------------------------------------------------
FAM, ARM = "fwd_rows", "embed_rows_fast_kernel"
# try_fast_rows: 1..8 fields, ID_I64 or PROD_I64 of one width (lpr a power of two), out_col % 4 == 0, any id column
# and stride.  try_fast_ids refuses first: field 0 is not at out_col 0, or it is a product.


# 8 fields at width 16 (lpr 4, per_block 64 * 4 = 256 items): batch 77 -> 616 items, 3 passes, the last partly live;
# out_col order 64, 0, 16, 32, 112, 128, 144, 160: columns 48..63 and 80..111 are written by nobody; idx_stride 3
def _fill(b):
    u, i = b.ids([21, 33, 21], "ends", bad=(1,)), b.ids([33, 21, 40], "zipf", bad=(2,))
    t = [b.table(v, 16) for v in (21, 33, 40, 21, 33, 21, 33, 40)]
    b.id(t[0], u, 0, out_col=64)
    b.id(t[1], u, 1, out_col=0)
    b.prod(t[3], u, 2, t[4], i, 0, out_col=16)
    b.id(t[2], i, 2, out_col=32)
    b.prod(t[5], i, 1, t[6], u, 1, out_col=112)          # bad ids in the second factor (u column 1)
    b.prod(t[1], u, 1, t[7], i, 2, out_col=128)          # bad ids in both factors, at the same samples
    b.id(t[6], i, 0, out_col=144)
    b.id(t[7], i, 2, out_col=160)


_add("fwd_rows_8_mixed", FAM, ARM, 77, _fill)


# a ninth field: n > 8 refuses, the generic kernel takes all nine (everything aligned: VEC 4)
def _fill(b):
    u = b.ids([21, 33], "uniform", bad=(0,))
    t = [b.table(21 if k % 2 == 0 else 33, 16) for k in range(10)]
    b.prod(t[0], u, 0, t[1], u, 1)
    for k in range(2, 10):
        b.id(t[k], u, k % 2)


_add("fwd_rows_9_refused", FAM, "embed_fwd_kernel<4>", 77, _fill)


# width 64 (lpr 16, per_block 16 * 4 = 64 items), batch 1000 x 3 fields: NeuralCF's form, 47 passes; bad ids in the
# first factor only
def _fill(b):
    u, i = b.ids([50], "zipf", bad=(0,)), b.ids([70], "uniform")
    tu, ti, gu, gi = b.table(50, 64), b.table(70, 64), b.table(50, 64), b.table(70, 64)
    b.id(tu, u)
    b.id(ti, i)
    b.prod(gu, u, 0, gi, i, 0)


_add("fwd_rows_ncf_bad_first", FAM, ARM, 1000, _fill)

# ---------------------------------------------------------------------------------------------------------------
# forward, generic kernel
# ---------------------------------------------------------------------------------------------------------------
FAM = "fwd_generic"


def _all_kinds(width, bag_rows=5):
    """one field of every kind: ID_I64 (bad ids), ID_F32 (bad ids), BAG, DENSE at an x column that is a multiple of
    four, PROD_I64 (bad ids in both factors, at the same samples)"""
    def fill(b):
        m = b.ids([29, 31], "ends", bad=(0, 1))
        b.id(b.table(29, width), m, 0)
        b.idf(b.table(37, width), "zipf", bad=True)
        b.bag(b.table(bag_rows, width))
        b.pad_x()
        b.dense(width)
        b.pad_x()
        b.prod(b.table(29, width), m, 0, b.table(31, width), m, 1)
    return fill


# batch < 4096 keeps the bag in the gather kernel; x, out and tables 16-byte aligned, ldx % 4 == 0, widths and columns
# multiples of four -> VEC 4: 5 fields x 2 units = 10 units per sample, 370 units
_add("fwd_generic_all_kinds_vec4", FAM, "embed_fwd_kernel<4>", 37, _all_kinds(8))
# width 6: width % 4 != 0 -> VEC 1, 30 units per sample
_add("fwd_generic_all_kinds_vec1", FAM, "embed_fwd_kernel<1>", 37, _all_kinds(6))


# grid = min(ceil(batch * units / 256), 2048): three width-12 id fields and a width-4 dense column are 10 units of four
# floats; batch 52500 -> 525000 units > 2048 * 256 = 524288: threads 0..711 take a second trip
def _fill(b):
    m = b.ids([300, 400, 500], "zipf", bad=(1,))
    for f, v in enumerate((300, 400, 500)):
        b.id(b.table(v, 12), m, f)
    b.dense(4)


_add("fwd_generic_grid_stride", FAM, "embed_fwd_kernel<4>", 52500, _fill)

# ---------------------------------------------------------------------------------------------------------------
# forward, wide bags
# ---------------------------------------------------------------------------------------------------------------
FAM, ARM = "fwd_bag", "bag_fwd_kernel"


# ctr_embed_fwd_bags: batch >= 4096, BAG of width >= 32, width % 4 == 0, table 16-byte aligned; at most 16 bags.
# rows 1, 3, 4, 5, 21: the 4-unrolled loop runs 0, 0, 1, 1, 5 times, the tail 1, 3, 0, 1, 1 times.
# batch 4095: refused, the bags stay in embed_fwd_kernel<4>
def _fill(b):
    for rows in (1, 3, 4, 5, 21):
        b.bag(b.table(rows, 32))


_add("fwd_bag_rows_b4096", FAM, ARM, 4096, _fill)
_add("fwd_bag_rows_b4095", FAM, "embed_fwd_kernel<4>", 4095, _fill)


# width 36 is taken (9 units per sample), width 28 < 32 refused: the re-plan leaves one bag to the gather kernel
def _fill(b):
    b.bag(b.table(3, 36))
    b.bag(b.table(4, 28))


_add("fwd_bag_w36_w28", FAM, ARM + " + embed_fwd_kernel<4>", 4096, _fill)


# 17 bags of width 32: B.n stops at 16, the 17th is the gather kernel's
def _fill(b):
    for _ in range(17):
        b.bag(b.table(2, 32))


_add("fwd_bag_17", FAM, ARM + " + embed_fwd_kernel<4>", 4096, _fill)


# ldo odd: vec_store 0, four 4-byte stores per unit
def _fill(b):
    b.bag(b.table(5, 32))
    b.bag(b.table(2, 64))


_add("fwd_bag_odd_ldo", FAM, ARM, 4096, _fill, ldo=4 + 96 + 5)


# bags beside id fields: handled = {bags}, nrest = 2 < nfields = 4 -> make_plan again over the two id fields
def _fill(b):
    m = b.ids([600, 700], "quarter0", bad=(0,))
    b.id(b.table(600, 16), m, 0)
    b.bag(b.table(4, 32))
    b.id(b.table(700, 8), m, 1)
    b.bag(b.table(21, 32))


_add("fwd_bag_beside_ids", FAM, ARM + " + embed_fwd_kernel<4>", 4096, _fill)

# ---------------------------------------------------------------------------------------------------------------
# backward, lean scatter of an id matrix
# ---------------------------------------------------------------------------------------------------------------
FAM, ARM = "bwd_fast", "embed_ids_fast_bwd_kernel"
# try_fast_ids_bwd: the id-matrix shape, width a power of two <= 64.  The sorted path stays out because
# batch < 8 * vocab (300 < 400, 200 < 320); items = batch * F < 512 * 1024 keeps the hot kernel out
_add("bwd_fast_w1", FAM, ARM, 300, _idm(3, 1, 50, "zipf", bad=(0, 2)))
_add("bwd_fast_w2_quarter0", FAM, ARM, 300, _idm(3, 2, 50, "quarter0"))
_add("bwd_fast_w8_frozen", FAM, ARM, 300, _idm(4, 8, 50, "ends", bad=(1,), frozen=(2,)))
_add("bwd_fast_w64", FAM, ARM, 200, _idm(2, 64, 40, "quarter0", bad=(1,)))
# items = 512 * 1024 - 1 = 524287 (a prime: one field); vocab 70000 > 8192 keeps the sorted path out
_add("bwd_fast_items_below_hot", FAM, ARM, 524287, _idm(1, 1, 70000, "zipf", bad=(0,)))

# ---------------------------------------------------------------------------------------------------------------
# backward, hot-row scatter
# ---------------------------------------------------------------------------------------------------------------
FAM = "bwd_hot"
# items >= 512 * 1024, width <= 32, every vocab < 2^24; <11> unless 2048 * width * 4 > 140 KiB (width 32 -> <9>).
# 256 workgroups of 1024 threads walk per = ceil(items / 256) items each.  vocab 9000 > 8192 keeps the sorted path out.
# width 1, items = 8 * 65536 = 524288 exactly: per 2048; an item's one lane answers itself (__shfl branch)
_add("bwd_hot_w1_items_exact", FAM, "embed_ids_hot_bwd_kernel<11> __shfl", 65536,
     _idm(8, 1, 9000, "zipf", bad=(0, 5), frozen=(3,)))


# width 4, items = 8 * 65539 = 524312 = 2048 * 256 + 24: per 2049, 256 workgroups, the last one short.  Row a of field
# 0 and row b of field 1 share a slot ((key * 2654435761 mod 2^32) >> 21, key = field << 24 | row) and fill a third
# of their column each: one is admitted, the other stays on global atomics.  Row 8999 of field 2 is touched exactly
# twice, at samples 1000 and 1050 (items 8002 and 8402: one workgroup's slice)
def _fill(b):
    m = b.ids([9000] * 8, "zipf", bad=(7,))
    ra, rb = colliding_rows(9000)
    ids = b.mats[m]
    s = torch.arange(b.batch)
    ids[s % 3 == 0, 0] = ra
    ids[s % 3 == 1, 1] = rb
    ids[ids[:, 2] == 8999, 2] = 8998
    ids[1000, 2] = ids[1050, 2] = 8999
    for f in range(8):
        b.id(b.table(9000, 4), m, f)


_add("bwd_hot_w4_collision", FAM, "embed_ids_hot_bwd_kernel<11> __shfl", 65539, _fill)
# width 16: an item is one DPP row, the first lane's answer comes by row broadcast
_add("bwd_hot_w16_dpp", FAM, "embed_ids_hot_bwd_kernel<11> DPP", 65536, _idm(8, 16, 9000, "zipf", bad=(2,)))
# width 32: 2048 * 32 * 4 = 256 KiB > 140 KiB -> <9>
_add("bwd_hot_w32_slots9", FAM, "embed_ids_hot_bwd_kernel<9> __shfl", 65536,
     _idm(8, 32, 9000, "quarter0", bad=(4,), frozen=(0,)))
# width 64 > 32: the plain scatter at any size
_add("bwd_hot_w64_stays_plain", FAM, "embed_ids_fast_bwd_kernel", 65536, _idm(8, 64, 9000, "zipf", bad=(1,)))

# ---------------------------------------------------------------------------------------------------------------
# backward, sorted path
# ---------------------------------------------------------------------------------------------------------------
FAM, ARM = "bwd_sorted", "seg_reduce_kernel"


# ctr_embed_bwd_sorted takes a field when width % 4 == 0, out_col % 4 == 0, width <= 256, the gradient is 16-byte
# aligned, vocab <= 8192 and batch >= 8 * vocab.  lpr = pow2_ceil(width / 4) lanes own a sorted position; a workgroup
# has 256 / lpr groups of 8 positions.
#   width   4: lpr  1;  width 12: lpr 4 (3 live lanes, 1 dead);  width 20: lpr 8 (5 live, 3 dead);
#   width 256: lpr 64 (4 groups of 8 positions per workgroup).  401 % 8 = 1, 203 % 8 = 3: the last group is short
def _two_columns(width, vocab, pattern):
    def fill(b):
        m = b.ids([vocab, vocab], pattern, bad=(0, 1))
        b.id(b.table(vocab, width), m, 0)
        b.id(b.table(vocab, width), m, 1)
    return fill


for _w, _v, _b, _p in ((4, 50, 401, "uniform"), (12, 33, 300, "zipf"), (20, 25, 203, "quarter0"), (256, 20, 200, "ends")):
    _add(f"bwd_sorted_w{_w}", FAM, ARM, _b, _two_columns(_w, _v, _p))
# width 260 > 256: shape_ok fails; wider than 64, so the lean scatter refuses as well
_add("bwd_sorted_w260_refused", FAM, "embed_bwd_kernel<1>", 200, _idm(1, 260, 20, "ends", bad=(0,)))
# thresholds: vocab 37, batch 296 = 8 * 37 taken, 295 refused (the id matrix then takes the lean scatter);
# vocab 8192 at batch 65536 = 8 * 8192 taken (64 sort workgroups of 1024 samples), vocab 8193 > kMaxVocab refused
_add("bwd_sorted_batch_eq_8v", FAM, ARM, 296, _idm(2, 8, 37, "ends", bad=(0,)))
_add("bwd_sorted_batch_8v_minus_1", FAM, "embed_ids_fast_bwd_kernel", 295, _idm(2, 8, 37, "ends", bad=(0,)))
_add("bwd_sorted_vocab_8192", FAM, ARM, 65536, _idm(1, 4, 8192, "ends", bad=(0,)))
_add("bwd_sorted_vocab_8193", FAM, "embed_ids_fast_bwd_kernel", 65544, _idm(1, 4, 8193, "ends", bad=(0,)))
# batch 140000 > 131072: nblk = min(137, 128) = 128, chunk = ceil(140000 / 128) = 1094 > 1024 samples per sort
# workgroup.  One id field: |g| <= 1 is 64 units per sample, 140000 * 64 < 2^24 even if every id were equal
_add("bwd_sorted_batch_140000", FAM, ARM, 140000, _idm(1, 4, 100, "zipf", bad=(0,)))
# one run over the whole batch (every group's head meets its neighbours in the LDS merge) / ids already sorted
_add("bwd_sorted_all_equal", FAM, ARM, 1000, _idm(1, 8, 16, "equal", bad=(0,)))
_add("bwd_sorted_sorted_ids", FAM, ARM, 1000, _idm(1, 8, 64, "sorted", bad=(0,)))


# ID_F32: the job reads its ids from an x column
def _fill(b):
    b.idf(b.table(30, 8), "zipf", bad=True)
    b.idf(b.table(41, 4), "ends")


_add("bwd_sorted_id_f32", FAM, ARM, 333, _fill)


# two tables on one id column: one job, two streams
def _fill(b):
    m = b.ids([30], "zipf", bad=(0,))
    b.id(b.table(30, 4), m)
    b.id(b.table(30, 12), m)


_add("bwd_sorted_two_tables_one_column", FAM, ARM, 300, _fill)
# nine id columns: kMaxJobs = 8, job_of returns -1 for the ninth, which embed_bwd_kernel<1> scatters in the same call
# (the lean scatter is skipped: the sorted path took something)
_add("bwd_sorted_9_jobs", FAM, ARM + " + embed_bwd_kernel<1>", 100, _idm(9, 4, 10, "uniform", bad=(0, 8)))


# 17 fields on three columns: kMaxStreams = 16, the 17th goes to embed_bwd_kernel<1>
def _fill(b):
    m = b.ids([12, 12, 12], "uniform", bad=(1,))
    for k in range(17):
        b.id(b.table(12, 4), m, k % 3)


_add("bwd_sorted_17_streams", FAM, ARM + " + embed_bwd_kernel<1>", 128, _fill)


# NeuralCF's form: MLP user / item rows and the GMF product on the same two columns; each job's companion column is
# the product's other factor (use_ckeys 1 on both streams).  Bad ids in both columns, at the same samples
def _fill(b):
    u, i = b.ids([20], "zipf", bad=(0,)), b.ids([30], "ends", bad=(0,))
    b.id(b.table(20, 8), u)
    b.id(b.table(30, 8), i)
    b.prod(b.table(20, 8), u, 0, b.table(30, 8), i, 0)


_add("bwd_sorted_prod_companion", FAM, ARM, 400, _fill)


# a product alone with the bad ids in one column only: the first factor's, then the second factor's (width 12: lpr 4)
def _one_bad(second):
    def fill(b):
        u = b.ids([20], "zipf", bad=() if second else (0,))
        i = b.ids([30], "uniform", bad=(0,) if second else ())
        b.prod(b.table(20, 12), u, 0, b.table(30, 12), i, 0)
    return fill


_add("bwd_sorted_prod_bad_first", FAM, ARM, 400, _one_bad(False))
_add("bwd_sorted_prod_bad_second", FAM, ARM, 400, _one_bad(True))


# two products on first column c0 with partners c1 and c2: job(c0)'s companion is c1 (the first product wins), so the
# second product's first stream has use_ckeys 0 and loads its partner ids itself.  Bad ids in c0 and c2
def _fill(b):
    m = b.ids([20, 30, 25], "zipf", bad=(0, 2))
    b.prod(b.table(20, 8), m, 0, b.table(30, 8), m, 1)
    b.prod(b.table(20, 8), m, 0, b.table(25, 8), m, 2)


_add("bwd_sorted_two_prods_one_column", FAM, ARM, 400, _fill)


# the same with bad ids in c2 alone: only the stream that loads its partner ids itself sees them
def _fill(b):
    m = b.ids([20, 30, 25], "zipf", bad=(2,))
    b.prod(b.table(20, 8), m, 0, b.table(30, 8), m, 1)
    b.prod(b.table(20, 8), m, 0, b.table(25, 8), m, 2)


_add("bwd_sorted_two_prods_bad_partner", FAM, ARM, 400, _fill)


# a product of two tables on ONE id column: j1 == j2, the job is its own companion
def _fill(b):
    m = b.ids([30], "zipf", bad=(0,))
    b.prod(b.table(30, 8), m, 0, b.table(30, 8), m, 0)


_add("bwd_sorted_prod_same_column", FAM, ARM, 300, _fill)


# a product with its second gradient missing: g2 false, refused -> embed_bwd_kernel<1> with grad2 NULL
def _fill(b):
    m = b.ids([20, 30], "zipf", bad=(0, 1))
    b.prod(b.table(20, 8), m, 0, b.table(30, 8, frozen=True), m, 1)


_add("bwd_sorted_prod_one_grad", FAM, "embed_bwd_kernel<1>", 300, _fill)


# a gradient one float off 16-byte alignment: refused, the id matrix takes the lean scatter
def _fill(b):
    m = b.ids([30], "zipf", bad=(0,))
    b.id(b.table(30, 8, grad_shift=True), m)


_add("bwd_sorted_grad_unaligned", FAM, "embed_ids_fast_bwd_kernel", 300, _fill)
# the workspace through the C entry: NULL refuses; one job of vocab 10 at batch 100 needs
# 2 * ceil4(1 * 10) + ceil4(10) + 2 * 100 = 236 floats: 236 is taken (and written), 235 refused (left untouched)
assert sorted_need(100, [(10, False)]) == 236
_add("bwd_sorted_ws_null", FAM, "embed_ids_fast_bwd_kernel", 100, _idm(1, 4, 10, bad=(0,)), ws=None)
_add("bwd_sorted_ws_exact", FAM, ARM, 100, _idm(1, 4, 10, bad=(0,)), ws=236, ws_written=True)
_add("bwd_sorted_ws_one_short", FAM, "embed_ids_fast_bwd_kernel", 100, _idm(1, 4, 10, bad=(0,)), ws=235, ws_written=False)

# ---------------------------------------------------------------------------------------------------------------
# backward, bag tables
# ---------------------------------------------------------------------------------------------------------------
FAM, ARM = "bwd_bag", "bag_bwd_kernel"


# ctr_embed_bwd_bags: workspace present, width a power of two <= 1024, rows <= 32; at most 16 bags;
# nblk = min(ceil(batch / 128), 512) slabs; one launch per register tile: rows <= 2 -> <2>, <= 8 -> <8>, <= 32 -> <32>.
# make_plan bounds the stage first: sum of widths <= 4096 floats, sum of rows * width * 4 <= 96 KiB.
# rows 2 | 3, 8 | 9, 32 sit on the tile edges; 33 > 32 is left to embed_bwd_kernel<1> (LDS accumulators, slabs);
# batch 300 -> 3 slabs
def _fill(b):
    for rows in (2, 3, 8, 9, 32, 33):
        b.bag(b.table(rows, 16))


_add("bwd_bag_row_tiles", FAM, ARM + "<2|8|32> + embed_bwd_kernel<1>", 300, _fill)


# widths 1, 16, 64, 128 (2 chunks along blockIdx.z), 1024 (16 chunks) in one call: <2> gets widths 1 and 1024 in one
# launch (zmax 16: the width-1 bag's workgroups with blockIdx.z > 0 return), <8> widths 16 and 64, <32> width 128;
# width 24 is no power of two -> embed_bwd_kernel<1>
def _fill(b):
    for rows, width in ((2, 1), (3, 16), (8, 64), (9, 128), (2, 1024), (5, 24)):
        b.bag(b.table(rows, width))


_add("bwd_bag_widths", FAM, ARM + "<2|8|32> + embed_bwd_kernel<1>", 300, _fill)


# 17 bags: B.n stops at 16, the 17th is left to embed_bwd_kernel<1>
def _fill(b):
    for _ in range(17):
        b.bag(b.table(3, 4))


_add("bwd_bag_17", FAM, ARM + "<8> + embed_bwd_kernel<1>", 260, _fill)


# NULL workspace (C entry): no bag kernel and no slabs: LDS accumulators flushed with atomics, grid cap 128
def _fill(b):
    b.bag(b.table(3, 16))
    b.bag(b.table(9, 8))


_add("bwd_bag_ws_null", FAM, "embed_bwd_kernel<1> atomics", 300, _fill, ws=None)


# bag_floats = 172 * 24 = 4128 > 4096 (width 24: generic): grid = ceil(3000 * 24 / 256) = 282, capped at 256 slabs with
# the wrapper's workspace and at 64 workgroups of atomics without one
def _fill(b):
    b.bag(b.table(172, 24))


_add("bwd_bag_floats_4128_slabs", FAM, "embed_bwd_kernel<1> slabs", 3000, _fill)
_add("bwd_bag_floats_4128_atomics", FAM, "embed_bwd_kernel<1> atomics", 3000, _fill, ws=None)


# bags beside id fields with bad ids: the sorted path takes the vocab-20 field (300 >= 160), the bag kernel the bag,
# embed_bwd_kernel<1> the vocab-500 field (row 0, a quarter of the ids, summed in LDS: hot_floats 8)
def _fill(b):
    m = b.ids([20, 500], "quarter0", bad=(0, 1))
    b.id(b.table(20, 8), m, 0)
    b.bag(b.table(5, 16))
    b.id(b.table(500, 8), m, 1)


_add("bwd_bag_beside_ids", FAM, ARM + "<8> + seg_reduce_kernel + embed_bwd_kernel<1>", 300, _fill)

# ---------------------------------------------------------------------------------------------------------------
# backward, generic kernel
# ---------------------------------------------------------------------------------------------------------------
FAM = "bwd_generic"
# all five kinds at width 6 (width % 4 != 0 and no power of two: no other path takes a field), with the wrapper's
# workspace (slabs for the bag) and with NULL (atomics)
_add("bwd_generic_all_kinds_slabs", FAM, "embed_bwd_kernel<1> slabs", 37, _all_kinds(6))
_add("bwd_generic_all_kinds_atomics", FAM, "embed_bwd_kernel<1> atomics", 37, _all_kinds(6), ws=None)


# ---------------------------------------------------------------------------------------------------------------
# the entry points' selectors, restated: which kernels a case launches
# ---------------------------------------------------------------------------------------------------------------
def _pow2(v):
    return v > 0 and v & (v - 1) == 0


def _id_matrix_shape(c, w):
    """field i is an ID_I64 of width w at out_col i * w reading column i of one (batch, nfields) matrix"""
    n, m = len(c.specs), c.specs[0].ikey
    return c.specs[0].kind == ref.ID_I64 and all(s.kind == ref.ID_I64 and s.width == w and s.out_col == i * w and s.ikey == (m[0], i) and s.idx_stride == n
               for i, s in enumerate(c.specs))


def _tables_aligned(c, s):
    return s.tkey not in c.table_shift and (s.tkey2 is None or s.tkey2 not in c.table_shift)


def forward_kernels(c: Case):
    """ctr_embed_fwd: try_fast_ids, try_fast_rows, ctr_embed_fwd_bags, then the gather kernel over the rest"""
    S, w = c.specs, c.specs[0].width
    io16 = c.left % 4 == 0 and c.ldo % 4 == 0             # ctr_aligned16(out) && ldo % 4 == 0
    lanes = w % 4 == 0 and w <= 256 and _pow2(w // 4)
    if lanes and io16 and _id_matrix_shape(c, w) and all(_tables_aligned(c, s) for s in S):
        return {"embed_ids_fast_kernel"}
    if (len(S) <= 8 and lanes and io16 and all(s.kind in (ref.ID_I64, ref.PROD_I64) and s.width == w and s.out_col % 4 == 0
                                                and _tables_aligned(c, s) for s in S)):
        return {"embed_rows_fast_kernel"}
    bags = [s for s in S if s.kind == ref.BAG and s.width >= 32 and s.width % 4 == 0 and _tables_aligned(c, s)]
    bags = bags[:16] if c.batch >= 4096 else []
    rest = [s for s in S if not any(s is b for b in bags)]
    out = {"bag_fwd_kernel"} if bags else set()
    if rest:
        vec4 = io16 and all(s.width % 4 == 0 and s.out_col % 4 == 0 and (s.kind == ref.DENSE or _tables_aligned(c, s))
                            and (s.kind != ref.DENSE or (c.x.shape[1] % 4 == 0 and s.src_col % 4 == 0)) for s in rest)
        out.add("embed_fwd_kernel<4>" if vec4 else "embed_fwd_kernel<1>")
    return out


def backward_kernels(c: Case):
    """ctr_embed_bwd: the sorted path, else the lean / hot scatter of an id matrix; then the bag kernel and
    embed_bwd_kernel<1> (a backward plan always has one float per unit) over what is left"""
    S, batch = c.specs, c.batch
    ws_floats = {"ops": 16 * 1024 * 1024, None: 0}.get(c.ws, c.ws)
    has = lambda key: key is not None and key not in c.frozen                      # noqa: E731
    g16 = lambda key: has(key) and key not in c.grad_shift                       # noqa: E731
    small = lambda v: v <= 8192 and batch >= 8 * v                               # noqa: E731
    handled, jobs, comp, streams = set(), [], set(), 0
    if c.ws is not None and c.left % 4 == 0 and c.ldo % 4 == 0:
        for i, s in enumerate(S):
            if not (s.width % 4 == 0 and s.out_col % 4 == 0 and s.width <= 256):
                continue
            if s.kind in (ref.ID_I64, ref.ID_F32) and g16(s.tkey) and small(s.table.shape[0]):
                key = (s.ikey if s.kind == ref.ID_I64 else ("x", s.src_col), s.table.shape[0])
                if streams + 1 > 16 or (key not in jobs and len(jobs) == 8):
                    continue
                jobs += [key] if key not in jobs else []
                streams += 1
                handled.add(i)
            elif (s.kind == ref.PROD_I64 and g16(s.tkey) and g16(s.tkey2) and small(s.table.shape[0])
                  and small(s.table2.shape[0]) and _tables_aligned(c, s)):
                keys = list(dict.fromkeys([(s.ikey, s.table.shape[0]), (s.ikey2, s.table2.shape[0])]))
                new = [k for k in keys if k not in jobs]
                if streams + 2 > 16 or len(jobs) + len(new) > 8:
                    continue
                jobs += new
                comp |= set(keys)
                streams += 2
                handled.add(i)
        need = sorted_need(batch, [(k[1], k in comp) for k in jobs])
        if need > ws_floats:
            handled = set()
        else:
            ws_floats -= need
    out = {"seg_reduce_kernel"} if handled else set()
    w = S[0].width
    if not handled and _pow2(w) and w <= 64 and _id_matrix_shape(c, w):
        hot = w <= 32 and batch * len(S) >= 512 * 1024 and len(S) <= 255 and all(s.table.shape[0] < 2 ** 24 for s in S)
        return {("embed_ids_hot_bwd_kernel<9>" if 2048 * w * 4 > 140 * 1024 else "embed_ids_hot_bwd_kernel<11>")
                if hot else "embed_ids_fast_bwd_kernel"}
    if c.ws is not None and c.x is not None:
        bags = [i for i, s in enumerate(S) if s.kind == ref.BAG and has(s.tkey) and _pow2(s.width) and s.width <= 1024
                and s.bag_size <= 32][:16]
        slab = sum(S[i].bag_size * S[i].width for i in bags)
        if bags and min(-(-batch // 128), 512) * slab <= ws_floats:
            handled |= set(bags)
            out |= {f"bag_bwd_kernel<{2 if S[i].bag_size <= 2 else 8 if S[i].bag_size <= 8 else 32}>" for i in bags}
    if any(i not in handled and s.kind != ref.DENSE and (has(s.tkey) or has(s.tkey2)) for i, s in enumerate(S)):
        out.add("embed_bwd_kernel<1>")
    return out


def claimed_kernels(arm_):
    """'bag_bwd_kernel<2|8|32> + embed_bwd_kernel<1> slabs' -> the four kernel names"""
    out = set()
    for part in arm_.split(" + "):
        name = part.split(" ")[0]
        if "|" in name:
            stem, tail = name.split("<")
            out |= {f"{stem}<{t}>" for t in tail.rstrip(">").split("|")}
        else:
            out.add(name)
    return out


# cases whose reference takes well under a second: the CPU tests' autograd comparison and mutations run on these (the
# hot-row family's two narrowest cases stand for it)
SMALL = [n for n, r in _REG.items() if r[2] <= 5000 or n in ("bwd_hot_w1_items_exact", "bwd_hot_w4_collision")]
