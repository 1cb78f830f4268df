"""float64 restatement of ctr_linear_fwd / ctr_linear_bwd as include/ctrhip.h words them, the comparisons that go with it,
the operands both sides share and the table of cases tests/test_gpu_linear_arms.py runs.  Plain torch on the CPU: nothing
here imports the HIP library, so tests/test_linear_ref_cpu.py can show without a GPU that every comparison rejects a
slightly wrong kernel at every case of the table.

    y  = act(x w^T + b + residual)
    gz = gy * act'(y)            (through the saved OUTPUT y: relu mask y > 0, sigmoid y (1 - y))
    gx (= | +=) gz w             gw += gz^T x             gb += sum_m gz

The reference is applied to the STARTING contents of gx / gw / gb: gw and gb start as randn * sqrt(m) (the gradient's own
magnitude), gx as NaN when it is assigned and as randn when it is accumulated.  Every operand is a view into a larger
buffer (leading dimension, element offset); what a strided output's buffer holds outside the view is SENTINEL and has
to stay so.

Tolerances are those of tests/test_gpu_ops.py (test_linear_forward / test_linear_backward), with inputs drawn the same
way (randn, w / sqrt(k)): forward rtol 1e-5, atol 4e-6; gx rtol 1e-5, atol 1e-5; gw and gb rtol 1e-5, atol 2e-6 max(1,
sqrt(m)), the allowed error being atol + rtol |float64 result, starting contents included|.

WORKSPACE EXTENT.  Each backward case names the arm of ctr_linear_bwd it claims and the number of workspace floats that
arm writes, derived in the comment beside it from the constants of the entry points:

    single unit   (linear_n1.hip)     grid (k + 1);  grid = min(ceil(m lpr / 256), 1024), lpr = pow2_ceil(k / 4 or k) <= 64;
                                      slabs need gw, grid > 8 and grid (k + 1) <= workspace_floats, else atomics (0)
    skinny        (linear_skinny.hip) blocks (n k + n);  blocks = min(2048, floor(workspace / slab)), then
                                      rows_per_wave = ceil(m / 4 blocks), blocks = ceil(m / 4 rows_per_wave)
    direct-to-LDS (gemm_dlds_dw.hip)  parts (n k + (gb ? n : 0));  parts = min(2 kCtrCUs / (ty tz), floor(workspace / slab)),
                                      rows = max(128, ceil16(ceil(m / parts))), parts = ceil(m / rows)
    tile slabs    (linear.hip)        splits n k (+ splits n behind them with gb);  splits = min(ceil(target / tiles),
                                      ceil(m / 128)), target = 1536 (1024 from 4 tiles on), clamped to fit = floor(workspace
                                      / (n k + n)) when fit >= 8; slabs need splits > 8 and splits (n k + n) <= workspace
    atomic epilogues                  0

The GPU test holds the table against the floats that were really written: that is how a test knows which arm ran, and
what ties the table to the C code.  plan_bwd() below is no second authority: it is the arithmetic of the comments in
Python, restricted to the conditions the table's operands vary (y and gy are always contiguous here, for instance), so
that the CPU test catches a slip in a hand-derived extent before a GPU run does.  When the entry points change, the GPU
test says so; plan_bwd() and the comments are then corrected together, or plan_bwd() is dropped."""
import math
import zlib
from dataclasses import dataclass
from typing import Optional

import torch

ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
CTR_OK, CTR_EINVAL, CTR_ELIMIT = 0, -1, -2
SENTINEL = -12345.5
GUARD = 1 << 16              # floats on either side of the workspace slice
AMPLE = 1 << 23              # workspace floats that clamp no arm of the table (the largest extent is 4325376)

FWD_TOL = dict(rtol=1e-5, atol=4e-6)
GX_TOL = dict(rtol=1e-5, atol=1e-5)


def gw_tol(m):
    return dict(rtol=1e-5, atol=2e-6 * max(1.0, m ** 0.5))


# ---------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------
def check_close(got, want, rtol, atol, what):
    """|got - want| <= atol + rtol |want| per element (a NaN fails); prints and returns the worst |err| / allowed"""
    got = got.detach().cpu().to(torch.float64)
    want = want.detach().cpu().to(torch.float64)
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    if got.numel() == 0:
        return 0.0
    err = (got - want).abs()
    ratio = err / (atol + rtol * want.abs())
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max())
    print(f"{what}: max |err| {float(torch.nan_to_num(err, nan=float('inf')).max()):.3e}, max |err| / allowed {worst:.3f}")
    assert worst <= 1.0, f"{what}: max |err| / allowed = {worst}"
    return worst


def check_gaps(buf, spec, what):
    """everything of the flat buffer outside the view keeps SENTINEL"""
    buf = buf.detach().cpu()
    inside = torch.zeros(buf.numel(), dtype=torch.bool)
    inside.as_strided((spec.rows, spec.cols), (spec.ld, 1), spec.off).fill_(True)
    touched = int(((buf != SENTINEL) & ~inside).sum())
    print(f"{what}: {touched} floats outside the view written")
    assert touched == 0, f"{what}: {touched} floats outside the view were written"


def rejects(check, *args, **kw):
    """True when ``check`` raises AssertionError"""
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


def written(ws_slice):
    """which floats of the workspace slice were written (no longer hold SENTINEL)"""
    return ws_slice != SENTINEL


def extent_of(mask):
    """one past the last written float, and how many below it were written"""
    idx = torch.nonzero(mask.reshape(-1))
    if idx.numel() == 0:
        return 0, 0
    return int(idx.max()) + 1, int(idx.numel())


# ---------------------------------------------------------------------------------------------------------------
# operands: views into larger buffers
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class View:
    rows: int
    cols: int
    ld: int
    off: int

    def numel(self):
        return self.off + (self.rows - 1) * self.ld + self.cols + 5 if self.rows else self.off + 5

    def of(self, buf):
        return buf.as_strided((self.rows, self.cols), (self.ld, 1), self.off)

    def aligned16(self):
        """16-byte aligned rows, given a 16-byte aligned buffer"""
        return self.off % 4 == 0 and self.ld % 4 == 0


def place(spec, values):
    """a SENTINEL-filled flat float32 buffer with ``values`` in the view"""
    buf = torch.full((spec.numel(),), SENTINEL, dtype=torch.float32)
    spec.of(buf).copy_(values)
    return buf


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def _act(z, act):
    return torch.relu(z) if act == ACT_RELU else torch.sigmoid(z) if act == ACT_SIGMOID else z


def _act_grad(y, act):
    if act == ACT_RELU:
        return (y > 0).to(torch.float64)
    if act == ACT_SIGMOID:
        return y * (1 - y)
    return torch.ones_like(y)


def linear_fwd_ref(x, w, bias, residual, act, tail0=None, mutate=None):
    """float64 y.  ``mutate`` (negative controls; ``tail0`` = first column of the second launch): "res_tail_col0" takes
    the residual of the tail columns from column 0 on, "bias_tail0" the tail's bias from bias[0] on (a launch whose
    pointer was not advanced)"""
    z = x.double() @ w.double().t()
    n = w.shape[0]
    if bias is not None:
        b = bias.double().clone()
        if mutate == "bias_tail0":
            b[tail0:] = bias.double()[:n - tail0]
        z = z + b
    if residual is not None:
        r = residual.double().clone()
        if mutate == "res_tail_col0":
            r[:, tail0:] = residual.double()[:, :n - tail0]
        z = z + r
    return _act(z, act)


BWD_MUTATIONS = ("drop_first_chunk", "drop_last_chunk", "assign_gw", "assign_gb", "gb_twice", "shift_chunk",
                 "relu_from_gy", "gx_flip", "write_gaps")
FWD_MUTATIONS = ("res_tail_col0", "bias_tail0")


def linear_bwd_ref(x, w, y, gy, act, gx0, gw0, gb0, accumulate, mutate=None):
    """float64 {gx, gw, gb} from the starting contents (None: not asked for).  ``mutate``: the negative controls of
    tests/test_linear_ref_cpu.py (a kernel that is wrong in one small way)"""
    gyd = gy.double()
    m, n = gyd.shape
    if act == ACT_NONE:
        gz = gyd
    elif mutate == "relu_from_gy":
        gz = gyd * (gyd > 0)
    else:
        gz = gyd * _act_grad(y.double(), act)
    out = {"gx": None, "gw": None, "gb": None}
    if gx0 is not None:
        acc = accumulate != (mutate == "gx_flip")
        prod = gz @ w.double()
        out["gx"] = gx0.double() + prod if acc else prod
    if gw0 is not None:
        xd = x.double()
        lo, hi = 0, m
        if mutate == "drop_first_chunk":
            lo = min(128, m)
        if mutate == "drop_last_chunk":
            hi = 128 * ((m - 1) // 128)
        gzs, xs = gz[lo:hi], xd[lo:hi]
        sw = gzs.t() @ xs
        k = xd.shape[1]
        if mutate == "shift_chunk":      # columns [c0, c0 + 4) land one row (one column, for a single row) further
            c0 = 4 * (k // 8)
            c1 = min(c0 + 4, k)
            sw[:, c0:c1] = sw[:, c0:c1].roll(1, 0 if n > 1 else 1)
        out["gw"] = sw if mutate == "assign_gw" else gw0.double() + sw
        if gb0 is not None:
            sb = gzs.sum(0)
            if mutate == "gb_twice":
                sb = 2 * sb
            out["gb"] = sb if mutate == "assign_gb" else gb0.double() + sb
    return out


# ---------------------------------------------------------------------------------------------------------------
# backward cases
# ---------------------------------------------------------------------------------------------------------------
SLAB_ARMS = ("n1_slab", "skinny", "dlds_dw", "tile_slab", "tile_seg")    # sums formed in a fixed order
ATOMIC_ARMS = ("n1_atomic", "tile_atomic")
ARMS = SLAB_ARMS + ATOMIC_ARMS + ("none",)                               # none: no weight gradient asked for


@dataclass
class BwdCase:
    name: str
    m: int
    n: int
    k: int
    arm: str
    extent: int
    act: int = ACT_NONE
    ws: Optional[int] = AMPLE       # workspace_floats; None: NULL workspace
    gx: bool = True
    gw: bool = True
    gb: bool = True
    acc: bool = False               # accumulate_gx
    ldx: int = 0                    # 0: k
    xoff: int = 0
    ldw: int = 0
    woff: int = 0
    ldgx: int = 0
    ldgw: int = 0
    gwoff: int = 0
    same_xgy: bool = False          # x and gy are one pointer (n == k)
    no_w: bool = False              # w == NULL (gx == NULL)

    def views(self):
        m, n, k = self.m, self.n, self.k
        return {"x": View(m, k, self.ldx or k, self.xoff), "w": View(n, k, self.ldw or k, self.woff),
                "y": View(m, n, n, 0), "gy": View(m, n, n, 0), "gx": View(m, k, self.ldgx or k, 0),
                "gw": View(n, k, self.ldgw or k, self.gwoff), "gb": View(1, n, n, 0)}

    def fixed_order(self):
        return self.arm in SLAB_ARMS


def bwd_operands(c):
    """{name: (View, flat buffer)} of the case, drawn as test_linear_backward draws them; y is the float32 image of the
    float64 forward (the layer's saved output).  Outputs hold their starting contents."""
    gen = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    m, n, k = c.m, c.n, c.k
    x = torch.randn(m, k, generator=gen)
    w = torch.randn(n, k, generator=gen) / k ** 0.5
    b = torch.randn(n, generator=gen)
    gy = x.clone() if c.same_xgy else torch.randn(m, n, generator=gen)
    y = linear_fwd_ref(x, w, b, None, c.act).float()
    gx0 = torch.randn(m, k, generator=gen) if c.acc else torch.full((m, k), float("nan"))
    gw0 = torch.randn(n, k, generator=gen) * m ** 0.5
    gb0 = torch.randn(1, n, generator=gen) * m ** 0.5
    v = c.views()
    vals = {"x": x, "w": w, "y": y, "gy": gy, "gx": gx0, "gw": gw0, "gb": gb0}
    return {name: (v[name], place(v[name], vals[name])) for name in vals}


def bwd_reference(c, ops_, mutate=None):
    g = lambda name: ops_[name][0].of(ops_[name][1])  # noqa: E731
    return linear_bwd_ref(g("x"), g("w"), g("y"), g("gy"), c.act, g("gx") if c.gx else None, g("gw") if c.gw else None,
                          g("gb").reshape(-1) if c.gb else None, c.acc, mutate)


def check_bwd(c, got, want):
    """got: {gx, gw, gb} (the views after the call; None where not asked for); returns the worst |err| / allowed"""
    worst = 0.0
    if c.gx:
        worst = max(worst, check_close(got["gx"], want["gx"], what=f"{c.name} gx", **GX_TOL))
    if c.gw:
        worst = max(worst, check_close(got["gw"], want["gw"], what=f"{c.name} gw", **gw_tol(c.m)))
    if c.gb:
        worst = max(worst, check_close(got["gb"].reshape(-1), want["gb"], what=f"{c.name} gb", **gw_tol(c.m)))
    return worst


def mutation_applies(c, mutate):
    """False where the mutation is the identity on this case (it names an output or a mask the case does not have)"""
    if mutate in ("drop_first_chunk", "drop_last_chunk", "assign_gw", "shift_chunk"):
        return c.gw and (mutate != "shift_chunk" or c.n > 1 or c.k > 1)
    if mutate in ("assign_gb", "gb_twice"):
        return c.gb
    if mutate == "relu_from_gy":
        return c.act == ACT_RELU and (c.gx or c.gw)
    if mutate == "gx_flip":
        return c.gx
    if mutate == "write_gaps":
        return c.gw and (c.ldgw or c.k) != c.k
    raise ValueError(mutate)


# ---- the dispatch of ctr_linear_bwd, restated (csrc/linear.hip, linear_n1.hip, linear_skinny.hip, gemm_dlds_dw.hip) ----
K_CUS = 256                   # kCtrCUs
MAX_SEGMENTS = 40             # CTR_MAX_SEGMENTS


def _cdiv(a, b):
    return -(-a // b)


def pick_nt(n):
    return 1 if n <= 32 else 2 if n <= 64 else 4


def padded(rows, cols):
    nt = pick_nt(cols)
    return _cdiv(rows, 128) * 128 * _cdiv(cols, 32 * nt) * 32 * nt


def effective_splits(K, splits):
    chunk = _cdiv(_cdiv(K, splits), 16) * 16
    return _cdiv(K, chunk)


def plan_bwd(c):
    """(arm, workspace floats written) of the case: a consistency check of the table's comments (see the module text)"""
    m, n, k, ws = c.m, c.n, c.k, c.ws
    v = c.views()
    x16 = v["x"].aligned16()
    contiguous_gw = (c.ldgw or k) == k
    if not (c.gx or c.gw):
        return "none", 0
    if n == 1 and k <= 512:                                      # ctr_n1_supported: k <= 64 * 8
        vec = k % 4 == 0 and x16 and v["w"].aligned16() and (not c.gx or v["gx"].aligned16())
        units = k // 4 if vec else k
        lpr = min(64, 1 << max(0, math.ceil(math.log2(units))))
        grid = min(max(1, _cdiv(m * lpr, 256)), K_CUS * 8, 1024)
        slabs = c.gw and ws is not None and ws >= grid * (k + 1) and grid > 8
        return ("n1_slab", grid * (k + 1)) if slabs else (("n1_atomic", 0) if c.gw else ("none", 0))
    if not c.gw:
        return "none", 0
    if ws is not None and k in (8, 16, 32) and n <= 64 and m >= 65536 and contiguous_gw and x16:
        slab = n * k + n
        blocks = min(2048, ws // slab)
        if blocks >= 1:
            rows_per_wave = _cdiv(m, blocks * 4)
            return "skinny", _cdiv(m, rows_per_wave * 4) * slab
    if ws is not None and contiguous_gw and m >= 4096 and ((n >= 96 and k >= 32) or (k >= 96 and n >= 32)):
        swap = n < 96 or (k >= 96 and padded(k, n) < padded(n, k))
        wide, narrow = (k, n) if swap else (n, k)
        ty, tz = _cdiv(wide, 128), _cdiv(narrow, 32 * pick_nt(narrow))
        slab = n * k + (n if c.gb else 0)
        parts = min(max(1, K_CUS * 2 // (ty * tz)), ws // slab)
        if parts >= 1:
            rows = max(128, _cdiv(_cdiv(m, parts), 16) * 16)
            return "dlds_dw", _cdiv(m, rows) * slab
    tiles_nk = _cdiv(n, 128) * _cdiv(k, 32 * pick_nt(k))
    tiles_kn = _cdiv(k, 128) * _cdiv(n, 32 * pick_nt(n))
    tiles = min(tiles_nk, tiles_kn)
    target = 1024 if tiles >= 4 else 1536
    splits = max(1, min(_cdiv(target, tiles), _cdiv(m, 128)))
    slab = n * k
    if ws is not None and splits > 8:
        fit = ws // (slab + n)
        if fit >= 8 and splits > fit:
            splits = fit
    splits = effective_splits(m, splits)
    seg_ok = contiguous_gw or n + 1 <= MAX_SEGMENTS
    if splits > 8 and ws is not None and ws >= splits * (slab + n) and seg_ok:
        return ("tile_slab" if contiguous_gw else "tile_seg"), splits * slab + (splits * n if c.gb else 0)
    return "tile_atomic", 0


R, S = ACT_RELU, ACT_SIGMOID
BWD_CASES = [
    # ---- single unit (linear_n1.hip): k % 4 == 0 and aligned rows -> lpr = pow2_ceil(k / 4)
    # k = 64: lpr 16, grid = ceil(5000 * 16 / 256) = 313 > 8, slab k + 1 = 65: 313 * 65 = 20345
    BwdCase("n1_slabs", 5000, 1, 64, "n1_slab", 313 * 65, act=S),
    # one float short of 313 slabs: atomics (the grid is capped at 128 then)
    BwdCase("n1_one_float_short", 5000, 1, 64, "n1_atomic", 0, act=S, ws=313 * 65 - 1),
    BwdCase("n1_null_workspace", 5000, 1, 64, "n1_atomic", 0, act=R, ws=None),
    # grid = ceil(100 * 16 / 256) = 7 <= 8: atomics even with a workspace
    BwdCase("n1_grid7", 100, 1, 64, "n1_atomic", 0),
    # k = 20: 5 vector lanes -> lpr 8, grid = ceil(5000 * 8 / 256) = 157, slab 21: 3297
    BwdCase("n1_k20_vector_lanes", 5000, 1, 20, "n1_slab", 157 * 21, act=R),
    # k = 3, x one float off a 16-byte boundary: scalar lanes, lpr 4, grid = ceil(5000 * 4 / 256) = 79, slab 4: 316
    BwdCase("n1_k3_scalar_lanes", 5000, 1, 3, "n1_slab", 79 * 4, act=S, ldx=5, xoff=1),
    # k > 512: not a single-unit kernel.  Tile dX with contraction n = 1; tile dW: tiles = min(1 * 5, 5 * 1) = 5 >= 4 ->
    # target 1024 -> 205 chunks, capped at ceil(1200 / 128) = 10 > 8: slabs, 10 * 516 weights + 10 * 1 bias
    BwdCase("n1_k516_tile", 1200, 1, 516, "tile_slab", 10 * 516 + 10, act=S),
    # ceil(1025 / 128) = 9 chunks of 128 rows: 9 * 513 + 9
    BwdCase("n1_k513_tile", 1025, 1, 513, "tile_slab", 9 * 513 + 9, act=R),

    # ---- skinny (linear_skinny.hip): m = 65536, slab = n k + n = 816 / 2112
    # ample: 2048 blocks, rows_per_wave = ceil(65536 / 8192) = 8, blocks = ceil(65536 / 32) = 2048
    BwdCase("skinny_48x16", 65536, 48, 16, "skinny", 2048 * 816, act=R),
    BwdCase("skinny_64x32", 65536, 64, 32, "skinny", 2048 * 2112, act=S, gx=False),
    # room for 100 slabs: rows_per_wave = ceil(65536 / 400) = 164, blocks = ceil(65536 / 656) = 100: to the last float
    BwdCase("skinny_48x16_100_slabs", 65536, 48, 16, "skinny", 100 * 816, ws=100 * 816, gx=False),
    BwdCase("skinny_64x32_100_slabs", 65536, 64, 32, "skinny", 100 * 2112, act=R, ws=100 * 2112),
    # less than one slab: ctr_skinny_dw has no block to run and the call falls through to the tile kernel, where
    # tiles = 1 -> 1536 chunks, capped at 512; fit = 0 < 8 and 512 * 816 floats are not there: atomics (64 chunks)
    BwdCase("skinny_48x16_short_workspace", 65536, 48, 16, "tile_atomic", 0, act=R, ws=815),
    BwdCase("skinny_64x32_short_workspace", 65536, 64, 32, "tile_atomic", 0, ws=2111, gx=False),
    BwdCase("skinny_48x16_null", 65536, 48, 16, "tile_atomic", 0, ws=None, gx=False),
    BwdCase("skinny_64x32_null", 65536, 64, 32, "tile_atomic", 0, act=S, ws=None),
    # ldgw = 2k: refused by the skinny and the direct-to-LDS dW; n + 1 = 49 / 65 > 40 segments: atomic epilogue
    BwdCase("skinny_48x16_ldgw_2k", 65536, 48, 16, "tile_atomic", 0, ldgw=32, gx=False),
    BwdCase("skinny_64x32_ldgw_2k", 65536, 64, 32, "tile_atomic", 0, act=R, ldgw=64, gwoff=32, gx=False),
]

# ---- direct-to-LDS dW (gemm_dlds_dw.hip), m = 4100.  parts = 512 / (ty tz) -> rows = ceil16(ceil(4100 / parts)) < 128 ->
# 128 rows per part -> ceil(4100 / 128) = 33 parts.  Room for 3 slabs: rows = ceil16(1367) = 1376 -> 3 parts.  Less than
# one slab: CTR_ELIMIT inside, on to the tile kernel: 33 chunks, fit = 0 < 8, no room for 33 slabs: atomics.
#   128 x 32:  n >= 96 -> not swapped, ty = tz = 1.   32 x 96: n < 96 -> swapped, ty = tz = 1.
#   41 x 96:   swapped, 64-unit tile (pick_nt(41) = 2), ty = tz = 1, with an n tail: 41 % 4 = 1, so the last chunk of a
#              gy / y row is fetched from column 37 and unit 40 is read 3 floats further right (tail_shift on the n side)
#   161 x 163: padded(163, 161) = padded(161, 163) = 256 * 256 -> not swapped, ty = tz = 2, parts = 128; rows of x, gy and
#              gw on 4-byte boundaries only
# The kernel is instantiated per (tile width, activation, orientation) and reads y only with an activation: the ample
# workspace runs every shape with all three.  WHAT THE EXTENT SHOWS: with an ample workspace the tile-slab arm would
# make the same 33 chunks and write the same number of floats (only the bias is laid out differently), so the
# `_ample` extents do not tell the two arms apart; the `_3_slabs` cases do (there the tile kernel has fit = 3 < 8 and
# 33 chunks: atomics, nothing written).
for _n, _k, _ca in ((128, 32, R), (32, 96, ACT_NONE), (41, 96, R), (161, 163, S)):
    for _gb in (True, False):
        _slab = _n * _k + (_n if _gb else 0)
        _tag = f"dlds_dw_{_n}x{_k}_{'gb' if _gb else 'nogb'}"
        BWD_CASES += [
            BwdCase(f"{_tag}_ample", 4100, _n, _k, "dlds_dw", 33 * _slab, act=_ca, gb=_gb, gx=_gb),
            BwdCase(f"{_tag}_3_slabs", 4100, _n, _k, "dlds_dw", 3 * _slab, act=_ca, gb=_gb, gx=False, ws=3 * _slab),
            BwdCase(f"{_tag}_short", 4100, _n, _k, "tile_atomic", 0, act=_ca, gb=_gb, gx=not _gb, ws=_slab - 1),
        ]
        BWD_CASES += [BwdCase(f"{_tag}_ample_act{_a}", 4100, _n, _k, "dlds_dw", 33 * _slab, act=_a, gb=_gb, gx=False)
                      for _a in (ACT_NONE, R, S) if _a != _ca]

BWD_CASES += [
    # ---- tile kernel dW (linear.hip).  tiles = 1 for n, k <= 128 -> 1536 chunks, capped at ceil(m / 128)
    # 64 x 128: padded(128, 64) = 128 * 64 < padded(64, 128) = 128 * 128 -> swapped (X^T gZ); 10 chunks: 10 * 8192 + 10 * 64
    BwdCase("tile_swapped", 1200, 64, 128, "tile_slab", 10 * 8192 + 10 * 64, act=R),
    # 128 x 64: not swapped; 10 * 8192 + 10 * 128
    BwdCase("tile_not_swapped", 1200, 128, 64, "tile_slab", 10 * 8192 + 10 * 128, act=S),
    # the chunk boundary: 1024 rows = 8 chunks, not more than 8 -> atomics; 1025 rows = 9 -> slabs, 9 * 960 + 9 * 24
    BwdCase("tile_m1024_8_chunks", 1024, 24, 40, "tile_atomic", 0, act=S),
    BwdCase("tile_m1025_9_chunks", 1025, 24, 40, "tile_slab", 9 * 960 + 9 * 24, act=S),
    # the workspace clamp: 2000 rows = 16 chunks; room for exactly 9 slab + bias pairs -> fit = 9 >= 8 -> 9 chunks of
    # ceil16(ceil(2000 / 9)) = 224 rows, the workspace used to its last float; room for 7 -> fit < 8 -> 16 chunks, atomics
    BwdCase("tile_clamped_to_9", 2000, 24, 40, "tile_slab", 9 * 984, act=R, ws=9 * 984),
    BwdCase("tile_room_for_7", 2000, 24, 40, "tile_atomic", 0, act=R, ws=7 * 984),
    # NULL workspace, 128 * 65 + 1 rows = 66 chunks: capped at 64 (m >= 4096, but the direct-to-LDS dW needs a workspace)
    BwdCase("tile_null_64_chunk_cap", 128 * 65 + 1, 24, 40, "tile_atomic", 0, ws=None),
    BwdCase("tile_m1", 1, 24, 40, "tile_atomic", 0, act=S),
    BwdCase("tile_m127", 127, 24, 40, "tile_atomic", 0, act=R),
]

# ---- strided gw, the NeuralCF form: w and gw are the halves [:, :k] / [:, k:] of (n, 2k) matrices, gb on the second
# call only, gx accumulated.  Refused by the direct-to-LDS dW (ldgw != k).  n + 1 <= 40: slabs + one reduction segment per
# row; n = 40, 64: atomic epilogue.  k = 40: slab = 40 n; 1200 rows = 10 chunks, 4100 rows = 33 chunks (of 128 rows)
for _m, _chunks in ((1200, 10), (4100, 33)):
    for _n in (24, 39, 40, 64):
        _seg = _n + 1 <= 40
        _ha = {24: R, 39: S}.get(_n, ACT_NONE)        # (NeuralCF calls without one; the segment arm reads y like any other)
        BWD_CASES += [
            BwdCase(f"halves_n{_n}_m{_m}_first", _m, _n, 40, "tile_seg" if _seg else "tile_atomic",
                    _chunks * 40 * _n if _seg else 0, act=_ha, gb=False, acc=True, ldw=80, ldgw=80),
            BwdCase(f"halves_n{_n}_m{_m}_second", _m, _n, 40, "tile_seg" if _seg else "tile_atomic",
                    _chunks * (40 * _n + _n) if _seg else 0, act=_ha, acc=True, ldw=80, woff=40, ldgw=80, gwoff=40),
        ]

BWD_CASES += [
    # ---- which outputs are asked for (1200 x 24 x 40: 10 chunks, slab 960)
    BwdCase("gx_only", 300, 24, 40, "none", 0, act=R, gw=False, gb=False),
    BwdCase("gw_and_gb_only", 1200, 24, 40, "tile_slab", 10 * 960 + 10 * 24, act=S, gx=False),
    BwdCase("gw_without_gb", 1200, 24, 40, "tile_slab", 10 * 960, act=R, gb=False),
    BwdCase("gw_only_null_w", 1200, 24, 40, "tile_slab", 10 * 960, gx=False, gb=False, no_w=True),
    # PNN's p = S^T S: x and gy one pointer, n = k = 40: 10 * 1600
    BwdCase("x_is_gy", 1200, 40, 40, "tile_slab", 10 * 1600, gx=False, gb=False, same_xgy=True),
    # DIN: x a column slice, gw without gb, gx accumulated
    BwdCase("column_slice_x", 1200, 36, 24, "tile_slab", 10 * 864, gb=False, acc=True, ldx=48, xoff=24),
    # the direct-to-LDS dX splits its columns: 161 = 128 + 33, 129 = 96 + 33 (a remainder of 1 borrows 32); gx strided
    BwdCase("dx_split_161_accumulate", 300, 32, 161, "none", 0, act=R, gw=False, gb=False, acc=True, ldgx=164),
    BwdCase("dx_split_129_accumulate", 300, 32, 129, "none", 0, act=S, gw=False, gb=False, acc=True, ldgx=132),
    BwdCase("dx_split_161_assign", 300, 32, 161, "none", 0, gw=False, gb=False, ldgx=164),
    # n < 4 or k < 4: the tile dX (300 rows = 3 chunks: atomics)
    BwdCase("tile_dx_n2", 300, 2, 40, "tile_atomic", 0, act=R),
    BwdCase("tile_dx_n3", 300, 3, 40, "tile_atomic", 0, act=S, acc=True, ldgx=43),
    BwdCase("tile_dx_k3", 300, 24, 3, "tile_atomic", 0, act=R),
]


def bwd_case(name):
    return next(c for c in BWD_CASES if c.name == name)


# ---------------------------------------------------------------------------------------------------------------
# forward cases: (name, m, n, k, act, first column of the second launch or of the negative control's "tail")
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class FwdCase:
    name: str
    m: int
    n: int
    k: int
    act: int
    tail0: Optional[int]      # first column the mutations treat as the second launch (None: a single column)
    arm: str                  # what ctr_linear_fwd does with it (not observable: a note for the reader)


FWD_CASES = [
    # tail_cols: m >= 4096, n > 128, n % 128 in 1..16 -> the last n % 128 columns get a launch of their own
    FwdCase("tail_2_of_130", 4096, 130, 40, R, 128, "direct-to-LDS 128 + direct-to-LDS 2"),
    FwdCase("tail_16_of_144", 4096, 144, 40, S, 128, "direct-to-LDS 128 + direct-to-LDS 16"),
    FwdCase("no_tail_145", 4096, 145, 40, R, 128, "n % 128 = 17: no tail; gemm_dlds.hip splits 128 + 17 itself"),
    FwdCase("no_tail_m4095", 4095, 130, 40, ACT_NONE, 128, "m < 4096: one direct-to-LDS launch of 130 columns"),
    FwdCase("tail_1_of_129", 4096, 129, 40, S, 128, "direct-to-LDS 128 + single-unit kernel"),
    FwdCase("tail_k3", 4096, 130, 3, R, 128, "k < 4: both launches on the tile kernel"),
    FwdCase("n1_k516", 1200, 1, 516, S, None, "k > 512: direct-to-LDS forward"),
    FwdCase("n1_k513", 1200, 1, 513, R, None, "k > 512: direct-to-LDS forward, 4-byte aligned rows"),
]
# the tile forward: k < 4
FWD_CASES += [FwdCase(f"tile_k{_k}_act{_a}", 300, 24, _k, _a, 12, "tile kernel") for _k in (1, 2, 3) for _a in (0, 1, 2)]


def fwd_operands(c):
    """x, w (/ sqrt(k)), bias, residual and a y buffer with ldy = n + 3 (NaN in the view, SENTINEL in the gaps)"""
    gen = torch.Generator().manual_seed(zlib.crc32(("fwd_" + c.name).encode()))
    x = torch.randn(c.m, c.k, generator=gen)
    w = torch.randn(c.n, c.k, generator=gen) / c.k ** 0.5
    b = torch.randn(c.n, generator=gen)
    r = torch.randn(c.m, c.n, generator=gen)
    yv = View(c.m, c.n, c.n + 3, 0)
    return x, w, b, r, yv, place(yv, torch.full((c.m, c.n), float("nan")))


def check_fwd(c, got, want):
    return check_close(got, want, what=f"{c.name} y", **FWD_TOL)
