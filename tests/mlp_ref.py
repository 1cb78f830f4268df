"""float64 restatement of ctr_mlp_fwd / ctr_mlp_head_fwd / ctr_mlp_bwd as include/ctrhip.h words them, the comparisons
that go with it, the operands both sides share, the tables of cases tests/test_gpu_mlp_arms.py runs and plan(), the
arithmetic of csrc/mlp_fused.hip's build() and dispatch in Python.  Plain torch on the CPU: nothing here imports the HIP
library, so tests/test_mlp_ref_cpu.py can show without a GPU that every comparison rejects a slightly wrong kernel at
every case.

    y_i  = act_i(y_{i-1} W_i^T + b_i)              (y_{-1} = x; b_i may be NULL)
    out  = act(x_extra . w[:p] + y_last . w[p:] + c)
    gz_i = gy_i * act_i'(y_i)                      (through the SAVED output: relu mask y > 0, sigmoid y (1 - y))
    gw_i += gz_i^T y_{i-1}      gb_i += sum_m gz_i      gy_{i-1} = gz_i W_i      gx = gz_0 W_0 (assigned)

The references are applied to the STARTING contents of gw / gb, drawn as randn * sqrt(m) (the gradient's own
magnitude); gx and every forward output start as NaN.  Every operand is a view (leading dimension, element offset)
into a larger buffer whose other floats hold SENTINEL and have to keep it; a buffer reaches one whole row past the
view, so that a kernel writing the row behind a ragged last tile is seen.  The saved outputs a backward case reads are
the float32 image of the float64 forward: the backward is judged on its own.

TWO COMPARISONS, both against float64 and never against the fused kernel's own output of another run:

* layer-local, at the dense layer's tolerances (linear_ref.FWD_TOL, gw_tol(m)): y_i against float64 of layer i applied
  to the saved y_{i-1} the call itself wrote; gw_i / gb_i against the float64 product of the reference gz_i (the float64
  chain from gy through the saved outputs, masks from the saved outputs) and the saved input.  The kernel's gz_i has
  come through the fp32 chain of the layers above, which the dense layer's tolerance has to absorb; where it cannot,
  the rule is in check_bwd()'s text, not a wider number.
* end to end: the last y (rtol 1e-5, atol 1e-5), the head (rtol 1e-5, atol 2e-6) and gx (rtol 1e-4, atol 1e-5) against
  the float64 stack on the original input -- the tolerances tests/test_gpu_ops.py holds the same quantities to.

plan() IS NO SECOND AUTHORITY.  It restates build() and the dispatch of the three entry points so that the case tables
can say which arm a case claims and the CPU test can show that every arm has a case.  What ties it to the C code is what
the GPU test can observe: the workspace floats the backward writes end exactly at grid * slab (so `slab`, the grid cap of
256 against DienAttShape's 512, and with it the pinned-shape match of DienAttShape are observed), and a refusal returns
the planned code and leaves every output and the workspace at the sentinel.  Claimed by arithmetic only: MAXT, the
flush's `copies`, the LDS strides and bytes, gvec, the straddling slot pairs, the remainder chunks, and the match of
NcfShape / NcfTowerShape (same grid cap as DynShape) -- a wrong result on those arms fails the comparisons, but nothing
shows that the arm named is the arm that ran.

copies == 1.  The flush keeps 4, 2 or 1 copies of a layer's n k + n sums in the dead weight and tile region (`avail`
floats).  test_mlp_ref_cpu.py enumerates every admissible 1- to 3-layer stack with widths in multiples of 8 up to 128:
within the 160 KB cap and 16 accumulator tiles copies == 1 is NOT reachable: of the 93641 layers flushed there, 93458
run with 4 copies, 183 with 2 (the narrowest is the single layer 72 -> 120; [80, 128, 8] is the case here) and none
with 1 -- a layer large enough to need it brings weights and tiles that make `avail` more than twice its sums.  The
single-copy arm of the flush is dead code under today's limits; it stays, since the limits are the host's to move."""
import re
import zlib
from dataclasses import dataclass, field
from typing import Optional

import torch

from linear_ref import (ACT_NONE, ACT_RELU, ACT_SIGMOID, CTR_EINVAL, CTR_ELIMIT, CTR_OK, FWD_TOL, GUARD,  # noqa: F401
                        SENTINEL, View, _act, _act_grad, check_close, check_gaps, extent_of, gw_tol, rejects, written)

CTR_EALIGN = -4
Y_TOL = dict(rtol=1e-5, atol=1e-5)        # last y, end to end
HEAD_TOL = dict(rtol=1e-5, atol=2e-6)
GX_E2E_TOL = dict(rtol=1e-4, atol=1e-5)
R, S, N = ACT_RELU, ACT_SIGMOID, ACT_NONE

# ---------------------------------------------------------------------------------------------------------------
# plan(): build() and the dispatch of csrc/mlp_fused.hip
# ---------------------------------------------------------------------------------------------------------------
K_WAVES, K_MAX_DIM, K_MAX_LAYERS, K_HEAD_MAX, K_SLACK = 4, 128, 8, 192, 32
LDS_CAP = 160 * 1024
STACK_DESC_BYTES = 888          # sizeof(StackDesc): 8 LayerDesc of 104 bytes + 6 ints + db_off[8]
PINNED = {                      # name: (N, K, ACT, MAXT of the backward)
    "NcfShape": ((64, 32, 16, 8, 64), (128, 64, 32, 16, 8), (R, R, R, R, N), 14),
    "NcfTowerShape": ((64, 32, 16, 8), (128, 64, 32, 16), (R, R, R, R), 12),
    "DienAttShape": ((64, 32, 1), (32, 64, 32), (R, R, N), 6),
}
NCF, NCF_TOWER, DIEN_ATT = ([128, 64, 32, 16, 8, 64], [128, 64, 32, 16, 8], [32, 64, 32, 1])


def _cdiv(a, b):
    return -(-a // b)


def _r(v, q):
    return _cdiv(v, q) * q


@dataclass
class Plan:
    code: int = CTR_OK
    tiles: list = field(default_factory=list)        # dW accumulator tiles per layer
    acc_off: list = field(default_factory=list)
    ntiles: int = 0
    maxt: Optional[int] = None
    sa: int = 0
    sb: int = 0
    wfloats: int = 0
    lds_bytes: int = 0
    slab: int = 0
    cap: int = 256
    grid: int = 0
    extent: int = 0                                  # workspace floats written: grid * slab (backward)
    copies: list = field(default_factory=list)
    dx_rem: list = field(default_factory=list)       # per layer: "0", "<=8", "<=16", "<=24", ">24"
    k_rem: list = field(default_factory=list)        # per layer: k % 32
    pair_roles: list = field(default_factory=list)   # per layer: set of "A", "B", "AB" over the slot pairs it is in
    two_rows_one_pair: list = field(default_factory=list)
    pinned: Optional[str] = None
    second_tile: bool = False
    odd_stride: bool = False                         # an LDS row pitch that is no multiple of 16 bytes
    gvec: bool = False


def plan(dims, acts, backward, m=1, *, ks=None, x_aligned=True, ldx=None, mid_aligned=True, has_gb=True, ws=None,
         head_p=None, head_ldx=None, gy_aligned=True, ldgy=None):
    """what the entry point does with a stack of widths ``dims`` (k0, n0, n1, ...) at ``m`` rows: Plan.code is the
    return value, the rest describes the launch.  ``ks`` overrides the k of the layers (a broken chain), ``ws`` is
    workspace_floats (None: ample), ``head_p``: the call is ctr_mlp_head_fwd"""
    ns = list(dims[1:])
    ks = list(ks) if ks is not None else list(dims[:-1])
    nl = len(ns)
    p = Plan()
    if m == 0:
        return p
    ldx = ks[0] if ldx is None else ldx
    if not x_aligned or ldx % 4:
        p.code = CTR_EALIGN
        return p
    if not 1 <= nl <= K_MAX_LAYERS:
        p.code = CTR_ELIMIT
        return p
    woff = 0
    for i, (n, k) in enumerate(zip(ns, ks)):
        if n < 1 or k < 8:
            p.code = CTR_EINVAL
        elif n > K_MAX_DIM or k > K_MAX_DIM or k % 8:
            p.code = CTR_ELIMIT
        elif i > 0 and k != ns[i - 1]:
            p.code = CTR_EINVAL
        elif i < nl - 1 and not mid_aligned:
            p.code = CTR_EALIGN
        elif backward and not has_gb:
            p.code = CTR_EINVAL
        if p.code != CTR_OK:
            return p
        p.acc_off.append(p.ntiles)
        p.tiles.append(_cdiv(n, 32) * _cdiv(k, 32))
        p.ntiles += p.tiles[-1]
        woff += _r(n, 8) * (k + 4) + _r(n, 4)
        p.slab += n * k + n
        rem = n % 32
        p.dx_rem.append("0" if rem == 0 else "<=8" if rem <= 8 else "<=16" if rem <= 16 else "<=24" if rem <= 24 else ">24")
        p.k_rem.append(k % 32)
    p.wfloats = _r(woff, 4)
    wa = wb = 0
    if backward:
        for i, (n, k) in enumerate(zip(ns, ks)):
            if (nl - 1 - i) % 2 == 0:
                wa, wb = max(wa, _r(n, 8)), max(wb, k)
            else:
                wb, wa = max(wb, _r(n, 8)), max(wa, k)
        tile_floats = K_WAVES * 32 * (wa + 4 + wb + 4)
        if max(n * k + n for n, k in zip(ns, ks)) > tile_floats:
            p.code = CTR_ELIMIT
            return p
        p.lds_bytes = 4 * (p.wfloats + tile_floats + K_WAVES * sum(ns) + K_SLACK)
    else:
        for i, (n, k) in enumerate(zip(ns, ks)):
            if i % 2:
                wb, wa = max(wb, k), max(wa, n)
            else:
                wa, wb = max(wa, k), max(wb, n)
        p.lds_bytes = 4 * (p.wfloats + K_WAVES * 32 * (wa + 4 + wb + 4) + K_SLACK)
    p.sa, p.sb = wa + 4, wb + 4
    p.odd_stride = p.sa % 4 != 0 or p.sb % 4 != 0
    if p.lds_bytes + STACK_DESC_BYTES > LDS_CAP:
        p.code = CTR_ELIMIT
        return p
    if ldx < ks[0]:
        p.code = CTR_EINVAL
        return p
    for name, (pn, pk, pa, _) in PINNED.items():
        if tuple(ns) == pn and tuple(ks) == pk and tuple(acts) == pa:
            p.pinned = name
    grid = _cdiv(_cdiv(m, 32), K_WAVES)
    if head_p is not None:
        if head_p > 64 or head_p % 8 or head_p + ns[-1] > K_HEAD_MAX:
            p.code = CTR_ELIMIT
        elif head_p and (head_ldx if head_ldx is not None else head_p) % 4:
            p.code = CTR_EALIGN
        if p.code != CTR_OK:
            return p
        p.pinned = p.pinned if p.pinned == "NcfTowerShape" else None      # every other stack: <DynShape, true>
    if backward:
        if p.ntiles > 16:
            p.code = CTR_ELIMIT
            return p
        p.maxt = 8 if p.ntiles <= 8 else 12 if p.ntiles <= 12 else 14 if p.ntiles <= 14 else 16
        if ws is not None and ws < min(grid, 256) * p.slab:
            p.code = CTR_ELIMIT
            return p
        if p.pinned:
            p.maxt = PINNED[p.pinned][3]
    if p.pinned == "DienAttShape" and 2 * p.lds_bytes <= LDS_CAP:
        p.cap = 512
    p.grid = min(grid, p.cap)
    if backward and ws is not None and ws < p.grid * p.slab:
        p.code = CTR_ELIMIT
        return p
    p.second_tile = _cdiv(m, 32) > p.grid * K_WAVES
    if backward:
        p.extent = p.grid * p.slab
        avail = p.wfloats + K_WAVES * 32 * (p.sa + p.sb)
        for i, (n, k) in enumerate(zip(ns, ks)):
            cnt = n * k + n
            p.copies.append(4 if 4 * cnt <= avail else 2 if 2 * cnt <= avail else 1)
            roles = set()
            two = False
            for s2 in range(0, p.maxt + p.maxt % 2, 2):
                a = 0 <= s2 - p.acc_off[i] < p.tiles[i]
                b = 0 <= s2 + 1 - p.acc_off[i] < p.tiles[i]
                if a or b:
                    roles.add("AB" if a and b else "A" if a else "B")
                nkt = _cdiv(k, 32)
                two = two or (a and b and (s2 - p.acc_off[i]) % nkt == 0 and (s2 + 1 - p.acc_off[i]) % nkt == 0)
            p.pair_roles.append(roles)
            p.two_rows_one_pair.append(two)
        ldgy = ns[-1] if ldgy is None else ldgy
        p.gvec = bool(p.pinned) and ns[-1] % 4 == 0 and ldgy % 4 == 0 and gy_aligned
    return p


def source_constants(text):
    """the constants plan() restates, read from the text of csrc/mlp_fused.hip"""
    out = {name: int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))
           for name in ("kWaves", "kMaxDim", "kMaxLayers", "kHeadMax", "kSlack")}
    act = {"CTR_ACT_NONE": N, "CTR_ACT_RELU": R, "CTR_ACT_SIGMOID": S}
    for shape in PINNED:
        body = re.search(rf"struct {shape} \{{(.*?)\n\}};", text, re.S).group(1)
        arr = lambda nm: re.search(rf"constexpr int {nm}\[\d+\] = \{{([^}}]*)\}};", body).group(1).split(",")  # noqa: E731
        out[shape] = (tuple(int(v) for v in arr("N")), tuple(int(v) for v in arr("K")), tuple(act[v.strip()] for v in arr("ACT")))
    return out


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    dims: list                      # k0, n0, n1, ...
    acts: list
    m: int
    claims: str                     # the arm the case is here for (held against plan() by the CPU test)
    nobias: tuple = ()              # layers with b == NULL
    gx: bool = True
    ldx_pad: int = 0                # ldx = k0 + ldx_pad, x starts xoff floats in
    xoff: int = 0
    ldy_pad: int = 0                # intermediate outputs: ldy = n + ldy_pad
    last_pad: int = 0               # the last output: ld = n + last_pad, last_off floats in
    last_off: int = 0
    gy_pad: int = 0
    gy_off: int = 0
    gx_pad: int = 0
    ws_room: int = 0                # workspace_floats = grid * slab + ws_room
    head_p: Optional[int] = None    # ctr_mlp_head_fwd with p extra columns
    head_act: int = S
    ldout: int = 1
    xe_pad: int = 0

    @property
    def nl(self):
        return len(self.dims) - 1

    def layers(self):
        return list(zip(self.dims[1:], self.dims[:-1]))          # (n, k)

    def plan(self, backward):
        return plan(self.dims, self.acts, backward, self.m, ldx=self.dims[0] + self.ldx_pad,
                    ldgy=self.dims[-1] + self.gy_pad, gy_aligned=self.gy_off % 4 == 0, head_p=self.head_p,
                    head_ldx=None if self.head_p is None else self.head_p + self.xe_pad)

    def views(self):
        m, d = self.m, self.dims
        v = {"x": View(m, d[0], d[0] + self.ldx_pad, self.xoff), "gx": View(m, d[0], d[0] + self.gx_pad, 0),
             "gy": View(m, d[-1], d[-1] + self.gy_pad, self.gy_off)}
        for i, (n, k) in enumerate(self.layers()):
            last = i == self.nl - 1
            v[f"y{i}"] = View(m, n, n + (self.last_pad if last else self.ldy_pad), self.last_off if last else 0)
            v[f"w{i}"] = v[f"gw{i}"] = View(n, k, k, 0)
            v[f"b{i}"] = v[f"gb{i}"] = View(1, n, n, 0)
        if self.head_p is not None:
            v["xe"] = View(m, self.head_p, self.head_p + self.xe_pad, 0)
            v["hw"] = View(1, self.head_p + d[-1], self.head_p + d[-1], 0)
            v["hc"] = View(1, 1, 1, 0)
            v["out"] = View(m, 1, self.ldout, 0)
        return v


A_DIMS, A_ACTS = [8, 24, 64, 16, 5], [R, S, R, N]
STACK_CASES = [
    Case("A_m37", A_DIMS, A_ACTS, 37, "MAXT 8, acc_off 0 1 3 5: every pair straddles two layers; k remainders 8 24 0 16; "
         "dX remainders 24 0 16 5, npad 3; b NULL on the first and a middle layer", nobias=(0, 2), ldy_pad=4),
    Case("A_second_tile", A_DIMS, A_ACTS, 32768 + 37, "DynShape: a wave's second tile, and it is the ragged one",
         ldx_pad=8, xoff=4, ws_room=1000),
    Case("B_one_tile_wide", [32, 64, 30], [R, S], 100, "MAXT 8; both slots of a pair start a row of tiles; dX remainder "
         "above 24, npad 2; sigmoid mask through an unaligned last y", last_pad=1, last_off=1, gy_pad=1, gy_off=1),
    Case("C_stride34", [8, 16, 30], [R, N], 100, "forward sa = 34: float4 LDS accesses at a 136-byte row pitch",
         last_pad=1, last_off=1, gx_pad=1),
    Case("D_maxt12", [64, 128, 8], [R, N], 129, "DynShape MAXT 12; gx == NULL", gx=False, ws_room=1000),
    Case("E_copies2", [80, 128, 8], [R, S], 4 * 32 * 3 + 5, "flush copies == 2 on layer 0; MAXT 16; LDS within 4 KB of the "
         "cap", ldy_pad=4),
    Case("G_tower_m37", NCF_TOWER, [R] * 4, 37, "pinned NcfTowerShape without a head, backward MAXT 12", ldx_pad=8, xoff=4,
         nobias=(1,)),
    Case("G_tower_second_tile", NCF_TOWER, [R] * 4, 65536 + 37, "pinned shape: a wave's second tile, ragged"),
    Case("H_dien_m100", DIEN_ATT, [R, R, N], 100, "DienAttShape: dot-product last layer, backward MAXT 6", last_pad=2,
         last_off=1, ws_room=1000),
    Case("H_dien_grid512", DIEN_ATT, [R, R, N], 65536 + 37, "DienAttShape: grid cap 512, extent 512 slab, second tile"),
    Case("I_ncf_ldgy65", NCF, [R, R, R, R, N], 1029, "NcfShape, gY rows at 65 floats: tile_load1 in a kPre kernel", gy_pad=1),
    Case("I_ncf_gy_off1", NCF, [R, R, R, R, N], 1029, "NcfShape, gY one float off 16 bytes: tile_load1 in a kPre kernel",
         gy_pad=4, gy_off=1),
    Case("I_ncf_gvec", NCF, [R, R, R, R, N], 1029, "NcfShape, gY as dwordx4 (the arm the two above leave)", ldx_pad=8, xoff=4),
    Case("J_maxt14", [24, 56, 104, 16], [R, R, R], 4097, "DynShape MAXT 14 through the C entry", ldx_pad=8, xoff=4, ldy_pad=4,
         nobias=(1,), last_pad=1, last_off=1),
    Case("J_maxt16", [64, 128, 8, 40, 1], [R, N, S, S], 1500, "DynShape MAXT 16 through the C entry; n = 1 behind a sigmoid",
         gx=False, gy_pad=2, gy_off=1),
]
STACK_CASES += [Case(f"A_m{_m}", A_DIMS, A_ACTS, _m, f"m = {_m}: one tile, {'ragged' if _m % 32 else 'full'}" if _m < 33 else
                     "m = 33: a second wave with a single row", last_pad=1, last_off=1) for _m in (1, 31, 32, 33)]
FWD_CASES = STACK_CASES
BWD_CASES = STACK_CASES
HEAD_CASES = [
    Case("head_A_p0", A_DIMS, A_ACTS, 37, "generic head, p = 0, odd n_last = 5", head_p=0, head_act=N),
    Case("head_A_p8_ldout3_second_tile", A_DIMS, A_ACTS, 32768 + 37, "p = 8, ldout = 3, ragged second tile", head_p=8,
         ldout=3, xe_pad=4, ldx_pad=8, xoff=4),
    Case("head_p64_n128", [64, 8, 128], [R, R], 100, "p + n_last = 192 = kHeadMax", head_p=64),
    Case("head_D_p8", [64, 128, 8], [R, N], 129, "p = 8 behind a wide layer", head_p=8, ldout=2, nobias=(0,)),
    Case("head_ncf_is_generic", NCF, [R, R, R, R, N], 100, "a pinned NcfShape stack with a head runs <DynShape, true>",
         head_p=16),
]
# case F: the forward runs fused, the backward's 8 + 8 + 2 accumulator tiles are refused and ops goes layer by layer.
# ([128, 128, 8] would not do: its forward needs 203 KB of LDS and is refused as well.)
F_DIMS, F_ACTS, F_M = [40, 104, 40, 8], [R, R, N], 1056


@dataclass
class Refusal:
    name: str
    entry: str                      # "fwd", "bwd" or "head"
    dims: list
    code: int
    m: int = 100
    ks: Optional[list] = None
    tweak: str = ""                 # x_off1, ldx_odd, mid_off1, no_gb, ws_short, head_ldx_odd
    head_p: Optional[int] = None

    def acts(self):
        if self.dims == DIEN_ATT:
            return [R, R, N]
        return [R] * (len(self.dims) - 1)

    def plan(self):
        backward = self.entry == "bwd"
        d = self.dims
        ws = None
        if self.tweak == "ws_short":
            ws = plan(d, self.acts(), True, self.m).extent - 1
        return plan(d, self.acts(), backward, self.m, ks=self.ks, x_aligned=self.tweak != "x_off1",
                    ldx=(self.ks or d)[0] + (1 if self.tweak == "ldx_odd" else 0), mid_aligned=self.tweak != "mid_off1",
                    has_gb=self.tweak != "no_gb", ws=ws, head_p=self.head_p,
                    head_ldx=None if self.head_p is None else self.head_p + (1 if self.tweak == "head_ldx_odd" else 0))


REFUSALS = [
    Refusal("k_not_multiple_of_8", "fwd", [12, 8, 8], CTR_ELIMIT),
    Refusal("k_below_8", "fwd", [4, 8, 8], CTR_EINVAL),
    Refusal("n_above_128", "fwd", [8, 136, 8], CTR_ELIMIT),
    Refusal("k_above_128", "bwd", [136, 8], CTR_ELIMIT),
    Refusal("nine_layers", "fwd", [8] * 10, CTR_ELIMIT),
    Refusal("broken_chain", "bwd", [8, 16, 8], CTR_EINVAL, ks=[8, 24]),
    Refusal("x_off_16_bytes", "fwd", [8, 16, 8], CTR_EALIGN, tweak="x_off1"),
    Refusal("x_off_16_bytes_bwd", "bwd", [8, 16, 8], CTR_EALIGN, tweak="x_off1"),
    Refusal("ldx_odd", "fwd", [8, 16, 8], CTR_EALIGN, tweak="ldx_odd"),
    Refusal("intermediate_y_off_16_bytes", "fwd", [8, 16, 8], CTR_EALIGN, tweak="mid_off1"),
    Refusal("lds_cap_eight_128x128", "fwd", [128] * 9, CTR_ELIMIT),
    Refusal("lds_cap_eight_128x128_bwd", "bwd", [128] * 9, CTR_ELIMIT),
    Refusal("seventeen_tiles", "bwd", F_DIMS, CTR_ELIMIT, m=F_M),
    Refusal("workspace_one_float_short", "bwd", A_DIMS, CTR_ELIMIT, m=1000, tweak="ws_short"),
    Refusal("dien_workspace_512_slabs_less_one", "bwd", DIEN_ATT, CTR_ELIMIT, m=65536 + 37, tweak="ws_short"),
    Refusal("backward_without_gb", "bwd", [8, 16, 8], CTR_EINVAL, tweak="no_gb"),
    Refusal("head_p72", "head", [8, 16, 8], CTR_ELIMIT, head_p=72),
    Refusal("head_p12", "head", [8, 16, 8], CTR_ELIMIT, head_p=12),
    Refusal("head_ldx_odd", "head", [8, 16, 8], CTR_EALIGN, head_p=8, tweak="head_ldx_odd"),
]


def arms_claimed():
    """{arm class: [cases]} over the tables, from plan(): what test_mlp_ref_cpu.py holds complete"""
    arms = {}

    def add(arm, name):
        if name not in arms.setdefault(arm, []):
            arms[arm].append(name)
    for c in BWD_CASES:
        b, f = c.plan(True), c.plan(False)
        assert b.code == CTR_OK and f.code == CTR_OK, c.name
        add(f"MAXT {b.maxt}" + (" pinned" if b.pinned else ""), c.name)
        for rem in b.dx_rem:
            add(f"dX remainder {rem}", c.name)
        for rem in f.k_rem:
            add(f"forward k remainder {rem}", c.name)
        for cp in b.copies:
            add(f"copies {cp}", c.name)
        for roles in b.pair_roles:
            for role in roles & {"A", "B"}:
                add(f"straddling pair, {role} only", c.name)
        if any(b.two_rows_one_pair):
            add("two rows of tiles in one pair", c.name)
        if f.odd_stride:
            add("odd forward stride", c.name)
        add(f"grid cap {b.cap}", c.name)
        if b.second_tile:
            add("second tile, " + ("pinned" if b.pinned else "DynShape"), c.name)
        if b.pinned:
            add(f"{b.pinned} without a head", c.name)
            if b.pinned != "DienAttShape":
                add("pinned gY " + ("dwordx4" if b.gvec else "tile_load1"), c.name)
    for c in HEAD_CASES:
        f = c.plan(False)
        assert f.code == CTR_OK, c.name
        add("generic head", c.name)
        if f.second_tile:
            add("generic head, second tile", c.name)
        if c.head_p + c.dims[-1] == K_HEAD_MAX:
            add("head at kHeadMax", c.name)
    for r in REFUSALS:
        add(f"refusal {r.code} ({r.entry})", r.name)
    return arms


REQUIRED_ARMS = (
    ["MAXT 8", "MAXT 12", "MAXT 14", "MAXT 16", "MAXT 14 pinned", "MAXT 12 pinned", "MAXT 6 pinned"]
    + [f"dX remainder {r}" for r in ("0", "<=8", "<=16", "<=24", ">24")] + [f"forward k remainder {r}" for r in (0, 8, 16, 24)]
    + ["copies 4", "copies 2", "straddling pair, A only", "straddling pair, B only", "two rows of tiles in one pair",
       "odd forward stride", "grid cap 256", "grid cap 512", "second tile, DynShape", "second tile, pinned",
       "NcfShape without a head", "NcfTowerShape without a head", "DienAttShape without a head", "pinned gY dwordx4",
       "pinned gY tile_load1", "generic head", "generic head, second tile", "head at kHeadMax"]
    + [f"refusal {code} ({entry})" for code, entry in ((CTR_ELIMIT, "fwd"), (CTR_ELIMIT, "bwd"), (CTR_ELIMIT, "head"),
                                                      (CTR_EINVAL, "fwd"), (CTR_EINVAL, "bwd"), (CTR_EALIGN, "fwd"),
                                                      (CTR_EALIGN, "bwd"), (CTR_EALIGN, "head"))])


# ---------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------
def place(spec, values):
    """a SENTINEL-filled flat float32 buffer with ``values`` in the view; it reaches one row past the view"""
    buf = torch.full((spec.off + spec.rows * spec.ld + spec.cols + 5,), SENTINEL, dtype=torch.float32)
    spec.of(buf).copy_(values)
    return buf


def blank(spec):
    return place(spec, torch.full((spec.rows, spec.cols), float("nan")))


def operands(c):
    """{name: (View, flat buffer)}.  x, w (/ sqrt(k)), b, gy drawn as tests/test_gpu_ops.py draws them; y_i the float32
    image of the float64 forward (what a backward reads); gw / gb at their non-zero start; gx, out: NaN"""
    gen = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    m = c.m
    scale = max(1, m) ** 0.5
    vals = {"x": torch.randn(m, c.dims[0], generator=gen), "gy": torch.randn(m, c.dims[-1], generator=gen),
            "gx": torch.full((m, c.dims[0]), float("nan"))}
    for i, (n, k) in enumerate(c.layers()):
        vals[f"w{i}"] = torch.randn(n, k, generator=gen) / k ** 0.5
        vals[f"b{i}"] = torch.randn(1, n, generator=gen)
        vals[f"gw{i}"] = torch.randn(n, k, generator=gen) * scale
        vals[f"gb{i}"] = torch.randn(1, n, generator=gen) * scale
    if c.head_p is not None:
        width = c.head_p + c.dims[-1]
        vals["xe"] = torch.randn(m, c.head_p, generator=gen)
        vals["hw"] = torch.randn(1, width, generator=gen) / width ** 0.5
        vals["hc"] = torch.randn(1, 1, generator=gen)
        vals["out"] = torch.full((m, 1), float("nan"))
    ys = mlp_fwd_ref(vals["x"], [vals[f"w{i}"] for i in range(c.nl)], _biases(c, vals), c.acts)
    for i, y in enumerate(ys):
        vals[f"y{i}"] = y.float()
    v = c.views()
    return {name: (v[name], place(v[name], vals[name])) for name in vals}


def _biases(c, vals):
    return [None if i in c.nobias else vals[f"b{i}"].reshape(-1) for i in range(c.nl)]


def get(ops_, name):
    view, buf = ops_[name]
    return view.of(buf)


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def layer_ref(xin, w, b, act):
    z = xin.double() @ w.double().t()
    if b is not None:
        z = z + b.double()
    return _act(z, act)


def mlp_fwd_ref(x, ws, bs, acts):
    """float64 [y_0, ..., y_last]"""
    ys, h = [], x.double()
    for w, b, a in zip(ws, bs, acts):
        h = layer_ref(h, w, b, a)
        ys.append(h)
    return ys


def head_ref(xe, y_last, hw, hc, p, act):
    w = hw.double().reshape(-1)
    z = y_last.double() @ w[p:] + hc.double().reshape(())
    if p:
        z = z + xe.double() @ w[:p]
    return _act(z, act).reshape(-1, 1)


FWD_MUTATIONS = ("y_tile_from_neighbour", "ragged_row_written", "bias_dropped", "head_no_extra", "head_last_column_dropped")
BWD_MUTATIONS = ("gw_row_dropped", "sigmoid_as_relu", "gb_untouched", "assign_gw", "assign_gb", "gx_ragged_row_written")


def fwd_reference(c, ops_):
    """{"ys": float64 outputs on the original input, "out": the head on them (or None)}"""
    ws = [get(ops_, f"w{i}") for i in range(c.nl)]
    bs = [None if i in c.nobias else get(ops_, f"b{i}").reshape(-1) for i in range(c.nl)]
    ys = mlp_fwd_ref(get(ops_, "x"), ws, bs, c.acts)
    out = None
    if c.head_p is not None:
        out = head_ref(get(ops_, "xe") if c.head_p else None, ys[-1], get(ops_, "hw"), get(ops_, "hc"), c.head_p, c.head_act)
    return {"ys": ys, "out": out}


def check_fwd(c, ops_, got_ys, got_out, want):
    """got_ys: what the call left in the views y_i; want: fwd_reference().  Returns the worst |err| / allowed"""
    worst = 0.0
    for i in range(c.nl):
        xin = get(ops_, "x") if i == 0 else got_ys[i - 1].detach().cpu()
        b = None if i in c.nobias else get(ops_, f"b{i}").reshape(-1)
        local = layer_ref(xin, get(ops_, f"w{i}"), b, c.acts[i])
        worst = max(worst, check_close(got_ys[i], local, what=f"{c.name} y{i} (layer-local)", **FWD_TOL))
    worst = max(worst, check_close(got_ys[-1], want["ys"][-1], what=f"{c.name} last y (end to end)", **Y_TOL))
    if c.head_p is not None:
        local = head_ref(get(ops_, "xe") if c.head_p else None, got_ys[-1].detach().cpu(), get(ops_, "hw"), get(ops_, "hc"),
                         c.head_p, c.head_act)
        worst = max(worst, check_close(got_out, local, what=f"{c.name} head (layer-local)", **HEAD_TOL))
        worst = max(worst, check_close(got_out, want["out"], what=f"{c.name} head (end to end)", **HEAD_TOL))
    return worst


def fwd_mutation_layer(c, mutate):
    """the layer a forward mutation is applied at, or None where it is the identity on this case"""
    if mutate == "y_tile_from_neighbour":
        wide = [i for i, (n, _) in enumerate(c.layers()) if n > 32]
        return wide[-1] if wide else None
    if mutate == "ragged_row_written":
        return c.nl - 1
    if mutate == "bias_dropped":
        with_bias = [i for i in range(c.nl) if i not in c.nobias]
        return with_bias[len(with_bias) // 2]
    if mutate == "head_no_extra":
        return c.nl if c.head_p else None
    if mutate == "head_last_column_dropped":
        return c.nl if c.head_p is not None else None
    raise ValueError(mutate)


def fwd_mutated(c, ops_, want, mutate):
    """(ys, out) as float32, the way a kernel wrong in one small way would leave them; every later layer follows the
    true (unsaved) activations, as the kernel's LDS tiles do"""
    li = fwd_mutation_layer(c, mutate)
    ys = [y.float() for y in want["ys"]]
    out = None if want["out"] is None else want["out"].float()
    if mutate == "y_tile_from_neighbour":          # the last 32-column tile of a layer stored from the tile before it
        n = c.dims[li + 1]
        t0 = 32 * ((n - 1) // 32)
        ys[li][:, t0:n] = ys[li][:, t0 - 32:n - 32]
    elif mutate == "bias_dropped":
        w = get(ops_, f"w{li}")
        xin = get(ops_, "x") if li == 0 else want["ys"][li - 1]
        ys[li] = layer_ref(xin, w, None, c.acts[li]).float()
    elif mutate == "head_no_extra":
        out = head_ref(None, want["ys"][-1], get(ops_, "hw")[:, c.head_p:], get(ops_, "hc"), 0, c.head_act).float()
    elif mutate == "head_last_column_dropped":
        hw = get(ops_, "hw").clone()
        hw[0, -1] = 0.0
        out = head_ref(get(ops_, "xe") if c.head_p else None, want["ys"][-1], hw, get(ops_, "hc"), c.head_p, c.head_act).float()
    return ys, out


def gz_chain(c, ops_, mutate=None):
    """float64 gz_i of every layer, from gy down through the SAVED outputs"""
    g = get(ops_, "gy").double()
    gz = [None] * c.nl
    for i in range(c.nl - 1, -1, -1):
        y = get(ops_, f"y{i}").double()
        if c.acts[i] == S and mutate == "sigmoid_as_relu":
            gz[i] = g * (y > 0)
        else:
            gz[i] = g * _act_grad(y, c.acts[i]) if c.acts[i] != N else g
        g = gz[i] @ get(ops_, f"w{i}").double()
    return gz, g


def bwd_mutation_layer(c, mutate):
    if mutate == "sigmoid_as_relu":
        return c.acts.index(S) if S in c.acts else None
    if mutate == "gx_ragged_row_written":
        return 0 if c.gx else None
    if c.m == 0:
        return None
    return c.nl // 2


def bwd_reference(c, ops_, mutate=None):
    """float64 {"gx": (m, k0) or None, "gw": [...], "gb": [...]} from the starting contents.  ``mutate``: the negative
    controls of tests/test_mlp_ref_cpu.py, applied at bwd_mutation_layer()"""
    gz, g = gz_chain(c, ops_, mutate)
    li = bwd_mutation_layer(c, mutate) if mutate else None
    out = {"gx": g if c.gx else None, "gw": [], "gb": []}
    for i in range(c.nl):
        xin = (get(ops_, "x") if i == 0 else get(ops_, f"y{i - 1}")).double()
        gzi = gz[i]
        if mutate == "gw_row_dropped" and i == li:           # the row that weighs most in this layer's sums
            row = int((gzi.abs().sum(1) * xin.abs().sum(1)).argmax())
            gzi = gzi.clone()
            gzi[row] = 0.0
        sw, sb = gzi.t() @ xin, gzi.sum(0)
        gw0, gb0 = get(ops_, f"gw{i}").double(), get(ops_, f"gb{i}").double().reshape(-1)
        if mutate == "gw_row_dropped":
            sb = gz[i].sum(0)
        out["gw"].append(sw if (mutate == "assign_gw" and i == li) else gw0 + sw)
        if mutate == "gb_untouched" and i == li:
            out["gb"].append(gb0)
        else:
            out["gb"].append(sb if (mutate == "assign_gb" and i == li) else gb0 + sb)
    return out


def check_bwd(c, got, want):
    """got: {"gx", "gw": [...], "gb": [...]} as the call left them.  gw_i / gb_i at the dense layer's gw_tol(m), gx at
    the end-to-end tolerance.  A case whose fp32 gz chain cannot meet gw_tol(m) is not given a wider number here: the
    layer-by-layer ctr_linear_* path (ops.FUSED_MLP = False) is run on the same operands against the same float64 result,
    the fused stack is allowed twice that path's worst error and the measured figure is written beside the case (none
    of today's cases needs it).  Returns the worst |err| / allowed"""
    worst = 0.0
    if c.gx:
        worst = max(worst, check_close(got["gx"], want["gx"], what=f"{c.name} gx (end to end)", **GX_E2E_TOL))
    for i in range(c.nl):
        worst = max(worst, check_close(got["gw"][i], want["gw"][i], what=f"{c.name} gw{i}", **gw_tol(max(1, c.m))))
        worst = max(worst, check_close(got["gb"][i].reshape(-1), want["gb"][i], what=f"{c.name} gb{i}", **gw_tol(max(1, c.m))))
    return worst
