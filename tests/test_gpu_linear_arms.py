"""GPU: every arm of ctr_linear_bwd and the split launches of ctr_linear_fwd (csrc/linear.hip and the kernels it chooses
among) through the C entry points, against the float64 reference of tests/linear_ref.py.

ops.linear_bwd always passes a fresh 16M-float scratch, a contiguous gw and zero-filled gradients; include/ctrhip.h
promises more: any workspace size or none, gw / gb ADDED to, a fixed order of the sums with a workspace.  Each case of
linear_ref.BWD_CASES names the arm it claims and the workspace floats that arm writes (the arithmetic is beside the
case); here every case

* starts from non-zero gw / gb (gx: NaN, or random when accumulated) in buffers whose gaps hold a sentinel,
* gets its workspace as a slice between two sentinel guards: the written floats must end exactly at the table's
  extent (nothing for an atomic arm) and the guards keep the sentinel -- which is how the test knows the arm,
* meets the float64 result within the tolerances of test_linear_backward (tests/test_linear_ref_cpu.py shows that they
  reject small mutations at every case), with the worst |err| / allowed printed,
* is run twice from the same start: gx is bit-identical on every arm, gw and gb on the slab and segment arms.

Measured on an MI355X: every case is below 0.4 of the allowed error except two groups.  The atomic tile arm at 65536
rows reaches 0.4 - 0.6 (64 chunks of 1024 rows; the order of the atomics varies from run to run).  The direct-to-LDS dW
confined to 3 slabs at 4100 rows reaches 0.65 - 0.98 (0.98 at 32 x 96 without gb and without an activation, 0.3 at 161
x 163): each part adds 1376 rows in one fp32 chain.  That arm's order is fixed, so the figure repeats, but it leaves no
margin: a precision limit of ctr_gemm_dlds_dw with few parts, recorded in include/ctrhip.h, not a tolerance to widen."""
import pytest
import torch

import linear_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL, GUARD = ref.SENTINEL, ref.GUARD


@pytest.fixture(scope="module")
def ops():
    from deeplearningrecommendationsystem_amd import ops as o
    return o


def _lib():
    from deeplearningrecommendationsystem_amd import _lib as L
    return L


def _workspace(floats):
    """None, or a sentinel-filled buffer with GUARD floats on either side of the slice the call gets"""
    if floats is None:
        return None
    return torch.full((GUARD + floats + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)


def _check_workspace(c, ws, floats):
    """the written floats end at the table's extent, every float below it was written, the guards are untouched"""
    if ws is None:
        assert c.extent == 0
        print(f"{c.name}: NULL workspace ({c.arm})")
        return
    extent, count = ref.extent_of(ref.written(ws[GUARD:GUARD + floats]))
    print(f"{c.name}: workspace extent observed {extent}, table {c.extent} ({c.arm}), {count} floats written")
    assert bool((ws[:GUARD] == SENTINEL).all()), f"{c.name}: the guard in front of the workspace was written"
    assert bool((ws[GUARD + floats:] == SENTINEL).all()), f"{c.name}: the guard behind the workspace was written"
    assert extent == c.extent, f"{c.name}: {extent} workspace floats written, the {c.arm} arm writes {c.extent}"
    assert count == extent, f"{c.name}: {extent - count} floats below the extent were never written"


def _call_bwd(c, dev, ws, gw=True, gb=True, gx=True, m=None):
    """one ctr_linear_bwd call on the device buffers ``dev``; gw / gb / gx False: that pointer passed as NULL"""
    v = c.views()
    ptr = lambda name: dev[name].data_ptr() + 4 * v[name].off  # noqa: E731
    gy, ldgy = (ptr("x"), v["x"].ld) if c.same_xgy else (ptr("gy"), v["gy"].ld)
    rc = _lib().load().ctr_linear_bwd(
        ptr("x"), v["x"].ld, None if c.no_w else ptr("w"), v["w"].ld,
        ptr("y") if c.act != ref.ACT_NONE else None, v["y"].ld, gy, ldgy,
        ptr("gx") if c.gx and gx else None, v["gx"].ld, int(c.acc),
        ptr("gw") if c.gw and gw else None, v["gw"].ld, ptr("gb") if c.gb and gb else None,
        c.m if m is None else m, c.n, c.k, c.act,
        None if ws is None else ws.data_ptr() + 4 * GUARD, 0 if c.ws is None else c.ws, _lib().stream_ptr())
    torch.cuda.synchronize()
    return rc


def _run_bwd(c, ops_):
    dev = {name: buf.to(DEV) for name, (_, buf) in ops_.items()}
    ws = _workspace(c.ws)
    rc = _call_bwd(c, dev, ws)
    assert rc == ref.CTR_OK, f"{c.name}: ctr_linear_bwd returned {rc}"
    return dev, ws


def _views(c, dev):
    v = c.views()
    return {name: v[name].of(dev[name]) for name in ("gx", "gw", "gb")}


def _check_case(c, ops_, dev, ws):
    want = ref.bwd_reference(c, ops_)
    got = _views(c, dev)
    worst = ref.check_bwd(c, got, want)
    for name in ("gx", "gw", "gb"):                     # gaps of the outputs; outputs not asked for keep their start
        view, start = ops_[name]
        ref.check_gaps(dev[name], view, f"{c.name} {name} buffer")
        if not getattr(c, name):
            assert torch.equal(dev[name].cpu().nan_to_num(nan=1.5), start.nan_to_num(nan=1.5)), f"{c.name}: {name} written"
    for name in ("x", "w", "y", "gy"):
        assert torch.equal(dev[name].cpu(), ops_[name][1]), f"{c.name}: the input {name} was written"
    _check_workspace(c, ws, c.ws)
    return worst


@pytest.mark.parametrize("c", ref.BWD_CASES, ids=lambda c: c.name)
def test_backward_arm(c):
    ops_ = ref.bwd_operands(c)
    dev, ws = _run_bwd(c, ops_)
    worst = _check_case(c, ops_, dev, ws)
    print(f"{c.name}: worst |err| / allowed {worst:.3f}")
    # a second call from the same start
    dev2, _ = _run_bwd(c, ops_)
    a, b = _views(c, dev), _views(c, dev2)
    if c.gx:
        assert torch.equal(a["gx"], b["gx"]), f"{c.name}: gx differs between two calls"
    if c.fixed_order():
        assert torch.equal(a["gw"], b["gw"]), f"{c.name}: gw of the {c.arm} arm differs between two calls"
        if c.gb:
            assert torch.equal(a["gb"], b["gb"]), f"{c.name}: gb of the {c.arm} arm differs between two calls"


@pytest.mark.parametrize("m", [1200, 4100])
@pytest.mark.parametrize("n", [24, 39, 40, 64])
def test_both_halves_of_one_strided_gw(n, m):
    """the NeuralCF form: two calls into the halves [:, :k] and [:, k:] of one (n, 2k) gradient, gb on the second only.
    Each call adds to its half and leaves the other half bit-identical"""
    first, second = ref.bwd_case(f"halves_n{n}_m{m}_first"), ref.bwd_case(f"halves_n{n}_m{m}_second")
    k = first.k
    whole = ref.View(n, 2 * k, 2 * k, 0)
    gen = torch.Generator().manual_seed(n * 7 + m)
    shared = ref.place(whole, torch.randn(n, 2 * k, generator=gen) * m ** 0.5)
    ops_a = ref.bwd_operands(first)
    ops_a["gw"] = (ops_a["gw"][0], shared.clone())
    dev_a, ws_a = _run_bwd(first, ops_a)
    want = ref.bwd_reference(first, ops_a)
    ref.check_bwd(first, _views(first, dev_a), want)
    _check_workspace(first, ws_a, first.ws)
    after_a = dev_a["gw"].cpu()
    assert torch.equal(whole.of(after_a)[:, k:], whole.of(shared)[:, k:]), "the first call wrote the second half"
    ref.check_gaps(after_a, whole, "shared gw buffer after the first call")
    ops_b = ref.bwd_operands(second)
    ops_b["gw"] = (ops_b["gw"][0], after_a.clone())
    dev_b, ws_b = _run_bwd(second, ops_b)
    want = ref.bwd_reference(second, ops_b)
    ref.check_bwd(second, _views(second, dev_b), want)
    _check_workspace(second, ws_b, second.ws)
    after_b = dev_b["gw"].cpu()
    assert torch.equal(whole.of(after_b)[:, :k], whole.of(after_a)[:, :k]), "the second call wrote the first half"
    ref.check_gaps(after_b, whole, "shared gw buffer after the second call")


@pytest.mark.parametrize("name", ["tile_swapped", "tile_m1024_8_chunks"])
def test_profiling_split_issues_dx_and_dw_as_two_calls(ops, name):
    """with a KernelProfiler installed ops.linear_bwd issues dX and dW separately: bit-identical to the single call on
    a slab arm, within tolerance on an atomic arm (the wrapper's 16M-float scratch leaves both shapes on their arm:
    10 chunks > 8 -> slabs, 8 chunks -> atomics)"""
    c = ref.bwd_case(name)
    ops_ = ref.bwd_operands(c)
    v = c.views()
    t = {nm: v[nm].of(buf).clone() for nm, (_, buf) in ops_.items()}
    want = ref.bwd_reference(c, ops_)

    def run():
        d = {nm: val.to(DEV) for nm, val in t.items()}
        ops.linear_bwd(d["x"], d["w"], d["y"], d["gy"], c.act, d["gx"], d["gw"], d["gb"].reshape(-1))
        torch.cuda.synchronize()
        return d

    single = run()
    prof = ops.KernelProfiler()
    ops.set_profiler(prof)
    try:
        split = run()
    finally:
        ops.set_profiler(None)
    labels = sorted(r[0] for r in prof.records)
    assert labels == sorted(f"linear_bwd_{p}[{c.m}x{c.n}x{c.k}]" for p in ("dx", "dw")), labels
    for d, what in ((single, "single call"), (split, "split calls")):
        print(what)
        ref.check_bwd(c, d, want)
    assert torch.equal(single["gx"], split["gx"])
    if c.fixed_order():
        assert torch.equal(single["gw"], split["gw"]) and torch.equal(single["gb"], split["gb"])


@pytest.mark.parametrize("name", ["tile_m1025_9_chunks", "n1_slabs"])
def test_gb_without_gw_is_refused_before_anything_is_written(name):
    """on a tile shape (dX would be enqueued first) and on a single-unit shape (whose kernel could form gb alone: the
    header's "needs gw" holds for every shape)"""
    c = ref.bwd_case(name)
    ops_ = ref.bwd_operands(c)
    dev = {name: buf.to(DEV) for name, (_, buf) in ops_.items()}
    ws = _workspace(c.ws)
    assert _call_bwd(c, dev, ws, gw=False) == ref.CTR_EINVAL
    for name, (_, buf) in ops_.items():
        assert torch.equal(dev[name].cpu().nan_to_num(nan=1.5), buf.nan_to_num(nan=1.5)), f"{name} was written"
    assert bool((ws == SENTINEL).all())


def test_an_empty_batch_is_ok_and_writes_nothing():
    c = ref.bwd_case("tile_m1025_9_chunks")
    ops_ = ref.bwd_operands(c)
    dev = {name: buf.to(DEV) for name, (_, buf) in ops_.items()}
    ws = _workspace(c.ws)
    assert _call_bwd(c, dev, ws, m=0) == ref.CTR_OK
    for name, (_, buf) in ops_.items():
        assert torch.equal(dev[name].cpu().nan_to_num(nan=1.5), buf.nan_to_num(nan=1.5)), f"{name} was written"
    assert bool((ws == SENTINEL).all())


@pytest.mark.parametrize("c", ref.FWD_CASES, ids=lambda c: c.name)
def test_forward_split_launches_and_tile_kernel(c):
    """residual, bias and a strided y (ldy = n + 3) whose gaps keep the sentinel"""
    x, w, b, r, yv, ybuf = ref.fwd_operands(c)
    xd, wd, bd, rd, yd = (t.to(DEV) for t in (x, w, b, r, ybuf))
    rc = _lib().load().ctr_linear_fwd(xd.data_ptr(), c.k, wd.data_ptr(), c.k, bd.data_ptr(), rd.data_ptr(), c.n,
                                      yd.data_ptr(), yv.ld, c.m, c.n, c.k, c.act, _lib().stream_ptr())
    torch.cuda.synchronize()
    assert rc == ref.CTR_OK
    worst = ref.check_fwd(c, yv.of(yd), ref.linear_fwd_ref(x, w, b, r, c.act))
    ref.check_gaps(yd, yv, f"{c.name} y buffer")
    print(f"{c.name} ({c.arm}): worst |err| / allowed {worst:.3f}")
