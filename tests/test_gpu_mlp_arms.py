"""GPU: every arm of the fused MLP stack (csrc/mlp_fused.hip: ctr_mlp_fwd, ctr_mlp_head_fwd, ctr_mlp_bwd) through the C
entry points, against the float64 reference of tests/mlp_ref.py.

ops.mlp_fwd / ops.mlp_bwd admit m >= 1024 with a bias on every layer, allocate contiguous outputs, start gw / gb at zero,
always ask for gx and pass a 16M-float scratch; include/ctrhip.h promises more.  Each case of mlp_ref names the arm it
is here for (tests/test_mlp_ref_cpu.py holds the names against plan() and shows that no arm is without a case); here
every case

* is one call with every operand a view into a sentinel-filled buffer: the gaps, the row behind a ragged last tile, the
  inputs and the outputs not asked for (gx == NULL) stay bit-identical;
* meets both comparisons of mlp_ref (layer-local at the dense layer's tolerances, end to end at those of
  tests/test_gpu_ops.py), the worst |err| / allowed printed;
* starts gw / gb at non-zero contents of the gradient's own magnitude;
* gets its workspace as a slice between two sentinel guards: the written floats end exactly at plan()'s grid * slab and
  every float below was written -- which is what ties plan() to the C code (the slab, the grid cap of 256, and
  DienAttShape's 512);
* is run twice from the same start: y, out, gx, gw and gb are bit-identical (the partials are merged in a fixed order).

Every refusal returns the code mlp_ref.REFUSALS gives and leaves every buffer and the workspace at the sentinel.

Claimed by arithmetic only (plan()), not observable from outside: MAXT, the flush's copies, gvec, the LDS strides, the
straddling slot pairs and remainder chunks, and that NcfShape / NcfTowerShape were matched.

Measured on an MI355X, worst |err| / allowed over all cases: y_i layer-local 0.28 (NcfTowerShape at 65573 rows, layer 0;
below 0.16 elsewhere), last y end to end 0.08, head 0.10, gx 0.04, gw_i 0.43 and gb_i 0.26 (NcfShape at 1029 rows, the
same figures whichever way gY is fetched; below 0.15 on every DynShape case).  No case needs the rule for a long gz
chain in mlp_ref.check_bwd.  Workspace extents observed, all equal to plan(): A 1 x 2941 and 256 x 2941 at 32805 rows, B
4062, C 654, D 2 x 9352, E 4 x 11400, NcfTowerShape 11000 and 256 x 11000 at 65573 rows, DienAttShape 4225 and 512 x 4225
at 65573 rows, NcfShape 9 x 11576, J 33 x 9008 and 12 x 9753.  Every output was bit-identical between two runs.  The
forward at an LDS row pitch of 136 bytes (C_stride34: the odd last width is the widest tenant of its tile, so float4
accesses of the other layers are 8-byte aligned) is as accurate as any other case: gfx950 serves them, and build()
keeps the forward widths unrounded."""
import ctypes as C

import pytest
import torch

import mlp_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL, GUARD = ref.SENTINEL, ref.GUARD


def _lib():
    from deeplearningrecommendationsystem_amd import _lib as L
    return L


def _same(a, b):
    return torch.equal(a.cpu().nan_to_num(nan=1.5), b.cpu().nan_to_num(nan=1.5))


class Call:
    """the device buffers of one case and the three entry points on them"""

    def __init__(self, c, ops_, forward):
        self.c, self.ops_, self.v = c, ops_, c.views()
        self.dev = {name: buf.to(DEV) for name, (_, buf) in ops_.items()}
        if forward:                                          # the outputs start as NaN, not as the saved values
            for i in range(c.nl):
                self.dev[f"y{i}"] = ref.blank(self.v[f"y{i}"]).to(DEV)
        self.start = {name: t.cpu() for name, t in self.dev.items()}
        self.ws = None

    def ptr(self, name):
        return self.dev[name].data_ptr() + 4 * self.v[name].off

    def view(self, name):
        return self.v[name].of(self.dev[name])

    def layers(self, grads):
        c = self.c
        arr = (_lib().MlpLayer * c.nl)()
        for i, (n, k) in enumerate(c.layers()):
            e = arr[i]
            e.w, e.b = self.ptr(f"w{i}"), None if i in c.nobias else self.ptr(f"b{i}")
            e.y, e.ldy = self.ptr(f"y{i}"), self.v[f"y{i}"].ld
            e.n, e.k, e.act = n, k, c.acts[i]
            if grads:
                e.gw, e.gb = self.ptr(f"gw{i}"), self.ptr(f"gb{i}")
        return arr

    def fwd(self, m=None):
        c, lib = self.c, _lib().load()
        m = c.m if m is None else m
        if c.head_p is None:
            rc = lib.ctr_mlp_fwd(self.ptr("x"), self.v["x"].ld, m, self.layers(False), c.nl, _lib().stream_ptr())
        else:
            hd = _lib().MlpHead(self.ptr("xe") if c.head_p else None, self.v["xe"].ld if c.head_p else 0, self.ptr("hw"),
                                self.ptr("hc"), self.ptr("out"), c.ldout, c.head_p, c.head_act)
            rc = lib.ctr_mlp_head_fwd(self.ptr("x"), self.v["x"].ld, m, self.layers(False), c.nl, C.byref(hd),
                                      _lib().stream_ptr())
        torch.cuda.synchronize()
        return rc

    def bwd(self, ws_floats, m=None):
        c = self.c
        self.ws = torch.full((GUARD + ws_floats + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        rc = _lib().load().ctr_mlp_bwd(self.ptr("x"), self.v["x"].ld, c.m if m is None else m, self.layers(True), c.nl,
                                       self.ptr("gy"), self.v["gy"].ld, self.ptr("gx") if c.gx else None, self.v["gx"].ld,
                                       self.ws.data_ptr() + 4 * GUARD, ws_floats, _lib().stream_ptr())
        torch.cuda.synchronize()
        return rc

    def unchanged(self, names):
        for name in names:
            assert _same(self.dev[name], self.start[name]), f"{self.c.name}: {name} was written"

    def gaps(self, names):
        for name in names:
            ref.check_gaps(self.dev[name], self.v[name], f"{self.c.name} {name} buffer")


def _inputs(c, backward):
    names = ["x"] + [f"w{i}" for i in range(c.nl)] + [f"b{i}" for i in range(c.nl)]
    if backward:
        names += ["gy"] + [f"y{i}" for i in range(c.nl)]
    if c.head_p is not None:
        names += ["xe", "hw", "hc"]
    return names


@pytest.mark.parametrize("c", ref.FWD_CASES + ref.HEAD_CASES, ids=lambda c: c.name)
def test_forward_arm(c):
    ops_ = ref.operands(c)
    want = ref.fwd_reference(c, ops_)
    call = Call(c, ops_, True)
    assert call.fwd() == ref.CTR_OK
    ys = [call.view(f"y{i}") for i in range(c.nl)]
    out = call.view("out") if c.head_p is not None else None
    worst = ref.check_fwd(c, ops_, ys, out, want)
    print(f"{c.name}: forward worst |err| / allowed {worst:.3f}")
    call.gaps([f"y{i}" for i in range(c.nl)] + (["out"] if c.head_p is not None else []))
    call.unchanged(_inputs(c, False) + ["gx"] + [f"g{t}{i}" for t in "wb" for i in range(c.nl)])
    again = Call(c, ops_, True)
    assert again.fwd() == ref.CTR_OK
    for name in [f"y{i}" for i in range(c.nl)] + (["out"] if c.head_p is not None else []):
        assert torch.equal(call.dev[name], again.dev[name]), f"{c.name}: {name} differs between two calls"


@pytest.mark.parametrize("c", ref.BWD_CASES, ids=lambda c: c.name)
def test_backward_arm(c):
    ops_ = ref.operands(c)
    want = ref.bwd_reference(c, ops_)
    p = c.plan(True)
    floats = p.extent + c.ws_room                            # ws_room == 0: the workspace ends with the last slab

    def run():
        call = Call(c, ops_, False)
        assert call.bwd(floats) == ref.CTR_OK
        return call
    call = run()
    got = {"gx": call.view("gx") if c.gx else None, "gw": [call.view(f"gw{i}") for i in range(c.nl)],
           "gb": [call.view(f"gb{i}") for i in range(c.nl)]}
    worst = ref.check_bwd(c, got, want)
    print(f"{c.name}: backward worst |err| / allowed {worst:.3f}")
    call.gaps(["gx"] + [f"g{t}{i}" for t in "wb" for i in range(c.nl)])
    call.unchanged(_inputs(c, True) + ([] if c.gx else ["gx"]))
    extent, count = ref.extent_of(ref.written(call.ws[GUARD:GUARD + floats]))
    print(f"{c.name}: workspace extent observed {extent}, plan {p.grid} x {p.slab} = {p.extent}, {count} floats written")
    assert bool((call.ws[:GUARD] == SENTINEL).all()), f"{c.name}: the guard in front of the workspace was written"
    assert bool((call.ws[GUARD + floats:] == SENTINEL).all()), f"{c.name}: the guard behind the workspace was written"
    assert extent == p.extent, f"{c.name}: {extent} workspace floats written, plan() says {p.grid} x {p.slab}"
    assert count == extent, f"{c.name}: {extent - count} floats below the extent were never written"
    again = run()
    for name in ["gx"] + [f"g{t}{i}" for t in "wb" for i in range(c.nl)]:
        assert _same(call.dev[name], again.dev[name]), f"{c.name}: {name} differs between two calls"


def test_an_empty_batch_is_ok_and_writes_nothing():
    c = next(x for x in ref.STACK_CASES if x.name == "A_m37")
    ops_ = ref.operands(c)
    for forward in (True, False):
        call = Call(c, ops_, forward)
        assert (call.fwd(m=0) if forward else call.bwd(1000, m=0)) == ref.CTR_OK
        call.unchanged(list(call.dev))
        assert forward or bool((call.ws == SENTINEL).all())


def _buffers(r):
    """sentinel-filled device buffers of a refusal, each with room for its widest reading"""
    ns, ks = r.dims[1:], r.ks or r.dims[:-1]
    full = lambda count: torch.full((count + 64,), SENTINEL, dtype=torch.float32, device=DEV)  # noqa: E731
    b = {"x": full(r.m * (ks[0] + 8)), "gx": full(r.m * (ks[0] + 8)), "gy": full(r.m * (ns[-1] + 8))}
    for i, (n, k) in enumerate(zip(ns, ks)):
        b[f"w{i}"], b[f"gw{i}"], b[f"b{i}"], b[f"gb{i}"] = full(n * k), full(n * k), full(n), full(n)
        b[f"y{i}"] = full(r.m * (n + 8))
    if r.head_p is not None:
        b["xe"], b["hw"], b["hc"], b["out"] = full(r.m * (r.head_p + 8)), full(r.head_p + ns[-1]), full(1), full(r.m)
    return b


@pytest.mark.parametrize("r", ref.REFUSALS, ids=lambda r: r.name)
def test_refusal_returns_its_code_and_enqueues_nothing(r):
    lib, L = _lib().load(), _lib()
    ns, ks = r.dims[1:], r.ks or r.dims[:-1]
    b = _buffers(r)
    nl = len(ns)
    arr = (L.MlpLayer * nl)()
    for i, (n, k) in enumerate(zip(ns, ks)):
        e = arr[i]
        e.w, e.b, e.y, e.ldy = b[f"w{i}"].data_ptr(), b[f"b{i}"].data_ptr(), b[f"y{i}"].data_ptr(), n + (4 if i < nl - 1 else 0)
        e.n, e.k, e.act = n, k, r.acts()[i]
        e.gw, e.gb = b[f"gw{i}"].data_ptr(), b[f"gb{i}"].data_ptr()
    if r.tweak == "mid_off1":
        arr[0].y += 4
    if r.tweak == "no_gb":
        arr[0].gb = None
    x = b["x"].data_ptr() + (4 if r.tweak == "x_off1" else 0)
    ldx = ks[0] + (1 if r.tweak == "ldx_odd" else 0)
    ws = None
    if r.entry == "fwd":
        rc = lib.ctr_mlp_fwd(x, ldx, r.m, arr, nl, L.stream_ptr())
    elif r.entry == "head":
        hd = L.MlpHead(b["xe"].data_ptr(), r.head_p + (1 if r.tweak == "head_ldx_odd" else 0), b["hw"].data_ptr(),
                       b["hc"].data_ptr(), b["out"].data_ptr(), 1, r.head_p, ref.S)
        rc = lib.ctr_mlp_head_fwd(x, ldx, r.m, arr, nl, C.byref(hd), L.stream_ptr())
    else:
        floats = 1 << 20
        if r.tweak == "ws_short":
            floats = ref.plan(r.dims, r.acts(), True, r.m).extent - 1
        ws = torch.full((GUARD + floats + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        rc = lib.ctr_mlp_bwd(x, ldx, r.m, arr, nl, b["gy"].data_ptr(), ns[-1], b["gx"].data_ptr(), ks[0],
                             ws.data_ptr() + 4 * GUARD, floats, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == r.code == r.plan().code, f"{r.name}: returned {rc}"
    for name, t in b.items():
        assert bool((t == SENTINEL).all()), f"{r.name}: {name} was written"
    assert ws is None or bool((ws == SENTINEL).all()), f"{r.name}: the workspace was written"


def test_forward_fused_backward_refused_through_ops():
    """case F: 18 accumulator tiles.  ops.mlp_fwd runs the stack as one launch, ctr_mlp_bwd refuses it and ops.mlp_bwd
    goes layer by layer on the activations the fused forward saved: equal to float64 and to FUSED_MLP = False"""
    from deeplearningrecommendationsystem_amd import ops
    dims, acts_, m = ref.F_DIMS, ref.F_ACTS, ref.F_M
    g = torch.Generator().manual_seed(m)
    x = torch.randn(m, dims[0], generator=g)
    ws = [torch.randn(n, k, generator=g) / k ** 0.5 for k, n in zip(dims[:-1], dims[1:])]
    bs = [torch.randn(n, generator=g) for n in dims[1:]]
    gy = torch.randn(m, dims[-1], generator=g)

    def run(fused, profiler=None):
        ops.FUSED_MLP = fused
        ops.set_profiler(profiler)
        try:
            layers = [ops.Layer(w.to(DEV), b.to(DEV), a) for w, b, a in zip(ws, bs, acts_)]
            acts = ops.mlp_fwd(x.to(DEV), layers)
            grads, gx = ops.mlp_bwd(acts, layers, gy.to(DEV), None)
            torch.cuda.synchronize()
        finally:
            ops.FUSED_MLP = True
            ops.set_profiler(None)
        return acts, grads, gx
    acts_f, grads_f, gx_f = run(True)
    acts_l, grads_l, gx_l = run(False)
    prof = ops.KernelProfiler()
    run(True, prof)
    labels = [rec[0] for rec in prof.records]
    print(labels)
    assert any(lb.startswith("mlp_fused_fwd") for lb in labels) and not any(lb.startswith("mlp_fused_bwd") for lb in labels)
    assert sum(lb.startswith("linear_bwd") for lb in labels) >= len(ws)

    c = ref.Case("F", dims, acts_, m, "")
    want_ys = ref.mlp_fwd_ref(x, ws, bs, acts_)
    ref.check_close(acts_f[-1], want_ys[-1], what="F last y, fused", **ref.Y_TOL)
    ref.check_close(acts_l[-1], want_ys[-1], what="F last y, layer by layer", **ref.Y_TOL)
    for what, saved, grads, gx in (("fused forward", acts_f, grads_f, gx_f), ("layer by layer", acts_l, grads_l, gx_l)):
        ops_ = {"gy": (ref.View(m, dims[-1], dims[-1], 0), gy.reshape(-1))}
        for i, (n, k) in enumerate(c.layers()):
            ops_[f"y{i}"] = (ref.View(m, n, n, 0), saved[i + 1].cpu().reshape(-1))
            ops_[f"w{i}"] = (ref.View(n, k, k, 0), ws[i].reshape(-1))
            ops_[f"gw{i}"], ops_[f"gb{i}"] = (ref.View(n, k, k, 0), torch.zeros(n * k)), (ref.View(1, n, n, 0), torch.zeros(n))
        ops_["x"] = (ref.View(m, dims[0], dims[0], 0), x.reshape(-1))
        print(what)
        ref.check_bwd(c, {"gx": gx, "gw": [gw for gw, _ in grads], "gb": [gb for _, gb in grads]}, ref.bwd_reference(c, ops_))
    # the two paths against each other: the outputs directly; the gradients meet through float64 above, each path's
    # masks taken from its own saved outputs (a relu unit within rounding of zero may differ between the two forwards)
    ref.check_close(acts_f[-1], acts_l[-1], what="F last y, fused against layer by layer", **ref.Y_TOL)
