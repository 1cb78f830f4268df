"""What every wrapper of the C ABI (include/ctrhip.h) is built from: the call frame, the profiler it reads (the one
profiler state of the package), the operand checks the kernel families share and the backward launches' scratch."""
from typing import Optional

import torch

from .. import _lib


# ---------------------------------------------------------------------------
# optional per-launch timing (bench.py): a HIP event pair on the stream the
# kernel is enqueued on, plus the launch's algorithmic bytes / flops
# ---------------------------------------------------------------------------
class KernelProfiler:
    """HIP-event timing of every C-ABI call of the steps run while it is installed.

    ``spacer_us`` > 0 keeps the GPU busy for about that long (``torch.cuda._sleep``) before each bracketed call: start
    event, launch and end event are then all queued before the GPU reaches them, so the pair measures the kernel(s) of
    the call and not the host's launch latency (without it a 70 us kernel reads ~85 us; with it the numbers agree with
    rocprofv3 to a few per cent)."""

    def __init__(self, spacer_us: float = 0.0):
        self.records = []
        self.spacer_cycles = 0
        if spacer_us > 0:
            # calibrate _sleep: cycles per microsecond of whatever clock it spins on
            probe = 200_000
            torch.cuda._sleep(probe)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(probe)
            b.record()
            torch.cuda.synchronize()
            us = max(a.elapsed_time(b) * 1e3, 1e-3)
            self.spacer_cycles = max(1, int(probe / us * spacer_us))

    def add(self, label, nbytes, flops, start, end):
        self.records.append((label, nbytes, flops, start, end))

    def summary(self):
        """{label: dict(calls, total_us, avg_us, bytes, flops)} -- call after a sync.  ``bytes`` / ``flops`` are the
        AVERAGE per call of what the calls under that label declared, ``avg_us`` the average duration: a label that
        covers launches of different shapes (two stacks through ``mlp_fused_fwd``) then still gives a physically
        possible rate, total work over total time (round 2 divided the first call's work by the average time of
        all calls and printed a fraction above 1).  ``shapes`` counts the distinct (bytes, flops) pairs seen."""
        torch.cuda.synchronize()
        return self.fold([(label, nbytes, flops, start.elapsed_time(end) * 1e3)
                          for label, nbytes, flops, start, end in self.records])

    @staticmethod
    def fold(timed):
        """``summary`` over (label, bytes, flops, microseconds) records"""
        out = {}
        for label, nbytes, flops, us in timed:
            d = out.setdefault(label, dict(calls=0, total_us=0.0, total_bytes=0, total_flops=0, _shapes=set()))
            d["calls"] += 1
            d["total_us"] += us
            d["total_bytes"] += nbytes
            d["total_flops"] += flops
            d["_shapes"].add((nbytes, flops))
        for d in out.values():
            d["avg_us"] = d["total_us"] / d["calls"]
            d["bytes"] = d["total_bytes"] / d["calls"]
            d["flops"] = d["total_flops"] / d["calls"]
            d["shapes"] = len(d.pop("_shapes"))
        return out


_profiler: Optional[KernelProfiler] = None


def set_profiler(p: Optional[KernelProfiler]) -> None:
    global _profiler
    _profiler = p


def _timed(label, meta, fn, *args):
    """run one C call; when a profiler is installed bracket it with events"""
    p = _profiler
    if p is None:
        return fn(*args)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if p.spacer_cycles:
        torch.cuda._sleep(p.spacer_cycles)
    start.record()
    rc = fn(*args)
    end.record()
    nbytes, flops = meta()
    p.add(label, nbytes, flops, start, end)
    return rc


def _call(label, symbol, meta, *args):
    """``symbol`` of the loaded library under ``_timed``, its return code checked: for a wrapper that only checks it"""
    _lib.check(_timed(label, meta, getattr(_lib.load(), symbol), *args), symbol)


def _profiling() -> bool:
    """whether a profiler is installed: a wrapper whose C call covers several launches then issues them one by one"""
    return _profiler is not None


_REFUSED = (_lib.CTR_ELIMIT, _lib.CTR_EALIGN)  # nothing was enqueued, the caller takes its other path


def _refused(rc, label) -> bool:
    """whether the library refused the ``_timed`` call that returned ``rc``; nothing ran then, so the profiler's record
    of it goes and what the caller issues instead is what gets timed"""
    if rc not in _REFUSED:
        return False
    if _profiler is not None and _profiler.records and _profiler.records[-1][0] == label:
        _profiler.records.pop()
    return True


SCRATCH_FLOATS = 16 * 1024 * 1024  # 64 MiB: per-workgroup partials of the weight-gradient reductions


def _scratch(device) -> torch.Tensor:
    """device scratch for one backward launch.  Taken from torch's caching allocator per call (a few microseconds,
    no hipMalloc in steady state), so it follows the usual stream-ordered lifetime rules, not shared global state."""
    return torch.empty(SCRATCH_FLOATS, dtype=torch.float32, device=device)


def _mat(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{what}: expected a 2-D float32 tensor with unit inner stride, got "
                         f"{tuple(t.shape)} {t.dtype} strides {t.stride()}")
    _lib.require_device(t)
    return t


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))


def _i64(*tensors):
    _lib.require_device(*tensors)
    for t in tensors:
        if t is not None and (t.dtype != torch.int64 or not t.is_contiguous()):
            raise ValueError("expected contiguous int64 tensors")


def _f32_vectors(name, what, *tensors):
    """``tensors`` flattened and contiguous on the device, float32 or ``name: what must be float32``"""
    vecs = [t.detach().reshape(-1).contiguous() for t in tensors]
    _lib.require_device(*vecs)
    if any(t.dtype != torch.float32 for t in vecs):
        raise ValueError(f"{name}: {what} must be float32")
    return vecs


def _flat_f32(name, what, t, n=None):
    if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or (n is not None and t.shape[0] != n):
        raise ValueError(f"{name}: {what} must be a contiguous (N,) float32 tensor")


def _flat_int(name, what, t, dtype, n):
    if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or t.shape[0] != n:
        raise ValueError(f"{name}: {what} must be a contiguous ({n},) {str(dtype).replace('torch.', '')} tensor")
