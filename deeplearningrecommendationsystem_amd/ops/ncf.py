"""NeuralCF's table-row path (csrc/ncf_proj.hip, rows_sum.hip) and matrix factorisation's dot (csrc/mf.hip)."""
import ctypes as C
from typing import Optional

import torch

from .. import _lib
from .._lib import ACT_SIGMOID
from ._call import _REFUSED, SCRATCH_FLOATS, _call, _ld, _mat, _profiling, _scratch, _timed


# ---------------------------------------------------------------------------
# NeuralCF with the first tower layer on the table rows (csrc/ncf_proj.hip)
# ---------------------------------------------------------------------------
def few_table_rows(rows: int, batch: int) -> bool:
    """the admission both of NeuralCF's table-row paths share: a batch worth a launch over the tables' ``rows`` (both
    tables together), with every row met by four samples on average"""
    return batch >= 4096 and batch >= 4 * rows


class NcfCounts:
    """the bucket plan of ``ctr_ncf_proj_fwd`` (one holder per model): per-row sample counts of the batch's chunks,
    row totals, bucket offsets and block totals, built by every training forward and read by its backward.  The
    kernels write every entry they read later and never touch the buffer's first word (it stays the zero written
    here), so in the usual forward -> backward rhythm the buffer is filled once, here.  ``take`` hands it out when no
    forward owns it; while a forward's plan still waits for its
    backward (two graphs alive at once) a later forward gets a freshly zeroed buffer of its own instead, and after a
    training forward that never got its backward the buffer is cleared before it is handed out again."""

    def __init__(self):
        self.buf, self.state = None, "clean"

    def take(self, rows: int, device):
        n = rows * _lib.CTR_NCF_PROJ_COUNT_STRIDE      # chunk counts, total and offset per row (ctrhip.h)
        if self.buf is None or self.buf.numel() < n or self.buf.device != device:
            self.buf, self.state = torch.zeros(n, dtype=torch.int32, device=device), "clean"
        if self.state == "dirty":            # a training forward whose graph was dropped without a backward
            self.buf.zero_()
            self.state = "clean"
        if self.state == "clean":
            self.state = "busy"
            return self.buf, True
        return torch.zeros(n, dtype=torch.int32, device=device), False


class NcfProj:
    """one forward of ``ctr_ncf_proj_fwd`` and what its backward needs.  ``tables`` = (gmf_u, gmf_i, mlp_u, mlp_i),
    ``hidden`` = the four tower layers, ``proj`` = (w, b) of ``linear``, ``head`` = (w, b) of ``linear2``."""

    def __init__(self, user_idx, item_idx, tables, hidden, proj, head, err_flag, training, counts: "NcfCounts" = None):
        self.user_idx, self.item_idx = user_idx, item_idx
        self.tables, self.hidden, self.proj, self.head = tables, hidden, proj, head
        gmf_u, gmf_i, mlp_u, mlp_i = tables
        dev = gmf_u.device
        self.batch, self.nu, self.ni = user_idx.numel(), gmf_u.shape[0], gmf_i.shape[0]
        m, rows = self.batch, self.nu + self.ni
        self.ptab = torch.empty((rows, hidden[0].weight.shape[0]), dtype=torch.float32, device=dev)
        self.wfold = torch.empty(76, dtype=torch.float32, device=dev)
        # every per-sample buffer has a spare row m: lanes without a sample store there (unconditional, countable stores)
        self.ys = [torch.empty((m + 1, layer.weight.shape[0]), dtype=torch.float32, device=dev) for layer in hidden[1:]]
        self.prob_buf = torch.empty((m + 1, 1), dtype=torch.float32, device=dev)
        self.prob = self.prob_buf[:m]
        self._holder, self._owns = None, False
        self.plan = self.ranks = None
        if training:
            self._holder = counts if counts is not None else NcfCounts()
            self.plan, self._owns = self._holder.take(rows, dev)
            self.ranks = torch.empty(2 * (m + 1), dtype=torch.int32, device=dev)
        self.err_flag, self.training = err_flag, training

    def __del__(self):
        # a training forward that never saw its backward: the holder clears the plan before it hands it out again
        if getattr(self, "_owns", False) and self._holder.state == "busy":
            self._holder.state = "dirty"

    def _desc(self):
        gmf_u, gmf_i, mlp_u, mlp_i = self.tables
        d = _lib.NcfProj()
        d.user_idx, d.user_stride = self.user_idx.data_ptr(), self.user_idx.stride(0) if self.user_idx.numel() > 1 else 1
        d.item_idx, d.item_stride = self.item_idx.data_ptr(), self.item_idx.stride(0) if self.item_idx.numel() > 1 else 1
        d.batch, d.num_users, d.num_items = self.batch, self.nu, self.ni
        d.mlp_user, d.mlp_item, d.gmf_user, d.gmf_item = (t.data_ptr() for t in (mlp_u, mlp_i, gmf_u, gmf_i))
        d.mlp_dim, d.mf_dim = mlp_u.shape[1], gmf_u.shape[1]
        for k, layer in enumerate(self.hidden):
            e = d.layers[k]
            e.w, e.b, e.n, e.k, e.act = layer.weight.data_ptr(), _lib.ptr(layer.bias), layer.weight.shape[0], layer.weight.shape[1], layer.act
            if k:
                e.y, e.ldy = self.ys[k - 1].data_ptr(), _ld(self.ys[k - 1])
        pw, pb = self.proj
        hw, hb = self.head
        d.proj_w, d.ld_proj_w, d.proj_b, d.proj_n, d.proj_k = pw.data_ptr(), _ld(pw), _lib.ptr(pb), pw.shape[0], pw.shape[1]
        d.head_w, d.head_b, d.head_act = hw.data_ptr(), _lib.ptr(hb), ACT_SIGMOID
        d.prob, d.ldprob, d.err_flag = self.prob.data_ptr(), 1, _lib.ptr(self.err_flag)
        d.ptab, d.wfold, d.plan, d.ranks = self.ptab.data_ptr(), self.wfold.data_ptr(), _lib.ptr(self.plan), _lib.ptr(self.ranks)
        d.training = 1 if self.training else 0
        return d

    def bucket_offsets(self) -> torch.Tensor:
        """(rows + 1) int32 of the training forward's plan: row v's bucket is the slots [o[v], o[v + 1]), user rows first
        (the plan's layout, csrc/ncf_proj.hip: 4 int32 of head, 64 chunks x rows bases, rows totals, the offsets, then
        the block totals)"""
        rows = self.nu + self.ni
        return self.plan[4 + 65 * rows: 4 + 66 * rows + 1]

    @staticmethod
    def supported(tables, hidden, proj, batch) -> bool:
        gmf_u, gmf_i, mlp_u, mlp_i = tables
        rows = gmf_u.shape[0] + gmf_i.shape[0]
        dims = [tuple(layer.weight.shape) for layer in hidden]
        return (dims == [(64, 128), (32, 64), (16, 32), (8, 16)] and gmf_u.shape[1] == 64 and mlp_u.shape[1] == 64 and
                tuple(proj[0].shape) == (64, 8) and all(layer.bias is not None for layer in hidden) and
                rows <= _lib.CTR_NCF_PROJ_MAX_ROWS and few_table_rows(rows, batch) and 2 * batch < 2 ** 31)

    # algorithmic bytes / flops of the launches: per sample unless said otherwise
    def _meta(self, which):
        m, rows = self.batch, self.nu + self.ni
        tower = 64 * 32 + 32 * 16 + 16 * 8
        shift = 8                            # the plan's chunks of the batch (csrc/ncf_proj.hip, plan_of)
        while (64 << shift) < m:
            shift += 1
        chunks = -(-m // (1 << shift))
        blocks = -(-rows // 256)             # the rows of one plan workgroup; block totals only for more than one
        blk = chunks * blocks * 4 if blocks > 1 else 0
        return {
            # (rows, 64) tables read, (rows, 64) projected rows written; one 64 x 64 product per row
            # (+ in training, by the rank workgroups of the same launch: ids, an 8-byte rank record per sample, a
            # histogram of the rows per chunk and its sums over the blocks)
            "ncfp_prep": lambda: (rows * 512 + ((m * (16 + 8) + chunks * rows * 4 + blk) if self.training else 0),
                                  2 * rows * 64 * 64),
            # ids, four 256-byte rows (cache-resident tables), saved activations + prob written; tower + head
            # (+ in training, by the plan workgroups of the same launch: the histograms read and written back as
            # absolute bases, row totals and bucket offsets written, and plan workgroup k reads the block totals of
            # the k blocks in front of it)
            "ncfp_fwd": lambda: (m * (16 + 4 * 256 + 4 * (32 + 16 + 8) + 4) +
                                 ((2 * chunks * rows * 4 + 2 * rows * 4 + blk * (blocks - 1) // 2) if self.training else 0),
                                 2 * m * (tower + 72 + 64)),
            # ids, prob, gprob, ranks, two absolute bases (slot = base + rank: no copy of the offsets), two projected
            # rows, saved activations read; gz0 row stored once + two records
            "ncfp_bwd": lambda: (m * (16 + 16 + 8 + 2 * 256 + 4 * (32 + 16 + 8) + 256 + 32), 4 * m * tower + 2 * m * 8),
            # per slot: its record, the gz0 row and the partner row the record names read; (rows, 128) sums added
            # (the slab reduction and the head fold left this launch: they ride with ncfp_finish, phase 4)
            "ncfp_segsum": lambda: (2 * m * (256 + 16 + 256) + rows * 512, 2 * 2 * m * 64 * 2),
            # sums + tables read, table gradients read-modify-written; three 64 x 64 products per row
            # (+ on workgroups of their own: ncfp_bwd's slabs summed into the tower gradients, the head fold's chain
            # rule and the fused loss -- a few hundred KB, not counted)
            "ncfp_finish": lambda: (rows * (512 + 512 + 4 * 256), 3 * 2 * rows * 64 * 64),
        }[which]

    def forward(self) -> torch.Tensor:
        d = self._desc()
        fn = _lib.load().ctr_ncf_proj_fwd
        if not _profiling():
            rc = fn(C.byref(d), _lib.stream_ptr())
        else:   # one call per launch, so that each gets its own event pair
            rc = 0
            for phase, label in ((1, "ncfp_prep"), (2, "ncfp_fwd")):
                d.phases = phase
                rc = rc or _timed(label, self._meta(label), fn, C.byref(d), _lib.stream_ptr())
        if rc in _REFUSED:
            return None
        _lib.check(rc, "ctr_ncf_proj_fwd")
        return self.prob

    def backward(self, gprob: Optional[torch.Tensor], grads: dict, zero: Optional[torch.Tensor],
                 target: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None) -> None:
        """``grads[id(param)]``: where each parameter's gradient accumulates; ``zero``: the flat buffer behind them,
        cleared by the call's first launch.  With ``target`` (float32, one element per sample, any stride) ``gprob`` is
        not read: the gradient is the binary cross entropy's for an upstream of exactly 1, formed inside the per-sample
        launch, and ``loss`` (a float32 scalar, optional) receives the mean loss from the call's last launch."""
        if getattr(self, "_spent", False):
            # the first backward hands the plan buffer back to its holder: the next forward may have rebuilt it for
            # other ids by the time a second backward over this forward would read it
            raise RuntimeError("NeuralCF backward consumes what its forward saved: run the forward again before a second "
                               "backward (retain_graph is not supported)")
        self._spent = True
        gmf_u, gmf_i, mlp_u, mlp_i = self.tables
        d = self._desc()
        g = _lib.NcfProjGrad()
        if gprob is not None:
            gprob = gprob.reshape(-1)
            g.gprob, g.ldgprob = gprob.data_ptr(), gprob.stride(0) if gprob.numel() > 1 else 1
        if target is not None:
            _lib.require_device(target)
            if target.dtype != torch.float32 or target.dim() != 1 or target.numel() != self.batch:
                raise ValueError("NcfProj.backward: target must be float32 with one element per sample, flattened")
            g.target, g.ldtarget = target.data_ptr(), target.stride(0) if target.numel() > 1 else 1
        if loss is not None:
            _lib.require_device(loss)
            if loss.dtype != torch.float32 or loss.numel() != 1:
                raise ValueError("NcfProj.backward: loss must be one float32")
            g.loss = loss.data_ptr()
        for k, layer in enumerate(self.hidden):
            g.layers[k].gw, g.layers[k].gb = grads[id(layer.weight)].data_ptr(), grads[id(layer.bias)].data_ptr()
        g.g_mlp_user, g.g_mlp_item, g.g_gmf_user, g.g_gmf_item = (grads[id(t)].data_ptr() for t in (mlp_u, mlp_i, gmf_u, gmf_i))
        pw, pb = self.proj
        hw, hb = self.head
        g.g_proj_w, g.ld_g_proj_w, g.g_proj_b = grads[id(pw)].data_ptr(), _ld(grads[id(pw)]), _lib.ptr(grads.get(id(pb)))
        g.g_head_w, g.g_head_b = grads[id(hw)].data_ptr(), _lib.ptr(grads.get(id(hb)))
        need = C.c_int64(0)
        _lib.check(_lib.load().ctr_ncf_proj_workspace_floats(self.batch, self.nu, self.ni, C.byref(need)), "workspace")
        ws = _scratch(gmf_u.device) if need.value <= SCRATCH_FLOATS else torch.empty(need.value, dtype=torch.float32,
                                                                                      device=gmf_u.device)
        g.workspace, g.workspace_floats = ws.data_ptr(), ws.numel()
        g.zero_buf, g.zero_floats = _lib.ptr(zero), zero.numel() if zero is not None else 0
        fn = _lib.load().ctr_ncf_proj_bwd
        if not _profiling():
            rc = fn(C.byref(d), C.byref(g), _lib.stream_ptr())
        else:
            rc = 0
            for phase, label in ((1, "ncfp_bwd"), (2, "ncfp_segsum"), (4, "ncfp_finish")):
                g.phases = phase
                rc = rc or _timed(label, self._meta(label), fn, C.byref(d), C.byref(g), _lib.stream_ptr())
        _lib.check(rc, "ctr_ncf_proj_bwd")
        if self._owns:
            self._holder.state = "clean"     # (the plan has been read; the next forward rewrites what it reads)
        self._owns = False


def rows_sum_act_fwd(table_a, idx_a, table_b, idx_b, act: int, out, err_flag=None) -> torch.Tensor:
    """out[b] = act(table_a[idx_a[b]] + table_b[idx_b[b]]) (ctr_rows_sum_act_fwd)"""
    out = _mat(out, "out")
    _lib.require_device(table_a, table_b, idx_a, idx_b)
    batch, width = idx_a.numel(), table_a.shape[1]
    _call("rows_sum_act_fwd", "ctr_rows_sum_act_fwd", lambda: (batch * (16 + 12 * width), batch * width),
          table_a.data_ptr(), idx_a.data_ptr(), idx_a.stride(0) if batch > 1 else 1, table_a.shape[0], table_b.data_ptr(),
          idx_b.data_ptr(), idx_b.stride(0) if batch > 1 else 1, table_b.shape[0], batch, width, act, out.data_ptr(),
          _ld(out), _lib.ptr(err_flag), _lib.stream_ptr())
    return out


def mf_fwd(user_table, item_table, user_idx, item_idx, err_flag=None) -> torch.Tensor:
    _lib.require_device(user_table, item_table, user_idx, item_idx)
    batch = user_idx.numel()
    prob = torch.empty(batch, dtype=torch.float32, device=user_table.device)
    dim = user_table.shape[1]
    _call("mf_fwd", "ctr_mf_fwd", lambda: (batch * (8 * dim + 16 + 4), 2 * batch * dim), user_table.data_ptr(),
          user_table.shape[0], item_table.data_ptr(), item_table.shape[0], dim, user_idx.data_ptr(), item_idx.data_ptr(),
          batch, prob.data_ptr(), _lib.ptr(err_flag), _lib.stream_ptr())
    return prob


def mf_bwd(user_table, item_table, user_idx, item_idx, prob, gprob, guser, gitem) -> None:
    dim, batch = user_table.shape[1], user_idx.numel()
    _call("mf_bwd", "ctr_mf_bwd", lambda: (batch * (8 * dim + 16 + 8 + 16 * dim), 4 * batch * dim), user_table.data_ptr(),
          user_table.shape[0], item_table.data_ptr(), item_table.shape[0], dim, user_idx.data_ptr(), item_idx.data_ptr(),
          batch, prob.data_ptr(), gprob.data_ptr(), _lib.ptr(guser), _lib.ptr(gitem), _lib.stream_ptr())
