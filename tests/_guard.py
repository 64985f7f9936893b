"""Guard-band harness: buffers between canary bytes, and the three-run
protocol of tests/test_guard_gpu.py (plain helpers, any torch device).

``guarded(shape, dtype, device, payload=..., guard_byte=...)`` makes one flat
uint8 allocation ``[front guard | payload | back guard]``.  Each guard is
GUARD_BYTES (1 MiB, the size of test_gram_x3_stays_inside_its_workspace's
canary), so the payload starts at torch's base alignment plus 1 MiB and the
16-byte row contracts of include/trex_hip.h hold; the back guard starts at the
byte after the payload with no rounding, so a 4-byte load over the tail of an
odd-length int8 table reads guard bytes.

The protocol runs one call three times with the same environment:

    run   buffers                      input guards     output prefill   output guards
    R0    the engine method's own      -                -                -
    R1    guarded                      0x01             0x00             0xA5
    R2    guarded                      0xFF             0xFF             0x5A

(0x01 is a valid leaf code and a tiny float, 0xFF is code -1 and a NaN.)  R1 ==
R2 bitwise catches an output entry that was never written and a read past an
input that reaches a result; both == R0; every guard of every buffer intact;
every input payload unchanged.  The workspace is a guarded buffer of exactly
the size the matching ``*_workspace_bytes`` function returns, zeroed with
trex_workspace_init where the header asks for that and prefilled like an
output where it does not.

An output (or in/out table) may have a **kept region** (``keep=``: a boolean
mask of its entries): entries the header says the call leaves alone --
trex_tree_gram_skip's cached block, trex_datagen_nk_tree's root row, padding
that is the caller's to zero.  It is prefilled like any output (``fill=``: the
caller's bytes there instead, e.g. the zeros a header asks for); after the
call every kept byte still holds what it held before (a write into the
region is flagged with its entries), and R1 == R2 == R0 is asked outside it
only, where a never-written entry shows as ever.

R1 and R2 drive the C ABI directly (one thin wrapper per entry point below,
argument lists as in trex_amd/sankoff.py and trex_amd/ragged.py), because
several engine methods allocate their own outputs.
"""

from __future__ import annotations

import numpy as np
import torch

GUARD_BYTES = 1 << 20

# run -> guard byte of inputs, prefill byte of outputs, guard byte of outputs
PROTOCOL = {1: dict(in_guard=0x01, prefill=0x00, out_guard=0xA5),
            2: dict(in_guard=0xFF, prefill=0xFF, out_guard=0x5A)}


def _bytes_of(x):
    """flat uint8 CPU tensor of a numpy array's / tensor's bytes."""
    if isinstance(x, torch.Tensor):
        t = x.detach().cpu().contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(x))
    return t.reshape(-1).view(torch.uint8).clone()


def _entry_bytes(view):
    """(numel, itemsize) uint8 CPU tensor: the bytes of every entry."""
    t = view.detach().cpu().contiguous()
    return t.reshape(-1).view(torch.uint8).reshape(t.numel(), t.element_size())


class Guarded:
    """Handle of one guarded allocation (see ``guarded``)."""

    def __init__(self, flat, view, nbytes, guard_byte, host):
        self.flat, self.view, self.nbytes, self.guard_byte, self.host = (flat, view, nbytes,
                                                                         guard_byte, host)

    def payload_bytes(self):
        return self.flat[GUARD_BYTES:GUARD_BYTES + self.nbytes]

    def check(self, name="buffer"):
        """Both guards still hold their fill byte everywhere; the message gives
        the first and last offending byte offset relative to the payload
        (negative: before it; >= its size: behind it)."""
        g = self.guard_byte
        front = self.flat[:GUARD_BYTES] != g
        back = self.flat[GUARD_BYTES + self.nbytes:] != g
        if not (bool(front.any()) or bool(back.any())):
            return
        off = torch.cat([front.nonzero().reshape(-1).cpu() - GUARD_BYTES,
                         back.nonzero().reshape(-1).cpu() + self.nbytes])
        raise AssertionError(
            f"{name}: {off.numel()} guard byte(s) overwritten around a payload of {self.nbytes} "
            f"bytes: first at offset {int(off.min())}, last at offset {int(off.max())} "
            f"(payload = offsets 0 .. {self.nbytes - 1})")

    def unchanged(self, name="input"):
        """The payload still equals the host copy it was filled from."""
        assert self.host is not None, f"{name}: no host copy to compare with"
        now = self.payload_bytes().cpu()
        bad = (now != self.host).nonzero().reshape(-1)
        if bad.numel() == 0:
            return
        item = self.view.element_size()
        raise AssertionError(
            f"{name}: input overwritten: {bad.numel()} byte(s) differ from the host copy, first "
            f"in element {int(bad[0]) // item}, last in element {int(bad[-1]) // item} of "
            f"{self.view.numel()}")


def guarded(shape, dtype, device, payload=0, guard_byte=0xA5):
    """(typed payload view, handle) of ``[front guard | payload | back guard]``.

    payload: an int (every payload byte gets that value) or an array / tensor
    of ``dtype`` with ``shape``'s element count (copied in; the handle keeps
    the bytes for ``unchanged``)."""
    shape = tuple(int(s) for s in (shape if hasattr(shape, "__len__") else (shape,)))
    item = torch.empty((), dtype=dtype).element_size()
    nbytes = int(np.prod(shape, dtype=np.int64)) * item
    assert nbytes > 0, "empty payload"
    flat = torch.full((2 * GUARD_BYTES + nbytes,), guard_byte, dtype=torch.uint8, device=device)
    body = flat[GUARD_BYTES:GUARD_BYTES + nbytes]
    host = None
    if isinstance(payload, (int, np.integer)):
        body.fill_(int(payload))
    else:
        host = _bytes_of(payload)
        assert host.numel() == nbytes, (host.numel(), nbytes)
        body.copy_(host)
    view = body.view(dtype).reshape(shape)
    assert view.data_ptr() == flat.data_ptr() + GUARD_BYTES
    return view, Guarded(flat, view, nbytes, guard_byte, host)


class Run:
    """The guarded buffers of one call of run R1 or R2."""

    def __init__(self, device, r):
        self.device = torch.device(device)
        self.r = r
        self.p = PROTOCOL[r]
        self.inputs, self.outputs, self.scratch = {}, {}, {}
        self.keep = {}  # output name -> (bool mask of kept entries, their bytes before the call)

    def _add(self, table, name, handle):
        assert not any(name in t for t in (self.inputs, self.outputs, self.scratch)), name
        table[name] = handle

    def input(self, name, array):
        if array is None:
            return None
        dtype = array.dtype if isinstance(array, torch.Tensor) else torch.from_numpy(
            np.asarray(array)).dtype
        v, h = guarded(tuple(array.shape), dtype, self.device, payload=array,
                       guard_byte=self.p["in_guard"])
        self._add(self.inputs, name, h)
        return v

    def _keep(self, name, view, keep, fill=None):
        """Register the kept region of output ``name`` (see the module
        docstring); fill: a value written to the kept entries first."""
        if keep is None:
            return
        mask = torch.as_tensor(np.asarray(keep, dtype=bool)).reshape(tuple(view.shape))
        if fill is not None:
            view.masked_fill_(mask.to(view.device), fill)
        self.keep[name] = (mask, _entry_bytes(view)[mask.reshape(-1)].clone())

    def output(self, name, shape, dtype, keep=None, fill=None):
        v, h = guarded(shape, dtype, self.device, payload=self.p["prefill"],
                       guard_byte=self.p["out_guard"])
        self._add(self.outputs, name, h)
        self._keep(name, v, keep, fill)
        return v

    def inout(self, name, array, keep=None):
        """An in/out table: the caller's bytes between output guards; what the
        call leaves of them is compared between the runs like an output."""
        dtype = array.dtype if isinstance(array, torch.Tensor) else torch.from_numpy(
            np.asarray(array)).dtype
        v, h = guarded(tuple(array.shape), dtype, self.device, payload=array,
                       guard_byte=self.p["out_guard"])
        self._add(self.outputs, name, h)
        self._keep(name, v, keep)
        return v

    def workspace(self, nbytes, init=False, name="workspace"):
        """uint8 workspace of exactly nbytes; init: trex_workspace_init."""
        v, h = guarded((nbytes,), torch.uint8, self.device, payload=self.p["prefill"],
                       guard_byte=self.p["out_guard"])
        self._add(self.scratch, name, h)
        if init:
            from trex_amd._lib import check, lib, ptr, stream_handle

            check(lib().trex_workspace_init(ptr(v), nbytes, stream_handle(self.device)))
        return v

    def finish(self):
        """Synchronise; every guard intact, every input unchanged; the outputs
        as CPU tensors {name: tensor}."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for kind, table in (("input", self.inputs), ("output", self.outputs),
                            ("workspace", self.scratch)):
            for name, h in table.items():
                h.check(f"R{self.r} {kind} {name}")
        for name, h in self.inputs.items():
            h.unchanged(f"R{self.r} input {name}")
        for name, (mask, before) in self.keep.items():
            now = _entry_bytes(self.outputs[name].view)[mask.reshape(-1)]
            bad = (now != before).any(dim=1).nonzero().reshape(-1)
            if bad.numel():
                idx = mask.reshape(-1).nonzero().reshape(-1)[bad]
                raise AssertionError(
                    f"R{self.r} output {name}: kept region written: {bad.numel()} of "
                    f"{int(mask.sum())} kept entries changed, first at flat index {int(idx[0])}, "
                    f"last at {int(idx[-1])} of {mask.numel()}")
        return {name: h.view.cpu().clone() for name, h in self.outputs.items()}


_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def assert_bitwise(a, b, what):
    """Two tensors of one dtype and shape hold the same bytes (a NaN equals the
    same NaN); the message names the first and last differing entry."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (
        f"{what}: {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}")
    it = _INT_OF[a.element_size()]
    bad = (a.reshape(-1).view(it) != b.reshape(-1).view(it)).nonzero().reshape(-1)
    if bad.numel():
        i, j = int(bad[0]), int(bad[-1])
        raise AssertionError(
            f"{what}: {bad.numel()} of {a.numel()} entries differ, first at flat index {i} "
            f"({a.reshape(-1)[i].item()!r} vs {b.reshape(-1)[i].item()!r}), last at {j}")


def protocol(device, r0, call):
    """R0 / R1 / R2 of one call.  r0() -> {name: device tensor} from the engine
    method; call(run) enqueues the same call on ``run``'s guarded buffers.
    Returns R1's outputs (CPU)."""
    ref = r0()
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    ref = {k: v.detach().cpu().clone() for k, v in ref.items() if v is not None}
    outs, keep = {}, {}
    for r in (1, 2):
        run = Run(device, r)
        call(run)
        outs[r] = run.finish()
        keep[r] = {k: m for k, (m, _) in run.keep.items()}
    assert set(outs[1]) == set(outs[2]) and set(ref) <= set(outs[1]), (sorted(ref), sorted(outs[1]))
    assert set(keep[1]) == set(keep[2]) and all(torch.equal(keep[1][k], keep[2][k])
                                                for k in keep[1]), "kept regions differ"

    def outside(k, t):
        """t with its kept entries (checked by finish) zeroed."""
        return t.masked_fill(keep[1][k], 0) if k in keep[1] else t

    for k in outs[1]:
        assert_bitwise(outside(k, outs[1][k]), outside(k, outs[2][k]),
                       f"{k}: R1 vs R2 (an entry never written, or a read outside an input)")
    for k in ref:
        assert_bitwise(outside(k, outs[1][k]), outside(k, ref[k].reshape(outs[1][k].shape)),
                       f"{k}: R1 vs R0")
    return outs[1]


# ---------------------------------------------------------------------------
# C ABI wrappers (include/trex_hip.h), one per entry point
# ---------------------------------------------------------------------------
F32, I8, I32 = torch.float32, torch.int8, torch.int32


def _abi(device):
    from trex_amd._lib import check, lib, ptr, stream_handle

    return check, lib(), ptr, stream_handle(torch.device(device))


def _common(run, plan, leaves, cost):
    return (run.input("plan", plan.host), run.input("leaves", leaves), run.input("cost", cost))


def _dp_shape(plan, L, Q):
    return (plan.B, plan.n_int, L, Q)


def sankoff_fwd(run, plan, leaves, cost, L, Q, tau, *, site_score=True, workspace_bytes=None):
    check, lib, ptr, st = _abi(run.device)
    pl, lv, c = _common(run, plan, leaves, cost)
    dp = run.output("dp", _dp_shape(plan, L, Q), F32)
    ss = run.output("site_score", (plan.B, L), F32) if site_score else None
    ts = run.output("tree_score", (plan.B,), F32)
    nb = int(workspace_bytes or lib.trex_workspace_bytes(plan.B, L, plan.n_all, Q))
    ws = run.workspace(nb, init=True)
    check(lib.trex_sankoff_fwd(ptr(pl), plan.slot_word, ptr(lv), ptr(c), plan.B, L, plan.n_all, Q,
                               float(tau), 0, ptr(dp), ptr(ss), ptr(ts), ptr(ws), nb, st))


def sankoff_bwd(run, plan, leaves, cost, L, Q, tau, dp, d_tree_score, *, workspace_bytes=None):
    check, lib, ptr, st = _abi(run.device)
    pl, lv, c = _common(run, plan, leaves, cost)
    dpt = run.input("dp", dp)
    dts = run.input("d_tree_score", d_tree_score)
    dc = run.output("d_cost", (Q, Q), F32)
    mg = run.output("marginals", _dp_shape(plan, L, Q), F32)
    an = run.output("anc_states", (plan.B, plan.n_int, L), I8)
    nb = int(workspace_bytes or lib.trex_workspace_bytes(plan.B, L, plan.n_all, Q))
    ws = run.workspace(nb, init=True)
    check(lib.trex_sankoff_bwd(ptr(pl), plan.slot_word, ptr(lv), ptr(c), plan.B, L, plan.n_all, Q,
                               float(tau), 0, ptr(dpt), ptr(dts), ptr(dc), ptr(mg), ptr(an),
                               ptr(ws), nb, st))


def sankoff_fwd_bwd(run, plan, leaves, cost, L, Q, tau, d_tree_score, *, workspace_bytes=None):
    check, lib, ptr, st = _abi(run.device)
    pl, lv, c = _common(run, plan, leaves, cost)
    dts = run.input("d_tree_score", d_tree_score)
    dp = run.output("dp", _dp_shape(plan, L, Q), F32)
    ss = run.output("site_score", (plan.B, L), F32)
    ts = run.output("tree_score", (plan.B,), F32)
    dc = run.output("d_cost", (Q, Q), F32)
    mg = run.output("marginals", _dp_shape(plan, L, Q), F32)
    an = run.output("anc_states", (plan.B, plan.n_int, L), I8)
    nb = int(workspace_bytes or lib.trex_workspace_bytes(plan.B, L, plan.n_all, Q))
    ws = run.workspace(nb, init=True)
    check(lib.trex_sankoff_fwd_bwd(ptr(pl), plan.slot_word, ptr(lv), ptr(c), plan.B, L, plan.n_all,
                                   Q, float(tau), 0, ptr(dp), ptr(ss), ptr(ts), ptr(dts), ptr(dc),
                                   ptr(mg), ptr(an), ptr(ws), nb, st))


def sankoff_backtrack(run, plan, cost, dp, L, Q):
    check, lib, ptr, st = _abi(run.device)
    pl, c, dpt = run.input("plan", plan.host), run.input("cost", cost), run.input("dp", dp)
    an = run.output("anc_states", (plan.B, plan.n_int, L), I8)
    check(lib.trex_sankoff_backtrack(ptr(pl), plan.backtrack_ok, ptr(c), ptr(dpt), plan.B, L,
                                     plan.n_all, Q, ptr(an), st))


def dp_to_trex_layout(run, plan, dp, leaves, L, Q):
    check, lib, ptr, st = _abi(run.device)
    dpt, lv = run.input("dp", dp), run.input("leaves", leaves)
    out = run.output("trex_dp", (plan.B, L, plan.n_all, Q), F32)
    check(lib.trex_dp_to_trex_layout(ptr(dpt), ptr(lv), plan.B, L, plan.n_all, Q, ptr(out), st))


def sankoff_outside(run, plan, leaves, cost, L, Q, tau, dp):
    check, lib, ptr, st = _abi(run.device)
    pl, lv, c = run.input("nni_plan", plan.nni_host), run.input("leaves", leaves), \
        run.input("cost", cost)
    dpt = run.input("dp", dp)
    out = run.output("outside", _dp_shape(plan, L, Q), F32)
    check(lib.trex_sankoff_outside(ptr(pl), ptr(lv), ptr(c), plan.B, L, plan.n_all, Q, float(tau),
                                   ptr(dpt), ptr(out), st))


def sankoff_nni(run, plan, leaves, cost, L, Q, tau, dp, outside):
    check, lib, ptr, st = _abi(run.device)
    pl, lv, c = run.input("nni_plan", plan.nni_host), run.input("leaves", leaves), \
        run.input("cost", cost)
    dpt, ot = run.input("dp", dp), run.input("outside", outside)
    score = run.output("nni_score", (plan.B, plan.n_int - 1, 2), F32)
    nb = int(lib.trex_nni_workspace_bytes(plan.B, L, plan.n_all, Q))
    ws = run.workspace(nb)
    check(lib.trex_sankoff_nni(ptr(pl), ptr(lv), ptr(c), plan.B, L, plan.n_all, Q, float(tau),
                               ptr(dpt), ptr(ot), ptr(score), ptr(ws), nb, st))


def sankoff_attach(run, plan, leaves, cost, L, Q, tau, dp, outside, *, new_leaf=None,
                   sub_rows=None):
    check, lib, ptr, st = _abi(run.device)
    pl, lv, c = run.input("attach_plan", plan.attach_host), run.input("leaves", leaves), \
        run.input("cost", cost)
    dpt, ot = run.input("dp", dp), run.input("outside", outside)
    nl, sr = run.input("new_leaf", new_leaf), run.input("sub_rows", sub_rows)
    score = run.output("attach_score", (plan.B, plan.n_all), F32)
    nb = int(lib.trex_attach_workspace_bytes(plan.B, L, plan.n_all, Q))
    ws = run.workspace(nb)
    check(lib.trex_sankoff_attach(ptr(pl), ptr(lv), ptr(c), plan.B, L, plan.n_all, Q, float(tau),
                                  ptr(dpt), ptr(ot), ptr(nl), ptr(sr), ptr(score), ptr(ws), nb,
                                  st))


def sankoff_ragged(run, phase, plan, leaves, cost, Q, tau, *, dp=None, d_tree_score=None):
    """phase 1 forward, 2 adjoint (dp: the forward's packed table), 3 fused;
    every optional output is asked for."""
    check, lib, ptr, st = _abi(run.device)
    p = plan
    pl, lv, c = run.input("plan", p.host), run.input("leaves", leaves), run.input("cost", cost)
    ss = ts = dts = dc = mg = an = None
    if phase == 2:
        dpt = run.input("dp", dp)
    else:
        dpt = run.output("dp", (p.row_sites, Q), F32)
        ss = run.output("site_score", (p.sites,), F32)
        ts = run.output("tree_score", (p.B,), F32)
    if phase & 2:
        dts = run.input("d_tree_score", d_tree_score)
        dc = run.output("d_cost", (Q, Q), F32)
        mg = run.output("marginals", (p.row_sites, Q), F32)
        an = run.output("anc_states", (p.row_sites,), I8)
    nb = int(lib.trex_ragged_workspace_bytes(p.items, Q))
    ws = run.workspace(nb)
    check(lib.trex_sankoff_ragged(phase, ptr(pl), p.B, p.n_slots, p.max_leaves, p.items, ptr(lv),
                                  ptr(c), Q, float(tau), 0, ptr(dpt), ptr(ss), ptr(ts), ptr(dts),
                                  ptr(dc), ptr(mg), ptr(an), ptr(ws), nb, st))


def sankoff_ragged_backtrack(run, plan, cost, dp, Q):
    check, lib, ptr, st = _abi(run.device)
    p = plan
    pl, c, dpt = run.input("plan", p.host), run.input("cost", cost), run.input("dp", dp)
    an = run.output("anc_states", (p.row_sites,), I8)
    check(lib.trex_sankoff_ragged_backtrack(ptr(pl), p.B, p.items, p.steps, p.backtrack_ok, ptr(c),
                                            ptr(dpt), Q, ptr(an), st))


def run_dp(run, children, seqs, cost, dp, bt):
    """children int32 (n_all, 2); seqs float32 (n, n_codes, L); dp (L, n_all,
    Q) and bt (L, n_all, Q, 4) in/out."""
    check, lib, ptr, st = _abi(run.device)
    L, n_all, Q = dp.shape
    ch, sq, c = run.input("children", children), run.input("seqs", seqs), run.input("cost", cost)
    dpt, btt = run.inout("dp", dp), run.inout("bt", bt)
    check(lib.trex_run_dp(ptr(ch), n_all, L, Q, ptr(sq), int(seqs.shape[1]), ptr(c), ptr(dpt),
                          ptr(btt), st))


def backtrack_generic(run, root_node, dp, bt, n_leaves, max_steps=1 << 26):
    """root states from dp (root_state NULL); outputs: states (n_all, L) and
    the status word (zeroed by the caller, as vmapped_backtrack does)."""
    check, lib, ptr, st = _abi(run.device)
    L, n_all, Q = dp.shape
    dpt, btt = run.input("dp", dp), run.input("bt", bt)
    out = run.output("states", (n_all, L), I32)
    status = run.inout("status", np.zeros(1, np.int32))
    nb = int(lib.trex_backtrack_workspace_bytes(n_all, L))
    ws = run.workspace(nb, name="stack")
    check(lib.trex_backtrack_generic(int(root_node), None, ptr(dpt), ptr(btt), n_all,
                                     int(n_leaves), L, Q, ptr(out), ptr(ws), nb, max_steps,
                                     ptr(status), st))


def dp_root_total(run, dp):
    check, lib, ptr, st = _abi(run.device)
    L, n_all, Q = dp.shape
    dpt = run.input("dp", dp)
    site_min = run.output("site_min", (L,), F32)
    total = run.output("total", (1,), F32)
    check(lib.trex_dp_root_total(ptr(dpt), L, n_all, Q, ptr(site_min), ptr(total), st))
