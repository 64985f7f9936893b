"""C ABI wrappers of the tree-cost, optimiser, NK and datagen entry points for
the guard-band protocol (tests/_guard.py), one per entry point of
include/trex_hip.h, argument lists as in trex_amd/tree.py, evals.py, nk.py and
datagen.py.  tests/test_guard_tree_gpu.py and test_guard_nk_datagen_gpu.py
drive them.

Every wrapper takes a ``run`` (a ``_guard.Run`` for R1 / R2, or a ``Plain``
for an R0 on plain torch tensors where no Python wrapper of the entry point
exists) and host arrays; optional pointers are ``None`` for NULL.  In-place
tensors go through ``run.inout``.

``refuse=<TREX_E_* code>``: the entry point must return that code, and every
output is a kept region as a whole (every byte still at its prefill).
"""

from __future__ import annotations

import numpy as np
import torch

from _guard import F32, I8, I32, _abi

F64, U8 = torch.float64, torch.uint8
E_ARG, E_UNSUPPORTED = -1, -3  # TREX_E_ARG, TREX_E_UNSUPPORTED (include/trex_hip.h)


class Plain:
    """``Run``'s interface on plain torch tensors (torch's caching allocator,
    no guards, no prefill): the R0 of an entry point without a Python wrapper
    is the same ABI call on these."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.r = 0
        self.outs = {}

    def _t(self, array):
        t = array if isinstance(array, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(array))
        return t.to(self.device).contiguous().clone()

    def input(self, name, array):
        return None if array is None else self._t(array)

    def output(self, name, shape, dtype, keep=None, fill=None):
        t = torch.empty(shape, dtype=dtype, device=self.device)
        if keep is not None and fill is not None:
            t.masked_fill_(torch.as_tensor(np.asarray(keep, dtype=bool)).to(self.device), fill)
        self.outs[name] = t
        return t

    def inout(self, name, array, keep=None):
        self.outs[name] = self._t(array)
        return self.outs[name]

    def workspace(self, nbytes, init=False, name="workspace"):
        assert not init
        return torch.empty(nbytes, dtype=U8, device=self.device)


def plain(device, call):
    """r0 of ``_guard.protocol``: ``call`` on plain tensors."""
    def r0():
        run = Plain(device)
        call(run)
        return run.outs
    return r0


def _go(run, name, *args, refuse=None):
    """lib.<name>(*args, stream): tensors pass as their pointers."""
    check, lib, ptr, st = _abi(run.device)
    rc = getattr(lib, name)(*[ptr(a) if isinstance(a, torch.Tensor) else a for a in args], st)
    if refuse is None:
        check(rc)
    else:
        assert rc == refuse, f"{name}: expected a refusal with code {refuse}, got {rc}"


def _out(run, name, shape, dtype, refuse=None, keep=None, fill=None):
    if refuse is not None:
        keep, fill = np.ones(shape, bool), None
    return run.output(name, shape, dtype, keep=keep, fill=fill)


def _io(run, name, array, refuse=None, keep=None):
    if refuse is not None:
        keep = np.ones(np.shape(array), bool)
    return run.inout(name, array, keep=keep)


def _lib(run):
    return _abi(run.device)[1]


def tree_ws_bytes(run, N, K):
    return int(_lib(run).trex_tree_workspace_bytes(N, K))


def step_state(count=0, bc1=0.0, bc2=0.0, T=0.0, Tn=0.0):
    """Host image of a device step state (trex_step_state_bytes() = 32 bytes:
    int count, float bc1, bc2, T, Tn, 3 pad words)."""
    st = np.zeros(8, np.int32)
    st[0] = count
    st[1:5] = np.array([bc1, bc2, T, Tn], np.float32).view(np.int32)
    return st


# ---------------------------------------------------------------------------
# GEMM family (tree_gram.hip, tree_mf.hip)
# ---------------------------------------------------------------------------
def skip_block(N, skip):
    """Kept region of trex_tree_gram_skip*'s G: both i, j < 64 floor(skip / 64)."""
    t0 = 64 * (skip // 64)
    keep = np.zeros((N, N), bool)
    keep[:t0, :t0] = True
    return keep if t0 else None


def tree_gram(run, S, *, skip=None, max_abs=None, refuse=None):
    """trex_tree_gram (skip None), _gram_skip, _gram_skip_x3 (max_abs given)."""
    N, K = S.shape
    s = run.input("S", S)
    g = _out(run, "G", (N, N), F32, refuse, keep=skip_block(N, skip or 0))
    nb = tree_ws_bytes(run, N, K)
    ws = run.workspace(nb)
    if skip is None:
        _go(run, "trex_tree_gram", s, N, K, g, ws, nb, refuse=refuse)
    elif max_abs is None:
        _go(run, "trex_tree_gram_skip", s, N, K, skip, g, ws, nb, refuse=refuse)
    else:
        _go(run, "trex_tree_gram_skip_x3", s, N, K, skip, float(max_abs), g, ws, nb, refuse=refuse)


def tree_gram_x3p(run, S16, skip, max_abs, *, codes=None, n_leaf=0, Q=4, refuse=None):
    """trex_tree_gram_skip_x3p, and _x3p_codes when codes is given (S16: the
    pre-split operand as the (N, K) int32 words trex_tree_split_x3 wrote)."""
    N, K = S16.shape
    s = run.input("S16", S16)
    g = _out(run, "G", (N, N), F32, refuse, keep=skip_block(N, skip))
    nb = tree_ws_bytes(run, N, K)
    ws = run.workspace(nb)
    if codes is None:
        _go(run, "trex_tree_gram_skip_x3p", s, N, K, skip, float(max_abs), g, ws, nb,
            refuse=refuse)
    else:
        c = run.input("codes", codes)
        _go(run, "trex_tree_gram_skip_x3p_codes", s, N, K, skip, float(max_abs), c, codes.size,
            n_leaf, Q, g, ws, nb, refuse=refuse)


def tree_gram_mirror(run, Gm, row0):
    """G in/out; only G[i][j], i < row0 <= j, is written."""
    N = Gm.shape[0]
    keep = np.ones((N, N), bool)
    keep[:row0, row0:] = False
    g = run.inout("G", Gm, keep=keep)
    _go(run, "trex_tree_gram_mirror", g, N, row0)


def tree_mf(run, M, S):
    N, K = S.shape
    m, s = run.input("M", M), run.input("S", S)
    d = run.output("dS", (N, K), F32)
    _go(run, "trex_tree_mf", m, s, N, K, d)


def tree_mf_rows(run, M, S, row0, nrows, *, max_abs=None, codes=None, n_leaf=0, Q=4, refuse=None):
    """trex_tree_mf_rows; _mf_rows_x3 (max_abs = (max_abs_m, max_abs_s));
    _mf_rows_x3_codes (codes given too)."""
    N, K = S.shape
    m, s = run.input("M", M), run.input("S", S)
    d = _out(run, "dS_rows", (nrows, K), F32, refuse)
    if max_abs is None:
        _go(run, "trex_tree_mf_rows", m, s, N, K, row0, nrows, d, refuse=refuse)
    elif codes is None:
        _go(run, "trex_tree_mf_rows_x3", m, s, N, K, row0, nrows, float(max_abs[0]),
            float(max_abs[1]), d, refuse=refuse)
    else:
        c = run.input("codes", codes)
        _go(run, "trex_tree_mf_rows_x3_codes", m, s, N, K, row0, nrows, float(max_abs[0]),
            float(max_abs[1]), c, codes.size, n_leaf, Q, d, refuse=refuse)


def tree_mf_rows_x3p(run, M16, S16, row0, nrows, max_abs, *, codes=None, n_leaf=0, Q=4,
                     refuse=None):
    """M16 (N, ldm) and S16 (N, K): int32 words of the pre-split operands."""
    N, K = S16.shape
    ldm = M16.shape[1]
    m, s = run.input("M16", M16), run.input("S16", S16)
    c = run.input("codes", codes)
    d = _out(run, "dS_rows", (nrows, K), F32, refuse)
    _go(run, "trex_tree_mf_rows_x3p", m, ldm, s, N, K, row0, nrows, float(max_abs[0]),
        float(max_abs[1]), c, 0 if codes is None else codes.size, n_leaf, Q, d, refuse=refuse)


def tree_split_x3(run, X, cols, max_abs, ldo):
    """X (rows, ldx) f32; out (rows, ldo) words, every one written by the
    call (groups past cols zero: the padding is the kernel's, not the caller's)."""
    rows, ldx = X.shape
    x = run.input("X", X)
    out = run.output("out", (rows, ldo), I32)
    _go(run, "trex_tree_split_x3", x, rows, cols, ldx, float(max_abs), out, ldo)


def tree_leaf_codes(run, S, n_leaf, L, Q, *, refuse=None):
    """S (N, L * Q); codes [lcr][L] bytes and the status word (the call
    clears it first), both outputs."""
    lib = _lib(run)
    nb = int(lib.trex_tree_leaf_codes_bytes(n_leaf, L))
    s = run.input("S", S)
    codes = _out(run, "codes", (max(nb, L),), U8, refuse)
    status = _out(run, "status", (1,), I32, refuse)
    _go(run, "trex_tree_leaf_codes", s, n_leaf, L, Q, codes, max(nb, L), status, refuse=refuse)


# ---------------------------------------------------------------------------
# surrogate, constraint, costs, topology / sequence maps (tree.hip)
# ---------------------------------------------------------------------------
def tree_surrogate(run, S, A, *, grads=True):
    """S (N, K); dS / dA / G_out all given or all NULL."""
    N, K = S.shape
    s, a = run.input("S", S), run.input("A", A)
    loss = run.output("loss", (1,), F32)
    dS = run.output("dS", (N, K), F32) if grads else None
    dA = run.output("dA", (N, N), F32) if grads else None
    Go = run.output("G_out", (N, N), F32) if grads else None
    nb = tree_ws_bytes(run, N, K)
    ws = run.workspace(nb)
    _go(run, "trex_tree_surrogate", s, a, N, K, loss, dS, dA, Go, ws, nb)


def tree_surrogate_combine(run, A, Gm):
    """workspace: exactly 8 N bytes."""
    N = A.shape[0]
    a, g = run.input("A", A), run.input("G", Gm)
    loss = run.output("loss", (1,), F32)
    dA, M = run.output("dA", (N, N), F32), run.output("M", (N, N), F32)
    ws = run.workspace(8 * N)
    _go(run, "trex_tree_surrogate_combine", a, g, N, loss, dA, M, ws)


def tree_surrogate_constraint(run, A, Gm, scale, grad_scale, *, state=None, max_abs_m=0.0,
                              ldm16=0):
    """workspace: exactly N + (N - 1) / 2 doubles; M16 (ldm16 > 0): every word
    of [N][ldm16] is written by the call (zero past N)."""
    N = A.shape[0]
    a, g = run.input("A", A), run.input("G", Gm)
    st = run.input("state", state)
    loss = run.output("loss", (1,), F32)
    dA, M = run.output("dA", (N, N), F32), run.output("M", (N, N), F32)
    M16 = run.output("M16", (N, ldm16), I32) if ldm16 else None
    ws = run.workspace(8 * (N + (N - 1) // 2))
    _go(run, "trex_tree_surrogate_constraint", a, g, N, float(scale), float(grad_scale), st, loss,
        dA, M, float(max_abs_m), M16, ldm16, ws)


def tree_constraint(run, A, scale, grad_scale, *, loss0=None, dA0=None, state=None):
    """trex_tree_constraint, or _dev when state is given.  loss0 given:
    accumulate = 1, the loss is in/out; dA0 given: dA in/out (+=)."""
    N = A.shape[0]
    a = run.input("A", A)
    st = run.input("state", state)
    acc = int(loss0 is not None)
    loss = run.inout("loss", loss0) if acc else run.output("loss", (1,), F32)
    dA = run.inout("dA", dA0) if dA0 is not None else None
    ws = run.workspace(tree_ws_bytes(run, N, 1))
    if state is None:
        _go(run, "trex_tree_constraint", a, N, float(scale), float(grad_scale), loss, acc, dA, ws)
    else:
        _go(run, "trex_tree_constraint_dev", a, N, float(scale), st, loss, acc, dA, ws)


def tree_soft_cost(run, S, A, C, ckind):
    """S (N, L, Q); W_scratch [N][L][Q] is scratch when ckind > 0."""
    N, L, Q = S.shape
    s, a, c = run.input("S", S), run.input("A", A), run.input("C", C)
    loss = run.output("loss", (1,), F32)
    W = run.workspace(N * L * Q * 4, name="W_scratch") if ckind else None
    nb = tree_ws_bytes(run, N, L * Q)
    ws = run.workspace(nb)
    _go(run, "trex_tree_soft_cost", s, a, c, ckind, N, L, Q, loss, W, ws, nb)


def tree_compute_cost(run, S, A, subst):
    N, L, Q = S.shape
    s, a, c = run.input("S", S), run.input("A", A), run.input("subst", subst)
    cost = run.output("cost", (1,), F32)
    ws = run.workspace(tree_ws_bytes(run, N, 1))
    _go(run, "trex_tree_compute_cost", s, a, c, N, L, Q, cost, ws)


def tree_discretize(run, A, n_nodes):
    nrows, ncols = A.shape
    a = run.input("A", A)
    out = run.output("out", (nrows, n_nodes), F32)
    _go(run, "trex_tree_discretize", a, nrows, ncols, n_nodes, out)


def tree_update_tree(run, theta, noise, gates, T):
    n_m1, n_anc = theta.shape
    N = n_m1 + 1
    th, nz, gt = run.input("theta", theta), run.input("noise", noise), run.input("gates", gates)
    A = run.output("A", (N, N), F32)
    _go(run, "trex_tree_update_tree", th, nz, gt, N, n_anc, float(T), A)


def tree_update_tree_bwd(run, A, dA, gates, n_anc, T):
    N = A.shape[0]
    a, d, gt = run.input("A", A), run.input("dA", dA), run.input("gates", gates)
    dth = run.output("dtheta", (N - 1, n_anc), F32)
    _go(run, "trex_tree_update_tree_bwd", a, d, gt, N, n_anc, float(T), dth)


ADAM = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-8)


def _hyper(h=ADAM):
    return float(h["lr"]), float(h["b1"]), float(h["b2"]), float(h["eps"])


def tree_update_tree_bwd_adam(run, A, dA, gates, n_anc, T, params, mu, nu, *, dtheta=True, count=1,
                              state=None):
    N = A.shape[0]
    a, d, gt = run.input("A", A), run.input("dA", dA), run.input("gates", gates)
    st = run.input("state", state)
    dth = run.output("dtheta", (N - 1, n_anc), F32) if dtheta else None
    p, m, v = run.inout("params", params), run.inout("mu", mu), run.inout("nu", nu)
    _go(run, "trex_tree_update_tree_bwd_adam", a, d, gt, N, n_anc, float(T), dth, p, m, v,
        0 if state is not None else count, st, *_hyper())


def tree_update_seq(run, x, T):
    n_anc, L, Q = x.shape
    xi = run.input("x", x)
    s = run.output("s_anc", (n_anc, L, Q), F32)
    _go(run, "trex_tree_update_seq", xi, n_anc, L, Q, float(T), s)


def tree_update_seq_bwd(run, s_anc, ds_anc, T):
    n_anc, L, Q = s_anc.shape
    s, ds = run.input("s_anc", s_anc), run.input("ds_anc", ds_anc)
    dx = run.output("dx", (n_anc, L, Q), F32)
    _go(run, "trex_tree_update_seq_bwd", s, ds, n_anc, L, Q, float(T), dx)


# ---------------------------------------------------------------------------
# optimiser kernels (tree_opt.hip)
# ---------------------------------------------------------------------------
def adam_step(run, params, grads, mu, nu, *, count=3, state=None, parts=None, clip=0.0):
    """trex_adam_step, or _dev when state is given; parts: the fp64 clip
    partials (None: no clipping)."""
    n = params.size
    g, pt, st = run.input("grads", grads), run.input("parts", parts), run.input("state", state)
    p, m, v = run.inout("params", params), run.inout("mu", mu), run.inout("nu", nu)
    tail = (pt, 0 if parts is None else parts.size, float(clip))
    if state is None:
        _go(run, "trex_adam_step", p, g, m, v, n, count, *_hyper(), *tail)
    else:
        _go(run, "trex_adam_step_dev", p, g, m, v, n, st, *_hyper(), *tail)


# kind -> (b1, b2, eps, weight_decay), as trex_amd.evals.Optimizer
OPTAX = {0: (0.9, 0.999, 1e-8, 0.0), 1: (0.9, 0.999, 1e-8, 0.01), 2: (0.9, 0.0, 0.0, 0.0),
         3: (0.0, 0.9, 1e-8, 0.0)}


def optax_step(run, kind, params, grads, s1, s2, *, count=3, state=None, parts=None, clip=0.0):
    """trex_optax_step, or _dev when state is given.  sgd has no state2,
    rmsprop no state1: NULL."""
    n = params.size
    g, pt, st = run.input("grads", grads), run.input("parts", parts), run.input("state", state)
    p = run.inout("params", params)
    a = run.inout("state1", s1) if kind != 3 else None
    b = run.inout("state2", s2) if kind != 2 else None
    b1, b2, eps, wd = OPTAX[kind]
    tail = (0.01, b1, b2, eps, wd, pt, 0 if parts is None else parts.size, float(clip))
    if state is None:
        _go(run, "trex_optax_step", kind, p, g, a, b, n, count, *tail)
    else:
        _go(run, "trex_optax_step_dev", kind, p, g, a, b, n, st, *tail)


def sq_norm_parts(run, x, n_parts):
    xi = run.input("x", x)
    parts = run.output("parts", (n_parts,), F64)
    _go(run, "trex_sq_norm_parts", xi, x.size, parts, n_parts)


def adam_seq_step(run, s_anc, ds_anc, T, params, mu, nu, *, count=2, grads_out=True):
    n_anc, L, Q = s_anc.shape
    s, ds = run.input("s_anc", s_anc), run.input("ds_anc", ds_anc)
    p, m, v = run.inout("params", params), run.inout("mu", mu), run.inout("nu", nu)
    go = run.output("grads_out", (n_anc, L, Q), F32) if grads_out else None
    _go(run, "trex_adam_seq_step", s, ds, n_anc, L, Q, float(T), p, m, v, count, *_hyper(), go)


def adam_seq_update_step(run, ds_anc, T, Tn, params, mu, nu, *, count=2, state=None,
                         x3p_max_abs=None, dev=False):
    """trex_adam_seq_update_step; _dev (dev=True: T / Tn / count from state);
    _x3p (x3p_max_abs given: s16_next is the output, state optional)."""
    n_anc, L, Q = ds_anc.shape
    ds, st = run.input("ds_anc", ds_anc), run.input("state", state)
    p, m, v = run.inout("params", params), run.inout("mu", mu), run.inout("nu", nu)
    if x3p_max_abs is not None:
        s16 = run.output("s16_next", (n_anc, L, Q), I32)
        _go(run, "trex_adam_seq_update_step_x3p", ds, n_anc, L, Q, float(T), float(Tn), p, m, v,
            count, *_hyper(), st, float(x3p_max_abs), s16)
        return
    sn = run.output("s_next", (n_anc, L, Q), F32)
    if dev:
        _go(run, "trex_adam_seq_update_step_dev", ds, n_anc, L, Q, st, p, m, v, *_hyper(), sn)
    else:
        _go(run, "trex_adam_seq_update_step", ds, n_anc, L, Q, float(T), float(Tn), p, m, v, count,
            *_hyper(), sn)


def step_advance(run, state, b1, b2, temps):
    st = run.inout("state", state)
    t = run.input("temps", temps)
    _go(run, "trex_step_advance", st, float(b1), float(b2), t, 0 if temps is None else temps.size)


def gumbel_noise(run, seed, state, n):
    st = run.input("state", state)
    out = run.output("out", (n,), F32)
    _go(run, "trex_gumbel_noise", int(seed), st, n, out)


# ---------------------------------------------------------------------------
# NK (nk.hip) and datagen (datagen.hip)
# ---------------------------------------------------------------------------
def nk_parental_logits(run, S, rows, inter, k, F):
    """S (N, L, Q); rows int32 (R,); inter int32 (L, k) (None when k = 0)."""
    _, L, Q = S.shape
    R = rows.size
    s, r, it, f = (run.input("S", S), run.input("rows", rows),
                   run.input("interactions", inter if k else None), run.input("fitness", F))
    out = run.output("logits", (R, L, Q), F32)
    _go(run, "trex_nk_parental_logits", s, r, R, L, Q, it, k, f, out)


def nk_landscape_loss(run, plan, n_parents, n_nonroot, S, inter, k, F, mask, lam, surrogate, *,
                      d_S_in=None, d_S=True):
    """workspace: exactly trex_nk_workspace_bytes; plan / interactions int32."""
    N, L, Q = S.shape
    pl, s, f = run.input("plan", plan), run.input("S", S), run.input("fitness", F)
    it = run.input("interactions", inter if k else None)
    mk, su, di = run.input("seq_mask", mask), run.input("surrogate", surrogate), \
        run.input("d_S_in", d_S_in)
    loss = run.output("loss", (1,), F32)
    dS = run.output("d_S", (N, L, Q), F32) if d_S else None
    nb = int(_lib(run).trex_nk_workspace_bytes(N, L, Q, k, n_parents))
    ws = run.workspace(nb)
    n_valid = float(L if mask is None else mask.sum())
    _go(run, "trex_nk_landscape_loss", pl, n_parents, s, N, L, Q, it, k, f, mk, n_valid, float(lam),
        n_nonroot, su, di, loss, dS, ws, nb)


def datagen_groundtruth(run, seed, n_leaves, L, Q, n_mut):
    seqs = run.output("seqs", (2 * n_leaves - 1, L), I8)
    nb = int(_lib(run).trex_datagen_workspace_bytes(n_leaves, n_mut))
    ws = run.workspace(nb)
    _go(run, "trex_datagen_groundtruth", int(seed), n_leaves, L, Q, n_mut, seqs, ws, nb)


def datagen_uniform_states(run, seed, n, Q):
    out = run.output("out", (n,), I8)
    _go(run, "trex_datagen_uniform_states", int(seed), n, Q, out)


def datagen_nk_tree(run, seed, Q, inter, F, parent, order, offsets, root, seqs0, rate, std, cp,
                    branch_length):
    """seqs0 (n_nodes, L) int8 with the root row filled: in/out, the root row
    kept; offsets (level_offsets) is a host array."""
    n, L = seqs0.shape
    K = inter.shape[1]
    it, f = run.input("interactions", inter if K else None), run.input("fitness", F)
    pa, od = run.input("parent", parent), run.input("order", order)
    keep = np.zeros((n, L), bool)
    keep[root] = True
    sq = run.inout("seqs", seqs0, keep=keep)
    off = np.ascontiguousarray(offsets, np.int32)
    _go(run, "trex_datagen_nk_tree", int(seed), n, L, Q, K, it, f, pa, od, off.ctypes.data,
        len(off) - 1, float(rate), float(std), float(cp), int(branch_length), sq)
