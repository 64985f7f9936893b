"""Guard-band tests: the tree-cost and optimiser kernels stay inside their
buffers ("Memory contract").

Every case is one ``_guard.protocol`` run (tests/_guard.py; wrappers in
tests/_guard_tree.py) on tiny shapes: R0 on the Python wrapper's own buffers
-- or, where the entry point has none, the same ABI call on plain torch
tensors (``_guard_tree.plain``) -- then R1 and R2 through the C ABI on buffers
between 1 MiB canaries with different guard and prefill bytes.  R1 == R2 == R0
bitwise outside kept regions, every kept byte still at its prefill, every
guard intact, every input unchanged, workspaces of exactly the documented
size.  No oracle and no tolerance: values are pinned by tests/test_tree_gpu.py.

GEMM shapes (N, K, skip, row0); the Gram / MF cases run under TREX_GRAM =
TREX_MF in {5, 3, 6}:

    (33, 20, 0, 17)    one row into a second 32-row strip, K % 16 = 4; n_leaf = 17, lcr = 0:
                       the codes entry points refuse (TREX_E_ARG), outputs untouched
    (64, 4, 0, 0)      one 16-B piece per row, exact tiles
    (97, 36, 64, 49)   one row past three strips, 4 columns past a 32-column block, a kept
                       64 x 64 block of G, lcr = 32
    (97, 204, 0, 37)   row0 % 32 != 0, the ragged K tail of test_gram_every_tile_rung
    (130, 36, 65, 65)  two rows past a 128-row pass, lcr = 64
    (320, 204, 64, -)  Grams only: rung 13 of the tiles-per-wave ladder
    (33, 165, 0, 17)   L = 33, Q = 5: rows only 4-B aligned.  The f32 entry points run it; the
                       x3 ones refuse it (K % 4 != 0: TREX_E_UNSUPPORTED, the pre-split ones
                       TREX_E_ARG) and must leave their outputs untouched

x3 operands: S a softmax with one-hot leaf rows, M normal x 20 with max_abs_m =
1.01 max|M|.  Padding of the pre-split operands (M16 past N, split_x3 past
cols) is written by the kernels themselves (include/trex_hip.h), so it is an
ordinary output here: compared in full between R1 and R2.

Shapes the entry points refuse, adjusted or checked as refusals:
trex_adam_seq_update_step_x3p is Q = 4 only -- (16, 67, 4) runs, (1, 1, 2) and
(3, 33, 5) are refusals (TREX_E_ARG, nothing written).

Entry point -> test ids:

    trex_tree_gram, trex_tree_gram_skip               test_gram_f32[<ver>-<shape>]
    trex_tree_gram_skip_x3, _x3p, _x3p_codes          test_gram_x3[<ver>-<shape>]
    trex_tree_gram_mirror                             test_gram_mirror[<N>-<row0>]
    trex_tree_mf, trex_tree_mf_rows                   test_mf_f32[<ver>-<shape>]
    trex_tree_mf_rows_x3, _x3_codes,                  test_mf_x3[<ver>-<shape>]
    trex_tree_mf_rows_x3p (codes NULL and given)
    trex_tree_split_x3                                test_split_x3[<shape>]
    trex_tree_leaf_codes                              test_leaf_codes[<shape>]
    trex_tree_surrogate                               test_surrogate[<N>-<K>-grads|loss]
    trex_tree_surrogate_combine                       test_surrogate_combine[<N>]
    trex_tree_surrogate_constraint                    test_surrogate_constraint[<N>-<state>-<m16>]
    trex_tree_constraint, trex_tree_constraint_dev    test_constraint[<N>-<entry>-<acc>-<dA>]
    trex_tree_soft_cost                               test_soft_cost[<shape>-<ckind>]
    trex_tree_compute_cost                            test_compute_cost[<shape>]
    trex_tree_discretize                              test_discretize
    trex_tree_update_tree                             test_update_tree[<n_leaf>-<noise>-<gates>]
    trex_tree_update_tree_bwd                         test_update_tree_bwd[<n_leaf>-<gates>]
    trex_tree_update_tree_bwd_adam                    test_update_tree_bwd_adam[<n_leaf>-...]
    trex_tree_update_seq, trex_tree_update_seq_bwd    test_update_seq[<shape>]
    trex_adam_step, trex_adam_step_dev                test_adam_step[<n>-<parts>-<entry>]
    trex_optax_step, trex_optax_step_dev              test_optax_step[<kind>-<n>-<parts>-<entry>]
    trex_sq_norm_parts                                test_sq_norm_parts[<n>]
    trex_adam_seq_step                                test_adam_seq_step[<shape>-<grads_out>]
    trex_adam_seq_update_step, _dev, _x3p             test_adam_seq_update_step[<shape>-<entry>]
    trex_step_advance                                 test_step_advance[<case>]
    trex_gumbel_noise                                 test_gumbel_noise[<n>-<state>]
    kept regions on the device                        test_harness_flags_a_write_into_a_kept_region_...

Left out of the three guard files (this one, test_guard_gpu.py,
test_guard_nk_datagen_gpu.py):
    host-only planners (trex_plan_build, trex_nni_plan_build, trex_attach_plan_build,
      trex_ragged_plan_build, trex_fused4_program_build, trex_nk_plan_build): no device memory
    trex_comm_*, trex_allreduce_sum: need more than one rank
    *_bytes / *_ints / trex_version / trex_dp_site_major / trex_tree_leaf_code_rows /
      trex_last_error: size and version queries
    trex_workspace_init: the harness's own zero fill (every test_guard_gpu.py workspace)
    trex_sankoff_fwd_bwd_prog, trex_site_weighted_sum, trex_sankoff_nni_w, trex_sankoff_attach_w:
      Sankoff entry points added after test_guard_gpu.py; they belong in that file's families
      (the fused program next to test_uniform, the weights next to test_outside_nni_attach),
      not among the tree-cost kernels, and are still to be added there
    trex_debug_site2_launches: a host counter
    captured replay of the tree loop: test_tree_device_loop_is_bitwise_eager
    K = 32 800 (five-column-tile MF) and the C5-size shapes: test_tree_gpu.py
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _guard as G
import _guard_tree as W
from trex_amd import tree as TR
from trex_amd._lib import check, lib, ptr, stream_handle

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["5", "3", "6"])
def gram_version(request, monkeypatch):
    """Every Gram / MF kernel version: v5 (one wave per SIMD; the f32 default),
    v3 (the x3 default), v6 (the x3 Gram at two waves per SIMD, A/B)."""
    monkeypatch.setenv("TREX_GRAM", request.param)
    monkeypatch.setenv("TREX_MF", request.param)
    return request.param


def _t(x, device):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device).contiguous()


def _f32(rng, *shape):
    return rng.normal(size=shape).astype(np.float32)


# ---------------------------------------------------------------------------
# the harness's kept regions, once on the device (tests/test_guard_cpu.py
# has the CPU cases): a stand-in for a skip Gram (torch ops) that writes one
# entry of its kept block
# ---------------------------------------------------------------------------
def test_harness_flags_a_write_into_a_kept_region_on_the_device(device):
    N, skip = 70, 64
    S = _f32(np.random.default_rng(0), N, 8)

    def stand_in(run, spoil):
        s = run.input("S", S)
        g = run.output("G", (N, N), torch.float32, keep=W.skip_block(N, skip))
        full = s[:, :1] + s[:, 1][None, :]
        g[skip:] = full[skip:]
        g[:skip, skip:] = full[:skip, skip:]
        if spoil:
            g[63, 63] = full[63, 63]

    r0 = lambda: dict(G=_t(S[:, :1] + S[:, 1][None, :], device))  # noqa: E731
    G.protocol(device, r0, lambda run: stand_in(run, False))
    with pytest.raises(AssertionError, match=rf"output G: kept region written: 1 of 4096 kept "
                                             rf"entries changed, first at flat index {63 * N + 63}"):
        G.protocol(device, r0, lambda run: stand_in(run, True))


# ---------------------------------------------------------------------------
# GEMM family
# ---------------------------------------------------------------------------
GEMM = [(33, 20, 0, 17), (64, 4, 0, 0), (97, 36, 64, 49), (97, 204, 0, 37), (130, 36, 65, 65)]
GRAM_ONLY = [(320, 204, 64, None)]
RAGGED = [(33, 165, 0, 17)]  # Q = 5: f32 entry points only, the x3 ones refuse


def _sid(c):
    return f"{c[0]}x{c[1]}-s{c[2]}-r{c[3]}"


_CASES = {}


def gemm_case(device, N, K):
    """Host arrays of one (N, K): S (softmax, one-hot leaf rows), M, and --
    where K % 4 == 0 -- the pre-split operands and leaf codes as the library
    itself writes them (trex_tree_split_x3, trex_tree_leaf_codes)."""
    if (N, K) in _CASES:
        return _CASES[(N, K)]
    Q = 5 if K % 4 else 4
    L = K // Q
    rng = np.random.default_rng(1000 * N + K)
    nl = (N + 1) // 2
    x = rng.normal(size=(N, L, Q)) * 3
    S = np.exp(x - x.max(-1, keepdims=True))
    S /= S.sum(-1, keepdims=True)
    S[:nl] = np.eye(Q)[rng.integers(0, Q, size=(nl, L))]
    S = S.reshape(N, K).astype(np.float32)
    M = (rng.normal(size=(N, N)) * 20).astype(np.float32)
    c = dict(S=S, M=M, nl=nl, L=L, Q=Q, mm=1.01 * float(np.abs(M).max()), ldm=32 * ((N + 31) // 32),
             lcr=int(lib().trex_tree_leaf_code_rows(nl)), S16=None, M16=None, codes=None)
    if K % 4 == 0:
        st = stream_handle(torch.device(device))
        Sd, Md = _t(S, device), _t(M, device)
        S16 = torch.empty((N, K), dtype=torch.int32, device=device)
        M16 = torch.empty((N, c["ldm"]), dtype=torch.int32, device=device)
        check(lib().trex_tree_split_x3(ptr(Sd), N, K, K, 1.0, ptr(S16), K, st))
        check(lib().trex_tree_split_x3(ptr(Md), N, N, N, c["mm"], ptr(M16), c["ldm"], st))
        c["S16"], c["M16"] = S16.cpu().numpy(), M16.cpu().numpy()
        if c["lcr"] > 0:
            cb = torch.empty(int(lib().trex_tree_leaf_codes_bytes(nl, L)), dtype=torch.uint8,
                             device=device)
            status = torch.zeros(1, dtype=torch.int32, device=device)
            check(lib().trex_tree_leaf_codes(ptr(Sd), nl, L, 4, ptr(cb), cb.numel(), ptr(status),
                                             st))
            assert int(status.item()) == 0
            c["codes"] = cb.cpu().numpy()
    _CASES[(N, K)] = c
    return c


def _protocol(device, call):
    return G.protocol(device, W.plain(device, call), call)


@pytest.mark.parametrize("N,K,skip,row0", GEMM + GRAM_ONLY + RAGGED,
                         ids=[_sid(c) for c in GEMM + GRAM_ONLY + RAGGED])
def test_gram_f32(device, gram_version, N, K, skip, row0):
    c = gemm_case(device, N, K)
    _protocol(device, lambda run: W.tree_gram(run, c["S"]))
    _protocol(device, lambda run: W.tree_gram(run, c["S"], skip=skip))


@pytest.mark.parametrize("N,K,skip,row0", GEMM + GRAM_ONLY + RAGGED,
                         ids=[_sid(c) for c in GEMM + GRAM_ONLY + RAGGED])
def test_gram_x3(device, gram_version, N, K, skip, row0):
    c = gemm_case(device, N, K)
    if K % 4:
        _protocol(device, lambda run: W.tree_gram(run, c["S"], skip=skip, max_abs=1.0,
                                                  refuse=W.E_UNSUPPORTED))
        _protocol(device, lambda run: W.tree_gram_x3p(run, c["S"].view(np.int32), skip, 1.0,
                                                      refuse=W.E_ARG))
        return
    _protocol(device, lambda run: W.tree_gram(run, c["S"], skip=skip, max_abs=1.0))
    _protocol(device, lambda run: W.tree_gram_x3p(run, c["S16"], skip, 1.0))
    if c["lcr"] > 0:
        _protocol(device, lambda run: W.tree_gram_x3p(run, c["S16"], skip, 1.0, codes=c["codes"],
                                                      n_leaf=c["nl"]))
    else:  # n_leaf < 32: no code rows, refused
        _protocol(device, lambda run: W.tree_gram_x3p(
            run, c["S16"], skip, 1.0, codes=np.zeros(c["L"], np.uint8), n_leaf=c["nl"],
            refuse=W.E_ARG))


@pytest.mark.parametrize("N,row0", [(97, 64), (130, 64), (97, 37), (33, 0), (64, 64)],
                         ids=lambda v: str(v))
def test_gram_mirror(device, N, row0):
    Gm = _f32(np.random.default_rng(N + row0), N, N)
    _protocol(device, lambda run: W.tree_gram_mirror(run, Gm, row0))


@pytest.mark.parametrize("N,K,skip,row0", GEMM + RAGGED, ids=[_sid(c) for c in GEMM + RAGGED])
def test_mf_f32(device, gram_version, N, K, skip, row0):
    c = gemm_case(device, N, K)
    _protocol(device, lambda run: W.tree_mf(run, c["M"], c["S"]))
    _protocol(device, lambda run: W.tree_mf_rows(run, c["M"], c["S"], row0, N - row0))


@pytest.mark.parametrize("N,K,skip,row0", GEMM + RAGGED, ids=[_sid(c) for c in GEMM + RAGGED])
def test_mf_x3(device, gram_version, N, K, skip, row0):
    c = gemm_case(device, N, K)
    nr, mx = N - row0, (c["mm"], 1.0)
    if K % 4:
        _protocol(device, lambda run: W.tree_mf_rows(run, c["M"], c["S"], row0, nr, max_abs=mx,
                                                     refuse=W.E_UNSUPPORTED))
        M16 = np.zeros((N, c["ldm"]), np.int32)
        _protocol(device, lambda run: W.tree_mf_rows_x3p(run, M16, c["S"].view(np.int32), row0, nr,
                                                         mx, refuse=W.E_ARG))
        return
    _protocol(device, lambda run: W.tree_mf_rows(run, c["M"], c["S"], row0, nr, max_abs=mx))
    _protocol(device, lambda run: W.tree_mf_rows_x3p(run, c["M16"], c["S16"], row0, nr, mx))
    if c["lcr"] > 0:
        kw = dict(codes=c["codes"], n_leaf=c["nl"])
        _protocol(device, lambda run: W.tree_mf_rows(run, c["M"], c["S"], row0, nr, max_abs=mx,
                                                     **kw))
        _protocol(device, lambda run: W.tree_mf_rows_x3p(run, c["M16"], c["S16"], row0, nr, mx,
                                                         **kw))
    else:  # n_leaf < 32: no code rows, refused
        kw = dict(codes=np.zeros(c["L"], np.uint8), n_leaf=c["nl"], refuse=W.E_ARG)
        _protocol(device, lambda run: W.tree_mf_rows(run, c["M"], c["S"], row0, nr, max_abs=mx,
                                                     **kw))
        _protocol(device, lambda run: W.tree_mf_rows_x3p(run, c["M16"], c["S16"], row0, nr, mx,
                                                         **kw))


@pytest.mark.parametrize("N,K,skip,row0", GEMM, ids=[_sid(c) for c in GEMM])
def test_split_x3(device, N, K, skip, row0):
    """M: cols = N, ldo = 32 ceil(N / 32) (the groups past N are the kernel's
    to zero); S: ldo = K.  == the operands gemm_case holds (R0)."""
    c = gemm_case(device, N, K)
    out = _protocol(device, lambda run: W.tree_split_x3(run, c["M"], N, c["mm"], c["ldm"]))["out"]
    assert np.array_equal(out.numpy(), c["M16"])
    pad = out.numpy().reshape(N, c["ldm"] // 4, 4)[:, (N + 3) // 4:]
    assert not pad.any()  # whole groups past cols: zero
    out = _protocol(device, lambda run: W.tree_split_x3(run, c["S"], K, 1.0, K))["out"]
    assert np.array_equal(out.numpy(), c["S16"])


@pytest.mark.parametrize("N,K,skip,row0", GEMM, ids=[_sid(c) for c in GEMM])
def test_leaf_codes(device, N, K, skip, row0):
    c = gemm_case(device, N, K)
    refuse = None if c["lcr"] > 0 else W.E_ARG
    out = _protocol(device, lambda run: W.tree_leaf_codes(run, c["S"], c["nl"], c["L"], 4,
                                                          refuse=refuse))
    if refuse is None:
        assert int(out["status"][0]) == 0 and np.array_equal(out["codes"].numpy(), c["codes"])


# ---------------------------------------------------------------------------
# surrogate, constraint, costs
# ---------------------------------------------------------------------------
def _SA(N, K, seed=0):
    rng = np.random.default_rng(seed + 31 * N + K)
    return rng.random((N, K)).astype(np.float32), rng.random((N, N)).astype(np.float32)


# inside the one-launch small path (N <= 64 and N K <= 4096) and one step outside each limit
@pytest.mark.parametrize("grads", [True, False], ids=["grads", "loss"])
@pytest.mark.parametrize("N,K", [(7, 12), (64, 64), (65, 12), (64, 68)],
                         ids=lambda v: str(v))
def test_surrogate(device, N, K, grads):
    S, A = _SA(N, K)

    def r0():
        if not grads:
            return dict(loss=TR.compute_surrogate_cost(_t(S, device), _t(A, device)))
        loss, dS, dA = TR.surrogate_cost_and_grads(_t(S, device), _t(A, device))
        return dict(loss=loss, dS=dS, dA=dA)

    G.protocol(device, r0, lambda run: W.tree_surrogate(run, S, A, grads=grads))


def _gram_of(S):
    return (S.astype(np.float64) @ S.astype(np.float64).T).astype(np.float32)


@pytest.mark.parametrize("N", [7, 97])
def test_surrogate_combine(device, N):
    S, A = _SA(N, 12)
    Gm = _gram_of(S)
    _protocol(device, lambda run: W.tree_surrogate_combine(run, A, Gm))


@pytest.mark.parametrize("m16", [False, True], ids=["m16null", "m16"])
@pytest.mark.parametrize("state", [False, True], ids=["host", "state"])
@pytest.mark.parametrize("N", [7, 97])
def test_surrogate_constraint(device, N, state, m16):
    S, A = _SA(N, 12)
    Gm = _gram_of(S)
    st = W.step_state(3, 0.271, 0.003, 0.7, 0.6) if state else None
    ldm = 32 * ((N + 31) // 32) if m16 else 0
    _protocol(device, lambda run: W.tree_surrogate_constraint(
        run, A, Gm, 10.0, 0.7, state=st, max_abs_m=float(N + 1), ldm16=ldm))


@pytest.mark.parametrize("dA", [False, True], ids=["dAnull", "dA"])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("N", [3, 7, 97])
def test_constraint(device, N, dev, acc, dA):
    rng = np.random.default_rng(N)
    A = rng.random((N, N)).astype(np.float32)
    st = W.step_state(3, 0.271, 0.003, 0.7, 0.6) if dev else None
    kw = dict(loss0=np.array([1.5], np.float32) if acc else None,
              dA0=_f32(rng, N, N) if dA else None, state=st)
    call = lambda run: W.tree_constraint(run, A, 10.0, 1.0, **kw)  # noqa: E731
    if not (dev or acc or dA):  # the Python wrapper's call
        G.protocol(device, lambda: dict(loss=TR.enforce_graph_constraints(_t(A, device), 10.0)),
                   call)
    else:
        _protocol(device, call)


def _SAC(N, L, Q):
    rng = np.random.default_rng(N + L + Q)
    return (rng.random((N, L, Q)).astype(np.float32), rng.random((N, N)).astype(np.float32), rng)


@pytest.mark.parametrize("ckind", [0, 1, 2])
@pytest.mark.parametrize("N,L,Q", [(7, 5, 3), (33, 17, 4)], ids=lambda v: str(v))
def test_soft_cost(device, N, L, Q, ckind):
    S, A, rng = _SAC(N, L, Q)
    C = {0: None, 1: rng.random(Q).astype(np.float32),
         2: rng.random((Q, Q)).astype(np.float32)}[ckind]
    r0 = lambda: dict(loss=TR.compute_soft_cost(  # noqa: E731
        _t(S, device), _t(A, device), None if C is None else _t(C, device)))
    G.protocol(device, r0, lambda run: W.tree_soft_cost(run, S, A, C, ckind))


@pytest.mark.parametrize("N,L,Q", [(7, 5, 3), (33, 17, 4)], ids=lambda v: str(v))
def test_compute_cost(device, N, L, Q):
    S, A, rng = _SAC(N, L, Q)
    C = rng.integers(0, 5, size=(Q, Q)).astype(np.float32)
    r0 = lambda: dict(cost=TR.compute_cost(_t(S, device), _t(A, device), _t(C, device)))  # noqa
    G.protocol(device, r0, lambda run: W.tree_compute_cost(run, S, A, C))


def test_discretize(device):
    for nrows, ncols, n_nodes in ((3, 3, 3), (33, 33, 33), (7, 5, 9)):
        A = np.random.default_rng(nrows).random((nrows, ncols)).astype(np.float32)
        r0 = lambda: dict(out=TR.discretize_tree_topology(_t(A, device), n_nodes))  # noqa: E731
        G.protocol(device, r0, lambda run: W.tree_discretize(run, A, n_nodes))


# ---------------------------------------------------------------------------
# update_tree / update_seq and their VJPs
# ---------------------------------------------------------------------------
def _tree_inputs(nl):
    N, n_anc = 2 * nl - 1, nl - 1
    rng = np.random.default_rng(nl)
    theta = _f32(rng, N - 1, n_anc)
    noise = rng.gumbel(size=(N - 1, n_anc)).astype(np.float32)
    gates = rng.random((N - 1, n_anc)).astype(np.float32)
    A = rng.random((N, N)).astype(np.float32)
    A /= A.sum(1, keepdims=True)
    return N, n_anc, theta, noise, gates, A, _f32(rng, N, N), rng


@pytest.mark.parametrize("gates", [False, True], ids=["gnull", "gates"])
@pytest.mark.parametrize("noise", [False, True], ids=["nnull", "noise"])
@pytest.mark.parametrize("nl", [2, 4, 33])
def test_update_tree(device, nl, noise, gates):
    N, n_anc, theta, nz, gt, _, _, _ = _tree_inputs(nl)
    nz, gt = (nz if noise else None), (gt if gates else None)
    r0 = lambda: dict(A=TR.update_tree(None if nz is None else _t(nz, device),  # noqa: E731
                                       {"tree_params": _t(theta, device)}, 0.7,
                                       None if gt is None else _t(gt, device)))
    G.protocol(device, r0, lambda run: W.tree_update_tree(run, theta, nz, gt, 0.7))


@pytest.mark.parametrize("gates", [False, True], ids=["gnull", "gates"])
@pytest.mark.parametrize("nl", [2, 4, 33])
def test_update_tree_bwd(device, nl, gates):
    N, n_anc, _, _, gt, A, dA, _ = _tree_inputs(nl)
    _protocol(device, lambda run: W.tree_update_tree_bwd(run, A, dA, gt if gates else None, n_anc,
                                                         0.7))


@pytest.mark.parametrize("state", [False, True], ids=["host", "state"])
@pytest.mark.parametrize("dtheta", [False, True], ids=["dthnull", "dtheta"])
@pytest.mark.parametrize("gates", [False, True], ids=["gnull", "gates"])
@pytest.mark.parametrize("nl", [2, 4, 33])
def test_update_tree_bwd_adam(device, nl, gates, dtheta, state):
    N, n_anc, theta, _, gt, A, dA, rng = _tree_inputs(nl)
    mu, nu = 0.1 * _f32(rng, N - 1, n_anc), 0.01 * rng.random((N - 1, n_anc)).astype(np.float32)
    st = W.step_state(3, 0.271, 0.003, 0.7, 0.6) if state else None
    _protocol(device, lambda run: W.tree_update_tree_bwd_adam(
        run, A, dA, gt if gates else None, n_anc, 1.0, theta, mu, nu, dtheta=dtheta, count=3,
        state=st))


SEQ = [(1, 1, 2), (3, 33, 5), (16, 67, 4)]


def _seq_inputs(n_anc, L, Q):
    rng = np.random.default_rng(n_anc + L + Q)
    x = _f32(rng, n_anc, L, Q)
    s = np.exp(0.7 * x - (0.7 * x).max(-1, keepdims=True))
    s = (s / s.sum(-1, keepdims=True)).astype(np.float32)
    mu, nu = 0.1 * _f32(rng, n_anc, L, Q), 0.01 * rng.random((n_anc, L, Q)).astype(np.float32)
    return x, s, _f32(rng, n_anc, L, Q), mu, nu


@pytest.mark.parametrize("n_anc,L,Q", SEQ, ids=lambda v: str(v))
def test_update_seq(device, n_anc, L, Q):
    x, s, ds, _, _ = _seq_inputs(n_anc, L, Q)
    S0 = np.zeros((2 * n_anc + 1, L, Q), np.float32)
    r0 = lambda: dict(s_anc=TR.update_seq({"ancestors": _t(x, device)}, _t(S0, device),  # noqa
                                          0.7)[n_anc + 1:])
    G.protocol(device, r0, lambda run: W.tree_update_seq(run, x, 0.7))
    _protocol(device, lambda run: W.tree_update_seq_bwd(run, s, ds, 0.7))


# ---------------------------------------------------------------------------
# optimiser kernels
# ---------------------------------------------------------------------------
def _opt_inputs(n, n_parts):
    rng = np.random.default_rng(n + n_parts)
    p, g = _f32(rng, n), _f32(rng, n)
    mu, nu = 0.1 * _f32(rng, n), 0.01 * rng.random(n).astype(np.float32)
    parts = rng.random(n_parts) * 4.0 / n_parts if n_parts else None  # norm ~ 1.4 > clip 1
    return p, g, mu, nu, parts


STATE = W.step_state(3, 0.271, 0.002997, 0.7, 0.6)  # count 3: 1 - 0.9^3, 1 - 0.999^3


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("n_parts", [0, 512, 1024])
@pytest.mark.parametrize("n", [1, 3, 1025])
def test_adam_step(device, n, n_parts, dev):
    p, g, mu, nu, parts = _opt_inputs(n, n_parts)
    _protocol(device, lambda run: W.adam_step(run, p, g, mu, nu, count=3,
                                              state=STATE if dev else None, parts=parts, clip=1.0))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("n_parts", [0, 512, 1024])
@pytest.mark.parametrize("n", [1, 3, 1025])
@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=["adam", "adamw", "sgd", "rmsprop"])
def test_optax_step(device, kind, n, n_parts, dev):
    p, g, s1, s2, parts = _opt_inputs(n, n_parts)
    _protocol(device, lambda run: W.optax_step(run, kind, p, g, s1, s2, count=3,
                                               state=STATE if dev else None, parts=parts,
                                               clip=1.0))


@pytest.mark.parametrize("n", [1, 511, 513, 4099])
def test_sq_norm_parts(device, n):
    """Every one of the 512 parts is written (R1 == R2), also with n < 512."""
    x = _f32(np.random.default_rng(n), n)
    out = _protocol(device, lambda run: W.sq_norm_parts(run, x, 512))["parts"]
    np.testing.assert_allclose(float(out.sum()), float((x.astype(np.float64) ** 2).sum()),
                               rtol=1e-12)


@pytest.mark.parametrize("grads_out", [False, True], ids=["gonull", "go"])
@pytest.mark.parametrize("n_anc,L,Q", SEQ, ids=lambda v: str(v))
def test_adam_seq_step(device, n_anc, L, Q, grads_out):
    x, s, ds, mu, nu = _seq_inputs(n_anc, L, Q)
    _protocol(device, lambda run: W.adam_seq_step(run, s, ds, 0.7, x, mu, nu, count=3,
                                                  grads_out=grads_out))


@pytest.mark.parametrize("entry", ["host", "dev", "x3p", "x3p-state"])
@pytest.mark.parametrize("n_anc,L,Q", SEQ, ids=lambda v: str(v))
def test_adam_seq_update_step(device, n_anc, L, Q, entry):
    x, _, ds, mu, nu = _seq_inputs(n_anc, L, Q)
    if entry in ("host", "dev"):
        _protocol(device, lambda run: W.adam_seq_update_step(
            run, ds, 0.7, 0.6, x, mu, nu, count=3, state=STATE if entry == "dev" else None,
            dev=entry == "dev"))
        return
    st = STATE if entry == "x3p-state" else None
    if Q == 4:
        _protocol(device, lambda run: W.adam_seq_update_step(run, ds, 0.7, 0.6, x, mu, nu, count=3,
                                                             state=st, x3p_max_abs=1.0))
        return

    def refused(run):  # Q != 4: TREX_E_ARG, nothing written (outputs and in/outs kept whole)
        n = (n_anc, L, Q)
        d, s_ = run.input("ds_anc", ds), run.input("state", st)
        p, m, v = (W._io(run, k, a, W.E_ARG) for k, a in (("params", x), ("mu", mu), ("nu", nu)))
        s16 = W._out(run, "s16_next", n, torch.int32, W.E_ARG)
        W._go(run, "trex_adam_seq_update_step_x3p", d, n_anc, L, Q, 0.7, 0.6, p, m, v, 3,
              *W._hyper(), s_, 1.0, s16, refuse=W.E_ARG)

    _protocol(device, refused)


@pytest.mark.parametrize("case", ["notemps", "t1", "t3", "t3-past-the-end"])
def test_step_advance(device, case):
    """temps NULL; 1 and 3 temperatures; a count already past the schedule's
    end (T and Tn clamp to the last entry: no read behind temps, whose R2
    guard is NaN)."""
    temps = {"notemps": None, "t1": np.array([0.9], np.float32)}.get(
        case, np.array([0.9, 0.8, 0.7], np.float32))
    st = W.step_state(5 if case.endswith("end") else 1, 0.1, 0.001, 0.5, 0.4)
    out = _protocol(device, lambda run: W.step_advance(run, st, 0.9, 0.999, temps))["state"]
    assert int(out[0]) == int(st[0]) + 1
    if temps is not None:
        T, Tn = out[3:5].numpy().view(np.float32)
        k = int(out[0])
        assert T == temps[min(k - 1, temps.size - 1)] and Tn == temps[min(k, temps.size - 1)]


@pytest.mark.parametrize("state", [False, True], ids=["stnull", "state"])
@pytest.mark.parametrize("n", [1, 3, 1025])
def test_gumbel_noise(device, n, state):
    call = lambda run: W.gumbel_noise(run, 0x1234ABCD5678, W.step_state(4) if state else None,  # noqa
                                      n)
    if state:
        G.protocol(device, lambda: dict(out=TR.gumbel_noise_step(0x1234ABCD5678, 4, (n,), device)),
                   call)
    else:
        _protocol(device, call)
