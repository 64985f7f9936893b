"""Guard-band tests: the NK and datagen kernels stay inside their buffers
("Memory contract"; harness in tests/_guard.py, wrappers in
tests/_guard_tree.py, the protocol as in tests/test_guard_tree_gpu.py).  No
oracle and no tolerance: values are pinned by tests/test_nk_gpu.py and
tests/test_datagen_gpu.py.

The NK plan and ``interactions`` are int32 inputs whose R2 guards read as -1:
an index read past either would turn into an out-of-range gather.  The
landscape loss runs on a workspace of exactly ``trex_nk_workspace_bytes``.

Entry point -> test ids ((Q, k, R, L) / (n_leaves, L, Q, k)):

    trex_nk_parental_logits          test_parental_logits[<Q>-<k>-<R>-<L>]: rows unsorted, one
                                     duplicate.  (4, 2, 7, 33), (2, 6, 3, 40) register kernel;
                                     (4, 4, 3, 5), (2, 10, 5, 15) per-pair kernel; (3, 2, 5, 9)
                                     rolled generic; (20, 2, 5, 9) wide alphabet; (4, 0, 3, 7) k = 0
    trex_nk_landscape_loss           test_landscape_loss[<case>]:
      eval                           (32, 15, 2, 10); R0 LandscapeAwareLoss
      v4, v4-nograd, v4-generic,     (4, 33, 4, 2), seq_mask with zeros, root with parent =
      v4-rolled                      self; d_S / d_S_in NULL (nograd); TREX_NK_V4=0 (generic);
                                     TREX_NK_REG=0 (rolled); R0 LandscapeAwareLoss
      q3                             (4, 9, 3, 2), d_S_in NULL with d_S given; R0 the ABI call
      k0                             (4, 7, 4, 0), seq_mask with zeros; R0 the ABI call
      chunks                         (65, 130, 4, 1): n_parents L > 8192, two-level chunk sum
    trex_datagen_groundtruth         test_groundtruth[...], exact workspace
    trex_datagen_uniform_states      test_uniform_states[<n>]
    trex_datagen_nk_tree             test_nk_tree: 7 nodes, an unfilled BFS slot (node 6
                                     repeated), seqs in/out with the root row kept

What the three guard files leave out, and why: the end of
tests/test_guard_tree_gpu.py's table.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _guard as G
import _guard_tree as W
from oracle import nk_ref as nk
from trex_amd import datagen as DG
from trex_amd import nk as NK
from trex_amd._lib import check, lib, ptr

pytestmark = pytest.mark.gpu


def _protocol(device, call):
    return G.protocol(device, W.plain(device, call), call)


# ---------------------------------------------------------------------------
# NK
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Q,k,R,L", [(4, 2, 7, 33), (2, 6, 3, 40), (4, 4, 3, 5), (2, 10, 5, 15),
                                     (3, 2, 5, 9), (20, 2, 5, 9), (4, 0, 3, 7)],
                         ids=lambda v: str(v))
def test_parental_logits(device, Q, k, R, L):
    rng = np.random.default_rng(100 * Q + k)
    if k:
        inter, F = nk.random_landscape(L, k, Q, seed=k)
    else:
        inter, F = np.zeros((L, 0), np.int32), rng.uniform(size=(L, Q)).astype(np.float32)
    inter, F = np.asarray(inter, np.int32), np.asarray(F, np.float32)
    N = R + 2
    S = rng.dirichlet(np.ones(Q), size=(N, L)).astype(np.float32)
    rows = rng.permutation(N)[:R].astype(np.int32)  # unsorted ...
    if R > 1:
        rows[-1] = rows[0]  # ... with one duplicate
    if R > 2 and np.all(np.diff(rows[:-1]) > 0):
        rows[:2] = rows[1::-1].copy()
    land = NK.NKLandscape(inter, F, Q, device)
    r0 = lambda: dict(logits=NK.compute_parental_logits(  # noqa: E731
        torch.as_tensor(S[rows], device=device), land, k))
    G.protocol(device, r0, lambda run: W.nk_parental_logits(run, S, rows, inter, k, F))


def _case(n_leaves, L, Q, k, seed, mask=False, root_self=False):
    """tests/test_nk_gpu.py's balanced-tree case."""
    rng = np.random.default_rng(seed)
    n_all = 2 * n_leaves - 1
    if k:
        inter, F = nk.random_landscape(L, k, Q, seed=seed + 1)
    else:
        inter, F = np.zeros((L, 0), np.int32), rng.uniform(size=(L, Q)).astype(np.float32)
    leaves = rng.integers(0, Q, size=(n_leaves, L))
    A = np.zeros((n_all, n_all), np.float32)
    A[np.arange(n_all - 1), n_leaves + np.arange(n_all - 1) // 2] = 1.0
    if root_self:
        A[-1, -1] = 1.0
    anc = rng.normal(size=(n_all - n_leaves, L, Q)).astype(np.float32)
    m = None
    if mask:
        m = (rng.random(L) > 0.25).astype(np.float32)
        m[1] = 0.0
    S0 = np.zeros((n_all, L, Q), np.float32)
    S0[np.arange(n_leaves)[:, None], np.arange(L)[None, :], leaves] = 1.0
    return dict(S0=S0, A=A, inter=np.asarray(inter, np.int32), F=np.asarray(F, np.float32), anc=anc,
                mask=m, rng=rng)


# case -> (n_leaves, L, Q, k, mask, root_self, env, r0 kind, d_S, d_S_in)
LOSS = {
    "eval": (32, 15, 2, 10, False, False, {}, "class", True, True),
    "v4": (4, 33, 4, 2, True, True, {}, "class", True, True),
    "v4-nograd": (4, 33, 4, 2, True, True, {}, "class", False, False),
    "v4-generic": (4, 33, 4, 2, True, True, {"TREX_NK_V4": "0"}, "class", True, True),
    "v4-rolled": (4, 33, 4, 2, True, True, {"TREX_NK_REG": "0"}, "class", True, True),
    "q3": (4, 9, 3, 2, False, False, {}, "abi", True, False),
    "k0": (4, 7, 4, 0, True, False, {}, "abi", True, True),
    "chunks": (65, 130, 4, 1, False, False, {}, "class", True, True),
}


@pytest.mark.parametrize("case", list(LOSS))
def test_landscape_loss(device, monkeypatch, case):
    n_leaves, L, Q, k, mask, root_self, env, kind, want_dS, want_in = LOSS[case]
    for key in ("TREX_NK_V4", "TREX_NK_REG", "TREX_NK_PP", "TREX_NK_SPLIT", "TREX_NK_X3"):
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    c = _case(n_leaves, L, Q, k, seed=L + Q, mask=mask, root_self=root_self)
    N, lam = c["S0"].shape[0], 0.8
    if kind == "class":
        # R0: LandscapeAwareLoss's own call, on its own buffers; R1 / R2 get
        # the operands it passed (S after update_seq, its surrogate and the
        # surrogate's dS)
        land = NK.NKLandscape(c["inter"], c["F"], Q, device)
        fn = NK.LandscapeAwareLoss(c["A"], n_leaves, land, lam, k, seq_mask=c["mask"])
        assert fn.fitness_on
        fn.value_and_grad(torch.as_tensor(c["anc"], device=device),
                          torch.as_tensor(c["S0"], device=device), want_grad=want_dS)
        torch.cuda.synchronize()
        plan, n_parents, n_nonroot = fn.plan.cpu().numpy(), fn.n_parents, fn.n_nonroot
        S, sur = fn.S.cpu().numpy(), fn.sur.cpu().numpy()
        d_in = fn.dS_sur.cpu().numpy() if want_in else None
        r0 = lambda: dict(loss=fn.loss, d_S=fn.dS if want_dS else None)  # noqa: E731
    else:
        parent = np.argmax(c["A"], axis=1).astype(np.int32)
        plan = np.zeros(int(lib().trex_nk_plan_ints(N, L, k)), np.int32)
        info = np.zeros(2, np.int32)
        check(lib().trex_nk_plan_build(ptr(parent), N, ptr(c["inter"]), L, k, ptr(plan), ptr(info)))
        n_parents, n_nonroot = int(info[0]), int(info[1])
        S = c["S0"].copy()
        x = c["anc"].astype(np.float64)
        e = np.exp(x - x.max(-1, keepdims=True))
        S[n_leaves:] = (e / e.sum(-1, keepdims=True)).astype(np.float32)
        sur = np.array([1.25], np.float32)
        d_in = c["rng"].normal(size=S.shape).astype(np.float32) if want_in else None
        r0 = None
    if root_self:
        assert n_nonroot == N - 1  # the root is its own parent

    def call(run):
        W.nk_landscape_loss(run, plan, n_parents, n_nonroot, S, c["inter"], k, c["F"], c["mask"],
                            lam, sur, d_S_in=d_in, d_S=want_dS)

    G.protocol(device, r0 or W.plain(device, call), call)


# ---------------------------------------------------------------------------
# datagen
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nl,L,Q,mut", [(8, 33, 4, 5), (16, 67, 20, 3)], ids=lambda v: str(v))
def test_groundtruth(device, nl, L, Q, mut):
    r0 = lambda: dict(seqs=DG.generate_groundtruth_device(nl, Q, mut, L, seed=11,  # noqa: E731
                                                          device=device)[0])
    G.protocol(device, r0, lambda run: W.datagen_groundtruth(run, 11, nl, L, Q, mut))


@pytest.mark.parametrize("n", [1, 3, 1001])
def test_uniform_states(device, n):
    r0 = lambda: dict(out=DG.uniform_states_device((n,), 4, seed=5, device=device))  # noqa: E731
    G.protocol(device, r0, lambda run: W.datagen_uniform_states(run, 5, n, 4))


def nk_tree_adjacency():
    """7 nodes, root 0 (its own parent), internal 1 and 2, leaves 3 .. 6; the
    edge of leaf 5 has weight 0.5: argmax still names its parent, but the
    reference's BFS (children = entries equal to 1) never reaches it, so one
    slot of the order stays unfilled and reads as node 6."""
    A = np.zeros((7, 7), np.float32)
    A[0, 0] = 1.0
    for child, par in ((1, 0), (2, 0), (3, 1), (4, 1), (5, 2), (6, 2)):
        A[child, par] = 1.0
    A[5, 2] = 0.5
    return A


def test_nk_tree(device):
    L, Q, K, bl = 33, 2, 2, 3
    A = nk_tree_adjacency()
    root, parent, order, offsets = DG.bfs_levels(A)
    assert root == 0 and list(order).count(6) == 2 and 5 not in order  # the unfilled slot
    land = DG.create_nk_model_landscape(L, K, seed=3, n_states=Q)
    inter = np.asarray(land["interactions"], np.int32)
    F = np.asarray(land["fitness_tables"], np.float32)
    root_seq = np.random.default_rng(4).integers(0, Q, size=L).astype(np.int8)
    seqs0 = np.zeros((7, L), np.int8)
    seqs0[root] = root_seq
    r0 = lambda: dict(seqs=DG.generate_tree_data_device(  # noqa: E731
        land, A, root_seq, 0.3, seed=9, coupled_mutation_prob=0.5, n_states=Q,
        mutation_rate_noise_std=0.2, branch_length=bl, device=device))
    out = G.protocol(device, r0, lambda run: W.datagen_nk_tree(
        run, 9, Q, inter, F, parent, order, offsets, root, seqs0, 0.3, 0.2, 0.5, bl))["seqs"]
    assert not out[5].any()  # never reached: the caller's zeros
