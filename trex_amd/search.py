"""Tree search on the Sankoff engine: stepwise-addition starting trees and NNI
hill climbing.

The reference scores one given tree per ``run_sankoff`` call
(src/trex/sankoff.py:114-188) and has no search; this module adds the first
step a parsimony user takes next.  Every round scores all 2 (n_leaves - 2)
NNI neighbours of every tree of the batch from one forward and one outside
pass (``SankoffEngine.nni_scores``, sankoff_nni.hip) instead of one forward
per neighbour.  Stepwise addition scores a new taxon on all 2k - 1 edges of
every k-taxon tree the same way (``SankoffEngine.attach_scores``).
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .sankoff import SankoffEngine, _default_device, _torch
from .topology import TreePlan, apply_nni, insert_leaf, relabel_leaves


@dataclass
class HillClimbResult:
    children: np.ndarray  # (B, n_all, 2) int32: the trees the climb ended on
    scores: np.ndarray  # (B,) float32: their scores (engine forward)
    history: list  # per tree: its score before the first move and after every move
    n_moves: np.ndarray  # (B,) int64: moves applied per tree
    rounds: int  # rounds that moved at least one tree (= n_moves.max())


def nni_hill_climb(children, leaves, cost, *, tau: float = 0.0, min_gain: float = 1e-5,
                   max_rounds: int = 100, device=None) -> HillClimbResult:
    """Steepest-descent NNI search, every tree of the batch on its own.

    children (B, n_all, 2) or (n_all, 2) proper rooted binary trees; leaves
    int8 (B, n_leaves, L) or (n_leaves, L) (shared by all trees); cost (Q, Q).
    Each round scores all neighbours of every tree and takes the lowest (ties:
    the lowest (v, k)); the move is applied only if ``score_new < score -
    min_gain * |score|`` -- relative, and by default the 1e-5 parity bar of
    the kernels, so a gain inside their rounding is never taken.  The plan is
    rebuilt for the batch after every round that moved a tree; the climb stops
    when no tree moves or after ``max_rounds`` rounds of moves.
    """
    torch = _torch()
    device = torch.device(device) if device is not None else _default_device()
    ch = np.array(children, dtype=np.int32, copy=True)
    if ch.ndim == 2:
        ch = ch[None]
    if ch.ndim != 3 or ch.shape[2] != 2:
        raise ValueError(f"children must be (B, n_all, 2), got {ch.shape}")
    B, n_all, _ = ch.shape
    nl = (n_all + 1) // 2
    lv = torch.as_tensor(leaves).to(device=device, dtype=torch.int8)
    if lv.ndim == 2:
        lv = lv[None].expand(B, -1, -1)
    if lv.ndim != 3 or tuple(lv.shape[:2]) != (B, nl):
        raise ValueError(f"leaves must be ({B}, {nl}, L) or ({nl}, L), got {tuple(lv.shape)}")
    lv = lv.contiguous()
    L = int(lv.shape[2])
    c = torch.as_tensor(cost).to(device=device, dtype=torch.float32).contiguous()
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError(f"cost must be (Q, Q), got {tuple(c.shape)}")
    Q = int(c.shape[0])
    if not min_gain >= 0.0:
        raise ValueError("min_gain must be >= 0")

    def forward(ch_now):
        eng = SankoffEngine(TreePlan(ch_now), L, Q, device)
        return eng, eng.forward(lv, c, tau)

    history = [[] for _ in range(B)]
    n_moves = np.zeros(B, dtype=np.int64)
    rounds = 0
    eng, f = forward(ch)
    score = f.tree_score.cpu().numpy()
    for b in range(B):
        history[b].append(float(score[b]))
    while rounds < max_rounds:
        nb =eng.nni_scores(lv, c, tau, dp=f.dp).cpu().numpy().reshape(B, -1)
        best = nb.argmin(axis=1)  # first minimum: the lowest (v, k)
        moved = []
        for b in range(B):
            new = float(nb[b, best[b]])
            cur = float(score[b])
            if new < cur - min_gain * abs(cur):
                ch[b] = apply_nni(ch[b], nl + int(best[b]) // 2, int(best[b]) % 2)
                moved.append(b)
        if not moved:
            break
        rounds += 1
        eng, f = forward(ch)
        score = f.tree_score.cpu().numpy()
        for b in moved:
            n_moves[b] += 1
            history[b].append(float(score[b]))
    return HillClimbResult(ch, score.astype(np.float32), history, n_moves, rounds)


@dataclass
class StepwiseResult:
    children: np.ndarray  # (B, 2n - 1, 2) int32: one tree per addition sequence
    scores: np.ndarray  # (B,) float32: their scores (engine forward)
    order: np.ndarray  # (B, n) int64: the addition sequences


@dataclass
class SearchResult(HillClimbResult):
    start_scores: np.ndarray  # (B,) float32: the stepwise-addition trees' scores
    order: np.ndarray  # (B, n) int64: their addition sequences


# the three rooted trees on leaves 0, 1, 2: ((0, 1), 2), ((0, 2), 1), ((1, 2), 0)
_TRIPLETS = np.array([[[-1, -1]] * 3 + [[a, b], [c, 3]] for a, b, c in
                      ((0, 1, 2), (0, 2, 1), (1, 2, 0))], dtype=np.int32)


def stepwise_addition(leaves, cost, *, order=None, n_trees: int = 1, seed: int = 0,
                      tau: float = 0.0, device=None) -> StepwiseResult:
    """Starting trees by stepwise addition, B addition sequences in one batch.

    leaves int8 (n, L), one alignment of n >= 3 taxa; cost (Q, Q), Q <= 20.
    ``order`` (B, n): each row a permutation of the taxa, the sequence in
    which tree b takes them; ``order=None``: tree 0 takes the taxa as given,
    trees 1 .. n_trees - 1 permutations drawn from
    ``np.random.default_rng(seed)``.  Every sequence starts from the lowest
    scoring of the three rooted trees on its first three taxa (one forward;
    ties: the lowest index of ((0, 1), 2), ((0, 2), 1), ((1, 2), 0)).  Taxon k
    = 3 .. n - 1 then goes on the edge where ``SankoffEngine.attach_scores``
    is lowest (ties: the lowest node id) by ``insert_leaf``: one plan, one
    forward, one outside pass and one scoring pass per step for the whole
    batch.  The trees are returned with the alignment's taxon ids.
    """
    torch = _torch()
    device = torch.device(device) if device is not None else _default_device()
    lv = torch.as_tensor(leaves).to(device=device, dtype=torch.int8)
    if lv.ndim != 2 or lv.shape[0] < 3:
        raise ValueError(f"leaves must be (n >= 3, L), got {tuple(lv.shape)}")
    lv = lv.contiguous()
    n, L = int(lv.shape[0]), int(lv.shape[1])
    c = torch.as_tensor(cost).to(device=device, dtype=torch.float32).contiguous()
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError(f"cost must be (Q, Q), got {tuple(c.shape)}")
    Q = int(c.shape[0])
    if order is None:
        if n_trees < 1:
            raise ValueError("n_trees must be >= 1")
        rng = np.random.default_rng(seed)
        order = np.stack([np.arange(n)] + [rng.permutation(n) for _ in range(n_trees - 1)])
    order = np.asarray(order)
    if order.ndim != 2 or order.shape[1] != n or order.shape[0] < 1:
        raise ValueError(f"order must be (B, {n}), got {order.shape}")
    if not (np.sort(order, axis=1) == np.arange(n)[None, :]).all():
        raise ValueError(f"every row of order must be a permutation of 0..{n - 1}")
    order = order.astype(np.int64)
    B = order.shape[0]
    taxa = lv[torch.from_numpy(order).to(device)]  # (B, n, L): tree b's taxa in its sequence

    def engine(ch_now):
        return SankoffEngine(TreePlan(ch_now), L, Q, device)

    first = taxa[:, :3].repeat_interleave(3, dim=0).contiguous()
    ts = engine(np.tile(_TRIPLETS, (B, 1, 1))).forward(first, c, tau).tree_score
    pick = ts.cpu().numpy().reshape(B, 3).argmin(axis=1)  # first minimum
    ch = [_TRIPLETS[i] for i in pick]
    for k in range(3, n):
        eng = engine(np.stack(ch))
        sc = eng.attach_scores(taxa[:, :k].contiguous(), c, tau,
                               new_leaf=taxa[:, k].contiguous())
        where = sc.cpu().numpy().argmin(axis=1)  # first minimum: the lowest node id
        ch = [insert_leaf(ch[b], int(where[b])) for b in range(B)]
    out = np.stack([relabel_leaves(ch[b], order[b]) for b in range(B)])
    shared = lv[None].expand(B, -1, -1).contiguous()
    scores = engine(out).forward(shared, c, tau).tree_score.cpu().numpy()
    return StepwiseResult(out, scores.astype(np.float32), order)


def parsimony_search(leaves, cost, *, n_trees: int, seed: int = 0, tau: float = 0.0,
                     min_gain: float = 1e-5, max_rounds: int = 100, device=None) -> SearchResult:
    """``stepwise_addition`` over ``n_trees`` addition sequences, then
    ``nni_hill_climb`` on its trees."""
    start = stepwise_addition(leaves, cost, n_trees=n_trees, seed=seed, tau=tau, device=device)
    r = nni_hill_climb(start.children, leaves, cost, tau=tau, min_gain=min_gain,
                       max_rounds=max_rounds, device=device)
    return SearchResult(r.children, r.scores, r.history, r.n_moves, r.rounds, start.scores,
                        start.order)
