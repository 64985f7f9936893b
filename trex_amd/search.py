"""Tree search on the Sankoff engine: NNI hill climbing.

The reference scores one given tree per ``run_sankoff`` call
(src/trex/sankoff.py:114-188) and has no search; this module adds the first
step a parsimony user takes next.  Every round scores all 2 (n_leaves - 2)
NNI neighbours of every tree of the batch from one forward and one outside
pass (``SankoffEngine.nni_scores``, sankoff_nni.hip) instead of one forward
per neighbour.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .sankoff import SankoffEngine, _default_device, _torch
from .topology import TreePlan, apply_nni


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
