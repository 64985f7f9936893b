"""Tree search on the Sankoff engine: stepwise-addition starting trees, NNI and
SPR hill climbing.

The reference scores one given tree per ``run_sankoff`` call
(src/trex/sankoff.py:114-188) and has no search; this module adds the first
step a parsimony user takes next.  Every round scores all 2 (n_leaves - 2)
NNI neighbours of every tree of the batch from one forward and one outside
pass (``SankoffEngine.nni_scores``, sankoff_nni.hip) instead of one forward
per neighbour.  Stepwise addition scores a new taxon on all 2k - 1 edges of
every k-taxon tree the same way (``SankoffEngine.attach_scores``).

Every search takes a weight per site (DESIGN.md "Site weights"): pattern
counts of a compressed alignment (``compress_sites``), the reweighting of the
parsimony ratchet (``parsimony_ratchet``), bootstrap replicates
(``bootstrap_weights``, ``bootstrap_search``, ``clade_support``).
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .sankoff import SankoffEngine, _default_device, _torch
from .topology import TreePlan, apply_nni, apply_spr, insert_leaf, relabel_leaves


@dataclass
class HillClimbResult:
    children: np.ndarray  # (B, n_all, 2) int32: the trees the climb ended on
    scores: np.ndarray  # (B,) float32: their scores (engine forward)
    history: list  # per tree: its score before the first move and after every move
    n_moves: np.ndarray  # (B,) int64: moves applied per tree
    rounds: int  # rounds that moved at least one tree (= n_moves.max())


def _host_weights(weights, B, L):
    """Host site weights -> float32 (B, L): ``weights`` is (L,), shared by all
    trees, or (B, L); finite and >= 0."""
    w = np.asarray(weights)
    if w.dtype.kind not in "fiub":
        raise ValueError(f"weights must be numbers, got dtype {w.dtype}")
    if w.ndim == 1:
        w = np.broadcast_to(w[None], (B, w.shape[0]))
    if w.shape != (B, L):
        raise ValueError(f"weights must be ({L},) or ({B}, {L}), got {np.shape(weights)}")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("weights must be finite and >= 0")
    return np.ascontiguousarray(w, dtype=np.float32)


def _leaf_tensor(leaves, device):
    """Leaves on the device: int32 input stays int32 (state sets, DESIGN.md
    "State-set leaves"), anything else becomes int8 codes."""
    torch = _torch()
    lv = torch.as_tensor(leaves)
    return lv.to(device=device, dtype=torch.int32 if lv.dtype == torch.int32 else torch.int8)


def _n_sites(leaves):
    return int(leaves.shape[-1] if hasattr(leaves, "shape") else np.shape(leaves)[-1])


def _site_weights(weights, B, L, device):
    """``weights`` of a search function -> contiguous float32 (B, L) tensor on
    ``device``, or None.  numpy (or a list) is validated on the host; a tensor
    is taken as given (its values are not read: nothing synchronises)."""
    if weights is None:
        return None
    torch = _torch()
    if not torch.is_tensor(weights):
        return torch.from_numpy(_host_weights(weights, B, L)).to(device)
    w = weights.to(device=device, dtype=torch.float32)
    if w.ndim == 1:
        w = w[None].expand(B, -1)
    if tuple(w.shape) != (B, L):
        raise ValueError(f"weights must be ({L},) or ({B}, {L}), got {tuple(weights.shape)}")
    return w.contiguous()


def _tree_inputs(children, leaves, cost, device, weights):
    """What a function on a batch of given trees starts with: ``(device, ch
    (B, n_all, 2) int32 copy, leaves (B, n_leaves, L) on the device, cost (Q,
    Q) float32 on the device, weights (B, L) on the device or None)``."""
    torch = _torch()
    device = torch.device(device) if device is not None else _default_device()
    ch = np.array(children, dtype=np.int32, copy=True)
    if ch.ndim == 2:
        ch = ch[None]
    if ch.ndim != 3 or ch.shape[2] != 2:
        raise ValueError(f"children must be (B, n_all, 2), got {ch.shape}")
    B, n_all, _ = ch.shape
    nl = (n_all + 1) // 2
    lv = _leaf_tensor(leaves, device)
    if lv.ndim == 2:
        lv = lv[None].expand(B, -1, -1)
    if lv.ndim != 3 or tuple(lv.shape[:2]) != (B, nl):
        raise ValueError(f"leaves must be ({B}, {nl}, L) or ({nl}, L), got {tuple(lv.shape)}")
    lv = lv.contiguous()
    c = torch.as_tensor(cost).to(device=device, dtype=torch.float32).contiguous()
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError(f"cost must be (Q, Q), got {tuple(c.shape)}")
    return device, ch, lv, c, _site_weights(weights, B, int(lv.shape[2]), device)


def describe_trees(children, leaves, cost, *, tau: float = 0.0, weights=None, device=None):
    """Per-branch change counts and branch lengths of given trees, one call
    from child lists to ``SankoffEngine.edge_changes``' ``EdgeChanges``
    (device tensors indexed by the branch's child node id).  ``children``,
    ``leaves``, ``cost`` and ``weights`` as for ``nni_hill_climb``.  tau = 0:
    the counts follow the engine's own backtrack, and a branch whose
    ``length_max`` is 0 has length 0 in every most-parsimonious reconstruction
    (unsupported: it can be collapsed).  ``topology.to_newick`` writes a tree
    with ``lengths[b]`` on its branches."""
    device, ch, lv, c, w = _tree_inputs(children, leaves, cost, device, weights)
    eng = SankoffEngine(TreePlan(ch), int(lv.shape[2]), int(c.shape[0]), device)
    return eng.edge_changes(lv, c, tau, weights=w)


def _hill_climb(neighbours, apply_move, children, leaves, cost, tau, min_gain, max_rounds, device,
                weights) -> HillClimbResult:
    """The steepest-descent climb ``nni_hill_climb`` and ``spr_hill_climb``
    share.  ``neighbours(eng, leaves, cost, tau, dp, weights)``: the scores of
    every tree's neighbours, (B, ...) with the moves on the trailing axes;
    ``apply_move(children, nl, n_all, i)``: one tree after its move of
    flattened index i."""
    device, ch, lv, c, w = _tree_inputs(children, leaves, cost, device, weights)
    B, n_all, _ = ch.shape
    nl = (n_all + 1) // 2
    L, Q = int(lv.shape[2]), int(c.shape[0])
    if not min_gain >= 0.0:
        raise ValueError("min_gain must be >= 0")

    def forward(ch_now):
        eng = SankoffEngine(TreePlan(ch_now), L, Q, device)
        return eng, eng.forward(lv, c, tau, weights=w)

    history = [[] for _ in range(B)]
    n_moves = np.zeros(B, dtype=np.int64)
    rounds = 0
    eng, f = forward(ch)
    score = f.tree_score.cpu().numpy()
    for b in range(B):
        history[b].append(float(score[b]))
    while rounds < max_rounds:
        nb = neighbours(eng, lv, c, tau, f.dp, w).cpu().numpy().reshape(B, -1)
        best = nb.argmin(axis=1)  # first minimum: the lowest flattened move
        moved = []
        for b in range(B):
            new = float(nb[b, best[b]])
            cur = float(score[b])
            if new < cur - min_gain * abs(cur):
                ch[b] = apply_move(ch[b], nl, n_all, int(best[b]))
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


def nni_hill_climb(children, leaves, cost, *, tau: float = 0.0, min_gain: float = 1e-5,
                   max_rounds: int = 100, device=None, weights=None) -> HillClimbResult:
    """Steepest-descent NNI search, every tree of the batch on its own.

    children (B, n_all, 2) or (n_all, 2) proper rooted binary trees; leaves
    int8 codes or int32 state sets (``encode_alignment``), (B, n_leaves, L) or
    (n_leaves, L) (shared by all trees); cost (Q, Q).
    Each round scores all neighbours of every tree and takes the lowest (ties:
    the lowest (v, k)); the move is applied only if ``score_new < score -
    min_gain * |score|`` -- relative, and by default the 1e-5 parity bar of
    the kernels, so a gain inside their rounding is never taken.  The plan is
    rebuilt for the batch after every round that moved a tree; the climb stops
    when no tree moves or after ``max_rounds`` rounds of moves.

    ``weights``: site weights, (L,) shared by all trees or (B, L) (pattern
    counts from ``compress_sites``, a ratchet's reweighting, bootstrap
    replicates).  Every score compared or returned is then the weighted one;
    the acceptance rule is unchanged.  Given as numpy they are validated on
    the host as finite and >= 0.
    """
    return _hill_climb(
        lambda eng, lv, c, t, dp, w: eng.nni_scores(lv, c, t, dp=dp, weights=w),
        lambda ch, nl, n_all, i: apply_nni(ch, nl + i // 2, i % 2),
        children, leaves, cost, tau, min_gain, max_rounds, device, weights)


def spr_hill_climb(children, leaves, cost, *, tau: float = 0.0, min_gain: float = 1e-5,
                   max_rounds: int = 100, device=None, weights=None) -> HillClimbResult:
    """Steepest-descent SPR search: ``nni_hill_climb`` with the SPR
    neighbourhood.  Every round scores all (n_all - 1) n_all moves (v, x) of
    every tree (``SankoffEngine.spr_scores``: one forward, one outside and one
    SPR pass; moves that do not exist score +inf) and takes the lowest (ties:
    the lowest flattened (v, x)) by ``apply_spr``.  Arguments, the acceptance
    rule, ``weights`` and the result are those of ``nni_hill_climb``.  An SPR
    local optimum is an NNI local optimum too."""
    return _hill_climb(
        lambda eng, lv, c, t, dp, w: eng.spr_scores(lv, c, t, dp=dp, weights=w),
        lambda ch, nl, n_all, i: apply_spr(ch, i // n_all, i % n_all),
        children, leaves, cost, tau, min_gain, max_rounds, device, weights)


_CLIMBS = {"nni": nni_hill_climb, "spr": spr_hill_climb}


def _climb(moves):
    """The hill climb of a search function's ``moves`` argument."""
    if moves not in _CLIMBS:
        raise ValueError(f"moves must be 'nni' or 'spr', got {moves!r}")
    return _CLIMBS[moves]


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
                      tau: float = 0.0, device=None, weights=None) -> StepwiseResult:
    """Starting trees by stepwise addition, B addition sequences in one batch.

    leaves int8 codes or int32 state sets (n, L), one alignment of n >= 3
    taxa; cost (Q, Q), Q <= 20.
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
    ``weights``: site weights as in ``nni_hill_climb``, (L,) or (B, L); the
    triplet forward, the attachment scores and the final scores are weighted.
    """
    torch = _torch()
    device = torch.device(device) if device is not None else _default_device()
    lv = _leaf_tensor(leaves, device)
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
    w = _site_weights(weights, B, L, device)
    taxa = lv[torch.from_numpy(order).to(device)]  # (B, n, L): tree b's taxa in its sequence

    def engine(ch_now):
        return SankoffEngine(TreePlan(ch_now), L, Q, device)

    first = taxa[:, :3].repeat_interleave(3, dim=0).contiguous()
    w3 = None if w is None else w.repeat_interleave(3, dim=0).contiguous()
    ts = engine(np.tile(_TRIPLETS, (B, 1, 1))).forward(first, c, tau, weights=w3).tree_score
    pick = ts.cpu().numpy().reshape(B, 3).argmin(axis=1)  # first minimum
    ch = [_TRIPLETS[i] for i in pick]
    for k in range(3, n):
        eng = engine(np.stack(ch))
        sc = eng.attach_scores(taxa[:, :k].contiguous(), c, tau,
                               new_leaf=taxa[:, k].contiguous(), weights=w)
        where = sc.cpu().numpy().argmin(axis=1)  # first minimum: the lowest node id
        ch = [insert_leaf(ch[b], int(where[b])) for b in range(B)]
    out = np.stack([relabel_leaves(ch[b], order[b]) for b in range(B)])
    shared = lv[None].expand(B, -1, -1).contiguous()
    scores = engine(out).forward(shared, c, tau, weights=w).tree_score.cpu().numpy()
    return StepwiseResult(out, scores.astype(np.float32), order)


def parsimony_search(leaves, cost, *, n_trees: int, seed: int = 0, tau: float = 0.0,
                     min_gain: float = 1e-5, max_rounds: int = 100, device=None,
                     weights=None, moves: str = "nni") -> SearchResult:
    """``stepwise_addition`` over ``n_trees`` addition sequences, then
    ``nni_hill_climb`` (``moves="nni"``) or ``spr_hill_climb``
    (``moves="spr"``) on its trees; ``weights`` ((L,) or (n_trees, L)) go to
    both."""
    climb = _climb(moves)
    start = stepwise_addition(leaves, cost, n_trees=n_trees, seed=seed, tau=tau, device=device,
                              weights=weights)
    r = climb(start.children, leaves, cost, tau=tau, min_gain=min_gain, max_rounds=max_rounds,
              device=device, weights=weights)
    return SearchResult(r.children, r.scores, r.history, r.n_moves, r.rounds, start.scores,
                        start.order)


# ---------------------------------------------------------------------------
# site weights: pattern compression, the parsimony ratchet, bootstrap support
# ---------------------------------------------------------------------------
def compress_sites(leaves):
    """Identical columns of one (n, L) alignment scored once: returns
    (patterns (n, P) int8, counts (P,) float32, index (L,) int64) with the
    distinct columns in order of first occurrence, ``patterns[:, index] ==
    leaves`` and ``counts == bincount(index)``.  The missing code -1 is a
    symbol like any other.  int32 leaves are state sets: the patterns are
    int32 too and a cell's whole mask is the symbol.  Host numpy; ``counts``
    are the ``weights`` of the scoring and search functions on ``patterns``."""
    lv = np.asarray(leaves)
    if lv.ndim != 2 or lv.shape[0] < 1 or lv.shape[1] < 1:
        raise ValueError(f"leaves must be (n, L), got {lv.shape}")
    lv = np.ascontiguousarray(lv.astype(np.int32 if lv.dtype == np.int32 else np.int8))
    cols = np.ascontiguousarray(lv.T).view(np.dtype((np.void, lv.shape[0] * lv.itemsize)))
    cols = cols.reshape(-1)
    _, first, inv = np.unique(cols, return_index=True, return_inverse=True)
    by_first = np.argsort(first, kind="stable")  # sorted patterns -> first-occurrence order
    rank = np.empty_like(by_first)
    rank[by_first] = np.arange(by_first.size)
    index = rank[inv.reshape(-1)].astype(np.int64)
    patterns = np.ascontiguousarray(lv[:, first[by_first]])
    counts = np.bincount(index, minlength=by_first.size).astype(np.float32)
    return patterns, counts, index


@dataclass
class RatchetResult:
    children: np.ndarray  # (B, n_all, 2) int32: the best tree of every start tree
    scores: np.ndarray  # (B,) float32: their scores under ``weights``
    history: list  # per tree: its best score after the first climb and after each iteration
    n_improved: np.ndarray  # (B,) int64: iterations that gave a strictly lower best


def parsimony_ratchet(children, leaves, cost, *, weights=None, n_iter: int = 10,
                      frac: float = 0.25, seed: int = 0, tau: float = 0.0,
                      min_gain: float = 1e-5, max_rounds: int = 100,
                      device=None, moves: str = "nni") -> RatchetResult:
    """The parsimony ratchet on a batch of start trees, each on its own.

    ``children`` and ``leaves`` as for ``nni_hill_climb``; ``weights`` host
    site weights, (L,) or (B, L), None: ones.  The start trees are climbed
    under ``weights``.  Every iteration then draws ``mask = rng.random((B, L))
    < frac`` from the one ``np.random.default_rng(seed)`` (one draw of that
    shape per iteration), climbs the current trees under ``weights * (1 +
    mask)`` -- the drawn sites count twice -- and climbs the result under
    ``weights`` again.  The search goes on from that tree whatever its score;
    each tree keeps the best tree it has seen, replaced only by a strictly
    lower score.  ``moves``: every climb is ``nni_hill_climb`` ("nni") or
    ``spr_hill_climb`` ("spr").
    """
    climb = _climb(moves)
    if n_iter < 0:
        raise ValueError("n_iter must be >= 0")
    if not 0.0 <= frac <= 1.0:
        raise ValueError("frac must be in [0, 1]")
    ch = np.array(children, dtype=np.int32, copy=True)
    if ch.ndim == 2:
        ch = ch[None]
    B = ch.shape[0]
    L = _n_sites(leaves)
    w0 = _host_weights(np.ones(L, np.float32) if weights is None else weights, B, L)
    kw = dict(tau=tau, min_gain=min_gain, max_rounds=max_rounds, device=device)
    rng = np.random.default_rng(seed)
    r = climb(ch, leaves, cost, weights=w0, **kw)
    best_ch, best = r.children.copy(), r.scores.copy()
    history = [[float(s)] for s in best]
    n_improved = np.zeros(B, dtype=np.int64)
    cur = r.children
    for _ in range(n_iter):
        mask = rng.random((B, L)) < frac
        up = climb(cur, leaves, cost, weights=w0 * (1.0 + mask).astype(np.float32), **kw)
        r = climb(up.children, leaves, cost, weights=w0, **kw)
        cur = r.children
        better = r.scores < best
        best_ch[better] = cur[better]
        best[better] = r.scores[better]
        n_improved += better
        for b in range(B):
            history[b].append(float(best[b]))
    return RatchetResult(best_ch, best.astype(np.float32), history, n_improved)


def bootstrap_weights(counts, n_replicates: int, seed: int = 0):
    """(n_replicates, L) float32 bootstrap replicates of an alignment whose
    column l stands for ``counts[l]`` sites (ones for an uncompressed one):
    ``default_rng(seed).multinomial(N, counts / N, size=n_replicates)`` with
    ``N = counts.sum()``, in float64."""
    c = np.asarray(counts, dtype=np.float64)
    if c.ndim != 1 or c.size < 1 or not np.isfinite(c).all() or (c < 0).any():
        raise ValueError("counts must be a non-empty (L,) vector of finite values >= 0")
    N = int(round(float(c.sum())))
    if N < 1 or n_replicates < 1:
        raise ValueError("counts must sum to >= 1 and n_replicates must be >= 1")
    rep = np.random.default_rng(seed).multinomial(N, c / N, size=int(n_replicates))
    return rep.astype(np.float32)


@dataclass
class BootstrapResult:
    search: SearchResult  # tree b: the search under replicate b's weights
    weights: np.ndarray  # (n_replicates, L) float32: the replicates' site weights


def bootstrap_search(leaves, cost, *, n_replicates: int, weights=None, seed: int = 0,
                     tau: float = 0.0, min_gain: float = 1e-5, max_rounds: int = 100,
                     device=None, moves: str = "nni") -> BootstrapResult:
    """One ``parsimony_search`` tree per bootstrap replicate, all replicates
    in the launches of one batch: tree b is built and climbed under row b of
    ``bootstrap_weights(weights, n_replicates, seed)`` (``weights``: the (L,)
    pattern counts of ``leaves``, None: ones).  ``clade_support`` of a
    reference tree over ``result.search.children`` gives its support values.
    ``moves``: as in ``parsimony_search``."""
    _climb(moves)
    L = _n_sites(leaves)
    counts = np.ones(L, np.float32) if weights is None else weights
    bw = bootstrap_weights(counts, n_replicates, seed)
    res = parsimony_search(leaves, cost, n_trees=n_replicates, seed=seed, tau=tau,
                           min_gain=min_gain, max_rounds=max_rounds, device=device, weights=bw,
                           moves=moves)
    return BootstrapResult(res, bw)


def _clades(children):
    """Leaf set (frozenset) under every internal node of one rooted tree, in
    node order (every child has an id below its parent's)."""
    ch = np.asarray(children)
    if ch.ndim != 2 or ch.shape[1] != 2 or ch.shape[0] % 2 == 0:
        raise ValueError(f"children must be (n_all, 2) with n_all odd, got {ch.shape}")
    n_all = ch.shape[0]
    nl = (n_all + 1) // 2
    below = [frozenset([x]) for x in range(nl)]
    for node in range(nl, n_all):
        c0, c1 = int(ch[node, 0]), int(ch[node, 1])
        if not (0 <= c0 < node and 0 <= c1 < node):
            raise ValueError(f"node {node}: children {c0}, {c1} are not below it")
        below.append(below[c0] | below[c1])
    return below[nl:]


def clade_support(children_ref, trees):
    """(n_int,) float64: for every internal node of ``children_ref`` (in node
    order) the share of ``trees`` ((T, n_all, 2) or (n_all, 2)) that contain
    its leaf set as a clade.  The trees are rooted, so these are rooted
    clades; the root's is all taxa and always 1.0."""
    ref = _clades(children_ref)
    tr = np.asarray(trees)
    if tr.ndim == 2:
        tr = tr[None]
    if tr.ndim != 3 or tr.shape[0] < 1 or tr.shape[1:] != np.asarray(children_ref).shape:
        raise ValueError(f"trees must be (T, {len(ref) * 2 + 1}, 2), got {tr.shape}")
    fams = [set(_clades(t)) for t in tr]
    return np.array([sum(s in f for f in fams) / len(fams) for s in ref], dtype=np.float64)
