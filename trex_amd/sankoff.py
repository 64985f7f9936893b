"""trex's ``sankoff`` module on MI355X.

Mirrors maraxen/trex ``src/trex/sankoff.py``: ``run_sankoff`` (:114-188),
``run_dp`` (:24-94), ``vectorized_dp`` (:97) and ancestral reconstruction
(:166-185, 191-267), plus what trex's readme promises but its code lacks -- a
differentiable score: ``sankoff_value_and_grad`` returns d(total)/d(cost)
(the tie-averaged subgradient JAX would give for tau=0, the softmin adjoint
for tau>0; DESIGN.md "Softmin").

All arithmetic runs in libtrexhip.so (HIP, gfx950).  torch is used only for
device memory and streams.  There is no CPU fallback.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._lib import TREX_FLAG_HARD_ROOT, check, lib, ptr, stream_handle
from .topology import TreePlan, children_from_adjacency

SENTINEL = 1e5  # src/trex/sankoff.py:152


def _torch():
    import torch

    return torch


def _default_device():
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError("trex_amd needs a ROCm GPU (MI355X); no CPU fallback exists")
    return torch.device("cuda", torch.cuda.current_device())


def leaf_codes(sequences, n_states: int, device=None):
    """trex leaf states -> int8 codes on the device.

    ``seq.astype(int32)`` is XLA's convert: truncation toward zero,
    saturation, NaN -> 0; negative states wrap once, anything else out of
    range is a dropped scatter (all-1e5 row, sankoff.py:49-52); such leaves
    get code -1.
    """
    torch = _torch()
    device = device or _default_device()
    s = torch.as_tensor(sequences).to(device=device, dtype=torch.float64)
    s = torch.trunc(s)
    s = torch.where(torch.isnan(s), torch.zeros_like(s), s)
    s = torch.where(s < 0, s + n_states, s)
    ok = (s >= 0) & (s < n_states)
    return torch.where(ok, s, torch.full_like(s, -1)).to(torch.int8).contiguous()


@dataclass
class ForwardResult:
    tree_score: "object"  # (B,) float32
    dp: "object"  # (B, n_int, L, Q) float32, site-major (trex's per-site rows)
    site_score: "object"  # (B, L) float32 or None


@dataclass
class EdgeChanges:
    counts: "object"  # (B, n_all, Q, Q) float32: [b, child node, parent state, child state]
    lengths: "object"  # (B, n_all) float32: sum_ij counts * cost
    length_min: "object"  # (B, n_all) float32, tau = 0; None at tau > 0
    length_max: "object"  # (B, n_all) float32, tau = 0; None at tau > 0


class SankoffEngine:
    """Batched Sankoff for a fixed (topology batch, L, Q): the hot path.

    leaves: int8 (B, n_leaves, L) codes on the device; cost: float32 (Q, Q).
    ``forward``, ``outside``, ``nni_scores``, ``attach_scores``, ``spr_scores`` and
    ``edge_changes`` also take int32 leaves: state sets, bit j of a cell = state j is allowed there
    (``sets_from_codes``, ``encode_alignment``; DESIGN.md "State-set leaves";
    Q <= 20, proper rooted binary trees).  The adjoint has no state-set form.
    Everything is enqueued on torch's current stream; nothing synchronises.
    """

    def __init__(self, plan: TreePlan, n_sites: int, n_states: int, device=None):
        torch = _torch()
        self.plan = plan
        self.L = int(n_sites)
        self.Q = int(n_states)
        self.device = torch.device(device) if device is not None else _default_device()
        self.plan_dev = plan.device(self.device)
        nbytes = lib().trex_workspace_bytes(plan.B, self.L, plan.n_all, self.Q)
        if nbytes <= 0:
            raise ValueError("bad shape for workspace")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        # arrival counters of the in-kernel reductions start at zero
        check(lib().trex_workspace_init(ptr(self.workspace), nbytes, stream_handle(self.device)))
        # Q = 4: the plan's steps predecoded for the fused softmin kernel
        # (sankoff_fused4.hip), built and uploaded once; None when the planner
        # refuses the topology (the generic kernel then takes every call)
        self.fused4_prog = self._fused4_program() if self.Q == 4 else None

    def _fused4_program(self):
        from ._lib import TREX_E_UNSUPPORTED, has_fused4

        L = lib()
        if not has_fused4():
            return None
        p = self.plan
        n = L.trex_fused4_program_ints(p.B, p.n_all)
        if n <= 0:
            return None
        host = np.zeros(n, dtype=np.int32)
        rc = L.trex_fused4_program_build(p.host.ctypes.data, p.B, p.n_all, host.ctypes.data)
        if rc == TREX_E_UNSUPPORTED:
            return None
        check(rc)
        return _torch().from_numpy(host).to(self.device)

    @staticmethod
    def _flags(hard_root):
        return TREX_FLAG_HARD_ROOT if hard_root else 0

    # -- shapes ------------------------------------------------------------
    @property
    def site_major(self) -> bool:
        """DP / marginal tables are site-major (B, n_int, L, Q) for every Q
        (trex_dp_site_major, include/trex_hip.h)."""
        return bool(lib().trex_dp_site_major(self.Q))

    @property
    def dp_shape(self):
        if self.site_major:
            return (self.plan.B, self.plan.n_int, self.L, self.Q)
        return (self.plan.B, self.plan.n_int, self.Q, self.L)

    def state_rows(self, table):
        """(B, n_int, Q, L) view of a DP / marginal table (the oracle's
        node-state-site order)."""
        return table.transpose(2, 3) if self.site_major else table

    def _check_inputs(self, leaves, cost, sets=False):
        """``sets``: the caller also takes int32 state sets.  Returns whether
        ``leaves`` are state sets."""
        torch = _torch()
        p = self.plan
        is_sets = leaves.dtype == torch.int32
        if is_sets and not sets:
            raise ValueError("int32 state-set leaves are not supported here: the adjoint "
                             "(backward, fwd_bwd, value_and_grad) and to_trex_layout take int8 "
                             "codes only")
        if ((leaves.dtype != torch.int8 and not is_sets)
                or tuple(leaves.shape) != (p.B, p.n_leaves, self.L)):
            raise ValueError(f"leaves must be int8 {(p.B, p.n_leaves, self.L)}"
                             f"{' (codes) or int32 (state sets)' if sets else ''}, got "
                             f"{leaves.dtype} {tuple(leaves.shape)}")
        if cost.dtype != torch.float32 or tuple(cost.shape) != (self.Q, self.Q):
            raise ValueError(f"cost must be float32 ({self.Q}, {self.Q})")
        for t in (leaves, cost):
            if not t.is_contiguous() or t.device != self.device:
                raise ValueError("inputs must be contiguous tensors on the engine's device")
        if is_sets:
            from ._lib import has_leaf_sets

            if not has_leaf_sets():
                raise RuntimeError(f"{lib()._name} has no state-set leaf entry points "
                                   "(trex_sankoff_sets_fwd, _sets_outside, _sets_nni_w, "
                                   "_sets_attach_w): rebuild libtrexhip.so")
        return is_sets

    def _scratch(self, name):
        """The uint8 workspace of pass ``name`` ("sets_fwd", "nni", "attach",
        "spr", "edge"), trex_<name>_workspace_bytes long: kept in ``self._<name>_ws``,
        grown when too small, never initialised."""
        p = self.plan
        nbytes = getattr(lib(), f"trex_{name}_workspace_bytes")(p.B, self.L, p.n_all, self.Q)
        ws = getattr(self, f"_{name}_ws", None)
        if ws is None or ws.numel() < max(nbytes, 1):
            ws = _torch().empty(max(nbytes, 1), dtype=_torch().uint8, device=self.device)
            setattr(self, f"_{name}_ws", ws)
        return ws

    def _check_tensor(self, t, what, shape, dtype=None):
        """``t`` is a contiguous tensor of ``shape`` and ``dtype`` (None:
        float32) on the engine's device; ValueError naming it ``what``
        otherwise."""
        name = "float32" if dtype is None else str(dtype)
        if (not hasattr(t, "dtype") or t.dtype != (dtype or _torch().float32)
                or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device):
            raise ValueError(f"{what} must be a contiguous {name} {shape} tensor on the engine's "
                             "device")

    def _check_weights(self, weights):
        """Site weights: a contiguous float32 (B, L) tensor on the engine's
        device, one row per tree.  Values are not read here (nothing
        synchronises): they must be finite, and scores carry the kernels'
        relative bar only when they are >= 0."""
        from ._lib import has_site_weights

        self._check_tensor(weights, "weights", (self.plan.B, self.L))
        if not has_site_weights():
            raise RuntimeError(f"{lib()._name} has no site-weight entry points "
                               "(trex_site_weighted_sum, trex_sankoff_nni_w, "
                               "trex_sankoff_attach_w): rebuild libtrexhip.so")

    # -- kernels -----------------------------------------------------------
    def weighted_score(self, site_score, weights, out=None):
        """(B,) float32 ``sum_l weights[b, l] * site_score[b, l]`` of a
        forward's ``site_score`` (B, L): products and sum in fp64 in a fixed
        order, rounded once; repeated calls are bitwise equal.  Weights are
        finite; the relative bar of the site scores carries over only when
        they are >= 0."""
        torch = _torch()
        self._check_weights(weights)
        B = self.plan.B
        self._check_tensor(site_score, "site_score", (B, self.L))
        if out is None:
            out = torch.empty((B,), dtype=torch.float32, device=self.device)
        else:
            self._check_tensor(out, "out", (B,))
        check(lib().trex_site_weighted_sum(ptr(site_score), ptr(weights), B, self.L, ptr(out),
                                           stream_handle(self.device)))
        return out

    def forward(self, leaves, cost, tau: float = 0.0, *, dp=True, site_score=False,
                hard_root=False, out=None, weights=None) -> ForwardResult:
        """Post-order DP (sankoff.py:24-97) + per-tree total (sankoff.py:187).

        ``weights`` (float32 (B, L), finite): ``tree_score`` is the weighted
        total ``sum_l weights[b, l] * site_score[b, l]`` (``weighted_score``)
        and ``site_score`` is returned too; the DP table is per site and does
        not depend on the weights.  ``hard_root`` keeps its meaning: it
        selects how each site's score is taken from the root row, and the
        weighted total is the weighted sum of those site scores."""
        torch = _torch()
        is_sets = self._check_inputs(leaves, cost, sets=True)
        if weights is not None:
            self._check_weights(weights)
            site_score = True
        p = self.plan
        o = out or {}
        if dp is True:
            dp_t = o.get("dp")
            if dp_t is None:
                dp_t = torch.empty(self.dp_shape, dtype=torch.float32, device=self.device)
        elif dp is not False and dp is not None:
            dp_t = dp
        else:
            raise ValueError("forward writes the DP table (trex returns it); pass dp=True")
        ss = None
        if site_score:
            ss = o.get("site_score")
            if ss is None:
                ss = torch.empty((p.B, self.L), dtype=torch.float32, device=self.device)
        ts = o.get("tree_score")
        if ts is None:
            ts = torch.empty((p.B,), dtype=torch.float32, device=self.device)
        flags = self._flags(hard_root)
        if is_sets:
            ws = self._scratch("sets_fwd")
            check(lib().trex_sankoff_sets_fwd(
                ptr(p.attach_device(self.device)), ptr(leaves), ptr(cost), p.B, self.L, p.n_all,
                self.Q, float(tau), flags, ptr(dp_t), ptr(ss), ptr(ts), ptr(ws), ws.numel(),
                stream_handle(self.device)))
        else:
            check(lib().trex_sankoff_fwd(
                ptr(self.plan_dev), p.slot_word, ptr(leaves), ptr(cost), p.B, self.L, p.n_all,
                self.Q, float(tau), flags, ptr(dp_t), ptr(ss), ptr(ts), ptr(self.workspace),
                self.workspace.numel(), stream_handle(self.device)))
        if weights is not None:
            self.weighted_score(ss, weights, out=ts)
        return ForwardResult(ts, dp_t, ss)

    def backward(self, leaves, cost, tau: float, dp, d_tree_score=None, *, marginals=False,
                 anc_states=False, hard_root=False, out=None):
        """Adjoint sweep: (d_cost, marginals | None, anc_states | None)."""
        torch = _torch()
        self._check_inputs(leaves, cost)
        p = self.plan
        if dp is None or tuple(dp.shape) != self.dp_shape:
            raise ValueError("backward needs the forward's dp table")
        o = out or {}
        dc = o.get("d_cost")
        if dc is None:
            dc = torch.empty((self.Q, self.Q), dtype=torch.float32, device=self.device)
        mg = None
        if marginals:
            mg = o.get("marginals")
            if mg is None:
                mg = torch.empty(self.dp_shape, dtype=torch.float32, device=self.device)
        an = None
        if anc_states:
            an = torch.empty((p.B, p.n_int, self.L), dtype=torch.int8, device=self.device)
        if d_tree_score is not None:
            d_tree_score = torch.as_tensor(d_tree_score, dtype=torch.float32,
                                           device=self.device).contiguous()
            if d_tree_score.shape != (p.B,):
                raise ValueError("d_tree_score must be (B,)")
        flags = self._flags(hard_root)
        check(lib().trex_sankoff_bwd(
            ptr(self.plan_dev), p.slot_word, ptr(leaves), ptr(cost), p.B, self.L, p.n_all,
            self.Q, float(tau), flags, ptr(dp), ptr(d_tree_score), ptr(dc), ptr(mg), ptr(an),
            ptr(self.workspace), self.workspace.numel(), stream_handle(self.device)))
        return dc, mg, an

    def fwd_bwd(self, leaves, cost, tau: float = 0.0, d_tree_score=None, *, site_score=False,
                marginals=False, anc_states=False, hard_root=False, out=None):
        """Fused forward + adjoint in one launch (trex_sankoff_fwd_bwd).

        Returns (ForwardResult, d_cost, marginals | None, anc_states | None).
        """
        torch = _torch()
        self._check_inputs(leaves, cost)
        p = self.plan
        o = out or {}

        def buf(key, shape, dtype, want=True):
            if not want:
                return None
            t = o.get(key)
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=self.device)
            return t

        dp_t = buf("dp", self.dp_shape, torch.float32)
        ss = buf("site_score", (p.B, self.L), torch.float32, site_score)
        ts = buf("tree_score", (p.B,), torch.float32)
        dc = buf("d_cost", (self.Q, self.Q), torch.float32)
        mg = buf("marginals", self.dp_shape, torch.float32, marginals)
        an = buf("anc_states", (p.B, p.n_int, self.L), torch.int8, anc_states)
        if d_tree_score is not None:
            d_tree_score = torch.as_tensor(d_tree_score, dtype=torch.float32,
                                           device=self.device).contiguous()
            if d_tree_score.shape != (p.B,):
                raise ValueError("d_tree_score must be (B,)")
        flags = self._flags(hard_root)
        args = (ptr(self.plan_dev), p.slot_word, ptr(leaves), ptr(cost), p.B, self.L, p.n_all,
                self.Q, float(tau), flags, ptr(dp_t), ptr(ss), ptr(ts), ptr(d_tree_score), ptr(dc),
                ptr(mg), ptr(an), ptr(self.workspace), self.workspace.numel(),
                stream_handle(self.device))
        if self.fused4_prog is not None:
            check(lib().trex_sankoff_fwd_bwd_prog(*args, ptr(self.fused4_prog)))
        else:
            check(lib().trex_sankoff_fwd_bwd(*args))
        return ForwardResult(ts, dp_t, ss), dc, mg, an

    def backtrack(self, cost, dp):
        """trex-exact ancestral states (B, n_int, L) int8 (sankoff.py:166-185)."""
        torch = _torch()
        p = self.plan
        an = torch.empty((p.B, p.n_int, self.L), dtype=torch.int8, device=self.device)
        check(lib().trex_sankoff_backtrack(
            ptr(self.plan_dev), p.backtrack_ok, ptr(cost), ptr(dp), p.B, self.L, p.n_all,
            self.Q, ptr(an), stream_handle(self.device)))
        return an

    # -- search passes (sankoff_rows.h, sankoff_nni / _sets / _spr.hip) ------
    def _check_table(self, t, what):
        self._check_tensor(t, what, self.dp_shape)

    def _scoring_tables(self, leaves, cost, tau, dp, outside, weights, also=None):
        """What every scoring call starts with: the inputs checked (``also``:
        the call's own argument check, run next), then ``(is_sets, dp,
        outside)`` with the forward and / or the outside pass run for a table
        that was not given."""
        is_sets = self._check_inputs(leaves, cost, sets=True)
        if weights is not None:
            self._check_weights(weights)
        if also is not None:
            also()
        if dp is None:
            if outside is not None:
                raise ValueError("outside without the dp table it was computed from")
            dp = self.forward(leaves, cost, tau).dp
        self._check_table(dp, "dp")
        if outside is None:
            outside = self.outside(leaves, cost, tau, dp)
        self._check_table(outside, "outside")
        return is_sets, dp, outside

    def outside(self, leaves, cost, tau: float, dp):
        """Outside table (B, n_int, L, Q) of ``dp`` (a forward's table at the
        same tau): O_root = 0, O_c[j] = (+)_i (C[i][j] + O_p[i] + M_s[i])."""
        torch = _torch()
        is_sets = self._check_inputs(leaves, cost, sets=True)
        self._check_table(dp, "dp")
        p = self.plan
        out = torch.empty(self.dp_shape, dtype=torch.float32, device=self.device)
        fn = lib().trex_sankoff_sets_outside if is_sets else lib().trex_sankoff_outside
        check(fn(
            ptr(p.nni_device(self.device)), ptr(leaves), ptr(cost), p.B, self.L, p.n_all, self.Q,
            float(tau), ptr(dp), ptr(out), stream_handle(self.device)))
        return out

    def nni_scores(self, leaves, cost, tau: float = 0.0, *, dp=None, outside=None, weights=None):
        """Tree scores of all NNI neighbours, float32 (B, n_int - 1, 2): entry
        [b, v - n_leaves, k] is tree b after ``apply_nni(children[b], v, k)``
        (plain score: no hard_root).  Runs the forward and / or the outside
        pass when ``dp`` / ``outside`` are not given.  ``weights`` (float32
        (B, L), finite): every site's move score is multiplied by its weight
        in fp64 where the sites are summed; the tables stay unweighted.
        All-ones weights give the bits of the unweighted call; the relative
        bar holds only for weights >= 0."""
        torch = _torch()
        is_sets, dp, outside = self._scoring_tables(leaves, cost, tau, dp, outside, weights)
        p = self.plan
        ws = self._scratch("nni")
        score = torch.empty((p.B, p.n_int - 1, 2), dtype=torch.float32, device=self.device)
        head = (ptr(p.nni_device(self.device)), ptr(leaves), ptr(cost), p.B, self.L, p.n_all,
                self.Q, float(tau), ptr(dp), ptr(outside))
        tail = (ptr(score), ptr(ws), ws.numel(), stream_handle(self.device))
        if is_sets:
            check(lib().trex_sankoff_sets_nni_w(*head, ptr(weights), *tail))
        elif weights is None:  # also what an older library under TREX_HIP_LIB has
            check(lib().trex_sankoff_nni(*head, *tail))
        else:
            check(lib().trex_sankoff_nni_w(*head, ptr(weights), *tail))
        return score

    def attach_scores(self, leaves, cost, tau: float = 0.0, *, new_leaf=None, sub_rows=None,
                      dp=None, outside=None, weights=None):
        """Tree scores after attaching a subtree on every edge, float32
        (B, n_all): entry [b, x] is tree b with the subtree on the edge above
        node x (``insert_leaf(children[b], x)`` for a leaf; x = n_all - 1 is a
        new root; plain score).  The subtree is ``new_leaf``, (B, L) leaf
        cells of ``leaves``' dtype (int8 codes or int32 sets), or ``sub_rows``, float32 (B, L, Q) inside rows (a subtree's
        root DP row).  Runs the forward and / or the outside pass when ``dp``
        / ``outside`` are not given.  ``weights`` (float32 (B, L), finite):
        site weights as in ``nni_scores``."""
        torch = _torch()
        p = self.plan

        def check_subtree():
            if (new_leaf is None) == (sub_rows is None):
                raise ValueError("give exactly one of new_leaf and sub_rows")
            if sub_rows is None:
                self._check_tensor(new_leaf, "new_leaf", (p.B, self.L), leaves.dtype)
            else:
                self._check_tensor(sub_rows, "sub_rows", (p.B, self.L, self.Q), torch.float32)

        is_sets, dp, outside = self._scoring_tables(leaves, cost, tau, dp, outside, weights,
                                                    check_subtree)
        ws = self._scratch("attach")
        score = torch.empty((p.B, p.n_all), dtype=torch.float32, device=self.device)
        head = (ptr(p.attach_device(self.device)), ptr(leaves), ptr(cost), p.B, self.L, p.n_all,
                self.Q, float(tau), ptr(dp), ptr(outside), ptr(new_leaf), ptr(sub_rows))
        tail = (ptr(score), ptr(ws), ws.numel(), stream_handle(self.device))
        if is_sets:
            check(lib().trex_sankoff_sets_attach_w(*head, ptr(weights), *tail))
        elif weights is None:
            check(lib().trex_sankoff_attach(*head, *tail))
        else:
            check(lib().trex_sankoff_attach_w(*head, ptr(weights), *tail))
        return score

    def spr_scores(self, leaves, cost, tau: float = 0.0, *, dp=None, outside=None, weights=None):
        """Tree scores of all SPR neighbours, float32 (B, n_all - 1, n_all):
        entry [b, v, x] is tree b after ``apply_spr(children[b], v, x)`` --
        the subtree of v pruned and regrafted on the edge above x (plain
        score); +inf where the move does not exist (x in subtree(v), x = v's
        parent).  Entry [b, v, sibling(v)] is the tree's own score.  Leaves are
        int8 codes or int32 state sets.  Runs the forward and / or the outside
        pass when ``dp`` / ``outside`` are not given.  ``weights`` (float32
        (B, L), finite): site weights as in ``nni_scores``."""
        torch = _torch()
        p = self.plan
        is_sets, dp, outside = self._scoring_tables(leaves, cost, tau, dp, outside, weights,
                                                    lambda: p.spr_device(self.device))
        ws = self._scratch("spr")
        score = torch.empty((p.B, p.n_all - 1, p.n_all), dtype=torch.float32, device=self.device)
        fn = lib().trex_sankoff_sets_spr_w if is_sets else lib().trex_sankoff_spr_w
        check(fn(ptr(p.spr_device(self.device)), ptr(leaves), ptr(cost), p.B, self.L, p.n_all, self.Q, float(tau),
                 ptr(dp), ptr(outside), ptr(weights), ptr(score), ptr(ws), ws.numel(),
                 stream_handle(self.device)))
        return score

    def edge_changes(self, leaves, cost, tau: float = 0.0, *, dp=None, outside=None, states=None,
                     weights=None) -> EdgeChanges:
        """What happens on every branch (DESIGN.md "Per-branch changes"):
        ``EdgeChanges(counts (B, n_all, Q, Q), lengths (B, n_all), length_min,
        length_max)``, indexed by the branch's lower (child) node id;
        ``counts[b, c, i, j]`` has the parent's state i first, as ``cost[i,
        j]``; the root's entries are 0.

        tau > 0: ``counts`` are the posterior expected numbers of sites (site
        weights) with the pair of states (i, j) on the branch -- their sum
        over the branches is ``value_and_grad``'s ``d_cost``; ``length_min``
        and ``length_max`` are None and ``states`` must not be given.

        tau = 0: ``counts`` follow the reconstruction ``states`` (int8 (B,
        n_int, L), default ``self.backtrack(cost, dp)``); a leaf takes the
        cheapest state its cell allows under its parent's state (first index
        on ties); a site with a value outside [0, Q) in ``states`` is left out
        of the branches that touch that node.  ``length_min`` / ``length_max``
        are the branch's least and largest length over ALL most-parsimonious
        reconstructions: a branch with ``length_max == 0`` is unsupported.
        They compare fp32 sums for equality: exact for integer and dyadic
        costs; for other costs the ties are the ones fp32 sees.

        ``lengths = sum_ij counts * cost``.  Leaves are int8 codes or int32
        state sets.  Runs the forward and / or the outside pass when ``dp`` /
        ``outside`` are not given.  ``weights`` (float32 (B, L), finite): site
        weights as in ``nni_scores``.  Sums over sites are fp64 in a fixed
        order: repeated calls are bitwise equal."""
        from ._lib import has_edge_changes

        torch = _torch()
        p = self.plan
        hard = not tau > 0.0

        def check_states():
            if not has_edge_changes():
                raise RuntimeError(f"{lib()._name} has no per-branch change entry points "
                                   "(trex_sankoff_edge_changes_w, "
                                   "trex_sankoff_sets_edge_changes_w): rebuild libtrexhip.so")
            if states is None:
                return
            if not hard:
                raise ValueError("states are a tau = 0 reconstruction; at tau > 0 the counts are "
                                 "posterior expectations")
            self._check_tensor(states, "states", (p.B, p.n_int, self.L), torch.int8)

        is_sets, dp, outside = self._scoring_tables(leaves, cost, tau, dp, outside, weights,
                                                    check_states)
        if hard and states is None:
            states = self.backtrack(cost, dp)
        ws = self._scratch("edge")

        def new(*shape):
            return torch.empty(shape, dtype=torch.float32, device=self.device)

        counts, lengths = new(p.B, p.n_all, self.Q, self.Q), new(p.B, p.n_all)
        lmin, lmax = (new(p.B, p.n_all), new(p.B, p.n_all)) if hard else (None, None)
        fn = lib().trex_sankoff_sets_edge_changes_w if is_sets else lib().trex_sankoff_edge_changes_w
        check(fn(ptr(p.attach_device(self.device)), ptr(leaves), ptr(cost), p.B, self.L, p.n_all,
                 self.Q, float(tau), ptr(dp), ptr(outside), ptr(states), ptr(weights),
                 ptr(counts), ptr(lengths), ptr(lmin), ptr(lmax), ptr(ws), ws.numel(),
                 stream_handle(self.device)))
        return EdgeChanges(counts, lengths, lmin, lmax)

    def value_and_grad(self, leaves, cost, tau: float = 0.0, d_tree_score=None,
                       hard_root=False):
        """(tree_score (B,), d_cost (Q, Q)) -- fused fwd + adjoint launch."""
        f, dc, _, _ = self.fwd_bwd(leaves, cost, tau, d_tree_score, hard_root=hard_root)
        return f.tree_score, dc

    def to_trex_layout(self, dp, leaves):
        """engine dp table -> trex VmappedDPTable per tree: (B, L, n_all, Q)."""
        torch = _torch()
        p = self.plan
        if leaves.dtype == torch.int32:
            raise ValueError("to_trex_layout does not support int32 state-set leaves: the trex "
                             "table's leaf rows are written from int8 codes")
        out = torch.empty((p.B, self.L, p.n_all, self.Q), dtype=torch.float32,
                          device=self.device)
        check(lib().trex_dp_to_trex_layout(ptr(dp), ptr(leaves), p.B, self.L, p.n_all, self.Q,
                                           ptr(out), stream_handle(self.device)))
        return out


# ---------------------------------------------------------------------------
# trex module API
# ---------------------------------------------------------------------------
_PLANS: dict = {}
_ENGINES: dict = {}


def _plan_for(adjacency) -> TreePlan:
    a = np.ascontiguousarray(np.asarray(adjacency, dtype=np.float32))
    key = (a.shape, a.tobytes())
    plan = _PLANS.get(key)
    if plan is None:
        if len(_PLANS) > 256:
            _PLANS.clear()
        plan = TreePlan.from_adjacency(a)
        _PLANS[key] = plan
    return plan


def _engine_for(plan: TreePlan, L: int, Q: int, device) -> SankoffEngine:
    key = (id(plan), L, Q, str(device))
    eng = _ENGINES.get(key)
    if eng is None:
        if len(_ENGINES) > 64:
            _ENGINES.clear()
        eng = SankoffEngine(plan, L, Q, device)
        _ENGINES[key] = eng
    return eng


def _to_host(x):
    if hasattr(x, "detach"):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _prepare(adjacency_matrix, cost_matrix, sequences, n_all, n_states, n_leaves, device):
    torch = _torch()
    adj = _to_host(adjacency_matrix)
    if adj.shape != (n_all, n_all):
        raise ValueError(f"adjacency_matrix must be ({n_all}, {n_all}), got {adj.shape}")
    device = device or _default_device()
    seqs = torch.as_tensor(sequences)
    # the DP reads (n_all+1)//2 leaf rows whatever n_leaves says (sankoff.py:46,49);
    # run_sankoff copies n_leaves of them into the reconstruction (:162)
    need = max(n_leaves, (n_all + 1) // 2)
    if seqs.ndim != 2 or seqs.shape[0] < need:
        raise ValueError(f"sequences must be (>= {need}, L), got {tuple(seqs.shape)}")
    cost = torch.as_tensor(cost_matrix).to(device=device, dtype=torch.float32).contiguous()
    if tuple(cost.shape) != (n_states, n_states):
        raise ValueError(f"cost_matrix must be ({n_states}, {n_states})")
    plan = _plan_for(adj)
    L = int(seqs.shape[1])
    eng = _engine_for(plan, L, n_states, device)
    codes = leaf_codes(seqs[:(n_all + 1) // 2], n_states, device)[None].contiguous()
    return plan, eng, codes, cost, seqs


# the engine's alphabet limit (int8 leaf codes / ancestral states,
# include/trex_hip.h); run_sankoff takes the raw-table kernels past it
ENGINE_MAX_STATES = 128


def _run_sankoff_raw(adjacency_matrix, cost_matrix, sequences, n_all, n_states, n_leaves,
                     return_path, device):
    """run_sankoff for n_states > ENGINE_MAX_STATES on the reference's own
    tables (sankoff.py:141-188 step for step): the raw-table DP
    (``trex_run_dp``: sentinel-filled (L, n_all, Q) table, (L, n_all, Q, 4)
    backtracking table), the reference's DFS from the root row's first argmin
    (``trex_backtrack_generic``), the total from ``trex_dp_root_total``."""
    torch = _torch()
    device = torch.device(device) if device is not None else _default_device()
    adj = np.array(_to_host(adjacency_matrix), dtype=np.float32, copy=True)
    if adj.shape != (n_all, n_all):
        raise ValueError(f"adjacency_matrix must be ({n_all}, {n_all}), got {adj.shape}")
    adj[-1, -1] = 0  # sankoff.py:141
    seqs = _f32_dev(sequences, device)
    if seqs.ndim != 2 or seqs.shape[0] < max(n_leaves, (n_all + 1) // 2):
        raise ValueError(f"sequences must be (>= {max(n_leaves, (n_all + 1) // 2)}, L), "
                         f"got {tuple(seqs.shape)}")
    cost = _f32_dev(cost_matrix, device)
    if tuple(cost.shape) != (n_states, n_states):
        raise ValueError(f"cost_matrix must be ({n_states}, {n_states})")
    L = int(seqs.shape[1])
    dp, bt = vectorized_dp(adj, torch.full((L, n_all, n_states), SENTINEL, dtype=torch.float32,
                                           device=device),
                           torch.zeros((L, n_all, n_states, 4), dtype=torch.float32,
                                       device=device), seqs, cost, device=device)
    recon = torch.zeros((n_all, L), dtype=torch.float32, device=device)
    recon[:n_leaves] = seqs[:n_leaves]
    if return_path:
        chars = vmapped_backtrack(n_all - 1, None, bt, n_all, n_leaves, dp=dp, device=device)
        recon[n_leaves:] = chars[n_leaves:].to(torch.float32)
    site_min = torch.empty(L, dtype=torch.float32, device=device)
    total = torch.empty((), dtype=torch.float32, device=device)
    check(lib().trex_dp_root_total(ptr(dp), L, n_all, n_states, ptr(site_min), ptr(total),
                                   stream_handle(device)))
    return recon, dp, total


def run_sankoff(adjacency_matrix, cost_matrix, sequences, n_all: int, n_states: int,
                n_leaves: int, *, return_path: bool = False, device=None):
    """Sankoff over one tree (sankoff.py:114-188).

    Returns (reconstructed (n_all, L) f32, dp (L, n_all, Q) f32, total f32[]) as
    device tensors with trex's layouts and values.  Alphabets past the
    engine's 128 states run on the raw-table kernels (``_run_sankoff_raw``).
    """
    torch = _torch()
    if n_states > ENGINE_MAX_STATES:
        return _run_sankoff_raw(adjacency_matrix, cost_matrix, sequences, n_all, n_states,
                                n_leaves, return_path, device)
    plan, eng, codes, cost, seqs = _prepare(adjacency_matrix, cost_matrix, sequences, n_all,
                                            n_states, n_leaves, device)
    f = eng.forward(codes, cost, 0.0, dp=True)
    dp_trex = eng.to_trex_layout(f.dp, codes)[0]
    L = eng.L
    recon = torch.zeros((n_all, L), dtype=torch.float32, device=eng.device)
    recon[:n_leaves] = seqs[:n_leaves].to(device=eng.device, dtype=torch.float32)
    if return_path:
        if n_leaves == (n_all + 1) // 2:
            anc = eng.backtrack(cost, f.dp)[0]
            recon[n_leaves:] = anc.to(torch.float32)
        else:
            # the reference backtracks with the n_leaves argument while its DP
            # used (n_all+1)//2 leaf rows (sankoff.py:46 vs :179): rows the
            # two disagree on follow the raw backtracking table, so take the
            # raw-table path (run_dp's table, then the reference's DFS)
            adj = np.array(_to_host(adjacency_matrix), dtype=np.float32, copy=True)
            adj[-1, -1] = 0
            _, bt = vectorized_dp(adj, torch.full((L, n_all, n_states), SENTINEL,
                                                  dtype=torch.float32, device=eng.device),
                                  torch.zeros((L, n_all, n_states, 4), dtype=torch.float32,
                                              device=eng.device),
                                  seqs.to(device=eng.device, dtype=torch.float32), cost)
            chars = vmapped_backtrack(n_all - 1, None, bt, n_all, n_leaves, dp=dp_trex)
            recon[n_leaves:] = chars[n_leaves:].to(torch.float32)
    return recon, dp_trex, f.tree_score[0]


def sankoff_value_and_grad(adjacency_matrix, cost_matrix, sequences, n_all: int,
                           n_states: int, n_leaves: int, *, tau: float = 0.0,
                           hard_root: bool = False, device=None):
    """(total, d total / d cost_matrix) for one tree.

    tau = 0: exactly ``jax.value_and_grad(lambda C: run_sankoff(adj, C, ...)[2])``
    semantics (hard min, tie-averaged subgradient).  tau > 0: softmin score
     and its exact gradient.
    """
    _, eng, codes, cost, _ = _prepare(adjacency_matrix, cost_matrix, sequences, n_all,
                                      n_states, n_leaves, device)
    ts, dc = eng.value_and_grad(codes, cost, tau, hard_root=hard_root)
    return ts[0], dc


# ---------------------------------------------------------------------------
# raw-table entry points: run_dp / vectorized_dp / backtrack_sankoff_jit on the
# reference's own table layouts (rundp.hip)
# ---------------------------------------------------------------------------
def _f32_dev(x, device):
    torch = _torch()
    return torch.as_tensor(x).to(device=device, dtype=torch.float32).contiguous()


def _raw_dp(adjacency_matrix, dp, bt, seqs3, cost_matrix, device):
    """dp (L, n_all, Q), bt (L, n_all, Q, 4), seqs3 (n, n_codes, L) -> new (dp, bt)."""
    torch = _torch()
    adj = _to_host(adjacency_matrix)
    if adj.ndim != 2 or adj.shape[0] != adj.shape[1]:
        raise ValueError(f"adjacency_matrix must be square, got {adj.shape}")
    n_all = adj.shape[0]
    L, n2, Q = dp.shape
    if n2 != n_all or tuple(bt.shape) != (L, n_all, Q, 4):
        raise ValueError(f"tables must be ({L}, {n_all}, {Q}) and ({L}, {n_all}, {Q}, 4), got "
                         f"{tuple(dp.shape)} and {tuple(bt.shape)}")
    nl = (n_all + 1) // 2
    if seqs3.shape[0] < nl or seqs3.shape[2] != L:
        raise ValueError(f"sequences need >= {nl} leaf rows over {L} sites")
    cost = _f32_dev(cost_matrix, device)
    if tuple(cost.shape) != (Q, Q):
        raise ValueError(f"cost_matrix must be ({Q}, {Q})")
    # run_dp does not drop the root self-loop (run_sankoff does, sankoff.py:141)
    ch = children_from_adjacency(adj, drop_root_self_loop=False)[0]
    ch_dev = torch.as_tensor(ch, device=device).contiguous()
    dp_out = _f32_dev(dp, device).clone()
    bt_out = _f32_dev(bt, device).clone()
    sq = _f32_dev(seqs3, device)
    check(lib().trex_run_dp(ptr(ch_dev), n_all, L, Q, ptr(sq), int(sq.shape[1]), ptr(cost),
                            ptr(dp_out), ptr(bt_out), stream_handle(device)))
    return dp_out, bt_out


def run_dp(adjacency_matrix, dynamic_programming_table, backtracking_table, sequences,
           cost_matrix, *, device=None):
    """trex's ``run_dp`` (sankoff.py:24-94) for one site on the device.

    dynamic_programming_table (n_all, Q) and backtracking_table (n_all, Q, 4)
    as the caller initialised them (inputs are not modified); sequences
    (n >= (n_all+1)//2,) states, or (n, k): ``.at[i, sequences[i]]`` then
    zeroes all k listed states of leaf i.  Returns new (dp, bt) tensors.
    """
    torch = _torch()
    device = torch.device(device) if device is not None else _default_device()
    dp = torch.as_tensor(dynamic_programming_table)
    bt = torch.as_tensor(backtracking_table)
    if dp.ndim != 2 or bt.ndim != 3:
        raise ValueError("run_dp takes one site's (n_all, Q) / (n_all, Q, 4) tables")
    sq = torch.as_tensor(sequences).to(torch.float32)
    if sq.ndim == 1:
        sq = sq[:, None]
    if sq.ndim != 2:
        raise ValueError("sequences must be (n,) or (n, k)")
    d, b = _raw_dp(adjacency_matrix, dp[None], bt[None], sq[:, :, None], cost_matrix, device)
    return d[0], b[0]


def vectorized_dp(adjacency_matrix, dynamic_programming_table, backtracking_table, sequences,
                  cost_matrix, *, device=None):
    """``vmap(run_dp, (None, 0, 0, 1, None))`` (sankoff.py:97): tables
    (L, n_all, Q) / (L, n_all, Q, 4), sequences (n, L).  Returns new tables."""
    torch = _torch()
    device = torch.device(device) if device is not None else _default_device()
    dp = torch.as_tensor(dynamic_programming_table)
    bt = torch.as_tensor(backtracking_table)
    sq = torch.as_tensor(sequences)
    if dp.ndim != 3 or bt.ndim != 4 or sq.ndim != 2:
        raise ValueError("vectorized_dp takes (L, n_all, Q), (L, n_all, Q, 4), (n, L)")
    return _raw_dp(adjacency_matrix, dp, bt, sq[:, None, :], cost_matrix, device)


_MAX_BACKTRACK_STEPS = 1 << 26


def vmapped_backtrack(root_node, root_states, backtracking_table, n_all: int, n_leaves: int, *,
                      dp=None, device=None):
    """``vmap(backtrack_sankoff_jit, in_axes=(None, 0, 0, None, None),
    out_axes=1)`` (sankoff.py:166-180): bt (L, n_all, Q, 4), root_states (L,)
    -> int32 (n_all, L).  root_states None: first argmin of dp[:, root_node]
    (dp (L, n_all, Q), sankoff.py:172).  A table whose DFS would not terminate
    (the reference hangs) raises TrexError(TREX_E_TOPOLOGY)."""
    from ._lib import TREX_E_TOPOLOGY, TrexError

    torch = _torch()
    bt = torch.as_tensor(backtracking_table)
    device = (torch.device(device) if device is not None
              else (bt.device if bt.is_cuda else _default_device()))
    bt = _f32_dev(bt, device)
    if bt.ndim != 4 or bt.shape[1] != n_all or bt.shape[3] != 4:
        raise ValueError(f"backtracking_table must be (L, {n_all}, Q, 4)")
    L, _, Q, _ = bt.shape
    rs = None
    dpt = None
    if root_states is not None:
        rs = torch.as_tensor(root_states).to(device=device, dtype=torch.int32).reshape(-1)
        if rs.numel() != L:
            raise ValueError(f"root_states must have {L} entries")
        rs = rs.contiguous()
    else:
        if dp is None:
            raise ValueError("root_states or dp is required")
        dpt = _f32_dev(dp, device)
        if tuple(dpt.shape) != (L, n_all, Q):
            raise ValueError(f"dp must be ({L}, {n_all}, {Q})")
    out = torch.empty((n_all, L), dtype=torch.int32, device=device)
    nbytes = int(lib().trex_backtrack_workspace_bytes(n_all, L))
    stack = torch.empty(nbytes, dtype=torch.uint8, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    check(lib().trex_backtrack_generic(int(root_node), ptr(rs), ptr(dpt), ptr(bt), n_all,
                                       int(n_leaves), L, Q, ptr(out), ptr(stack), nbytes,
                                       _MAX_BACKTRACK_STEPS, ptr(status), stream_handle(device)))
    if int(status.item()) != 0:
        raise TrexError(TREX_E_TOPOLOGY, "backtrack_sankoff_jit: the DFS over this backtracking "
                        "table does not terminate (the reference would not return)")
    return out


def backtrack_sankoff_jit(root_node, root_state, backtracking_table, n_all: int, n_leaves: int,
                          *, device=None):
    """trex's ``backtrack_sankoff_jit`` (sankoff.py:191-267) for one site:
    bt (n_all, Q, 4), root_state scalar -> int32 (n_all,) reconstructed states."""
    torch = _torch()
    bt = torch.as_tensor(backtracking_table)
    if bt.ndim != 3:
        raise ValueError("backtrack_sankoff_jit takes one site's (n_all, Q, 4) table; "
                         "use vmapped_backtrack for (L, n_all, Q, 4)")
    rs = torch.as_tensor(root_state).reshape(1)
    return vmapped_backtrack(root_node, rs, bt[None], n_all, n_leaves, device=device)[:, 0]
