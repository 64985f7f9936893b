"""Tree topologies: trex adjacency conventions -> device plans.

Adjacency orientation follows trex: ``adj[i, j] == 1`` means node ``i`` is a
child of node ``j`` (src/trex/utils/types.py:30-35).  Leaves are
0..n_leaves-1, internal nodes n_leaves..n_all-1, the root is n_all-1.
"""

from __future__ import annotations


import numpy as np

from ._lib import TREX_PLAN_HEADER_INTS, check, lib


def children_from_adjacency(adj, *, drop_root_self_loop: bool = True) -> np.ndarray:
    """trex's child lists for every node.

    ``jnp.where(adj[:, node] == 1, size=2, fill_value=-1)[0]``
    (src/trex/sankoff.py:60) applied after run_sankoff zeroes ``adj[-1, -1]``
    (sankoff.py:141; ``drop_root_self_loop=False`` is run_dp called directly,
    which does not).  ``adj``: (n_all, n_all) or (B, n_all, n_all).
    Returns int32 (B, n_all, 2).
    """
    a = np.asarray(adj)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[1] != a.shape[2]:
        raise ValueError(f"adjacency must be (n_all, n_all) or (B, n_all, n_all), got {a.shape}")
    mask = a == 1
    if drop_root_self_loop:
        mask[:, -1, -1] = False
    B, n_all, _ = mask.shape
    # cumulative count down each column; first hit has count 1, second count 2
    cnt = np.cumsum(mask, axis=1)
    out = np.full((B, n_all, 2), -1, dtype=np.int32)
    for k in (1, 2):
        hit = mask & (cnt == k)
        has = hit.any(axis=1)  # (B, n_all)
        row = hit.argmax(axis=1)
        out[:, :, k - 1] = np.where(has, row, -1)
    return out


def create_balanced_binary_tree(n_leaves: int) -> np.ndarray:
    """Adjacency of trex's balanced tree (src/trex/evals/benchmark.py:781-791)."""
    n_anc = n_leaves - 1
    n_total = n_leaves + n_anc
    adj = np.zeros((n_total, n_total), dtype=np.float32)
    adj[np.arange(n_leaves), n_leaves + np.arange(n_leaves) // 2] = 1
    adj[n_leaves + np.arange(n_anc - 1), n_leaves + (np.arange(n_anc - 1) + n_leaves) // 2] = 1
    return adj


def random_topologies(B: int, n_leaves: int, seed: int) -> np.ndarray:
    """Random binary topologies as child lists (B, n_all, 2).

    Coalescent merge: two random active nodes join under new node n_leaves+k,
    so every child id is lower than its parent (trex's post-order numbering).
    """
    rng = np.random.default_rng(seed)
    n_all = 2 * n_leaves - 1
    out = np.full((B, n_all, 2), -1, dtype=np.int32)
    for b in range(B):
        active = list(range(n_leaves))
        for k in range(n_leaves - 1):
            i, j = rng.choice(len(active), size=2, replace=False)
            ci, cj = active[i], active[j]
            parent = n_leaves + k
            lo, hi = min(ci, cj), max(ci, cj)
            out[b, parent] = (lo, hi)  # jnp.where returns rows ascending
            active = [x for t, x in enumerate(active) if t not in (i, j)] + [parent]
    return out


def adjacency_from_children(children: np.ndarray) -> np.ndarray:
    """Inverse of children_from_adjacency for well-formed child lists."""
    ch = np.asarray(children)
    if ch.ndim == 2:
        ch = ch[None]
    B, n_all, _ = ch.shape
    adj = np.zeros((B, n_all, n_all), dtype=np.float32)
    for b in range(B):
        for node in range(n_all):
            for c in ch[b, node]:
                if c >= 0:
                    adj[b, c, node] = 1
    return adj


def apply_nni(children, v: int, k: int) -> np.ndarray:
    """Child lists (n_all, 2) of the NNI neighbour (v, k) of one tree.

    ``v`` is an internal node other than the root, u its parent, s its
    sibling and (a0, a1) = ``children[v]`` in stored order; the move swaps
    a_k with s, so v gets {s, a_(1-k)} and u gets {a_k, v} (the move of
    ``SankoffEngine.nni_scores``' entry ``[v - n_leaves, k]``).  The result
    is valid under trex's numbering: leaf ids are unchanged, internal nodes
    are renumbered in post-order by a DFS from the root that visits children
    in ascending id order, so every child id is below its parent's and the
    root is n_all - 1; each pair is stored ascending.
    """
    ch = np.asarray(children)
    if ch.ndim != 2 or ch.shape[1] != 2:
        raise ValueError(f"children must be (n_all, 2), got {ch.shape}")
    n_all = ch.shape[0]
    nl = (n_all + 1) // 2
    if not (nl <= v < n_all - 1) or k not in (0, 1):
        raise ValueError(f"move ({v}, {k}): v must be internal and not the root, k 0 or 1")
    kids = {node: [int(ch[node, 0]), int(ch[node, 1])] for node in range(nl, n_all)}
    parents = [u for u, pair in kids.items() if v in pair]
    if len(parents) != 1:
        raise ValueError(f"node {v} does not have exactly one parent")
    u = parents[0]
    s = kids[u][0] if kids[u][1] == v else kids[u][1]
    a = kids[v]
    kids[v] = [s, a[1 - k]]
    kids[u] = [a[k], v]
    return _renumber(kids, n_all - 1, {c: c for c in range(nl)})


def _renumber(kids, root, leaf_id, key=None) -> np.ndarray:
    """Child lists of the tree ``kids`` (internal node -> its two children;
    every other node is a leaf with the new id ``leaf_id[node]``): internal
    nodes numbered in post-order by a DFS from ``root`` that visits children
    in ascending ``key`` order (default: the node itself), each pair stored
    ascending, the root last."""
    key = key or (lambda node: node)
    nl = len(leaf_id)
    n_all = 2 * nl - 1
    new_id = dict(leaf_id)
    out = np.full((n_all, 2), -1, dtype=np.int32)
    nxt = nl
    stack = [(root, False)]
    while stack:
        node, done = stack.pop()
        if node not in kids:
            continue
        if not done:
            if len(stack) > 2 * n_all:
                raise ValueError("children do not describe a tree")
            stack.append((node, True))
            for c in sorted(kids[node], key=key, reverse=True):
                stack.append((c, False))
            continue
        if nxt >= n_all:
            raise ValueError("children do not describe a tree")
        new_id[node] = nxt
        out[nxt] = sorted(new_id[c] for c in kids[node])
        nxt += 1
    if nxt != n_all:
        raise ValueError("children do not describe a tree")
    return out


def _proper_kids(children):
    """{internal node: [c0, c1]} of one proper rooted binary tree's child
    lists (what trex_nni_plan_build accepts); ValueError otherwise."""
    ch = np.asarray(children)
    if ch.ndim != 2 or ch.shape[1] != 2 or ch.shape[0] < 3 or ch.shape[0] % 2 == 0:
        raise ValueError(f"children must be (n_all, 2) with n_all odd and >= 3, got {ch.shape}")
    n_all = ch.shape[0]
    nl = (n_all + 1) // 2
    kids, seen = {}, set()
    for node in range(nl, n_all):
        c0, c1 = int(ch[node, 0]), int(ch[node, 1])
        if not (0 <= c0 < node and 0 <= c1 < node) or c0 == c1 or c0 in seen or c1 in seen:
            raise ValueError(f"children are not a proper rooted binary tree (node {node})")
        seen.update((c0, c1))
        kids[node] = [c0, c1]
    return kids, nl, n_all


def insert_leaf(children, x: int) -> np.ndarray:
    """Child lists (n_all + 2, 2) of one tree after a new leaf is attached on
    the edge above node ``x`` (``x = n_all - 1``: a new root above the old
    one) -- the tree of ``SankoffEngine.attach_scores``' entry ``[x]``.

    Old leaf ids are unchanged and the new leaf is ``n_leaves`` (the old
    count).  Internal nodes are renumbered by ``apply_nni``'s rule; the DFS
    orders children by their ids in the grown tree before renumbering: old
    leaves keep theirs, the new leaf is ``n_leaves``, old internal node v is
    v + 1, and the new internal node takes x's place among its parent's
    children.
    """
    kids, nl, n_all = _proper_kids(children)
    if not 0 <= x < n_all:
        raise ValueError(f"x must be a node id in [0, {n_all}), got {x}")
    up = lambda c: c if c < nl else c + 1  # noqa: E731
    grown = {up(node): [up(c) for c in pair] for node, pair in kids.items()}
    w = "w"
    x_up = up(int(x))
    grown[w] = [x_up, nl]
    root = up(n_all - 1)
    if x_up == root:
        root = w
    else:
        for pair in grown.values():
            if pair is not grown[w] and x_up in pair:
                pair[pair.index(x_up)] = w
    key = lambda node: (x_up, 1) if node == w else (node, 0)  # noqa: E731
    return _renumber(grown, root, {c: c for c in range(nl + 1)}, key)


def apply_spr(children, v: int, x: int) -> np.ndarray:
    """Child lists (n_all, 2) of the SPR neighbour (v, x) of one tree -- the
    tree of ``SankoffEngine.spr_scores``' entry ``[v, x]``.

    ``v`` is any node but the root, u its parent and s its sibling.  Prune: u
    disappears and s takes its place (u the root: s is the root of what
    remains).  Regraft: a new node w with children {x, v} goes on the edge
    above ``x``, any node of the remaining tree (x the remaining root: w is
    the new root); ``x = s`` gives the tree back.  Internal nodes are
    renumbered by ``apply_nni``'s rule, the DFS ordering children by their old
    ids, w taking x's place among its parent's children (as in
    ``insert_leaf``).  ValueError for v the root, x in subtree(v) or x = u.
    """
    kids, nl, n_all = _proper_kids(children)
    v, x = int(v), int(x)
    if not 0 <= v < n_all - 1:
        raise ValueError(f"v must be a node other than the root, in [0, {n_all - 1}), got {v}")
    if not 0 <= x < n_all:
        raise ValueError(f"x must be a node id in [0, {n_all}), got {x}")
    u = next(node for node, pair in kids.items() if v in pair)
    s = kids[u][0] if kids[u][1] == v else kids[u][1]
    below, todo = set(), [v]
    while todo:
        node = todo.pop()
        below.add(node)
        todo.extend(kids.get(node, ()))
    if x in below or x == u:
        raise ValueError(f"move ({v}, {x}): x must not be in subtree(v) nor v's parent {u}")
    del kids[u]
    root = n_all - 1
    if u == root:
        root = s
    else:
        g = next(pair for pair in kids.values() if u in pair)
        g[g.index(u)] = s
    w = "w"
    if x == root:
        root = w
    else:
        p = next(pair for pair in kids.values() if x in pair)
        p[p.index(x)] = w
    kids[w] = [x, v]
    key = lambda node: (x, 1) if node == w else (node, 0)  # noqa: E731
    return _renumber(kids, root, {c: c for c in range(nl)}, key)


def relabel_leaves(children, perm) -> np.ndarray:
    """Child lists of one tree with leaf j renamed ``perm[j]`` (a permutation
    of the leaf ids); internal nodes are renumbered by ``apply_nni``'s rule,
    the DFS ordering children by their new leaf id / old internal id."""
    kids, nl, n_all = _proper_kids(children)
    perm = np.asarray(perm)
    if perm.shape != (nl,) or sorted(perm.tolist()) != list(range(nl)):
        raise ValueError(f"perm must be a permutation of 0..{nl - 1}")
    leaf_id = {j: int(perm[j]) for j in range(nl)}
    return _renumber(kids, n_all - 1, leaf_id, lambda node: leaf_id.get(node, node))


def to_newick(children, names=None, lengths=None, support=None, fmt="%g") -> str:
    """One proper rooted binary tree's child lists (n_all, 2) as a Newick
    string, ``(...);``.  Children are written in stored order.  ``names``:
    the leaves' labels (default: their ids), written as given.  ``lengths``
    (n_all,), indexed by node id as ``SankoffEngine.edge_changes``' outputs:
    ``:length`` behind every node but the root.  ``support`` (n_int,), what
    ``clade_support`` returns: the internal nodes' labels, the root's
    included.  Numbers are written with ``fmt``.  ValueError for child lists
    that are not a proper rooted binary tree (``insert_leaf``'s rule)."""
    kids, nl, n_all = _proper_kids(children)
    if names is None:
        names = [str(x) for x in range(nl)]
    if len(names) != nl:
        raise ValueError(f"names must have {nl} entries, got {len(names)}")
    if lengths is not None:
        lengths = np.asarray(lengths, dtype=np.float64)
        if lengths.shape != (n_all,):
            raise ValueError(f"lengths must be ({n_all},), got {lengths.shape}")
    if support is not None:
        support = np.asarray(support, dtype=np.float64)
        if support.shape != (n_all - nl,):
            raise ValueError(f"support must be ({n_all - nl},), got {support.shape}")
    text = {}
    for node in range(n_all):  # children come before their parents
        if node < nl:
            s = str(names[node])
        else:
            s = "(" + ",".join(text.pop(c) for c in kids[node]) + ")"
            if support is not None:
                s += fmt % support[node - nl]
        if lengths is not None and node != n_all - 1:
            s += ":" + fmt % lengths[node]
        text[node] = s
    return text[n_all - 1] + ";"


def _build_plan(name: str, what: str, children: np.ndarray, B: int, n_all: int,
                *info) -> np.ndarray:
    """trex_<name>_ints, an int32 buffer of that size, trex_<name>_build into
    it (``info``: the builder's trailing output arrays; ``what``: the plan in
    words).  TrexError when the builder refuses the trees."""
    L = lib()
    n = getattr(L, f"trex_{name}_ints")(B, n_all)
    if n <= 0:
        raise ValueError(f"bad {what} shape B={B} n_all={n_all}")
    buf = np.zeros(n, dtype=np.int32)
    check(getattr(L, f"trex_{name}_build")(children.ctypes.data, B, n_all, buf.ctypes.data,
                                           *(a.ctypes.data for a in info)))
    return buf


def device_copy(cache: dict, host: np.ndarray, device):
    """``host`` as a device tensor, copied once per device (``cache``: the
    copies made so far, by device)."""
    import torch

    key = str(device)
    if key not in cache:
        cache[key] = torch.from_numpy(host).to(device)
    return cache[key]


class TreePlan:
    """A batch of topologies compiled by the host planner (trex_plan_build)."""

    def __init__(self, children: np.ndarray):
        ch = np.ascontiguousarray(children, dtype=np.int32)
        if ch.ndim == 2:
            ch = ch[None]
        if ch.ndim != 3 or ch.shape[2] != 2:
            raise ValueError(f"children must be (B, n_all, 2), got {ch.shape}")
        self.B, self.n_all, _ = ch.shape
        self.n_leaves = (self.n_all + 1) // 2
        self.n_int = self.n_all - self.n_leaves
        info = np.zeros(4, dtype=np.int32)
        self.host = _build_plan("plan", "plan", ch, self.B, self.n_all, info)
        self.children = ch
        # info[0]: stack depth | (lane-program slots + 1) << 16; the C calls
        # take the whole word
        self.slot_word = int(info[0])
        self.n_slots = self.slot_word & 0xFFFF
        self.lane_slots = ((self.slot_word >> 16) & 0xFF) - 1
        self.backtrack_ok = int(info[1])
        self.n_dag_nodes = int(info[2])
        self.n_unreached = int(info[3])
        self._dev = {"plan": {}, "nni": {}, "attach": {}, "spr": {}}
        self._search_host = {}  # the search plans built so far, by kind

    # -- the search plans (trex_{nni,attach,spr}_plan_build), built on first use --
    def _search_plan(self, kind: str, device=None):
        """The NNI / attach / SPR plan (include/trex_hip.h) as int32: the host
        array, built once, or with ``device`` its copy there (cached per
        device).  TrexError (TREX_E_TOPOLOGY) when a tree of the batch is not
        a proper rooted binary tree of at least 3 leaves."""
        host = self._search_host.get(kind)
        if host is None:
            if kind == "spr":
                from ._lib import has_spr

                if not has_spr():
                    raise RuntimeError(f"{lib()._name} has no SPR entry points "
                                       "(trex_spr_plan_build, trex_sankoff_spr_w, "
                                       "trex_sankoff_sets_spr_w): rebuild libtrexhip.so")
            what = {"nni": "NNI plan", "attach": "attach plan", "spr": "SPR plan"}[kind]
            host = self._search_host[kind] = _build_plan(f"{kind}_plan", what, self.children,
                                                         self.B, self.n_all)
        return host if device is None else device_copy(self._dev[kind], host, device)

    nni_host = property(lambda self: self._search_plan("nni"), doc="The NNI plan, int32.")
    attach_host = property(lambda self: self._search_plan("attach"), doc="The attach plan, int32.")
    spr_host = property(lambda self: self._search_plan("spr"), doc="The SPR plan, int32.")

    def nni_device(self, device):
        """The NNI plan as an int32 device tensor (cached per device)."""
        return self._search_plan("nni", device)

    def attach_device(self, device):
        """The attach plan as an int32 device tensor (cached per device)."""
        return self._search_plan("attach", device)

    def spr_device(self, device):
        """The SPR plan as an int32 device tensor (cached per device)."""
        return self._search_plan("spr", device)

    @property
    def nni_table(self) -> np.ndarray:
        """int32 (B, n_int - 1, 4): node ids (u, a0, a1, s) of v = n_leaves + e
        -- v's parent, its two children in stored order and its sibling --
        decoded from the NNI plan.  Move (v, k) swaps a_k with s."""
        ni = self.n_int
        per = 8 * ni - 4
        body = self.nni_host[TREX_PLAN_HEADER_INTS:].reshape(self.B, per)
        mv = body[:, 4 * ni:].reshape(self.B, ni - 1, 4)
        out = np.empty_like(mv)
        out[:, :, 0] = mv[:, :, 0] + self.n_leaves
        d = mv[:, :, 1:]
        out[:, :, 1:] = np.where((d >> 24) == 1, d & 0xFFFF, (d & 0xFFFF) + self.n_leaves)
        return out

    @classmethod
    def from_adjacency(cls, adj) -> "TreePlan":
        return cls(children_from_adjacency(adj))

    def device(self, device):
        """The plan as an int32 device tensor (cached per device)."""
        return device_copy(self._dev["plan"], self.host, device)

    @property
    def fwd_steps(self) -> np.ndarray:
        """(B, n_int, 4) encoded forward steps (see trex_common.h)."""
        o = TREX_PLAN_HEADER_INTS
        return self.host[o:o + self.B * self.n_int * 4].reshape(self.B, self.n_int, 4)
