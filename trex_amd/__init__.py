"""trex_amd -- MI355X-native engine for trex's batched Sankoff / tree-cost path.

Mirrors the public functions of maraxen/trex ``trex.sankoff`` (and, as they
land, ``trex.tree``) on top of hand-written HIP kernels for gfx950 in
``libtrexhip.so`` (C ABI: include/trex_hip.h).  See DESIGN.md.
"""

from ._lib import LIB_PATH, TrexError, lib  # noqa: F401
from .leafsets import encode_alignment, sets_from_codes  # noqa: F401
from .sankoff import (  # noqa: F401
    EdgeChanges,
    SankoffEngine,
    backtrack_sankoff_jit,
    leaf_codes,
    run_dp,
    run_sankoff,
    sankoff_value_and_grad,
    vectorized_dp,
    vmapped_backtrack,
)
from .search import (  # noqa: F401
    BootstrapResult,
    HillClimbResult,
    RatchetResult,
    SearchResult,
    StepwiseResult,
    bootstrap_search,
    bootstrap_weights,
    clade_support,
    compress_sites,
    describe_trees,
    nni_hill_climb,
    parsimony_ratchet,
    parsimony_search,
    spr_hill_climb,
    stepwise_addition,
)
from .topology import (  # noqa: F401
    TreePlan,
    apply_nni,
    apply_spr,
    children_from_adjacency,
    create_balanced_binary_tree,
    insert_leaf,
    random_topologies,
    relabel_leaves,
    to_newick,
)

__all__ = [
    "LIB_PATH", "TrexError", "lib", "SankoffEngine", "leaf_codes", "run_sankoff", "run_dp",
    "vectorized_dp", "backtrack_sankoff_jit", "vmapped_backtrack",
    "sankoff_value_and_grad", "TreePlan", "children_from_adjacency",
    "create_balanced_binary_tree", "random_topologies", "apply_nni", "nni_hill_climb",
    "HillClimbResult", "insert_leaf", "relabel_leaves", "stepwise_addition", "StepwiseResult",
    "parsimony_search", "SearchResult", "compress_sites", "parsimony_ratchet", "RatchetResult",
    "bootstrap_weights", "bootstrap_search", "BootstrapResult", "clade_support",
    "sets_from_codes", "encode_alignment", "apply_spr", "spr_hill_climb",
    "EdgeChanges", "describe_trees", "to_newick",
]
