"""CPU: ``ops`` as a package -- the names callers reach through it, the layering of its family modules, the mirrored
limits its constants derive from, and the ``ops.FUSED_MLP`` switch as ``dense`` reads it."""
import ast
import importlib
import inspect
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS_DIR = os.path.join(ROOT, "deeplearningrecommendationsystem_amd", "ops")
PKG = "deeplearningrecommendationsystem_amd.ops"

# every ``ops.<name>`` and ``from ...ops import <name>`` of the tree (package, tests/, dev/, scripts/, bench.py, compat/)
# when ``ops`` was one file
SURFACE = """
ACT_NONE ACT_RELU ACT_SIGMOID AFM_GRID_ATTENTION AFM_GRID_CROSS AFM_GRID_ITEM_TILE AFM_GRID_MAX_EMBED
AFM_GRID_USER_TILE ALS_ERR_INDEX ALS_ERR_PIVOT ALS_MAX_DIM CF_KNN_MAX_K DEEPFM_GRID_ITEM_TILE
DEEPFM_GRID_USER_TILE DIEN_GRID_ATTENTION DIEN_GRID_EMBED DIEN_GRID_KEEP DIN_GRID_ATTENTION FUSED_MLP FieldSpec
GDCF_MAX_DIM GRAPH_ERR_INDEX GRAPH_MAX_DIM GRAPH_SEGMENT GROUP_MAX_K GraphPlan Head KernelProfiler
LOWRANK_GRID_ITEM_TILE LOWRANK_GRID_USER_TILE Layer NcfCounts NcfProj PNN_GRID_ITEM_TILE PNN_GRID_USER_TILE
RANK_ERR_COUNT RANK_ERR_LENGTH RANK_ERR_OFFSETS RANK_ERR_SURVIVOR RANK_MASK_BITS SCORE_CHUNK SCRATCH_FLOATS
SOFTMAX_FULL_MAX_DIM TOPK_MAX_K WIDEDEEP_GRID_ITEM_TILE WIDEDEEP_GRID_USER_TILE _field_array _lib act_bwd
act_mask_bwd afm_grid_scores afm_grid_supported allpairs_bwd allpairs_fwd als_gram als_gram_workspace_bytes
als_solve_rows als_solve_rows_weighted als_supported biinteract_bwd biinteract_fwd cf_knn cross_bwd cross_fwd
deepfm_grid_scores deepfm_grid_supported dien_grid_hidden dien_grid_supported din_concat_bwd din_concat_fwd
din_grid_pool din_grid_supported din_pool_bwd din_pool_fwd din_scatter_bwd embed_bwd embed_fwd
embed_mlp_head_fwd eval_candidates few_table_rows ffm_fused_bwd ffm_fused_fwd ffm_head_bwd ffm_head_fwd
fields_fm_bwd fields_fm_fwd fm_wide_bwd fm_wide_fwd fold_head_bwd fold_head_fwd gauc_groups gdcf_cols gdcf_rows
graph_plan graph_propagate graph_supported group_rank gru_bwd gru_fused_bwd gru_fused_fwd gru_fwd itemcf_scores
linear_bwd linear_dx_masked linear_dx_scatter linear_fwd linear_fwd_dot linear_group_fwd linear_n1_bwd_masked
lowrank_grid_scores lowrank_grid_supported mf_bwd mf_fwd mlp_bwd mlp_fwd mlp_head_bwd ncf_grid_scores
ncf_grid_supported pairprod_bwd pairprod_fwd pnn_grid_scores pnn_grid_supported rank_filter rank_mask
rank_metrics_lists rank_metrics_scores rows1_scatter rows_sum_act_fwd score_counts set_profiler
softmax_full_cols softmax_full_rows topk_rows usercf_scores widedeep_grid_scores widedeep_grid_supported
zero_grads
""".split()

BASE = {"_call"}                                   # imports no module of the package
SHARED = ("embed", "dense")                        # the families others may import; dense itself imports embed
FAMILIES = {"embed", "dense", "ncf", "grid", "interact", "sequence", "dense_cf", "csr", "evaluate"}


def _modules():
    return sorted(f[:-3] for f in os.listdir(OPS_DIR) if f.endswith(".py") and f != "__init__.py")


def _sibling_imports(name):
    """the modules of the package that ``name`` imports, read off its import statements"""
    tree = ast.parse(open(os.path.join(OPS_DIR, name + ".py")).read())
    found = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.level == 1:
            found.update([node.module.split(".")[0]] if node.module else [a.name for a in node.names])
        elif isinstance(node, ast.ImportFrom) and node.level == 0 and (node.module or "").startswith(PKG + "."):
            found.add(node.module[len(PKG) + 1:].split(".")[0])
        elif isinstance(node, ast.Import):
            found.update(a.name[len(PKG) + 1:].split(".")[0] for a in node.names if a.name.startswith(PKG + "."))
    return found


def test_every_name_in_use_is_reachable_through_the_package():
    ops = importlib.import_module(PKG)
    assert len(SURFACE) == len(set(SURFACE)) == 137
    modules = {name: importlib.import_module(f"{PKG}.{name}") for name in _modules()}
    for name in SURFACE:
        assert hasattr(ops, name), f"ops.{name} is gone"
        obj = getattr(ops, name)
        if inspect.isfunction(obj) or inspect.isclass(obj):
            home = obj.__module__.rsplit(".", 1)[-1]
            assert obj.__module__.startswith(PKG + ".") and getattr(modules[home], name) is obj, name
    assert ops._lib is importlib.import_module("deeplearningrecommendationsystem_amd._lib")
    assert not hasattr(ops, "__all__")
    # one profiler state: the setter the package hands out writes what _timed reads
    prof = object()
    try:
        ops.set_profiler(prof)
        assert modules["_call"]._profiler is prof and modules["_call"]._profiling()
    finally:
        ops.set_profiler(None)
    assert modules["_call"]._profiler is None


def test_the_package_init_holds_re_exports_only():
    tree = ast.parse(open(os.path.join(OPS_DIR, "__init__.py")).read())
    body = tree.body[1:] if isinstance(tree.body[0], ast.Expr) else tree.body
    assert ast.get_docstring(tree) and all(isinstance(node, ast.ImportFrom) for node in body)


def test_family_modules_do_not_import_each_other():
    """read off the import statements: ``_call`` imports no sibling, ``embed`` only ``_call``, ``dense`` only those two,
    every other family only ``_call``, ``embed`` and ``dense`` -- so there is no cycle and each imports alone"""
    assert set(_modules()) == BASE | FAMILIES
    for name in _modules():
        siblings = _sibling_imports(name)
        if name in BASE:
            assert not siblings, (name, siblings)
        elif name == "embed":
            assert siblings <= BASE, (name, siblings)
        elif name == "dense":
            assert siblings <= BASE | {"embed"}, (name, siblings)
        else:
            assert siblings <= BASE | set(SHARED), (name, siblings)
        lines = open(os.path.join(OPS_DIR, name + ".py")).read().count("\n")
        assert lines <= 600, f"ops/{name}.py has {lines} lines"


def test_limits_of_the_header_reach_ops_through_lib_mirrors():
    ops = importlib.import_module(PKG)
    lib = ops._lib
    derived = dict(TOPK_MAX_K="CTR_TOPK_MAX_K", CF_KNN_MAX_K="CTR_CF_KNN_MAX_K", RANK_MAX_ROWS="CTR_RANK_MAX_ROWS",
                   RANK_MASK_BITS="CTR_RANK_MASK_BITS", RANK_ERR_OFFSETS="CTR_RANK_ERR_OFFSETS",
                   RANK_ERR_LENGTH="CTR_RANK_ERR_LENGTH", RANK_ERR_SURVIVOR="CTR_RANK_ERR_SURVIVOR",
                   RANK_ERR_COUNT="CTR_RANK_ERR_COUNT")
    for name, mirror in derived.items():
        assert isinstance(getattr(lib, mirror), int), mirror
        assert getattr(ops, name) == getattr(lib, mirror), name
    assert (ops.TOPK_MAX_K, ops.CF_KNN_MAX_K, ops.RANK_MAX_ROWS, ops.RANK_MASK_BITS) == (4096, 64, 1 << 24, 0xFFFFFFFF)
    assert (ops.RANK_ERR_OFFSETS, ops.RANK_ERR_LENGTH, ops.RANK_ERR_SURVIVOR, ops.RANK_ERR_COUNT) == (1, 2, 4, 8)
    # none of them is written as a literal in the package again
    for name in _modules():
        tree = ast.parse(open(os.path.join(OPS_DIR, name + ".py")).read())
        for node in tree.body:
            if isinstance(node, ast.Assign) and any(isinstance(n, ast.Constant) and isinstance(n.value, int)
                                                    for n in ast.walk(node.value)):
                targets = {t.id for tgt in node.targets for t in ast.walk(tgt) if isinstance(t, ast.Name)}
                assert not targets & set(derived), (name, targets & set(derived))


def test_the_fused_mlp_switch_is_read_from_the_package():
    """``ops.FUSED_MLP = False`` lands on the package object: ``dense`` must consult that, not its own global"""
    ops = importlib.import_module(PKG)
    dense = importlib.import_module(PKG + ".dense")
    layers = [ops.Layer(torch.zeros(8, 8), torch.zeros(8), ops.ACT_RELU) for _ in range(2)]
    x = torch.zeros(1024, 8)
    assert ops.FUSED_MLP is True
    try:
        assert dense._fusable(x, layers) is True
        ops.FUSED_MLP = False
        assert dense._fusable(x, layers) is False
        ops.FUSED_MLP = True
        assert dense._fusable(x, layers) is True
    finally:
        ops.FUSED_MLP = True
    assert dense._fusable(x[:1023], layers) is False and dense._fusable(x, layers[:1]) is False
