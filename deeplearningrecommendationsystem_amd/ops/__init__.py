"""Host-side wrappers over the C ABI (include/ctrhip.h), one module per kernel family.

PyTorch is plumbing here: it owns device memory and the stream; every function passes raw pointers + leading
dimensions to libctrhip and enqueues on torch's current stream.  2-D operands may be column slices of a wider buffer
(stride(1) must be 1), which is how the reference's ``torch.cat`` calls disappear: producers write straight into the
consumer's operand.

``_call`` holds the call frame, the profiler and the shared checks; a family module imports it and, at most, ``embed``
and ``dense``.  Callers use the names below as ``ops.<name>``; ``ops.FUSED_MLP`` is read from here at call time.
"""
from .. import _lib
from .._lib import ACT_NONE, ACT_RELU, ACT_SIGMOID
from ._call import SCRATCH_FLOATS, KernelProfiler, set_profiler
from .embed import FieldSpec, _field_array, embed_bwd, embed_fwd
from .dense import (FUSED_MLP, Head, Layer, act_bwd, act_mask_bwd, cross_bwd, cross_fwd, embed_mlp_head_fwd, fold_head_bwd,
                    fold_head_fwd, linear_bwd, linear_fwd, mlp_bwd, mlp_fwd, mlp_head_bwd, zero_grads)
from .ncf import NcfCounts, NcfProj, few_table_rows, mf_bwd, mf_fwd, rows_sum_act_fwd
from .grid import (AFM_GRID_ATTENTION, AFM_GRID_CROSS, AFM_GRID_ITEM_TILE, AFM_GRID_MAX_EMBED, AFM_GRID_USER_TILE,
                   DEEPFM_GRID_HIDDEN, DEEPFM_GRID_ITEM_TILE, DEEPFM_GRID_USER_TILE, DIEN_GRID_ATTENTION, DIEN_GRID_EMBED,
                   DIEN_GRID_KEEP, DIN_GRID_ATTENTION, DIN_GRID_EMBED, LOWRANK_GRID_ITEM_TILE, LOWRANK_GRID_MAX_RANK,
                   LOWRANK_GRID_USER_TILE, PNN_GRID_CROSS, PNN_GRID_HIDDEN, PNN_GRID_ITEM_TILE, PNN_GRID_MAX_EMBED,
                   PNN_GRID_USER_TILE, WIDEDEEP_GRID_HIDDEN, WIDEDEEP_GRID_ITEM_TILE, WIDEDEEP_GRID_USER_TILE,
                   afm_grid_scores, afm_grid_supported, deepfm_grid_scores, deepfm_grid_supported, dien_grid_hidden,
                   dien_grid_supported, din_grid_pool, din_grid_supported, lowrank_grid_scores, lowrank_grid_supported,
                   ncf_grid_scores, ncf_grid_supported, pnn_grid_scores, pnn_grid_supported, widedeep_grid_scores,
                   widedeep_grid_supported)
from .interact import (ALLPAIRS_MAX_VECTORS, allpairs_bwd, allpairs_fwd, biinteract_bwd, biinteract_fwd, ffm_fused_bwd,
                       ffm_fused_fwd, ffm_head_bwd, ffm_head_fwd, fields_fm_bwd, fields_fm_fwd, fm_wide_bwd, fm_wide_fwd,
                       pairprod_bwd, pairprod_fwd, rows1_scatter)
from .sequence import (din_concat_bwd, din_concat_fwd, din_pool_bwd, din_pool_fwd, din_scatter_bwd, gru_bwd, gru_fused_bwd,
                       gru_fused_fwd, gru_fwd, linear_dx_masked, linear_dx_scatter, linear_fwd_dot, linear_group_fwd,
                       linear_n1_bwd_masked)
from .dense_cf import (CF_KNN_MAX_K, GDCF_MAX_DIM, SOFTMAX_FULL_MAX_DIM, SOFTMAX_FULL_MAX_SPLITS, TOPK_MAX_K, cf_knn,
                       gdcf_cols, gdcf_rows, itemcf_scores, softmax_full_cols, softmax_full_rows, topk_rows, usercf_scores)
from .csr import (ALS_ERR_INDEX, ALS_ERR_PIVOT, ALS_MAX_DIM, GRAPH_ERR_INDEX, GRAPH_ERR_PLAN, GRAPH_MAX_DIM, GRAPH_SEGMENT,
                  GraphPlan, als_gram, als_gram_workspace_bytes, als_solve_rows, als_solve_rows_weighted, als_supported,
                  graph_plan, graph_propagate, graph_supported, graph_workspace_bytes)
from .evaluate import (GAUC_SLAB, GAUC_SMALL, GROUP_MAX_K, RANK_ERR_COUNT, RANK_ERR_LENGTH, RANK_ERR_OFFSETS,
                       RANK_ERR_SURVIVOR, RANK_MASK_BITS, RANK_MAX_ROWS, SCORE_CHUNK, eval_candidates, gauc_groups,
                       group_rank, rank_filter, rank_mask, rank_metrics_lists, rank_metrics_scores, score_counts)
