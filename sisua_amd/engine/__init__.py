"""sisua_amd.engine: the one namespace for everything that crosses the C-ABI (include/sisua_hip.h).

Thin, mechanical wrappers: they convert numpy arrays to pointers, check arguments so that a refusal never asks for the device, and raise
`SmxError` on any non-zero status.  All arithmetic happens in libsisua_hip.so.  Importing this package needs no GPU and loads nothing.

One module per kernel family; this file only re-exports, by explicit name, so callers and tests keep reaching (and patching) every wrapper
as `engine.<name>`:

  _args        array -> pointer converters and the argument checks more than one family shares
  _model       `Engine`, the owner of one `smx_model`, and what builds its configuration
  _kernels     single launches of the training step by themselves (tests)
  _correlate   gene x protein correlation sums        _cluster     silhouette, Lloyd's k-means
  _gmm         the 1-D and the full-covariance mixture  _prep        count-matrix preprocessing
  _neighbors   PCA, kNN, UMAP graph and layout, t-SNE _mi          mutual information
  _groups      group moments and rank sums            _mbkmeans    mini-batch k-means
  _logreg      logistic regression                    _louvain     Louvain communities, modularity
  _gbt         gradient-boosted trees

A new feature's wrappers go into a new `_feature.py` beside these (the underscore keeps a module from shadowing an exported name).  Its
names are then added to the imports below and to tests/golden/engine_api.json, which tests/test_engine_namespace_host.py holds this
namespace to.
"""
from sisua_amd._hip import SmxError, check, smx_config, smx_metrics
from sisua_amd.engine._args import (_csr3, _csr_ptrs, _dp, _f32, _fp, _fps, _ip, _label_ids, _matrix_ptrs, _ptr, _sparse)
from sisua_amd.engine._cluster import k_cluster_kmeans, k_cluster_silhouette
from sisua_amd.engine._correlate import _col_operands, _col_outputs, k_col_correlate, k_col_rank2
from sisua_amd.engine._gbt import (GBT_MAX_BINS, GBT_MAX_CELLS, GBT_MAX_CLASSES, GBT_MAX_DEPTH, GBT_MAX_GENES, GBT_MAX_PASS, GBT_MAX_Q,
                                   GBT_MAX_RESIDENT, _gbt_input, _gbt_tree_params, gbt_init_raw, k_gbt_bin, k_gbt_decision, k_gbt_fit,
                                   k_gbt_grow)
from sisua_amd.engine._gmm import (ILL_DEFINED_COVARIANCE, _gmm_matrix, gmm_n_train, k_gmm1d_fit, k_gmm1d_predict, k_gmm_full_fit,
                                   k_gmm_full_predict)
from sisua_amd.engine._groups import (MOMENT_MAX_ACC, MOMENT_MAX_GROUPS, RANK_MAX_CELLS, RANK_MAX_GROUPS, _group_labels, k_group_moments,
                                      k_group_ranksums)
from sisua_amd.engine._kernels import (OPT_CARRIERS, _bn_slabs, _bn_vec, _scvi_layout, k_adam, k_bn_bwd, k_bn_fwd, k_count_llk, k_gemm,
                                       k_head_fused, k_head_fused_stress, k_label_loss, k_noise, k_opt, k_opt_carrier, k_row_select, k_scvi_head_bwd,
                                       k_scvi_head_fwd, k_scvi_head_train)
from sisua_amd.engine._logreg import (LR_MAX_CLASSES, LR_MAX_GENES, LR_MAX_RESIDENT, _lr_input, _lr_params, _lr_penalty, k_logreg_decision,
                                      k_logreg_eval, k_logreg_fit)
from sisua_amd.engine._louvain import (LOUVAIN_MAX_ENTRIES, LOUVAIN_MAX_VERTICES, _louvain_graph, k_louvain, k_modularity,
                                       louvain_table_degree)
from sisua_amd.engine._mbkmeans import (MBK_MAX_CLUSTERS, MBK_MAX_GENES, MBK_MAX_RESIDENT, MBK_MAX_SEED_ROWS, MBK_MAX_TRIALS, _mbk_centres,
                                        _mbk_input, k_mbkmeans_predict, k_mbkmeans_seed, k_mbkmeans_step)
from sisua_amd.engine._mi import MI_MAX_CELLS, MI_MAX_NEIGHBORS, _mi_check, _mi_cols, _mi_tables, k_mi_cells, mutual_info
from sisua_amd.engine._model import (STREAM_DEC_DROPOUT, STREAM_ENC_DROPOUT, STREAM_ENCL_DROPOUT, STREAM_EPS_L, STREAM_EPS_Z,
                                     STREAM_INPUT_DROPOUT, _SCHED_TARGETS, Engine, _check_u16, _tril_scale, gene_indices, make_smx_config)
from sisua_amd.engine._neighbors import (KNN_MAX_D, KNN_MAX_K, PCA_MAX_COMPONENTS, PCA_MAX_GENES, TSNE_MAX_COMPONENTS, UMAP_MAX_COMPONENTS,
                                         UMAP_MAX_EPOCHS, UMAP_MAX_NEGATIVES, _pca_input, _tsne_problem, _umap_problem, k_knn, k_knn_umap,
                                         k_pca_cov, k_pca_project, k_tsne_affinities, k_tsne_fit, k_tsne_gradient, k_umap_layout, k_umap_pow)
from sisua_amd.engine._prep import PREP_FUNCS, _prep_input, k_prep_apply, k_prep_stats
