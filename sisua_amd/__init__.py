"""sisua_amd -- MI355X-native (gfx950) implementation of the SISUA VAE training
hot path behind the reference's SingleCellModel.fit/predict/encode surface.

Python host code -> ctypes -> libsisua_hip.so (hand-written HIP kernels).  There
is no CPU fallback: without the built library and a visible MI355X every
compute entry point raises `SmxError`.
"""
from sisua_amd._hip import SmxError  # noqa: F401
from sisua_amd.boosting import GradientBoostingClassifier, importance_matrix  # noqa: F401
from sisua_amd.communities import louvain, modularity  # noqa: F401
from sisua_amd.config import ModelConfig, NetConf, RVmeta  # noqa: F401
from sisua_amd.distributions import correlations_from_sums, protein_operands  # noqa: F401
from sisua_amd.label_threshold import ProbabilisticEmbedding  # noqa: F401
from sisua_amd.logistic import LogisticRegression  # noqa: F401
from sisua_amd.metrics import correlation_list, dci_scores, marker_correlations, marker_scores  # noqa: F401
from sisua_amd.minibatch_kmeans import MiniBatchKMeans  # noqa: F401
from sisua_amd.mixture import GaussianMixture  # noqa: F401
from sisua_amd.mutual_info import mutual_information  # noqa: F401
from sisua_amd.neighbors import PCA, TSNE, UMAP, umap  # noqa: F401
from sisua_amd.rank_groups import rank_genes_groups, rank_genes_groups_logreg  # noqa: F401

__version__ = "0.1.0"
