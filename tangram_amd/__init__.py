"""tangram_amd -- MI355X-native drop-in for the hot path of broadinstitute/Tangram:
`map_cells_to_space` -> `Mapper` / `MapperConstrained` training loop, running in hand-written HIP kernels
behind a C ABI (include/tangram_hip.h).  Importing this package does not import scanpy."""
from .mapping_optimizer import Mapper, MapperConstrained          # noqa: F401
from .mapping_utils import map_cells_to_space, adata_to_cluster_expression, density_priors  # noqa: F401
from . import preprocess                                          # noqa: F401
from .utils import project_genes, compare_spatial_geneexp, score_genes       # noqa: F401
from .gene_score import gene_scores, gene_scores_sharded, GeneScorer, ShardedGeneScorer   # noqa: F401
from .sparse_project import project_sparse, SparseMap             # noqa: F401
from .batched import train_many, MapperBatch                                   # noqa: F401
from .cross_validation import cross_val, cv_data_gen                        # noqa: F401
from . import mapping_parameter_tuning                                      # noqa: F401
from .mapping_parameter_tuning import (pearson_corr, vote_entropy, consensus_entropy, mapping_consistency,   # noqa: F401
                                       train_multiple_Mapper)

__version__ = "0.1.0"
