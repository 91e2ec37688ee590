"""The validation metrics of Mapper._val_loss_fn (tg_mapper_validate) on every kernel path against the fp64 formula
oracle.tangram_oracle.validation_metrics (-m gpu).  The case table, what a case checks and the bounds are those of the CPU twin on
the emulator, tests/test_validation_metrics.py (parity_common.validation_cases(True): the same edges, three cell tiles where the
edge is about genes, and the 256-tile all-genes width K = 5 888 of tests/test_gpu_wide_genes.py); the coverage test of both tables
lives there.

No MI355X measurement of this table has been taken yet: the figures below are the emulator's (the same kernel sources on the CPU,
tests/test_validation_metrics.py) and are to be replaced by the GPU's with the first GPU run of this module, which prints them per
case (pytest -s, "validation case <id>: ...").  Largest |library - fp64 formula| on the emulator:
    precision                bound   total     gene_sim  weighted  entropy
    fp32 (+ clusters mode)   1e-5    9.6e-8    4.3e-8    5.1e-8    1.2e-7
    bf16x3 (+ two products)  1e-5    4.5e-7    2.0e-7    3.3e-7    3.0e-7
    bf16                     1e-3    1.7e-4    1.1e-4    1.0e-4    4.4e-5
    spot shards (bf16x3)     1e-5    4.5e-8    2.7e-8    3.0e-8    7.8e-8
"""
import pytest

from tests import parity_common as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = pc.validation_cases(True)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_validation_metrics_against_fp64_formula(case):
    pc.run_validation_case(DEV, case)


UNDISTURBED = [
    ("clusters-path", dict(C=18, K=20, V=70)),
    ("rowpass-256-threads", dict(C=300, K=8, V=300)),
    ("rowpass-512-threads", dict(C=40, K=8, V=4100)),
    ("adam-update", dict(C=70, K=8, V=16400)),
    ("lambda-g2-0", dict(C=300, K=8, V=300, lambda_g2=0.0)),
    ("pipeline-bands-3", dict(C=420, K=16, V=150, pipeline_bands=3)),
    ("pipeline-bands-3-two-steps-per-call", dict(C=420, K=16, V=150, pipeline_bands=3, calls=(2, 2))),
]


@pytest.mark.parametrize("kw", [k for _, k in UNDISTURBED], ids=[i for i, _ in UNDISTURBED])
def test_validation_leaves_training_alone(kw):
    pc.validation_undisturbed_case(DEV, **kw)


def test_constrained_handle_refuses_validation():
    pc.validation_refused_case(DEV)


# (world, K, rank whose block holds no spot of gene 0): 1 010 spots are ragged on 2 and on 3 shards; 300 genes are two voxstat parts
SHARDS = [(2, 48, None), (3, 300, None), (2, 300, None), (3, 48, None), (3, 48, 1),
          # nine and sixteen shards: the second trip of the eight-wide per-rank loops (tests/many_rank_cases.py); the rank without a
          # spot of gene 0 is one of the second trip
          (9, 300, None), (16, 300, 11)]


@pytest.mark.parametrize("world,K,empty", SHARDS, ids=[f"world{w}-genes{K}" + ("-gene-empty-on-a-shard" if e is not None else "") for w, K, e in SHARDS])
def test_validation_on_spot_shards(world, K, empty):
    pc.validation_shards_case(DEV, "bf16x3", world, 400, K, 1010, empty_gene_on_rank=empty)
