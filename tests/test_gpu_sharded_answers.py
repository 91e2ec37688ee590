"""Gene scores over spot shards on the MI355X: the checks of tests/test_sharded_answers.py on cuda:0, the ranks as threads of one
process on the one device -- the same tables, the same exact data bit for bit, the same derived bounds
(tests/sharded_answers_cases.py)."""
import pytest
import torch

from tests import sharded_answers_cases as sa

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def hip_library():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from tangram_amd import _capi
    _capi._install_library_for_tests(None)
    assert not _capi.is_emulated()
    yield


@pytest.mark.parametrize("V,world", sa.PARTITIONS)
def test_exact_moments_and_scores_over_shards(V, world):
    sa.check_exact(DEV, V, world)


@pytest.mark.parametrize("V,world", sa.PARTITIONS)
def test_general_floats_within_the_derived_bounds(V, world):
    sa.check_general_floats(DEV, V, world)


def test_a_column_that_is_zero_on_one_rank_only():
    sa.check_zero_columns(DEV)


def test_one_rank_returns_the_unsharded_bits():
    sa.check_one_rank(DEV)


def test_merge_argument_errors():
    sa.check_merge_arguments(DEV)


@pytest.mark.parametrize("world,V", sa.E2E)
def test_score_genes_distributed(world, V):
    sa.check_score_genes_distributed(DEV, world, V)


@pytest.mark.parametrize("case", sa.AGREE_CASES, ids=[c["id"] for c in sa.AGREE_CASES])
def test_agreement_over_shards_against_the_gathered_result(case):
    sa.check_agreement_case(DEV, case)


@pytest.mark.parametrize("world,V,R", sa.SVAL_CASES)
def test_gene_expr_consistency_over_shards(world, V, R):
    sa.check_agreement_with_s_val(DEV, world, V, R)


def test_agreement_refusals():
    sa.check_agreement_refusals(DEV)
