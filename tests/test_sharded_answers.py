"""Gene scores over spot shards on the CPU emulator (same kernel sources): tg_gene_scores_merge, gene_scores_sharded and
score_genes(distributed=True) with the ranks as threads of one process.  Tables and checks: tests/sharded_answers_cases.py; the same
cases run on the GPU in tests/test_gpu_sharded_answers.py."""
import pytest

from tests import sharded_answers_cases as sa
from tests.hipsim.build_sim import build_sim

DEV = "cpu"


@pytest.fixture(scope="module")
def sim():
    from tangram_amd import _capi
    path = build_sim()
    if path is None:
        pytest.skip("host clang not available to build the emulator")
    _capi._install_library_for_tests(path)
    yield path
    _capi._install_library_for_tests(None)


def test_case_tables_cover_every_edge():
    sa.check_case_tables()


@pytest.mark.parametrize("V,world", sa.PARTITIONS)
def test_exact_moments_and_scores_over_shards(sim, V, world):
    sa.check_exact(DEV, V, world)


@pytest.mark.parametrize("V,world", sa.PARTITIONS)
def test_general_floats_within_the_derived_bounds(sim, V, world):
    sa.check_general_floats(DEV, V, world)


def test_a_column_that_is_zero_on_one_rank_only(sim):
    sa.check_zero_columns(DEV)


def test_one_rank_returns_the_unsharded_bits(sim):
    sa.check_one_rank(DEV)


def test_merge_argument_errors(sim):
    sa.check_merge_arguments(DEV)


@pytest.mark.parametrize("world,V", sa.E2E)
def test_score_genes_distributed(sim, world, V):
    sa.check_score_genes_distributed(DEV, world, V)


def test_agreement_tables_cover_every_edge():
    sa.check_agreement_tables()


@pytest.mark.parametrize("case", sa.AGREE_CASES, ids=[c["id"] for c in sa.AGREE_CASES])
def test_agreement_over_shards_against_the_gathered_result(sim, case):
    sa.check_agreement_case(DEV, case)


@pytest.mark.parametrize("world,V,R", sa.SVAL_CASES)
def test_gene_expr_consistency_over_shards(sim, world, V, R):
    sa.check_agreement_with_s_val(DEV, world, V, R)


def test_agreement_refusals(sim):
    sa.check_agreement_refusals(DEV)
