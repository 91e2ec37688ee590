"""Per-gene scores (tg_score.h) on the MI355X: the checks of tests/test_gene_scores.py on cuda:0 -- the same tables, the same exact
data bit for bit, the same derived bounds (tests/gene_score_cases.py)."""
import pytest
import torch

from tests import gene_score_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def hip_library():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from tangram_amd import _capi
    _capi._install_library_for_tests(None)
    assert not _capi.is_emulated()
    yield


def test_case_tables_cover_every_edge():
    gc.check_case_tables(DEV)


@pytest.mark.parametrize("aligned", [False, True], ids=["odd-pitch", "aligned"])
@pytest.mark.parametrize("n_spots", gc.SPOT_SIZES)
def test_exact_moments_and_scores(n_spots, aligned):
    gc.check_exact(DEV, n_spots, aligned)


@pytest.mark.parametrize("n_spots,n_genes", gc.FLOAT_CASES)
def test_general_floats_within_the_derived_bounds(n_spots, n_genes):
    gc.check_general_floats(DEV, n_spots, n_genes)


def test_position_independence_and_reproducibility():
    gc.check_position_independence(DEV)


def test_degenerate_columns():
    gc.check_degenerate_columns(DEV)


def test_argument_errors():
    gc.check_argument_errors(DEV)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
def test_compare_spatial_geneexp(sparse):
    gc.check_compare_surface(DEV, sparse)


@pytest.mark.parametrize("route", gc.TIE_ROUTES)
def test_score_genes_ties(route):
    gc.check_score_genes_tie(DEV, route)


def test_score_genes_refusals():
    gc.check_score_genes_refusals(DEV)


def test_train_score_invariant():
    gc.check_train_score_invariant(DEV)


def test_route_errors_are_the_same_in_project_genes_and_score_genes():
    gc.check_route_errors(DEV)


def test_all_zero_sparse_block():
    gc.check_all_zero_sparse_block(DEV)


def test_unnormalised_dense_mapping(golden_dir):
    gc.check_unnormalised_dense_mapping(DEV, golden_dir)
