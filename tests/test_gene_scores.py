"""Per-gene scores (tg_score.h) on the CPU emulator (same kernel sources): moments and score bit for bit against NumPy float64 on
exactly representable data at every height, width, pitch and alignment of the tables, general floats against the derived bounds,
position independence and reproducibility, degenerate columns, the argument errors of the C ABI, compare_spatial_geneexp on dense
and CSR inputs, score_genes tied to its own block projections and to compare_spatial_geneexp(project_genes(...)) on every route,
and the reference's train-score invariant.  Tables and checks: tests/gene_score_cases.py; the same cases run on the GPU in
tests/test_gpu_gene_scores.py."""
import pytest

from tests import gene_score_cases as gc
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


def test_case_tables_cover_every_edge(sim):
    gc.check_case_tables(DEV)


@pytest.mark.parametrize("aligned", [False, True], ids=["odd-pitch", "aligned"])
@pytest.mark.parametrize("n_spots", gc.SPOT_SIZES)
def test_exact_moments_and_scores(sim, n_spots, aligned):
    gc.check_exact(DEV, n_spots, aligned)


@pytest.mark.parametrize("n_spots,n_genes", gc.FLOAT_CASES)
def test_general_floats_within_the_derived_bounds(sim, n_spots, n_genes):
    gc.check_general_floats(DEV, n_spots, n_genes)


def test_position_independence_and_reproducibility(sim):
    gc.check_position_independence(DEV)


def test_degenerate_columns(sim):
    gc.check_degenerate_columns(DEV)


def test_argument_errors(sim):
    gc.check_argument_errors(DEV)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
def test_compare_spatial_geneexp(sim, sparse):
    gc.check_compare_surface(DEV, sparse)


@pytest.mark.parametrize("route", gc.TIE_ROUTES)
def test_score_genes_ties(sim, route):
    gc.check_score_genes_tie(DEV, route)


def test_score_genes_refusals(sim):
    gc.check_score_genes_refusals(DEV)


def test_reference_holds_the_train_score_invariant():
    gc.check_reference_invariant()


def test_train_score_invariant(sim):
    gc.check_train_score_invariant(DEV)


def test_route_errors_are_the_same_in_project_genes_and_score_genes(sim):
    gc.check_route_errors(DEV)


def test_all_zero_sparse_block(sim):
    gc.check_all_zero_sparse_block(DEV)


def test_unnormalised_dense_mapping(sim, golden_dir):
    gc.check_unnormalised_dense_mapping(DEV, golden_dir)
