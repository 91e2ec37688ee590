"""Genes projected from a sparse mapping (tg_sparse.h) on the CPU emulator (same kernel sources): the spot-major image and its order,
the projection bit for bit against the float64 product on exactly representable data at every pattern, gene width, pitch and
alignment of the tables, general floats against the fma-chain bound, bit reproducibility, the tie to the dense projection of the
same engine, project_genes(truncated=True) and the argument errors of the C ABI.  Tables and checks: tests/sparse_project_cases.py;
the same cases run on the GPU in tests/test_gpu_sparse_project.py."""
import pytest

from tests import sparse_project_cases as sc
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


def _id(p):
    return "-".join(str(x) for x in p)


def test_case_tables_cover_every_edge():
    sc.check_case_tables()


@pytest.mark.parametrize("i", range(len(sc.PATTERNS)), ids=[_id(p) for p in sc.PATTERNS])
def test_exact_patterns(sim, i):
    sc.check_exact_pattern(DEV, i)


@pytest.mark.parametrize("aligned", [False, True], ids=["odd-pitch", "aligned"])
@pytest.mark.parametrize("p", sc.WIDTH_PATTERNS, ids=_id)
def test_exact_gene_widths(sim, p, aligned):
    sc.check_exact_widths(DEV, p, aligned)


@pytest.mark.parametrize("p", sc.IMAGE_PATTERNS, ids=_id)
def test_image_order(sim, p):
    sc.check_image_order(DEV, p)


@pytest.mark.parametrize("C,V", sc.FLOAT_CASES)
def test_general_floats_within_the_chain_bound(sim, C, V):
    sc.check_general_floats(DEV, C, V)


def test_bit_reproducibility(sim):
    sc.check_bit_reproducibility(DEV)


def test_tie_to_the_dense_projection(sim):
    sc.check_pipeline_tie(DEV, 300, 5, 257)


def test_public_surface(sim):
    sc.check_public_surface(DEV)


def test_argument_errors(sim):
    sc.check_argument_errors(DEV)
