"""Genes projected from a sparse mapping, on the MI355X (-m gpu): the tables and checks of tests/sparse_project_cases.py, the same
ones tests/test_sparse_project.py runs on the emulator; the tie to the dense projection at 4 096 cells x 1 500 spots."""
import pytest

from tests import sparse_project_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _id(p):
    return "-".join(str(x) for x in p)


@pytest.mark.parametrize("i", range(len(sc.PATTERNS)), ids=[_id(p) for p in sc.PATTERNS])
def test_exact_patterns(i):
    sc.check_exact_pattern(DEV, i)


@pytest.mark.parametrize("aligned", [False, True], ids=["odd-pitch", "aligned"])
@pytest.mark.parametrize("p", sc.WIDTH_PATTERNS, ids=_id)
def test_exact_gene_widths(p, aligned):
    sc.check_exact_widths(DEV, p, aligned)


@pytest.mark.parametrize("p", sc.IMAGE_PATTERNS, ids=_id)
def test_image_order(p):
    sc.check_image_order(DEV, p)


@pytest.mark.parametrize("C,V", sc.FLOAT_CASES)
def test_general_floats_within_the_chain_bound(C, V):
    sc.check_general_floats(DEV, C, V)


def test_bit_reproducibility():
    sc.check_bit_reproducibility(DEV)


def test_tie_to_the_dense_projection():
    sc.check_pipeline_tie(DEV, 4096, 64, 1500)


def test_public_surface():
    sc.check_public_surface(DEV)


def test_argument_errors():
    sc.check_argument_errors(DEV)
