"""Gene projection from the resident mapping on every handle kind (-m gpu): every kernel path, precision and filter setting, gene-
block, pitch and cell-count edges, the trained state, the routes and the front end, per gene column against fp64 from the handle's
own logits.  Reference, bound, checks and the values measured on MI355X: tests/project_genes_cases.py; the CPU twin on the emulator
is tests/test_project_genes.py."""
import pytest

from tests import project_genes_cases as pg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KIND_CASES = pg.kind_cases(gpu=True)
EDGE_CASES = [(K, filt, precision) for K in pg.EDGE_KS for filt, precision in pg.EDGE_CONFIGS]
CELL_CASES = [(C, filt, precision) for C in pg.CELL_COUNTS for filt, precision in pg.CELL_CONFIGS]
PRECISIONS = ("fp32", "bf16x3", "bf16")


@pytest.mark.parametrize("case", KIND_CASES, ids=[c["id"] for c in KIND_CASES])
def test_kind_precision_filter(case):
    pg.run_kind_case(DEV, case)


@pytest.mark.parametrize("K,filt,precision", EDGE_CASES)
def test_gene_block_edges(K, filt, precision):
    pg.check_gene_block_edges(DEV, K, filt, precision)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("K", [7, 8])
def test_pitch_and_alignment(K, precision):
    pg.check_pitch_and_alignment(DEV, K, precision)


@pytest.mark.parametrize("C,filt,precision", CELL_CASES)
def test_cell_count_edges(C, filt, precision):
    pg.check_cell_count(DEV, C, filt, precision)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("C", pg.LARGE_LOGIT_CELLS)
def test_padding_rows_large_logits(C, precision):
    pg.check_padding_rows_large_logits(DEV, C, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_single_cell_column(precision):
    pg.check_single_cell_column(DEV, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_trained_state(precision):
    pg.check_trained_state(DEV, precision)


@pytest.mark.parametrize("constrained", [False, True], ids=["mapper", "constrained"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_handle_untouched(precision, constrained):
    pg.check_handle_untouched(DEV, precision, constrained)


def test_csr_route():
    pg.check_csr_route(DEV)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("world", [2, 3])
def test_spot_shards(world, precision):
    pg.check_shards(DEV, world, precision)


def test_batch_member():
    pg.check_batch_member(DEV)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_front_end(precision):
    pg.check_front_end(DEV, precision)
