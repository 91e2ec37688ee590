"""Gene projection from the resident mapping on every handle kind, on the HIP emulator (CPU; the GPU run of the whole table is
tests/test_gpu_project_genes.py).  Reference, bound, checks and measured values: tests/project_genes_cases.py."""
import pytest

from tests import project_genes_cases as pg
from tests.hipsim.build_sim import build_sim


@pytest.fixture(scope="module")
def sim():
    from tangram_amd import _capi
    path = build_sim()
    if path is None:
        pytest.skip("host clang not available to build the emulator")
    _capi._install_library_for_tests(path)
    yield path
    _capi._install_library_for_tests(None)


KIND_CASES = pg.kind_cases(gpu=False)


def test_case_tables():
    from tests import test_gpu_project_genes as gpu
    pg.check_kind_tables(gpu.KIND_CASES, KIND_CASES)
    assert gpu.EDGE_CASES == EDGE_CASES and gpu.CELL_CASES == CELL_CASES and gpu.PRECISIONS == PRECISIONS
    assert {K for K, _, _ in EDGE_CASES} == {1, 7, 8, 130} and pg.edge_widths(8) == [1, 7, 8, 9, 16, 17, 23] and pg.edge_widths(1) == [1, 2, 3]
    assert {C for C, _, _ in CELL_CASES} == {33, 63, 64, 65, 127, 128, 129}
    assert ("unfiltered", "bf16") in {(f, p) for _, f, p in EDGE_CASES} & {(f, p) for _, f, p in CELL_CASES}


@pytest.mark.parametrize("case", KIND_CASES, ids=[c["id"] for c in KIND_CASES])
def test_emulated_kind_precision_filter(sim, case):
    pg.run_kind_case("cpu", case)


EDGE_CASES = [(K, filt, precision) for K in pg.EDGE_KS for filt, precision in pg.EDGE_CONFIGS]


@pytest.mark.parametrize("K,filt,precision", EDGE_CASES)
def test_emulated_gene_block_edges(sim, K, filt, precision):
    pg.check_gene_block_edges("cpu", K, filt, precision)


PRECISIONS = ("fp32", "bf16x3", "bf16")


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("K", [7, 8])
def test_emulated_pitch_and_alignment(sim, K, precision):
    pg.check_pitch_and_alignment("cpu", K, precision)


CELL_CASES = [(C, filt, precision) for C in pg.CELL_COUNTS for filt, precision in pg.CELL_CONFIGS]


@pytest.mark.parametrize("C,filt,precision", CELL_CASES)
def test_emulated_cell_count_edges(sim, C, filt, precision):
    pg.check_cell_count("cpu", C, filt, precision)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("C", pg.LARGE_LOGIT_CELLS)
def test_emulated_padding_rows_large_logits(sim, C, precision):
    pg.check_padding_rows_large_logits("cpu", C, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_emulated_single_cell_column(sim, precision):
    pg.check_single_cell_column("cpu", precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_emulated_trained_state(sim, precision):
    pg.check_trained_state("cpu", precision)


@pytest.mark.parametrize("constrained", [False, True], ids=["mapper", "constrained"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_emulated_handle_untouched(sim, precision, constrained):
    pg.check_handle_untouched("cpu", precision, constrained)


def test_emulated_csr_route(sim):
    pg.check_csr_route("cpu")


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("world", [2, 3])
def test_emulated_spot_shards(sim, world, precision):
    pg.check_shards("cpu", world, precision)


def test_emulated_batch_member(sim):
    pg.check_batch_member("cpu")


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_emulated_front_end(sim, precision):
    pg.check_front_end("cpu", precision)
