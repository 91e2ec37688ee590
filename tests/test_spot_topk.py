"""Each spot's k most probable cells without the dense mapping (tg_spot_topk.h), on the CPU emulator (same kernel sources): cells and
value bits against the dense result of the same handle at every spot count, cell count and slab edge of the tables, the split into
slabs, ties, the filter of constrained mode, column sums and mass, the undisturbed training state, spot shards, argument errors and
the public surface.  Tables and checks: tests/spot_topk_cases.py; the same cases run on the GPU in tests/test_gpu_spot_topk.py.
Every comparison of lists is exact; the column sums are held to 1 ulp of the fp64 sum of the dense values."""
import pytest

from tests import spot_topk_cases as sc
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


def _ids(table):
    return ["-".join(str(x) for x in c) for c in table]


def test_case_tables_cover_every_edge():
    """The tables hold every spot count, cell count, list length and shard shape the checks are there for."""
    sc.check_case_tables()


def test_limits_mirror_the_kernel_header(sim):
    sc.check_limits()


@pytest.mark.parametrize("C,K,V,precision", sc.SPOT_CASES, ids=_ids(sc.SPOT_CASES))
def test_spot_edges_against_the_dense_result(sim, C, K, V, precision):
    sc.check_spot_case(DEV, C, K, V, precision)


@pytest.mark.parametrize("C,k", sc.CELL_CASES, ids=_ids(sc.CELL_CASES))
def test_cell_and_slab_edges(sim, C, k):
    sc.check_cell_case(DEV, C, k)


def test_lists_do_not_depend_on_the_split_into_slabs(sim):
    sc.check_split_independence(DEV)


@pytest.mark.parametrize("layout", sc.TIE_LAYOUTS)
def test_ties(sim, layout):
    sc.check_ties(DEV, layout)


@pytest.mark.parametrize("case", sc.FILTER_CASES)
def test_filter_of_constrained_mode(sim, case):
    sc.check_filter(DEV, case)


def test_filter_needs_a_constrained_handle(sim):
    sc.check_filter_needs_a_constrained_handle(DEV)


def test_column_sums_and_mass(sim):
    sc.check_mass(DEV)


def test_training_state_is_undisturbed(sim):
    sc.check_undisturbed(DEV)


@pytest.mark.parametrize("world,V,k", sc.SHARD_CASES, ids=_ids(sc.SHARD_CASES))
def test_spot_shards(sim, world, V, k):
    sc.check_shards(DEV, world, V, k)


def test_argument_errors(sim):
    sc.check_argument_errors(DEV)


def test_train_spot_top_k(sim):
    sc.check_train_spot_top_k(DEV)


@pytest.mark.parametrize("mode", ["cells", "constrained"])
def test_map_cells_to_space_spot_top_k(sim, mode):
    sc.check_map_cells_to_space_spot_top_k(DEV, mode)
