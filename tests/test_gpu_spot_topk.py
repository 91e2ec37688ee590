"""Each spot's k most probable cells without the dense mapping, on the MI355X (-m gpu): the tables and checks of
tests/spot_topk_cases.py, the same ones tests/test_spot_topk.py runs on the emulator.  Every comparison of lists is exact (cells equal,
values bit for bit against the dense result of the same handle); the column sums are held to 1 ulp of the fp64 sum of the dense
values."""
import pytest

from tests import spot_topk_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(table):
    return ["-".join(str(x) for x in c) for c in table]


def test_limits_mirror_the_kernel_header():
    sc.check_limits()


@pytest.mark.parametrize("C,K,V,precision", sc.SPOT_CASES, ids=_ids(sc.SPOT_CASES))
def test_spot_edges_against_the_dense_result(C, K, V, precision):
    sc.check_spot_case(DEV, C, K, V, precision)


@pytest.mark.parametrize("C,k", sc.CELL_CASES, ids=_ids(sc.CELL_CASES))
def test_cell_and_slab_edges(C, k):
    sc.check_cell_case(DEV, C, k)


def test_lists_do_not_depend_on_the_split_into_slabs():
    sc.check_split_independence(DEV)


@pytest.mark.parametrize("layout", sc.TIE_LAYOUTS)
def test_ties(layout):
    sc.check_ties(DEV, layout)


@pytest.mark.parametrize("case", sc.FILTER_CASES)
def test_filter_of_constrained_mode(case):
    sc.check_filter(DEV, case)


def test_filter_needs_a_constrained_handle():
    sc.check_filter_needs_a_constrained_handle(DEV)


def test_column_sums_and_mass():
    sc.check_mass(DEV)


def test_training_state_is_undisturbed():
    sc.check_undisturbed(DEV)


@pytest.mark.parametrize("world,V,k", sc.SHARD_CASES, ids=_ids(sc.SHARD_CASES))
def test_spot_shards(world, V, k):
    sc.check_shards(DEV, world, V, k)


def test_argument_errors():
    sc.check_argument_errors(DEV)


def test_train_spot_top_k():
    sc.check_train_spot_top_k(DEV)


@pytest.mark.parametrize("mode", ["cells", "constrained"])
def test_map_cells_to_space_spot_top_k(mode):
    sc.check_map_cells_to_space_spot_top_k(DEV, mode)
