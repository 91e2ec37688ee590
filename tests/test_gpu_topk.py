"""Each cell's k most probable spots without the dense mapping, on the MI355X (-m gpu): the tables and checks of tests/topk_cases.py,
the same ones tests/test_topk.py runs on the emulator.  Every comparison is exact (indices equal, values bit for bit against the
dense result of the same handle)."""
import pytest

from tests import topk_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(table):
    return ["-".join(str(x) for x in c) for c in table]


def test_limits_mirror_the_kernel_header():
    tc.check_limits()


@pytest.mark.parametrize("C,K,V,precision", tc.KERNEL_CASES, ids=_ids(tc.KERNEL_CASES))
def test_row_topk_against_the_dense_result(C, K, V, precision):
    tc.check_kernel_case(DEV, C, K, V, precision)


@pytest.mark.parametrize("layout", tc.TIE_LAYOUTS)
def test_ties(layout):
    tc.check_ties(DEV, layout)


def test_constrained_mode_is_the_unfiltered_softmax():
    tc.check_constrained(DEV)


@pytest.mark.parametrize("n_in,k", tc.MERGE_CASES, ids=_ids(tc.MERGE_CASES))
def test_merge_kernel(n_in, k):
    tc.check_merge(DEV, n_in, k)


@pytest.mark.parametrize("world,V,k", tc.SHARD_CASES, ids=_ids(tc.SHARD_CASES))
def test_spot_shards(world, V, k):
    tc.check_shards(DEV, world, V, k)


def test_training_state_is_undisturbed():
    tc.check_undisturbed(DEV)


def test_argument_errors():
    tc.check_argument_errors(DEV)


def test_train_top_k():
    tc.check_train_top_k(DEV)


@pytest.mark.parametrize("mode", ["cells", "constrained"])
def test_map_cells_to_space_top_k(mode):
    tc.check_map_cells_to_space_top_k(DEV, mode)
