"""Each cell's k most probable spots without the dense mapping (tg_topk.h), on the CPU emulator (same kernel sources): indices and
value bits against the dense result of the same handle at every row length of the table, ties, constrained mode, the merge kernel
alone, spot shards, the undisturbed training state, argument errors and the public surface.  Tables and checks:
tests/topk_cases.py; the same cases run on the GPU in tests/test_gpu_topk.py.  Every reference is exact: no tolerance.

Each of these edits, tried alone on the emulator, fails tests of this module:
    the tie-break flipped (the spot index packed without its complement, so the larger spot wins): test_ties, both layouts;
    the chunk carry dropped (the list restarted at every chunk but the last): test_row_topk_against_the_dense_result[3-5-8193-bf16x3]
        and [3-5-16387-bf16x3], test_ties[across-the-chunk-boundary];
    the `v < V` guard widened to the pitch Vp (load and key): test_row_topk_against_the_dense_result at V = 1, 2, 63, 65 (both C),
        test_ties, test_constrained_mode_is_the_unfiltered_softmax, test_spot_shards at V = 10 and 131 (indices >= V, or past the shard);
    the pad ordering of the merge inverted (a pad packed as the largest word): every test_merge_kernel case, test_spot_shards[3-10-5]
        and [3-131-64].
"""
import pytest

from tests import topk_cases as tc
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
    """The tables hold every row length, list length and shard shape the checks are there for."""
    tc.check_case_tables()


def test_limits_mirror_the_kernel_header(sim):
    tc.check_limits()


@pytest.mark.parametrize("C,K,V,precision", tc.KERNEL_CASES, ids=_ids(tc.KERNEL_CASES))
def test_row_topk_against_the_dense_result(sim, C, K, V, precision):
    tc.check_kernel_case(DEV, C, K, V, precision)


@pytest.mark.parametrize("layout", tc.TIE_LAYOUTS)
def test_ties(sim, layout):
    tc.check_ties(DEV, layout)


def test_constrained_mode_is_the_unfiltered_softmax(sim):
    tc.check_constrained(DEV)


@pytest.mark.parametrize("n_in,k", tc.MERGE_CASES, ids=_ids(tc.MERGE_CASES))
def test_merge_kernel(sim, n_in, k):
    tc.check_merge(DEV, n_in, k)


@pytest.mark.parametrize("world,V,k", tc.SHARD_CASES, ids=_ids(tc.SHARD_CASES))
def test_spot_shards(sim, world, V, k):
    tc.check_shards(DEV, world, V, k)


def test_training_state_is_undisturbed(sim):
    tc.check_undisturbed(DEV)


def test_argument_errors(sim):
    tc.check_argument_errors(DEV)


def test_train_top_k(sim):
    tc.check_train_top_k(DEV)


@pytest.mark.parametrize("mode", ["cells", "constrained"])
def test_map_cells_to_space_top_k(sim, mode):
    tc.check_map_cells_to_space_top_k(DEV, mode)
