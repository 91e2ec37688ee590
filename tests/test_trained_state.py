"""The training step from trained-state logits on every kernel path, on the HIP emulator (CPU; the GPU run of the whole table is
tests/test_gpu_trained_state.py).  Families, checks, bounds and measured values: tests/trained_state_cases.py."""
import pytest

from tests import trained_state_cases as ts
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


CASES = ts.step_cases(gpu=False)


def test_case_tables_cover_every_path():
    from tests.test_gpu_trained_state import CASES as GPU_CASES
    ts.check_case_tables(GPU_CASES, CASES)
    assert {c["path"] for c in CASES} >= {"rowpass256", "tile256", "rowpass512", "clusters", "oracle300"}
    assert callable(test_emulated_spot_shards) and callable(test_emulated_batch)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_emulated_step_from_trained_state(sim, case):
    ts.run_step_case("cpu", case)


def test_emulated_two_products_bit_equal(sim):
    ts.check_two_products("cpu")


def test_emulated_gated_out_cells(sim):
    ts.check_gated_out_cells("cpu")


@pytest.mark.parametrize("variant", ["plain", "constrained"])
def test_emulated_spot_shards(sim, variant):
    ts.check_shards("cpu", variant)


@pytest.mark.parametrize("mode", ["cells", "clusters"])
def test_emulated_batch(sim, mode):
    ts.check_batch("cpu", mode)
