"""The clusters-mode kernels at every cluster count and tile edge, on the HIP emulator (CPU; the GPU run of the whole table is
tests/test_gpu_clusters_kernels.py).  Sweeps, checks, bounds and measured values: tests/clusters_cases.py."""
import pytest

from tests import clusters_cases as cc
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


CASES = cc.step_cases(gpu=False)


def test_case_table_names_every_edge():
    from tests.test_gpu_clusters_kernels import CASES as GPU_CASES
    cc.check_case_tables(GPU_CASES, CASES)
    assert callable(test_emulated_batched_twins) and callable(test_emulated_path_predicate)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_emulated_clusters_step(sim, case):
    cc.run_step_case("cpu", case)


@pytest.mark.parametrize("C,K,V,lambda_g2", cc.BATCH_CASES, ids=[f"C{c[0]}-g2-{c[3]}" for c in cc.BATCH_CASES])
def test_emulated_batched_twins(sim, C, K, V, lambda_g2):
    cc.check_batch("cpu", C, K, V, lambda_g2)


def test_emulated_path_predicate(sim):
    cc.check_path_predicate("cpu")
