"""The clusters-mode kernels (tg_sc_forward, tg_sc_backward, their batched twins, tg_prep_ssmall) at every cluster count and tile
edge (-m gpu), through the C ABI against the fp64 oracle.  Sweeps, checks, bounds and the values measured on MI355X:
tests/clusters_cases.py; the CPU twin on the emulator is tests/test_clusters_kernels.py."""
import pytest

from tests import clusters_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = cc.step_cases(gpu=True)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_clusters_step(case):
    cc.run_step_case(DEV, case)


@pytest.mark.parametrize("C,K,V,lambda_g2", cc.BATCH_CASES, ids=[f"C{c[0]}-g2-{c[3]}" for c in cc.BATCH_CASES])
def test_batched_twins(C, K, V, lambda_g2):
    cc.check_batch(DEV, C, K, V, lambda_g2)


def test_path_predicate():
    cc.check_path_predicate(DEV)
