"""The training step from trained-state logits on every kernel path (-m gpu): peaked and underflowing rows, a saturated filter,
a checkpoint at step 300, through the C ABI against the fp64 oracle.  Families, checks, bounds and the values measured on MI355X:
tests/trained_state_cases.py; the CPU twin on the emulator is tests/test_trained_state.py."""
import pytest

from tests import trained_state_cases as ts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = ts.step_cases(gpu=True)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_step_from_trained_state(case):
    ts.run_step_case(DEV, case)


def test_two_products_bit_equal():
    ts.check_two_products(DEV)


def test_gated_out_cells():
    ts.check_gated_out_cells(DEV)


@pytest.mark.parametrize("variant", ["plain", "constrained"])
def test_spot_shards(variant):
    ts.check_shards(DEV, variant)


@pytest.mark.parametrize("mode", ["cells", "clusters"])
def test_batch(mode):
    ts.check_batch(DEV, mode)
