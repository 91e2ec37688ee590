"""Spot shards on 8, 9, 12 and 16 ranks on the MI355X (-m gpu): the tables and checks of tests/many_rank_cases.py, the same ones
tests/test_many_ranks.py runs on the emulator -- the training step over the callback transport (ranks are threads of this process,
so one process has the GPU open), the spatial terms on nine blocks and the empty block.

The peer transport's second trip (tg_peer_exchange, tg_link_sum, tg_link_sum2, tg_link_get8 and the peer form of the merge at 9 and
16 ranks) is covered on the emulator only: nine or more ranks polling inside kernels on one shared card is not a deployment form
(deployment is one rank per GPU) and would put more waiting kernels on the card's few hardware queues than anything measured so far.
tests/test_gpu_zz_peer_processes.py keeps the 2- to 8-process cases.

Measured on the MI355X: the 42 tests of this module take 6 s together (the slowest 1.2 s, the first, which loads the library); the
largest errors per precision stand in the docstring of tests/many_rank_cases.py."""
import pytest

from tests import many_rank_cases as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP_CASES = mr.step_cases()


@pytest.mark.parametrize("case", STEP_CASES, ids=[c["id"] for c in STEP_CASES])
def test_training_step_on_many_shards(case):
    mr.check_step_case(DEV, case)


def test_spatial_terms_on_nine_blocks():
    mr.check_spatial_blocks(DEV)


def test_empty_block_is_refused_on_every_rank():
    mr.check_empty_block(DEV)
