"""Spot shards on 8, 9, 12 and 16 ranks on the CPU emulator (same kernel sources): the second trip of every eight-wide per-rank
loop.  Tables, checks, measured values and the perturbation table: tests/many_rank_cases.py; the training step, the spatial blocks
and the empty block run on the GPU too (tests/test_gpu_many_ranks.py), the peer transport at 9 and 16 ranks runs here only."""
import pytest

from tests import many_rank_cases as mr
from tests.hipsim.build_sim import build_sim

DEV = "cpu"
STEP_CASES = mr.step_cases()
PEER_STEPS = [(w, v, p, f) for w in mr.PEER_WORLDS for v, p in mr.PEER_VARIANTS for f in (True, False)]


@pytest.fixture(scope="module")
def sim():
    from tangram_amd import _capi
    path = build_sim()
    if path is None:
        pytest.skip("host clang not available to build the emulator")
    _capi._install_library_for_tests(path)
    yield path
    _capi._install_library_for_tests(None)


def test_case_tables_pin_the_worlds_and_the_shard_widths():
    mr.check_case_tables()


@pytest.mark.parametrize("case", STEP_CASES, ids=[c["id"] for c in STEP_CASES])
def test_training_step_on_many_shards(sim, case):
    mr.check_step_case(DEV, case)


def test_spatial_terms_on_nine_blocks(sim):
    mr.check_spatial_blocks(DEV)


def test_empty_block_is_refused_on_every_rank(sim):
    mr.check_empty_block(DEV)


@pytest.fixture(scope="module")
def peer_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("peer"))


@pytest.mark.parametrize("n", mr.PEER_EXCHANGE_N)
@pytest.mark.parametrize("world", mr.PEER_WORLDS)
def test_peer_exchange_all_reduce_and_gather(sim, peer_dir, world, n):
    mr.check_peer_exchange(mr.peer_processes(world, sim, peer_dir), world, n)


@pytest.mark.parametrize("world,variant,precision,fused", PEER_STEPS,
                         ids=[f"world{w}-{v}-{p}-{'fused' if f else 'exchange-kernels'}" for w, v, p, f in PEER_STEPS])
def test_peer_transport_equals_the_callback_transport(sim, peer_dir, world, variant, precision, fused):
    mr.check_peer_step(mr.peer_processes(world, sim, peer_dir), world, variant, precision, fused)
