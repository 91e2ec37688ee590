"""Batches of mappings with spatial terms on the CPU emulator (the emulated C ABI): the cases of tests/batched_spatial_cases.py.
The device runs the same table in tests/test_gpu_batched_spatial.py."""
import pytest

from tests import batched_spatial_cases as cases
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


@pytest.mark.parametrize("case", cases.case_table(False), ids=lambda c: c[0])
def test_spatial_batch_has_the_bits_of_each_mapping_alone_emulated(sim, case):
    cases.run_case("cpu", case)


@pytest.mark.parametrize("name", sorted(cases.REFUSALS))
def test_spatial_batch_refusals_emulated(sim, name):
    cases.REFUSALS[name]("cpu")


def test_tuning_trial_with_spatial_terms_goes_through_one_batch_emulated(sim):
    cases.tuning_trial_case("cpu")


def test_batch_key_of_spatial_mappers():
    """Mappers with spatial terms get a key; different sets of terms (or cell-type counts) get different keys; the key reads the
    cell-type count only where the islands term is on."""
    from types import SimpleNamespace
    from tangram_amd import batched

    class Mapper:
        def __init__(self, n_types=None, C=4200, V=1100, **lam):
            cfg = dict(lambda_neighborhood_g1=0, lambda_ct_islands=0, lambda_getis_ord=0, lambda_moran=0, lambda_geary=0, pipeline_bands=0,
                       lambda_r=0, lambda_l1=0, lambda_l2=0, beta1=0.9, beta2=0.999, tile_size=0, fwd_splits=0)
            cfg.update(lam)
            if n_types is not None:
                cfg["n_cell_types"] = n_types
            self._engine = SimpleNamespace(C=C, K=249, V=V, cfg=SimpleNamespace(**cfg), precision="bf16x3", device="cuda:0", _torch_stream=None)
            self._sharded = None

    class MapperConstrained(Mapper):
        pass

    key = batched._batch_key
    plain, nb = key(Mapper()), key(Mapper(lambda_neighborhood_g1=0.96))
    assert plain is not None and nb is not None and plain != nb
    assert nb == key(Mapper(lambda_neighborhood_g1=0.5))                                   # lambda VALUES are per mapping
    ct18, ct19 = key(Mapper(18, lambda_ct_islands=0.17)), key(Mapper(19, lambda_ct_islands=0.17))
    assert None not in (ct18, ct19) and ct18 != ct19 and ct18 != nb
    assert key(Mapper(18, lambda_neighborhood_g1=0.96)) == nb                              # no islands term: the count does not matter
    getis, moran = key(Mapper(lambda_getis_ord=0.5)), key(Mapper(lambda_moran=0.5))
    assert None not in (getis, moran) and getis != moran
    assert key(Mapper(lambda_getis_ord=0.5, lambda_geary=1.0)) not in (getis, moran)
    tuner = dict(lambda_neighborhood_g1=0.96, lambda_ct_islands=0.17, lambda_getis_ord=0.5)
    assert key(Mapper(18, **tuner)) == key(Mapper(18, **tuner)) and key(Mapper(18, **tuner)) not in (nb, ct18, getis)
    assert key(MapperConstrained(lambda_neighborhood_g1=0.96)) is None                    # the terms exist in Mapper only
    assert key(Mapper(18, C=26431, V=9852, **tuner)) is None                               # above BATCH_MAX_ELEMENTS, like plain mappers
    assert key(Mapper(18, V=16385, C=100, **tuner)) is None and key(Mapper(18, pipeline_bands=2, **tuner)) is None
