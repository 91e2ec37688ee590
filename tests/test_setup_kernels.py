"""The set-up and pre-processing kernels of tg_setup.h at every loop boundary, on the CPU emulator (same kernel sources): the CSR
gathers value for value, the row sums, the density prior and the cluster sums against math.fsum rounded once, the bf16-exactness
verdict against the general path, the device initialiser against its formula.  Tables and checks: tests/setup_cases.py; the same
cases run on the GPU in tests/test_gpu_setup_kernels.py.

Largest error per family on the emulator (bound in brackets):
    row sums, dense and CSR            0.4999 ulp  (0.5 + 1e-6); a float32 running sum of the 5000-value rows: 45.9 ulp dense, 40.8 CSR
    density vs r / sum(r)              0.49998 ulp (0.5 + 1e-6)
    density vs exact rowsum / total    1.39 ulp    (1.5), at n = 1023; 1.21 at n = 5000, 1.22 at n = 20 000
    cluster sums and means             0.49995 ulp (0.5 + 1e-6)
    initialiser vs formula             1.5e-6      (1e-5): direct 1.5e-6, narrow 5.3e-7, index above 2^32 4.0e-7, plane 1.1e-6
The exactness check finds 2^-133 (a denormal bf16 holds) exact and 2^-140 not, and +inf exact; none of the three is pinned.

Each of these edits of tg_setup.h, tried alone, fails tests of this module: the stride 256 -> 512 in tg_csr_gather_cols
(test_csr_gather_columns, 20 cases); `double s` -> `float s` in tg_row_sums (test_row_sums_dense from 65 columns on, both
test_row_sums_csr); either `i < n` loop of tg_normalize_total cut to one trip (test_density[1025], [5000], [20000]); K + 1 -> K in the
element count of tg_s_exact_check (the S-last-element, S-last-row-first-column, d_source-last-row and ct-last-row-last-column cases);
`>> 27` -> `>> 26` in tg_counter_normal (every test_init_normal_*).
"""
import pytest

from tests import setup_cases as sc
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


def _ids(table):
    return ["-".join(str(x) for x in c) for c in table]


def test_case_tables_cover_every_edge():
    """The tables hold every boundary value the kernels' loops have: they cannot be thinned without this test failing."""
    sc.check_case_tables()


def test_reference_helpers():
    """The references' own tools: ulp32 at the binade edges, the 64-bit counter against a NumPy uint64 evaluation."""
    import numpy as np
    assert sc.ulp32(1.0) == 2.0 ** -23 and sc.ulp32(1.9999999) == 2.0 ** -23 and sc.ulp32(2.0) == 2.0 ** -22 and sc.ulp32(0.75) == 2.0 ** -24
    assert sc.ulp_error(np.float32(1.0) + np.float32(2.0 ** -23), 1.0) == 1.0
    seed64 = sc.mixed_seed(42, 1)
    idx = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 12345, 200000 * 50000 - 1], dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = idx * np.uint64(0x9E3779B97F4A7C15) + (np.uint64(seed64) ^ np.uint64(0xD1B54A32D192ED03)) * np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(30); z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27); z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    for i, zi in zip(idx, z):
        assert sc.counter_bits(seed64, int(i)) == (int(zi) >> 40, int(zi) & 0xFFFFFF)


@pytest.mark.parametrize("matrix,sel,pad", sc.GATHER_CASES, ids=_ids(sc.GATHER_CASES))
def test_csr_gather_columns(sim, matrix, sel, pad):
    sc.check_csr_gather("cpu", matrix, sel, pad)


@pytest.mark.parametrize("matrix,width,pad", sc.BLOCK_CASES, ids=_ids(sc.BLOCK_CASES))
def test_csr_columns_to_dense_blocks(sim, matrix, width, pad):
    sc.check_csr_blocks("cpu", matrix, width, pad)


def test_project_genes_from_csr_with_a_short_last_block(sim):
    sc.check_project_genes_sparse("cpu")


@pytest.mark.parametrize("nrows,ncols,pad", sc.ROW_SUM_DENSE_CASES, ids=_ids(sc.ROW_SUM_DENSE_CASES))
def test_row_sums_dense(sim, nrows, ncols, pad):
    sc.check_row_sums_dense("cpu", nrows, ncols, pad)


@pytest.mark.parametrize("name", list(sc.ROW_SUM_CSR_CASES))
def test_row_sums_csr(sim, name):
    sc.check_row_sums_csr("cpu", name)


@pytest.mark.parametrize("n", sc.DENSITY_N)
def test_density(sim, n):
    sc.check_density("cpu", n)


@pytest.mark.parametrize("layout,ncols,pads", sc.CLUSTER_CASES, ids=_ids(sc.CLUSTER_CASES))
def test_cluster_aggregate(sim, layout, ncols, pads):
    sc.check_cluster_aggregate("cpu", layout, ncols, pads)


@pytest.mark.parametrize("where,value,verdict", [c[1:] for c in sc.SX_CASES], ids=[c[0] for c in sc.SX_CASES])
def test_s_exact_verdict_and_invariant(sim, where, value, verdict):
    """(The library takes a cell-type encoding that is not one-hot, so the 1/3 case of the last cell-type column is kept.)"""
    sc.check_s_exact("cpu", where, value, verdict)


@pytest.mark.parametrize("seed", sc.INIT_DIRECT["seeds"])
@pytest.mark.parametrize("stream_id", sc.INIT_DIRECT["stream_ids"])
def test_init_normal_against_its_formula(sim, seed, stream_id):
    sc.check_init_direct("cpu", seed, stream_id)


@pytest.mark.parametrize("n_cols,col0,pad", sc.INIT_NARROW_CASES, ids=_ids(sc.INIT_NARROW_CASES))
def test_init_normal_narrow_padded_blocks(sim, n_cols, col0, pad):
    sc.check_init_narrow("cpu", n_cols, col0, pad)


def test_init_normal_at_indices_above_2_32(sim):
    sc.check_init_index_above_2_32("cpu")


def test_init_normal_plane_below_the_grid_cap(sim):
    """The emulator cannot reach the 16 384-block cap of tg_init_normal (4.2 M quads, thread by thread): the same comparisons on a
    300 x 410 plane; the cap itself is exercised in tests/test_gpu_setup_kernels.py only."""
    sc.check_init_plane("cpu", "cpu")
