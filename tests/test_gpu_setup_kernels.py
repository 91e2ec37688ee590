"""The set-up and pre-processing kernels of tg_setup.h at every loop boundary on the MI355X (-m gpu): the tables and checks of
tests/setup_cases.py, the same ones tests/test_setup_kernels.py runs on the emulator (the coverage test of the tables lives there
and here), plus the one case only the hardware can run: a plane above tg_init_normal's cap of 16 384 blocks."""
import pytest

from tests import setup_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(table):
    return ["-".join(str(x) for x in c) for c in table]


def test_case_tables_cover_every_edge():
    sc.check_case_tables()


@pytest.mark.parametrize("matrix,sel,pad", sc.GATHER_CASES, ids=_ids(sc.GATHER_CASES))
def test_csr_gather_columns(matrix, sel, pad):
    sc.check_csr_gather(DEV, matrix, sel, pad)


@pytest.mark.parametrize("matrix,width,pad", sc.BLOCK_CASES, ids=_ids(sc.BLOCK_CASES))
def test_csr_columns_to_dense_blocks(matrix, width, pad):
    sc.check_csr_blocks(DEV, matrix, width, pad)


def test_project_genes_from_csr_with_a_short_last_block():
    sc.check_project_genes_sparse(DEV)


@pytest.mark.parametrize("nrows,ncols,pad", sc.ROW_SUM_DENSE_CASES, ids=_ids(sc.ROW_SUM_DENSE_CASES))
def test_row_sums_dense(nrows, ncols, pad):
    sc.check_row_sums_dense(DEV, nrows, ncols, pad)


@pytest.mark.parametrize("name", list(sc.ROW_SUM_CSR_CASES))
def test_row_sums_csr(name):
    sc.check_row_sums_csr(DEV, name)


@pytest.mark.parametrize("n", sc.DENSITY_N)
def test_density(n):
    sc.check_density(DEV, n)


@pytest.mark.parametrize("layout,ncols,pads", sc.CLUSTER_CASES, ids=_ids(sc.CLUSTER_CASES))
def test_cluster_aggregate(layout, ncols, pads):
    sc.check_cluster_aggregate(DEV, layout, ncols, pads)


@pytest.mark.parametrize("where,value,verdict", [c[1:] for c in sc.SX_CASES], ids=[c[0] for c in sc.SX_CASES])
def test_s_exact_verdict_and_invariant(where, value, verdict):
    """(The library takes a cell-type encoding that is not one-hot, so the 1/3 case of the last cell-type column is kept.)"""
    sc.check_s_exact(DEV, where, value, verdict)


@pytest.mark.parametrize("seed", sc.INIT_DIRECT["seeds"])
@pytest.mark.parametrize("stream_id", sc.INIT_DIRECT["stream_ids"])
def test_init_normal_against_its_formula(seed, stream_id):
    print("max |got - ref|:", sc.check_init_direct(DEV, seed, stream_id))


@pytest.mark.parametrize("n_cols,col0,pad", sc.INIT_NARROW_CASES, ids=_ids(sc.INIT_NARROW_CASES))
def test_init_normal_narrow_padded_blocks(n_cols, col0, pad):
    print("max |got - ref|:", sc.check_init_narrow(DEV, n_cols, col0, pad))


def test_init_normal_at_indices_above_2_32():
    print("max |got - ref|:", sc.check_init_index_above_2_32(DEV))


def test_init_normal_plane_above_the_grid_cap():
    """4200 x 4100: 4.3 M quads against the cap of 16 384 x 256 = 4.19 M threads, so the grid-stride loop makes its second trip."""
    print("max |got - ref|:", sc.check_init_plane(DEV, "gpu"))
