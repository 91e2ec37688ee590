"""The consistency metrics of repeated mappings on the MI355X (-m gpu): the tables, bounds and checks of tests/consistency_cases.py,
the same ones tests/test_consistency.py runs on the emulator -- votes exact, Pearson within 1e-9, vote entropy within 1e-6 and
consensus entropy within 1.5e-6 of the fp64 statement on the dense results of the same handles; both loaders bit for bit.  Here also
the shipped launch beyond TG_CONSIST_MAX_PARTS rows (GRID_CASES, PLANE_ROW_CASES: workgroups that take two and three rows), which
costs the emulator 20 - 50 s a case."""
import pytest

from tests import consistency_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(table):
    return ["-".join(str(x) for x in c) for c in table]


def test_limits_mirror_the_kernel_header():
    cc.check_limits()


@pytest.mark.parametrize("C,V,R,family", cc.KERNEL_CASES, ids=_ids(cc.KERNEL_CASES))
def test_kernel_case(C, V, R, family):
    cc.check_kernel_case(DEV, C, V, R, family)


def test_pearson_span():
    cc.check_pearson_span(DEV)


def test_ties():
    cc.check_ties(DEV)


def test_steps_and_modes():
    cc.check_steps_and_modes(DEV)


@pytest.mark.parametrize("n_cols,ld,offset,R", cc.PLANE_CASES, ids=_ids(cc.PLANE_CASES))
def test_plane_case(n_cols, ld, offset, R):
    cc.check_plane_case(DEV, n_cols, ld, offset, R)


@pytest.mark.parametrize("n_rows,max_parts,n_cols,ld,offset,R", cc.ROW_LOOP_CASES, ids=_ids(cc.ROW_LOOP_CASES))
def test_row_loop_case(n_rows, max_parts, n_cols, ld, offset, R):
    cc.check_row_loop_case(DEV, n_rows, max_parts, n_cols, ld, offset, R)


@pytest.mark.parametrize("C,V,R,family", cc.GRID_CASES, ids=_ids(cc.GRID_CASES))
def test_kernel_case_beyond_the_grid(C, V, R, family):
    cc.check_kernel_case(DEV, C, V, R, family)


@pytest.mark.parametrize("n_rows,n_cols,ld,offset,R", cc.PLANE_ROW_CASES, ids=_ids(cc.PLANE_ROW_CASES))
def test_plane_case_beyond_the_grid(n_rows, n_cols, ld, offset, R):
    cc.check_plane_case(DEV, n_cols, ld, offset, R, C=n_rows)


def test_training_state_is_undisturbed():
    cc.check_undisturbed(DEV)


def test_argument_errors():
    cc.check_argument_errors(DEV)


def test_public_surface():
    cc.check_public_surface(DEV)
