"""The consistency metrics of repeated mappings (tg_consist.h; tg_mapper_consistency / tg_planes_consistency;
tangram_amd.mapping_parameter_tuning) on the CPU emulator (same kernel sources): votes, Pearson correlations and both entropies
against an fp64 NumPy statement on the dense results of the same handles, at every row length, row count and run count of the
tables; ties; both loaders bit for bit; plain planes of any pitch and alignment; the row loop of a workgroup; repeatability; the undisturbed training state;
argument errors; the public surface against `train_many(val_each=1)`.  Tables, bounds and checks: tests/consistency_cases.py; the
same cases run on the GPU in tests/test_gpu_consistency.py.

Each of these edits of tg_consist.h, tried alone on the emulator, fails the tests named (or, where said so, must not):
    the tie-break flipped (`k >= bk[r]`, and the column packed without its complement): test_ties and every test_plane_case with
        n_cols >= 5 (the duplicated maximum of row 1);
    the `v < V` guard widened to the pitch (V = ld in tg_consist_rows): test_kernel_case at every V that is not a multiple of 64 (all
        but [3-64-..] and [3-2048-..]), test_ties, test_steps_and_modes, test_plane_case wherever ld > n_cols (the 1e30 behind the
        columns wins the votes), test_argument_errors, test_public_surface;
    the chunk carry of the argmax dropped (bk / bv reset at every chunk): test_ties, test_kernel_case[3-2049-3-shared], [3-4099-3-half],
        [3-2049-8-iid1], test_plane_case[2049-2052-0-2];
    the shift omitted in the covariance (`dx = p`): PASSES everything -- the correlation does not depend on the shift, which is
        there for the size of the sums;
    the fp64 accumulators turned to float (sums and products rounded to fp32): check 3 fails in test_kernel_case (12 of 16 cases),
        test_plane_case (9 of 10), test_steps_and_modes, test_argument_errors, test_public_surface;
    the pair order transposed (the correlations written in the order of np.triu_indices; the two orders hold the same pairs up to
        R = 3): test_kernel_case[40-257-8-half], [3-2049-8-iid1], test_plane_case[1000-1004-1-8];
    the finish kernel's stride loop made one trip: test_kernel_case[257-65-3-iid1] and [257-130-2-trained], test_row_loop_case[300-257-..];
    the moments reset at every row of a workgroup (`acc` zeroed inside the row loop): check 3 fails in every test_row_loop_case with a
        correlation (5 of 6; [9-1-64-64-0-1] has one run);
    the row parity not toggled (`phase ^= 1` dropped: one copy of the per-row LDS words, still one barrier per row -- a race, which
        the emulator shows only as far as its fixed fiber order exposes it): the votes of test_row_loop_case[9-4-2049-2052-0-3].
The row loop itself (a workgroup's second, third ... row) is walked by test_row_loop_case with a handful of rows and a capped grid
(tg_debug_planes_consistency); the shipped launch beyond TG_CONSIST_MAX_PARTS rows runs on the GPU only (GRID_CASES, PLANE_ROW_CASES).
ROW_LOOP_CASES go through the plane entry point, so they walk the loop behind the two plain loaders: behind the LOGITS loader (the
same body after the load) a workgroup takes a second and third row on the GPU only, in GRID_CASES.
"""
import os

import pytest

from tests import consistency_cases as cc
from tests.hipsim.build_sim import build_sim

DEV = "cpu"


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
    cc.check_case_tables()


def test_limits_mirror_the_kernel_header(sim):
    cc.check_limits()


def test_oracle_statement_against_the_reference_functions():
    """The NumPy statement the other tests trust, against the reference's own three functions on three small cubes."""
    if not os.path.exists(cc.reference_source()):
        pytest.skip("the reference tree is not present")
    cc.check_oracle_against_reference()


@pytest.mark.parametrize("C,V,R,family", cc.KERNEL_CASES, ids=_ids(cc.KERNEL_CASES))
def test_kernel_case(sim, C, V, R, family):
    cc.check_kernel_case(DEV, C, V, R, family)


def test_pearson_span(sim):
    cc.check_pearson_span(DEV)


def test_ties(sim):
    cc.check_ties(DEV)


def test_steps_and_modes(sim):
    cc.check_steps_and_modes(DEV)


@pytest.mark.parametrize("n_cols,ld,offset,R", cc.PLANE_CASES, ids=_ids(cc.PLANE_CASES))
def test_plane_case(sim, n_cols, ld, offset, R):
    cc.check_plane_case(DEV, n_cols, ld, offset, R)


@pytest.mark.parametrize("n_rows,max_parts,n_cols,ld,offset,R", cc.ROW_LOOP_CASES, ids=_ids(cc.ROW_LOOP_CASES))
def test_row_loop_case(sim, n_rows, max_parts, n_cols, ld, offset, R):
    cc.check_row_loop_case(DEV, n_rows, max_parts, n_cols, ld, offset, R)


def test_training_state_is_undisturbed(sim):
    cc.check_undisturbed(DEV)


def test_argument_errors(sim):
    cc.check_argument_errors(DEV)


def test_public_surface(sim):
    cc.check_public_surface(DEV)
