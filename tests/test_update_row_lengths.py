"""The update kernel at every row length on the cells-mode GEMM path, on the HIP emulator (CPU; the GPU run of the whole table is
tests/test_gpu_update_row_lengths.py).  A single GPU and more than 32 cells take the GEMM kernels (tg_is_clusters_problem is false);
which update kernel runs then depends on the number of spots V (tg_launch_update in tangram_amd/csrc/tg_capi.hip; the ladder from V to
(NQ, NT) is tg_with_row_length, shared with the batched tg_adam_rowpass_b, and (FULL, X16, STREAM) is tg_with_update_flags):

    V               kernel(s)                                                     instantiation
    <= 1024         tg_adam_rowpass                                               <FULL, X16, 1, 256, STREAM>
    1025 - 2048     tg_adam_rowpass                                               <FULL, X16, 2, 256, STREAM>
    2049 - 4096     tg_adam_rowpass                                               <FULL, X16, 4, 256, STREAM>
    4097 - 6144     tg_adam_rowpass                                               <FULL, X16, 3, 512, true>
    6145 - 8192     tg_adam_rowpass                                               <FULL, X16, 4, 512, true>
    8193 - 10240    tg_adam_rowpass                                               <FULL, X16, 5, 512, true>
    10241 - 12288   tg_adam_rowpass                                               <FULL, X16, 6, 512, true>
    12289 - 16384   tg_adam_rowpass                                               <FULL, X16, 8, 512, true>
    > 16384         tg_bwd_kernel (row-dot epilogue), tg_rowsum_parts, tg_adam_update  <FULL, X16, true, 1024> for C <= 64,
                                                                                       <FULL, X16, true, 256> above

FULL: constrained mode or lambda_r / lambda_l1 / lambda_l2 != 0.  X16: plain bf16 (X stored in bf16).  STREAM: stream_once,
C * Vp * (12 + 4, or 2 with X16) bytes > 192 MiB -- only the GPU table reaches it.  Each row has at most one quad that straddles V
and takes the masked path; all but three of the V below are not multiples of 4.

This table is the subset of the GPU one that keeps the emulator at about four minutes of CPU: every (NQ, NT, X16, FULL) of
tg_adam_rowpass, and tg_adam_update at both widths.  Every case asserts what tests/parity_common.update_row_case asserts, within
parity_common.ROW_TOL; largest values measured on the emulator over this table (MI355X: tests/test_gpu_update_row_lengths.py):
    precision   bound   grad      P         den       F
    fp32        5e-5    7.3e-7    9.7e-7    6.5e-6    1.1e-7
    bf16x3      5e-5    7.9e-6    5.0e-6    3.0e-5    1.4e-7
    bf16        1e-2    3.4e-3    1.9e-3    2.9e-3    2.4e-6
"""
import pytest

from tests import parity_common as pc
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

# (C, K, V, variant, precision, tile_size, expected tile): four cases per rowpass instantiation -- (bf16 | fp32 or bf16x3) x
# (plain | regularised or constrained) -- at the cheapest row lengths of each, and the two widths of tg_adam_update
CASES = [
    (33, 8, 1024, "plain", "bf16", 256, 256), (64, 8, 1021, "regularised", "bf16", 0, 128),
    (65, 8, 1023, "plain", "fp32", 0, 128), (300, 8, 1021, "constrained", "bf16x3", 0, 128),
    (33, 8, 1025, "constrained", "bf16", 0, 128), (65, 8, 2048, "plain", "bf16", 0, 128),
    (64, 8, 1025, "regularised", "fp32", 0, 128), (33, 8, 1027, "plain", "bf16x3", 0, 128),
    (65, 8, 2049, "plain", "bf16", 0, 128), (33, 8, 2051, "constrained", "bf16", 0, 128),
    (64, 8, 2049, "plain", "bf16x3", 0, 128), (65, 8, 2053, "regularised", "fp32", 0, 128),
    (33, 8, 4097, "plain", "bf16", 256, 256), (65, 8, 4097, "regularised", "bf16", 0, 128),
    (64, 8, 4099, "constrained", "fp32", 0, 128), (33, 8, 4992, "plain", "bf16x3", 0, 128),
    (65, 8, 6145, "plain", "bf16", 0, 128), (33, 8, 6145, "constrained", "bf16", 0, 128),
    (64, 8, 6147, "plain", "fp32", 0, 128), (33, 8, 6145, "regularised", "bf16x3", 0, 128),
    (33, 8, 8193, "plain", "bf16", 0, 128), (64, 8, 8193, "regularised", "bf16", 0, 128),
    (65, 8, 8193, "plain", "bf16x3", 0, 128), (33, 8, 8195, "constrained", "fp32", 0, 128),
    (64, 8, 10241, "plain", "bf16", 0, 128), (33, 8, 10241, "constrained", "bf16", 0, 128),
    (33, 8, 10243, "plain", "fp32", 0, 128), (65, 8, 10241, "regularised", "bf16x3", 0, 128),
    (33, 8, 12289, "plain", "bf16", 0, 128), (65, 8, 12289, "regularised", "bf16", 0, 128),
    (64, 8, 12289, "constrained", "bf16x3", 0, 128), (33, 8, 12291, "plain", "fp32", 0, 128),
    (64, 8, 16385, "regularised", "bf16", 0, 128),        # tg_adam_update<true, true, true, 1024>
    (65, 8, 16385, "constrained", "fp32", 0, 128),        # tg_adam_update<true, false, true, 256>
]


def _id(c):
    C, K, V, var, prec, tile, _ = c
    return f"C{C}-V{V}-{var}-{prec}" + ("-t256" if tile else "")


def _kinds(cases):
    return {pc.update_instantiation(C, V, prec, var) for C, K, V, var, prec, tile, _ in cases}


def _all_kinds():
    """Every instantiation tg_launch_update (tg_with_update_flags x tg_with_row_length) can select for a single GPU with C > 32."""
    kinds = set()
    for full in (False, True):
        for x16 in (False, True):
            for stream in (False, True):
                kinds |= {("tg_adam_rowpass", full, x16, nq, 256, stream) for nq in (1, 2, 4)}
            kinds |= {("tg_adam_rowpass", full, x16, nq, 512, True) for nq in (3, 4, 5, 6, 8)}
            kinds |= {("tg_adam_update", full, x16, None, nt, True) for nt in (1024, 256)}
    return kinds


def test_case_tables_cover_every_instantiation():
    """The emulator table reaches every (NQ, NT, X16, FULL) of tg_adam_rowpass without STREAM and both widths of tg_adam_update;
    the GPU table reaches every instantiation, each kernel family also on the 256 layout."""
    from tests.test_gpu_update_row_lengths import CASES as GPU_CASES
    every = _all_kinds()
    assert len(every) == 2 * 2 * (2 * 3 + 5 + 2)
    emu = _kinds(CASES)
    assert emu >= {k for k in every if k[0] == "tg_adam_rowpass" and not k[5]}, sorted(map(str, every - emu))
    assert {k[4] for k in emu if k[0] == "tg_adam_update"} == {1024, 256}
    gpu = _kinds(GPU_CASES)
    stream256 = {k for k in every if k[0] == "tg_adam_rowpass" and k[4] == 256 and k[5]}     # (one case per stream_once branch)
    assert gpu >= every - stream256, sorted(map(str, every - stream256 - gpu))
    assert gpu & stream256, "no case takes the streaming 256-thread rowpass"
    for table in (CASES, GPU_CASES):
        fam = {(pc.update_instantiation(C, V, p, v)[0], pc.update_instantiation(C, V, p, v)[4]) for C, K, V, v, p, t, _ in table if t == 256}
        assert {("tg_adam_rowpass", 256), ("tg_adam_rowpass", 512)} <= fam
    fam = {pc.update_instantiation(C, V, p, v)[4] for C, K, V, v, p, t, _ in GPU_CASES if t == 256 and V > 16384}
    assert fam, "no tile_size=256 case on the two-kernel path"
    assert {C for C, *_ in GPU_CASES} >= {33, 64, 65, 300}
    for V in (1024, 1025, 2048, 2049, 4096, 4097, 6144, 6145, 8192, 8193, 10240, 10241, 12288, 12289, 16384, 16385):
        assert any(c[2] == V for c in GPU_CASES), V


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_emulated_update_row_lengths(sim, case):
    C, K, V, var, prec, tile, expect_tile = case
    pc.update_row_case("cpu", C, K, V, var, prec, tile=tile, expect_tile=expect_tile, seed=C + V)
