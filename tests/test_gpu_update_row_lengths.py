"""The update kernel at every row length on the cells-mode GEMM path (-m gpu): one case table through the C ABI against the fp64
oracle, every case checked by tests/parity_common.update_row_case (schedule, first-step gradient per row and on the straddling quad,
3 epochs of history, P and the second moment element-wise, the filter, the padding columns).  The CPU twin on the emulator, with a
subset of this table, is tests/test_update_row_lengths.py; its docstring maps each V to the instantiation it selects.

The table: every capacity of tg_with_row_length (tg_capi.hip) and the value one past it, the switch to the two-kernel path at 16 385 spots, for
each precision (fp32, bf16x3, bf16 -- X16) and variant (plain, regularised, constrained -- FULL), with C cycling through 33 (one
past the clusters-mode bound), 64 / 65 (tg_adam_update's 1 024- / 256-thread switch) and 300 (three cell tiles, the history
workgroup behind the last), some cases on the 256 layout; and one case per branch of stream_once (C * Vp * 16 B > 192 MiB).

Bounds (parity_common.ROW_TOL) and the largest values measured on MI355X over this table (grad: the worse of the row check and
the last-four-columns check; F: the filter logits; the filter's denominator stays under 2e-5 everywhere):
    precision   bound   grad      P         den       F
    fp32        5e-5    1.8e-6    1.5e-6    6.4e-6    1.6e-7
    bf16x3      5e-5    1.7e-5    3.0e-6    2.0e-5    1.4e-7
    bf16        1e-2    4.8e-3    1.9e-3    6.5e-3    2.0e-6
"""
import pytest

from tests import parity_common as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

V_LIST = [1024, 1025, 2048, 2049, 4096, 4097, 4992, 6144, 6145, 8192, 8193, 10240, 10241, 12288, 12289, 16383, 16384, 16385, 20001]
PRECISIONS = ["fp32", "bf16x3", "bf16"]
VARIANTS = ["plain", "regularised", "constrained"]


def _cases():
    """(C, K, V, variant, precision, tile_size, expected tile)"""
    out, j = [], 0
    for V in V_LIST:
        for i, (prec, var) in enumerate((p, v) for p in PRECISIONS for v in VARIANTS):
            if V > 16384:          # both widths of tg_adam_update for every (X16, FULL): 64 and 65 alternate between the two V
                C = (64, 65)[(i + (V == 20001)) % 2]
            else:
                C = (33, 64, 65, 300)[j % 4]
            tile = 256 if j % 7 == 3 else 0
            out.append((C, 8 + 8 * (j % 4), V, var, prec, tile, 256 if tile else 128))
            j += 1
    out += [
        (300, 16, 20001, "regularised", "bf16", 256, 256),       # several cell tiles on the two-kernel path
        (300, 24, 16385, "constrained", "fp32", 0, 128),
        # stream_once: C * Vp * 16 B > 192 MiB (tg_capi.hip, tg_mapper_create)
        (13000, 12, 1024, "plain", "fp32", 0, 256),             # tg_adam_rowpass<.., 1, 256, STREAM>
        (4200, 12, 4096, "regularised", "bf16x3", 0, 256),      # tg_adam_rowpass<.., 4, 256, STREAM>
        (800, 12, 16384, "constrained", "fp32", 0, 128),        # the streaming backward GEMM in front of the 512-thread rowpass
    ]
    return out


CASES = _cases()


def _id(c):
    C, K, V, var, prec, tile, _ = c
    return f"C{C}-V{V}-{var}-{prec}" + ("-t256" if tile else "")


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_update_row_lengths_against_oracle_fp64(case):
    C, K, V, var, prec, tile, expect_tile = case
    out = pc.update_row_case(DEV, C, K, V, var, prec, tile=tile, expect_tile=expect_tile, seed=C + V)
    print(_id(case), out)
