"""Tables and checks of the spot-wise top-k result path (tg_spot_topk.h: tg_spot_topk, tg_spot_colsum_finish, with tg_topk_merge_rows
over the slabs; tg_mapper_spot_topk_query_bytes / tg_mapper_result_spot_topk; HipMapperEngine / ShardedMapperEngine /
Mapper(.Constrained).result_spot_topk; train(spot_top_k=), map_cells_to_space(spot_top_k=)), shared by tests/test_spot_topk.py
(emulator, device "cpu") and tests/test_gpu_spot_topk.py (MI355X).

Every comparison of lists is exact: the expected entries of a spot are `np.lexsort((cells, -P[cells, v]))[:k]` over the admitted cells
of the DENSE result of the same handle -- value descending, equal values by ascending cell --, padded with (0.0, -1), and values are
compared as bit patterns.

Column sums: the reference is the fp64 sum of the dense result's fp32 values over the admitted cells, rounded to fp32; the bound is
1 ulp of it.  The kernel adds the same fp64 terms in another grouping (slab by slab), at most a few thousand of them: the two fp64
sums differ by far less than an fp32 ulp (n * 2^-53 relative against 2^-24), so the two roundings land on the same float or, when
the sum sits at a rounding boundary, on neighbours.  Largest deviation seen over every case of this file: 0 ulp, on the emulator
and on an MI355X alike."""
import ctypes as ct

import numpy as np
import pytest
import torch

from tangram_amd import _capi

KMAX = _capi.SPOT_TOPK_MAX
STRIP = _capi.SPOT_TOPK_STRIP
SLAB = _capi.SPOT_TOPK_MIN_SLAB_ROWS                 # the smallest slab height a caller may force = rows loaded ahead
LAM = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5)
KS_ALL = (1, 3, 5, 12, KMAX)                          # one k per list length the kernel is instantiated for: 1, 4, 8, 16, 32
KS = (1, 5, KMAX)

# 1. spot edges (C, K, V, precision): around the 64-lane wave, the strip of one workgroup, three strips; every V that is no multiple
# of 64 has padding columns behind it (100: 28 of them)
SPOT_VS = (1, 2, 63, 64, 65, 100, STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 3)
SPOT_CASES = [(40, 5, V, "bf16x3") for V in SPOT_VS] + [(40, 5, STRIP + 1, "fp32"), (40, 5, STRIP + 1, "bf16")]
# 2. cell and slab edges (C, k) at V = 65 and slab_rows = SLAB: 2 SLAB + 1 leaves a last slab of a single row
CELL_V = 65


def cell_counts(k):
    return sorted({c for c in (1, k - 1, k, k + 1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 3, 2 * SLAB + 1) if c >= 1})


CELL_CASES = [(C, k) for k in KS for C in cell_counts(k)]
TIE_LAYOUTS = ("inside-one-slab", "across-a-slab-boundary", "all-rows-equal", "equal-p-from-distinct-logits")
FILTER_CASES = ("none", "fewer-than-k", "nobody", "exactly-an-f")
# 8. spot shards (world, V, k): blocks down to one spot wide (9 ranks on 10 spots; 16 ranks need 16 spots)
SHARD_CASES = [(w, V, k) for w in (2, 3, 9) for V in (10, 100, 131) for k in (5, KMAX)] + \
              [(16, V, k) for V in (100, 131) for k in (5, KMAX)]

MAX_ULP = [0.0]                                        # largest column-sum deviation seen in this process, in ulp


def check_case_tables():
    assert (KMAX, STRIP, SLAB) == (32, 256, 8)
    assert {V for _, _, V, _ in SPOT_CASES} >= {1, 2, 63, 64, 65, STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 3}
    assert any(V % 64 for _, _, V, _ in SPOT_CASES) and {C for C, *_ in SPOT_CASES} == {40}
    assert {p for *_, p in SPOT_CASES} == {"bf16x3", "fp32", "bf16"}
    for k in KS:
        assert {C for C, kk in CELL_CASES if kk == k} >= {c for c in (1, k - 1, k, k + 1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 3) if c >= 1}
        assert any(C > SLAB and C % SLAB == 1 for C, kk in CELL_CASES if kk == k)            # a last slab of one row
    assert set(KS) == {1, 5, KMAX} and set(KS_ALL) >= set(KS)
    lens = {1 if k <= 1 else 4 if k <= 4 else 8 if k <= 8 else 16 if k <= 16 else 32 for k in KS_ALL}
    assert lens == {1, 4, 8, 16, 32}                                                         # every instantiation runs
    assert {w for w, _, _ in SHARD_CASES} == {2, 3, 9, 16} and {V for _, V, _ in SHARD_CASES} == {10, 100, 131}
    assert {k for _, _, k in SHARD_CASES} == {5, KMAX} and (9, 10, 5) in SHARD_CASES          # 9 ranks, 10 spots: blocks one spot wide
    assert all(V >= w for w, V, _ in SHARD_CASES)


def check_limits():
    """_capi.SPOT_TOPK_* mirror the kernel header; the slab rule at 30 000 x 10 000 fills the chip."""
    out = (ct.c_int32 * 4)()
    assert _capi.lib().tg_debug_spot_topk_limits(30000, 10000, out) == 0
    assert (out[0], out[1], out[2]) == (_capi.SPOT_TOPK_MAX, _capi.SPOT_TOPK_STRIP, _capi.SPOT_TOPK_MIN_SLAB_ROWS) == (KMAX, STRIP, SLAB)
    rows = out[3]
    n_wg = -(-10000 // STRIP) * -(-30000 // rows)
    assert rows % SLAB == 0 and 768 <= n_wg <= 1024, (rows, n_wg)                              # 3 - 4 workgroups per CU of 256
    assert _capi.lib().tg_debug_spot_topk_limits(40, 65, out) == 0 and out[3] >= 40            # a small problem is one slab


def _np(t):
    return t.detach().cpu().numpy()


def host_spot_topk(P, k, admitted=None):
    """(values [V, k], cells [V, k]) of the dense mapping P [C, V] over the admitted cells: value descending, equal values by
    ascending cell, (0.0, -1) behind the last admitted cell."""
    C, V = P.shape
    cells = np.arange(C) if admitted is None else np.flatnonzero(admitted)
    val = np.zeros((V, k), dtype=np.float32)
    idx = np.full((V, k), -1, dtype=np.int32)
    for v in range(V):
        order = cells[np.lexsort((cells, -P[cells, v]))[:k]]
        val[v, :len(order)] = P[order, v]
        idx[v, :len(order)] = order
    return val, idx


def host_colsum(P, admitted=None):
    rows = P if admitted is None else P[admitted]
    return rows.astype(np.float64).sum(axis=0).astype(np.float32)


def assert_spot_topk_equals_dense(got, P, k, where, admitted=None):
    val, idx = (_np(x) for x in got[:2])
    assert val.shape == idx.shape == (P.shape[1], k) and val.dtype == np.float32 and idx.dtype == np.int32, where
    rv, ri = host_spot_topk(P, k, admitted)
    np.testing.assert_array_equal(idx, ri, err_msg=f"{where}: cells")
    np.testing.assert_array_equal(val.view(np.uint32), rv.view(np.uint32), err_msg=f"{where}: value bits")
    if len(got) > 2:
        total, ref = _np(got[2]), host_colsum(P, admitted)
        assert total.shape == (P.shape[1],) and total.dtype == np.float32, where
        ulp = np.abs(total.astype(np.float64) - ref.astype(np.float64)) / np.maximum(np.spacing(ref).astype(np.float64), 2.0 ** -149)
        MAX_ULP[0] = max(MAX_ULP[0], float(ulp.max()))
        print(f"{where}: column sums off by at most {ulp.max():.2f} ulp")
        assert (ulp <= 1.0).all(), f"{where}: column sums off by {ulp.max()} ulp"


def _problem(C, K, V, seed):
    from tests import parity_common as pc
    return pc.validation_problem(C, K, V, seed)


def _engine(device, C, K, V, precision="bf16x3", M0=None, seed=None):
    from tangram_amd.engine import HipMapperEngine
    S, G, d, M = _problem(C, K, V, C + V if seed is None else seed)
    return HipMapperEngine(S, G, M if M0 is None else M0, d=d, device=device, precision=precision, lambdas=LAM)


def check_spot_case(device, C, K, V, precision):
    """result_spot_topk against the dense result of the same handle, before any step and after 3, for one k per instantiated list
    length (k = 12 and 32 exceed no cell count here: C = 40), as one slab (the list is written straight to the outputs) and as
    slabs of SLAB rows (partial lists + merge), with the column sums."""
    e = _engine(device, C, K, V, precision)
    for steps in (0, 3):
        if steps:
            e.step(steps, 0.1, e.new_history(steps), 0)
        P = _np(e.result())
        for k in KS_ALL:
            for slab_rows in (0, SLAB):
                got = e.result_spot_topk(k, colsum=True, slab_rows=slab_rows)
                assert_spot_topk_equals_dense(got, P, k, f"C{C} V{V} {precision} k={k} slab_rows={slab_rows} after {steps} steps")
    e.release()


def check_cell_case(device, C, k):
    """Cell counts around k and around the slab height at V = 65, slabs of SLAB rows; a k beyond the number of cells ends in pads."""
    e = _engine(device, C, 5, CELL_V)
    e.step(2, 0.1, e.new_history(2), 0)
    P = _np(e.result())
    got = e.result_spot_topk(k, colsum=True, slab_rows=SLAB)
    assert_spot_topk_equals_dense(got, P, k, f"C{C} k={k}")
    if k > C:
        assert (_np(got[1])[:, C:] == -1).all() and (_np(got[0])[:, C:] == 0).all() and (_np(got[1])[:, :C] >= 0).all()
    e.release()


def check_split_independence(device, C=83, V=300):
    """The lists and values do not depend on how the cells are cut into slabs."""
    e = _engine(device, C, 5, V)
    e.step(3, 0.1, e.new_history(3), 0)
    P = _np(e.result())
    for k in (5, KMAX):
        ref = None
        for slab_rows in (SLAB, 3 * SLAB + 1, C, 0):
            got = tuple(_np(x) for x in e.result_spot_topk(k, slab_rows=slab_rows))
            if ref is None:
                ref = got
                assert_spot_topk_equals_dense(tuple(torch.as_tensor(x) for x in got), P, k, f"split k={k} slab_rows={slab_rows}")
            np.testing.assert_array_equal(got[0].view(np.uint32), ref[0].view(np.uint32), err_msg=f"k={k} slab_rows={slab_rows}: values")
            np.testing.assert_array_equal(got[1], ref[1], err_msg=f"k={k} slab_rows={slab_rows}: cells")
    e.release()


def tie_logits(layout, C=20, V=65):
    """M0 [C, V] for slabs of SLAB rows: rows of identical logits give identical p bits."""
    rng = np.random.default_rng(len(layout))
    M = rng.standard_normal((C, V)).astype(np.float32)
    if layout == "inside-one-slab":
        M[5] = M[2]
    elif layout == "across-a-slab-boundary":
        M[SLAB] = M[SLAB - 1]
        M[2 * SLAB + 1] = M[SLAB - 1]
    elif layout == "all-rows-equal":
        M[:] = M[0]
    else:
        # column 10: logits that RISE with the cell index and all underflow to p = 0 -- ranking the logits would take the last
        # cells, ranking p takes cells 0, 1, 2 ...; column 11: one cell with p > 0 on top of such a column
        M[:, 10] = -300.0 + np.arange(C, dtype=np.float32)
        M[:, 11] = -300.0 + np.arange(C, dtype=np.float32)
        M[C - 3, 11] = 0.5
    return M


def check_ties(device, layout):
    M0 = tie_logits(layout)
    C, V = M0.shape
    e = _engine(device, C, 5, V, M0=M0, seed=3)
    P = _np(e.result())
    Pb = P.view(np.uint32)
    if layout == "inside-one-slab":
        assert (Pb[5] == Pb[2]).all()
    elif layout == "across-a-slab-boundary":
        assert (Pb[SLAB] == Pb[SLAB - 1]).all() and (Pb[2 * SLAB + 1] == Pb[SLAB - 1]).all()
    elif layout == "all-rows-equal":
        assert (Pb == Pb[0]).all()
    else:
        assert (P[:, 10] == 0).all() and (P[:, 11] == 0).sum() == C - 1 and len(np.unique(M0[:, 10])) == C
    for k in KS_ALL:
        for slab_rows in (SLAB, 0):
            got = e.result_spot_topk(k, slab_rows=slab_rows)
            assert_spot_topk_equals_dense(got, P, k, f"ties {layout} k={k} slab_rows={slab_rows}")
            cells = _np(got[1])
            n = min(k, C)
            if layout == "all-rows-equal":
                assert (cells[:, :n] == np.arange(n)).all(), "equal values: cells 0 .. k - 1 for every spot"
            elif layout == "equal-p-from-distinct-logits":
                assert cells[10, :n].tolist() == list(range(n)), "decided on p, not on the logits"
                assert cells[11, :n].tolist() == [C - 3] + [c for c in range(C) if c != C - 3][:n - 1]
            else:
                twins = (2, 5) if layout == "inside-one-slab" else (SLAB - 1, SLAB)
                for v in range(V):                                      # the lower cell stands directly in front of its twin
                    row = cells[v].tolist()
                    if twins[1] in row:
                        assert row.index(twins[0]) + 1 == row.index(twins[1]), (layout, v, row)
    e.release()


def _constrained_engine(device, C=40, K=12, V=100, steps=2):
    from tangram_amd.engine import HipMapperEngine
    from oracle import tangram_oracle as orc
    data = orc.make_synthetic(C, K, V, seed=5)
    M0, F0 = orc.reference_init_MF_constrained(C, V, 6)
    lam = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5, lambda_count=1.0, lambda_f_reg=1.0)
    e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], F0=F0, mode="constrained", device=device, lambdas=lam, target_count=20.0)
    if steps:
        e.step(steps, 0.1, e.new_history(steps), 0)
    return e


def check_filter(device, case, k=5):
    """Constrained mode: only cells with f_c > threshold take part (strictly), in lists, pads and column sums."""
    e = _constrained_engine(device)
    P, F = (_np(x) for x in e.result(with_filter=True))
    Fs = np.sort(F)
    assert len(np.unique(F)) == len(F) and (F > 0).all()
    thr = {"none": None, "fewer-than-k": Fs[-3], "nobody": Fs[-1], "exactly-an-f": Fs[len(Fs) // 2]}[case]
    admitted = np.ones(len(F), dtype=bool) if thr is None else F > thr
    assert admitted.sum() == {"none": len(F), "fewer-than-k": 2, "nobody": 0, "exactly-an-f": len(F) - len(F) // 2 - 1}[case]
    for slab_rows in (SLAB, 0):
        got = e.result_spot_topk(k, min_filter=None if thr is None else float(thr), colsum=True, slab_rows=slab_rows)
        assert_spot_topk_equals_dense(got, P, k, f"filter {case} slab_rows={slab_rows}", admitted)
        val, cells, total = (_np(x) for x in got)
        if case == "fewer-than-k":
            assert (cells[:, 2:] == -1).all() and (val[:, 2:] == 0).all() and (cells[:, :2] >= 0).all()
        if case == "nobody":
            assert (cells == -1).all() and (val == 0).all() and (total == 0).all()
        if case == "exactly-an-f":
            assert not (cells == int(np.flatnonzero(F == thr)[0])).any(), "f_c == threshold must drop the cell: the comparison is strict"
    for bad in (-1.0, float("nan")):                                    # a negative threshold or NaN admits every cell
        assert_spot_topk_equals_dense(e.result_spot_topk(k, min_filter=bad), P, k, f"min_filter={bad}")
    e.release()


def check_filter_needs_a_constrained_handle(device):
    e = _engine(device, 40, 5, 65)
    with pytest.raises(ValueError, match="unconstrained mapper, which has no filter"):
        e.result_spot_topk(3, min_filter=0.5)
    with pytest.raises(ValueError, match="unconstrained"):
        e.result_spot_topk(3, min_filter=0.0)
    P = _np(e.result())
    assert_spot_topk_equals_dense(e.result_spot_topk(3, min_filter=-1.0), P, 3, "after the refused calls")
    e.release()


def check_mass(device):
    """Mapper.result_spot_topk(k, mass=True): NumPy arrays; the share of the column sum lies in (0, 1], up to one rounding."""
    from tangram_amd.mapping_optimizer import Mapper, MapperConstrained
    S, G, d, M0 = _problem(40, 5, 70, 9)
    m = Mapper(S, G, d=d, lambda_d=1, device=device, M_init=M0)
    m.train(3, print_each=None)
    P = _np(m._engine.result())
    one_ulp = np.float32(1.0) + np.spacing(np.float32(1.0))
    for k in KS:
        val, cells, mass = m.result_spot_topk(k, mass=True)
        assert all(isinstance(x, np.ndarray) for x in (val, cells, mass)) and mass.shape == (70,) and mass.dtype == np.float32
        assert_spot_topk_equals_dense((torch.as_tensor(val), torch.as_tensor(cells)), P, k, f"Mapper k={k}")
        ref = val.astype(np.float64).sum(axis=1) / host_colsum(P).astype(np.float64)
        np.testing.assert_allclose(mass, ref, rtol=3e-7, atol=0)                 # (two fp32 roundings: the column sum and the share)
        assert (mass > 0).all() and (mass <= one_ulp).all(), (k, mass.min(), mass.max())
    v2, c2 = m.result_spot_topk(5)
    assert v2.shape == c2.shape == (70, 5)
    m.release()
    F0 = np.random.default_rng(3).standard_normal(40).astype(np.float32)
    mc = MapperConstrained(S, G, d, lambda_d=1, target_count=20, device=device, M_init=M0, F_init=F0)
    mc.train(2, print_each=None)
    Pc, Fc = (_np(x) for x in mc._engine.result(with_filter=True))
    thr = float(np.sort(Fc)[-4])                                                  # three cells admitted, k = 5 >= admitted: mass 1
    val, cells, mass = mc.result_spot_topk(5, thr, mass=True)
    assert_spot_topk_equals_dense((torch.as_tensor(val), torch.as_tensor(cells)), Pc, 5, "MapperConstrained", Fc > np.float32(thr))
    assert (cells[:, 3:] == -1).all() and (mass > 0).all() and (mass <= one_ulp).all() and (np.abs(mass - 1) <= 2e-7).all()
    val, cells = mc.result_spot_topk(5)
    assert_spot_topk_equals_dense((torch.as_tensor(val), torch.as_tensor(cells)), Pc, 5, "MapperConstrained without a threshold")
    mc.release()


def _state_of(e):
    M, m1, m2, step = e.logits()
    return [_np(x).copy() for x in (M, m1, m2)] + [step]


def check_undisturbed(device, C=40, K=5, V=257):
    """2 steps, result_spot_topk (twice: the same bits), 2 steps == 4 steps: history, logits and both Adam moments bit for bit,
    padding columns included."""
    S, G, d, M0 = _problem(C, K, V, C + V)
    from tangram_amd.engine import HipMapperEngine
    res = []
    for ask in (True, False):
        e = HipMapperEngine(S, G, M0, d=d, device=device, precision="bf16x3", lambdas=LAM)
        hist = e.new_history(4)
        e.step(2, 0.1, hist, 0)
        if ask:
            a, b = (e.result_spot_topk(7, colsum=True, slab_rows=SLAB) for _ in range(2))
            for x, y in zip(a, b):
                np.testing.assert_array_equal(_np(x).view(np.uint32), _np(y).view(np.uint32))
        e.step(2, 0.1, hist, 2)
        res.append([_np(hist).copy()] + _state_of(e))
        e.release()
    for name, x, y in zip(("history", "M", "exp_avg", "exp_avg_sq", "step"), res[0], res[1]):
        np.testing.assert_array_equal(x, y, err_msg=name)


def check_shards(device, world, V, k, C=40, K=5, n=3):
    """Spot shards (threads, tests/local_comm.py): every rank's result_spot_topk after n steps is the column top-k of that run's
    result_full(), identical on all ranks, column sums included."""
    from tangram_amd.sharded import make_sharded
    from tests.local_comm import run_ranks
    S, G, d, M0 = _problem(C, K, V, 13 + V)

    def rank_fn(comm):
        sh = make_sharded(S, G, M0, d=d, device=device, precision="bf16x3", lambdas=LAM, comm=comm)
        sh.run(n, 0.1, sh.eng.new_history(n), 0)
        P = _np(sh.result_full())
        got = tuple(_np(x) for x in sh.result_spot_topk(k, colsum=True, slab_rows=SLAB))
        plain = tuple(_np(x) for x in sh.result_spot_topk(k))
        width = sh.eng.V
        sh.release()
        return P, got, plain, width

    res = run_ranks(world, rank_fn)
    P = res[0][0]
    assert P.shape == (C, V) and sum(r[3] for r in res) == V
    if (world, V) == (9, 10):
        assert min(r[3] for r in res) == 1                                        # blocks one spot wide
    for r in range(world):
        np.testing.assert_array_equal(res[r][0], P)
        for a, b in zip(res[r][1], res[0][1]):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"rank {r}: other bits than rank 0")
        for a, b in zip(res[r][2], res[0][1][:2]):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"rank {r}: the call without column sums differs")
    assert_spot_topk_equals_dense(tuple(torch.as_tensor(x) for x in res[0][1]), P, k, f"{world} shards V{V} k={k}")


def check_argument_errors(device):
    """The TG_ERR_INVALID cases raise ValueError with the library's message; the handle stays usable."""
    e = _engine(device, 40, 5, 10, seed=1)
    for k in (0, -3, KMAX + 1):
        with pytest.raises(ValueError, match=rf"k = {k} is outside \[1, {KMAX}\]"):
            e.result_spot_topk(k)
    for rows in (-1, 1, SLAB - 1):
        with pytest.raises(ValueError, match=f"at least {SLAB}"):
            e.result_spot_topk(3, slab_rows=rows)
    lib = _capi.lib()
    val = torch.zeros((10, 4), dtype=torch.float32, device=e.device)
    cell = torch.zeros((10, 4), dtype=torch.int32, device=e.device)
    nbytes = ct.c_size_t()
    e._call(lib.tg_mapper_spot_topk_query_bytes, e._h, 4, SLAB, ct.byref(nbytes))
    assert nbytes.value >= 2 * 10 * 5 * 4 * 4 + 5 * 10 * 8                              # 5 slabs: two list planes and the column sums
    scratch = torch.zeros(nbytes.value // 8 + 1, dtype=torch.int64, device=e.device)
    with pytest.raises(ValueError, match="bytes_out is NULL"):
        e._call(lib.tg_mapper_spot_topk_query_bytes, e._h, 4, SLAB, None)
    for v, c, s, msg in ((None, cell.data_ptr(), scratch.data_ptr(), "an output is NULL"), (val.data_ptr(), None, scratch.data_ptr(), "an output is NULL"),
                         (val.data_ptr(), cell.data_ptr(), None, "scratch is NULL")):
        with pytest.raises(ValueError, match=msg):
            e._call(lib.tg_mapper_result_spot_topk, e._h, 4, -1.0, SLAB, s, v, c, None)
    with pytest.raises(_capi.TangramHipError, match="not ready"):
        _capi.check(lib.tg_mapper_result_spot_topk(None, 4, -1.0, 0, scratch.data_ptr(), val.data_ptr(), cell.data_ptr(), None))
    e._call(lib.tg_mapper_result_spot_topk, e._h, 4, -1.0, SLAB, scratch.data_ptr(), val.data_ptr(), cell.data_ptr(), None)
    P = _np(e.result())
    assert_spot_topk_equals_dense((val, cell), P, 4, "the raw call after the refused ones")
    assert_spot_topk_equals_dense(e.result_spot_topk(KMAX, colsum=True), P, KMAX, "k beyond the 40 cells is no error")
    e.release()


def check_train_spot_top_k(device):
    """Mapper.train / MapperConstrained.train(spot_top_k=k): what they return is unchanged; `spot_top` holds the lists."""
    from tangram_amd.mapping_optimizer import Mapper, MapperConstrained
    S, G, d, M0 = _problem(40, 5, 70, 9)
    dense, hist0 = Mapper(S, G, d=d, lambda_d=1, device=device, M_init=M0).train(4, print_each=None)
    m = Mapper(S, G, d=d, lambda_d=1, device=device, M_init=M0)
    assert m.spot_top is None
    X, hist = m.train(4, print_each=None, spot_top_k=6)
    np.testing.assert_array_equal(X, dense)
    assert hist["main_loss"] == hist0["main_loss"]
    st = m.spot_top
    assert set(st) == {"spot_top_cells", "spot_top_values", "spot_top_k_mass", "spot_top_k"} and st["spot_top_k"] == 6
    assert st["spot_top_cells"].shape == st["spot_top_values"].shape == (70, 6) and st["spot_top_k_mass"].shape == (70,)
    assert_spot_topk_equals_dense((torch.as_tensor(st["spot_top_values"]), torch.as_tensor(st["spot_top_cells"])), dense, 6, "train")
    val, cells, mass = m.result_spot_topk(6, mass=True)
    np.testing.assert_array_equal(val.view(np.uint32), st["spot_top_values"].view(np.uint32))
    np.testing.assert_array_equal(cells, st["spot_top_cells"])
    np.testing.assert_array_equal(mass, st["spot_top_k_mass"])
    import scipy.sparse as sp
    Xs, _ = m.train(1, print_each=None, top_k=4, spot_top_k=3)                    # both at once
    assert sp.isspmatrix_csr(Xs) and m.spot_top["spot_top_k"] == 3 and m.spot_top["spot_top_cells"].shape == (70, 3)
    m.release()
    F0 = np.random.default_rng(3).standard_normal(40).astype(np.float32)
    kw = dict(lambda_d=1, target_count=20, device=device, M_init=M0, F_init=F0)
    Pd, Fd, _ = MapperConstrained(S, G, d, **kw).train(3, print_each=None)
    mc = MapperConstrained(S, G, d, **kw)
    Pc, Fc, _ = mc.train(3, print_each=None, spot_top_k=6)
    np.testing.assert_array_equal(Pc, Pd)
    np.testing.assert_array_equal(Fc, Fd)
    st = mc.spot_top
    assert_spot_topk_equals_dense((torch.as_tensor(st["spot_top_values"]), torch.as_tensor(st["spot_top_cells"])), Pd, 6, "constrained train")
    mc.release()


def check_map_cells_to_space_spot_top_k(device, mode):
    """map_cells_to_space(spot_top_k=5) against the same call without the key: X and every other key unchanged, the new keys with
    the specified shapes, their contents those of result_spot_topk of the same mapper; with top_k= as well both results are there."""
    import scipy.sparse as sp
    import tangram_amd as tg
    from tests.test_map_cells_to_space import _adatas
    kw = dict(mode=mode, device=device, num_epochs=4, random_state=42, verbose=False, keep_mapper=True)
    if mode == "constrained":
        kw.update(target_count=10, lambda_g2=1)
    plain = tg.map_cells_to_space(*_adatas(), **kw)
    top = tg.map_cells_to_space(*_adatas(), spot_top_k=5, **kw)
    C, V = plain.X.shape
    np.testing.assert_array_equal(np.asarray(top.X), np.asarray(plain.X))
    assert set(top.uns) == set(plain.uns) | {"spot_top_k"} and "spot_top_k" not in plain.uns and top.uns["spot_top_k"] == 5
    assert set(top.var.columns) == set(plain.var.columns) | {"spot_top_k_mass"} and set(top.obs.columns) == set(plain.obs.columns)
    assert set(top.varm.keys()) == set(plain.varm.keys()) | {"spot_top_cells", "spot_top_values"}
    cells, vals = np.asarray(top.varm["spot_top_cells"]), np.asarray(top.varm["spot_top_values"])
    assert cells.shape == vals.shape == (V, 5) and cells.dtype == np.int32 and vals.dtype == np.float32
    assert_spot_topk_equals_dense((torch.as_tensor(vals), torch.as_tensor(cells)), np.asarray(plain.X), 5, f"map_cells_to_space {mode}")
    v2, c2, mass = top._tangram_amd_mapper.result_spot_topk(5, mass=True)
    np.testing.assert_array_equal(v2.view(np.uint32), vals.view(np.uint32))
    np.testing.assert_array_equal(c2, cells)
    np.testing.assert_array_equal(top.var["spot_top_k_mass"].to_numpy(), mass)
    assert top.uns["train_genes_df"].equals(plain.uns["train_genes_df"])
    both = tg.map_cells_to_space(*_adatas(), spot_top_k=5, top_k=4, **kw)
    assert sp.isspmatrix_csr(both.X) and both.uns["top_k"] == 4 and both.uns["spot_top_k"] == 5 and "top_k_mass" in both.obs
    np.testing.assert_array_equal(np.asarray(both.varm["spot_top_cells"]), cells)
    np.testing.assert_array_equal(np.asarray(both.varm["spot_top_values"]).view(np.uint32), vals.view(np.uint32))
    for a in (plain, top, both):
        a._tangram_amd_mapper.release()
