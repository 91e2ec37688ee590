"""Tables and checks of the top-k result path (tg_topk.h: tg_row_topk, tg_topk_merge_rows; tg_mapper_result_topk / tg_topk_merge;
HipMapperEngine / ShardedMapperEngine / Mapper(.Constrained).result_topk; train(top_k=), map_cells_to_space(top_k=)), shared by
tests/test_topk.py (emulator, device "cpu") and tests/test_gpu_topk.py (MI355X).

Every reference is exact: the expected entries of a row are `np.lexsort((np.arange(V), -P[c]))[:k]` of the DENSE result of the same
handle -- value descending, equal values by ascending spot -- and values are compared as bit patterns.  No tolerance appears, except
the 1e-6 the float64 `top_k_mass` column is given against the float32 rows it sums."""
import ctypes as ct

import numpy as np
import pytest
import torch

from tangram_amd import _capi

CHUNK = _capi.TOPK_CHUNK
KS = (1, 2, 7, 64)
LAM = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5)

# (C, K, V, precision): row lengths around the 64-lane wave, the 256-thread workgroup and the 1 024-spot float4 sweep of one
# workgroup; 40 cells take the GEMM kernels, 18 the clusters-mode kernels; the chunk cases (3 rows: under 1 MB of logits) put the
# row end on, next to and two chunks past the chunk boundary.
KERNEL_CASES = [(40, 5, V, "bf16x3") for V in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025)] + \
               [(18, 5, V, "bf16x3") for V in (65, 257)] + \
               [(3, 5, V, "bf16x3") for V in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)] + \
               [(40, 5, 257, "fp32"), (40, 5, 257, "bf16")]
TIE_LAYOUTS = ("one-chunk", "across-the-chunk-boundary")
MERGE_CHUNK = 512                 # TG_MERGE_CHUNK of tg_topk.h: entries tg_topk_merge_rows ranks at a time, k survivors carried on
# past one chunk (the carry of tg_topk_merge_rows): one entry, k - 1, k and k + 1 entries (k = 64) into the second chunk -- 576 is nine
# shards of 64 --, one short of two chunks, two chunks (sixteen shards of 64), one entry into the third and into the fourth
MERGE_CARRY_N = (513, 575, 576, 577, 1023, 1024, 1025, 1537)
MERGE_CASES = [(n_in, k) for k in (1, 5, 64) for n_in in sorted({k, 2 * k, 3 * k + 1, 512}) + list(MERGE_CARRY_N)]
# worlds 9 and 16: the lists of a row are 9 k and 16 k long, 576 and 1 024 at k = 64 (131 spots: every shard narrower than k)
SHARD_CASES = [(world, V, k) for world in (2, 3) for V, k in ((100, 7), (10, 5), (131, 64))] + \
              [(world, V, k) for world in (9, 16) for V, k in ((131, 64), (1010, 64), (100, 7))]


def check_case_tables():
    assert {V for _, _, V, _ in KERNEL_CASES} >= {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3}
    assert {C for C, _, _, _ in KERNEL_CASES} == {3, 18, 40} and {p for *_, p in KERNEL_CASES} == {"bf16x3", "fp32", "bf16"}
    assert all(C * V * 4 < (1 << 20) for C, _, V, _ in KERNEL_CASES if V >= CHUNK - 1)
    assert {n for n, _ in MERGE_CASES} >= {1, 2, 4, 5, 10, 16, 64, 128, 193, 512} | set(MERGE_CARRY_N) and {k for _, k in MERGE_CASES} == {1, 5, 64}
    assert set(MERGE_CARRY_N) == {513, 575, 576, 577, 1023, 1024, 1025, 1537} and MERGE_CHUNK == 512
    assert all((n, k) in MERGE_CASES for n in MERGE_CARRY_N for k in (1, 5, 64))
    assert {(w, V) for w, V, _ in SHARD_CASES} == {(w, V) for w in (2, 3) for V in (100, 10, 131)} | {(w, V) for w in (9, 16) for V in (131, 1010, 100)}
    assert all(-(-10 // 3) < k for w, V, k in SHARD_CASES if (w, V) == (3, 10))             # every shard narrower than k
    assert {(w, w * k) for w, V, k in SHARD_CASES if V == 131 and w > 8} == {(9, 576), (16, 1024)}      # n_in of the merge: past one chunk
    assert all(-(-131 // w) < k for w, V, k in SHARD_CASES if V == 131 and w > 8)


def check_limits():
    """_capi.TOPK_MAX / TOPK_CHUNK mirror the kernel header."""
    out = (ct.c_int32 * 2)()
    assert _capi.lib().tg_debug_topk_limits(out) == 0
    assert (out[0], out[1]) == (_capi.TOPK_MAX, _capi.TOPK_CHUNK) == (64, CHUNK)


def host_topk(P, k):
    """(values, indices) [C, k] of the dense rows P: value descending, equal values by ascending column."""
    idx = np.stack([np.lexsort((np.arange(P.shape[1]), -P[c]))[:k] for c in range(P.shape[0])])
    return np.take_along_axis(P, idx, 1), idx.astype(np.int32)


def _np(t):
    return t.detach().cpu().numpy()


def assert_topk_equals_dense(got, P, k, where):
    val, idx = (_np(x) for x in got)
    assert val.shape == idx.shape == (P.shape[0], k) and val.dtype == np.float32 and idx.dtype == np.int32, where
    rv, ri = host_topk(P, k)
    np.testing.assert_array_equal(idx, ri, err_msg=f"{where}: indices (an index >= {P.shape[1]} is a padding column)")
    np.testing.assert_array_equal(val.view(np.uint32), np.ascontiguousarray(rv).view(np.uint32), err_msg=f"{where}: value bits")


def _problem(C, K, V, seed):
    from tests import parity_common as pc
    return pc.validation_problem(C, K, V, seed)


def check_kernel_case(device, C, K, V, precision):
    """result_topk against the dense result of the same handle, before any step (row statistics of tg_row_stats) and after 3 (row
    statistics carried by the update kernels), for every k of KS that the row admits and k = V on rows of at most 64 spots."""
    from tangram_amd.engine import HipMapperEngine
    S, G, d, M0 = _problem(C, K, V, C + V)
    e = HipMapperEngine(S, G, M0, d=d, device=device, precision=precision, lambdas=LAM)
    ks = sorted({k for k in KS if k <= V} | ({V} if V <= _capi.TOPK_MAX else set()))
    for steps in (0, 3):
        if steps:
            e.step(steps, 0.1, e.new_history(steps), 0)
        P = _np(e.result())
        for k in ks:
            assert_topk_equals_dense(e.result_topk(k), P, k, f"C{C} V{V} {precision} k={k} after {steps} steps")
    e.release()


def tie_logits(layout):
    """(M0 [6, V], expected {row: {k: indices}}): the rows a comparison of values alone gets wrong."""
    V = 300 if layout == "one-chunk" else CHUNK + 70
    edge = 150 if layout == "one-chunk" else CHUNK                      # the ties sit on both sides of `edge`
    rng = np.random.default_rng(V)
    M = np.zeros((6, V), dtype=np.float32)
    M[0] = np.round(rng.standard_normal(V) * 2) / 2                      # multiples of 0.5: many exact ties, also at the k-th place
    M[1] = 0.25                                                          # all equal: the first k spots
    M[2, edge + 5] = 200.0                                               # the rest underflows to exactly 0: the peak, then spots 0, 1, ...
    M[3] = -4.0                                                          # a plateau of 9 equal logits straddling `edge` under one peak
    M[3, edge - 3:edge + 6] = 3.0
    M[3, edge + 10] = 5.0
    M[4] = np.round(rng.standard_normal(V)) * 0.5
    M[4, edge - 40:edge + 40] = 2.5                                      # 80 ties at the top: more than any k, across `edge`
    M[5] = np.round(rng.standard_normal(V) * 2) / 2
    M[5, :edge] -= 8.0                                                   # everything that matters lies behind `edge`
    expect = {1: {k: list(range(k)) for k in KS},
              2: {k: [edge + 5] + list(range(k - 1)) for k in KS},
              3: {7: [edge + 10] + list(range(edge - 3, edge + 3)), 2: [edge + 10, edge - 3]},
              4: {k: list(range(edge - 40, edge - 40 + k)) for k in KS}}
    return M, expect


def check_ties(device, layout):
    from tangram_amd.engine import HipMapperEngine
    M0, expect = tie_logits(layout)
    C, V = M0.shape
    S, G, d, _ = _problem(C, 5, V, 3)
    e = HipMapperEngine(S, G, M0, d=d, device=device, precision="bf16x3", lambdas=LAM)
    P = _np(e.result())
    assert (P[2] == 0).sum() == V - 1 and P[2, np.argmax(M0[2])] == 1.0, "the +200 row must underflow to exact zeros"
    assert len(np.unique(P[0])) < V // 4 and len(np.unique(P[1])) == 1
    for k in KS:
        got = e.result_topk(k)
        assert_topk_equals_dense(got, P, k, f"ties {layout} k={k}")
        idx = _np(got[1])
        for row, by_k in expect.items():
            if k in by_k:
                assert idx[row].tolist() == by_k[k], (layout, row, k, idx[row].tolist())
    e.step(3, 0.1, e.new_history(3), 0)
    P = _np(e.result())
    for k in KS:
        assert_topk_equals_dense(e.result_topk(k), P, k, f"ties {layout} k={k} after 3 steps")
    e.release()


def check_constrained(device):
    """Constrained mode: softmax(M) without the filter, i.e. the first array of result(with_filter=True)."""
    from tangram_amd.engine import HipMapperEngine
    from oracle import tangram_oracle as orc
    C, K, V = 40, 12, 100
    data = orc.make_synthetic(C, K, V, seed=5)
    M0, F0 = orc.reference_init_MF_constrained(C, V, 6)
    lam = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5, lambda_count=1.0, lambda_f_reg=1.0)
    e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], F0=F0, mode="constrained", device=device, lambdas=lam, target_count=20.0)
    for steps in (0, 3):
        if steps:
            e.step(steps, 0.1, e.new_history(steps), 0)
        P, F = e.result(with_filter=True)
        for k in KS:
            assert_topk_equals_dense(e.result_topk(k), _np(P), k, f"constrained k={k} after {steps} steps")
        np.testing.assert_array_equal(_np(e.filter_values()), _np(F))          # the filter without the dense plane
    e.release()


def merge_reference(val, idx, k):
    pad = idx < 0
    out_v = np.zeros((val.shape[0], k), dtype=np.float32)
    out_i = np.full((val.shape[0], k), -1, dtype=np.int32)
    for r in range(val.shape[0]):
        order = np.lexsort((idx[r], -val[r].astype(np.float64), pad[r]))[:k]      # pads last, value descending, index ascending
        order = order[~pad[r][order]]
        out_v[r, :len(order)] = val[r][order]
        out_i[r, :len(order)] = idx[r][order]
    return out_v, out_i


def check_merge(device, n_in, k):
    """tg_topk_merge alone: lists with duplicated values, pads (index -1, with values above every real one: a pad must lose on its
    index alone), a row of pads only and a row without pads, at a pitch larger than the list."""
    dev = torch.device(device)
    rng = np.random.default_rng(1000 * n_in + k)
    n_rows, ld = 9, n_in + 3
    val = (rng.integers(0, 6, size=(n_rows, ld)) / 4).astype(np.float32)
    idx = np.stack([rng.permutation(4 * n_in + 7)[:ld] for _ in range(n_rows)]).astype(np.int32)
    pad = rng.random((n_rows, ld)) < 0.3
    pad[5] = True
    pad[6] = False
    pad[7, : n_in - min(n_in, max(k - 1, 1))] = True                          # fewer than k real entries where the list allows
    idx[pad] = -1
    val[pad] = 9.0
    ri = _merge_against_reference(dev, val, idx, n_in, k, "")
    assert (ri[5] == -1).all() and (ri[6] >= 0).sum() == min(k, n_in)
    if n_in > MERGE_CHUNK:
        val, idx, expect = merge_carry_rows(n_in, k)
        ri = _merge_against_reference(dev, val, idx, n_in, k, " (carry rows)")
        for row, want in expect.items():
            got = ri[CARRY_ROWS[row]].tolist()[:len(want)]            # (fewer than k placed entries: they lead, the background follows)
            assert got == want, (row, n_in, k, got, want)


def _merge_against_reference(dev, val, idx, n_in, k, what):
    """tg_topk_merge on the lists val / idx [n_rows, ld >= n_in] against merge_reference, indices equal and values bit for bit;
    returns the reference's indices."""
    n_rows, ld = val.shape
    tv, ti = torch.as_tensor(val, device=dev), torch.as_tensor(idx, device=dev)
    out_v = torch.full((n_rows, k), 7.0, dtype=torch.float32, device=dev)
    out_i = torch.full((n_rows, k), 7, dtype=torch.int32, device=dev)
    stream = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
    _capi.check(_capi.lib().tg_topk_merge(tv.data_ptr(), ti.data_ptr(), n_rows, n_in, ld, k, out_v.data_ptr(), out_i.data_ptr(), stream))
    rv, ri = merge_reference(val[:, :n_in], idx[:, :n_in], k)
    np.testing.assert_array_equal(_np(out_i), ri, err_msg=f"merge n_in={n_in} k={k}{what}: indices")
    np.testing.assert_array_equal(_np(out_v).view(np.uint32), rv.view(np.uint32), err_msg=f"merge n_in={n_in} k={k}{what}: values")
    return ri


# The rows of merge_carry_rows: lists longer than one chunk of tg_topk_merge_rows, built so that the k entries carried from chunk to
# chunk decide the result.
CARRY_ROWS = dict(winners_last=0, winners_first=1, winners_first_scattered=2, tie_across_512=3, pads_interleaved=4, first_chunk_all_pads=5,
                  later_chunk_all_pads=6, fewer_than_k=7, none_real=8, signs_zeros_denormals=9, zeros_across_512=10)


def merge_carry_rows(n_in, k):
    """(val [11, n_in + 3] float32, idx int32, {row name: expected indices}) for n_in > MERGE_CHUNK.  Real entries of a row carry
    pairwise different spot indices in an order unrelated to their position; the background lies in [-3, -2); a pad has index -1 and
    the value 9 (above every real one: it must lose on its index alone).

    winners_last             the k largest values at the last k positions (the last chunk and, where it is shorter than k, the end of
                             the one before): nothing of the first chunk survives
    winners_first(_scattered) the k largest at positions 0 .. k - 1, and scattered over the first chunk: the result is the carry alone
    tie_across_512           one value at positions 512 - k .. 512 + k - 1; the positions from 512 on hold the lower spot indices, so
                             the winners arrive in the later chunk and displace equal carried entries
    pads_interleaved         every second entry a pad;  first_chunk_all_pads / later_chunk_all_pads: positions 0 .. 511 / 512 .. 1023
                             (or to the end) are pads -- a chunk that adds nothing to the carry, a carry of pads only
    fewer_than_k             k - 1 real entries (none for k = 1), half of them behind position 512: the row ends in (0, -1)
    none_real                pads only
    signs_zeros_denormals    the candidates are +-1e-40 and +-1.4e-45 (denormals), +0.0, -0.0, -1.0 and 2^-126, on both sides of 512; the
                             rest of the row is below -2, so every k takes them in float order
    zeros_across_512         +0.0 and -0.0 are the largest values, they compare equal as floats: the lower spot index wins whatever its
                             sign bit and its chunk, and the sign bit comes out as it went in"""
    assert n_in > MERGE_CHUNK and 1 <= k <= 64
    rng = np.random.default_rng(7000 * n_in + k)
    n_rows, ld, E = len(CARRY_ROWS), n_in + 3, MERGE_CHUNK
    val = -2.0 - rng.random((n_rows, ld), dtype=np.float32)
    idx = np.stack([rng.permutation(4 * n_in + 7)[:ld] for _ in range(n_rows)]).astype(np.int32)
    top = (5.0 + np.arange(k, dtype=np.float32))[rng.permutation(k)]
    expect = {}

    def put(row, pos, values):
        r = CARRY_ROWS[row]
        val[r, pos] = values
        order = np.lexsort((idx[r, pos], -np.asarray(values, dtype=np.float64)))[:k]
        expect[row] = idx[r, np.asarray(pos)[order]].tolist()

    put("winners_last", np.arange(n_in - k, n_in), top)
    put("winners_first", np.arange(k), top)
    put("winners_first_scattered", np.sort(rng.permutation(E)[:k]), top)
    r = CARRY_ROWS["tie_across_512"]
    pos = np.arange(E - k, min(E + k, n_in))
    idx[r, pos] = np.sort(idx[r, pos])[::-1]                    # descending spot index along the positions: the later, the better
    val[r, pos] = 3.0
    expect["tie_across_512"] = idx[r, pos[::-1][:k]].tolist()
    assert idx[r, pos[-1]] < idx[r, pos[0]] and pos[-1] >= E > pos[0]
    pads = np.zeros((n_rows, ld), dtype=bool)
    pads[CARRY_ROWS["pads_interleaved"], 0::2] = True
    pads[CARRY_ROWS["first_chunk_all_pads"], :E] = True
    pads[CARRY_ROWS["later_chunk_all_pads"], E:2 * E] = True
    r = CARRY_ROWS["fewer_than_k"]
    real = np.concatenate([rng.permutation(E)[:(k - 1) // 2], E + rng.permutation(n_in - E)[:min(k - 1 - (k - 1) // 2, n_in - E)]]).astype(int)
    pads[r] = True
    pads[r, real] = False
    pads[CARRY_ROWS["none_real"]] = True
    small = np.array([1e-40, -1e-40, 1.4e-45, -1.4e-45, 0.0, -0.0, -1.0, 2.0 ** -126], dtype=np.float32)
    assert (np.abs(small[:4]) > 0).all() and (np.abs(small[:4]) < 2.0 ** -126).all() and np.signbit(small[5])
    last = n_in - 1 if n_in - 1 > E else 400                   # (513: position 512 is the last one)
    put("signs_zeros_denormals", np.array([3, E - 1, E, last, 100, E - 2, 7, 300]), small)
    r = CARRY_ROWS["zeros_across_512"]
    pos = np.array([10, 20, E - 1, E, last])
    idx[r, pos] = np.sort(idx[r, pos])[[3, 1, 4, 0, 2]]        # the lowest spot index sits behind position 512, on a -0.0
    val[r, pos] = np.array([0.0, -0.0, 0.0, -0.0, -0.0], dtype=np.float32)
    order = np.argsort(idx[r, pos])[:k]
    expect["zeros_across_512"] = idx[r, pos[order]].tolist()
    idx[pads] = -1
    val[pads] = 9.0
    expect["none_real"] = [-1] * k
    rv, ri = merge_reference(val[:, :n_in], idx[:, :n_in], k)
    n_real = len(real)
    assert n_real < k and (ri[CARRY_ROWS["fewer_than_k"], :n_real] >= 0).all() and (ri[CARRY_ROWS["fewer_than_k"], n_real:] == -1).all()
    expect["fewer_than_k"] = ri[CARRY_ROWS["fewer_than_k"]].tolist()
    assert (ri[CARRY_ROWS["first_chunk_all_pads"]] >= 0).sum() == min(k, n_in - E)
    for row in ("later_chunk_all_pads", "pads_interleaved"):
        assert (ri[CARRY_ROWS[row]] >= 0).all(), row
    return val, idx, expect


def check_shards(device, world, V, k, C=40, K=5, n=3):
    """Spot shards (threads, tests/local_comm.py): every rank's result_topk after n steps is the top-k of that run's result_full()."""
    from tangram_amd.sharded import make_sharded
    from tests.local_comm import run_ranks
    S, G, d, M0 = _problem(C, K, V, 13 + V)

    def rank_fn(comm):
        sh = make_sharded(S, G, M0, d=d, device=device, precision="bf16x3", lambdas=LAM, comm=comm)
        sh.run(n, 0.1, sh.eng.new_history(n), 0)
        P = _np(sh.result_full())
        got = tuple(_np(x) for x in sh.result_topk(k))
        local = tuple(_np(x) for x in sh.eng.result_topk(k))
        sh.release()
        return P, got, local, sh.eng.V

    res = run_ranks(world, rank_fn)
    P = res[0][0]
    assert P.shape == (C, V)
    for r in range(world):
        np.testing.assert_array_equal(res[r][0], P)
        np.testing.assert_array_equal(res[r][1][0].view(np.uint32), res[0][1][0].view(np.uint32), err_msg=f"rank {r}: other values than rank 0")
        np.testing.assert_array_equal(res[r][1][1], res[0][1][1], err_msg=f"rank {r}: other indices than rank 0")
        width = res[r][3]                                                       # a shard narrower than k ends its rows in (0, -1)
        assert (res[r][2][1][:, min(width, k):] == -1).all() and (res[r][2][0][:, min(width, k):] == 0).all()
        assert (res[r][2][1][:, :min(width, k)] >= 0).all()
    assert_topk_equals_dense(tuple(torch.as_tensor(x) for x in res[0][1]), P, k, f"{world} shards V{V} k={k}")


def _state_of(e):
    M, m1, m2, step = e.logits()
    return [_np(x).copy() for x in (M, m1, m2)] + [step]


def check_undisturbed(device, C=40, K=5, V=257):
    """2 steps, result_topk (twice: the same bits), 2 steps == 4 steps: history, logits and both Adam moments bit for bit,
    padding columns included."""
    from tangram_amd.engine import HipMapperEngine
    S, G, d, M0 = _problem(C, K, V, C + V)
    res = []
    for ask in (True, False):
        e = HipMapperEngine(S, G, M0, d=d, device=device, precision="bf16x3", lambdas=LAM)
        hist = e.new_history(4)
        e.step(2, 0.1, hist, 0)
        if ask:
            a, b = e.result_topk(7), e.result_topk(7)
            np.testing.assert_array_equal(_np(a[0]).view(np.uint32), _np(b[0]).view(np.uint32))
            np.testing.assert_array_equal(_np(a[1]), _np(b[1]))
        e.step(2, 0.1, hist, 2)
        res.append([_np(hist).copy()] + _state_of(e))
        e.release()
    for name, x, y in zip(("history", "M", "exp_avg", "exp_avg_sq", "step"), res[0], res[1]):
        np.testing.assert_array_equal(x, y, err_msg=name)


def check_argument_errors(device):
    """The TG_ERR_INVALID cases raise ValueError with the library's message; the handle stays usable."""
    from tangram_amd.engine import HipMapperEngine
    S, G, d, M0 = _problem(40, 5, 10, 1)
    e = HipMapperEngine(S, G, M0, d=d, device=device, precision="bf16x3", lambdas=LAM)
    for k, msg in ((0, "outside"), (-3, "outside"), (65, "outside"), (11, "exceeds the 10 spots")):
        with pytest.raises(ValueError, match=msg):
            e.result_topk(k)
    buf = torch.zeros((40, 4), dtype=torch.float32, device=e.device)
    ibuf = torch.zeros((40, 4), dtype=torch.int32, device=e.device)
    lib = _capi.lib()
    for val, idx in ((None, ibuf.data_ptr()), (buf.data_ptr(), None)):
        with pytest.raises(ValueError, match="NULL"):
            e._call(lib.tg_mapper_result_topk, e._h, 4, val, idx)
    for k in (0, 65):
        with pytest.raises(ValueError, match="outside"):
            e.topk_merge(buf, ibuf, k)
    with pytest.raises(ValueError, match="null"):
        _capi.check(lib.tg_topk_merge(buf.data_ptr(), ibuf.data_ptr(), 40, 4, 4, 2, None, ibuf.data_ptr(), e._hip_stream))
    with pytest.raises(ValueError, match="bad lists"):
        _capi.check(lib.tg_topk_merge(buf.data_ptr(), ibuf.data_ptr(), 40, 4, 3, 2, buf.data_ptr(), ibuf.data_ptr(), e._hip_stream))
    assert_topk_equals_dense(e.result_topk(10), _np(e.result()), 10, "after the refused calls")
    e.release()


def check_train_top_k(device):
    """Mapper.train(top_k=4): a canonical CSR matrix whose entries are the dense run's at the kept places (same M_init)."""
    import scipy.sparse as sp
    from tangram_amd.mapping_optimizer import Mapper, MapperConstrained
    S, G, d, M0 = _problem(40, 5, 70, 9)
    dense, _ = Mapper(S, G, d=d, lambda_d=1, device=device, M_init=M0).train(4, print_each=None)
    m = Mapper(S, G, d=d, lambda_d=1, device=device, M_init=M0)
    X, hist = m.train(4, print_each=None, top_k=4)
    assert sp.isspmatrix_csr(X) and X.shape == dense.shape and X.dtype == np.float32 and X.has_canonical_format
    assert (np.diff(X.indptr) == 4).all() and len(hist["main_loss"]) == 4
    rv, ri = host_topk(dense, 4)
    for c in range(dense.shape[0]):
        cols = X.indices[X.indptr[c]:X.indptr[c + 1]]
        assert sorted(cols.tolist()) == cols.tolist() == sorted(ri[c].tolist())
        np.testing.assert_array_equal(X.data[X.indptr[c]:X.indptr[c + 1]].view(np.uint32), dense[c, cols].view(np.uint32))
    val, idx = m.result_topk(4)
    assert isinstance(val, np.ndarray) and isinstance(idx, np.ndarray)
    np.testing.assert_array_equal(idx, ri)
    np.testing.assert_array_equal(val.view(np.uint32), np.ascontiguousarray(rv).view(np.uint32))
    m.release()
    F0 = np.random.default_rng(3).standard_normal(40).astype(np.float32)
    kw = dict(lambda_d=1, target_count=20, device=device, M_init=M0, F_init=F0)
    Pd, Fd, _ = MapperConstrained(S, G, d, **kw).train(3, print_each=None)
    mc = MapperConstrained(S, G, d, **kw)
    Xc, Fc, _ = mc.train(3, print_each=None, top_k=4)
    np.testing.assert_array_equal(Fc, Fd)
    rv, ri = host_topk(Pd, 4)
    np.testing.assert_array_equal(mc.result_topk(4)[1], ri)
    np.testing.assert_array_equal(np.asarray(Xc.todense())[np.arange(40)[:, None], ri].view(np.uint32), np.ascontiguousarray(rv).view(np.uint32))
    mc.release()


def check_map_cells_to_space_top_k(device, mode):
    """map_cells_to_space(top_k=4) against the dense call on the synthetic AnnData of tests/test_map_cells_to_space.py, and
    project_genes on its sparse result."""
    import scipy.sparse as sp
    import tangram_amd as tg
    from tests.test_map_cells_to_space import _adatas
    kw = dict(mode=mode, device=device, num_epochs=4, random_state=42, verbose=False, keep_mapper=True)
    if mode == "constrained":
        kw.update(target_count=10, lambda_g2=1)
    ad_sc, ad_sp = _adatas()
    dense = tg.map_cells_to_space(ad_sc, ad_sp, **kw)
    ad_sc2, ad_sp2 = _adatas()
    top = tg.map_cells_to_space(ad_sc2, ad_sp2, top_k=4, **kw)
    assert sp.isspmatrix_csr(top.X) and top.X.shape == dense.X.shape and (np.diff(top.X.indptr) == 4).all()
    assert top.uns["top_k"] == 4 and top.obs["top_k_mass"].dtype == np.float64
    rv, ri = host_topk(np.asarray(dense.X), 4)
    np.testing.assert_allclose(top.obs["top_k_mass"].to_numpy(), rv.astype(np.float64).sum(axis=1), rtol=0, atol=1e-6)
    np.testing.assert_array_equal(np.asarray(top.X.todense())[np.arange(ri.shape[0])[:, None], ri].view(np.uint32),
                                  np.ascontiguousarray(rv).view(np.uint32))
    assert top.uns["train_genes_df"].equals(dense.uns["train_genes_df"])
    hd, ht = dense.uns["training_history"], top.uns["training_history"]
    assert set(hd) == set(ht)
    for key in hd:
        np.testing.assert_array_equal(np.asarray(hd[key]), np.asarray(ht[key]), err_msg=key)
    if mode == "constrained":
        np.testing.assert_array_equal(top.obs["F_out"].to_numpy(), dense.obs["F_out"].to_numpy())
    with pytest.raises(ValueError, match=r"mapper=adata_map\._tangram_amd_mapper"):
        tg.project_genes(top, _adatas()[0], device=device)
    ge_top = tg.project_genes(top, _adatas()[0], mapper=top._tangram_amd_mapper)
    ge_dense = tg.project_genes(dense, _adatas()[0], mapper=dense._tangram_amd_mapper)
    np.testing.assert_array_equal(np.asarray(ge_top.X), np.asarray(ge_dense.X))
    top._tangram_amd_mapper.release()
    dense._tangram_amd_mapper.release()
