"""Spot shards on 8, 9, 12 and 16 ranks: tables and checks shared by tests/test_many_ranks.py (emulator, device "cpu") and
tests/test_gpu_many_ranks.py (MI355X).

Every per-rank loop of the kernels is unrolled eight wide, so it takes a second trip (or fills a second half) only from nine ranks
on: tg_merge_stats_body<false> (tg_update.h: `p0 += 8`, once for the maximum and once for Z, and the history tail summed over all
ranks), tg_merge_stats_body<true> (the halves h = 0, 1 of pm[16] / pz[16]), tg_peer_exchange, tg_link_sum, tg_link_sum2, tg_link_get8
(tg_peer.h: `r0 += 8`, the rank-order sum carried over the trip boundary), and tg_topk_merge_rows (tg_topk.h) ranks more than one
chunk of 512 entries only when nine shards or more send k = 64 entries each (tests/topk_cases.py: MERGE_CASES, SHARD_CASES).
WORLDS: 8 is the last single trip, 9 puts one rank into the second, 12 leaves it ragged, 16 fills it (TG_PEER_MAX).

The training step (check_step_case): C = 33 cells, K = 8 genes, V = 1 010 spots -- on 16 ranks two shards of 64 spots and fourteen
of 63, on both sides of the 64-float pitch, ragged on 9 and 12 too -- and V = 49, shards of 3 or 4 spots; callback transport through
tests/local_comm.run_ranks (ranks are threads of one process).  Starting logits: "normal", the reference's N(0, 1) draw, and
"peaked" (peaked_logits): row c has its maximum, 20 above the rest of the row, in the shard of rank c mod world, so from nine ranks
on some rows' maxima arrive in the second trip and the first trip's terms are rescaled by exp(pm - mx), others the other way round;
row 32 keeps all its mass on rank 0 (+200: every other rank's partial is scaled by an exp(pm - mx) that is exactly 0 in float32);
row 31 has two equal maxima, on ranks 7 and 8 (6 and 7 on eight ranks).  Checked: the same history bits on every rank; every history
column per epoch, the final mapping and the filter against the fp64 oracle (parity_common.update_row_oracle) within
parity_common.TOL[precision] -- the bounds of the 2- to 4-rank tests, none is widened for the larger world --; rows of the mapping sum
to 1 within the same bound.

Largest values measured over the step table (hist: |delta| / max(1, |ref|) over the columns; P, filter: max |delta|; rows: max
|sum - 1|; in brackets: the cases of world 16 alone):
    emulator    bound hist / P     hist                P                   filter              rows
    fp32        1e-5 / 2e-4        1.9e-7 (1.2e-7)     9.2e-7 (9.2e-7)     -                   2.1e-7 (8.7e-8)
    bf16x3      1e-5 / 2e-4        2.7e-7 (2.7e-7)     1.5e-6 (9.2e-7)     -                   2.2e-7 (1.7e-7)
    bf16        1e-3 / 5e-2        2.1e-4 (2.1e-4)     1.7e-4 (1.7e-4)     3.8e-7 (1.9e-7)     1.7e-7 (1.7e-7)
    MI355X
    fp32        1e-5 / 2e-4        3.7e-7 (2.9e-7)     9.2e-7 (9.2e-7)     -                   1.7e-7 (1.3e-7)
    bf16x3      1e-5 / 2e-4        3.7e-7 (3.4e-7)     1.6e-6 (9.2e-7)     -                   2.1e-7 (1.5e-7)
    bf16        1e-3 / 5e-2        2.1e-4 (2.1e-4)     1.7e-4 (1.7e-4)     3.8e-7 (1.9e-7)     1.6e-7 (1.6e-7)
Sixteen partials instead of four in the rank-order sums leave every figure where eight ranks put it, a factor of 25 and more under
its bound: every bound is parity_common.TOL as it stands, no term count enters one.  The 42 GPU tests of
tests/test_gpu_many_ranks.py take 6 s together on the MI355X; the emulator module takes four to five minutes.

Also here: the spatial terms on nine blocks of 56 spots (V = 501: the last block 53, Vsr no multiple of the block), the empty block
(V = 17 on 16 ranks: every rank raises the same ValueError before any collective), and -- emulator only -- the peer transport at 9 and
16 ranks: tg_peer_exchange as all-reduce and all-gather, and whole sharded steps, fused and with TG_PEER_FUSED=0, bit-identical to
the callback transport.

Perturbations of a scratch copy, run on the emulator (none committed); new: failures among the tests this change adds --
step[w]: the ten test_training_step_on_many_shards cases of world w; spatial: test_spatial_terms_on_nine_blocks; val[..]:
test_emulated_validation_on_spot_shards; merge[n-k]: test_topk.py::test_merge_kernel; shards[..]: test_topk.py::test_spot_shards;
peer[..]: test_peer_transport_equals_the_callback_transport.  Every run of step[8] passes under (a), (c), (d), (e): eight ranks
are one trip.
    perturbation                                                         new tests that fail
    (a) tg_merge_stats_body<false>: both loops stop at `p0 < 8`            33: step[9], step[12], step[16] (all 30), spatial, val[world9-genes300],
                                                                           val[world16-genes300-gene-empty-on-a-shard]
    (b) ... its second pass without `* tg_exp(pm[q] - mx)`                 43: step[8], step[9], step[12], step[16] (all 40), spatial, both val cases
                                                                           (and the three older val cases of 2 and 3 ranks)
    (c) ... the history tail summed over the first 8 ranks only           31: step[9], step[12], step[16] (all 30), spatial
    (d) tg_merge_stats_body<true> skips the half h = 1                    4: peer[world9-*-fused], peer[world16-*-fused] (plain and constrained)
    (e) tg_link_sum restarts `s` at r0 = 8                                 4: the same four fused peer cases
    (f) tg_topk_merge_rows: `ncarry = 0` after every chunk                 28: merge[n-k] for the 8 n past 512 x k in (1, 5, 64), shards[9-131-64],
                                                                           [9-1010-64], [16-131-64], [16-1010-64]
    (g) tg_topk_merge_rows writes the later chunks at `list[i]`            28: the same 28
Each of the seven is caught.  The emulator runs the work-items of a workgroup one after the other, so it cannot show a missing
barrier; between tg_topk_rank_keep and the next chunk's stores stands the barrier that ends tg_topk_rank_keep, and the GPU runs of
test_merge_kernel (20 rows a case, 11 of them built for the carry) pass with it.

Found by these tests: tg_topk_merge_rows ordered -0.0 behind +0.0 (its key is the bit pattern; as floats the two are equal and the
lower spot index decides): the new merge cases failed from merge[513-1] on, on the rows zeros_across_512 and signs_zeros_denormals
of topk_cases.merge_carry_rows.  The kernel now gives -0.0 the key of +0.0 and carries its sign bit beside the index.
"""
import functools
import os

import numpy as np

from tests import parity_common as pc

WORLDS = (8, 9, 12, 16)
C, K = 33, 8
V_WIDE, V_NARROW = 1010, 49
EPOCHS = 4
LR = 0.1
# (variant, precision): plain in fp32 and bf16x3, the regularisers, and constrained mode in bf16 (the path that reads rscale with the gate)
VARIANTS = (("plain", "fp32"), ("plain", "bf16x3"), ("regularised", "bf16x3"), ("constrained", "bf16"))
FAMILIES = ("normal", "peaked")
ROW_TWO_MAXIMA, ROW_ALL_ON_RANK0 = C - 2, C - 1
PEAK = 20.0

SPATIAL_CASE = dict(world=9, C=60, K=18, V=501, T=5, n=4)
EMPTY_BLOCK_CASE = dict(world=16, V=17)
PEER_WORLDS = (9, 16)
PEER_EXCHANGE_N = (1, 511, 512, 513)


def _case(world, V, variant, precision, family):
    return dict(id=f"world{world}-V{V}-{variant}-{precision}-{family}", world=world, V=V, variant=variant, precision=precision, family=family)


def step_cases():
    """Every world x variant x family at 1 010 spots; at 49 spots the peaked plain run and the N(0, 1) constrained one."""
    out = [_case(w, V_WIDE, v, p, f) for w in WORLDS for v, p in VARIANTS for f in FAMILIES]
    out += [_case(w, V_NARROW, v, p, f) for w in WORLDS for v, p, f in (("plain", "bf16x3", "peaked"), ("constrained", "bf16", "normal"))]
    return out


def shard_widths(V, world):
    from tangram_amd.sharded import shard_bounds
    return [hi - lo for lo, hi in (shard_bounds(V, world, r) for r in range(world))]


def check_case_tables():
    from tangram_amd.sharded import shard_bounds
    from tests import topk_cases as tc
    cases = step_cases()
    assert WORLDS == (8, 9, 12, 16) and {c["world"] for c in cases} == set(WORLDS) and max(WORLDS) == 16     # 16: TG_PEER_MAX
    for w in WORLDS:
        for V in (V_WIDE, V_NARROW):
            assert {(c["variant"], c["precision"]) for c in cases if (c["world"], c["V"]) == (w, V)} >= {("plain", "bf16x3"), ("constrained", "bf16")}
            assert {c["family"] for c in cases if (c["world"], c["V"]) == (w, V)} == set(FAMILIES)
        assert {(c["variant"], c["precision"], c["family"]) for c in cases if (c["world"], c["V"]) == (w, V_WIDE)} == \
            {(v, p, f) for v, p in VARIANTS for f in FAMILIES}
    assert sorted(shard_widths(V_WIDE, 16)) == [63] * 14 + [64] * 2 and sorted(shard_widths(V_NARROW, 16)) == [3] * 15 + [4]
    assert all(len(set(shard_widths(V_WIDE, w))) == 2 for w in (9, 12, 16)), "1 010 spots must be ragged on 9, 12 and 16 ranks"
    s = SPATIAL_CASE
    blocks = [shard_bounds(s["V"], s["world"], r, True) for r in range(s["world"])]
    assert [hi - lo for lo, hi in blocks] == [56] * 8 + [53]
    assert (s["world"] * 56) % 16 != 0 and (-(-s["world"] * 56 // 16) * 16) % 56 != 0     # Vsr = rup(9 * 56, TG_RB = 16) = 512: past the blocks, no multiple of one
    e = EMPTY_BLOCK_CASE
    assert (e["world"] - 1) * -(-e["V"] // e["world"]) >= e["V"]
    assert set(tc.MERGE_CARRY_N) == {513, 575, 576, 577, 1023, 1024, 1025, 1537}
    assert PEER_WORLDS == (9, 16) and PEER_EXCHANGE_N == (1, 511, 512, 513)


def peaked_logits(V, world, seed):
    """float32 logits [C, V] of the peaked family (module docstring) for `world` balanced shards."""
    from tangram_amd.sharded import shard_bounds
    rng = np.random.default_rng(seed)
    bounds = [shard_bounds(V, world, r) for r in range(world)]
    M = rng.standard_normal((C, V)) * (PEAK / 4.0)
    for c in range(C):
        lo, hi = bounds[c % world]
        M[c, rng.integers(lo, hi)] = M[c].max() + PEAK
    a, b = (7, 8) if world > 8 else (6, 7)
    M[ROW_TWO_MAXIMA] = rng.standard_normal(V) * (PEAK / 4.0)
    top = np.float32(M[ROW_TWO_MAXIMA].max() + PEAK)
    M[ROW_TWO_MAXIMA, [bounds[a][0] + 1, bounds[b][1] - 1]] = top
    M[ROW_ALL_ON_RANK0] = rng.standard_normal(V)
    M[ROW_ALL_ON_RANK0, bounds[0][0] + 2] += 200.0
    M = M.astype(np.float32)
    assert (M != 0).all()                                   # (sign(0) in the L1 term is a knife edge: tests/trained_state_cases.py)
    home = M.argmax(axis=1)
    rank_of = np.array([next(r for r, (lo, hi) in enumerate(bounds) if lo <= v < hi) for v in home])
    assert (rank_of[:C - 2] == np.arange(C - 2) % world).all() and rank_of[ROW_ALL_ON_RANK0] == 0
    assert (M[ROW_TWO_MAXIMA] == top).sum() == 2 and M[ROW_TWO_MAXIMA, bounds[a][0] + 1] == M[ROW_TWO_MAXIMA, bounds[b][1] - 1] == M[ROW_TWO_MAXIMA].max()
    if world > 8:
        assert set(rank_of[:C - 2]) & set(range(8, world)) and set(rank_of[:C - 2]) & set(range(8))
    lo, hi = bounds[0]
    off = np.delete(M[ROW_ALL_ON_RANK0], np.arange(lo, hi))
    assert (np.exp(np.float32(off.max()) - M[ROW_ALL_ON_RANK0].max(), dtype=np.float32) == 0).all()      # the other ranks' partials underflow
    return M


@functools.lru_cache(maxsize=None)
def _problem(V, variant):
    return pc.update_row_problem(C, K, V, variant, C + V)


def start_logits(V, variant, family, world):
    data, lam, M0, F0 = _problem(V, variant)
    if family == "peaked":
        M0 = peaked_logits(V, world, C + V + world)
    return data, lam, M0, F0


@functools.lru_cache(maxsize=None)
def oracle_run(V, variant, family, world, n=EPOCHS):
    """The fp64 oracle's n epochs: (terms per epoch, final mapping, final filter values or None).  The N(0, 1) start does not depend
    on the world: one run serves all four."""
    from oracle import tangram_oracle as orc
    data, lam, M0, F0 = start_logits(V, variant, family, world)
    o = pc.update_row_oracle(data, lam, M0, F0, variant)
    hist = [o.step(LR) for _ in range(n)]
    F = 1.0 / (1.0 + np.exp(-o.F)) if variant == "constrained" else None
    return hist, orc.softmax_rows(o.M), F


def _rank_run(make, device, V, variant, precision, family, world, n, profile, start=None):
    """One rank of a sharded run; `make(**kw)` is make_sharded with the communicator or the transport filled in.  `start`: the
    problem, where the caller drew it already (rank threads must not draw it themselves: the draw seeds NumPy's global generator)."""
    data, lam, M0, F0 = start or start_logits(V, variant, family, 8 if family == "normal" else world)
    kw = dict(F0=F0, mode="constrained", target_count=0.4 * C) if variant == "constrained" else {}
    sh = make(S=data["S"], G=data["G"], M0=M0, d=data["d"], device=device, precision=precision, lambdas=lam, **kw)
    hist = sh.eng.new_history(n)
    sh.run(n - 1, LR, hist, 0)
    if profile:
        sh.eng.profile(True)
    sh.run(1, LR, hist, n - 1)
    out = dict(names=[k for k, _, _ in sh.eng.profile_read()] if profile else None)
    try:
        sh.peer_check()
        out["timed_out"] = False
    except RuntimeError:
        out["timed_out"] = True
    res = sh.result_full(with_filter=True) if variant == "constrained" else (sh.result_full(), None)
    out.update(hist=hist.cpu().numpy().copy(), M=sh.eng.logits()[0][:, :sh.eng.V].cpu().numpy().copy(), P=res[0].cpu().numpy(),
               F=None if res[1] is None else res[1].cpu().numpy())
    sh.release()
    return out


def run_shards(device, world, V, variant, precision, family, transport="callbacks", n=EPOCHS, profile=False):
    """The sharded run on `world` threads (tests/local_comm.py); per rank a dict: hist [n, H_NTERMS], M (this rank's logits), P (the
    full mapping), F (the filter values, constrained mode), names (kernel names of the last step when `profile`), timed_out."""
    from tangram_amd.sharded import make_sharded
    from tests.local_comm import run_ranks
    start = start_logits(V, variant, family, 8 if family == "normal" else world)
    return run_ranks(world, lambda comm: _rank_run(lambda **kw: make_sharded(comm=comm, transport=transport, **kw), device, V, variant,
                                                   precision, family, world, n, profile, start))


def history_columns(variant, lam):
    from tangram_amd import _capi
    cols = [(_capi.H_TOTAL, "total_loss"), (_capi.H_MAIN, "main_loss"), (_capi.H_VG, "vg_reg"), (_capi.H_KL, "kl_reg")]
    if "lambda_r" in lam:
        cols.append((_capi.H_ENTROPY, "entropy_reg"))
    if variant == "constrained":
        cols += [(_capi.H_COUNT, "count_reg"), (_capi.H_FREG, "lambda_f_reg")]
    return cols


def check_step_case(device, case):
    world, V, variant, precision, family = (case[k] for k in ("world", "V", "variant", "precision", "family"))
    tol = pc.TOL[precision]
    res = run_shards(device, world, V, variant, precision, family)
    hist_o, Po, Fo = oracle_run(V, variant, family, 8 if family == "normal" else world)
    lam = _problem(V, variant)[1]
    out = dict(hist=0.0)
    for r in range(world):
        np.testing.assert_array_equal(res[r]["hist"], res[0]["hist"], err_msg=f"rank {r} reports another history than rank 0")
        np.testing.assert_array_equal(res[r]["P"], res[0]["P"], err_msg=f"rank {r} holds another mapping than rank 0")
    h, P, F = res[0]["hist"].astype(np.float64), res[0]["P"].astype(np.float64), res[0]["F"]
    errs = {}
    for col, k in history_columns(variant, lam):
        ref = np.array([float(t[k]) for t in hist_o])
        assert np.isfinite(ref).all(), f"inputs: {k} of the fp64 oracle {ref}"
        assert np.isfinite(h[:, col]).all(), f"{k}: {h[:, col]} where the fp64 oracle has {ref}"
        errs[k] = float(np.abs(h[:, col] - ref).max()) / max(1.0, float(np.abs(ref).max()))
        out["hist"] = max(out["hist"], errs[k])
    assert P.shape == (C, V) and np.isfinite(P).all()
    out["P"] = float(np.abs(P - Po).max())
    out["rows"] = float(np.abs(res[0]["P"].sum(axis=1, dtype=np.float64) - 1.0).max())
    if variant == "constrained":
        out["F"] = float(np.abs(F.astype(np.float64) - Fo).max())
    print(f"many-rank case {case['id']}: {out}")
    for k, err in errs.items():
        assert err <= tol["loss"], f"{k}: max per-epoch |delta| / max(1, |ref|) = {err:.3e} > {tol['loss']:.0e}"
    assert out["P"] <= tol["P"], f"max|P - Po| = {out['P']:.3e} > {tol['P']:.0e}"
    assert out["rows"] <= tol["P"], f"rows of result() sum to 1 +- {out['rows']:.3e} > {tol['P']:.0e}"
    if variant == "constrained":
        assert out["F"] <= tol["P"], f"filter: max|F - Fo| = {out['F']:.3e} > {tol['P']:.0e}"
    if family == "peaked":
        row = res[0]["P"][ROW_ALL_ON_RANK0]
        assert row.max() == 1.0 and (np.delete(row, int(row.argmax())) < 2.0 ** -100).all(), "the row with all its mass on rank 0"
    return out


# ---- spatial terms on nine blocks ---------------------------------------------------------------------------------------------
def check_spatial_blocks(device, precision="bf16x3"):
    """Neighbourhood, cell-type islands and one autocorrelation term (Moran) on nine spot blocks of 56 spots, the last of 53 --
    the comparisons and bounds of test_spatial_terms_on_spot_shards_match_single_engine (tests/test_gpu_parity.py, 2 and 3 ranks):
    the same history on every rank, history and mapping against the single engine, the total loss and the mapping against the
    fp64 oracle."""
    from oracle import tangram_oracle as orc
    from tangram_amd.engine import HipMapperEngine
    from tangram_amd.sharded import make_sharded
    from tangram_amd.synthetic import hex_grid_graph
    from tangram_amd import _capi
    from tests.local_comm import run_ranks
    s = SPATIAL_CASE
    world, Cs, Ks, V, T, n = (s[k] for k in ("world", "C", "K", "V", "T", "n"))
    data = orc.make_synthetic(Cs, Ks, V, seed=19, n_types=T)
    M0 = orc.reference_init_M(Cs, V, 2)
    N, W = hex_grid_graph(V)
    Ws = orc.grid_graph(V, standardized=True, self_inclusion=False)
    lam = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.3, lambda_neighborhood_g1=0.96, lambda_ct_islands=0.17, lambda_moran=0.3)
    graphs = dict(voxel_weights=W, neighborhood_filter=N, ct_encode=data["ct_encode"], spatial_weights=Ws)

    def rank_fn(comm):
        sh = make_sharded(data["S"], data["G"], M0, d=data["d"], device=device, precision=precision, lambdas=lam, comm=comm, **graphs)
        assert sh.spatial and sh.eng.V == (56 if comm.rank < 8 else 53)
        hist = sh.eng.new_history(n)
        sh.run(n, 0.1, hist)
        out = hist.cpu().numpy(), sh.result_full().cpu().numpy()
        sh.release()
        return out

    res = run_ranks(world, rank_fn)
    e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], device=device, precision=precision, lambdas=lam, **graphs)
    h1 = e.new_history(n)
    e.step(n, 0.1, h1)
    h1, P1 = h1.cpu().numpy(), e.result().cpu().numpy()
    e.release()
    o = orc.OracleMapper(data["S"], data["G"], d=data["d"], M0=M0, dtype=np.float64, voxel_weights=W.toarray(),
                         neighborhood_filter=N.toarray(), ct_encode=data["ct_encode"], spatial_weights=Ws, **lam)
    Po, ho = o.train(n, 0.1)
    cols = [_capi.H_TOTAL, _capi.H_MAIN, _capi.H_VG, _capi.H_KL, _capi.H_NB, _capi.H_CT, _capi.H_MORAN]
    assert np.isfinite(h1[:, cols]).all()
    for hist, P in res:
        np.testing.assert_array_equal(hist, res[0][0])
        np.testing.assert_allclose(hist[:, cols], h1[:, cols], atol=5e-6, rtol=2e-6)
        np.testing.assert_allclose(P, P1, atol=2e-6)
        np.testing.assert_allclose(hist[:, _capi.H_TOTAL], np.array(ho["total_loss"]), atol=2e-5, rtol=1e-5)
        assert np.abs(P - Po).max() < 2e-4


def check_empty_block(device):
    """17 spots on 16 ranks with a spatial term: blocks of ceil(17 / 16) = 2 spots leave ranks 9 to 15 without a spot.  Every rank
    raises the same ValueError, naming V and the world, before it enters a collective (a rank that went on would wait in
    run_ranks' barrier for the ones that raised, and run_ranks would report a broken barrier)."""
    from oracle import tangram_oracle as orc
    from tangram_amd.sharded import make_sharded
    from tests.local_comm import run_ranks
    world, V = EMPTY_BLOCK_CASE["world"], EMPTY_BLOCK_CASE["V"]
    data = orc.make_synthetic(C, K, V, seed=4, n_types=3)
    M0 = orc.reference_init_M(C, V, 5)
    W = orc.grid_graph(V, standardized=True, self_inclusion=True)
    lam = dict(lambda_g1=1.0, lambda_d=1.0, lambda_neighborhood_g1=0.5)

    def rank_fn(comm):
        try:
            sh = make_sharded(data["S"], data["G"], M0, d=data["d"], device=device, precision="bf16x3", lambdas=lam, comm=comm, voxel_weights=W)
        except ValueError as e:
            return str(e)
        sh.release()
        return None

    msgs = run_ranks(world, rank_fn)
    assert all(m is not None for m in msgs), f"ranks {[r for r, m in enumerate(msgs) if m is None]} constructed their shard"
    assert len(set(msgs)) == 1, msgs
    assert "V=17" in msgs[0] and "world=16" in msgs[0] and "own no spots" in msgs[0], msgs[0]

    # the balanced partition of a run without spatial terms gives every rank a spot: the same shape trains
    def plain_fn(comm):
        sh = make_sharded(data["S"], data["G"], M0, d=data["d"], device=device, precision="bf16x3", lambdas=dict(lambda_g1=1.0, lambda_d=1.0), comm=comm)
        hist = sh.eng.new_history(1)
        sh.run(1, LR, hist)
        out = hist.cpu().numpy().copy()
        sh.release()
        return out

    hists = run_ranks(world, plain_fn)
    assert np.isfinite(hists[0][:, 0]).all() and all(np.array_equal(h, hists[0], equal_nan=True) for h in hists)


# ---- the peer transport at 9 and 16 ranks (emulator) -------------------------------------------------------------------------
# One PROCESS per rank, as in tests/test_sharded_gloo.py (gloo bootstraps, POSIX shared memory stands in for the hipIpc mailboxes):
# the emulator is one machine per process and runs one kernel at a time, so a kernel that waits for its peers' kernels needs them in
# other processes.  The `world` processes are started once per world (peer_processes) and run every peer case of that world.
PEER_VARIANTS = (("plain", "bf16x3"), ("constrained", "bf16"))


def _exchange_inputs(world, n):
    rng = np.random.default_rng(100 * world + n)
    return (rng.standard_normal((world, n)) * 10.0 ** rng.integers(-3, 4, size=(world, n))).astype(np.float32)


def _fused_env(fused):
    if fused:
        os.environ.pop("TG_PEER_FUSED", None)
    else:
        os.environ["TG_PEER_FUSED"] = "0"


def _peer_worker(rank, world, port, sim_path, outdir):
    import ctypes as ct
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["TG_PEER_TIMEOUT_MS"] = "60000"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tangram_amd import _capi
        from tangram_amd.sharded import make_sharded
        _capi._install_library_for_tests(sim_path)
        lib = _capi.lib()
        out = {}
        # tg_peer_exchange alone: all-reduce and all-gather of n floats
        c, h = ct.c_void_p(), ct.create_string_buffer(64)
        _capi.check(lib.tg_comm_peer_create(world, rank, 1024, 0, h, ct.byref(c)))
        mine = torch.frombuffer(bytearray(h.raw), dtype=torch.uint8).clone()
        outs = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(outs, mine)
        _capi.check(lib.tg_comm_peer_connect(c, b"".join(bytes(o.numpy().tobytes()) for o in outs)))
        dist.barrier()
        for n in PEER_EXCHANGE_N:
            x = _exchange_inputs(world, n)
            red, gat = x[rank].copy(), np.full(world * n, np.nan, dtype=np.float32)
            _capi.check(lib.tg_comm_all_reduce_sum(c, red.ctypes.data, n, None))
            _capi.check(lib.tg_comm_all_gather(c, x[rank].ctypes.data, gat.ctypes.data, n, None))
            out[f"reduce-{n}"], out[f"gather-{n}"] = red, gat
        flag = ct.c_int(-1)
        _capi.check(lib.tg_comm_peer_status(c, ct.byref(flag)))
        out["exchange-timed-out"] = np.array(flag.value)
        dist.barrier()
        lib.tg_comm_destroy(c)
        # whole sharded runs over transport="peer"
        for variant, precision in PEER_VARIANTS:
            for fused in (True, False):
                _fused_env(fused)
                res = _rank_run(lambda **kw: make_sharded(transport="peer", **kw), "cpu", V_WIDE, variant, precision, "normal", world, EPOCHS, True)
                for k in ("hist", "M", "P", "F"):
                    if res[k] is not None:
                        out[f"{variant}-{int(fused)}-{k}"] = res[k]
                out[f"{variant}-{int(fused)}-timed-out"] = np.array(int(res["timed_out"]))
                out[f"{variant}-{int(fused)}-exchanges"] = np.array(sum(k.startswith("exchange_") for k in res["names"]))
        np.savez(os.path.join(outdir, f"peer_{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def peer_processes(world, sim_path, outdir):
    """Starts the `world` rank processes (once per world) and returns their results, in rank order."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    old = os.environ.get("TG_PEER_FUSED")
    try:
        mp.spawn(_peer_worker, args=(world, port, sim_path, outdir), nprocs=world, join=True)
    finally:
        if old is None:
            os.environ.pop("TG_PEER_FUSED", None)
        else:
            os.environ["TG_PEER_FUSED"] = old
    return [dict(np.load(os.path.join(outdir, f"peer_{r}.npz"))) for r in range(world)]


def check_peer_exchange(res, world, n):
    """tg_peer_exchange alone (tg_comm_all_reduce_sum / tg_comm_all_gather of n floats on `world` rank processes): the all-reduce is
    the float32 sum in rank order, bit for bit and the same on every rank; the all-gather returns every rank's vector; no poll
    timed out."""
    x = _exchange_inputs(world, n)
    want = x[0].copy()
    for r in range(1, world):
        want = want + x[r]                                   # float32, rank order
    for r in range(world):
        assert int(res[r]["exchange-timed-out"]) == 0, f"rank {r}: a poll timed out"
        np.testing.assert_array_equal(res[r][f"reduce-{n}"].view(np.uint32), want.view(np.uint32), err_msg=f"all-reduce of {n} floats on rank {r} of {world}")
        np.testing.assert_array_equal(res[r][f"gather-{n}"].view(np.uint32), x.reshape(-1).view(np.uint32), err_msg=f"all-gather of {n} floats on rank {r} of {world}")
    if n > 1:                                                 # the inputs: a sum that stopped or restarted at rank 8 is another number
        assert not np.array_equal(want, x[:8].sum(axis=0, dtype=np.float32)) and not np.array_equal(want, x[8:].sum(axis=0, dtype=np.float32))


def check_peer_step(res, world, variant, precision, fused):
    """A sharded run over transport="peer", with its exchanges inside the kernels (fused) or in exchange kernels (TG_PEER_FUSED=0):
    history, this rank's logits, the mapping and the filter bit-identical to the rank-order callback transport on the same shards
    (threads of this process), rank by rank; no poll timed out; the path asked for is the path taken."""
    assert (variant, precision) in PEER_VARIANTS
    ref = run_shards("cpu", world, V_WIDE, variant, precision, "normal", transport="callbacks", profile=True)
    tag = f"{variant}-{int(fused)}-"
    for r in range(world):
        assert int(res[r][tag + "timed-out"]) == 0, f"rank {r}: a peer exchange timed out"
        assert (int(res[r][tag + "exchanges"]) > 0) == (not fused), f"rank {r}: fused={fused} but the step ran {int(res[r][tag + 'exchanges'])} exchange kernels"
        assert [k for k in ref[r]["names"] if k.startswith("exchange_")], ref[r]["names"]
        assert np.isfinite(res[r][tag + "hist"][:, :4]).all(), f"rank {r}: history {res[r][tag + 'hist'][:, :4]}"
        for k in ("hist", "M", "P") + (("F",) if variant == "constrained" else ()):
            np.testing.assert_array_equal(res[r][tag + k], ref[r][k], err_msg=f"world {world}, rank {r}: {k} over the peer transport")
        np.testing.assert_array_equal(res[r][tag + "hist"], res[0][tag + "hist"])
