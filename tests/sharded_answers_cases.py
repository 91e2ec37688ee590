"""Gene scores and the agreement of repeated mappings over spot shards (the second part: see the comment above AGREE_CASES): tables and checks shared by tests/test_sharded_answers.py (emulator, device "cpu") and
tests/test_gpu_sharded_answers.py (MI355X).  Under test: tg_score_merge (tg_score.h) behind tg_gene_scores_merge,
tangram_amd.gene_scores_sharded / ShardedGeneScorer, and score_genes(..., distributed=True).  The ranks are threads of one process on
one device (tests/local_comm.run_ranks); every rank holds the rows shard_bounds gives it.

PARTITIONS: 130 spots on 2 and 3 ranks (blocks of 65: one row past the 64-row slab of tg_score_partials; 44 / 43 / 43), 49 spots on 8
ranks (blocks of 7 and 6) and on 16 (4 and 3: every block inside one wave's rows), 1 010 spots on 9 and 16 ranks (blocks of 113 / 112,
and of 64 / 63: on both sides of the slab).  GENES: 1, 255, 256, 257 around the 256-gene strip of tg_score_partials and the 256
threads of a tg_score_merge workgroup (257: a second workgroup with one live thread).  Both layouts of gene_score_cases.planes: odd
pitches 4 bytes off a 16-byte boundary, and 16-byte aligned ones.

EXACT data (gene_score_cases.exact_planes: integers in [0, 7], at most 1 010 spots, every partial sum an integer < 2^16) carries no
tolerance: the merged moments and scores are NumPy's float64 values and those of the unsharded gene_scores on the whole planes, bit
for bit, on every rank.  GENERAL floats are held to the derived bounds of gene_score_cases (assert_within_bounds: a moment within
n_spots 2^-53 sum |terms| -- the bound of a sum in ANY order, so the ranks add nothing to it --, a score within 2 n_spots 2^-52 of the
definition evaluated in extended precision), n_spots the TOTAL number of spots: no term for the number of ranks.

score_genes(distributed=True) end to end: C = 33 cells, 8 training genes + 5 held out (+ 4 genes only in adata_sc), 1 010 spots on 9
ranks and 49 on 16 (the shapes of many_rank_cases), mappers trained 4 epochs on the shards; gene_block = 5 leaves blocks of 5, 5, 3.
Against compare_spatial_geneexp(project_genes(..., mapper=...)) of the same run: the same index set, columns, is_training and
sparsities; scores within score_bound(V) -- both routes score the same per-rank projection bits, only the fp64 order differs.

Largest |score - reference| seen (printed by the checks; the smallest bound of the table is 2.2e-14, at 49 spots):
                                               emulator     MI355X
    general floats against the definition      1.7e-16      1.7e-16     (both at 49 spots on 16 ranks; 1.1e-16 everywhere else)
    score_genes against the gathered route     8.4e-17      5.6e-17     (1 010 spots on 9 ranks; 49 on 16: 5.6e-17 and 0)
The largest moment error on the MI355X is 0.065 of its bound (49 spots on 8 ranks).  Without tg_gene_scores_merge every test of the two
modules but the table check fails (the symbol is missing); the 18 GPU tests take 6 s together on the MI355X.
"""
import ctypes as ct

import numpy as np
import pandas as pd
import pytest
import torch

from tangram_amd import _capi
from tests import gene_score_cases as gc

PARTITIONS = ((130, 2), (130, 3), (49, 8), (49, 16), (1010, 9), (1010, 16))
GENES = (1, gc.STRIP - 1, gc.STRIP, gc.STRIP + 1)
LAYOUTS = (False, True)                                   # gene_score_cases.planes(aligned=...)
FLOAT_GENES = (gc.STRIP + 1,)
E2E = ((9, 1010), (16, 49))                               # (world, spots)
E2E_C, E2E_TRAIN, E2E_OVERLAP, E2E_BLOCK, E2E_EPOCHS = 33, 8, 13, 5, 4


def bounds(V, world):
    from tangram_amd.sharded import shard_bounds
    return [shard_bounds(V, world, r) for r in range(world)]


def check_case_tables():
    widths = {p: sorted({hi - lo for lo, hi in bounds(*p)}) for p in PARTITIONS}
    assert widths[(130, 2)] == [65] and gc.SLAB == 64
    assert widths[(130, 3)] == [43, 44]
    assert widths[(49, 8)] == [6, 7] and widths[(49, 16)] == [3, 4]
    assert widths[(1010, 9)] == [112, 113] and widths[(1010, 16)] == [63, 64]
    assert GENES == (1, 255, 256, 257) and set(LAYOUTS) == {False, True}
    assert max(V for V, _ in PARTITIONS) * 49 < 2 ** 16                                   # exact sums in any order
    assert {w for _, w in PARTITIONS} >= {2, 3, 8, 9, 16}
    assert E2E_OVERLAP % E2E_BLOCK != 0 and E2E_OVERLAP > 2 * E2E_BLOCK and E2E_C == 33


def _np(t):
    return t.detach().cpu().numpy()


def _run(world, fn):
    from tests.local_comm import run_ranks
    return run_ranks(world, fn)


def sharded_scores(device, pred, meas, world, aligned):
    """gene_scores_sharded of the planes cut by shard_bounds, on `world` rank threads -> per rank (score, moments) as NumPy."""
    import tangram_amd as tg
    cuts = bounds(pred.shape[0], world)

    def rank_fn(comm):
        lo, hi = cuts[comm.rank]
        pv, mv = gc.planes(pred[lo:hi], meas[lo:hi], device, aligned)
        sc, mom = tg.gene_scores_sharded(pv, mv, comm, moments=True)
        assert sc.dtype == mom.dtype == torch.float64 and tuple(sc.shape) == (pred.shape[1],) and tuple(mom.shape) == (3, pred.shape[1])
        only = tg.gene_scores_sharded(pv, mv, comm)
        return _np(sc), _np(mom), _np(only)

    return _run(world, rank_fn)


def _same_on_every_rank(res, where):
    for r, (sc, mom, only) in enumerate(res):
        gc.assert_same_bits(sc, res[0][0], f"{where}: score on rank {r} against rank 0")
        gc.assert_same_bits(mom, res[0][1], f"{where}: moments on rank {r} against rank 0")
        gc.assert_same_bits(only, sc, f"{where}: rank {r}, the score without the moments")


def check_exact(device, V, world):
    """Every gene count and layout at this partition: NumPy float64 and the unsharded gene_scores, bit for bit, on every rank."""
    import tangram_amd as tg
    for n in GENES:
        pred, meas = gc.exact_planes(V, n, 1000 * V + 10 * world + n)
        mom_ref, sc_ref = gc.definition64(pred, meas)
        for aligned in LAYOUTS:
            where = f"{V} spots on {world} ranks x {n} genes, aligned={aligned}"
            one_sc, one_mom = tg.gene_scores(*gc.planes(pred, meas, device, aligned), moments=True)
            res = sharded_scores(device, pred, meas, world, aligned)
            _same_on_every_rank(res, where)
            gc.assert_same_bits(res[0][1], mom_ref, where + ": moments against NumPy float64")
            gc.assert_same_bits(res[0][0], sc_ref, where + ": score against NumPy float64")
            gc.assert_same_bits(res[0][1], _np(one_mom), where + ": moments against the unsharded gene_scores")
            gc.assert_same_bits(res[0][0], _np(one_sc), where + ": score against the unsharded gene_scores")


def check_general_floats(device, V, world):
    """The derived bounds of gene_score_cases for the TOTAL number of spots; nothing is added for the ranks."""
    for n in FLOAT_GENES:
        for aligned in LAYOUTS:
            pred, meas = gc.float_planes(V, n, V + n + world)
            pred[0], meas[0] = np.abs(pred[0]) + 0.5, meas[0] + 0.25                      # no zero column: every score is a number
            res = sharded_scores(device, pred, meas, world, aligned)
            where = f"floats, {V} spots on {world} ranks x {n} genes, aligned={aligned}"
            _same_on_every_rank(res, where)
            assert np.isfinite(res[0][0]).all()
            gc.assert_within_bounds(res[0][1], res[0][0], pred, meas, where)


def check_zero_columns(device, V=130, world=3, n=gc.STRIP + 1):
    """A column that is all zero on ONE rank only scores a finite number (its moments are the other ranks'); all zero on every rank:
    0 / 0 = NaN, as in the unsharded call.  The neighbours keep their bits."""
    cuts = bounds(V, world)
    pred, meas = gc.float_planes(V, n, 17)
    for lo, hi in cuts:                                                                   # every rank holds something of every column
        pred[lo], meas[lo] = 1.0, 2.0
    base = sharded_scores(device, pred, meas, world, False)
    assert np.isfinite(base[0][0]).all()
    lo, hi = cuts[1]
    one_p, one_m, all_p, all_m = 3, gc.STRIP, 5, 7                                        # (gene STRIP: the second merge workgroup)
    p, m = pred.copy(), meas.copy()
    p[lo:hi, one_p], m[lo:hi, one_m] = 0.0, 0.0
    p[:, all_p], m[:, all_m] = 0.0, 0.0
    res = sharded_scores(device, p, m, world, False)
    _same_on_every_rank(res, "zero columns")
    sc, mom = res[0][0], res[0][1]
    assert np.isfinite(sc[[one_p, one_m]]).all() and (mom[1, one_p] > 0) and (mom[2, one_m] > 0), "a column empty on one rank only"
    assert np.isnan(sc[[all_p, all_m]]).all() and mom[1, all_p] == 0 and mom[2, all_m] == 0 and (mom[0, [all_p, all_m]] == 0).all()
    gc.assert_within_bounds(mom, sc, p, m, "zero columns")
    live = np.setdiff1d(np.arange(n), [one_p, one_m, all_p, all_m])
    gc.assert_same_bits(sc[live], base[0][0][live], "neighbours of the zero columns")


def check_one_rank(device, V=65, n=9):
    """W = 1: the merge starts from rank 0's value, so it returns the bits of the unsharded call."""
    import tangram_amd as tg
    pred, meas = gc.float_planes(V, n, 3)
    sc1, mom1 = tg.gene_scores(*gc.planes(pred, meas, device, False), moments=True)
    res = sharded_scores(device, pred, meas, 1, False)
    gc.assert_same_bits(res[0][0], _np(sc1), "one rank: score")
    gc.assert_same_bits(res[0][1], _np(mom1), "one rank: moments")


def check_merge_arguments(device):
    """tg_gene_scores_merge: TG_ERR_INVALID (-1) with the library's message for NULLs, W < 1 and n_genes < 1; each output works
    alone and lies between sentinels; ascending rank order, starting from rank 0's value."""
    from tangram_amd.preprocess import _stream
    lib = _capi.lib()
    dev = torch.device(device)
    W, n = 3, 300
    st = _stream(dev)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((W, 3, n)) * 10.0 ** rng.integers(-8, 9, size=(W, 3, n))
    x[:, 1:] = np.abs(x[:, 1:])
    x[0, 0, 5] = -0.0
    x[1:, 0, 5] = 0.0
    inp = torch.as_tensor(x, device=dev)
    mom = torch.full((3 * n + 2,), -7.0, dtype=torch.float64, device=dev)
    sc = torch.full((n + 2,), -7.0, dtype=torch.float64, device=dev)
    I, MO, SC = inp.data_ptr(), mom.data_ptr() + 8, sc.data_ptr() + 8
    for args, msg in (((None, W, n, MO, SC, st), "NULL"), ((I, W, n, None, None, st), "every output is NULL"),
                      ((I, 0, n, MO, SC, st), "at least one"), ((I, -1, n, MO, SC, st), "at least one"),
                      ((I, W, 0, MO, SC, st), "at least one"), ((I, W, -5, MO, SC, st), "at least one"),
                      ((I + 4, W, n, MO, SC, st), "aligned"), ((I, W, n, I + 8 * n, SC, st), "overlaps"),
                      ((I, W, n, MO, I + 8 * (3 * n * W - 1), st), "overlaps")):
        rc = lib.tg_gene_scores_merge(*args)
        assert rc == -1, f"{msg}: returned {rc}"                                          # TG_ERR_INVALID
        with pytest.raises(ValueError, match=msg):
            _capi.check(rc)
    assert (_np(mom) == -7.0).all() and (_np(sc) == -7.0).all(), "a refused call wrote an output"
    want = x[0].copy()
    for r in range(1, W):
        want = want + x[r]                                                                # float64, rank order
    with np.errstate(invalid="ignore", divide="ignore"):
        want_sc = want[0] / (np.sqrt(want[1]) * np.sqrt(want[2]))
    _capi.check(lib.tg_gene_scores_merge(I, W, n, MO, None, st))
    assert (_np(sc) == -7.0).all(), "the scores were written although score_out is NULL"
    _capi.check(lib.tg_gene_scores_merge(I, W, n, None, SC, st))
    m, s = _np(mom), _np(sc)
    assert m[0] == m[-1] == s[0] == s[-1] == -7.0, "a sentinel next to an output was overwritten"
    gc.assert_same_bits(m[1:-1].reshape(3, n), want, "merge: moments in rank order")
    gc.assert_same_bits(s[1:-1], want_sc, "merge: score")
    assert not np.array_equal(want, x[::-1].cumsum(axis=0)[-1]), "the inputs: another order of the ranks gives other bits"
    one = torch.full((3, n), -7.0, dtype=torch.float64, device=dev)
    _capi.check(lib.tg_gene_scores_merge(I, 1, n, one.data_ptr(), None, st))
    gc.assert_same_bits(_np(one), x[0], "W = 1 returns rank 0's bits")
    assert np.signbit(_np(one)[0, 5]) and not np.signbit(m[1:-1].reshape(3, n)[0, 5])


# ---- score_genes(distributed=True) ---------------------------------------------------------------------------------------------
class ShardMapper:
    """What score_genes / project_genes look at of a Mapper made with distributed=True, around a shard of tests/local_comm."""

    def __init__(self, sh):
        self._sharded, self._engine = sh, sh.eng

    def project_genes_device(self, S_all=None):
        return self._sharded.project_full(S_all)


class Unsharded:
    _sharded = None
    _engine = None


def check_score_genes_distributed(device, world, V):
    import tangram_amd as tg
    from oracle import tangram_oracle as orc
    from tangram_amd.anndata_lite import AnnDataLite
    from tangram_amd.sharded import make_sharded
    seed = 100 + V
    pairs = [[gc.make_adatas(E2E_C, E2E_TRAIN, V, E2E_OVERLAP, seed=seed) for _ in range(2)] for _ in range(world)]    # drawn on this thread
    ad_sc, ad_sp = pairs[0][0]
    train = list(ad_sc.uns["training_genes"])
    genes = list(ad_sp.uns["overlap_genes"])
    S = gc._dense(ad_sc.X)[:, ad_sc.var.index.get_indexer(train)]
    G = gc._dense(ad_sp.X)[:, ad_sp.var.index.get_indexer(train)]
    d = np.asarray(ad_sp.obs["rna_count_based_density"], dtype=np.float32)
    M0 = orc.reference_init_M(E2E_C, V, 7)
    uns = {"train_genes_df": pd.DataFrame(index=train)}

    def rank_fn(comm):
        (sc1, sp1), (sc2, sp2) = pairs[comm.rank]
        sh = make_sharded(S, G, M0, d=d, device=device, precision="bf16x3", lambdas=dict(lambda_g1=1.0, lambda_d=1.0), comm=comm)
        try:
            sh.run(E2E_EPOCHS, 0.1, sh.eng.new_history(E2E_EPOCHS), 0)
            assert sh.eng.V < V
            ad_map = AnnDataLite(_np(sh.result_full()), obs=sc1.obs.copy(), var=sp1.obs.copy(), uns=uns)
            mapper = ShardMapper(sh)
            df = tg.score_genes(ad_map, sc1, sp1, mapper=mapper, distributed=True, gene_block=E2E_BLOCK, device=device)
            full = tg.compare_spatial_geneexp(tg.project_genes(ad_map, sc2, mapper=mapper, device=device), sp2, sc2, device=device)
            sub = tg.score_genes(ad_map, sc1, sp1, genes=[genes[6], genes[1]], mapper=mapper, distributed=True, gene_block=1, device=device)
            # refusals: all of them before anything collective happens
            with pytest.raises(ValueError, match="spot-sharded"):
                tg.score_genes(ad_map, sc1, sp1, mapper=mapper, device=device)
            with pytest.raises(ValueError, match="distributed=True"):
                tg.score_genes(ad_map, sc1, sp1, mapper=Unsharded(), distributed=True, device=device)
            with pytest.raises(ValueError, match="distributed=True"):
                tg.score_genes(ad_map, sc1, sp1, distributed=True, device=device)
            with pytest.raises(ValueError, match="truncated"):
                tg.score_genes(ad_map, sc1, sp1, mapper=mapper, distributed=True, truncated=True, device=device)
        finally:
            sh.release()
        return df, full, sub

    res = _run(world, rank_fn)
    df, full, sub = res[0]
    cols = ["score", "is_training", "sparsity_sp", "sparsity_sc", "sparsity_diff"]
    assert list(df.columns) == list(full.columns) == cols and sorted(df.index) == sorted(full.index) == sorted(genes)
    assert "only_sc0" not in df.index and len(df) == E2E_OVERLAP and df["is_training"].sum() == E2E_TRAIN
    assert set(df.index[df["is_training"]]) == set(train)
    for col in cols[1:]:
        np.testing.assert_array_equal(df.loc[genes, col].to_numpy(), full.loc[genes, col].to_numpy(), err_msg=col)
    assert np.isfinite(df["score"].to_numpy()).all() and (np.diff(df["score"].to_numpy()) <= 0).all()
    dev = gc.assert_scores_close(df.loc[genes, "score"].to_numpy(), full.loc[genes, "score"].to_numpy(), gc.score_bound(V),
                                 f"score_genes(distributed=True), {V} spots on {world} ranks, against the gathered route")
    for r, (df_r, _, sub_r) in enumerate(res):
        assert list(df_r.index) == list(df.index) and list(df_r.columns) == cols, f"rank {r}: another frame than rank 0"
        for col in cols:
            a, b = df_r[col].to_numpy(), df[col].to_numpy()
            if col == "is_training":
                np.testing.assert_array_equal(a, b, err_msg=f"rank {r}: {col}")
            else:
                gc.assert_same_bits(a, b, f"rank {r}: {col}")
        assert list(sub_r.index) == list(sub.index)
    assert sorted(sub.index) == sorted([genes[6], genes[1]]) and len(sub) == 2
    gc.assert_same_bits(sub.loc[[genes[6], genes[1]], "score"].to_numpy(), df.loc[[genes[6], genes[1]], "score"].to_numpy(), "genes= subset")
    return dev


# ---- agreement of repeated mappings over spot shards ---------------------------------------------------------------------------
# tg_consist_rows<R, MODE, true> / tg_consist_merge<R> behind tg_mapper_consistency_shard, tg_planes_consistency_shard and
# tg_consistency_merge; mapper_consistency / mapping_consistency on mappers that carry `_sharded`.  C = 33 cells; R handles per rank
# at step 0 (the row statistics of a shard are global from its creation on, so equal logits on two ranks are equal p).  Families of
# many_rank_cases: "normal" (N(0, 1)) and "peaked" (row 31: two equal maxima on neighbouring ranks -- the vote goes to the lower
# global spot; row 32: all its mass on rank 0; needs eight ranks or more).  References: the fp64 statements of
# tests/consistency_cases.py on the result_full() planes of the same handles, with its bounds as they stand: votes exact, Pearson
# 1e-9, vote entropy 1e-6, consensus entropy 1.5e-6.  Every output is bit-identical on every rank.
#
# Largest deviations seen (bounds 1e-9 / 1e-6 / 1.5e-6 / 1e-9):
#                 pearson                 vote entropy          consensus entropy                   gene_expr_consistency (S_val)
#     emulator    1.1e-15 (R = 8)         4.6e-8 (R = 8)        1.1e-7 (49 spots on 2 ranks)        1.2e-13
#     MI355X      1.1e-15 (R = 8)         4.6e-8 (R = 8)        1.2e-7 (1 010 spots on 2 ranks)     1.0e-13
# The 32 GPU tests of this part take under 4 s together on the MI355X.  Without the new entries every one of them fails on the
# NotImplementedError of mapper_consistency or on the missing symbols.
AGREE_C = 33
AGREE_CASES = (
    [dict(world=w, V=1010, R=r, family="normal") for w in (2, 3, 8, 9, 16) for r in (1, 2, 3)]
    + [dict(world=w, V=1010, R=r, family="peaked") for w in (8, 9, 16) for r in (2, 3)]
    + [dict(world=w, V=49, R=r, family=f) for w, r, f in ((2, 2, "normal"), (3, 3, "normal"), (8, 2, "peaked"), (9, 1, "peaked"), (16, 3, "peaked"))]
    + [dict(world=9, V=1010, R=8, family="peaked"),
       dict(world=16, V=16, R=2, family="normal"),                    # every block one spot wide
       dict(world=2, V=4100, R=2, family="normal")])                  # 2 050 local spots: past the 2 048-column chunk
for _c in AGREE_CASES:
    _c["id"] = "world{world}-V{V}-R{R}-{family}".format(**_c)
SVAL_CASES = ((3, 1010, 3), (16, 49, 2))                               # (world, V, R)


class ShardHandle:
    """What mapper_consistency looks at of a Mapper made with distributed=True."""

    def __init__(self, sh):
        self._sharded, self._engine = sh, sh.eng


def check_agreement_tables():
    assert {c["world"] for c in AGREE_CASES} == {2, 3, 8, 9, 16} and {c["R"] for c in AGREE_CASES} == {1, 2, 3, 8}
    for w in (2, 3, 8, 9, 16):
        assert {c["R"] for c in AGREE_CASES if c["world"] == w and c["V"] == 1010} >= {1, 2, 3}
    assert any(c["V"] == c["world"] == 16 for c in AGREE_CASES)
    assert any(c["V"] // c["world"] > 2048 for c in AGREE_CASES)
    assert {c["family"] for c in AGREE_CASES} == {"normal", "peaked"} and all(c["world"] >= 8 for c in AGREE_CASES if c["family"] == "peaked")
    assert len({c["id"] for c in AGREE_CASES}) == len(AGREE_CASES)


def _agree_logits(case):
    from tests import many_rank_cases as mr
    assert mr.C == AGREE_C
    V, world, R = case["V"], case["world"], case["R"]
    if case["family"] == "peaked":
        return [mr.peaked_logits(V, world, 1000 + 10 * r + world) for r in range(R)]
    rng = np.random.default_rng(V + world + R)
    return [rng.standard_normal((AGREE_C, V)).astype(np.float32) for _ in range(R)]


def _agree_shards(device, comm, V, logits):
    from tangram_amd.sharded import make_sharded
    from tests import consistency_cases as cc
    S, G, d, _ = _AGREE_PROBLEMS[V]
    return [make_sharded(S, G, M0, d=d, device=device, precision="bf16x3", lambdas=cc.LAM, comm=comm) for M0 in logits]


_AGREE_PROBLEMS = {}


def _agree_problem(V):
    from tests import consistency_cases as cc
    if V not in _AGREE_PROBLEMS:                                       # drawn on the calling thread, never on a rank thread
        _AGREE_PROBLEMS[V] = cc._problem(AGREE_C, 5, V, AGREE_C + V)
    return _AGREE_PROBLEMS[V]


def check_agreement_case(device, case):
    from tangram_amd import mapping_parameter_tuning as mpt
    from tests import consistency_cases as cc
    from tests import many_rank_cases as mr
    V, world, R = case["V"], case["world"], case["R"]
    logits = _agree_logits(case)
    _agree_problem(V)

    def rank_fn(comm):
        shs = _agree_shards(device, comm, V, logits)
        try:
            out = mpt.mapper_consistency([ShardHandle(s) for s in shs], votes=True)
            cube = np.stack([_np(s.result_full()) for s in shs])
            return {k: _np(v) for k, v in out.items()}, cube
        finally:
            for s in shs:
                s.release()

    res = _run(world, rank_fn)
    out, cube = res[0]
    assert cube.shape == (R, AGREE_C, V)
    for r, (o, _) in enumerate(res):
        cc.assert_same_bits(o, out, f"{case['id']}: rank {r} against rank 0")
    dev = cc.assert_against_oracle({k: torch.as_tensor(v) for k, v in out.items()}, cube, case["id"])
    if case["family"] == "peaked":
        cuts = bounds(V, world)
        a, b = (7, 8) if world > 8 else (6, 7)
        for r in range(R):
            row = cube[r, mr.ROW_TWO_MAXIMA]
            lo_spot, hi_spot = cuts[a][0] + 1, cuts[b][1] - 1
            assert row[lo_spot] == row[hi_spot] == row.max(), "the inputs: the tie across two ranks exists in p"
            assert out["votes"][r, mr.ROW_TWO_MAXIMA] == lo_spot, "a tie across ranks goes to the lower global spot"
            assert cuts[0][0] <= out["votes"][r, mr.ROW_ALL_ON_RANK0] < cuts[0][1]
    return dev


def check_agreement_with_s_val(device, world, V, R):
    """mapping_consistency(..., S_val) on shards: gene_expr_consistency from each rank's own projections against pearson_corr over
    the project_full planes, within 1e-9; the three cell-map metrics are those of mapper_consistency; the same dict on every rank."""
    from tangram_amd import mapping_parameter_tuning as mpt
    case = dict(world=world, V=V, R=R, family="normal")
    logits = _agree_logits(case)
    _agree_problem(V)
    S_val = np.abs(np.random.default_rng(V).standard_normal((AGREE_C, 7))).astype(np.float32)

    def rank_fn(comm):
        shs = _agree_shards(device, comm, V, logits)
        try:
            got = mpt.mapping_consistency([ShardHandle(s) for s in shs], S_val)
            ref = float(mpt.pearson_corr([s.project_full(S_val) for s in shs]).mean())
            out = mpt.mapper_consistency([ShardHandle(s) for s in shs])
            return got, ref, {k: _np(v) for k, v in out.items()}
        finally:
            for s in shs:
                s.release()

    res = _run(world, rank_fn)
    got, ref, out = res[0]
    assert set(got) == {"cell_map_consistency", "cell_map_agreement", "cell_map_certainty", "gene_expr_consistency"}
    for r, (g, _, _) in enumerate(res):
        assert g == got, f"rank {r} reports {g}, rank 0 {got}"
    d = abs(got["gene_expr_consistency"] - ref)
    print(f"consistency-dev S_val world{world}-V{V}-R{R}: gene_expr={d:.3e}")
    assert d <= 1e-9, f"gene_expr_consistency {got['gene_expr_consistency']!r} against {ref!r}"
    assert got["cell_map_consistency"] == float(out["pearson"].mean())
    assert got["cell_map_agreement"] == float(1.0 - out["vote_entropy"].astype(np.float64).mean())
    return d


def check_agreement_refusals(device):
    """Mixed sharded and unsharded mappers: ValueError on every rank before anything collective; tg_mapper_consistency on a shard still
    returns TG_ERR_UNSUPPORTED; the new entries refuse NULLs and sizes out of range with TG_ERR_INVALID."""
    from tangram_amd import mapping_parameter_tuning as mpt
    from tangram_amd._device import workspace
    from tests import consistency_cases as cc
    V, world = 49, 2
    logits = _agree_logits(dict(world=world, V=V, R=2, family="normal"))
    _agree_problem(V)
    plain = cc.make_engines(device, AGREE_C, V, logits[:1])

    def rank_fn(comm):
        shs = _agree_shards(device, comm, V, logits)
        try:
            with pytest.raises(ValueError, match="mixture"):
                mpt.mapper_consistency([ShardHandle(shs[0]), plain[0]])
            with pytest.raises(ValueError, match="mixture"):
                mpt.mapping_consistency([plain[0], ShardHandle(shs[1])])
            lib, e0 = shs[0].eng._lib, shs[0].eng
            ws = workspace(lib.tg_consistency_query_bytes, 2, AGREE_C, device=e0.device, min_bytes=8)
            o = torch.zeros(AGREE_C, dtype=torch.float32, device=e0.device)
            arr = (ct.c_void_p * 2)(*[s.eng._h for s in shs])
            rc = lib.tg_mapper_consistency(arr, 2, ws.data_ptr(), None, o.data_ptr(), None, None)
            assert rc == -4, f"tg_mapper_consistency on a shard returned {rc}"                 # TG_ERR_UNSUPPORTED
            nb = ct.c_size_t()
            pk = torch.zeros(512, dtype=torch.int64, device=e0.device)
            for rc in (lib.tg_consistency_packet_bytes(2, AGREE_C, None), lib.tg_consistency_packet_bytes(9, AGREE_C, ct.byref(nb)),
                       lib.tg_consistency_packet_bytes(2, -1, ct.byref(nb)),
                       lib.tg_mapper_consistency_shard(None, 2, ws.data_ptr(), pk.data_ptr()),
                       lib.tg_mapper_consistency_shard(arr, 0, ws.data_ptr(), pk.data_ptr()),
                       lib.tg_mapper_consistency_shard(arr, 2, None, pk.data_ptr()),
                       lib.tg_mapper_consistency_shard(arr, 2, ws.data_ptr(), None),
                       lib.tg_consistency_merge(None, 2, 2, AGREE_C, 8 * 512, V, AGREE_C * V, None, o.data_ptr(), None, None, None),
                       lib.tg_consistency_merge(pk.data_ptr(), 0, 2, AGREE_C, 8 * 256, V, AGREE_C * V, None, o.data_ptr(), None, None, None),
                       lib.tg_consistency_merge(pk.data_ptr(), 2, 2, AGREE_C, 8 * 16, V, AGREE_C * V, None, o.data_ptr(), None, None, None),
                       lib.tg_consistency_merge(pk.data_ptr(), 2, 2, AGREE_C, 8 * 256, 1, AGREE_C, None, o.data_ptr(), None, None, None),
                       lib.tg_consistency_merge(pk.data_ptr(), 2, 2, AGREE_C, 8 * 256, V, AGREE_C * V, None, None, None, None, None)):
                assert rc == -1, rc                                                            # TG_ERR_INVALID
            return True
        finally:
            for s in shs:
                s.release()

    try:
        assert all(_run(world, rank_fn))
    finally:
        for e in plain:
            e.release()
