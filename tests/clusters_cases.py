"""The clusters-mode kernels (tangram_amd/csrc/tg_small.h: tg_sc_forward, tg_sc_backward, their batched twins, tg_prep_ssmall) at
every cluster count and tile edge: the table and the checks shared by tests/test_clusters_kernels.py (emulator, device "cpu") and
tests/test_gpu_clusters_kernels.py (MI355X).

Every step case goes through parity_common.update_row_case(smallc=True, precision="bf16x3", n=3): the first-step gradient per row in
the max norm and the last four columns on their own, P element-wise relative, Adam's denominator, the history columns of the terms
that are on, the padding, and the path (tg_debug_layout, tg_sc_forward / tg_sc_backward in the profile).  Bounds: the fp32 row of
ROW_TOL (5e-5) and TOL["fp32"]["loss"] (1e-5) -- the clusters-mode kernels compute in exact fp32 whatever precision is asked for.
The seed of a case is C + K + V.  The sweeps (the smallest shapes at which each piece can still go wrong):

    A  every cluster count C = 1 .. 32 at K = 70, V = 70: Kp = 128, both live waves hold real genes, the density column sits at
       wave 1, tile 0, lane group 1, register 2; one full spot block and one of 6 spots.  At the CM / NCB boundaries
       C in {4, 5, 16, 17, 28, 32} also regularised and constrained.
    B  gene-chunk edges at C = 18, V = 70: K in B_GENES (Kp = 128 .. 768: a density column alone in a new chunk, half-live last
       chunks, three full chunks), each with lambda_g2 0.5 and 0 (the VOX = false forward); K in {256, 384} also constrained.
    C  the density column's slot at C = 5, V = 70: p = 0 .. 63, K = p + 64 (p % 4) (256 for p = 0) puts column K into every (gene
       tile, lane group, register) and every wave; d_source for odd p.  lambda_d = C_LAMBDA_D.  Before the library is called the
       fp64 oracle has to show that in every row the gradient with lambda_d = 0 differs from the full one by at least a tenth of
       the row's largest |dM| (density_share): otherwise a wrong density column would sit inside the bound.
    D  spot-block edges at C = 18, K = 70: V in D_SPOTS; 16 384 is TG_ROWPASS_MAX_V, the last V on this path.
    E  the configurations of clusters mode at C in {13, 18, 26}, K = 250, V = 330: lambda_g2 = 0; d_source; no density (lambda_d = 0,
       d = None); lambda_g2 = 0 with d_source, what mode="clusters" really runs.  GPU table only: the tutorial's cross-validation
       shape C = 18, K = 250, V = 9 852 in that last configuration.
    F  batched twins (check_batch): three seeds in one tg_batch, bit-identical to each mapping trained alone.
    G  the path predicate (check_path_predicate): no training run.

The emulator table leaves the named cases of EMULATOR_LEAVES_OUT to the GPU table.

Largest values measured per sweep (grad: the row check; grad_quad: the last four columns; den: the worse of M's and the filter's;
hist: |delta| / max(1, |ref|)); bounds: grad, grad_quad, P, den 5e-5, hist 1e-5.  No case came within a factor 7 of a bound, the
float32 oracle was not needed on any:
                emulator                                            MI355X (the GPU table)
    sweep       grad      grad_quad  P         den       hist       grad      grad_quad  P         den       hist
    A           8.5e-7    6.3e-7     6.6e-7    6.5e-6    5.1e-7     7.6e-7    7.2e-7     7.2e-7    6.5e-6    5.1e-7
    B           7.3e-7    3.8e-7     5.7e-7    6.5e-6    6.3e-7     6.2e-7    3.9e-7     7.1e-7    6.5e-6    6.3e-7
    C           6.0e-7    6.7e-7     5.8e-7    6.3e-6    2.4e-7     6.0e-7    5.7e-7     6.6e-7    6.3e-6    2.8e-7
    D           5.6e-7    4.3e-7     5.6e-7    6.2e-6    1.6e-7     7.7e-7    4.6e-7     8.9e-7    6.3e-6    1.5e-7
    E           4.8e-7    5.4e-7     6.3e-7    6.2e-6    1.7e-7     5.8e-7    4.8e-7     9.7e-7    6.3e-6    2.5e-7
Sweep C at lambda_d = 1: the smallest share of the density term over the 64 cases and their rows is 0.45 (the largest 0.93), so
lambda_d was not raised.  F and G assert equality, they measure nothing.  The emulator runs its 166 tests in 45 s, the MI355X its
168 in 4 s (the longest, the first, 1 s).

Perturbations of a scratch copy of tg_small.h, run on the emulator (none committed, none run on a GPU); new: failures among the 166
tests of tests/test_clusters_kernels.py; old: failures in test_sim_parity, test_wide_genes, test_trained_state, test_batched,
test_update_row_lengths and test_sharded_gloo together:
    perturbation                                                      new tests that fail                                  old (of 187)
    (a) backward: ops.sx[gt][r][0] for every cb                          67: cases with C >= 17 (NCB = 2) in A, B, D, E           17 (sim_parity 8, trained_state 7, wide_genes 2)
    (b) colv takes register (rK + 1) & 3                                 161: every case with a density, the four batches         31 (sim_parity 15, trained_state 9, batched 4, ...)
    (c) vn mask `<= a.K`                                                 137: every case with lambda_g2 on                        23 (sim_parity 10, trained_state 8, batched 3, ...)
    (d) no coefficient reload at a new chunk                             17: the 16 cases of B with Kp >= 384, slot 0 of C        4 (sim_parity 2, wide_genes 2)
    (e) tg_prep_ssmall: augmentation column 1 with `aug` given           38: the 32 odd slots of C, the 6 d_source cases of E     6 (sim_parity 3, batched 2, sharded_gloo 1)
    (f) tg_sc_p_operands: spot tile st ^ 1 for j = CM / 4 - 1            160: every step case (the batches stay bit-equal)       33 (sim_parity 19, trained_state 8, batched 3, ...)
Each of the six is caught by the new tests, by exactly the cases built for it; each is also gross enough for some older test to see it
(d and e by four and six).
"""
import functools

import numpy as np

from tests import parity_common as pc

A_BOUNDARIES = (4, 5, 16, 17, 28, 32)
B_GENES = (1, 63, 64, 127, 128, 191, 255, 256, 257, 383, 384, 511, 512, 700)
B_CONSTRAINED = (256, 384)
D_SPOTS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4097, 16384)
E_CLUSTERS = (13, 18, 26)
E_CONFIGS = (dict(lambda_g2=0.0), dict(d_source=True), dict(density=False), dict(lambda_g2=0.0, d_source=True))
CROSS_VAL_SHAPE = (18, 250, 9852)
# lambda_d of sweep C: the value at which every case of the sweep meets the share condition on the fp64 oracle (density_share)
C_LAMBDA_D = 1.0
MIN_DENSITY_SHARE = 0.1
LR = 0.1


def cm_of(C):
    """tg_sc_cm: the compile-time cluster bound a problem of C clusters is dispatched to."""
    return (C + 3) // 4 * 4


def ncb_of(C):
    return (cm_of(C) + 15) // 16


def kp_of(K):
    """K genes and the augmentation column, padded to the 128-wide tile (tg_make_layout at tile 128)."""
    return -(-(K + 1) // 128) * 128


def density_slot(K):
    """(wave, gene tile, lane group, register) of column K in tg_sc_forward (dK = K - kw; gtK, grpK, rK)."""
    return ((K % 256) // 64, (K % 64) >> 4, (K & 15) >> 2, K & 3)


def slot_genes(p):
    return 256 if p == 0 else p + 64 * (p % 4)


def _case(sweep, C, K, V, variant="plain", lambda_g2=0.5, d_source=False, density=True, lambda_d=1.0, tag=""):
    cid = f"{sweep}{tag}-C{C}-K{K}-V{V}-{variant}" + ("-g2off" if lambda_g2 == 0 else "") + ("-dsource" if d_source else "") + \
        ("" if density else "-nodensity")
    return dict(id=cid, sweep=sweep, C=C, K=K, V=V, variant=variant, lambda_g2=lambda_g2, d_source=d_source, density=density,
                lambda_d=lambda_d if density else 0.0)


# ids of the step cases the emulator table leaves to the GPU table: handles of thousands of spots take it tens of seconds
EMULATOR_LEAVES_OUT = {"D-C18-K70-V4097-plain", "D-C18-K70-V16384-plain", "E-C18-K250-V9852-plain-g2off-dsource"}


def step_cases(gpu):
    out = []
    for C in range(1, 33):
        out.append(_case("A", C, 70, 70))
        if C in A_BOUNDARIES:
            out += [_case("A", C, 70, 70, "regularised"), _case("A", C, 70, 70, "constrained")]
    for K in B_GENES:
        out += [_case("B", 18, K, 70), _case("B", 18, K, 70, lambda_g2=0.0)]
        if K in B_CONSTRAINED:
            out.append(_case("B", 18, K, 70, "constrained"))
    for p in range(64):
        out.append(_case("C", 5, slot_genes(p), 70, d_source=bool(p % 2), lambda_d=C_LAMBDA_D, tag=f"-slot{p:02d}"))
    for V in D_SPOTS:
        out.append(_case("D", 18, 70, V))
    for C in E_CLUSTERS:
        for cfg in E_CONFIGS:
            out.append(_case("E", C, 250, 330, **cfg))
    C, K, V = CROSS_VAL_SHAPE
    out.append(_case("E", C, K, V, **E_CONFIGS[-1]))
    assert len({c["id"] for c in out}) == len(out)
    assert EMULATOR_LEAVES_OUT <= {c["id"] for c in out}
    if not gpu:
        out = [c for c in out if c["id"] not in EMULATOR_LEAVES_OUT]
    return out


BATCH_CASES = [(C, 300, 130, g2) for C in (13, 26) for g2 in (0.5, 0.0)]


@functools.lru_cache(maxsize=None)
def density_share(C, K, V, d_source, lambda_d):
    """The smallest share over the rows, on the fp64 oracle at the case's first step: max_v |dM - dM(lambda_d = 0)| / max_v |dM|."""
    seed = C + K + V
    data, lam, M0, F0 = pc.update_row_problem(C, K, V, "plain", seed, d_source=d_source, lambda_d=lambda_d)
    dM = pc.update_row_oracle(data, lam, M0, F0, "plain").loss_and_grad()[1]
    dM0 = pc.update_row_oracle(data, dict(lam, lambda_d=0.0), M0, F0, "plain").loss_and_grad()[1]
    return float((np.abs(dM - dM0).max(axis=1) / np.abs(dM).max(axis=1)).min())


def run_step_case(device, case):
    C, K, V = case["C"], case["K"], case["V"]
    if case["sweep"] == "C":                   # a condition on the inputs, evaluated on the checker before the library is called
        share = density_share(C, K, V, case["d_source"], case["lambda_d"])
        assert share >= MIN_DENSITY_SHARE, f"inputs: the density term moves a row of the oracle's gradient by only {share:.3f} of its largest |dM|"
    kw = {}
    if V == 1:
        # one spot: P = 1 and dM = P (dP - r) = 0 exactly, so "a fraction of the largest |dM|" is 0 both as Adam's eps (0 / 0 in the
        # oracle and the library alike) and as the scale of the gradient measure.  The measure of the saturated rows of
        # tests/trained_state_cases.py applies: the gradient against P (|dP| + |r|), which does not cancel, and torch's eps.
        kw = dict(start=dict(eps=1e-8), grad_scale="terms")
    out = pc.update_row_case(device, C, K, V, case["variant"], "bf16x3", n=3, seed=C + K + V, smallc=True, lambda_g2=case["lambda_g2"],
                             d_source=case["d_source"], density=case["density"], lambda_d=case["lambda_d"] if case["density"] else 1.0, **kw)
    print(case["id"], {k: v for k, v in out.items() if k != "kind"})
    return out


def check_case_tables(gpu_cases, emu_cases):
    """Every edge the sweeps exist for is in the table: a later edit cannot drop one."""
    def keys(cases, sweep):
        return {(c["C"], c["K"], c["V"], c["variant"], c["lambda_g2"], c["d_source"], c["density"]) for c in cases if c["sweep"] == sweep}
    for cases in (gpu_cases, emu_cases):
        a = keys(cases, "A")
        for C in range(1, 33):                                     # all 32 cluster counts, K = 70: the density column at (1, 0, 1, 2)
            assert (C, 70, 70, "plain", 0.5, False, True) in a, C
        assert density_slot(70) == (1, 0, 1, 2) and kp_of(70) == 128
        assert {cm_of(c[0]) for c in a} == set(range(4, 33, 4)) and {ncb_of(c[0]) for c in a} == {1, 2}      # every CM, both NCB
        for C in A_BOUNDARIES:
            assert (C, 70, 70, "regularised", 0.5, False, True) in a and (C, 70, 70, "constrained", 0.5, False, True) in a, C
        assert {cm_of(C) for C in A_BOUNDARIES} == {4, 8, 16, 20, 28, 32} and {cm_of(16), cm_of(17)} == {16, 20}
        b = keys(cases, "B")
        for K in B_GENES:
            for g2 in (0.5, 0.0):                                  # both VOX
                assert (18, K, 70, "plain", g2, False, True) in b, (K, g2)
        for K in B_CONSTRAINED:
            assert (18, K, 70, "constrained", 0.5, False, True) in b, K
        assert {kp_of(c[1]) for c in b} == set(range(128, 769, 128))                   # every Kp from 128 to 768
        assert kp_of(128) == 256 and kp_of(256) == 384 and kp_of(384) == 512 and kp_of(512) == 640    # the density column alone in its 128 columns
        assert {kp_of(K) // 128 % 2 for K in B_GENES} == {0, 1}                        # half-live last chunks and full ones
        c = [x for x in cases if x["sweep"] == "C"]
        assert all(x["C"] == 5 and x["V"] == 70 and x["lambda_d"] == C_LAMBDA_D and x["density"] for x in c)
        slots = {density_slot(x["K"]) for x in c}
        assert {w for w, _, _, _ in slots} == {0, 1, 2, 3}                             # all four waves
        assert {(g, r) for _, _, g, r in slots} == {(g, r) for g in range(4) for r in range(4)}
        assert any(x["d_source"] for x in c) and not all(x["d_source"] for x in c)
        d = keys(cases, "D")
        e = keys(cases, "E")
        for C in E_CLUSTERS:
            for g2, ds, dens in ((0.0, False, True), (0.5, True, True), (0.5, False, False), (0.0, True, True)):
                assert (C, 250, 330, "plain", g2, ds, dens) in e, (C, g2, ds, dens)
        assert {ncb_of(C) for C in E_CLUSTERS} == {1, 2} and {cm_of(C) for C in E_CLUSTERS} >= {16, 28}
        assert all(x["C"] <= pc.TG_SC_MAXC and x["V"] <= pc.ROWPASS_MAX_V for x in cases)
    gpu_c = [x for x in gpu_cases if x["sweep"] == "C"]
    assert {density_slot(x["K"])[1:] for x in gpu_c} == {(t, g, r) for t in range(4) for g in range(4) for r in range(4)}   # all 64 slots
    assert sorted(x["K"] for x in gpu_c) == sorted(slot_genes(p) for p in range(64))
    assert {v for _, _, v, *_ in keys(gpu_cases, "D")} == set(D_SPOTS) and max(D_SPOTS) == pc.ROWPASS_MAX_V
    assert {v for _, _, v, *_ in keys(emu_cases, "D")} >= set(D_SPOTS) - {4097, 16384}
    assert CROSS_VAL_SHAPE + ("plain", 0.0, True, True) in keys(gpu_cases, "E")
    ids = {x["id"] for x in gpu_cases}
    assert {x["id"] for x in emu_cases} <= ids and ids - {x["id"] for x in emu_cases} <= EMULATOR_LEAVES_OUT
    assert {(C, K, V) for C, K, V, _ in BATCH_CASES} == {(13, 300, 130), (26, 300, 130)} and {g2 for *_, g2 in BATCH_CASES} == {0.5, 0.0}


def check_batch(device, C, K, V, lambda_g2, epochs=5, seeds=(1, 2, 3)):
    """Three mappings of one clusters-mode problem from different seeds in ONE tg_batch (tg_sc_forward_b / tg_sc_backward_b; K = 300:
    Kp = 384, the chunk loop with a half-live last chunk) against each mapping trained alone: every history key, the logits and the
    mapping, bit for bit.  lambda_g2 = 0 runs with d_source, the clusters-mode configuration."""
    import ctypes as ct
    import tangram_amd as tg
    import tangram_amd.mapping_optimizer as mo
    from tests.test_batched import batches_taken
    data, lam, _, _ = pc.update_row_problem(C, K, V, "plain", C + K + V, lambda_g2=lambda_g2, d_source=lambda_g2 == 0)
    kw = dict(S=data["S"], G=data["G"], d=data["d"], d_source=data["d_source"], **lam)

    def builder(seed):
        return lambda: mo.Mapper(device=device, random_state=seed, gemm_precision="bf16x3", **kw)

    with batches_taken() as taken:
        res, mappers = tg.train_many([builder(s) for s in seeds], epochs, LR, device=device, batched=True)
    assert taken == [len(seeds)], taken
    logits = []
    for i, s in enumerate(seeds):
        e = mappers[i]._engine
        geo = (ct.c_int * 8)()
        assert e._lib.tg_debug_layout(ct.byref(e.cfg), geo) == 0 and geo[7] == 1, list(geo)
        assert e.effective_precision == "fp32"
        alone = builder(s)()
        P, hist = alone.train(num_epochs=epochs, learning_rate=LR, print_each=None)
        assert set(res[i][1]) == set(hist)
        for k in hist:
            np.testing.assert_array_equal(np.array(res[i][1][k], dtype=np.float64), np.array(hist[k], dtype=np.float64), err_msg=f"seed {s}: {k}")
        Mb, Ma = e.logits()[0].cpu().numpy()[:, :V], alone._engine.logits()[0].cpu().numpy()[:, :V]
        np.testing.assert_array_equal(Mb, Ma, err_msg=f"seed {s}: logits")
        np.testing.assert_array_equal(res[i][0], P, err_msg=f"seed {s}: mapping")
        assert np.isfinite(np.array(hist["total_loss"], dtype=np.float64)).all() and np.isfinite(P).all()
        assert np.isnan(np.array(hist["vg_reg"], dtype=np.float64)).all() == (lambda_g2 == 0)
        logits.append(Mb)
    assert not np.array_equal(logits[0], logits[1]) and not np.array_equal(logits[1], logits[2]), "the seeds gave one mapping"


def check_path_predicate(device):
    """tg_is_clusters_problem through tg_debug_layout (host only) and the effective precision of a handle that is created and not
    stepped, with bf16 asked for: the clusters path and exact fp32 at (C, V) = (32, 16 384), neither one cell or one spot further,
    nor with tile_size = 128, a spatial term or as a spot shard."""
    import ctypes as ct
    import scipy.sparse as sp
    from tangram_amd.engine import HipMapperEngine
    from oracle import tangram_oracle as orc
    K = 3

    def probe(C, V, **kw):
        data = orc.make_synthetic(C, K, V, seed=C + V)
        M0 = np.zeros((C, V), dtype=np.float32)
        e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], device=device, precision="bf16",
                            lambdas=dict(dict(lambda_g1=1.0, lambda_d=1.0), **kw.pop("lambdas", {})), **kw)
        geo = (ct.c_int * 8)()
        assert e._lib.tg_debug_layout(ct.byref(e.cfg), geo) == 0
        out = geo[7], e.effective_precision
        e.release()
        return out

    V = pc.ROWPASS_MAX_V
    assert probe(pc.TG_SC_MAXC, V) == (1, "fp32")
    assert probe(pc.TG_SC_MAXC + 1, V) == (0, "bf16")
    assert probe(pc.TG_SC_MAXC, V + 1) == (0, "bf16")
    # what else turns the path off does not depend on the shape: 70 spots (the emulator spends seconds on a handle of 16 384)
    V = 70
    assert probe(pc.TG_SC_MAXC, V) == (1, "fp32")
    assert probe(pc.TG_SC_MAXC, V, tile_size=128) == (0, "bf16")
    assert probe(pc.TG_SC_MAXC, V, n_ranks=1) == (0, "bf16")
    eye = sp.identity(V, dtype=np.float32, format="csr")
    assert probe(pc.TG_SC_MAXC, V, lambdas=dict(lambda_neighborhood_g1=0.5), voxel_weights=eye) == (0, "bf16")
    assert probe(pc.TG_SC_MAXC, V, lambdas=dict(lambda_moran=0.5), spatial_weights=eye) == (0, "bf16")
