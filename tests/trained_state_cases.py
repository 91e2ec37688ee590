"""The training step from the logits of a TRAINED mapping, on every kernel path: tables and checks shared by
tests/test_trained_state.py (emulator, device "cpu") and tests/test_gpu_trained_state.py (MI355X).

Every other step test starts from the reference's N(0, 1) draw, where a row spans 7 units and every exp argument is near 0.  A
trained mapping has rows that span 50 - 250 units, probabilities that are denormal or exactly 0 in float32, one spot with all the
mass, a saturated filter and a step counter in the hundreds.  The state families (functions of (C, V, seed) -> float32 logits):

    peaked40      N(0, 1) * 40 / 6 plus 40 at a home spot per cell: rows span ~110, every probability is a normal float32.  The
                  arithmetic of a peaked row without underflow: a wrong shift or a dropped rescale shows here and nothing else does.
    underflow90   the same with 90: rows span ~250, about a quarter of the probabilities are exactly 0 in float32 and more are
                  denormal.  0 * log 0, sums in which all terms but one vanish, partial (max, sum exp) pairs that underflow when merged.
                  90 is the cap: from 130 the oracle's own float32 run leaves a third of the bound on P.
    special rows  in both families (SPECIAL_ROWS): 0 a ramp from -B to B (+ 1/3: no logit is 0); 1 two equal maxima; 2 all logits equal (it also leaves
                  every spot a mass of 1 / (C V): rho > 0, the KL term is finite); 3 N(0, 1) plus 200 at one spot, the rest of the
                  row is exactly 0 in float32 (as in tests/topk_cases.py); 4 the home spot is the last valid column V - 1, in the
                  quad that straddles V.
    oracle300     the fp64 oracle's own (M, m, v, t) after 300 steps from N(0, 1), copied into the handle through logits() /
                  filter_state() / set_step: the bias corrections and moments at a large step count.  Once per process.
    filter        constrained mode (filter_logits): half of F0 at 0, the others at +-30, +-88, +-100 -- sigmoid(F) is exactly 0
                  or 1 in float32 at +-100 and denormal or 0 at -88, log(gate) in the forward's row constant is -inf.

The checker is parity_common.update_row_case with `start` and grad_scale="terms": the first-step gradient per row against
max_v P (|dP| + |r|) of the fp64 oracle (max|dM| cancels to 1e-12 of its terms on a saturated row: the old measure reads 1.0 for
the oracle's own float32 run from B = 40), history columns finite and within TOL, P relatively down to 2^-100 and below 2^-99
under it, exact zeros kept, rows of result() summing to 1, Adam's denominator, the filter, the padding, the kernel path, and the
conditioning guard (the oracle's float32 run within a third of each bound).

The gradient measure allows parity_common.grad_abs_floor absolutely: float32 has no relative precision below 2^-126 and the
hardware exponential flushes such probabilities.  No logit is exactly 0 (sign(0) in the L1 term is a knife edge).  Both were found
on MI355X: a ramp through 0 and two rows whose every gradient term is below 1e-34 failed there and not on the emulator.

Largest values measured over the tables, per precision of the bound that was applied (clusters-mode cases: the fp32 row); grad: the
worse of the row check and the last-four-columns check; den: the worse of M's and the filter's; hist: |delta| / max(1, |ref|);
guard: the fp64 oracle's own float32 run (a condition on the inputs, held to a third of the bound):
    emulator
    precision   grad / P / den bound   hist bound   grad      P         den       F         hist        guard grad  guard P   guard hist
    fp32        5e-5                   1e-5         3.4e-6    1.4e-5    6.5e-6    5.6e-8    4.8e-7      3.7e-6      1.4e-5    3.7e-7
    bf16x3      5e-5                   1e-5         7.4e-6    1.4e-5    9.8e-6    1.1e-7    1.0e-6      1.9e-6      1.3e-5    1.3e-6
    bf16        1e-2                   1e-3         3.6e-3    3.3e-4    1.8e-3    2.9e-5    4.0e-4      1.9e-6      1.3e-5    1.6e-7
    MI355X (measured on the GPU, the GPU table)
    fp32        5e-5                   1e-5         3.8e-6    1.6e-5    6.6e-6    5.6e-8    3.9e-7      (the guard runs on the host: the same
    bf16x3      5e-5                   1e-5         7.4e-6    1.6e-5    9.8e-6    1.1e-7    1.3e-6       values, over the two cases more of
    bf16        1e-2                   1e-3         3.6e-3    3.9e-4    4.5e-3    2.9e-5    4.0e-4       the GPU table)
The guard on P sits at 1.4e-5 of the 1.7e-5 it may reach: underflow90 is the sharpest state the bound on P admits.  With lambda_r on,
the oracle's float32 run is NaN from the first step (0 * log 0 on the row of exact zeros, as in the reference): the guard has nothing
finite to measure on the regularised and constrained cases, the library follows the fp64 oracle there.

Perturbations of a scratch copy, run on the emulator (none committed); new: failures among the 41 tests of
tests/test_trained_state.py, old: whether test_update_row_lengths / test_sim_parity / test_sharded_gloo / test_wide_genes fail too:
    perturbation                                                         new tests that fail                                   old
    (a) tg_row_stats_out: no `* tg_exp(tmax - wmax)` on the thread sums    37: every step case, gated cells, shards                 yes: 118 of 137 (all four files)
    (b) tg_merge_stats_body: no `* tg_exp(pm[p] - mx)`                     2: the spot shards, plain and constrained                yes: 13 (sharded_gloo 7, wide_genes 5, sim_parity 1)
    (c) tg_fwd_kernel: sh = 0 in the exponent                              32: the GEMM-path step cases, two products, gated cells, yes: 113 (all four files)
                                                                           shards, batch[cells]
    (d) tg_sc_forward: rmax = 0                                            9: the eight clusters-mode cases, batch[clusters]        yes: 21 (sim_parity 18, wide_genes 2, sharded_gloo 1)
    (e) rscale without `- tg_log(fgate)`                                   3: constrained bf16 (the path that reads rscale), both   yes: 6 (update_row_lengths 4, sim_parity 2)
                                                                           families and the 256 tile
Each of the five is caught by the new tests; each is also gross enough for the N(0, 1) suites to see it.
"""
import functools

import numpy as np

from tests import parity_common as pc

B_OF = {"peaked40": 40.0, "underflow90": 90.0}
SPECIAL_ROWS = dict(ramp=0, two_maxima=1, all_equal=2, plus200=3, home_last=4)
LR = 0.1


def family_logits(family, C, V, seed):
    """float32 logits [C, V] of a state family (module docstring)."""
    B = B_OF[family]
    assert C > len(SPECIAL_ROWS) and V >= 16
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((C, V)) * (B / 6.0)
    home = rng.integers(0, V, size=C)
    home[SPECIAL_ROWS["home_last"]] = V - 1
    M[np.arange(C), home] += B
    M[SPECIAL_ROWS["ramp"]] = np.linspace(-B, B, V) + 1.0 / 3.0
    r = SPECIAL_ROWS["two_maxima"]
    M[r] = rng.standard_normal(V) * (B / 6.0)
    M[r, [V // 3, (2 * V) // 3]] = np.float32(M[r].max() + B / 2.0)
    M[SPECIAL_ROWS["all_equal"]] = B / 4.0
    r = SPECIAL_ROWS["plus200"]
    M[r] = rng.standard_normal(V)
    M[r, V // 2 + 5] += 200.0
    M = M.astype(np.float32)
    # no logit is exactly 0: sign(0) = 0 in the L1 term is a knife edge -- the oracle's fp64 step moves such a logit by 1e-39 and its
    # L1 gradient is on from then, a float32 step (probability 1e-40, flushed) leaves it at 0 (a ramp through 0 did that on MI355X)
    assert (M != 0).all()
    return M


def filter_logits(C):
    """Constrained mode: half of the filter logits at 0 (the special rows among them: the all-equal row keeps its gate, so every
    spot keeps some gated mass), the others cycling through +-30, +-88, +-100."""
    F = np.zeros(C, dtype=np.float32)
    sat = np.array([30.0, -30.0, 88.0, -88.0, 100.0, -100.0], dtype=np.float32)
    idx = np.arange(len(SPECIAL_ROWS) + 1, C, 2)
    F[idx] = sat[np.arange(len(idx)) % len(sat)]
    return F


def family_start(family, C, V, seed, constrained):
    start = dict(M=family_logits(family, C, V, seed), zero_rows=(SPECIAL_ROWS["plus200"],))
    if constrained:
        start["F"] = filter_logits(C)
    return start


@functools.lru_cache(maxsize=None)
def oracle300(C, K, V, variant, seed, steps=300):
    """The fp64 oracle's state after `steps` steps of update_row_case's problem from its N(0, 1) draw, Adam's eps at
    ROW_EPS_FRACTION (the fp32 / bf16x3 one) of the largest first-step |dM|; rounded to float32, what a handle can hold."""
    data, lam, M0, F0 = pc.update_row_problem(C, K, V, variant, seed)
    o = pc.update_row_oracle(data, lam, M0, F0, variant)
    eps = float(np.float32(pc.ROW_EPS_FRACTION["bf16x3"] * np.abs(o.loss_and_grad()[1]).max()))
    for _ in range(steps):
        pc._oracle_adam_step(o, eps, LR)
    f32 = lambda x: np.asarray(x, dtype=np.float32)      # noqa: E731
    if variant == "constrained":
        return dict(M=f32(o.M), F=f32(o.F), m=f32(o.mM), v=f32(o.vM), mF=f32(o.mF), vF=f32(o.vF), t=o.t, eps=eps)
    return dict(M=f32(o.M), m=f32(o.m), v=f32(o.v), t=o.t, eps=eps)


def _case(path, C, K, V, variant, precision, family, tile=0, smallc=False):
    cid = f"{path}-C{C}-V{V}-{variant}-{precision}-{family}" + ("-t256" if tile else "")
    return dict(id=cid, path=path, C=C, K=K, V=V, variant=variant, precision=precision, family=family, tile=tile, smallc=smallc)


def step_cases(gpu):
    """The case table of the single-handle checker: one dict per case, `path` names the row of the path table it stands for.
    The emulator runs the same table except for the rows named in EMULATOR_LEAVES_OUT."""
    out = []
    for family in ("peaked40", "underflow90"):
        for precision in ("fp32", "bf16x3", "bf16"):
            for variant in ("plain", "regularised", "constrained"):
                out.append(_case("rowpass256", 65, 8, 1023, variant, precision, family))
    out.append(_case("tile256", 33, 8, 1024, "plain", "bf16x3", "underflow90", tile=256))
    out.append(_case("tile256", 33, 8, 1024, "constrained", "bf16", "underflow90", tile=256))
    out.append(_case("rowpass512", 33, 8, 4099, "plain", "bf16x3", "underflow90"))
    out.append(_case("rowpass512", 33, 8, 4099, "regularised", "fp32", "underflow90"))
    out.append(_case("two-kernel", 33, 8, 16385, "plain", "bf16x3", "underflow90"))
    out.append(_case("two-kernel", 33, 8, 16385, "constrained", "bf16", "underflow90"))
    for C, V in ((20, 300), (32, 65)):
        for variant in ("plain", "constrained"):
            for family in ("peaked40", "underflow90"):
                out.append(_case("clusters", C, 8, V, variant, "bf16x3", family, smallc=True))
    out.append(_case("oracle300", 65, 8, 257, "plain", "fp32", "oracle300"))
    out.append(_case("oracle300", 65, 8, 257, "plain", "bf16x3", "oracle300"))
    out.append(_case("oracle300", 65, 8, 257, "constrained", "bf16x3", "oracle300"))
    # read-outs at the stepped state (result_topk, project, project_genes of 300 genes -- 10 s on the emulator): from underflow90 on
    # the GEMM kernels in each precision and constrained, and on the clusters-mode kernels; the emulator keeps three of the six
    for c in out:
        key = (c["path"], c["C"], c["variant"], c["precision"])
        c["readouts"] = c["family"] == "underflow90" and key in (READOUTS if gpu else READOUTS_EMULATED)
    if not gpu:
        out = [c for c in out if (c["path"], c["precision"]) not in EMULATOR_LEAVES_OUT]
    return out


# (path, precision) the emulator table leaves to the GPU table: the emulator spends more than 20 s on a handle of 16 385 spots
EMULATOR_LEAVES_OUT = {("two-kernel", "bf16")}
READOUTS_EMULATED = {("rowpass256", 65, "plain", "bf16x3"), ("rowpass256", 65, "constrained", "bf16x3"), ("clusters", 20, "plain", "bf16x3")}
READOUTS = READOUTS_EMULATED | {("rowpass256", 65, "plain", "fp32"), ("rowpass256", 65, "plain", "bf16"), ("clusters", 20, "constrained", "bf16x3")}
SHARD_CASE = (65, 8, 300, 3)                # C, K, V, world
BATCH_CASES = {"cells": (40, 8, 300), "clusters": (20, 8, 300)}
TWO_PRODUCT_CASE = (65, 8, 1023)


def run_step_case(device, case):
    C, K, V, variant = case["C"], case["K"], case["V"], case["variant"]
    seed = C + V
    if case["family"] == "oracle300":
        start = oracle300(C, K, V, variant, seed)
    else:
        start = family_start(case["family"], C, V, seed + 7, variant == "constrained")
    out = pc.update_row_case(device, C, K, V, variant, case["precision"], tile=case["tile"], expect_tile=case["tile"] or 128, seed=seed,
                             start=start, grad_scale="terms", smallc=case["smallc"], readouts=case["readouts"])
    if not case["smallc"]:
        want = {"rowpass256": ("tg_adam_rowpass", 256), "tile256": ("tg_adam_rowpass", 256), "rowpass512": ("tg_adam_rowpass", 512),
                "two-kernel": ("tg_adam_update", 1024), "oracle300": ("tg_adam_rowpass", 256)}[case["path"]]
        assert (out["kind"][0], out["kind"][4]) == want, out["kind"]
    print(case["id"], {k: v for k, v in out.items() if k != "kind"})
    return out


def check_case_tables(gpu_cases, emu_cases):
    """Every row of the path table is in the GPU table; the emulator table holds at least the 256- and 512-thread rowpass, clusters
    mode and constrained mode (shards and batch are tests of their own in both modules)."""
    def rows(cases):
        return {(c["path"], c["C"], c["V"], c["variant"], c["precision"], c["family"]) for c in cases}
    gpu = rows(gpu_cases)
    for family in B_OF:
        for precision in ("fp32", "bf16x3", "bf16"):
            for variant in ("plain", "regularised", "constrained"):
                assert ("rowpass256", 65, 1023, variant, precision, family) in gpu
        for C, V in ((20, 300), (32, 65)):
            for variant in ("plain", "constrained"):
                assert ("clusters", C, V, variant, "bf16x3", family) in gpu
    assert {(p, C, V, v, pr) for p, C, V, v, pr, f in gpu if f == "underflow90"} >= {
        ("tile256", 33, 1024, "plain", "bf16x3"), ("tile256", 33, 1024, "constrained", "bf16"),
        ("rowpass512", 33, 4099, "plain", "bf16x3"), ("rowpass512", 33, 4099, "regularised", "fp32"),
        ("two-kernel", 33, 16385, "plain", "bf16x3"), ("two-kernel", 33, 16385, "constrained", "bf16")}
    assert {(v, pr) for p, C, V, v, pr, f in gpu if p == "oracle300" and (C, V) == (65, 257)} == {
        ("plain", "fp32"), ("plain", "bf16x3"), ("constrained", "bf16x3")}
    for table in (gpu_cases, emu_cases):
        kinds = {pc.update_instantiation(c["C"], c["V"], c["precision"], c["variant"])[:1] +
                 pc.update_instantiation(c["C"], c["V"], c["precision"], c["variant"])[4:5] for c in table if not c["smallc"]}
        assert {("tg_adam_rowpass", 256), ("tg_adam_rowpass", 512)} <= kinds, kinds
        assert any(c["smallc"] and c["C"] <= pc.TG_SC_MAXC for c in table) and any(c["variant"] == "constrained" for c in table)
        assert any(c["tile"] == 256 for c in table)
        assert all((c["C"] <= pc.TG_SC_MAXC) == c["smallc"] for c in table)
    assert ("tg_adam_update", 1024) in {pc.update_instantiation(c["C"], c["V"], c["precision"], c["variant"])[:1] +
                                        pc.update_instantiation(c["C"], c["V"], c["precision"], c["variant"])[4:5] for c in gpu_cases}
    assert rows(emu_cases) <= gpu


def check_two_products(device):
    """s_exact="auto" on a count-valued S (two matrix-core products per element) from underflow90: history, logits and both
    moments bit-equal to the general three-product path."""
    from tangram_amd.engine import HipMapperEngine
    C, K, V = TWO_PRODUCT_CASE
    data, lam, _, _ = pc.update_row_problem(C, K, V, "plain", C + V)
    M0 = family_logits("underflow90", C, V, C + V + 7)
    res = []
    for s_exact, want in ((False, "bf16x3"), ("auto", "bf16x3 (S exact: 2 products)")):
        e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], device=device, precision="bf16x3", lambdas=lam, s_exact=s_exact)
        assert e.effective_precision == want, e.effective_precision
        hist = e.new_history(3)
        e.step(3, LR, hist)
        res.append([hist.cpu().numpy().copy()] + [x.cpu().numpy().copy() for x in e.logits()[:3]])
        e.release()
    assert np.isfinite(res[0][0][:, 0]).all()
    for name, x, y in zip(("history", "M", "exp_avg", "exp_avg_sq"), res[0], res[1]):
        np.testing.assert_array_equal(x, y, err_msg=name)


def check_gated_out_cells(device, precision="bf16x3"):
    """Constrained mode from underflow90 with the saturated filter: a cell whose gate is exactly 0 contributes exactly nothing
    to the filtered projection -- project_genes(filtered) of S and of S with other numbers in those cells' rows are the same bits
    -- and project() holds no NaN and equals P^T (f S) of the fp64 oracle within TOL."""
    from tangram_amd.engine import HipMapperEngine
    from oracle import tangram_oracle as orc
    C, K, V = 65, 8, 1023
    data, lam, _, _ = pc.update_row_problem(C, K, V, "constrained", C + V)
    start = family_start("underflow90", C, V, C + V + 7, True)
    o = pc.update_row_oracle(data, lam, start["M"], start["F"], "constrained")
    e = HipMapperEngine(data["S"], data["G"], start["M"], d=data["d"], F0=start["F"], mode="constrained", target_count=0.4 * C,
                        device=device, precision=precision, lambdas=lam)
    hist = e.new_history(3)
    e.step(3, LR, hist)
    for _ in range(3):
        o.step(LR)
    gate = e.filter_values().cpu().numpy()
    out = gate == 0
    assert out.sum() >= (start["F"] == -100).sum() > 0 and np.isfinite(gate).all()
    assert (gate[start["F"] == 100] == 1).all()
    S2 = data["S"].copy()
    S2[out] = S2[out] * 3 + 5
    a = e.project_genes(data["S"], unfiltered=False).cpu().numpy()
    b = e.project_genes(S2, unfiltered=False).cpu().numpy()
    np.testing.assert_array_equal(a, b, err_msg="a cell with gate 0 contributes to the filtered projection")
    ref = orc.softmax_rows(o.M).T @ (o.S * (1.0 / (1.0 + np.exp(-o.F)))[:, None])
    for name, got in (("project()", e.project().cpu().numpy()), ("project_genes(filtered)", a)):
        assert np.isfinite(got).all(), name
        rel = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        assert rel <= pc.TOL[precision]["ghat"], f"{name}: relFro {rel:.3e}"
    assert np.isfinite(hist.cpu().numpy()[:, :1]).all() and np.isfinite(e.logits()[0].cpu().numpy()[:, :V]).all()
    e.release()


def check_shards(device, variant, precision="bf16x3", n=3):
    """Three spot shards (threads, tests/local_comm.py) from underflow90: two of three ranks hold none of most rows' mass, their
    (max, sum exp) pairs underflow in the merge.  The mapping and the history within the bounds of
    test_spot_shards_on_one_gpu_match_single_engine of the single engine, the history within TOL of the fp64 oracle and the same
    on every rank."""
    from tangram_amd.engine import HipMapperEngine
    from tangram_amd.sharded import make_sharded
    from tangram_amd import _capi
    from tests.local_comm import run_ranks
    C, K, V, world = SHARD_CASE
    data, lam, _, _ = pc.update_row_problem(C, K, V, variant, C + V)
    start = family_start("underflow90", C, V, C + V + 7, variant == "constrained")
    M0, F0 = start["M"], start.get("F")
    kw = dict(F0=F0, mode="constrained", target_count=0.4 * C) if variant == "constrained" else {}

    def rank_fn(comm):
        sh = make_sharded(data["S"], data["G"], M0, d=data["d"], device=device, precision=precision, lambdas=lam, comm=comm, **kw)
        hist = sh.eng.new_history(n)
        sh.run(n, LR, hist)
        out = hist.cpu().numpy(), sh.result_full().cpu().numpy()
        sh.release()
        return out

    res = run_ranks(world, rank_fn)
    e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], device=device, precision=precision, lambdas=lam, **kw)
    h1 = e.new_history(n)
    e.step(n, LR, h1)
    h1, P1 = h1.cpu().numpy(), e.result().cpu().numpy()
    e.release()
    o = pc.update_row_oracle(data, lam, M0, F0, variant)
    ho = [o.step(LR) for _ in range(n)]
    names = [(_capi.H_TOTAL, "total_loss"), (_capi.H_MAIN, "main_loss"), (_capi.H_VG, "vg_reg"), (_capi.H_KL, "kl_reg")]
    if variant == "constrained":
        names += [(_capi.H_ENTROPY, "entropy_reg"), (_capi.H_COUNT, "count_reg"), (_capi.H_FREG, "lambda_f_reg")]
    cols = [c for c, _ in names]
    for hist, P in res:
        np.testing.assert_array_equal(hist, res[0][0])
        np.testing.assert_allclose(hist[:, cols], h1[:, cols], atol=5e-6, rtol=2e-6)
        np.testing.assert_allclose(P, P1, atol=2e-6)
        for col, k in names:
            r = np.array([float(t[k]) for t in ho])
            assert np.isfinite(r).all() and np.isfinite(hist[:, col]).all(), (k, r, hist[:, col])
            err = float(np.abs(hist[:, col] - r).max())
            assert err <= pc.TOL[precision]["loss"] * max(1.0, float(np.abs(r).max())), f"{k}: max per-epoch |delta| {err:.3e}"
        np.testing.assert_allclose(P.sum(axis=1, dtype=np.float64), 1.0, atol=1e-6)


def check_batch(device, mode, precision="bf16x3", epochs=3):
    """Three mappings in one tg_batch -- two from underflow90 with different seeds, one from peaked40 -- bit-identical to each
    trained alone: every history key, the logits and the mapping.  mode "cells": 40 cells on the GEMM kernels; "clusters": 20
    cells on the clusters-mode kernels."""
    import tangram_amd as tg
    import tangram_amd.mapping_optimizer as mo
    from tests.test_batched import batches_taken
    C, K, V = BATCH_CASES[mode]
    data, lam, _, _ = pc.update_row_problem(C, K, V, "plain", C + V)
    kw = dict(S=data["S"], G=data["G"], d=data["d"], lambda_d=1, lambda_g1=1, lambda_g2=0.5)
    states = [family_logits("underflow90", C, V, 1), family_logits("underflow90", C, V, 2), family_logits("peaked40", C, V, 3)]

    def builder(M0):
        return lambda: mo.Mapper(device=device, M_init=M0, gemm_precision=precision, **kw)

    with batches_taken() as taken:
        res, mappers = tg.train_many([builder(M0) for M0 in states], epochs, LR, device=device, batched=True)
    assert taken == [3], taken
    for i, M0 in enumerate(states):
        alone = builder(M0)()
        P, hist = alone.train(num_epochs=epochs, learning_rate=LR, print_each=None)
        assert set(res[i][1]) == set(hist)
        for k in hist:
            np.testing.assert_array_equal(np.array(res[i][1][k], dtype=np.float64), np.array(hist[k], dtype=np.float64), err_msg=f"state {i}: {k}")
        Mb, Ma = mappers[i]._engine.logits()[0], alone._engine.logits()[0]
        np.testing.assert_array_equal(Mb.cpu().numpy()[:, :V], Ma.cpu().numpy()[:, :V], err_msg=f"state {i}: logits")
        np.testing.assert_array_equal(res[i][0], P, err_msg=f"state {i}: mapping")
        assert np.isfinite(np.array(hist["total_loss"], dtype=np.float64)).all() and np.isfinite(P).all()
        assert not np.array_equal(Ma.cpu().numpy()[:, :V], M0), "the step did not move the logits"
