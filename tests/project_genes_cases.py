"""Gene projection from the resident mapping (tg_mapper_project_genes) on every handle kind: tables and checks shared by
tests/test_project_genes.py (emulator, device "cpu") and tests/test_gpu_project_genes.py (MI355X).

Every workflow ends in this call -- project_genes(mapper=), score_genes, each fold of cross_val, the per-gene training scores,
ShardedMapperEngine.project_full -- and for a MapperConstrained handle all of them pass unfiltered=1, because adata_map.X is
softmax(M) without the filter.  That branch swaps two row constants of the forward GEMM (tg_fwd_args: rmul <- o_rinvz,
rlse2 <- o_rowent); the plain-bf16 operand path first runs a kernel of its own (tg_plain_rscale) that writes (max + ln Z) log2(e)
into the buffer tg_row_entropy otherwise owns.

Reference: the handle's OWN logits read back (logits(); constrained: filter_state()), then in NumPy float64
    unfiltered   softmax_rows(M).T @ S_all
    filtered     softmax_rows(M).T @ (sigmoid(F)[:, None] * S_all)
never result(), project() or another call of the code under test (check 8 alone takes the returned adata_map.X: it ties the
front end to the reference's definition adata_map.X.T @ adata_sc.X).

Bound, for every gene column g separately: ||got[:, g] - ref[:, g]||_2 <= TOL[row]["ghat"] * ||ref[:, g]||_2 with the project's
bounds of parity_common.TOL (1e-4 fp32, 1e-4 bf16x3, 1e-2 bf16).  The row is the precision the handle computes in
(effective_precision, asserted per case): a clusters-mode handle projects in fp32 whatever was asked for, a two-product handle
(bf16-exact S, s_exact="auto") projects a caller's block on the general bf16x3 kernels.  A whole-plane norm hides one wrong gene
column at a block seam (K = 8 cuts 300 genes into 38 blocks); a per-column one does not.  The columns are strictly positive
(gamma, or Poisson + 1), so no column norm is 0.

Checks (numbers as in the runners):
    1  kind x precision x filter: 128 tiles, tile_size = 256, clusters-mode kernels, the wide 128 x 512 forward geometry; fp32,
       bf16x3, bf16, two products; Mapper, MapperConstrained unfiltered and filtered; 3 steps at lr 0.1 from N(0, 1), 2K + 1 genes.
       The wide geometry exists for the split-bf16 forward only (tg_make_layout): that row holds bf16x3 and two products, at the
       shape tests/test_sim_parity.py pins geo[5] at (210 x 300 x 150, tile_size = 256: Kp = 512).
    2  gene-block edges: K in {1, 7, 8, 130} x n_genes in {1, K - 1, K, K + 1, 2K, 2K + 1, 3K - 1}.  An odd K starts every second
       block at S_dev + k0 with 4-byte alignment only.
    3  pitch and alignment: S_all at column offsets 0 - 3 of a wider tensor (pitch n + 5), through the C ABI with ld_out = n + 3 into
       a plane of sentinels that must survive beyond column n.
    4  cell-count edges C in {33, 63, 64, 65, 127, 128, 129}: tg_plain_rscale writes rows < C only; rows C .. Cp of o_rowent keep
       the 0 of the memset at creation or what tg_row_entropy left (lambda_r is on in these handles, so it has run), and a padding
       row of the bf16 softmax operand is then exp2(0 - 0) = 1, not the 0 that o_rscale's 3.0e38 gives.  And the same rows with the
       last cell's logits at +100 (check_padding_rows_large_logits), where that operand overflows.
    5  trained state: underflow90 with the saturated filter (gates of exactly 0 and 1; -ln f = +inf lives in o_rscale and must not
       reach the unfiltered call).  A cell whose gate is exactly 0 DOES contribute to the unfiltered output, by the fp64-predicted
       amount, and leaves the filtered output's bits alone.
    6  nothing of the handle moves: 2 steps, project unfiltered, project filtered, 2 steps == 4 steps, bit for bit (history, M, both
       moments, F and its moments); validate() around a projection; projection A, B, A.
    7  routes: scipy-CSR == dense in bits; spot shards (2, 3 ranks) against fp64 and project_full == the concatenation; a member of
       a tg_batch == the mapping trained alone.
    8  front end: tangram_amd.project_genes(adata_map, adata_sc, mapper=<constrained mapper>).

Largest per-column ratio ||got - ref|| / ||ref|| measured over all checks (both runners hold the same table), by the row of the
bound that was applied:
    row       bound    emulator    MI355X      where
    fp32      1e-4     1.8e-7      1.8e-7      K = 130, 260 genes, Mapper
    bf16x3    1e-4     3.6e-6      3.6e-6      the column with one cell (1e-3 in one cell of the last contraction step)
    bf16      1e-2     2.8e-3      2.8e-3      underflow90, filtered
On N(0, 1) states plain bf16 sits at 4e-4 - 1.3e-3.

What the checks found.  Check 4 as the issue states it passes: the padding rows C .. Cp of the unfiltered constant are multiplied
by the zero cells tg_prep_st puts into the S^T image.  That alone is not an invariant: the forward stages a padding row from the
LAST cell's logits and its own row constant, 0 here, so the plain-bf16 operand is exp2(M log2(e)) -- +inf once a logit of the last
cell passes 88.7, which Adam at lr 0.1 reaches within a thousand epochs, and inf * 0 is NaN in every gene of that spot.
check_padding_rows_large_logits (the last cell's logits at +100, C = 33, 65, 129) returned NaN on constrained unfiltered bf16 and
passed on bf16x3; tg_plain_rscale now fills rows C .. Cp with 3.0e38 as creation does for o_rscale, and the case passes.  The
underflow90 state of check 5 misses it by chance: its last cell's largest logit is below 88.7.

Perturbation of a scratch copy, run on the emulator (not committed): tg_fwd_args ignoring `unfiltered` for rlse2 only (rlse2 always
o_rscale).  21 of the then 100 tests fail, every one of them constrained unfiltered plain bf16 -- checks 1 (gemm128 and tile256; the
wide and clusters rows have no plain-bf16 forward), 2, 3, 4, the single-cell column, 5, 6, the spot shards and the front end; every
fp32, bf16x3, two-product, Mapper and filtered case passes.
"""
import ctypes as ct

import numpy as np

from tests import parity_common as pc
from tests import trained_state_cases as ts

LR = 0.1
LAM = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5)
LAM_C = dict(LAM, lambda_count=1.0, lambda_f_reg=1.0)
SENTINEL = -777.25
EFFECTIVE = {"fp32": "fp32", "bf16x3": "bf16x3", "bf16": "bf16", "two-product": "bf16x3 (S exact: 2 products)"}
FILTERS = ("mapper", "unfiltered", "filtered")          # Mapper; MapperConstrained with unfiltered=True / False

# largest per-column ratio seen in this process by bound row, and where
WORST = {}


def bound_row(effective_precision):
    """The row of TOL a handle is held to: what it computes in; a two-product handle projects on bf16x3."""
    return "bf16x3" if effective_precision.startswith("bf16x3") else effective_precision


def _np(t):
    return t.detach().cpu().numpy()


def sigmoid64(F):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(F, dtype=np.float64)))


def handle_logits(e):
    """(M [C, V], F [C] or None) of the handle as float64 copies of its own float32 state."""
    M = _np(e.logits()[0])[:, :e.V].astype(np.float64)
    F = _np(e.filter_state())[0, :e.C].astype(np.float64) if e.cfg.mode == 1 else None
    return M, F


def reference(M, F, S_all, unfiltered):
    from oracle import tangram_oracle as orc
    S = np.asarray(S_all, dtype=np.float64)
    if F is not None and not unfiltered:
        S = sigmoid64(F)[:, None] * S
    return orc.softmax_rows(M).T @ S


def check_columns(got, ref, row, label):
    """The per-column bound of the module docstring; returns the largest ratio."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{label}: NaN or Inf in the projection"
    den = np.linalg.norm(ref, axis=0)
    assert (den > 0).all(), f"{label}: a reference column is 0"
    ratio = np.linalg.norm(got - ref, axis=0) / den
    worst, g = float(ratio.max()), int(ratio.argmax())
    if worst > WORST.get(row, (0.0, ""))[0]:
        WORST[row] = (worst, label)
    print(f"PG-RATIO {row} {worst:.3e} column {g} of {ref.shape[1]}: {label}")
    bound = pc.TOL[row]["ghat"]
    assert worst <= bound, f"{label}: column {g} of {ref.shape[1]} is {worst:.3e} off (> {bound:.0e}, {row})"
    return worst


def gene_block(C, n, seed, kind="gamma"):
    """Strictly positive float32 [C, n]: gamma(1, 2) (not bf16-exact) or Poisson(0.7) + 1 (counts)."""
    rng = np.random.default_rng(seed)
    if kind == "gamma":
        S = rng.gamma(1.0, 2.0, size=(C, n)).astype(np.float32)
        return np.maximum(S, np.float32(1e-3))
    return (rng.poisson(0.7, size=(C, n)) + 1).astype(np.float32)


def make_handle(device, C, K, V, filt, precision, tile=0, seed=0, steps=3, lam=None, lambda_r=0.0, shift_last=0.0):
    """A handle after `steps` steps at lr 0.1 from the reference's N(0, 1) draw; S: negative-binomial counts (bf16-exact, what
    the two-product path needs).  shift_last (constrained): added to every logit of the last cell (softmax does not see it)."""
    from tangram_amd.engine import HipMapperEngine
    from oracle import tangram_oracle as orc
    data = orc.make_synthetic(C, K, V, seed=seed)
    prec, s_exact = ("bf16x3", "auto") if precision == "two-product" else (precision, False)
    if filt == "mapper":
        lam = dict(lam or LAM, lambda_r=lambda_r)
        e = HipMapperEngine(data["S"], data["G"], orc.reference_init_M(C, V, seed + 1), d=data["d"], device=device, precision=prec,
                            lambdas=lam, tile_size=tile, s_exact=s_exact)
    else:
        M0, F0 = orc.reference_init_MF_constrained(C, V, seed + 1)
        M0 = M0.copy()
        M0[C - 1] += np.float32(shift_last)
        lam = dict(lam or LAM_C, lambda_r=lambda_r)
        e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], F0=F0, mode="constrained", target_count=0.4 * C, device=device,
                            precision=prec, lambdas=lam, tile_size=tile, s_exact=s_exact)
    if steps:
        hist = e.new_history(steps)
        e.step(steps, LR, hist)
        assert np.isfinite(_np(hist)[:, 0]).all()
    return e


def layout(e):
    geo = (ct.c_int * 8)()
    assert e._lib.tg_debug_layout(ct.byref(e.cfg), geo) == 0
    return dict(tile=geo[0], wide=geo[5], smallc=geo[7])


def project_and_check(e, S_all, filt, label, row=None):
    """project_genes of S_all on handle e the way `filt` says, held per column to the fp64 reference from e's own logits."""
    M, F = handle_logits(e)
    unfiltered = filt != "filtered"
    got = _np(e.project_genes(S_all, unfiltered=unfiltered))
    check_columns(got, reference(M, F, S_all, unfiltered), row or bound_row(e.effective_precision), label)
    return got


# ---- 1. kind x precision x filter -------------------------------------------------------------------------------------------------
KIND_SHAPES = {"gemm128": (65, 8, 257, 0), "tile256": (65, 8, 257, 256), "clusters": (20, 8, 300, 0), "wide": (210, 300, 150, 256)}
KIND_PRECISIONS = {"gemm128": ("fp32", "bf16x3", "bf16", "two-product"), "tile256": ("fp32", "bf16x3", "bf16", "two-product"),
                   "clusters": ("fp32", "bf16x3", "bf16", "two-product"), "wide": ("bf16x3", "two-product")}


def kind_cases(gpu):
    """One table for both runners: the emulator needs about 4 s for a handle of the wide row, so it keeps it."""
    out = []
    for kind, (C, K, V, tile) in KIND_SHAPES.items():
        for precision in KIND_PRECISIONS[kind]:
            for filt in FILTERS:
                out.append(dict(id=f"{kind}-{precision}-{filt}", kind=kind, C=C, K=K, V=V, tile=tile, precision=precision, filt=filt))
    return out


def check_kind_tables(gpu_cases, emu_cases):
    ids = lambda cases: {c["id"] for c in cases}        # noqa: E731
    assert ids(emu_cases) <= ids(gpu_cases)
    for table in (gpu_cases, emu_cases):
        assert "gemm128-bf16-unfiltered" in ids(table), "constrained bf16 unfiltered: the path nothing else reaches"
        assert {c["kind"] for c in table} == set(KIND_SHAPES)
        for kind in ("gemm128", "tile256", "clusters"):
            assert {(c["precision"], c["filt"]) for c in table if c["kind"] == kind} == {
                (p, f) for p in ("fp32", "bf16x3", "bf16", "two-product") for f in FILTERS}
    assert {(c["precision"], c["filt"]) for c in gpu_cases if c["kind"] == "wide"} == {(p, f) for p in ("bf16x3", "two-product") for f in FILTERS}


def run_kind_case(device, case):
    C, K, V = case["C"], case["K"], case["V"]
    e = make_handle(device, C, K, V, case["filt"], case["precision"], tile=case["tile"], seed=C + V)
    geo = layout(e)
    if case["kind"] == "clusters":
        assert geo["smallc"] == 1, "20 cells must take the clusters-mode kernels"
        assert e.effective_precision == "fp32", e.effective_precision           # they project in fp32 whatever was asked for
    else:
        assert geo["smallc"] == 0 and geo["tile"] == (case["tile"] or 128), geo
        assert geo["wide"] == int(case["kind"] == "wide"), geo
        assert e.effective_precision == EFFECTIVE[case["precision"]], e.effective_precision
    n = 2 * K + 1
    project_and_check(e, gene_block(C, n, seed=n), case["filt"], case["id"])
    e.release()


# ---- 2. gene-block edges ----------------------------------------------------------------------------------------------------------
EDGE_KS = (1, 7, 8, 130)
EDGE_CONFIGS = (("unfiltered", "bf16x3"), ("unfiltered", "bf16"), ("mapper", "fp32"))
EDGE_C, EDGE_V = 65, 70


def edge_widths(K):
    return sorted({n for n in (1, K - 1, K, K + 1, 2 * K, 2 * K + 1, 3 * K - 1) if n >= 1})


def check_gene_block_edges(device, K, filt, precision):
    e = make_handle(device, EDGE_C, K, EDGE_V, filt, precision, seed=K, steps=2)
    assert e.effective_precision == precision
    for n in edge_widths(K):
        project_and_check(e, gene_block(EDGE_C, n, seed=1000 * K + n), filt, f"K={K} n_genes={n} {filt} {precision}")
    e.release()


# ---- 3. pitch and alignment -------------------------------------------------------------------------------------------------------
def check_pitch_and_alignment(device, K, precision):
    """Constrained, unfiltered.  S_all is columns off .. off + n of a [C, n + 5] tensor for off = 0 - 3: through project_genes (a
    view, pitch n + 5) and directly through the C ABI with ld_out = n + 3."""
    import torch
    C, V, n = 65, 70, 2 * K + 1
    e = make_handle(device, C, K, V, "unfiltered", precision, seed=K + 3, steps=2)
    M, F = handle_logits(e)
    wide = torch.as_tensor(gene_block(C, n + 5, seed=K), device=e.device)
    for off in range(4):
        view = wide[:, off:off + n]
        assert view.stride(0) == n + 5 and view.data_ptr() == wide.data_ptr() + 4 * off
        ref = reference(M, F, _np(view), True)
        label = f"K={K} {precision} offset {off}"
        a = _np(e.project_genes(view, unfiltered=True))
        check_columns(a, ref, precision, label + " (view)")
        out = torch.full((V, n + 3), SENTINEL, dtype=torch.float32, device=e.device)
        e._call(e._lib.tg_mapper_project_genes, e._h, view.data_ptr(), n + 5, n, out.data_ptr(), n + 3, 1, tensors=(wide, out))
        e._sync()
        out = _np(out)
        assert (out[:, n:] == np.float32(SENTINEL)).all(), f"{label}: the call wrote beyond column n of a row of pitch n + 3"
        np.testing.assert_array_equal(out[:, :n], a, err_msg=f"{label}: ld_out = n + 3 changes the values")
    e.release()


# ---- 4. cell-count edges ----------------------------------------------------------------------------------------------------------
CELL_COUNTS = (33, 63, 64, 65, 127, 128, 129)
CELL_CONFIGS = (("unfiltered", "bf16"), ("unfiltered", "bf16x3"), ("mapper", "bf16"))


def check_cell_count(device, C, filt, precision):
    """lambda_r on: tg_row_entropy has written o_rowent during the steps; the unfiltered call then overwrites rows < C of it."""
    K, V = 8, 65
    e = make_handle(device, C, K, V, filt, precision, seed=C, lambda_r=1e-3)
    assert e.effective_precision == precision and layout(e)["smallc"] == 0
    n = 2 * K + 1
    S_all = gene_block(C, n, seed=C + 1)
    a = project_and_check(e, S_all, filt, f"C={C} {filt} {precision}")
    if filt == "unfiltered":            # the filtered call in between leaves the unfiltered one its bits (and is right itself)
        project_and_check(e, S_all, "filtered", f"C={C} filtered {precision}")
        np.testing.assert_array_equal(_np(e.project_genes(S_all, unfiltered=True)), a)
    e.release()


LARGE_LOGIT_CELLS = (33, 65, 129)
LARGE_LOGIT_SHIFT = 100.0


def check_padding_rows_large_logits(device, C, precision):
    """Constrained, unfiltered, the last cell's logits near +100 (Adam at lr 0.1 gets there in a thousand epochs).  The forward
    stages the padding rows C .. Cp from the LAST cell's logits and their row constant: with the constant 0 the plain-bf16
    operand is exp2(100 log2(e) - 0) = +inf, and inf times the image's zero cell is NaN in every gene of that spot."""
    K, V = 8, 65
    e = make_handle(device, C, K, V, "unfiltered", precision, seed=C, shift_last=LARGE_LOGIT_SHIFT)
    M, _ = handle_logits(e)
    assert e.effective_precision == precision and M[C - 1].max() * np.log2(np.e) > 128 and C % 64 != 0
    S_all = gene_block(C, 2 * K + 1, seed=C + 2)
    for filt in ("unfiltered", "filtered", "unfiltered"):
        project_and_check(e, S_all, filt, f"last cell at +100, C={C} {filt} {precision}")
    e.release()


# ---- a column that is zero except in one cell -------------------------------------------------------------------------------------
def check_single_cell_column(device, precision):
    C, K, V = 65, 8, 70
    e = make_handle(device, C, K, V, "unfiltered", precision, seed=17)
    S_all = gene_block(C, 2 * K + 1, seed=3)
    S_all[:, 5] = 0
    S_all[C - 1, 5] = 2.5
    S_all[:, 8] = 0                     # the first column of the second block, one cell in the last contraction step
    S_all[C - 2, 8] = 1e-3
    for filt in ("unfiltered", "filtered"):
        got = project_and_check(e, S_all, filt, f"single-cell column {filt} {precision}")
        assert np.isfinite(got).all() and (got[:, [5, 8]] > 0).all()
    e.release()


# ---- 5. trained state -------------------------------------------------------------------------------------------------------------
def check_trained_state(device, precision):
    from tangram_amd.engine import HipMapperEngine
    C, K, V = 65, 8, 1023
    data, lam, _, _ = pc.update_row_problem(C, K, V, "constrained", C + V)
    start = ts.family_start("underflow90", C, V, C + V + 7, True)
    e = HipMapperEngine(data["S"], data["G"], start["M"], d=data["d"], F0=start["F"], mode="constrained", target_count=0.4 * C,
                        device=device, precision=precision, lambdas=lam)
    hist = e.new_history(3)
    e.step(3, LR, hist)
    assert np.isfinite(_np(hist)[:, :1]).all() and e.effective_precision == precision
    gate = _np(e.filter_values())
    out = gate == 0
    assert out.sum() >= (start["F"] == -100).sum() > 0 and (gate[start["F"] == 100] == 1).all() and np.isfinite(gate).all()
    M, F = handle_logits(e)
    n = 2 * K + 1
    S1 = gene_block(C, n, seed=5)
    S2 = S1.copy()
    S2[out] = S2[out] * 3 + 5
    u1 = project_and_check(e, S1, "unfiltered", f"underflow90 unfiltered {precision}")
    f1 = project_and_check(e, S1, "filtered", f"underflow90 filtered {precision}")
    u2 = project_and_check(e, S2, "unfiltered", f"underflow90 unfiltered, gated-out rows changed, {precision}")
    f2 = _np(e.project_genes(S2, unfiltered=False))
    np.testing.assert_array_equal(f1, f2, err_msg="a cell with gate 0 contributes to the filtered projection")
    # the gated-out cells DO contribute to the unfiltered output, by the fp64-predicted amount: each of u1, u2 is within
    # bound * ||ref|| of its reference (asserted above), so their difference is within bound * (||ref1|| + ||ref2||) of the
    # predicted one; the prediction itself must stand clear of that slack, or the assertion would say nothing
    r1, r2 = reference(M, F, S1, True), reference(M, F, S2, True)
    pred = r2 - r1
    slack = pc.TOL[precision]["ghat"] * (np.linalg.norm(r1, axis=0) + np.linalg.norm(r2, axis=0))
    assert (np.linalg.norm(pred, axis=0) >= 10 * slack).all(), "the changed rows do not move the reference enough to be seen"
    err = np.linalg.norm((u2.astype(np.float64) - u1.astype(np.float64)) - pred, axis=0)
    assert (err <= slack).all(), f"gated-out cells: the unfiltered output moved by other than the predicted amount ({(err / slack).max():.2f} of the slack)"
    for name, x in (("unfiltered", u1), ("filtered", f1), ("unfiltered 2", u2), ("filtered 2", f2)):
        assert np.isfinite(x).all(), name
    e.release()


# ---- 6. nothing of the handle moves -----------------------------------------------------------------------------------------------
def _state(e):
    M, m1, m2, step = e.logits()
    out = dict(M=_np(M)[:, :e.V].copy(), exp_avg=_np(m1)[:, :e.V].copy(), exp_avg_sq=_np(m2)[:, :e.V].copy(), step=np.array(step))
    if e.cfg.mode == 1:
        out["filter_state"] = _np(e.filter_state())[:, :e.C].copy()
    return out


def check_handle_untouched(device, precision, constrained):
    """update_row_problem's regularised / constrained variants: lambda_r is on, so the step reads o_rowent, the buffer the unfiltered
    call overwrites, and o_StP / o_Ghat / o_Gpart are rewritten by every projection."""
    from tangram_amd.engine import HipMapperEngine
    C, K, V = 65, 8, 257
    variant = "constrained" if constrained else "regularised"
    data, lam, M0, F0 = pc.update_row_problem(C, K, V, variant, C + V)
    kw = dict(F0=F0, mode="constrained", target_count=0.4 * C) if constrained else {}
    S_a, S_b = gene_block(C, 2 * K + 1, seed=1), gene_block(C, K - 1, seed=2, kind="counts")

    def handle():
        return HipMapperEngine(data["S"], data["G"], M0, d=data["d"], device=device, precision=precision, lambdas=lam, **kw)

    e, e4 = handle(), handle()
    h, h4 = e.new_history(4), e4.new_history(4)
    e4.step(4, LR, h4)
    e.step(2, LR, h)
    a1 = project_and_check(e, S_a, "unfiltered" if constrained else "mapper", f"untouched: A, {variant} {precision}")
    if constrained:
        fa = project_and_check(e, S_a, "filtered", f"untouched: A filtered, {variant} {precision}")
    else:
        v0 = e.validate()
        e.project_genes(S_a)
        v1 = e.validate()
        assert np.array_equal(np.array(v0, dtype=np.float32).view(np.int32), np.array(v1, dtype=np.float32).view(np.int32)), (v0, v1)
    project_and_check(e, S_b, "unfiltered" if constrained else "mapper", f"untouched: B, {variant} {precision}")
    np.testing.assert_array_equal(_np(e.project_genes(S_a, unfiltered=True)), a1, err_msg="projection A after B")
    if constrained:
        np.testing.assert_array_equal(_np(e.project_genes(S_a, unfiltered=False)), fa, err_msg="filtered projection A after B")
    e.step(2, LR, h, first_row=2)
    h, h4 = _np(h), _np(h4)
    assert np.isfinite(h4[:, 0]).all()
    np.testing.assert_array_equal(h.view(np.int32), h4.view(np.int32), err_msg="history: 2 steps, projections, 2 steps != 4 steps")
    s, s4 = _state(e), _state(e4)
    assert int(s["step"]) == 4
    for k in s4:
        np.testing.assert_array_equal(s[k], s4[k], err_msg=f"{k}: 2 steps, projections, 2 steps != 4 steps")
    e.release()
    e4.release()


# ---- 7. routes --------------------------------------------------------------------------------------------------------------------
def check_csr_route(device):
    """_project_genes_csr (blocks expanded on the device, one C-ABI call per block) == the dense route, bit for bit."""
    import scipy.sparse as sp
    C, K, V = 65, 8, 70
    e = make_handle(device, C, K, V, "unfiltered", "bf16x3", seed=23)
    for n in (K, K + 1, 2 * K + 1):
        dense = np.random.default_rng(n).poisson(0.7, size=(C, n)).astype(np.float32) * gene_block(C, n, seed=n)
        dense[0] = gene_block(1, n, seed=n + 1)                                 # no column is all zero
        assert (dense == 0).mean() > 0.3
        for unfiltered in (True, False):
            a = project_and_check(e, dense, "unfiltered" if unfiltered else "filtered", f"dense route n_genes={n}")
            b = _np(e.project_genes(sp.csr_matrix(dense), unfiltered=unfiltered))
            np.testing.assert_array_equal(a, b, err_msg=f"CSR route != dense route at n_genes = {n}, unfiltered = {unfiltered}")
    e.release()


def check_shards(device, world, precision):
    """Constrained spot shards as threads: each rank's project_genes against ITS rows of the fp64 reference (from the logits blocks
    of all ranks: the softmax runs over every spot), project_full == the concatenation of the ranks' blocks on every rank."""
    from oracle import tangram_oracle as orc
    from tangram_amd.sharded import make_sharded, shard_bounds
    from tests.local_comm import run_ranks
    C, K, V = 65, 8, 70
    data = orc.make_synthetic(C, K, V, seed=29)
    M0, F0 = orc.reference_init_MF_constrained(C, V, 30)
    S_all = gene_block(C, 2 * K + 1, seed=31)

    def rank_fn(comm):
        sh = make_sharded(data["S"], data["G"], M0, d=data["d"], F0=F0, mode="constrained", target_count=0.4 * C, device=device,
                          precision=precision, lambdas=LAM_C, comm=comm)
        hist = sh.eng.new_history(3)
        sh.run(3, LR, hist)
        mine = _np(sh.eng.project_genes(S_all, unfiltered=True)).copy()
        full = _np(sh.project_full(S_all, unfiltered=True)).copy()
        M, F = handle_logits(sh.eng)
        assert sh.eng.effective_precision == precision
        sh.release()
        return mine, full, M, F

    res = run_ranks(world, rank_fn)
    M = np.concatenate([r[2] for r in res], axis=1)
    assert M.shape == (C, V)
    ref = reference(M, res[0][3], S_all, True)
    cat = np.concatenate([r[0] for r in res], axis=0)
    for rank, (mine, full, _, F) in enumerate(res):
        lo, hi = shard_bounds(V, world, rank, False)
        np.testing.assert_array_equal(F, res[0][3])
        check_columns(mine, ref[lo:hi], precision, f"rank {rank} of {world}, {precision}")
        np.testing.assert_array_equal(full, cat, err_msg=f"rank {rank}: project_full != the ranks' blocks in order")


def check_batch_member(device, precision="bf16x3"):
    """Three MapperConstrained of clusters-mode size in one tg_batch: project_genes_device(S_test, unfiltered=True) of every member
    equals in bits the same mapping trained alone (and the fp64 reference from the member's logits)."""
    import tangram_amd as tg
    import tangram_amd.mapping_optimizer as mo
    from oracle import tangram_oracle as orc
    from tests.test_batched import batches_taken
    C, K, V, B = 20, 8, 300, 3
    data = orc.make_synthetic(C, K, V, seed=37)
    kw = dict(S=data["S"], G=data["G"], d=data["d"], lambda_d=1, lambda_g1=1, lambda_g2=0.5, lambda_count=1, lambda_f_reg=1, target_count=0.4 * C)
    inits = [orc.reference_init_MF_constrained(C, V, 40 + i) for i in range(B)]
    S_test = gene_block(C, 2 * K + 1, seed=41)

    def builder(i):
        return lambda: mo.MapperConstrained(device=device, M_init=inits[i][0], F_init=inits[i][1], gemm_precision=precision, **kw)

    with batches_taken() as taken:
        _, mappers = tg.train_many([builder(i) for i in range(B)], 3, LR, device=device, batched=True)
    assert taken == [B], taken
    for i in range(B):
        assert layout(mappers[i]._engine)["smallc"] == 1
        got = _np(mappers[i].project_genes_device(S_test, unfiltered=True))
        M, F = handle_logits(mappers[i]._engine)
        check_columns(got, reference(M, F, S_test, True), "fp32", f"batch member {i}")
        alone = builder(i)()
        alone.train(num_epochs=3, learning_rate=LR, print_each=None)
        np.testing.assert_array_equal(got, _np(alone.project_genes_device(S_test, unfiltered=True)), err_msg=f"member {i} != trained alone")
        assert not np.array_equal(M.astype(np.float32), inits[i][0]), "the batch did not train"
        alone.release()
    for m in mappers:
        m.release()


# ---- 8. front end -----------------------------------------------------------------------------------------------------------------
def check_front_end(device, precision):
    """tangram_amd.project_genes(adata_map, adata_sc, mapper=<constrained mapper>) == adata_map.X.T @ adata_sc.X in float64, per
    column: unfiltered=True is the reference's definition (adata_map.X is softmax(M) without the filter)."""
    import pandas as pd
    import tangram_amd as tg
    from tangram_amd.anndata_lite import AnnDataLite
    from oracle import tangram_oracle as orc
    C, K, V, extra = 65, 8, 70, 9
    data = orc.make_synthetic(C, K + extra, V, seed=43)
    genes = [f"g{i}" for i in range(K + extra)]
    S = data["S"] + 1.0                                                          # strictly positive columns
    G = data["G"]
    obs_sp = pd.DataFrame({"rna_count_based_density": G.sum(1) / G.sum(), "uniform_density": np.ones(V) / V}, index=[f"s{i}" for i in range(V)])
    ad_sc = AnnDataLite(S.astype(np.float32), obs=pd.DataFrame(index=[f"c{i}" for i in range(C)]), var=pd.DataFrame(index=genes))
    ad_sp = AnnDataLite(G, obs=obs_sp, var=pd.DataFrame(index=genes))
    for ad in (ad_sc, ad_sp):
        ad.uns["training_genes"] = genes[:K]
        ad.uns["overlap_genes"] = genes
    ad_map = tg.map_cells_to_space(ad_sc, ad_sp, mode="constrained", target_count=0.4 * C, device=device, num_epochs=3, random_state=7,
                                   verbose=False, gemm_precision=precision, keep_mapper=True)
    mapper = ad_map._tangram_amd_mapper
    assert isinstance(mapper, tg.mapping_optimizer.MapperConstrained) and bound_row(mapper._engine.effective_precision) == precision
    filt = np.asarray(ad_map.obs["F_out"], dtype=np.float64)
    assert filt.min() < 0.9, "a filter of ones would not tell unfiltered from filtered"
    ad_ge = tg.project_genes(ad_map, ad_sc, device=device, gemm_precision=precision, mapper=mapper)
    cols = [genes.index(g) for g in ad_ge.var.index]
    assert len(cols) == K + extra and ad_ge.X.shape == (V, K + extra)
    want = np.asarray(ad_map.X, dtype=np.float64).T @ np.asarray(ad_sc.X, dtype=np.float64)[:, cols]
    check_columns(np.asarray(ad_ge.X), want, precision, f"front end, constrained mapper, {precision}")
    mapper.release()
