"""Shared helpers of the parity tests (CPU-emulated and GPU).  The checker is the oracle / the golden
fixtures generated from the unmodified reference; the thing under test is always the C-ABI library."""
import os

import numpy as np

from oracle.gen_golden import CASES, build_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Stated fp32 tolerances (calibrated on the reference's own fp32-vs-fp64 / thread-count spread)
TOL = {
    #           per-epoch |d loss|   max|dP|   relFro(P^T S)
    "fp32":   dict(loss=1e-5, P=2e-4, ghat=1e-4),
    "bf16x3": dict(loss=1e-5, P=2e-4, ghat=1e-4),
    # bf16, max|dP| on the SMALL cases (tens to hundreds of spots: single probabilities of 0.1 - 1): calibrated in round 6 by running the 29
    # plain-bf16 cases of the GPU suite under shrinking bounds (scripts/gpu_r06f.sh, profiles/r06/run4_bf16_tolerance_scan): 28 pass at
    # 2e-2, 26 at 1e-2, 18 at 1e-3; the largest measured value is 3.5e-2 (golden constrained_entropy, 500 epochs), then 1.33e-2 (live
    # reference, spatial terms) and 1.26e-2 (golden cells_autocorr): the bound is 1.4 x the largest measurement, not a formality.  (At
    # full size the meaningful bound is relative: FULL_BOUNDS in tests/test_gpu_live_reference.py.)
    "bf16":   dict(loss=1e-3, P=float(os.environ.get("TG_TOL_BF16_P", 5e-2)), ghat=1e-2),      # (environment: the scan that calibrated the bound)
}


# The 500-epoch cases of the reference's own test grid are ill-conditioned: the reference's fp32 run drifts from its fp64 run (flat
# valley).  Beyond the well-conditioned prefix an implementation is held to this multiple of that drift, term by term and at the end
# point.  ONE bound for both kernel families (the clusters-mode kernels these 12-cluster cases run on by default, and the GEMM
# kernels pinned by `tile_size`), because the multiple an fp32 run ends at is amplified round-off of the transcendentals, not a
# property of a kernel family -- measured (scripts/exp_rounding_drift.py -> profiles/r04/exp_rounding/drift.json): the SAME kernel
# sources on the CPU emulator, with exp2 / exp / log rounded four different 1-ulp-accurate ways (host libm; towards zero; away from
# zero; hash-picked neighbour -- the last three also with the hardware's fp32 product x * log2(e) inside exp), end the seven cases at
#     largest multiple     libm    towards 0    away    hashed        MI355X (v_exp_f32 / v_log_f32)
#     clusters kernels     1.44      2.49       2.12     1.60          3.0   (round 3, profiles/r03)
#     GEMM kernels         2.22      1.72       2.74     2.00          2.2
# i.e. anywhere in 1.4 - 2.7 for either family from a 1-ulp change of three scalar functions; the hardware's 3.0 was one more draw
# from that distribution (round 4 therefore carried 4 = 1.5 x the largest emulated draw).
# Round 5 records what a GPU session measures (MEASURED_SPREAD below -> gpurun_out/own_spread_measured.json; committed copy:
# profiles/r05/final/own_spread_measured.json): with this round's kernels the largest multiples on MI355X are 1.47 (clusters-mode
# kernels, fp32 and bf16x3), 1.80 / 1.37 (GEMM kernels, bf16x3 / fp32) and 2.31 (GEMM kernels, plain bf16, against its own 100 x
# wider tolerance).  The kernels are bit-reproducible (no atomics), so these are properties of the build, not of a box: the bound
# goes back to 3 = 1.3 x the largest measured multiple (the round-4 advisor's request), one constant for both families.
OWN_SPREAD = 3.0
# every (case, term) whose whole-run check was decided by the drift bound leaves its measured multiple here; tests/conftest.py writes the
# list to gpurun_out/own_spread_measured.json at the end of a GPU session (round-4 advisor: record the multiples a round measures)
MEASURED_SPREAD = []


# The validation metrics of the golden case cells_val (check_against_golden): multiple of TOL[precision]["loss"] they are held to.
# Measured on the emulator (bf16x3, 7 epochs): 1.4e-7, i.e. 1 x would hold there; the 20-epoch GPU runs of the case in fp32, bf16x3 and
# plain bf16 (tests/test_gpu_parity.py) have not been measured since the figures are printed, so the factor stays where it was.  The
# 1 x bound is what tests/test_validation_metrics.py and tests/test_gpu_validation_metrics.py hold every path to, after 0, 1 and 3 steps.
VAL_GOLDEN_FACTOR = 10.0


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def run_case(name, device, precision, epochs=None, pin_gemm=False):
    """Train the tangram_amd Mapper on golden case `name`; returns (P, history dict, Ghat, golden npz, epochs).
    pin_gemm: the engine is built with tile_size = 128, which keeps a problem of at most 32 cells on the GEMM kernels."""
    import functools
    import tangram_amd.mapping_optimizer as mo
    if pin_gemm:
        orig = mo.HipMapperEngine
        mo.HipMapperEngine = functools.partial(orig, tile_size=128)
        try:
            out = run_case(name, device, precision, epochs)
            out["pin_gemm"] = True
            return out
        finally:
            mo.HipMapperEngine = orig
    z = load_golden(name)
    args, n_epochs, mode = build_inputs(name)
    val_each = args.pop("val_each", None)
    if epochs is not None:
        n_epochs = min(n_epochs, epochs)
    if mode == "constrained":
        m = mo.MapperConstrained(device=device, gemm_precision=precision, M_init=z["f32_M0"], F_init=z["f32_F0"], **args)
        P, F, hist = m.train(num_epochs=n_epochs, learning_rate=0.1, print_each=None)
    else:
        m = mo.Mapper(device=device, gemm_precision=precision, M_init=z["f32_M0"], **args)
        P, hist = m.train(num_epochs=n_epochs, learning_rate=0.1, print_each=None, val_each=val_each)
        F = None
    Ghat = m.project_genes_device().detach().cpu().numpy()
    return dict(P=P, F=F, hist=hist, Ghat=Ghat, z=z, epochs=n_epochs, mode=mode, name=name)


def check_against_golden(res, precision, full_length, own_spread=None):
    """Compare with the reference's fp64 run (ground truth) within the stated fp32 tolerance."""
    OWN_SPREAD = own_spread if own_spread is not None else globals()["OWN_SPREAD"]
    tol = TOL[precision]
    z, n = res["z"], res["epochs"]
    keys = ["main_loss", "total_loss", "kl_reg", "vg_reg", "entropy_reg"]
    if res["mode"] == "constrained":
        keys += ["count_reg", "lambda_f_reg"]
    # (the spatial terms enter total_loss; the reference keeps no separate history for them, :378-392)
    for k in keys:
        ref = z["f64_hist_" + k][:n]
        got = np.array([float(x) for x in res["hist"][k]], dtype=np.float64)
        if np.isnan(ref).all():
            assert np.isnan(got).all(), f"{k}: expected NaN history like the reference"
            continue
        scale = max(1.0, float(np.abs(ref).max()))
        if res["mode"] == "constrained" and k == "total_loss":
            scale *= 20.0        # the reference stores str(tensor) here: 4 printed decimals (mapping_optimizer.py:630)
        # The 500-epoch grid cases (the reference's own test grid) leave the well-conditioned regime after ~170 epochs: the
        # REFERENCE's fp32 run then drifts up to 1.3e-4 from its fp64 run in main_loss / kl_reg (flat valley) while total_loss
        # stays within 6e-6 (tests/test_oracle_golden.py).  Each term is held to the flat tolerance for as long as the
        # reference's own fp32 arithmetic stays within a third of it; total_loss additionally over the whole run, bounded
        # by the flat tolerance or 5x the reference's own fp32-vs-fp64 spread on the case.
        own = np.abs(z["f32_hist_" + k][:n] - ref) if ("f32_hist_" + k) in z.files else np.zeros(n)
        if res["mode"] == "constrained" and k == "total_loss":
            own = np.zeros(n)
        over = np.nonzero(own > tol["loss"] * scale / 3.0)[0]
        well = int(over[0]) if len(over) else n
        if res["mode"] == "grid":
            well = min(well, 100 if precision != "bf16" else 50)   # round-off grows ~10x per 50 epochs on these cases; any two fp32
                                                                  # implementations part ways by ~150 (bf16 operands: earlier)
        assert well >= min(n, 50), f"{k}: fixture ill-conditioned from epoch {well}"
        err = float(np.abs(got[:well] - ref[:well]).max())
        assert err <= tol["loss"] * scale, f"{k}: max per-epoch |delta| {err:.3e} > {tol['loss'] * scale:.1e}"
        if well < n:
            # ... and over the WHOLE run EVERY term stays within OWN_SPREAD x the reference's own fp32-vs-fp64 drift on the case
            # (measured: 1.0 - 2.2 x; round 2 held only total_loss, to 5 x)
            spread = float(np.abs(z["f32_hist_" + k][:n] - ref).max())
            bound = max(tol["loss"] * scale, OWN_SPREAD * spread * (tol["loss"] / 1e-5))
            err = float(np.abs(got - ref).max())
            if spread > 0 and OWN_SPREAD * spread * (tol["loss"] / 1e-5) > tol["loss"] * scale:      # the drift bound is the binding one: keep the multiple
                MEASURED_SPREAD.append(dict(case=res.get("name"), mode=res["mode"], precision=precision, pinned_gemm=bool(res.get("pin_gemm")),
                                            term=k, multiple=err / (spread * (tol["loss"] / 1e-5)), bound=OWN_SPREAD))
            assert err <= bound, f"{k} (full run): max per-epoch |delta| {err:.3e} > {bound:.1e} (the reference's own fp32 drift: {spread:.1e})"
    if full_length:
        dP = float(np.abs(res["P"] - z["f64_P"]).max())
        boundP = tol["P"]
        if res["mode"] == "grid":       # end point of an ill-conditioned 500-epoch run: relative to the reference's own fp32 spread
            boundP = max(tol["P"], OWN_SPREAD * float(np.abs(z["f32_P"] - z["f64_P"]).max()) * (tol["P"] / 2e-4))
        assert dP <= boundP, f"max|dP| {dP:.3e} > {boundP:.1e}"
        rel = float(np.linalg.norm(res["Ghat"] - z["f64_Ghat"]) / np.linalg.norm(z["f64_Ghat"]))
        bound_g = tol["ghat"]
        if res["mode"] == "grid":
            bound_g = max(bound_g, OWN_SPREAD * float(np.linalg.norm(z["f32_Ghat"] - z["f64_Ghat"]) / np.linalg.norm(z["f64_Ghat"])) * (tol["ghat"] / 1e-4))
        assert rel <= bound_g, f"relFro(P^T S) {rel:.3e} > {bound_g:.1e}"
        if res["F"] is not None:
            dF = float(np.abs(res["F"] - z["f64_F_out"]).max())
            assert dF <= tol["P"], f"max|dF| {dF:.3e}"
        am = (res["P"].argmax(1) == z["f64_P"].argmax(1)).mean()
        # (grid cases: 12 cluster rows whose largest entries are ~0.04 and nearly tied; one flipped row is 8 %)
        need = (0.9 if precision != "bf16" else 0.75) if res["mode"] == "grid" else (0.98 if precision != "bf16" else 0.9)
        assert am >= need, f"argmax agreement {am:.3f}"
    if "f64_hist_val_gene_sim" in z.files:       # Mapper._val_loss_fn metrics (mapping_optimizer.py:311-356)
        for k in ("val_total_loss", "val_gene_sim", "val_sp_sparsity_weighted_sim", "val_entropy"):
            got = np.array(res["hist"][k], dtype=np.float64)
            ref = z["f64_hist_" + k][:len(got)]
            assert len(got) > 0
            err = float(np.abs(got - ref).max())
            print(f"golden {res.get('name')} {precision} {k}: max |delta| over {len(got)} validations {err:.2e}")
            assert err <= VAL_GOLDEN_FACTOR * tol["loss"], (k, got, ref)
    np.testing.assert_allclose(res["P"].sum(axis=1), 1.0, atol=1e-5)
    assert (res["P"] >= 0).all()


def small_cluster_case(device, C, K, V, constrained, lambda_g2, seed, precision="bf16x3", n=3, tile_size=0):
    """One clusters-mode-sized problem (C <= 32: the library runs tg_sc_forward / tg_sc_backward instead of the GEMM kernels,
    asserted through tg_debug_layout) for n epochs against the fp64 oracle.  Tolerances: the fp32 row of TOL whatever `precision`
    says (that path computes in fp32 FMAs).  tile_size != 0 pins the GEMM path on the same problem."""
    import ctypes as ct
    from tangram_amd.engine import HipMapperEngine
    from tangram_amd import _capi
    from oracle import tangram_oracle as orc
    rng = np.random.default_rng(seed)
    data = orc.make_synthetic(C, K, V, seed=seed)
    lam = dict(lambda_g1=1.0, lambda_d=float(rng.choice([0.0, 1.0])), lambda_g2=lambda_g2, lambda_r=float(rng.choice([0.0, 1e-3])))
    d = data["d"] if lam["lambda_d"] > 0 or constrained else None
    if constrained:
        lam["lambda_d"] = lam["lambda_d"] or 1.0
        lam.update(lambda_count=1.0, lambda_f_reg=1.0)
        tc = max(1.0, 0.5 * C)
        M0, F0 = orc.reference_init_MF_constrained(C, V, seed)
        o = orc.OracleMapperConstrained(data["S"], data["G"], d, M0=M0, F0=F0, target_count=tc, dtype=np.float64, **lam)
        Po, Fo, ho = o.train(n, 0.1)
        e = HipMapperEngine(data["S"], data["G"], M0, d=d, F0=F0, mode="constrained", device=device, precision=precision, lambdas=lam,
                            target_count=tc, tile_size=tile_size)
    else:
        lam.update(lambda_l1=float(rng.choice([0.0, 1e-4])), lambda_l2=float(rng.choice([0.0, 1e-5])))
        ds = rng.dirichlet(np.ones(C)).astype(np.float32) if (d is not None and rng.integers(2)) else None
        M0 = orc.reference_init_M(C, V, seed)
        o = orc.OracleMapper(data["S"], data["G"], d=d, d_source=ds, M0=M0, dtype=np.float64, **lam)
        Po, ho = o.train(n, 0.1)
        e = HipMapperEngine(data["S"], data["G"], M0, d=d, d_source=ds, device=device, precision=precision, lambdas=lam, tile_size=tile_size)
    geo = (ct.c_int * 8)()
    assert e._lib.tg_debug_layout(ct.byref(e.cfg), geo) == 0
    assert geo[7] == int(tile_size == 0), "the small-C path is taken exactly when no tile size is pinned"
    hist = e.new_history(n)
    e.step(n, 0.1, hist)
    h = hist.cpu().numpy().astype(np.float64)
    tol = TOL["fp32"] if tile_size == 0 else TOL[precision]
    cols = [(_capi.H_TOTAL, "total_loss"), (_capi.H_MAIN, "main_loss")]
    if lam["lambda_g2"] > 0:
        cols.append((_capi.H_VG, "vg_reg"))
    if lam["lambda_d"] > 0:
        cols.append((_capi.H_KL, "kl_reg"))
    if lam["lambda_r"] > 0:
        cols.append((_capi.H_ENTROPY, "entropy_reg"))
    for col, k in cols:
        ref = np.array([float(x) for x in ho[k]])
        err = np.abs(h[:, col] - ref).max()
        assert err <= 3 * tol["loss"] * max(1.0, np.abs(ref).max()), (C, K, V, constrained, k, err)
    if constrained:
        P, F = e.result(with_filter=True)
        assert np.abs(F.cpu().numpy() - Fo).max() <= 2e-5
    else:
        P = e.result()
    assert np.abs(P.cpu().numpy() - Po).max() <= tol["P"], (C, K, V)
    return e


# ---- the update kernels at every row length on the GEMM path (tests/test_update_row_lengths.py on the emulator,
# tests/test_gpu_update_row_lengths.py on the GPU) ------------------------------------------------------------------------------
# Bounds of update_row_case, calibrated on the emulator and on MI355X (largest measured values: the two test modules' docstrings).
#   grad: per row, max|g - dM| / max|dM_row| of the first-step gradient (bf16: the 2-norm, ROW_GRAD_NORM); and the last four
#         columns of every row against the largest |dM| of those columns
#   P:    element-wise max|P - Po| / Po after n epochs
#   den:  element-wise relative error of Adam's denominator sqrt(v) / sqrt(1 - beta2^t) + eps after n epochs (the second moment as
#         the update uses it: an element whose gradient crosses zero has no relative precision in v itself)
#   F:    constrained mode, the filter logits, |F - Fo| / max(1, |Fo|), and the filter's denominator like `den`
ROW_TOL = {
    "fp32":   dict(grad=5e-5, P=5e-5, den=5e-5),
    "bf16x3": dict(grad=5e-5, P=5e-5, den=5e-5),
    "bf16":   dict(grad=1e-2, P=1e-2, den=1e-2),
}
# Norm of the per-row gradient check.  Plain bf16 rounds S, dGhat and X to 8 mantissa bits: where a row's largest P meets a dP close
# to r_c, single elements are off by more than 1e-2 (1.4e-2 measured, bit-identical on the emulator and MI355X, at the row's
# largest |dM|), so bf16 rows are held in the 2-norm -- the norm of the existing bf16 gradient bound (relative Frobenius 1e-2,
# tests/test_gpu_production_tiles.py), taken per row
ROW_GRAD_NORM = {"fp32": np.inf, "bf16x3": np.inf, "bf16": 2}
# Adam's eps of these runs as a fraction of the largest first-step |dM| (see update_row_case); plain bf16 takes a larger one, because
# its gradient carries ~1e-2 of round-off and the denominator of an element whose gradient is near zero is eps
ROW_EPS_FRACTION = {"fp32": 0.05, "bf16x3": 0.05, "bf16": 0.2}


def update_instantiation(C, V, precision, variant):
    """The update kernel a single-GPU, more-than-32-cell handle launches (tg_launch_update in tg_capi.hip: tg_with_update_flags
    x tg_with_row_length):
    (kernel, FULL, X16, NQ, NT, STREAM); NQ is None for tg_adam_update."""
    full, x16 = variant != "plain", precision == "bf16"
    if V > 16384:                                       # backward with the row-dot epilogue, tg_rowsum_parts, tg_adam_update
        return ("tg_adam_update", full, x16, None, 1024 if C <= 64 else 256, True)
    if V > 4096:
        nq = (V + 2047) // 2048
        return ("tg_adam_rowpass", full, x16, nq if nq <= 6 else 8, 512, True)
    nq = (V + 1023) // 1024
    vp = -(-V // 64) * 64
    stream = C * vp * (12 + (2 if x16 else 4)) > (192 << 20)      # tg_mapper::stream_once
    return ("tg_adam_rowpass", full, x16, 1 if nq <= 1 else (2 if nq <= 2 else 4), 256, stream)


def _oracle_adam_step(o, eps, lr):
    """OracleMapper(.Constrained).step with Adam's eps set (the oracle's own step uses torch's default 1e-8)."""
    from oracle import tangram_oracle as orc
    res = o.loss_and_grad()
    o.t += 1
    if len(res) == 3:
        terms, dM, dF = res
        orc.adam_update(o.M, dM, o.mM, o.vM, o.t, lr, eps=eps)
        orc.adam_update(o.F, dF, o.mF, o.vF, o.t, lr, eps=eps)
    else:
        terms, dM = res
        orc.adam_update(o.M, dM, o.m, o.v, o.t, lr, eps=eps)
    return terms, dM


def row_rel_err(got, ref, order=np.inf):
    """Per row: |got - ref| / |ref_row| in the max norm (order=inf) or the 2-norm (order=2)."""
    scale = np.linalg.norm(ref, ord=order, axis=1)
    return np.linalg.norm(got - ref, ord=order, axis=1) / np.where(scale > 0, scale, 1.0)


# A trained state (tests/trained_state_cases.py): probabilities are compared relatively down to this floor, 2^-100 (a float32
# normal number with 26 binades to spare); below it the library's value has to be below twice the floor
P_FLOOR = 2.0 ** -100
# ... and float32 has no relative precision below its smallest normal number, 2^-126: a gradient read from Adam's first moment
# (1 - beta1) g is that coarse, and a probability below it may be flushed to 0 (v_exp_f32 does), which moves r_c = sum_v P dP by up to
# V 2^-126 max|dP| and with it every g_cv = P (dP - r_c) of the row.  A row whose every term is that small -- a cell without counts
# whose only spot with mass has density 0: dP = 0 at the peak, scale 3e-85 or 1e-34 in the fp64 oracle -- is held to this absolutely
FLT_MIN_NORMAL = 2.0 ** -126


def grad_abs_floor(o):
    """[C, 1] absolute allowance of the scaled gradient measure (above), from the oracle's last loss_and_grad."""
    V = o.last["dP"].shape[1]
    return FLT_MIN_NORMAL * (1.0 / (1.0 - 0.9) + V * np.abs(o.last["dP"]).max(axis=1, keepdims=True))


def grad_scale_terms(o):
    """|P| (|dP| + |r|) [C, V] of the oracle's last loss_and_grad: the size of the terms of dM = P (dP - r) before they cancel."""
    L = o.last
    return L["P"] * (np.abs(L["dP"]) + np.abs(L["r"])[:, None])


def trained_P_errors(P, Po):
    """(largest relative error over the elements with Po >= P_FLOOR, largest P over the others)"""
    hi = Po >= P_FLOOR
    rel = np.abs(P - Po)[hi] / Po[hi]
    return float(rel.max()), float(P[~hi].max()) if (~hi).any() else 0.0


def _as_f32_like(x, like):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=like.device)


def _load_oracle_state(o, start):
    """A checkpoint (m, v, t[, mF, vF]) into an oracle built on its logits; the library holds float32, so does the oracle's start."""
    if "m" not in start:
        return
    f = lambda x: np.asarray(x, dtype=np.float32).astype(o.dt)      # noqa: E731
    if hasattr(o, "mF"):
        o.mM, o.vM, o.mF, o.vF = f(start["m"]), f(start["v"]), f(start["mF"]), f(start["vF"])
    else:
        o.m, o.v = f(start["m"]), f(start["v"])
    o.t = int(start["t"])


def update_row_problem(C, K, V, variant, seed, lambda_g2=0.5, d_source=False, density=True, lambda_d=1.0):
    """(data, lambdas, M0, F0) of update_row_case: make_synthetic(seed), the reference's initial draw of seed + 1, and for the
    variants but "plain" each regulariser at a fraction of the typical |dM| of the plain problem at that draw.
    lambda_g2 = 0 turns the per-spot cosine term off; d_source: data["d_source"] is a strictly positive [C] float32 vector that sums
    to 1, drawn from `seed` (Mapper only: the constrained mapper takes none); density off: lambda_d = 0 and data["d"] is None."""
    from oracle import tangram_oracle as orc
    data = dict(orc.make_synthetic(C, K, V, seed=seed), d_source=None)
    lam = dict(lambda_g1=1.0, lambda_d=float(lambda_d), lambda_g2=lambda_g2)
    if not density:
        assert not d_source, "d_source requires d"
        lam["lambda_d"], data["d"] = 0.0, None
    if d_source:
        assert variant != "constrained", "the constrained mapper takes no d_source"
        w = np.random.default_rng(seed).uniform(0.5, 1.5, size=C)
        data["d_source"] = (w / w.sum()).astype(np.float32)
    if variant == "constrained":
        M0, F0 = orc.reference_init_MF_constrained(C, V, seed + 1)
    else:
        M0, F0 = orc.reference_init_M(C, V, seed + 1), None
    if variant != "plain":
        _, g0 = orc.OracleMapper(data["S"], data["G"], d=data["d"], d_source=data["d_source"], M0=M0, dtype=np.float64, **lam).loss_and_grad()
        P0 = orc.softmax_rows(M0.astype(np.float64))
        logP = np.log(P0)
        ent = np.median(np.abs(P0 * (logP - (P0 * logP).sum(axis=1, keepdims=True))))
        gmed = float(np.median(np.abs(g0)))
        lam["lambda_r"] = float(np.float32(0.3 * gmed / ent))
        if variant == "regularised":
            lam["lambda_l1"] = float(np.float32(0.2 * gmed))
            lam["lambda_l2"] = float(np.float32(0.1 * gmed))
    if variant == "constrained":
        lam.update(lambda_count=1.0, lambda_f_reg=1.0)
    return data, lam, M0, F0


def update_row_oracle(data, lam, M0, F0, variant, dtype=np.float64):
    """The oracle of update_row_case at the logits M0 (and filter logits F0): target count 0.4 C in constrained mode."""
    from oracle import tangram_oracle as orc
    if variant == "constrained":
        return orc.OracleMapperConstrained(data["S"], data["G"], data["d"], M0=M0, F0=F0, target_count=0.4 * M0.shape[0], dtype=dtype, **lam)
    return orc.OracleMapper(data["S"], data["G"], d=data["d"], d_source=data.get("d_source"), M0=M0, dtype=dtype, **lam)


def _conditioning_guard(o64, data, lam, variant, M0, F0, start, eps, lr, n, dM, sc, floor, hist_o, cols, tol, ltol):
    """The oracle in float32 on the same case, measured like the library, against a third of each bound -- on the elements and
    columns where the float32 run is finite (lambda_r with an underflowed probability is 0 * log 0 = NaN there, as in the
    reference).  A condition on the inputs, evaluated on the checker alone."""
    from oracle import tangram_oracle as orc
    o = update_row_oracle(data, lam, M0, F0, variant, dtype=np.float32)
    _load_oracle_state(o, start)
    hist = []
    with np.errstate(all="ignore"):
        for i in range(n):
            terms, g = _oracle_adam_step(o, np.float32(eps), lr)
            hist.append(terms)
            if i == 0:
                g32 = g.astype(np.float64)
        P32 = orc.softmax_rows(o.M).astype(np.float64)
    guard = {}
    err = np.where(np.isfinite(g32), np.maximum(np.abs(g32 - dM) - floor, 0.0), 0.0).max(axis=1) / sc.max(axis=1)
    guard["grad"] = float(err.max())
    Po = orc.softmax_rows(o64.M)
    okP = np.isfinite(P32) & (Po >= P_FLOOR)
    guard["P"] = float((np.abs(P32 - Po)[okP] / Po[okP]).max()) if okP.any() else 0.0
    guard["hist"] = 0.0
    for _, k in cols:
        ref = np.array([float(x) for x in hist_o[k]])
        got = np.array([float(t[k]) for t in hist], dtype=np.float64)
        fin = np.isfinite(got)
        if fin.any():
            guard["hist"] = max(guard["hist"], float(np.abs(got - ref)[fin].max() / max(1.0, float(np.abs(ref).max()))))
    assert guard["grad"] <= tol["grad"] / 3, f"inputs: the oracle's float32 gradient is {guard['grad']:.2e} off (> {tol['grad'] / 3:.1e})"
    assert guard["P"] <= tol["P"] / 3, f"inputs: the oracle's float32 mapping is {guard['P']:.2e} off (> {tol['P'] / 3:.1e})"
    assert guard["hist"] <= ltol / 3, f"inputs: the oracle's float32 history is {guard['hist']:.2e} off (> {ltol / 3:.1e})"
    return guard


def _readouts_at_state(e, o, data, variant, P32, precision, seed):
    """The read-outs of a handle at its stepped state against fp64 from the oracle's logits: result_topk(8) bit-equal to result(),
    project() and project_genes of 300 genes within relFro TOL[precision]["ghat"]."""
    from oracle import tangram_oracle as orc
    from tests.topk_cases import assert_topk_equals_dense
    assert_topk_equals_dense(e.result_topk(8), P32, 8, "top-k at the stepped state")
    Po = orc.softmax_rows(o.M)
    S = data["S"].astype(np.float64)
    ref = Po.T @ (S * (1.0 / (1.0 + np.exp(-o.F)))[:, None]) if variant == "constrained" else Po.T @ S
    got = e.project().cpu().numpy().astype(np.float64)
    bound = TOL[precision]["ghat"]
    rel = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    assert np.isfinite(got).all() and rel <= bound, f"project(): relFro {rel:.3e} > {bound:.0e}"
    S_all = (np.random.default_rng(seed).poisson(0.7, size=(e.C, 300))).astype(np.float32)
    got = e.project_genes(S_all).cpu().numpy().astype(np.float64)
    ref = Po.T @ S_all.astype(np.float64)
    rel = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    assert np.isfinite(got).all() and rel <= bound, f"project_genes of 300 genes: relFro {rel:.3e} > {bound:.0e}"


def update_row_case(device, C, K, V, variant, precision, tile=0, expect_tile=128, n=3, seed=0, start=None, grad_scale=None,
                    smallc=False, readouts=False, lambda_g2=0.5, d_source=False, density=True, lambda_d=1.0):
    """One problem of C > 32 cells on the GEMM path against the fp64 oracle, n epochs; returns the measured errors.

    variant: "plain" (FULL off), "regularised" (lambda_r, lambda_l1, lambda_l2 on) or "constrained" (filter gate + lambda_r).
    The regularisers are scaled to the plain gradient of the problem so that each term moves dM visibly without drowning the
    rest.  Adam's eps is ROW_EPS_FRACTION[precision] of the largest first-step |dM|: with torch's 1e-8 the first step is lr * sign(g)
    wherever |g| >> 1e-8, and the few elements whose gradient crosses zero within the round-off of the GEMM precision then
    decide an element-wise comparison of P (measured: 5e-4 relative in bf16x3, 0.2 in bf16 at eps 1e-8).  The kernel's
    arithmetic is the same for any eps.

    start: the state the run begins from instead of the reference's N(0, 1) draw (tests/trained_state_cases.py) -- a dict with
    "M" [C, V] float32, "F" [C] for constrained, and for a checkpoint "m", "v", "t" (and "mF", "vF"), copied into the handle
    through logits() / filter_state() / set_step; "eps" overrides Adam's eps.  The regularisers keep the scale they have from the
    N(0, 1) draw of the same seed.  With a start the case asserts more (the trained-state list of _trained_checks) and the
    conditioning guard: the oracle's own float32 run stays within a third of every bound.
    grad_scale="terms": the first-step gradient is held per row against max_v P_cv (|dP_cv| + |r_c|) of the fp64 oracle, which
    does not cancel on a saturated row, instead of max_v |dM_cv|; every precision in the max norm.
    smallc: a problem of at most 32 cells on the clusters-mode kernels (tg_sc_forward / tg_sc_backward; bounds: the fp32 row).
    readouts: result_topk(8), project() and project_genes of 300 genes at the stepped state against fp64.
    lambda_g2, d_source, density, lambda_d: update_row_problem; a term that is turned off (vg_reg at lambda_g2 = 0, kl_reg without a
    density) is NaN in the history, as in the reference, and its column is not compared."""
    import ctypes as ct
    from tangram_amd.engine import HipMapperEngine
    from tangram_amd import _capi
    from oracle import tangram_oracle as orc
    lr = 0.1
    kind = None if smallc else update_instantiation(C, V, precision, variant)
    start = dict(start or {})
    data, lam, M0, F0 = update_row_problem(C, K, V, variant, seed, lambda_g2=lambda_g2, d_source=d_source, density=density, lambda_d=lambda_d)
    if "M" in start:
        M0, F0 = start["M"], start.get("F")
    o = update_row_oracle(data, lam, M0, F0, variant)
    kw = dict(F0=F0, mode="constrained", target_count=0.4 * C) if variant == "constrained" else {}
    _load_oracle_state(o, start)
    terms0, dM = o.loss_and_grad()[:2]
    eps = float(start.get("eps") or np.float32(ROW_EPS_FRACTION[precision] * np.abs(dM).max()))
    if start:                             # the inputs: every term the case compares is finite in the fp64 oracle before the library is called
        on = [k for k in terms0 if not (k == "entropy_reg" and "lambda_r" not in lam)]
        assert all(np.isfinite(float(terms0[k])) for k in on) and np.isfinite(dM).all(), f"inputs: fp64 terms {terms0}"
    e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], d_source=data["d_source"], device=device, precision=precision, lambdas=lam,
                        tile_size=tile, eps=eps, **kw)
    tol = ROW_TOL["fp32" if smallc else precision]
    ltol = TOL["fp32" if smallc else precision]["loss"]
    out = dict(kind=kind, eps=eps)
    # ---- schedule: the GEMM path (not the clusters-mode kernels), the tile, one cell band
    geo = (ct.c_int * 8)()
    assert e._lib.tg_debug_layout(ct.byref(e.cfg), geo) == 0
    assert (geo[7], geo[0], geo[6]) == (int(smallc), expect_tile, 1), f"smallc / tile / bands = {geo[7]}, {geo[0]}, {geo[6]}"
    M, m1, m2, _ = e.logits()
    pitch = M.shape[1]
    if "m" in start:                      # a checkpoint: moments and step counter into the fresh handle (the logits came with create)
        m1[:, :V].copy_(_as_f32_like(start["m"], m1))
        m2[:, :V].copy_(_as_f32_like(start["v"], m2))
        if variant == "constrained":
            fs = e.filter_state()
            fs[1, :C].copy_(_as_f32_like(start["mF"], fs))
            fs[2, :C].copy_(_as_f32_like(start["vF"], fs))
        e.set_step(int(start["t"]))
        assert e.logits()[3] == int(start["t"]) == o.t
    m1_before = m1[:, :V].cpu().numpy().astype(np.float64)
    pad0 = [x[:, V:].cpu().numpy().copy() for x in (M, m1, m2)]
    if variant == "constrained":
        fs = e.filter_state()
        fpad0 = fs[:, C:].cpu().numpy().copy()
    hist = e.new_history(n)
    e.profile(True)
    e.step(1, lr, hist, 0)
    names = [k for k, _, _ in e.profile_read()]
    e.profile(False)
    if smallc:
        assert "tg_sc_forward" in names and "tg_sc_backward" in names and "tg_fwd_kernel" not in names, names
    elif kind[0] == "tg_adam_rowpass":
        assert "tg_fwd_kernel" in names and "tg_sc_forward" not in names, names
        assert "tg_adam_rowpass" in names and "tg_adam_update" not in names and "tg_rowsum_parts" not in names, names
    else:
        assert "tg_rowsum_parts" in names and "tg_adam_update" in names and "tg_adam_rowpass" not in names, names
    # ---- first-step gradient from Adam's first moment: exp_avg = (1 - beta1) * g after one step
    terms, dM1 = _oracle_adam_step(o, eps, lr)
    assert np.array_equal(dM1, dM)
    hist_o = {k: [terms.get(k, np.nan)] for k in terms}
    q0 = max(0, V - 4)
    if "m" in start:                      # exp_avg = beta1 * exp_avg + (1 - beta1) * g
        g = (m1[:, :V].cpu().numpy().astype(np.float64) - 0.9 * m1_before) / 0.1
    else:
        g = m1[:, :V].cpu().numpy().astype(np.float64) / (1.0 - 0.9)
    if grad_scale == "terms":
        sc, floor = grad_scale_terms(o), grad_abs_floor(o)
        dg = np.maximum(np.abs(g - dM) - floor, 0.0)
        err_row = dg.max(axis=1) / sc.max(axis=1)
        err_quad = dg[:, q0:].max(axis=1) / sc[:, q0:].max()
    else:
        assert grad_scale is None, grad_scale
        sc, floor = np.abs(dM), 0.0
        err_row = row_rel_err(g, dM, ROW_GRAD_NORM[precision])
        # the last four columns of every row on their own (the quad that straddles V when V % 4 != 0), against their own largest |dM|
        err_quad = np.abs(g[:, q0:] - dM[:, q0:]).max(axis=1) / np.abs(dM[:, q0:]).max()
    out["grad"] = float(err_row.max())
    out["grad_quad"] = float(err_quad.max())
    assert out["grad"] <= tol["grad"], f"first-step gradient: row {int(err_row.argmax())}, {out['grad']:.3e} > {tol['grad']:.0e}"
    assert out["grad_quad"] <= tol["grad"], \
        f"first-step gradient, last four columns: row {int(err_quad.argmax())}, {out['grad_quad']:.3e} > {tol['grad']:.0e}"
    # ---- n epochs
    for _ in range(n - 1):
        terms, _ = _oracle_adam_step(o, eps, lr)
        for k in hist_o:
            hist_o[k].append(terms.get(k, np.nan))
    e.step(n - 1, lr, hist, 1)
    h = hist.cpu().numpy().astype(np.float64)
    cols = [(_capi.H_TOTAL, "total_loss"), (_capi.H_MAIN, "main_loss")]
    if lam["lambda_g2"] != 0:
        cols.append((_capi.H_VG, "vg_reg"))
    if data["d"] is not None:
        cols.append((_capi.H_KL, "kl_reg"))
    if "lambda_r" in lam:
        cols.append((_capi.H_ENTROPY, "entropy_reg"))
    if variant == "constrained":
        cols += [(_capi.H_COUNT, "count_reg"), (_capi.H_FREG, "lambda_f_reg")]
    for col, k in cols:
        ref = np.array([float(x) for x in hist_o[k]])
        if start:
            assert np.isfinite(ref).all(), f"inputs: {k} of the fp64 oracle {ref}"
            assert np.isfinite(h[:, col]).all(), f"{k}: {h[:, col]} where the fp64 oracle has {ref}"
        err = float(np.abs(h[:, col] - ref).max())
        out["hist"] = max(out.get("hist", 0.0), err / max(1.0, float(np.abs(ref).max())))
        assert err <= ltol * max(1.0, float(np.abs(ref).max())), f"{k}: max per-epoch |delta| {err:.3e}"
    if variant == "constrained":
        P, Fg = e.result(with_filter=True)
    else:
        P = e.result()
    P32 = P.cpu().numpy()
    P = P32.astype(np.float64)
    Po = orc.softmax_rows(o.M)
    if start:
        out["P"], out["P_low"] = trained_P_errors(P, Po)
        assert np.isfinite(P).all()
        assert out["P_low"] <= P_FLOOR * 2, f"an element below the floor holds {out['P_low']:.3e}"
        assert float(np.abs(P32.sum(axis=1, dtype=np.float64) - 1.0).max()) <= 1e-6, "rows of result() do not sum to 1"
        for c in start.get("zero_rows", ()):
            assert (np.delete(P32[c], int(np.argmax(start["M"][c]))) == 0).all() and P32[c].max() == 1.0, f"row {c}: exact zeros expected off the peak"
    else:
        out["P"] = float((np.abs(P - Po) / Po).max())
    assert out["P"] <= tol["P"], f"max|P - Po| / Po = {out['P']:.3e} > {tol['P']:.0e}"
    bc2 = np.sqrt(1.0 - 0.999 ** o.t)

    def den_err(v, vo):
        den, deno = np.sqrt(v) / bc2 + eps, np.sqrt(vo) / bc2 + eps
        return float((np.abs(den - deno) / deno).max())
    vo = o.vM if variant == "constrained" else o.v
    out["den"] = den_err(m2[:, :V].cpu().numpy().astype(np.float64), vo)
    assert out["den"] <= tol["den"], f"second moment (Adam's denominator): {out['den']:.3e} > {tol['den']:.0e}"
    if variant == "constrained":
        fs = e.filter_state().cpu().numpy().astype(np.float64)
        out["F"] = float((np.abs(fs[0, :C] - o.F) / np.maximum(1.0, np.abs(o.F))).max())
        out["F_den"] = den_err(fs[2, :C], o.vF)
        fo = 1.0 / (1.0 + np.exp(-o.F))
        assert np.isfinite(fs).all()
        assert float(np.abs(Fg.cpu().numpy() - fo).max()) <= tol["P"]
        assert out["F"] <= tol["P"], f"filter logits: {out['F']:.3e}"
        assert float(np.abs(fs[1, :C] - o.mF).max()) <= tol["grad"] * float(np.abs(o.mF).max()), "filter first moment"
        assert out["F_den"] <= tol["den"], f"filter second moment: {out['F_den']:.3e}"
        assert np.array_equal(e.filter_state()[:, C:].cpu().numpy(), fpad0), "filter padding changed"
    # ---- padding: the columns [V, pitch) of M and both moments hold what they held after create
    for name, x, x0 in zip(("M", "exp_avg", "exp_avg_sq"), (M, m1, m2), pad0):
        assert x.shape[1] == pitch
        assert np.array_equal(x[:, V:].cpu().numpy(), x0), f"padding of {name} changed"
    if start:
        assert np.isfinite(M[:, :V].cpu().numpy()).all() and np.isfinite(m2[:, :V].cpu().numpy()).all(), "a logit or a moment is not finite"
        out["guard"] = _conditioning_guard(o, data, lam, variant, M0, F0, start, eps, lr, n, dM, sc, floor, hist_o, cols, tol, ltol)
    if readouts:
        _readouts_at_state(e, o, data, variant, P32, precision if not smallc else "fp32", seed)
    e.release()
    return out


# ---- the CSR spatial-term kernels on irregular, weighted, asymmetric spot graphs (tests/test_spatial_graphs.py on the emulator,
# tests/test_gpu_spatial_graphs.py on the GPU) ----------------------------------------------------------------------------------
BETA1 = 0.9


def _grad_from_first_moment(eng, V):
    _, m1, _, _ = eng.logits()
    return m1[:, :V] / (1.0 - BETA1)            # exp_avg after one step = (1 - beta1) * grad


# term -> (lambda name, lambda of these kernel tests, history column name in _capi, the oracle's name of the term value).
# The lambdas are far above the tutorial's where the term is otherwise a vanishing share of the gradient (islands at 0.17 are
# 0.3 % of the gradient norm on the irregular graph, 4 % at 10; Geary at 0.3 is 3 %): every term has to be at least a tenth of the gradient for its own
# error to be visible (spatial_graph_case asserts that share on the oracle).
SPATIAL_TERMS = {
    "nb":    ("lambda_neighborhood_g1", 0.96, "H_NB", "nb_sim"),
    "ct":    ("lambda_ct_islands", 40.0, "H_CT", "ct_island"),
    "getis": ("lambda_getis_ord", 0.5, "H_GETIS", "getis_sim"),
    "moran": ("lambda_moran", 0.4, "H_MORAN", "moran_sim"),
    "geary": ("lambda_geary", 3.0, "H_GEARY", "geary_sim"),
}
ALL_FIVE = ("nb", "ct", "getis", "moran", "geary")
GRAD_TOL = 1e-5                  # first-step gradient, relative Frobenius norm (the bound of the existing spatial GPU tests)
PART_TOL = 2e-4                  # spatial part of the gradient: 2 * GRAD_TOL / share with share >= MIN_SHARE
MIN_SHARE = 0.1


def _row_standardised(W):
    rs = W.sum(axis=1, keepdims=True)
    rs[rs == 0] = 1
    return (W / rs).astype(np.float32)


def spatial_graphs(graph, V, seed):
    """The three dense float32 spot graphs of one case: voxel_weights (row-standardised + identity), neighborhood_filter,
    spatial_weights (row-standardised, no self loops) -- spatial_weights.py:5-29 roles -- on the pattern named by `graph`:
    "irregular" (oracle.tangram_oracle.irregular_graph), "ring<n>" (every row exactly n unequal non-zeros, asymmetric),
    "star_out" (all rows empty but one), "star_in" (no empty row, the transpose has V - 2 empty rows)."""
    from oracle import tangram_oracle as orc
    if graph == "irregular":
        return dict(voxel_weights=orc.irregular_graph(V, seed, True, True),
                    neighborhood_filter=orc.irregular_graph(V, seed, False, False, binary=True),
                    spatial_weights=orc.irregular_graph(V, seed, True, False))
    if graph.startswith("ring"):
        n = int(graph[4:])
        R = orc.ring_graph(V, n, seed)
        Nf = (R / np.float32(n)).astype(np.float32)               # unequal weights, row sums about 1: D = ct - N ct changes sign
    else:
        R = orc.star_graph(V, V // 3, graph == "star_out", seed)
        Nf = _row_standardised(R) if graph == "star_out" else R
    Ws = _row_standardised(R)
    return dict(voxel_weights=Ws + np.eye(V, dtype=np.float32), neighborhood_filter=Nf, spatial_weights=Ws)


def spatial_problem(C, K, V, T, graph, terms, seed):
    """(data, M0, lambdas, graph keywords of the enabled terms) of one spatial case."""
    from oracle import tangram_oracle as orc
    data = orc.make_synthetic(C, K, V, seed=seed, n_types=T)
    M0 = orc.reference_init_M(C, V, seed + 1)
    lam = dict(lambda_g1=1.0, lambda_d=1.0)
    for t in terms:
        lam[SPATIAL_TERMS[t][0]] = SPATIAL_TERMS[t][1]
    g = spatial_graphs(graph, V, seed)
    kw = {}
    if "nb" in terms:
        kw["voxel_weights"] = g["voxel_weights"]
    if "ct" in terms:
        kw.update(neighborhood_filter=g["neighborhood_filter"], ct_encode=data["ct_encode"])
    if set(terms) & {"getis", "moran", "geary"}:
        kw["spatial_weights"] = g["spatial_weights"]
    return data, M0, lam, kw


def spatial_oracle(C, K, V, T, graph, terms, seed, n=3):
    """fp64 oracle of one spatial case: per-epoch terms, the mapping after n epochs, the first-step gradient with the
    spatial terms and without them, and the spatial share of the gradient."""
    from oracle import tangram_oracle as orc
    data, M0, lam, kw = spatial_problem(C, K, V, T, graph, terms, seed)
    o = orc.OracleMapper(data["S"], data["G"], d=data["d"], M0=M0, dtype=np.float64, **lam, **kw)
    hist, dM = [], None
    for i in range(n):
        _, g = o.loss_and_grad()
        if i == 0:
            dM = g.copy()
        hist.append(o.step(0.1))
    base = {k: v for k, v in lam.items() if k in ("lambda_g1", "lambda_d")}
    _, dM0 = orc.OracleMapper(data["S"], data["G"], d=data["d"], M0=M0, dtype=np.float64, **base).loss_and_grad()
    share = float(np.linalg.norm(dM - dM0) / np.linalg.norm(dM))
    return dict(hist=hist, P=orc.softmax_rows(o.M), dM=dM, dM0=dM0, share=share)


def _engine_graphs(kw, csr):
    import scipy.sparse as sp
    return {k: (sp.csr_matrix(v) if csr and k != "ct_encode" else v) for k, v in kw.items()}


def spatial_graph_case(device, C, K, V, T, graph, terms, precision, tile=0, csr=False, seed=0, n=3, ref=None, part=True):
    """One problem with CSR spatial terms through the C ABI against the fp64 oracle, n epochs; returns the measured errors.

    Checks: every enabled history column -- total, main, KL and each spatial term's own column -- at TOL[precision]["loss"]; the
    mapping at TOL[precision]["P"]; the first-step gradient (Adam's first moment) at GRAD_TOL relative (1e-2 in plain bf16, the
    bound of tests/test_gpu_production_tiles.py); and, for `part`, the SPATIAL PART of the gradient by itself: engine and oracle
    run a second time with the spatial lambdas at 0, g_with - g_without is compared on both sides relative to the oracle's
    |g_with - g_without|.  Two gradients each within GRAD_TOL |g| differ from the truth's difference by at most 2 GRAD_TOL |g| =
    2 GRAD_TOL / share relative, share = |g_with - g_without| / |g_with|: the oracle's share must be at least MIN_SHARE (a
    condition on the inputs, evaluated on the checker) and the engine is held to PART_TOL = 2 GRAD_TOL / MIN_SHARE."""
    from tangram_amd.engine import HipMapperEngine
    from tangram_amd import _capi
    tol = TOL[precision]
    data, M0, lam, kw = spatial_problem(C, K, V, T, graph, terms, seed)
    ref = ref or spatial_oracle(C, K, V, T, graph, terms, seed, n)
    e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], device=device, precision=precision, lambdas=lam, tile_size=tile,
                        **_engine_graphs(kw, csr))
    hist = e.new_history(n)
    e.step(1, 0.1, hist, 0)
    g = _grad_from_first_moment(e, V).cpu().numpy().astype(np.float64)
    e.step(n - 1, 0.1, hist, 1)
    h = hist.cpu().numpy().astype(np.float64)
    P = e.result().cpu().numpy().astype(np.float64)
    e.release()
    out = dict(share=ref["share"])
    out["grad"] = float(np.linalg.norm(g - ref["dM"]) / np.linalg.norm(ref["dM"]))
    cols = [(_capi.H_TOTAL, "total_loss"), (_capi.H_MAIN, "main_loss"), (_capi.H_KL, "kl_reg")]
    cols += [(getattr(_capi, SPATIAL_TERMS[t][2]), SPATIAL_TERMS[t][3]) for t in terms]
    out["loss"] = {}
    for col, k in cols:
        r = np.array([float(x[k]) for x in ref["hist"]])
        out["loss"][k] = float(np.abs(h[:, col] - r).max() / max(1.0, float(np.abs(r).max())))
    out["P"] = float(np.abs(P - ref["P"]).max())
    if part:
        base = {k: v for k, v in lam.items() if k in ("lambda_g1", "lambda_d")}
        e0 = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], device=device, precision=precision, lambdas=base, tile_size=tile)
        e0.step(1, 0.1, e0.new_history(1), 0)
        g0 = _grad_from_first_moment(e0, V).cpu().numpy().astype(np.float64)
        e0.release()
        d_ref = ref["dM"] - ref["dM0"]
        out["part"] = float(np.linalg.norm((g - g0) - d_ref) / np.linalg.norm(d_ref))
    print(f"spatial case C{C} K{K} V{V} T{T} {graph} {'+'.join(terms)} {precision} tile{tile} csr{int(csr)}: {out}")
    if part:
        assert ref["share"] >= MIN_SHARE, f"inputs: the spatial terms are only {ref['share']:.3f} of the oracle's gradient"
    for k, err in out["loss"].items():
        assert err <= tol["loss"], f"{k}: max per-epoch |delta| {err:.3e} > {tol['loss']:.0e}"
    assert out["P"] <= tol["P"], f"max|dP| {out['P']:.3e} > {tol['P']:.0e}"
    gtol = 1e-2 if precision == "bf16" else GRAD_TOL
    assert out["grad"] <= gtol, f"first-step gradient rel err {out['grad']:.3e} > {gtol:.0e}"
    if part:
        ptol = PART_TOL * (gtol / GRAD_TOL)
        assert out["part"] <= ptol, f"spatial part of the first-step gradient rel err {out['part']:.3e} > {ptol:.0e}"
    return out


def spatial_cases(gpu):
    """The shared case table: (id, C, K, V, T, graph, terms, tile_size, csr).  The emulated table uses smaller C / V where the
    emulator's time demands and keeps every edge; the edge is named in the id."""
    big = gpu
    out = []
    C, K, V = 300, 50, 501                                        # 501 spots: not a multiple of 8 (the XCD bands of tg_spmm are unequal)
    for i, terms in enumerate([(t,) for t in ALL_FIVE] + [ALL_FIVE]):
        out.append((f"irregular-{'all5' if len(terms) == 5 else terms[0]}", C, K, V, 9, "irregular", terms, 0, i % 2 == 0))
    # every row exactly n non-zeros: one full trip of tg_spmm's eight-at-a-time loop, one past it, two full trips, one past them
    for i, nnz in enumerate((8, 9, 16, 17)):
        out.append((f"ring-rows-of-{nnz}", 300 if big else 60, 50 if big else 24, 131, 5, f"ring{nnz}", ALL_FIVE, 0, i % 2 == 1))
    out.append(("star-all-rows-empty-but-one", 300 if big else 60, 50 if big else 24, 67, 5, "star_out", ALL_FIVE, 0, True))
    out.append(("star-transpose-has-empty-rows", 300 if big else 60, 50 if big else 24, 67, 5, "star_in", ALL_FIVE, 0, False))
    # second trip of the gene strides of tg_spmm (4 x 256 genes per trip) and tg_ac_finalize (1 024 threads); 1 025 and 1 030: a ragged
    # last quad on the second trip
    for i, Kg in enumerate((1021, 1024, 1025, 1030, 2000)):
        out.append((f"genes-{Kg}-second-stride-trip", 500 if big else 40, Kg, 3000 if big else 100, 5, "irregular", ALL_FIVE, 0, i % 2 == 0))
    out.append(("genes-6200-all-genes-width", 300 if big else 33, 6200, 600 if big else 64, 5, "irregular", ALL_FIVE, 0, True))
    # cell types: the 64-thread stride of tg_ct_mask / tg_ct_grad (63, 64, 65, 130 types) and K + 1 + T below / at / above a multiple
    # of the tile on both layouts (Kp = K + 1 + T rounded up to the tile: tg_make_layout)
    for i, (Kg, T, tile) in enumerate(((63, 63, 128), (63, 64, 128), (63, 65, 128), (124, 130, 256), (125, 130, 256), (126, 130, 256))):
        for terms in (("ct",), ("nb", "ct")):
            out.append((f"types-{T}-aug-{Kg + 1 + T}-tile{tile}-{'+'.join(terms)}", 300, Kg, 70, T, "irregular", terms, tile, (i + len(terms)) % 2 == 0))
    # TG_RB = 16 spots per block of the per-gene partial kernels (tg_colstats, tg_ac_stats1/2, tg_ac_grad, tg_ac_refs)
    for i, Vs in enumerate((15, 16, 17, 33)):
        out.append((f"spots-{Vs}-row-block-of-16", 40, 20, Vs, 3, "ring9", ALL_FIVE, 0, i % 2 == 0))
    if gpu:
        out.append(("autocorr-at-size", 500, 257, 3000, 0, "irregular", ("getis", "moran", "geary"), 0, True))
    return out


def spatial_shards_case(device, precision, world=3, n=3, seed=11):
    """All five terms on `world` spot shards (threads, tests/local_comm.py) of the 1 001-spot irregular graph -- every shard
    gathers Ghat and evaluates the whole graph, the hub row reads rows of every shard -- against the single engine and the
    fp64 oracle (the comparisons of test_spatial_terms_on_spot_shards_match_single_engine, every spatial column included)."""
    from tangram_amd.engine import HipMapperEngine
    from tangram_amd.sharded import make_sharded
    from tangram_amd import _capi
    from tests.local_comm import run_ranks
    C, K, V, T = 120, 24, 1001, 5
    data, M0, lam, kw = spatial_problem(C, K, V, T, "irregular", ALL_FIVE, seed)
    graphs = _engine_graphs(kw, True)

    def rank_fn(comm):
        sh = make_sharded(data["S"], data["G"], M0, d=data["d"], device=device, precision=precision, lambdas=lam, comm=comm, **graphs)
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
    ref = spatial_oracle(C, K, V, T, "irregular", ALL_FIVE, seed, n)
    names = [(_capi.H_TOTAL, "total_loss"), (_capi.H_MAIN, "main_loss"), (_capi.H_KL, "kl_reg")]
    names += [(getattr(_capi, SPATIAL_TERMS[t][2]), SPATIAL_TERMS[t][3]) for t in ALL_FIVE]
    cols = [c for c, _ in names]
    tol = TOL[precision]
    for hist, P in res:
        np.testing.assert_array_equal(hist, res[0][0])                         # the same global history on every rank
        np.testing.assert_allclose(hist[:, cols], h1[:, cols], atol=5e-6, rtol=2e-6)
        np.testing.assert_allclose(P, P1, atol=2e-6)
        for col, k in names:
            r = np.array([float(x[k]) for x in ref["hist"]])
            err = float(np.abs(hist[:, col] - r).max())
            assert err <= tol["loss"] * max(1.0, float(np.abs(r).max())), f"{k}: max per-epoch |delta| {err:.3e}"
        assert float(np.abs(P - ref["P"]).max()) <= tol["P"]


def _run_engine(device, precision, data, M0, lam, graphs, n=3):
    from tangram_amd.engine import HipMapperEngine
    e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], device=device, precision=precision, lambdas=lam, **graphs)
    hist = e.new_history(n)
    e.step(n, 0.1, hist)
    out = hist.cpu().numpy(), e.result().cpu().numpy()
    e.release()
    return out


def spatial_csr_input_case(device, precision, seed=5):
    """The spot graphs as a caller may hand them: unsorted indices, explicit zeros, int64 indices, float64 data, csc / coo format give
    the same history and mapping as the canonical float32 CSR matrix, bit for bit; duplicate entries (summed by the conversion, in
    another order) within TOL."""
    import scipy.sparse as sp
    C, K, V, T = 80, 24, 131, 5
    data, M0, lam, kw = spatial_problem(C, K, V, T, "irregular", ALL_FIVE, seed)
    gk = [k for k in kw if k != "ct_encode"]
    canon = {k: sp.csr_matrix(kw[k]) for k in gk}
    for m in canon.values():
        m.sort_indices()
    h0, P0 = _run_engine(device, precision, data, M0, lam, dict(kw, **canon))
    rng = np.random.default_rng(seed)

    def unsorted(m):
        m = m.copy()
        for v in range(V):
            b, e = m.indptr[v], m.indptr[v + 1]
            perm = rng.permutation(e - b)
            m.indices[b:e], m.data[b:e] = m.indices[b:e][perm], m.data[b:e][perm]
        m.has_sorted_indices = False
        return m

    def explicit_zeros(m):
        coo = m.tocoo()
        zr, zc = rng.integers(0, V, 3 * V), rng.integers(0, V, 3 * V)
        free = np.asarray(m[zr, zc]).ravel() == 0
        zr, zc = zr[free], zc[free]
        out = sp.coo_matrix((np.concatenate([coo.data, np.zeros(len(zr), np.float32)]),
                             (np.concatenate([coo.row, zr]), np.concatenate([coo.col, zc]))), shape=(V, V))
        rows, inv = np.unique(np.stack([out.row, out.col]), axis=1, return_index=True)      # keep one entry per position
        out = sp.csr_matrix((out.data[inv], (out.row[inv], out.col[inv])), shape=(V, V))
        assert out.nnz > m.nnz and (out.data == 0).any()
        return out

    def int64_indices(m):
        return sp.csr_matrix((m.data, m.indices.astype(np.int64), m.indptr.astype(np.int64)), shape=m.shape)

    def float64_data(m):
        return sp.csr_matrix((m.data.astype(np.float64), m.indices, m.indptr), shape=m.shape)

    def duplicates(m):
        coo = m.tocoo()
        half = (coo.data * np.float32(0.5)).astype(np.float32)
        return sp.coo_matrix((np.concatenate([half, coo.data - half]), (np.concatenate([coo.row, coo.row]), np.concatenate([coo.col, coo.col]))),
                             shape=(V, V))

    variants = dict(unsorted=unsorted, explicit_zeros=explicit_zeros, int64_indices=int64_indices, float64_data=float64_data,
                    csc=lambda m: m.tocsc(), coo=lambda m: m.tocoo())
    for name, fn in variants.items():
        h, P = _run_engine(device, precision, data, M0, lam, dict(kw, **{k: fn(canon[k]) for k in gk}))
        np.testing.assert_array_equal(h, h0, err_msg=name)
        np.testing.assert_array_equal(P, P0, err_msg=name)
    h, P = _run_engine(device, precision, data, M0, lam, dict(kw, **{k: duplicates(canon[k]) for k in gk}))
    tol = TOL[precision]
    keep = ~np.isnan(h0)
    assert (np.isnan(h) == np.isnan(h0)).all()
    assert float(np.abs(h[keep] - h0[keep]).max()) <= tol["loss"] * max(1.0, float(np.abs(h0[keep]).max())), "duplicates: history"
    assert float(np.abs(P - P0).max()) <= tol["P"], "duplicates: mapping"


def spatial_determinism_case(device, precision, seed=7):
    """Two runs of the all-five irregular case: bit-identical histories and mappings (fixed-order reductions everywhere)."""
    cid, C, K, V, T, graph, terms, tile, csr = [c for c in spatial_cases(False) if c[0] == "irregular-all5"][0]
    data, M0, lam, kw = spatial_problem(C, K, V, T, graph, terms, seed)
    a = _run_engine(device, precision, data, M0, lam, _engine_graphs(kw, True))
    b = _run_engine(device, precision, data, M0, lam, _engine_graphs(kw, True))
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


# ---- the validation metrics of Mapper._val_loss_fn on every kernel path (tests/test_validation_metrics.py on the emulator,
# tests/test_gpu_validation_metrics.py on the GPU) -------------------------------------------------------------------------------
VAL_KEYS = ("val_total_loss", "val_gene_sim", "val_sp_sparsity_weighted_sim", "val_entropy")
# Conditioning of a case's inputs, evaluated on the checker only: the fp64 formula evaluated in NumPy float32 stays within a third
# of the tightest bound (TOL["fp32"]["loss"]) of its fp64 value at every point a case validates
VAL_COND = TOL["fp32"]["loss"] / 3.0
TG_RB, TG_GH_COLS, TG_SC_MAXC, ROWPASS_MAX_V = 16, 256, 32, 16384        # tg_kernels.h / tg_small.h / tg_capi.hip


def val_nky(K, tile):
    """Parts of voxstat: K + 1 gene columns padded to the tile (tg_make_layout), TG_GH_COLS columns per part (tg_ghat_reduce)."""
    Kp = -(-(K + 1) // (tile or 128)) * (tile or 128)
    return -(-Kp // TG_GH_COLS)


def validation_problem(C, K, V, seed, zero_genes=0, sharpen=1.0):
    """(S, G, d, M0) of one validation case.  zero_genes = z: the first z gene columns of G are zero in every spot, the next z in
    every spot but one (their non-zero fraction is 0 and 1 / V); the rest stay as drawn.  sharpen: factor on the initial logits."""
    from oracle import tangram_oracle as orc
    data = orc.make_synthetic(C, K, V, seed=seed)
    G = data["G"].copy()
    if zero_genes:
        z = int(zero_genes)
        assert 2 * z < K, "at least one gene stays as drawn: the weighted score needs a non-zero weight"
        G[:, :z] = 0.0
        G[:, z:2 * z] = 0.0
        G[np.arange(z) % V, np.arange(z, 2 * z)] = 3.0
    M0 = (orc.reference_init_M(C, V, seed + 1) * np.float32(sharpen)).astype(np.float32)
    return data["S"], G, data["d"], M0


def _val_check(got, M, S, G, out, where):
    """One validation of the library against the fp64 formula at logits M; keeps the largest errors in `out`."""
    from oracle import tangram_oracle as orc
    ref = orc.validation_metrics(M, S, G)
    ref32 = orc.validation_metrics(M, S, G, dtype=np.float32)
    assert all(np.isfinite(ref)), (where, ref)
    for k, g, r, r32 in zip(VAL_KEYS, got, ref, ref32):
        out["cond"] = max(out.get("cond", 0.0), abs(r32 - r))
        out[k] = max(out.get(k, 0.0), abs(g - r) if np.isfinite(g) else np.inf)
    out.setdefault("points", []).append((where, tuple(got), ref))
    return ref


def _val_assert(out, bound, label):
    print(f"validation case {label}: " + " ".join(f"{k}={out[k]:.2e}" for k in VAL_KEYS + ("cond",)))
    assert out["cond"] <= VAL_COND, f"inputs: the float32 evaluation of the checker is {out['cond']:.2e} from its float64 value (> {VAL_COND:.1e})"
    for k in VAL_KEYS:
        assert out[k] <= bound, f"{k}: |library - fp64 formula| = {out[k]:.3e} > {bound:.0e}   {out['points']}"


def validation_case(device, C, K, V, precision, tile=0, lambda_g2=0.5, pipeline_bands=0, zero_genes=0, sharpen=1.0, s_exact=False,
                    n=3, seed=0, label=""):
    """engine.validate() before any step, after one step and after n steps against oracle.validation_metrics (fp64) at the
    oracle's logits; returns the largest |difference| per metric.  Bound: TOL[precision]["loss"] absolute on each of the four
    numbers (the fp32 row for a clusters-mode handle, whatever precision was asked).  The path is asserted: the small-C flag, the
    tile and the bands of tg_debug_layout, the precision the handle reports, and (profile_read of the first step) the forward
    kernel and the update kernels of update_instantiation.  A handle with bands > 1 is not profiled: profiling switches the
    band pipeline off (tg_dispatch_step)."""
    import ctypes as ct
    from tangram_amd.engine import HipMapperEngine
    from oracle import tangram_oracle as orc
    S, G, d, M0 = validation_problem(C, K, V, seed, zero_genes, sharpen)
    lam = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=lambda_g2)
    smallc = C <= TG_SC_MAXC and tile == 0 and V <= ROWPASS_MAX_V
    o = orc.OracleMapper(S, G, d=d, M0=M0, dtype=np.float64, **lam)
    e = HipMapperEngine(S, G, M0, d=d, device=device, precision=precision, lambdas=lam, tile_size=tile, pipeline_bands=pipeline_bands,
                        s_exact="auto" if s_exact else False)
    geo = (ct.c_int * 8)()
    assert e._lib.tg_debug_layout(ct.byref(e.cfg), geo) == 0
    assert (geo[7], geo[0], geo[6]) == (int(smallc), tile or 128, max(1, pipeline_bands)), f"smallc / tile / bands = {geo[7]}, {geo[0]}, {geo[6]}"
    want = "fp32" if smallc else ("bf16x3 (S exact: 2 products)" if s_exact else precision)
    assert e.effective_precision == want, (e.effective_precision, want)
    bound = TOL["fp32" if smallc else precision]["loss"]
    out = dict(kind=("tg_sc" if smallc else update_instantiation(C, V, precision, "plain")))
    _val_check(e.validate(), o.M, S, G, out, "before any step")
    hist = e.new_history(n)
    if geo[6] == 1:
        e.profile(True)
        e.step(1, 0.1, hist, 0)
        names = [k for k, _, _ in e.profile_read()]
        e.profile(False)
        if smallc:
            assert "tg_sc_forward" in names and "tg_sc_backward" in names and "tg_fwd_kernel" not in names, names
        else:
            assert "tg_fwd_kernel" in names and "tg_sc_forward" not in names, names
            if out["kind"][0] == "tg_adam_rowpass":
                assert "tg_adam_rowpass" in names and "tg_adam_update" not in names and "tg_rowsum_parts" not in names, names
            else:
                assert "tg_rowsum_parts" in names and "tg_adam_update" in names and "tg_adam_rowpass" not in names, names
        assert "tg_gene_reduce" in names, names
    else:
        e.step(1, 0.1, hist, 0)
    o.step(0.1)
    _val_check(e.validate(), o.M, S, G, out, "after 1 step")
    e.step(n - 1, 0.1, hist, 1)
    for _ in range(n - 1):
        o.step(0.1)
    _val_check(e.validate(), o.M, S, G, out, f"after {n} steps")
    e.release()
    _val_assert(out, bound, label or f"C{C} K{K} V{V} {precision}")
    return out


def validation_cases(gpu):
    """The shared case table: dicts of id + the arguments of validation_case.  Every id names the edge it is there for.  The
    emulated table keeps every edge and uses fewer cells where the edge does not need them.  Every case runs in bf16x3 (the
    clusters-mode ones compute in fp32 whatever is asked); every third case of the GEMM path also in fp32 and in plain bf16; two
    cases on the two-product path (s_exact: make_synthetic's S is count-valued)."""
    Cs = 300 if gpu else 48                      # (GPU: three cell tiles where the edge is about genes)
    base = []

    def add(cid, C, K, V, **kw):
        base.append(dict(id=cid, C=C, K=K, V=V, precision="bf16x3", **kw))

    for V in (255, 256, 257, 513):               # tg_row_entropy: 256 threads stride over the spots of a row
        add(f"spots-{V}-row-entropy-stride-256", 48, 20, V)
    for V in (1023, 1024, 1025, 2050):           # tg_val_finalize: 1 024 threads stride over the spots
        add(f"spots-{V}-finalize-stride-1024", 48, 20, V)
    for K in (1023, 1024, 1025):                 # ... over the genes
        add(f"genes-{K}-finalize-stride-1024", 40, K, 64)
    for C in (1023, 1025):                       # ... over the row entropies
        add(f"cells-{C}-finalize-stride-1024", C, 20, 64)
    for tile in (128, 256):                      # voxstat parts of TG_GH_COLS = 256 gene columns, K + 1 padded to the tile
        for K in (254, 255, 256, 300):
            add(f"genes-{K}-tile{tile}-nky{val_nky(K, tile)}", Cs, K, 70, tile=tile)
    add("genes-600-nky3", Cs, 600, 70)
    add("lambda-g2-0-gemm-path", Cs, 20, 70, lambda_g2=0.0)
    add("lambda-g2-0-clusters-path", 18, 20, 70, lambda_g2=0.0)
    for V in (15, 16, 17, 33):                   # TG_RB = 16 spots per row block: gnnzpart / gfrac with genes that are zero (almost) everywhere
        add(f"spots-{V}-row-block-of-16-sparse-genes", 40, 20, V, zero_genes=4)
    add("spots-8200-tall-gene-reduce-sparse-genes", 40, 20, 8200, zero_genes=4)
    add("spots-4000-after-rowpass-256-threads", 40, 8, 4000)                    # the row constants each update family leaves
    add("spots-4100-after-rowpass-512-threads", 40, 8, 4100)
    add("spots-16400-cells-40-after-adam-update-1024-threads", 40, 8, 16400)
    add("spots-16400-cells-70-after-adam-update-256-threads", 70, 8, 16400)
    add("clusters-1-cell", 1, 9, 70)
    add("clusters-18-cells-250-genes-1300-spots", 18, 250, 1300)
    add("clusters-32-cells-1300-spots", 32, 9, 1300)
    add("clusters-32-cells-250-genes", 32, 250, 70)
    add("cells-33-first-gemm-path", 33, 9, 70)
    base.append(dict(id="clusters-18-cells-bf16-asked-fp32-runs", C=18, K=9, V=70, precision="bf16"))
    add("clusters-18-cells-default-path", 18, 9, 70)
    add("clusters-18-cells-tile128-pins-gemm-path", 18, 9, 70, tile=128)
    for b in (2, 3):
        add(f"pipeline-bands-{b}", 420, 16, 150, pipeline_bands=b)
    for K in (6015, 6016, 6200):                 # Kp = 6 016 / 6 144 / 6 272 on 128 tiles: below, at and past the self-emit bound (6 128)
        add(f"genes-{K}-all-genes-width", 40, K, 64)
    if gpu:
        # the 256-tile width of tests/test_gpu_wide_genes.py (K = 5 888: Kp = 6 144, the first off the self-emit path on 256 tiles) with
        # the tile pinned on 300 cells: at that module's 4 200 x 5 888 x 1 500 the fp64 checker alone takes 15 s of CPU per case
        add("genes-5888-all-genes-width-tile256", 300, 5888, 600, tile=256)
    add("sharpened-logits-x30-spots-300", 48, 20, 300, sharpen=30.0)
    out = list(base)
    # (the emulator spends half a minute per handle of 8 200 or 16 400 spots: those cases run in bf16x3 alone there)
    gemm = [c for c in base if not (c["C"] <= TG_SC_MAXC and not c.get("tile")) and c["K"] != 5888 and (gpu or c["V"] < 8000)]
    for i, c in enumerate(gemm):
        if i % 3 == 0:
            out.append(dict(c, id=c["id"] + "-fp32", precision="fp32"))
            out.append(dict(c, id=c["id"] + "-bf16", precision="bf16"))
    for cid in ("spots-257-row-entropy-stride-256", "genes-256-tile128-nky2"):
        c = [c for c in base if c["id"] == cid][0]
        out.append(dict(c, id=cid + "-two-products", s_exact=True))
    return out


def run_validation_case(device, case):
    kw = {k: v for k, v in case.items() if k != "id"}
    return validation_case(device, seed=case["C"] + case["V"], label=case["id"], **kw)


def _state_of(e):
    M, m1, m2, step = e.logits()
    return [x.cpu().numpy().copy() for x in (M, m1, m2)] + [step]


def validation_undisturbed_case(device, C, K, V, precision="bf16x3", calls=(1, 1, 1, 1), **kw):
    """A handle that validates (twice) after every call of `step` and a handle that never does: bit-identical history rows, logits
    and both Adam moments, padding columns included; the two validations in a row return identical floats."""
    from tangram_amd.engine import HipMapperEngine
    S, G, d, M0 = validation_problem(C, K, V, C + V)
    lam = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=kw.pop("lambda_g2", 0.5))
    res = []
    for validate in (True, False):
        e = HipMapperEngine(S, G, M0, d=d, device=device, precision=precision, lambdas=lam, **kw)
        hist = e.new_history(sum(calls))
        row = 0
        if validate:
            assert e.validate() == e.validate()
        for k in calls:
            e.step(k, 0.1, hist, row)
            row += k
            if validate:
                a, b = e.validate(), e.validate()
                assert a == b and all(np.isfinite(a)), (a, b)
        res.append([hist.cpu().numpy().copy()] + _state_of(e))
        e.release()
    for name, x, y in zip(("history", "M", "exp_avg", "exp_avg_sq"), res[0], res[1]):
        np.testing.assert_array_equal(x, y, err_msg=name)
    assert res[0][4] == res[1][4] == sum(calls)


def validation_refused_case(device):
    """MapperConstrained has no validation loss: the handle refuses, with the library's message, and trains on."""
    import pytest
    from tangram_amd.engine import HipMapperEngine
    from oracle import tangram_oracle as orc
    C, K, V = 40, 12, 50
    data = orc.make_synthetic(C, K, V, seed=5)
    M0, F0 = orc.reference_init_MF_constrained(C, V, 6)
    lam = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5, lambda_count=1.0, lambda_f_reg=1.0)
    e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], F0=F0, mode="constrained", device=device, lambdas=lam, target_count=20.0)
    hist = e.new_history(2)
    e.step(1, 0.1, hist, 0)
    with pytest.raises(Exception, match="MapperConstrained has no validation loss"):
        e.validate()
    e.step(1, 0.1, hist, 1)
    assert np.isfinite(hist.cpu().numpy()[:, 0]).all()
    e.release()


def validation_shards_case(device, precision, world, C, K, V, empty_gene_on_rank=None, n=3, seed=13):
    """Spot shards (threads, tests/local_comm.py) against the fp64 formula on the FULL problem: validate() before any step, after one
    and after n steps; every rank returns the same floats; the history and this rank's state are bit-identical to a sharded run
    that never validates.  empty_gene_on_rank = r: gene 0 is zero in every spot of rank r's block (its non-zero fraction comes
    from the other ranks alone) and gene 1 is zero in every spot of every OTHER rank's block."""
    from tangram_amd.sharded import make_sharded, shard_bounds
    from oracle import tangram_oracle as orc
    from tests.local_comm import run_ranks
    S, G, d, M0 = validation_problem(C, K, V, seed)
    if empty_gene_on_rank is not None:
        lo, hi = shard_bounds(V, world, empty_gene_on_rank)
        G[lo:hi, 0] = 0.0
        G[:lo, 1] = 0.0
        G[hi:, 1] = 0.0
        G[lo, 1] = 2.0
        assert G[:, 0].any() and G[:, 1].any()
    lam = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5)

    def rank_fn(comm, validate):
        sh = make_sharded(S, G, M0, d=d, device=device, precision=precision, lambdas=lam, comm=comm)
        hist = sh.eng.new_history(n)
        vals = []
        if validate:
            vals.append(sh.validate())
        sh.run(1, 0.1, hist, 0)
        if validate:
            vals.append(sh.validate())
            assert sh.validate() == vals[-1]
        sh.run(n - 1, 0.1, hist, 1)
        if validate:
            vals.append(sh.validate())
        out = [hist.cpu().numpy().copy()] + _state_of(sh.eng) + [vals]
        sh.release()
        return out

    with_val = run_ranks(world, lambda comm: rank_fn(comm, True))
    without = run_ranks(world, lambda comm: rank_fn(comm, False))
    o = orc.OracleMapper(S, G, d=d, M0=M0, dtype=np.float64, **lam)
    bound = TOL[precision]["loss"]
    out = {}
    for i, steps in enumerate((0, 1, n)):
        while o.t < steps:
            o.step(0.1)
        for r in range(world):
            assert with_val[r][5][i] == with_val[0][5][i], f"rank {r} holds other numbers than rank 0 after {steps} steps"
        _val_check(with_val[0][5][i], o.M, S, G, out, f"after {steps} steps")
    for r in range(world):
        for name, x, y in zip(("history", "M", "exp_avg", "exp_avg_sq", "step"), with_val[r], without[r]):
            np.testing.assert_array_equal(x, y, err_msg=f"rank {r}: {name}")
    _val_assert(out, bound, f"{world} shards C{C} K{K} V{V} {precision}" + (" (a gene empty on one shard)" if empty_gene_on_rank is not None else ""))
    return out
