"""GPU parity (-m gpu) at all-genes widths.  Tangram trains on every gene the two datasets share by default (`pp_adatas(..., genes=None)`:
15 000 - 20 000 on real data); the widest gene count elsewhere in the suite is 2 000.  Past Kp = 6128 padded gene columns (K = 6015 on
128 tiles, 5887 on 256) the loss is finalised by tg_loss_finalize instead of the self-deriving dGhat emitter, the update kernel has no
history workgroup and tg_batch refuses the mappings -- the branch of the schedule every default run takes.

 * 4 200 x 16 383 x 1 500: 256 tiles, Kp = 16 384 (64 gene tiles, the wide 128 x 512 forward under bf16x3, 512 backward contraction
   steps); 4 200 x 5 888 x 1 500: the first width off the self-emit path on 256 tiles.  bf16x3, fp32, bf16 and the two-product
   `s_exact` path on integer counts; Mapper with lambda_g2 and the regularisers, MapperConstrained; against the fp64 oracle.
 * clusters mode with all genes (18 x 16 000 x 9 852, the tutorial's spots), train_many / cross_val at that width.
 * spot shards (threads of this process, tests/local_comm.py) at K = 16 383; project_genes over 18 000 genes.
Tolerances: tests/parity_common.TOL (first-step gradient: rel 1e-5, plain bf16 1e-2); every case prints what it measured (pytest -s).
Largest measured on MI355X (both widths, Mapper and MapperConstrained):
    fp32 / bf16x3 (+ s_exact)   gradient rel 4.7e-7   |d loss| 1.5e-7   max|dP| 4.5e-8   relFro(Ghat) 4.0e-7   max|dF| 1.2e-7
    bf16                        gradient rel 9.0e-5   |d loss| 5.1e-6   max|dP| 1.5e-5   relFro(Ghat) 1.5e-4   max|dF| 1.2e-7
    2 spot shards (bf16x3)      gradient rel 2.1e-7   |d loss| 7.7e-8   max|dP| 1.9e-8
    clusters 18 x 16 000        gradient rel 3.0e-7   |d loss| 1.2e-7   max|dP| 1.7e-8   relFro(Ghat) 3.8e-7"""
import numpy as np
import pytest
import torch

from tests import parity_common as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETA1 = 0.9
N_EPOCHS = 3
WIDE = (4200, 16383, 1500)
EDGE256 = (4200, 5888, 1500)
LAM = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5, lambda_r=1e-3, lambda_l1=1e-4, lambda_l2=1e-5)
LAM_C = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5, lambda_r=1e-3, lambda_count=0.5, lambda_f_reg=1.0)
GRAD_TOL = {"fp32": 1e-5, "bf16x3": 1e-5, "bf16": 1e-2}


def _record(key, **vals):
    print("measured", key, " ".join(f"{k}={v:.2e}" for k, v in vals.items()))


def _hist_err(h, ref, cols):
    from tangram_amd import _capi
    worst = 0.0
    for k in cols:
        r = np.asarray([float(x) for x in ref[k]], dtype=np.float64)
        err = float(np.abs(h[:len(r), getattr(_capi, cols[k])].astype(np.float64) - r).max()) / max(1.0, float(np.abs(r).max()))
        worst = max(worst, err)
        assert np.isfinite(err), k
    return worst


_HCOLS = {"total_loss": "H_TOTAL", "main_loss": "H_MAIN", "vg_reg": "H_VG", "kl_reg": "H_KL", "entropy_reg": "H_ENTROPY"}
_HCOLS_C = dict(_HCOLS, count_reg="H_COUNT", lambda_f_reg="H_FREG")

_oracles = {}


def _oracle(shape, constrained):
    """fp64 oracle of one problem: initial logits, first-step gradient, per-epoch history, mapping (filter), projection."""
    key = (shape, constrained)
    if key in _oracles:
        return _oracles[key]
    from oracle import tangram_oracle as orc
    C, K, V = shape
    data = orc.make_synthetic(C, K, V, seed=41)
    S64 = data["S"].astype(np.float64)
    if constrained:
        M0, F0 = orc.reference_init_MF_constrained(C, V, 8)
        o = orc.OracleMapperConstrained(data["S"], data["G"], data["d"], M0=M0, F0=F0, target_count=float(V // 2), dtype=np.float64, **LAM_C)
        dM = o.loss_and_grad()[1]
        Po, Fo, ho = o.train(N_EPOCHS, 0.1)
        out = dict(F0=F0, F=Fo, Ghat=(Po * Fo[:, None]).T @ S64)
    else:
        M0 = orc.reference_init_M(C, V, 8)
        o = orc.OracleMapper(data["S"], data["G"], d=data["d"], M0=M0, dtype=np.float64, **LAM)
        dM = o.loss_and_grad()[1]
        Po, ho = o.train(N_EPOCHS, 0.1)
        out = dict(Ghat=Po.T @ S64)
    out.update(data=data, M0=M0, dM=dM, P=Po, hist=ho)
    _oracles[key] = out
    return out


# (the two-product path is a property of S: covered on the Mapper)
WIDE_CASES = [pytest.param(shape, c, p, id=f"{sid}-{'constrained' if c else 'mapper'}-{p}")
              for shape, sid in ((WIDE, "k16383"), (EDGE256, "k5888")) for c in (False, True)
              for p in ("bf16x3", "fp32", "bf16") + (() if c else ("bf16x3+s_exact",))]


@pytest.mark.parametrize("shape,constrained,precision", WIDE_CASES)
def test_all_genes_widths_against_oracle_fp64(shape, constrained, precision):
    """One GPU at all-genes widths past the self-emit bound: first-step gradient, per-epoch history, mapping (filter), projection."""
    import ctypes as ct
    from tangram_amd.engine import HipMapperEngine
    o = _oracle(shape, constrained)
    data = o["data"]
    C, K, V = shape
    prec, s_exact = (precision.split("+")[0], "auto") if precision.endswith("s_exact") else (precision, False)
    if constrained:
        e = HipMapperEngine(data["S"], data["G"], o["M0"], d=data["d"], F0=o["F0"], mode="constrained", device=DEV, precision=prec,
                            lambdas=LAM_C, target_count=float(V // 2))
    else:
        e = HipMapperEngine(data["S"], data["G"], o["M0"], d=data["d"], device=DEV, precision=prec, lambdas=LAM, s_exact=s_exact)
    if s_exact:
        assert "S exact" in e.effective_precision, e.effective_precision       # (make_synthetic's S is counts: bf16-exact)
    geo = (ct.c_int * 8)()
    assert e._lib.tg_debug_layout(ct.byref(e.cfg), geo) == 0
    assert geo[0] == 256 and -(-(K + 1) // 256) * 256 > 6128          # 256 tiles, past the self-emit bound
    hist = e.new_history(N_EPOCHS)
    e.step(1, 0.1, hist, 0)
    g = (e.logits()[1][:, :V] / (1.0 - BETA1)).cpu().numpy().astype(np.float64)
    rel = float(np.linalg.norm(g - o["dM"]) / np.linalg.norm(o["dM"]))
    del g
    e.step(N_EPOCHS - 1, 0.1, hist, 1)
    h = hist.cpu().numpy()
    dl = _hist_err(h, o["hist"], _HCOLS_C if constrained else _HCOLS)
    if constrained:
        P, F = (x.cpu().numpy() for x in e.result(with_filter=True))
        dF = float(np.abs(F - o["F"]).max())
    else:
        P, dF = e.result().cpu().numpy(), 0.0
    dP = float(np.abs(P - o["P"]).max())
    Gh = e.project().cpu().numpy()
    rg = float(np.linalg.norm(Gh - o["Ghat"]) / np.linalg.norm(o["Ghat"]))
    e.release()
    _record(f"{K}/{'constrained' if constrained else 'mapper'}/{precision}", grad_rel=rel, loss=dl, P=dP, F=dF, ghat_rel=rg)
    tol = pc.TOL[prec]
    assert rel <= GRAD_TOL[prec], f"first-step gradient rel err {rel:.3e}"
    assert dl <= tol["loss"], f"max per-epoch |d loss| (relative to max(1, |loss|)) {dl:.3e}"
    assert dP <= tol["P"], f"max|dP| {dP:.3e}"
    assert dF <= (2e-5 if prec != "bf16" else 5e-3), f"max|dF| {dF:.3e}"
    assert rg <= tol["ghat"], f"projection relFro {rg:.3e}"


def test_spot_shards_at_all_genes_width_against_oracle_fp64():
    """4 200 x 16 383 x 1 500 as 2 spot shards (threads, callback transport): Kp = 16 384 through the row-dot backward GEMM,
    tg_loss_finalize on each shard, the regulariser row sums all-reduced -- against the fp64 oracle; every rank the same history."""
    from tangram_amd.sharded import make_sharded
    from tests.local_comm import run_ranks
    o = _oracle(WIDE, False)
    data = o["data"]

    def rank_fn(comm):
        sh = make_sharded(data["S"], data["G"], o["M0"], d=data["d"], device=DEV, precision="bf16x3", lambdas=LAM, comm=comm,
                          transport="callbacks")
        hist = sh.eng.new_history(N_EPOCHS)
        sh.run(1, 0.1, hist, 0)
        g = (sh.eng.logits()[1][:, :sh.eng.V] / (1.0 - BETA1)).cpu().numpy().astype(np.float64)
        sh.run(N_EPOCHS - 1, 0.1, hist, 1)
        out = hist.cpu().numpy(), sh.result_full().cpu().numpy(), g
        sh.release()
        return out

    res = run_ranks(2, rank_fn)
    g = np.concatenate([r[2] for r in res], axis=1)
    rel = float(np.linalg.norm(g - o["dM"]) / np.linalg.norm(o["dM"]))
    dl = max(_hist_err(h, o["hist"], _HCOLS) for h, _, _ in res)
    dP = max(float(np.abs(P - o["P"]).max()) for _, P, _ in res)
    _record("16383/shards2/bf16x3", grad_rel=rel, loss=dl, P=dP)
    assert rel <= 1e-5, f"first-step gradient rel err {rel:.3e}"
    assert dl <= pc.TOL["bf16x3"]["loss"] and dP <= pc.TOL["bf16x3"]["P"], (dl, dP)
    np.testing.assert_array_equal(res[0][0], res[1][0])


# ------------------------------------------------------------------------------------------------------------------------
# clusters mode with all genes: the tutorial's 18 clusters x 9 852 spots
# ------------------------------------------------------------------------------------------------------------------------
CL = (18, 16000, 9852)


@pytest.fixture(scope="module")
def oracle_clusters():
    from oracle import tangram_oracle as orc
    C, K, V = CL
    data = orc.make_synthetic(C, K, V, seed=43)
    M0 = orc.reference_init_M(C, V, 3)
    lam = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5)
    o = orc.OracleMapper(data["S"], data["G"], d=data["d"], M0=M0, dtype=np.float64, **lam)
    dM = o.loss_and_grad()[1]
    Po, ho = o.train(N_EPOCHS, 0.1)
    return dict(data=data, M0=M0, lam=lam, dM=dM, P=Po, hist=ho, Ghat=Po.T @ data["S"].astype(np.float64))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_clusters_all_genes_against_oracle_fp64(oracle_clusters, precision):
    import ctypes as ct
    from tangram_amd.engine import HipMapperEngine
    o = oracle_clusters
    data = o["data"]
    V = CL[2]
    e = HipMapperEngine(data["S"], data["G"], o["M0"], d=data["d"], device=DEV, precision=precision, lambdas=o["lam"])
    geo = (ct.c_int * 8)()
    assert e._lib.tg_debug_layout(ct.byref(e.cfg), geo) == 0 and geo[7], list(geo)      # the clusters-mode kernels
    hist = e.new_history(N_EPOCHS)
    e.step(1, 0.1, hist, 0)
    g = (e.logits()[1][:, :V] / (1.0 - BETA1)).cpu().numpy().astype(np.float64)
    rel = float(np.linalg.norm(g - o["dM"]) / np.linalg.norm(o["dM"]))
    e.step(N_EPOCHS - 1, 0.1, hist, 1)
    dl = _hist_err(hist.cpu().numpy(), o["hist"], {k: c for k, c in _HCOLS.items() if k != "entropy_reg"})
    dP = float(np.abs(e.result().cpu().numpy() - o["P"]).max())
    Gh = e.project().cpu().numpy()
    rg = float(np.linalg.norm(Gh - o["Ghat"]) / np.linalg.norm(o["Ghat"]))
    e.release()
    _record(f"clusters16000/{precision}", grad_rel=rel, loss=dl, P=dP, ghat_rel=rg)
    tol = pc.TOL[precision]
    assert rel <= 1e-5 and dl <= tol["loss"] and dP <= tol["P"] and rg <= tol["ghat"], (rel, dl, dP, rg)


def test_train_many_and_cross_val_at_all_genes_width(oracle_clusters):
    """Past the bound the mappings cannot share a tg_batch: train_many trains them on streams, each the same bits as alone; cross_val
    (10 folds over 16 000 genes) gives the result of the reference's sequential procedure."""
    import tangram_amd as tg
    import tangram_amd.mapping_optimizer as mo
    from tangram_amd.batched import _batch_key
    from tests.test_cross_val import _sequential_reference_procedure
    from tests.test_map_cells_to_space import _adatas
    o = oracle_clusters
    data = o["data"]
    kw = dict(S=data["S"], G=data["G"], d=data["d"], **o["lam"])
    builder = lambda seed: (lambda: mo.Mapper(device=DEV, random_state=seed, gemm_precision="bf16x3", **kw))
    seeds = (1, 2, 3)
    res, mappers = tg.train_many([builder(s) for s in seeds], 4, 0.1, device=DEV)
    assert {_batch_key(m) for m in mappers} == {None}
    for i, s in enumerate(seeds):
        P, hist = builder(s)().train(num_epochs=4, learning_rate=0.1, print_each=None)
        np.testing.assert_array_equal(res[i][0], P, err_msg=f"seed {s}")
        for k in ("total_loss", "main_loss", "vg_reg", "kl_reg"):
            np.testing.assert_array_equal(np.array(res[i][1][k], dtype=np.float64), np.array(hist[k], dtype=np.float64), err_msg=k)
    del mappers, res
    ad_sc, ad_sp = _adatas(C=60, K=16000, V=3000, seed=6)
    folds = list(tg.cv_data_gen(ad_sc, ad_sp, "10fold"))
    ckw = dict(cluster_label="subclass_label", random_state=3, density_prior="rna_count_based")
    t_ref, tr_ref, _ = _sequential_reference_procedure(ad_sc, ad_sp, folds, "clusters", 4, device=DEV, **ckw)
    cv = tg.cross_val(ad_sc, ad_sp, mode="clusters", num_epochs=4, device=DEV, cv_mode="10fold", gemm_precision="fp32", **ckw)
    np.testing.assert_allclose(cv["avg_test_score"], t_ref.mean(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(cv["avg_train_score"], tr_ref.mean(), rtol=0, atol=1e-7)


@pytest.mark.parametrize("precision,rtol", [("fp32", 2e-6), ("bf16x3", 2e-5), ("bf16", 2e-2)])
def test_project_genes_over_all_genes(precision, rtol):
    """The projection Tangram ends with (utils.py:366-368): softmax(M)^T S_all over 18 000 genes, against the fp64 product (measured
    on MI355X, max |delta| / max |P^T S_all|: fp32 3.8e-7, bf16x3 2.5e-6, bf16 7.5e-4)."""
    from tangram_amd.engine import HipMapperEngine
    from oracle import tangram_oracle as orc
    C, K, V, K_all = 4200, 300, 1500, 18000
    data = orc.make_synthetic(C, K, V, seed=12)
    e = HipMapperEngine(data["S"], data["G"], orc.reference_init_M(C, V, 2), d=data["d"], device=DEV, precision=precision,
                        lambdas=dict(lambda_g1=1.0, lambda_d=1.0))
    e.step(2, 0.1, e.new_history(2))
    P = e.result().cpu().numpy().astype(np.float64)
    S_all = np.random.default_rng(3).gamma(1.0, 2.0, size=(C, K_all)).astype(np.float32)
    out = e.project_genes(S_all).cpu().numpy()
    e.release()
    want = P.T @ S_all.astype(np.float64)
    assert out.shape == (V, K_all)
    err = float(np.abs(out - want).max() / np.abs(want).max())
    _record(f"project_genes18000/{precision}", max_rel=err)
    assert err <= rtol, f"max |delta| / max |P^T S_all| {err:.3e}"
