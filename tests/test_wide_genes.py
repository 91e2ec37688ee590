"""All-genes widths on the emulated C ABI: Tangram trains on every gene the two datasets share by default (15 000 - 20 000 on real data),
and the schedule changes at a fixed gene count.  The dGhat emitter derives its coefficients itself (tg_dghat_emit<SELF>, one history
workgroup in the update kernel) only while its LDS, (2 Kp + 2 TG_RB) floats, fits 48 KiB: Kp <= 6128, i.e. K <= 6015 on 128 tiles
(Kp = rup(K + 1, 128)).  Past it the loss goes through tg_loss_finalize, tg_batch refuses the mappings, and the fused sharded step of the
peer transport (exchanges inside the kernels) must not be used: its E1 tail is pushed by the history workgroup that no longer exists.
K = 6015 / 6016 / 6200 cover both sides of the bound; the 256-tile side (K = 5887 / 5888) is covered on the GPU
(tests/test_gpu_wide_genes.py): its emulated geometry costs minutes."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import parity_common as pc
from tests.hipsim.build_sim import build_sim

BETA1 = 0.9
SH_C, SH_V, SH_STEPS = 40, 80, 2
SH_LAM = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5)
SH_LAM_REG = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5, lambda_r=1e-3, lambda_l1=1e-4, lambda_l2=1e-5)
SH_LAM_C = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5, lambda_r=1e-3, lambda_count=0.5, lambda_f_reg=2.0)
SH_TC = 20.0
# (problem name, lambdas, constrained)
SH_PROBLEMS = (("plain", SH_LAM, False), ("regs", SH_LAM_REG, False), ("constrained", SH_LAM_C, True))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sh_data(K):
    from oracle import tangram_oracle as orc
    data = orc.make_synthetic(SH_C, K, SH_V, seed=61)
    M0 = orc.reference_init_M(SH_C, SH_V, 7)
    M0c, F0c = orc.reference_init_MF_constrained(SH_C, SH_V, 7)
    return data, M0, M0c, F0c


def _wide_worker(rank, world, port, sim_path, outdir, K, variants):
    """Every variant (transport, TG_PEER_FUSED) on every problem, one process per rank; what each run left goes to one npz per rank."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["TG_PEER_TIMEOUT_MS"] = "3000"          # (a tail nobody sends: one bounded wait, not the default 20 s)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tangram_amd import _capi
        _capi._install_library_for_tests(sim_path)
        from tangram_amd.sharded import make_sharded
        data, M0, M0c, F0c = _sh_data(K)
        out = {}
        for var in variants:
            transport, fused0 = (var[:-len("_fused0")], True) if var.endswith("_fused0") else (var, False)
            for name, lam, constrained in SH_PROBLEMS:
                if fused0:
                    os.environ["TG_PEER_FUSED"] = "0"          # (read when the communicator is attached)
                try:
                    kw = dict(F0=F0c, mode="constrained", target_count=SH_TC) if constrained else {}
                    sh = make_sharded(data["S"], data["G"], M0c if constrained else M0, d=data["d"], device="cpu", precision="fp32",
                                      lambdas=lam, transport=transport, **kw)
                finally:
                    os.environ.pop("TG_PEER_FUSED", None)
                key = f"{var}/{name}/"
                hist = sh.eng.new_history(SH_STEPS)
                sh.eng.profile(True)
                sh.run(SH_STEPS, 0.1, hist)
                out[key + "kernels"] = np.array(";".join(k for k, _, _ in sh.eng.profile_read()))
                try:
                    sh.peer_check()
                    out[key + "peer_ok"] = np.array(1)
                except RuntimeError:
                    out[key + "peer_ok"] = np.array(0)
                out[key + "hist"] = hist.numpy()
                if not out[key + "peer_ok"]:                # (the results of a run whose exchange gave up are refused)
                    sh.release()
                    continue
                if constrained:
                    P, F = sh.result_full(with_filter=True)
                    out[key + "F"] = F.numpy()
                    out[key + "G"] = sh.project_full().numpy()
                else:
                    P = sh.result_full()
                out[key + "P"] = P.numpy()
                sh.release()
        np.savez(os.path.join(outdir, f"wide_{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


_single_cache = {}


def _single_and_oracle(sim_path, K, n):
    """The same problems on ONE handle of the emulated library, and the fp64 oracle."""
    if (K, n) in _single_cache:
        return _single_cache[(K, n)]
    from tangram_amd import _capi
    from tangram_amd.engine import HipMapperEngine
    from oracle import tangram_oracle as orc
    data, M0, M0c, F0c = _sh_data(K)
    out = {}
    _capi._install_library_for_tests(sim_path)
    try:
        for name, lam, constrained in SH_PROBLEMS:
            if constrained:
                e = HipMapperEngine(data["S"], data["G"], M0c, d=data["d"], F0=F0c, mode="constrained", device="cpu", precision="fp32",
                                    lambdas=lam, target_count=SH_TC)
            else:
                e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], device="cpu", precision="fp32", lambdas=lam)
            h = e.new_history(n)
            e.step(n, 0.1, h)
            out[name] = dict(hist=h.numpy(), P=e.result().numpy())
            e.release()
    finally:
        _capi._install_library_for_tests(None)
    for name, lam, constrained in SH_PROBLEMS:
        if constrained:
            o = orc.OracleMapperConstrained(data["S"], data["G"], data["d"], M0=M0c, F0=F0c, target_count=SH_TC, dtype=np.float64, **lam)
            Po, Fo, ho = o.train(n, 0.1)
            out[name].update(oP=Po, oF=Fo, oh=ho, oG=(Po * Fo[:, None]).T @ data["S"].astype(np.float64))
        else:
            o = orc.OracleMapper(data["S"], data["G"], d=data["d"], M0=M0, dtype=np.float64, **lam)
            Po, ho = o.train(n, 0.1)
            out[name].update(oP=Po, oh=ho)
    _single_cache[(K, n)] = out
    return out


_HCOLS = {"total_loss": "H_TOTAL", "main_loss": "H_MAIN", "vg_reg": "H_VG", "kl_reg": "H_KL", "entropy_reg": "H_ENTROPY"}
_HCOLS_C = dict(_HCOLS, count_reg="H_COUNT", lambda_f_reg="H_FREG")


def _active_cols(name):
    if name == "constrained":
        return _HCOLS_C
    return _HCOLS if name == "regs" else {k: c for k, c in _HCOLS.items() if k != "entropy_reg"}


def _spawn_and_check(tmp_path, world, K, variants):
    sim_path = build_sim()
    if sim_path is None:
        pytest.skip("host clang not available to build the emulator")
    mp.spawn(_wide_worker, args=(world, _free_port(), sim_path, str(tmp_path), K, variants), nprocs=world, join=True)
    z = [np.load(tmp_path / f"wide_{r}.npz") for r in range(world)]
    for r in range(1, world):                                   # every rank holds the same global history, mapping, filter, projection
        for k in z[0].files:
            if not k.endswith("/kernels"):
                np.testing.assert_array_equal(z[r][k], z[0][k], err_msg=f"rank {r}: {k}")
    z = z[0]
    from tangram_amd import _capi
    for var in variants:
        for name, _, _ in SH_PROBLEMS:
            key = f"{var}/{name}/"
            assert int(z[key + "peer_ok"]) == 1, f"{key}: a peer-memory exchange timed out waiting for another rank"
            h = z[key + "hist"][:, [getattr(_capi, c) for c in _active_cols(name).values()]]     # (terms that are off read NaN)
            assert np.isfinite(h).all(), f"{key}: history (row, term) {np.argwhere(~np.isfinite(h))[:4].tolist()} not finite"
            for k in ("hist", "P", "F", "G"):
                if key + k not in z.files:
                    continue
                if world == 2:               # a sum of two is the same bits in any order: every transport must agree bit for bit
                    np.testing.assert_array_equal(z[key + k], z[f"callbacks/{name}/{k}"], err_msg=f"{var} != callbacks: {name} {k}")
                else:                        # (gloo's ring does not add three ranks in rank order; the GPU tests compare bits there)
                    np.testing.assert_allclose(z[key + k], z[f"callbacks/{name}/{k}"], rtol=1e-6, atol=1e-7, err_msg=f"{var}: {name} {k}")
    ref = _single_and_oracle(sim_path, K, SH_STEPS)
    for name, _, constrained in SH_PROBLEMS:
        key = f"callbacks/{name}/"
        h, r = z[key + "hist"], ref[name]
        for k, c in _active_cols(name).items():
            col = getattr(_capi, c)
            np.testing.assert_allclose(h[:, col], r["hist"][:, col], atol=2e-6, rtol=1e-6, err_msg=f"{name} {k}: shards vs one handle")
            np.testing.assert_allclose(h[:, col], np.array(r["oh"][k], dtype=np.float64), atol=2e-5, rtol=1e-5, err_msg=f"{name} {k}: oracle")
        np.testing.assert_allclose(z[key + "P"], r["P"], atol=1e-6, err_msg=name)
        assert np.abs(z[key + "P"] - r["oP"]).max() < 1e-5, name
        if constrained:
            assert np.abs(z[key + "F"] - r["oF"]).max() < 1e-5
            assert np.linalg.norm(z[key + "G"] - r["oG"]) / np.linalg.norm(r["oG"]) < 1e-5
    return z


def _kernels(z, key):
    return set(str(z[key + "kernels"]).split(";"))


@pytest.mark.parametrize("K", [6015, 6016, 6200])
def test_two_shards_at_all_genes_widths(tmp_path, K):
    """2 ranks (processes, gloo) at both sides of the self-emit bound: plain Mapper, the regulariser row sums (lambda_r, l1, l2) and
    MapperConstrained over "callbacks", "peer" (fused step where it applies) and "peer" with TG_PEER_FUSED=0 -- bit for bit the same,
    finite, no exchange ever timed out, and the one-handle run / fp64 oracle within the tolerances of
    test_sharded_gloo.py::test_two_shards_match_single_and_oracle.  Which schedule ran is pinned by the kernels the step launched:
    up to the bound the peer step is fused (no exchange_all_reduce launch), past it the exchanges are kernels of their own."""
    z = _spawn_and_check(tmp_path, 2, K, ("callbacks", "peer", "peer_fused0"))
    self_emit = K <= 6015
    for name, _, _ in SH_PROBLEMS:
        cb, peer, p0 = _kernels(z, f"callbacks/{name}/"), _kernels(z, f"peer/{name}/"), _kernels(z, f"peer_fused0/{name}/")
        assert "tg_gene_reduce" in cb and "exchange_all_reduce" in cb, cb           # (profile_read names kernels on the emulator too)
        assert ("tg_loss_finalize" in cb) == (not self_emit), cb
        assert "exchange_all_reduce" in p0, p0
        assert ("exchange_all_reduce" in peer) == (not self_emit), (name, sorted(peer))


def test_two_shards_past_the_bound_peer_checked(tmp_path):
    """"peer_checked" (set-up self-test against the process group's own collectives, then the peer transport) past the bound."""
    _spawn_and_check(tmp_path, 2, 6200, ("callbacks", "peer_checked"))


def test_three_shards_past_the_bound_over_peer(tmp_path):
    """world 3 over the peer transport past the bound: three ranks bit-identical, equal to callbacks, the one handle and the oracle."""
    _spawn_and_check(tmp_path, 3, 6200, ("callbacks", "peer"))


# ------------------------------------------------------------------------------------------------------------------------
# one handle against the fp64 oracle
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    from tangram_amd import _capi
    path = build_sim()
    if path is None:
        pytest.skip("host clang not available to build the emulator")
    _capi._install_library_for_tests(path)
    yield path
    _capi._install_library_for_tests(None)


# (path, C, K): the GEMM kernels (C = 40) on both sides of the bound, the clusters-mode kernels (C <= 32), constrained, regularisers
SINGLE_CASES = [("gemm", 40, 6015), ("gemm", 40, 6016), ("gemm", 40, 6200), ("clusters", 20, 6200), ("constrained", 40, 6200),
                ("regs", 40, 6200)]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("path,C,K", SINGLE_CASES)
def test_single_handle_at_all_genes_widths_against_oracle(sim, path, C, K, precision):
    """First-step gradient, per-epoch history, mapping (and filter) and the projection against the fp64 oracle (pc.TOL)."""
    import ctypes as ct
    from tangram_amd import _capi
    from tangram_amd.engine import HipMapperEngine
    from oracle import tangram_oracle as orc
    V, n = 80, 3
    data = orc.make_synthetic(C, K, V, seed=17)
    S64 = data["S"].astype(np.float64)
    constrained = path == "constrained"
    lam = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5)
    if path == "regs":
        lam.update(lambda_r=1e-3, lambda_l1=1e-4, lambda_l2=1e-5)
    if constrained:
        lam.update(lambda_r=1e-3, lambda_count=0.5, lambda_f_reg=1.0)
        M0, F0 = orc.reference_init_MF_constrained(C, V, 9)
        o = orc.OracleMapperConstrained(data["S"], data["G"], data["d"], M0=M0, F0=F0, target_count=20.0, dtype=np.float64, **lam)
        e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], F0=F0, mode="constrained", device="cpu", precision=precision,
                            lambdas=lam, target_count=20.0)
    else:
        M0 = orc.reference_init_M(C, V, 9)
        o = orc.OracleMapper(data["S"], data["G"], d=data["d"], M0=M0, dtype=np.float64, **lam)
        e = HipMapperEngine(data["S"], data["G"], M0, d=data["d"], device="cpu", precision=precision, lambdas=lam)
    geo = (ct.c_int * 8)()
    assert e._lib.tg_debug_layout(ct.byref(e.cfg), geo) == 0
    assert bool(geo[7]) == (path == "clusters"), list(geo)           # smallc: the clusters-mode kernels
    dM = o.loss_and_grad()[1]
    hist = e.new_history(n)
    e.step(1, 0.1, hist, 0)
    g = e.logits()[1][:, :V].numpy().astype(np.float64) / (1.0 - BETA1)
    rel = np.linalg.norm(g - dM) / np.linalg.norm(dM)
    assert rel <= 1e-5, f"first-step gradient rel err {rel:.3e}"
    e.step(n - 1, 0.1, hist, 1)
    if constrained:
        Po, Fo, ho = o.train(n, 0.1)
        P, F = (x.numpy() for x in e.result(with_filter=True))
        assert np.abs(F - Fo).max() <= 2e-5
        ref_G = (Po * Fo[:, None]).T @ S64
    else:
        Po, ho = o.train(n, 0.1)
        P = e.result().numpy()
        ref_G = Po.T @ S64
    tol = pc.TOL[precision]
    h = hist.numpy().astype(np.float64)
    cols = dict(_HCOLS_C if constrained else _HCOLS)
    if "lambda_r" not in lam:
        cols.pop("entropy_reg")
    for k, c in cols.items():
        r = np.array([float(x) for x in ho[k]])
        err = np.abs(h[:, getattr(_capi, c)] - r).max()
        assert err <= tol["loss"] * max(1.0, np.abs(r).max()), f"{k}: max per-epoch |delta| {err:.3e}"
    assert np.abs(P - Po).max() <= tol["P"]
    Gh = e.project().numpy()
    assert np.linalg.norm(Gh - ref_G) / np.linalg.norm(ref_G) <= tol["ghat"]
    e.release()


# ------------------------------------------------------------------------------------------------------------------------
# batches: tg_batch up to the bound, streams past it -- the same bits as each mapping trained alone
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [6015, 6200])
def test_train_many_at_all_genes_widths(sim, K):
    import tangram_amd as tg
    import tangram_amd.mapping_optimizer as mo
    from tangram_amd.batched import MapperBatch, _batch_key
    from oracle import tangram_oracle as orc
    C, V, epochs = 40, 40, 2
    data = orc.make_synthetic(C, K, V, seed=5)
    kw = dict(S=data["S"], G=data["G"], d=data["d"], lambda_d=1, lambda_g1=1, lambda_g2=0.5)
    builder = lambda seed: (lambda: mo.Mapper(device="cpu", random_state=seed, gemm_precision="fp32", **kw))
    seeds = (1, 2, 3)
    res, mappers = tg.train_many([builder(s) for s in seeds], epochs, 0.1, device="cpu")
    keys = {_batch_key(m) for m in mappers}
    if K <= 6015:
        assert len(keys) == 1 and None not in keys, keys                  # grouped for one tg_batch ...
        MapperBatch([builder(s)() for s in seeds[:2]]).close()             # ... which the library accepts (no silent fall-back)
    else:
        assert keys == {None}                                              # past the bound: never grouped ...
        with pytest.raises(RuntimeError, match="genes"):                   # ... and the library says why it would refuse them
            MapperBatch([builder(s)() for s in seeds[:2]])
    solo = [builder(s)().train(num_epochs=epochs, learning_rate=0.1, print_each=None) for s in seeds]
    for i in range(3):
        np.testing.assert_array_equal(res[i][0], solo[i][0], err_msg=f"seed {seeds[i]}: mapping")
        for k in ("total_loss", "main_loss", "vg_reg", "kl_reg", "entropy_reg"):
            np.testing.assert_array_equal(np.array(res[i][1][k], dtype=np.float64), np.array(solo[i][1][k], dtype=np.float64), err_msg=k)
        assert np.isfinite(np.array(res[i][1]["total_loss"], dtype=np.float64)).all()


def test_cross_val_past_the_bound(sim):
    """cross_val with every gene past the bound (its folds cannot share a tg_batch): the folds train on streams and give the result of
    the reference's sequential procedure."""
    import tangram_amd as tg
    from tests.test_cross_val import _sequential_reference_procedure
    from tests.test_map_cells_to_space import _adatas
    ad_sc, ad_sp = _adatas(C=24, K=6200, V=30, seed=4)
    folds = list(tg.cv_data_gen(ad_sc, ad_sp, "10fold"))[:3]
    kw = dict(random_state=11, density_prior="uniform")
    t_ref, tr_ref, _ = _sequential_reference_procedure(ad_sc, ad_sp, folds, "cells", 2, **kw)
    import tangram_amd.cross_validation as cv_mod
    orig = cv_mod.cv_data_gen
    cv_mod.cv_data_gen = lambda *a, **k: iter(folds)
    try:
        cv = tg.cross_val(ad_sc, ad_sp, mode="cells", num_epochs=2, device="cpu", cv_mode="10fold", gemm_precision="fp32", **kw)
    finally:
        cv_mod.cv_data_gen = orig
    np.testing.assert_allclose(cv["avg_test_score"], t_ref.mean(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(cv["avg_train_score"], tr_ref.mean(), rtol=0, atol=1e-7)
