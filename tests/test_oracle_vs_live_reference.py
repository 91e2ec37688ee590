"""Differential tests against the UNMODIFIED reference optimizer, beyond the committed fixtures, on seeded random
configurations (shape, priors, every combination of loss terms incl. the spatial ones, both mapper classes):
 (1) the oracle vs the reference run in float64, started from the reference's own initial logits;
 (2) the product (the C-ABI library's kernels on the CPU emulator, fp32 and split-bf16 paths) vs the reference as shipped (fp32).

The reference's side of every case (its initial logits, per-epoch losses and final mapping) was recorded by
oracle/gen_live_golden.py into tests/golden/live_reference_cases.npz, like oracle/gen_golden.py produced the other fixtures;
the configurations are drawn from the seeds by the same functions here and there."""
import os

import numpy as np
import pytest

from oracle.gen_live_golden import emulator_case, oracle_case, ORACLE_EPOCHS, EMULATOR_EPOCHS


@pytest.fixture(scope="module")
def live(golden_dir):
    z = np.load(os.path.join(golden_dir, "live_reference_cases.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("seed", range(12))
def test_oracle_follows_the_live_reference(live, seed):
    from oracle import tangram_oracle as orc
    data, lam, kw, constrained, _ = oracle_case(seed)
    ref = lambda k: live[f"oracle{seed}_{k}"]
    n = ORACLE_EPOCHS
    M0, P_ref, ref_total, ref_main = ref("M0"), ref("P"), ref("total"), ref("main")
    assert len(ref_total) == n
    if constrained:
        o = orc.OracleMapperConstrained(data["S"], data["G"], data["d"], M0=M0, F0=ref("F0"), dtype=np.float64, **lam)
        P, F, ho = o.train(n, 0.1)
        np.testing.assert_allclose(F, ref("F"), atol=2e-8)
    else:
        o = orc.OracleMapper(data["S"], data["G"], M0=M0, dtype=np.float64, **lam, **kw)
        P, ho = o.train(n, 0.1)
    scale = max(1.0, np.abs(ref_total).max())
    # (MapperConstrained stringifies its history, mapping_optimizer.py:630: str(tensor) keeps 4 decimals -- P and F carry the precision)
    tol = 6e-5 if constrained else 2e-8
    np.testing.assert_allclose(np.array(ho["total_loss"], dtype=np.float64), ref_total, atol=tol * scale, rtol=0, err_msg=str(lam))
    np.testing.assert_allclose(np.array(ho["main_loss"], dtype=np.float64), ref_main, atol=tol, rtol=0, err_msg=str(lam))
    np.testing.assert_allclose(P, P_ref, atol=1e-7, err_msg=str(lam))       # (the reference builds its spatial indicators of G in fp32)


@pytest.mark.parametrize("seed", range(8))
def test_emulated_library_follows_the_live_reference_fp32(live, seed):
    """The product itself (the C-ABI library's kernels on the CPU emulator, fp32-parity paths) against the reference AS SHIPPED
    (float32, torch CPU) on seeded random configurations, within the stated fp32 tolerances of tests/parity_common.py -- the same
    comparison the golden fixtures make, on configurations no fixture spells out."""
    from tests.hipsim.build_sim import build_sim
    from tangram_amd import _capi
    from tests import parity_common as pc
    sim_path = build_sim()
    if sim_path is None:
        pytest.skip("host clang not available to build the emulator")
    data, lam, kw, constrained, _ = emulator_case(seed)
    ref = lambda k: live[f"emu{seed}_{k}"]
    n = EMULATOR_EPOCHS
    M0, P_ref = ref("M0"), ref("P")
    _capi._install_library_for_tests(sim_path)
    try:
        from tangram_amd.engine import HipMapperEngine
        if constrained:
            F0, F_ref = ref("F0"), ref("F")
            mk = lambda p: HipMapperEngine(data["S"], data["G"], M0, d=data["d"], F0=F0, mode="constrained", device="cpu", precision=p,
                                           lambdas=lam, **kw)
            ref_total = None                      # (stringified with 4 decimals: the mapping and the filter are compared instead)
        else:
            ref_total = ref("total")
            assert len(ref_total) == n
            F_ref = None
            mk = lambda p: HipMapperEngine(data["S"], data["G"], M0, device="cpu", precision=p, lambdas=lam, **kw)
        for prec in ("fp32", "bf16x3"):
            e = mk(prec)
            h = e.new_history(n)
            e.step(n, 0.1, h)
            tol = pc.TOL[prec]
            if ref_total is not None:
                err = np.abs(h[:, _capi.H_TOTAL].numpy().astype(np.float64) - ref_total).max()
                assert err <= 2 * tol["loss"] * max(1.0, np.abs(ref_total).max()), (prec, lam, err)
            out = e.result(with_filter=constrained)
            P = (out[0] if constrained else out).numpy()
            assert np.abs(P - P_ref).max() <= tol["P"], (prec, lam)
            if constrained:
                assert np.abs(out[1].numpy() - F_ref).max() <= 1e-4
    finally:
        _capi._install_library_for_tests(None)
