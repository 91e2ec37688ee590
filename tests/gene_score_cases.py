"""Tables and checks of the per-gene scores (tg_score.h: tg_score_partials / tg_score_finish; tg_gene_scores_query_bytes /
tg_gene_scores; tangram_amd.gene_scores / compare_spatial_geneexp / score_genes), shared by tests/test_gene_scores.py (emulator, device
"cpu") and tests/test_gpu_gene_scores.py (MI355X).

EXACT cases carry no tolerance: the planes hold integers in [0, 7] as floats, at most 1 025 spots, so every product is an integer
<= 49 and every partial sum an integer < 2^16 -- exact in fp64 in any order -- and the three moments must be NumPy's float64 sums,
the score `dot / (sqrt(pp) * sqrt(gg))` in NumPy float64 (IEEE square root and division), bit for bit.  The planes are column ranges
of wider NaN-filled buffers: an element read outside the range poisons a sum.  The outputs lie between sentinels.

GENERAL floats are held to derived bounds (nothing here is measured): the products of two fp32 values are exact in fp64, each of the
three sums of a gene is n_spots - 1 fp64 additions, so |moment - exact sum| <= n_spots 2^-53 sum |terms| (the standard bound of a sum
in ANY order, u = 2^-53); the score adds two square roots, a product and a quotient to three relative errors of <= n_spots 2^-53 each
(non-negative terms: sum |terms| = the sum), so |score - definition| <= 2 n_spots 2^-52 for |score| <= 1.  The definition is
evaluated from sums taken in extended precision (np.longdouble)."""
import ctypes as ct

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from tangram_amd import _capi

# the kernel's constants (checked against tg_debug_score_limits): genes of a strip, floats of the 16-byte path, rows of a slab,
# rows of a wave, slabs per round of tg_score_finish (its threads per gene), genes per workgroup of tg_score_finish
STRIP, VEC, SLAB, RPW, FIN_TPG, FIN_GENES = 256, 4, 64, 16, 16, 16
GENE_SIZES = (1, 3, 5, FIN_GENES + 1, STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 1)
SPOT_SIZES = (1, 2, 7, 9, RPW - 1, RPW + 1, SLAB - 1, SLAB, SLAB + 1, 3 * SLAB + 1, FIN_TPG * SLAB + 1)
FLOAT_CASES = [(SLAB + 1, STRIP + 1), (3 * SLAB + 1, 300), (FIN_TPG * SLAB + 1, 37)]
U53 = 2.0 ** -53


def score_bound(n_spots):
    return 2.0 * n_spots * 2.0 ** -52


def check_case_tables(device):
    lim = (ct.c_int32 * 6)()
    assert _capi.lib().tg_debug_score_limits(lim) == 0
    assert tuple(lim) == (STRIP, VEC, SLAB, RPW, FIN_TPG, FIN_GENES)
    assert {1, STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 1} <= set(GENE_SIZES)
    assert {1, 2, SLAB - 1, SLAB, SLAB + 1, 3 * SLAB + 1} <= set(SPOT_SIZES)
    assert max(SPOT_SIZES) > FIN_TPG * SLAB and -(-max(SPOT_SIZES) // SLAB) > FIN_TPG      # more slabs than one round of tg_score_finish
    assert any(n % VEC for n in GENE_SIZES) and any(RPW < n < SLAB and n % RPW for n in SPOT_SIZES)
    assert max(SPOT_SIZES) * 49 < 2 ** 16                                                  # the exactness argument above
    for aligned in (False, True):                                                          # the two layouts are what they claim to be
        for n in (1, 4, STRIP):
            a, b = planes(np.zeros((3, n), np.float32), np.zeros((3, n), np.float32), device, aligned)
            for v in (a, b):
                if aligned:
                    assert v.data_ptr() % 16 == 0 and v.stride(0) % VEC == 0
                else:
                    assert v.data_ptr() % 16 != 0 and v.stride(0) % 2 == 1
            assert a.stride(0) != b.stride(0)


def _np(t):
    return t.detach().cpu().numpy()


def _view(x, device, pitch, off):
    buf = torch.full((x.shape[0], pitch), float("nan"), dtype=torch.float32, device=device)
    buf[:, off:off + x.shape[1]] = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=device)
    return buf[:, off:off + x.shape[1]]


def planes(pred, meas, device, aligned):
    """The two planes as column ranges of NaN-filled buffers.  Odd: odd pitches (two different ones), the range starts at column 1
    (4 bytes off a 16-byte boundary).  Aligned: pitches multiples of 4, the range starts at column 4: the 16-byte loads run."""
    n = pred.shape[1]
    if aligned:
        n4 = -(-n // VEC) * VEC
        return _view(pred, device, n4 + 8, 4), _view(meas, device, n4 + 12, 4)
    odd = n + 3 if (n + 3) % 2 else n + 4
    return _view(pred, device, odd, 1), _view(meas, device, odd + 2, 1)


def raw_scores(pv, mv, want_moments=True, want_score=True):
    """tg_gene_scores on two device views -> (moments [3, n] or None, score [n] or None) as NumPy; outputs between sentinels."""
    from tangram_amd.preprocess import _stream
    lib = _capi.lib()
    dev = pv.device
    n_spots, n = (int(s) for s in pv.shape)
    nbytes = ct.c_size_t()
    _capi.check(lib.tg_gene_scores_query_bytes(n_spots, n, ct.byref(nbytes)))
    assert nbytes.value >= -(-n_spots // SLAB) * 3 * n * 8
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    mom = torch.full((3 * n + 2,), -7.0, dtype=torch.float64, device=dev)
    sc = torch.full((n + 2,), -7.0, dtype=torch.float64, device=dev)
    ld = lambda t: int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])              # noqa: E731
    _capi.check(lib.tg_gene_scores(pv.data_ptr(), ld(pv), mv.data_ptr(), ld(mv), n_spots, n, ws.data_ptr(),
                                   mom.data_ptr() + 8 if want_moments else None, sc.data_ptr() + 8 if want_score else None, _stream(dev)))
    mom, sc = _np(mom), _np(sc)
    assert mom[0] == mom[-1] == sc[0] == sc[-1] == -7.0, "a sentinel next to an output was overwritten"
    if not want_moments:
        assert (mom == -7.0).all(), "the moments were written although moments_out is NULL"
    if not want_score:
        assert (sc == -7.0).all(), "the scores were written although score_out is NULL"
    return (mom[1:-1].reshape(3, n) if want_moments else None), (sc[1:-1] if want_score else None)


def assert_same_bits(got, ref, where):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{where}: NaN pattern")
    np.testing.assert_array_equal(got[~nan].view(np.uint64), ref[~nan].view(np.uint64), err_msg=f"{where}: bits")


def definition64(pred, meas):
    """(moments, score) in NumPy float64 of the exact products (an exact data set: exact sums)."""
    p, m = pred.astype(np.float64), meas.astype(np.float64)
    mom = np.stack([(p * m).sum(axis=0), (p * p).sum(axis=0), (m * m).sum(axis=0)])
    with np.errstate(invalid="ignore", divide="ignore"):
        return mom, mom[0] / (np.sqrt(mom[1]) * np.sqrt(mom[2]))


def exact_planes(n_spots, n_genes, seed):
    rng = np.random.default_rng(seed)
    pred = (rng.integers(0, 8, size=(n_spots, n_genes)) * (rng.random((n_spots, n_genes)) < 0.6)).astype(np.float32)
    meas = (rng.integers(0, 8, size=(n_spots, n_genes)) * (rng.random((n_spots, n_genes)) < 0.6)).astype(np.float32)
    return pred, meas


def check_exact(device, n_spots, aligned):
    """Every gene width of the table at this height: moments and score bit for bit (all-zero columns included: NaN)."""
    for n in GENE_SIZES:
        pred, meas = exact_planes(n_spots, n, 100 * n_spots + n)
        mom_ref, sc_ref = definition64(pred, meas)
        mom, sc = raw_scores(*planes(pred, meas, device, aligned))
        where = f"{n_spots} spots x {n} genes, aligned={aligned}"
        assert_same_bits(mom, mom_ref, where + ": moments")
        assert_same_bits(sc, sc_ref, where + ": score")


def float_planes(n_spots, n_genes, seed, signed=False):
    rng = np.random.default_rng(seed)
    pred = rng.standard_normal((n_spots, n_genes)) * (rng.random((n_spots, n_genes)) < 0.3)
    meas = np.abs(rng.standard_normal((n_spots, n_genes))) * (rng.random((n_spots, n_genes)) < 0.3)
    return (pred if signed else np.abs(pred)).astype(np.float32), meas.astype(np.float32)


def assert_within_bounds(mom, sc, pred, meas, where):
    """The derived bounds of the module docstring; `sc` None: moments only."""
    n_spots = pred.shape[0]
    p, m = pred.astype(np.longdouble), meas.astype(np.longdouble)
    ref = np.stack([(p * m).sum(axis=0), (p * p).sum(axis=0), (m * m).sum(axis=0)])
    mag = np.stack([np.abs(p * m).sum(axis=0), (p * p).sum(axis=0), (m * m).sum(axis=0)])
    err = np.abs(mom.astype(np.longdouble) - ref).astype(np.float64)
    bound = (n_spots * U53 * mag).astype(np.float64)
    print(f"{where}: max moment error / bound {np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0)):.3f}")
    assert (err <= bound).all(), f"{where}: a moment is off by {err.max():.3e}"
    if sc is None:
        return
    with np.errstate(invalid="ignore", divide="ignore"):
        sc_ref = (ref[0] / (np.sqrt(ref[1]) * np.sqrt(ref[2]))).astype(np.float64)
    nan = np.isnan(sc_ref)
    np.testing.assert_array_equal(np.isnan(sc), nan, err_msg=f"{where}: NaN pattern of the score")
    d = np.abs(sc[~nan] - sc_ref[~nan])
    print(f"{where}: max |score - definition| {d.max() if d.size else 0.0:.3e}, bound {score_bound(n_spots):.3e}")
    assert (d <= score_bound(n_spots)).all(), f"{where}: score off by {d.max():.3e} > {score_bound(n_spots):.3e}"


def check_general_floats(device, n_spots, n_genes):
    for aligned in (False, True):
        pred, meas = float_planes(n_spots, n_genes, n_spots + n_genes)
        assert (pred >= 0).all() and (meas >= 0).all() and 0.6 < (pred == 0).mean() < 0.8
        mom, sc = raw_scores(*planes(pred, meas, device, aligned))
        assert_within_bounds(mom, sc, pred, meas, f"floats {n_spots} x {n_genes}, aligned={aligned}")
    pred, meas = float_planes(n_spots, n_genes, n_spots + n_genes + 1, signed=True)
    assert (pred < 0).any()
    mom, _ = raw_scores(*planes(pred, meas, device, False))
    assert_within_bounds(mom, None, pred, meas, f"sign-mixed pred {n_spots} x {n_genes}")


def check_position_independence(device, n_spots=3 * SLAB + 1):
    """One column: alone, as column 0 of a wide call, as the last column of an odd-width call (a second strip), as column 2 of a
    quad, under both layouts and in two calls: the same bits of all four numbers."""
    pred, meas = float_planes(n_spots, 300, 77)
    x, y = pred[:, 11].copy(), meas[:, 11].copy()
    assert np.count_nonzero(x * y) > 3
    seen = []
    for width, at in ((1, 0), (300, 0), (STRIP + 1, STRIP), (7, 2), (2 * STRIP + 1, STRIP - 1)):
        p, m = float_planes(n_spots, width, 1000 + width)
        p[:, at], m[:, at] = x, y
        for aligned in (False, True):
            pv, mv = planes(p, m, device, aligned)
            for call in range(2):
                mom, sc = raw_scores(pv, mv)
                seen.append((f"width {width}, column {at}, aligned={aligned}, call {call}", np.append(mom[:, at], sc[at])))
    assert_within_bounds(seen[0][1][:3, None], seen[0][1][3:], x[:, None], y[:, None], "the column alone")
    for where, v in seen[1:]:
        assert_same_bits(v, seen[0][1], f"{where} against {seen[0][0]}")


def check_degenerate_columns(device, n_spots=SLAB + 1, n=STRIP + 3):
    """All-zero measured / predicted columns score NaN (0 / 0) and leave every other gene's bits alone; each output works alone."""
    pred, meas = float_planes(n_spots, n, 5)
    pred[0], meas[0] = 1.0, 2.0                                       # no zero column to start with
    for aligned in (False, True):
        mom0, sc0 = raw_scores(*planes(pred, meas, device, aligned))
        assert not np.isnan(sc0).any()
        p, m = pred.copy(), meas.copy()
        zm, zp, both = (1, 4, STRIP), (2, STRIP - 1), (9,)
        m[:, list(zm + both)], p[:, list(zp + both)] = 0.0, 0.0
        mom, sc = raw_scores(*planes(p, m, device, aligned))
        dead = sorted(zm + zp + both)
        live = np.setdiff1d(np.arange(n), dead)
        assert np.isnan(sc[dead]).all(), "a zero norm must give 0 / 0 = NaN"
        assert (mom[0, dead] == 0).all() and (mom[2, list(zm + both)] == 0).all() and (mom[1, list(zp + both)] == 0).all()
        assert_same_bits(sc[live], sc0[live], "neighbours of the zero columns: score")
        assert_same_bits(mom[:, live], mom0[:, live], "neighbours of the zero columns: moments")
        only_m, none_s = raw_scores(*planes(p, m, device, aligned), want_score=False)
        none_m, only_s = raw_scores(*planes(p, m, device, aligned), want_moments=False)
        assert none_s is None and none_m is None
        assert_same_bits(only_m, mom, "moments alone")
        assert_same_bits(only_s, sc, "score alone")


def check_argument_errors(device):
    """Every invalid combination returns TG_ERR_INVALID -> ValueError with the library's message; a valid call afterwards is exact."""
    from tangram_amd.preprocess import _stream
    lib = _capi.lib()
    dev = torch.device(device)
    V, n = 70, 9
    p = torch.ones((V, n), dtype=torch.float32, device=dev)
    m = torch.ones((V, n), dtype=torch.float32, device=dev)
    nbytes = ct.c_size_t()
    _capi.check(lib.tg_gene_scores_query_bytes(V, n, ct.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    mom = torch.zeros((3, n), dtype=torch.float64, device=dev)
    sc = torch.zeros(n, dtype=torch.float64, device=dev)
    st = _stream(dev)
    P, M, W, MO, SC = p.data_ptr(), m.data_ptr(), ws.data_ptr(), mom.data_ptr(), sc.data_ptr()

    def refused(msg, fn, *args):
        with pytest.raises(ValueError, match=msg):
            _capi.check(fn(*args))

    refused("NULL", lib.tg_gene_scores_query_bytes, V, n, None)
    refused("NULL", lib.tg_gene_scores, None, n, M, n, V, n, W, MO, SC, st)
    refused("NULL", lib.tg_gene_scores, P, n, None, n, V, n, W, MO, SC, st)
    refused("NULL", lib.tg_gene_scores, P, n, M, n, V, n, None, MO, SC, st)
    refused("every output is NULL", lib.tg_gene_scores, P, n, M, n, V, n, W, None, None, st)
    for bad_v, bad_n in ((0, n), (-1, n), (V, 0), (V, -2)):
        refused("at least one", lib.tg_gene_scores_query_bytes, bad_v, bad_n, ct.byref(nbytes))
        refused("at least one", lib.tg_gene_scores, P, n, M, n, bad_v, bad_n, W, MO, SC, st)
    refused("pitch", lib.tg_gene_scores, P, n - 1, M, n, V, n, W, MO, SC, st)
    refused("pitch", lib.tg_gene_scores, P, n, M, n - 1, V, n, W, MO, SC, st)
    for big_v, big_n in ((2 ** 31, n), (2 ** 31 - 1, n), (2 ** 40, n), (V, 2 ** 31 - 1), (2 ** 30, 2 ** 30)):
        refused("32-bit", lib.tg_gene_scores_query_bytes, big_v, big_n, ct.byref(nbytes))
        refused("32-bit", lib.tg_gene_scores, P, big_n, M, big_n, big_v, big_n, W, MO, SC, st)
    _capi.check(lib.tg_gene_scores(P, n, M, n, V, n, W, MO, SC, st))
    np.testing.assert_array_equal(_np(mom), np.full((3, n), float(V)))
    np.testing.assert_array_equal(_np(sc), np.ones(n))
    # ... and the Python seam
    import tangram_amd as tg
    with pytest.raises(ValueError, match="same shape"):
        tg.gene_scores(np.ones((V, n), np.float32), np.ones((V, n + 1), np.float32), device=device)
    s, mo = tg.gene_scores(np.ones((V, n), np.float32), p, moments=True, device=device)
    assert s.dtype == torch.float64 and tuple(mo.shape) == (3, n) and (_np(s) == 1.0).all() and (_np(mo) == V).all()
    assert_same_bits(_np(tg.gene_scores(p.t().contiguous().t(), m, device=device)), np.ones(n), "a column-major argument")


# ------------------------------------------------------------------------------------------------------------------------------
# the public surface: compare_spatial_geneexp, score_genes
# ------------------------------------------------------------------------------------------------------------------------------
def make_adatas(C, n_train, V, n_overlap, seed, sparse=False, extra_sc=4):
    """AnnDataLite pair as pp_adatas leaves it: `n_overlap` shared genes (the first `n_train` train), `extra_sc` genes only in
    adata_sc (one of them all zero: project_genes filters it), 3 genes only in adata_sp; the shared genes in different orders."""
    from oracle import tangram_oracle as orc
    from tangram_amd.anndata_lite import AnnDataLite
    data = orc.make_synthetic(C, n_overlap + extra_sc, V, seed=seed)
    rng = np.random.default_rng(seed)
    S, G = data["S"].copy(), data["G"].copy()
    if extra_sc:
        S[:, n_overlap] = 0.0
    shared = [f"g{i}" for i in range(n_overlap)]
    sc_genes = shared + [f"only_sc{i}" for i in range(extra_sc)]
    sp_perm = rng.permutation(n_overlap)
    sp_genes = [shared[i] for i in sp_perm] + ["only_sp0", "only_sp1", "only_sp2"]
    G_sp = np.concatenate([G[:, sp_perm], rng.poisson(0.3, size=(V, 3)).astype(np.float32)], axis=1)
    obs_sc = pd.DataFrame({"subclass_label": rng.choice(["a", "b", "c"], size=C)}, index=[f"c{i}" for i in range(C)])
    obs_sp = pd.DataFrame({"rna_count_based_density": G.sum(1) / G.sum(), "uniform_density": np.ones(V) / V}, index=[f"s{i}" for i in range(V)])
    wrap = (lambda a: sp.csr_matrix(a)) if sparse else (lambda a: a)
    ad_sc = AnnDataLite(wrap(S), obs=obs_sc, var=pd.DataFrame(index=sc_genes))
    ad_sp = AnnDataLite(wrap(G_sp), obs=obs_sp, var=pd.DataFrame(index=sp_genes))
    for ad in (ad_sc, ad_sp):
        ad.uns["training_genes"] = shared[:n_train]
        ad.uns["overlap_genes"] = list(shared)
    return ad_sc, ad_sp


def _dense(X):
    return np.asarray(X.todense() if sp.issparse(X) else X, dtype=np.float32)


def host_scores(pred, meas):
    """The float64 definition on float32 planes, sums in extended precision."""
    p, m = pred.astype(np.longdouble), meas.astype(np.longdouble)
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((p * m).sum(axis=0) / (np.sqrt((p * p).sum(axis=0)) * np.sqrt((m * m).sum(axis=0)))).astype(np.float64)


def assert_scores_close(got, ref, bound, where):
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{where}: NaN pattern")
    d = np.abs(np.asarray(got)[~nan] - ref[~nan]).max() if (~nan).any() else 0.0
    print(f"{where}: max |score difference| {d:.3e}, bound {bound:.3e}")
    assert d <= bound, f"{where}: {d:.3e} > {bound:.3e}"
    return d


def check_compare_surface(device, sparse):
    import tangram_amd as tg
    from tangram_amd.anndata_lite import AnnDataLite
    C, V, n_overlap = 40, 70, 23
    ad_sc, ad_sp = make_adatas(C, 9, V, n_overlap, seed=4, sparse=sparse)
    rng = np.random.default_rng(1)
    ge_genes = list(ad_sc.var.index)
    ge_X = (np.abs(rng.standard_normal((V, len(ge_genes)))) * (rng.random((V, len(ge_genes))) < 0.5)).astype(np.float32)
    ge_X[:, 3] = 0.0                                                   # a gene that was never projected: NaN, sorted last
    var_ge = pd.DataFrame({"is_training": np.isin(ge_genes, ad_sc.uns["training_genes"])}, index=ge_genes)
    ad_ge = AnnDataLite(sp.csr_matrix(ge_X) if sparse else ge_X, obs=ad_sp.obs, var=var_ge, uns=ad_sc.uns)
    genes = list(ad_sp.uns["overlap_genes"])

    def reference_scores(names):
        a = ge_X[:, ad_ge.var.index.get_indexer(names)]
        b = _dense(ad_sp.X)[:, ad_sp.var.index.get_indexer(names)]
        return host_scores(a, b)

    df = tg.compare_spatial_geneexp(ad_ge, ad_sp, device=device, gene_block=8)           # 23 genes: blocks of 8, 8, 7
    assert list(df.columns) == ["score", "is_training", "sparsity_sp"] and sorted(df.index) == sorted(genes)
    assert_scores_close(df.loc[genes, "score"].to_numpy(), reference_scores(genes), score_bound(V), f"compare, sparse={sparse}")
    finite = df["score"].to_numpy()[~np.isnan(df["score"].to_numpy())]
    assert (np.diff(finite) <= 0).all() and np.isnan(df["score"].to_numpy()[-1]) and df.index[-1] == "g3"
    assert df["is_training"].sum() == 9 and set(df.index[df["is_training"]]) == set(ad_sc.uns["training_genes"])
    np.testing.assert_array_equal(df.loc[genes, "sparsity_sp"].to_numpy(),
                                  1 - (_dense(ad_sp.X)[:, ad_sp.var.index.get_indexer(genes)] != 0).sum(axis=0) / V)
    one_block = tg.compare_spatial_geneexp(ad_ge, ad_sp, device=device)
    assert_same_bits(one_block.loc[genes, "score"].to_numpy(), df.loc[genes, "score"].to_numpy(), "one block against blocks of 8")
    full = tg.compare_spatial_geneexp(ad_ge, ad_sp, ad_sc, device=device)
    assert list(full.columns) == ["score", "is_training", "sparsity_sp", "sparsity_sc", "sparsity_diff"]
    np.testing.assert_array_equal(full.loc[genes, "sparsity_sc"].to_numpy(),
                                  1 - (_dense(ad_sc.X)[:, ad_sc.var.index.get_indexer(genes)] != 0).sum(axis=0) / C)
    np.testing.assert_array_equal(full["sparsity_diff"].to_numpy(), (full["sparsity_sp"] - full["sparsity_sc"]).to_numpy())
    subset = ["g7", "g0", "g12", "g5"]
    sub = tg.compare_spatial_geneexp(ad_ge, ad_sp, ad_sc, genes=subset, device=device)
    assert sorted(sub.index) == sorted(subset) and len(sub) == 4 and (np.diff(sub["score"].to_numpy()) <= 0).all()
    assert_same_bits(sub.loc[subset, "score"].to_numpy(), df.loc[subset, "score"].to_numpy(), "the genes= subset")
    # ... and what is refused
    lame = AnnDataLite(ad_sp.X, obs=ad_sp.obs, var=ad_sp.var, uns={"training_genes": []})
    with pytest.raises(ValueError, match=r"Missing tangram parameters. Run `pp_adatas\(\)`."):
        tg.compare_spatial_geneexp(ad_ge, lame, device=device)
    with pytest.raises(ValueError, match=r"Missing tangram parameters. Use `project_genes\(\)` to get adata_ge."):
        tg.compare_spatial_geneexp(AnnDataLite(ad_ge.X, obs=ad_ge.obs, var=ad_ge.var, uns={}), ad_sp, device=device)
    with pytest.raises(ValueError, match=r"Missing tangram parameters. Run `pp_adatas\(\)`."):
        tg.compare_spatial_geneexp(ad_ge, ad_sp, AnnDataLite(ad_sc.X, obs=ad_sc.obs, var=ad_sc.var, uns={}), device=device)
    other = dict(ad_sc.uns, overlap_genes=genes[:-1])
    with pytest.raises(AssertionError):
        tg.compare_spatial_geneexp(AnnDataLite(ad_ge.X, obs=ad_ge.obs, var=ad_ge.var, uns=other), ad_sp, device=device)
    with pytest.raises(AssertionError):
        tg.compare_spatial_geneexp(ad_ge, ad_sp, AnnDataLite(ad_sc.X, obs=ad_sc.obs, var=ad_sc.var, uns=other), device=device)


TIE = dict(C=300, n_train=40, V=257, n_overlap=90, epochs=4, gene_block=32)      # 90 genes in blocks of 32, 32, 26
# the dense route projects through an engine of ONE gene column, i.e. one GEMM pass per gene: fewer genes, the same three blocks + a rest
TIE_DENSE = dict(C=100, n_train=8, V=65, n_overlap=14, epochs=4, gene_block=4)
TIE_ROUTES = ("mapper", "constrained", "dense", "truncated")
GHAT_TOL = 1e-4                                                                  # split-bf16 tolerance of Ghat
_mapped = {}


def tie_of(route):
    return TIE_DENSE if route == "dense" else TIE


def mapped(device, route):
    """(adata_map, fresh adata_sc, fresh adata_sp, keyword arguments of the route), mapped once per route and device."""
    import tangram_amd as tg
    key = (str(device), route)
    T = tie_of(route)
    if key not in _mapped:
        ad_sc, ad_sp = make_adatas(T["C"], T["n_train"], T["V"], T["n_overlap"], seed=11, sparse=route == "truncated")
        kw = dict(device=device, num_epochs=T["epochs"], random_state=42, verbose=False)
        if route == "constrained":
            ad_map = tg.map_cells_to_space(ad_sc, ad_sp, mode="constrained", target_count=200, lambda_f_reg=1, lambda_count=1,
                                           keep_mapper=True, **kw)
        elif route == "truncated":
            ad_map = tg.map_cells_to_space(ad_sc, ad_sp, top_k=6, **kw)
        else:
            ad_map = tg.map_cells_to_space(ad_sc, ad_sp, keep_mapper=route == "mapper", **kw)
        _mapped[key] = ad_map
    ad_sc, ad_sp = make_adatas(T["C"], T["n_train"], T["V"], T["n_overlap"], seed=11, sparse=route == "truncated")
    ad_map = _mapped[key]
    kw = dict(device=device)
    if route in ("mapper", "constrained"):
        kw["mapper"] = ad_map._tangram_amd_mapper
    if route == "truncated":
        kw["truncated"] = True
    return ad_map, ad_sc, ad_sp, kw


def blockwise_host_scores(device, route, ad_map, ad_sc, ad_sp, genes, gene_block):
    """The same per-block projection calls as score_genes makes -- same route, same blocks -- scored in float64 on the host."""
    from tangram_amd import utils
    S = _dense(ad_sc.X)
    cols_sc = pd.Index([g.lower() for g in ad_sc.var.index]).get_indexer(genes)
    G = _dense(ad_sp.X)[:, ad_sp.var.index.get_indexer(genes)]
    dev = torch.device(device)
    engine = sm = None
    if route == "dense":
        engine, rows = utils._projection_engine(ad_map, dev, "bf16x3")
        assert np.abs(rows - 1.0).max() <= 1e-6
    if route == "truncated":
        from tangram_amd import SparseMap
        sm = SparseMap(ad_map.X, device, n_cells=S.shape[0])
    out = []
    for k0 in range(0, len(genes), gene_block):
        blk = torch.as_tensor(np.ascontiguousarray(S[:, cols_sc[k0:k0 + gene_block]]), device=dev)
        if route == "mapper":
            pred = ad_map._tangram_amd_mapper.project_genes_device(blk)
        elif route == "constrained":
            pred = ad_map._tangram_amd_mapper.project_genes_device(blk, unfiltered=True)
        elif route == "dense":
            pred = engine.project_genes(blk, unfiltered=True)
        else:
            pred = sm.project_into(blk, torch.empty((sm.n_spots, blk.shape[1]), dtype=torch.float32, device=sm.device))
        out.append(host_scores(_np(pred), G[:, k0:k0 + gene_block]))
    if engine is not None:
        engine.release()
    return np.concatenate(out)


def check_score_genes_tie(device, route):
    """score_genes against (a) its own block projections scored on the host: the derived bound; (b) the full route
    compare_spatial_geneexp(project_genes(...)): the same index, columns and is_training, scores within the split-bf16 tolerance."""
    import tangram_amd as tg
    ad_map, ad_sc, ad_sp, kw = mapped(device, route)
    genes = list(ad_sp.uns["overlap_genes"])
    T = tie_of(route)
    gb = T["gene_block"]
    assert len(genes) % gb != 0 and len(genes) > 2 * gb
    df = tg.score_genes(ad_map, ad_sc, ad_sp, gene_block=gb, **kw)
    assert "only_sc0" not in df.index and len(df) == len(genes)
    ref = blockwise_host_scores(device, route, ad_map, ad_sc, ad_sp, genes, gb)
    assert_scores_close(df.loc[genes, "score"].to_numpy(), ref, score_bound(T["V"]), f"score_genes[{route}] against its own blocks")
    # the full route on fresh inputs
    _, ad_sc2, ad_sp2, _ = mapped(device, route)
    full = tg.compare_spatial_geneexp(tg.project_genes(ad_map, ad_sc2, **kw), ad_sp2, ad_sc2, device=device)
    assert list(df.columns) == list(full.columns) == ["score", "is_training", "sparsity_sp", "sparsity_sc", "sparsity_diff"]
    assert sorted(df.index) == sorted(full.index)
    for col in ("is_training", "sparsity_sp", "sparsity_sc", "sparsity_diff"):
        np.testing.assert_array_equal(df.loc[genes, col].to_numpy(), full.loc[genes, col].to_numpy(), err_msg=col)
    assert df["is_training"].sum() == T["n_train"]
    d = assert_scores_close(df.loc[genes, "score"].to_numpy(), full.loc[genes, "score"].to_numpy(), GHAT_TOL,
                            f"score_genes[{route}] against compare_spatial_geneexp(project_genes(...))")
    if d == 0.0 or route == "truncated":                               # the same kernels on the same columns: the order of the frame too
        assert list(df.index) == list(full.index)
    assert (np.diff(df["score"].to_numpy()) <= 0).all()
    # genes=: a subset in the caller's order, one short block
    subset = [genes[len(genes) // 2], genes[3], genes[-2]]
    sub = tg.score_genes(ad_map, mapped(device, route)[1], ad_sp, genes=subset, gene_block=2, **kw)
    assert sorted(sub.index) == sorted(subset)
    assert_same_bits(sub.loc[subset, "score"].to_numpy(), df.loc[subset, "score"].to_numpy(), f"score_genes[{route}](genes=...)")
    return d


def check_score_genes_refusals(device):
    import tangram_amd as tg
    dense, ad_sc, ad_sp, kw_m = mapped(device, "mapper")
    top, ad_sc_t, ad_sp_t, _ = mapped(device, "truncated")
    with pytest.raises(ValueError, match="sparse adata_map.X"):
        tg.score_genes(dense, ad_sc, ad_sp, truncated=True, device=device)
    with pytest.raises(ValueError, match="mapper="):
        tg.score_genes(top, ad_sc_t, ad_sp_t, truncated=True, mapper=kw_m["mapper"], device=device)
    with pytest.raises(ValueError, match=r"mapper=adata_map\._tangram_amd_mapper"):
        tg.score_genes(top, ad_sc_t, ad_sp_t, device=device)

    class Sharded:                                                     # what score_genes looks at before it touches the mapper
        _sharded = object()
        _engine = None
    with pytest.raises(ValueError, match="spot-sharded"):
        tg.score_genes(dense, ad_sc, ad_sp, mapper=Sharded(), device=device)
    from tangram_amd.anndata_lite import AnnDataLite
    short = AnnDataLite(ad_sc.X[:-1], obs=ad_sc.obs.iloc[:-1], var=ad_sc.var.copy(), uns=ad_sc.uns)
    with pytest.raises(ValueError, match="same `obs` index"):
        tg.score_genes(dense, short, ad_sp, device=device)
    with pytest.raises(ValueError, match=r"Run `pp_adatas\(\)`"):
        tg.score_genes(dense, ad_sc, AnnDataLite(ad_sp.X, obs=ad_sp.obs, var=ad_sp.var, uns={}), device=device)


# the reference's test_train_score_match (tests/tangram_test.py:159-210) on synthetic data: lambda_g1 = 1, every other term off
INVARIANT = dict(C=30, n_train=8, V=12, n_overlap=12, seed=3, epochs=100, lr=0.1, random_state=42)


def invariant_adatas():
    v = INVARIANT
    return make_adatas(v["C"], v["n_train"], v["V"], v["n_overlap"], seed=v["seed"])


def check_reference_invariant():
    """The unmodified reference loop (oracle.torch_port, pinned to the reference by tests/test_oracle_golden.py) holds the invariant on
    this data and epoch count by itself, with room on both sides of the rounding."""
    from oracle import tangram_oracle as orc
    from oracle.torch_port import TorchPortMapper
    v = INVARIANT
    ad_sc, ad_sp = invariant_adatas()
    train = ad_sc.uns["training_genes"]
    S = _dense(ad_sc.X)[:, ad_sc.var.index.get_indexer(train)]
    G = _dense(ad_sp.X)[:, ad_sp.var.index.get_indexer(train)]
    M0 = orc.reference_init_M(v["C"], v["V"], v["random_state"])
    P, hist = TorchPortMapper(S, G, lambda_g1=1.0, M0=M0).train(v["epochs"], v["lr"])
    score = host_scores((P.T @ S).astype(np.float32), G).mean()
    last = float(hist["main_loss"][-1])
    print(f"reference: mean training score {score:.6f}, main_loss[-1] {last:.6f}")
    assert round(score, 3) == round(last, 3)
    assert abs(score - last) < 1e-4 and 0.15 < (last * 1000) % 1 < 0.85, "too close to a rounding boundary to carry the test"
    return last


def check_train_score_invariant(device):
    import tangram_amd as tg
    v = INVARIANT
    ad_sc, ad_sp = invariant_adatas()
    ad_map = tg.map_cells_to_space(ad_sc, ad_sp, mode="cells", density_prior=None, lambda_d=0, lambda_g1=1, lambda_g2=0, device=device,
                                   num_epochs=v["epochs"], learning_rate=v["lr"], random_state=v["random_state"], verbose=False, keep_mapper=True)
    df = tg.score_genes(ad_map, ad_sc, ad_sp, mapper=ad_map._tangram_amd_mapper, device=device)
    ad_map._tangram_amd_mapper.release()
    score = float(df[df["is_training"]]["score"].mean())
    last = float(list(ad_map.uns["training_history"]["main_loss"])[-1])
    print(f"mean training score {score:.6f}, main_loss[-1] {last:.6f}")
    assert df["is_training"].sum() == v["n_train"]
    assert round(score, 3) == round(last, 3)


# ------------------------------------------------------------------------------------------------------------------------------
# project_genes' routes: one statement of the rules, one CSR upload, one rescaling
# ------------------------------------------------------------------------------------------------------------------------------
ROUTE_ERRORS = {       # the texts as the routes were first written, not read from the code under test
    "truncated with mapper=": "truncated=True projects the sparse adata_map.X itself: it cannot be combined with mapper=",
    "truncated with a dense X": "truncated=True needs a sparse adata_map.X (the top_k= result); a dense mapping is projected without it",
    "sparse X without a mapper": "adata_map.X is sparse (map_cells_to_space(..., top_k=k) keeps each cell's k most probable spots only): "
                                 "project with the trained mapping instead -- map with keep_mapper=True and pass "
                                 "mapper=adata_map._tangram_amd_mapper -- or project the truncated matrix itself with truncated=True",
    "obs index mismatch": "The two AnnDatas need to have same `obs` index.",
}


def check_route_errors(device):
    """project_genes and score_genes refuse the same four situations with the same words."""
    import tangram_amd as tg
    from tangram_amd.anndata_lite import AnnDataLite
    dense, _, _, kw_m = mapped(device, "mapper")
    top = mapped(device, "truncated")[0]

    def short(ad):
        return AnnDataLite(ad.X[:-1], obs=ad.obs.iloc[:-1], var=ad.var.copy(), uns=ad.uns)

    cases = {"truncated with mapper=": ("truncated", dict(truncated=True, mapper=kw_m["mapper"]), False),
             "truncated with a dense X": ("mapper", dict(truncated=True), False),
             "sparse X without a mapper": ("truncated", {}, False),
             "obs index mismatch": ("mapper", {}, True)}
    assert set(cases) == set(ROUTE_ERRORS)
    for what, (route, kw, cut) in cases.items():
        ad_map = top if route == "truncated" else dense
        for fn in ("project_genes", "score_genes"):
            _, ad_sc, ad_sp, _ = mapped(device, route)
            ad_sc = short(ad_sc) if cut else ad_sc
            args = (ad_map, ad_sc) + ((ad_sp,) if fn == "score_genes" else ())
            with pytest.raises(ValueError) as e:
                getattr(tg, fn)(*args, device=device, **kw)
            assert str(e.value) == ROUTE_ERRORS[what], f"{fn}, {what}"


def check_all_zero_sparse_block(device):
    """An all-zero scipy-sparse block of adata_sc.X (empty index and data arrays) through the three users of the CSR upload: zeros,
    and no complaint of the library about a NULL array."""
    from tangram_amd import SparseMap
    from tangram_amd.engine import HipMapperEngine
    from tangram_amd.gene_score import GeneBlocks
    C, V, K, n = 37, 21, 3, 7                                          # 7 genes: the engine expands blocks of K = 3, 3, 1
    rng = np.random.default_rng(5)
    Z = sp.csr_matrix((C, n), dtype=np.float32)
    assert Z.nnz == 0 and Z.data.size == 0
    eng = HipMapperEngine(rng.random((C, K), dtype=np.float32), rng.random((V, K), dtype=np.float32),
                          rng.standard_normal((C, V)).astype(np.float32), device=device)
    out = _np(eng.project_genes(Z))
    eng.release()
    assert out.shape == (V, n) and not out.any(), "HipMapperEngine.project_genes"
    X = sp.random(C, V, density=0.2, random_state=3, format="csr", dtype=np.float32)
    out = _np(SparseMap(X, device).project(Z))
    assert out.shape == (V, n) and not out.any(), "SparseMap.project"
    buf = torch.full((C, 5), 7.0, dtype=torch.float32, device=torch.device(device))
    view = GeneBlocks(Z, np.arange(n), device).fill(2, 4, buf)
    assert tuple(view.shape) == (C, 4) and not _np(view).any() and (_np(buf)[:, 4] == 7.0).all(), "GeneBlocks.fill"


def check_unnormalised_dense_mapping(device, golden_dir):
    """A dense adata_map.X whose rows sum to 0.5 .. 2 (P^T S = (P / r)^T (r S)): a dense host S, a scipy-sparse S and a device block
    give the same bits.  The stored array is project_genes of the commit before the routes were merged, on the emulator: the
    emulator reproduces its bits.  The GPU multiplies in another order: both are within 2^-14 |P|^T |S| of the exact product (bf16x3
    keeps 16 significand bits of either operand and drops the low x low product: 3 x 2^-16 per product; 40 fp32 additions, 2^-24
    each, and the fp32 exp / log of softmax(log P) fit in the remaining 2^-16), so they are within 2^-13 |P|^T |S| of each other."""
    import os
    import tangram_amd as tg
    from tangram_amd import utils
    from tangram_amd.anndata_lite import AnnDataLite
    z = np.load(os.path.join(golden_dir, "unnormalised_dense_projection.npz"))
    P, S, want = z["P"], z["S"], z["X_space"]
    rows = P.sum(axis=1)
    assert rows.min() < 0.7 and rows.max() > 1.5
    C, V = P.shape
    n = S.shape[1]
    genes, cells = [f"g{i}" for i in range(n)], [f"c{i}" for i in range(C)]
    got = {}
    for form in ("dense host S", "scipy-sparse S"):
        ad_map = AnnDataLite(P.copy(), obs=pd.DataFrame(index=cells), var=pd.DataFrame(index=[f"s{i}" for i in range(V)]),
                             uns={"train_genes_df": pd.DataFrame(index=genes[:4])})
        ad_sc = AnnDataLite(sp.csr_matrix(S) if form.startswith("scipy") else S.copy(), obs=pd.DataFrame(index=cells),
                            var=pd.DataFrame(index=genes))
        got[form] = np.asarray(tg.project_genes(ad_map, ad_sc, device=device).X)
    route = utils._Route(ad_map, C, None, False, device, "bf16x3")
    try:
        got["device block"] = _np(route.project(torch.as_tensor(S, device=torch.device(device))))
    finally:
        route.release()
    for form, x in got.items():
        assert x.dtype == np.float32 and x.shape == want.shape
        np.testing.assert_array_equal(x.view(np.uint32), got["dense host S"].view(np.uint32), err_msg=f"{form} against the dense host S")
    x = got["dense host S"]
    if torch.device(device).type == "cpu":
        np.testing.assert_array_equal(x.view(np.uint32), want.view(np.uint32), err_msg="against the stored projection")
    else:
        bound = 2.0 ** -13 * (np.abs(P.astype(np.float64)).T @ np.abs(S.astype(np.float64)))
        err = np.abs(x.astype(np.float64) - want)
        print(f"unnormalised dense mapping: max error / bound against the stored projection {(err / bound).max():.4f}")
        assert (err <= bound).all()
