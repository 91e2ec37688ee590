"""Tables and checks of the sparse projection path (tg_sparse.h: tg_sp_count / _scan / _scatter / _order, tg_sp_project;
tg_sparse_map_query_bytes / _build / _project; tangram_amd.SparseMap / project_sparse; project_genes(truncated=True)), shared by
tests/test_sparse_project.py (emulator, device "cpu") and tests/test_gpu_sparse_project.py (MI355X).

EXACT cases carry no tolerance: the entries of X are multiples of 2^-10 in [0, 1], S holds integers in [0, 7], a spot has at most
1 500 entries, so every partial sum is a multiple of 2^-10 below 1 500 * 7 < 2^14 -- 24 bits, exactly representable in fp32 -- and
the result must be the float64 product cast to float32, bit for bit.  `out` is a column range of a wider NaN-filled buffer: an
element nobody wrote, and a write outside the range, both show.

Every pattern of PATTERNS is projected at three gene widths of GENE_WIDTHS, rotating through the list (each width meets several
patterns of every kind), once with an odd pitch and offset (scalar loads and stores) -- and the two patterns of WIDTH_PATTERNS at
EVERY width, with the odd and with the 16-byte aligned layout.  The image is built once per pattern.

GENERAL floats are held to the standard bound of a length-n fma chain, |out - ref| <= gamma_n * sum |p s| with gamma_n =
n u / (1 - n u), u = 2^-24 and n the number of entries of that spot: derived, not measured (a term left out or taken twice
breaks it by orders of magnitude)."""
import ctypes as ct

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tangram_amd import _capi

U = 2.0 ** -24
GENE_WIDTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025)
LAM = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5)

# (kind, C, V, k)
K_PATTERNS = sorted({("k", C, V, min(k, V)) for C in (1, 3, 40, 300) for V in (1, 2, 63, 64, 65, 257) for k in (1, 4, min(V, 64))})
HUB_PATTERNS = [("hub", 300, 65, 0), ("hub", 1500, 65, 0)]              # spot 64 holds every cell: > 256 threads, > 1 024 of the LDS tile
PATTERNS = K_PATTERNS + HUB_PATTERNS + [("three-spots", 40, 1025, 0), ("ragged", 40, 65, 0), ("empty", 40, 65, 0)]
WIDTH_PATTERNS = [("ragged", 40, 65, 0), ("k", 40, 65, 4)]
IMAGE_PATTERNS = HUB_PATTERNS + [("ragged", 40, 65, 0)]
FLOAT_CASES = [(C, V) for C in (40, 300) for V in (65, 257)]           # k = 7, 3 steps
SPLITS = (1, 5, 256)
REPRO_GENES = 300


def check_case_tables():
    ks = {(C, V, k) for kind, C, V, k in PATTERNS if kind == "k"}
    for C in (1, 3, 40, 300):
        for V in (1, 2, 63, 64, 65, 257):
            assert {(C, V, min(1, V)), (C, V, min(4, V)), (C, V, min(V, 64))} <= ks, (C, V)
    assert ("hub", 300, 65, 0) in PATTERNS and ("hub", 1500, 65, 0) in PATTERNS
    assert ("three-spots", 40, 1025, 0) in PATTERNS and ("ragged", 40, 65, 0) in PATTERNS and ("empty", 40, 65, 0) in PATTERNS
    assert set(GENE_WIDTHS) == {1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025}
    assert all(p in PATTERNS for p in WIDTH_PATTERNS + IMAGE_PATTERNS) and len(WIDTH_PATTERNS) >= 1
    seen = {}
    for i, p in enumerate(PATTERNS):                                    # the rotation reaches every width from every kind with entries
        for n in widths_of(i):
            seen.setdefault(n, set()).add(p[0])
    assert all(seen[n] >= {"k"} for n in GENE_WIDTHS) and set(seen) == set(GENE_WIDTHS)
    assert max(C for _, C, _, _ in PATTERNS) <= 1500                    # the exactness argument above
    assert set(FLOAT_CASES) == {(40, 65), (40, 257), (300, 65), (300, 257)} and set(SPLITS) == {1, 5, 256} and REPRO_GENES > 256
    x = make_pattern(("hub", 1500, 65, 0))
    assert np.diff(x.tocsc().indptr)[64] == 1500 > 1024
    x = make_pattern(("three-spots", 40, 1025, 0))
    assert set(np.unique(x.indices)) == {0, 512, 1024}
    x = make_pattern(("ragged", 40, 65, 0))
    per_row = np.diff(x.indptr)
    assert per_row.min() == 0 and per_row.max() == 65 and len(set(per_row)) > 5
    assert make_pattern(("empty", 40, 65, 0)).nnz == 0


def widths_of(i):
    return [GENE_WIDTHS[(3 * i + j) % len(GENE_WIDTHS)] for j in range(3)]


def _exact_values(rng, n):
    return (rng.integers(0, 1025, size=n) / 1024.0).astype(np.float32)


def make_pattern(p):
    """A canonical float32 CSR matrix [C, V] with entries that are multiples of 2^-10 in [0, 1]."""
    kind, C, V, k = p
    rng = np.random.default_rng(7919 * C + 31 * V + k + len(kind))
    if kind == "k":
        cols = [np.sort(rng.choice(V, size=k, replace=False)) for _ in range(C)]
    elif kind == "hub":
        cols = [np.sort(np.append(rng.choice(V - 1, size=2, replace=False), V - 1)) for _ in range(C)]
    elif kind == "three-spots":
        spots = np.array([0, V // 2, V - 1])
        cols = [spots[rng.random(3) < 0.6] for _ in range(C)]
        cols[0], cols[1] = spots, spots[:0]
    elif kind == "ragged":
        m = sp.random(C, V, density=0.3, random_state=np.random.RandomState(5), format="csr")
        cols = [np.sort(m.indices[m.indptr[c]:m.indptr[c + 1]]) for c in range(C)]
        cols[0], cols[1], cols[C - 1] = np.arange(0), np.arange(V), np.arange(V)        # an empty row, full rows (the last one too)
        cols[7] = np.arange(0)
    elif kind == "empty":
        cols = [np.arange(0) for _ in range(C)]
    else:
        raise ValueError(kind)
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    indices = np.concatenate(cols).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
    x = sp.csr_matrix((_exact_values(rng, len(indices)), indices, indptr), shape=(C, V))
    assert x.has_canonical_format
    return x


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def layouts(S, V, device, aligned):
    """(S view with a pitch, out view inside a NaN-filled wider buffer, that buffer, the view's first column).  Odd: pitch n + 3,
    out at column 1 of n + 5.  Aligned: pitches multiples of 4, out at column 4: the 16-byte accesses run."""
    C, n = S.shape
    n4 = -(-n // 4) * 4
    pitch, width, off = (n4 + 4, n4 + 8, 4) if aligned else (n + 3, n + 5, 1)
    sbuf = torch.full((C, pitch), float("nan"), dtype=torch.float32, device=device)
    sbuf[:, :n] = torch.as_tensor(S, device=device)
    wide = torch.full((V, width), float("nan"), dtype=torch.float32, device=device)
    s_view, o_view = sbuf[:, :n], wide[:, off:off + n]
    if aligned:
        assert s_view.data_ptr() % 16 == 0 and o_view.data_ptr() % 16 == 0 and s_view.stride(0) % 4 == 0 and o_view.stride(0) % 4 == 0
    else:
        assert o_view.data_ptr() % 16 != 0
    return s_view, o_view, wide, off


def project_exact(sm, X, n_genes, aligned, where):
    rng = np.random.default_rng(1000 * n_genes + X.shape[0] + int(aligned))
    C, V = X.shape
    S = rng.integers(0, 8, size=(C, n_genes)).astype(np.float32)
    ref = np.asarray(X.astype(np.float64).T @ S.astype(np.float64)).astype(np.float32)
    s_view, o_view, wide, off = layouts(S, V, sm.device, aligned)
    sm.project_into(s_view, o_view)
    got = _np(wide)
    assert not np.isnan(got[:, off:off + n_genes]).any(), f"{where}: an element of out was not written"
    np.testing.assert_array_equal(_bits(got[:, off:off + n_genes]), _bits(ref), err_msg=f"{where}: bits of out against the float64 product")
    assert np.isnan(got[:, :off]).all() and np.isnan(got[:, off + n_genes:]).all(), f"{where}: a column outside the range was written"


def check_exact_pattern(device, i):
    from tangram_amd import SparseMap
    p = PATTERNS[i]
    X = make_pattern(p)
    sm = SparseMap(X, device)
    for n in widths_of(i):
        project_exact(sm, X, n, False, f"{p} n_genes={n}")


def check_exact_widths(device, p, aligned):
    from tangram_amd import SparseMap
    X = make_pattern(p)
    sm = SparseMap(X, device)
    for n in GENE_WIDTHS:
        project_exact(sm, X, n, aligned, f"{p} n_genes={n} aligned={aligned}")


def check_image_order(device, p):
    """spot_ptr = cumulative column counts; inside a spot the cells ascend strictly and val is X[c, v]: the image IS the CSC form."""
    from tangram_amd import SparseMap
    X = make_pattern(p)
    spot_ptr, cell, val = (_np(t) for t in SparseMap(X, device).image())
    csc = X.tocsc()
    csc.sort_indices()
    counts = np.bincount(X.indices, minlength=X.shape[1])
    np.testing.assert_array_equal(spot_ptr, np.concatenate([[0], np.cumsum(counts)]))
    for v in range(X.shape[1]):
        c = cell[spot_ptr[v]:spot_ptr[v + 1]]
        assert (np.diff(c) > 0).all(), f"{p}: the cells of spot {v} do not ascend strictly"
        np.testing.assert_array_equal(_bits(val[spot_ptr[v]:spot_ptr[v + 1]]), _bits(np.asarray(X[c, v].todense()).ravel()))
    np.testing.assert_array_equal(cell, csc.indices)
    np.testing.assert_array_equal(_bits(val), _bits(csc.data))


def topk_csr(val, idx, V):
    """The canonical CSR [C, V] of result_topk's (values, indices)."""
    val, idx = _np(val), _np(idx)
    order = np.argsort(idx, axis=1)
    C, k = idx.shape
    return sp.csr_matrix((np.take_along_axis(val, order, 1).ravel(), np.take_along_axis(idx, order, 1).ravel().astype(np.int32),
                          np.arange(0, C * k + 1, k, dtype=np.int64)), shape=(C, V))


_trained = {}


def trained_topk(device, C, V, k=7, K=5, precision="bf16x3", steps=3):
    """(X, S, G, engine-free): the top-k CSR of a small engine after `steps` steps; computed once per shape and shared."""
    key = (str(device), C, V, k, K, precision, steps)
    if key not in _trained:
        from tangram_amd.engine import HipMapperEngine
        from tests import parity_common as pc
        S, G, d, M0 = pc.validation_problem(C, K, V, C + V)
        e = HipMapperEngine(S, G, M0, d=d, device=device, precision=precision, lambdas=LAM)
        e.step(steps, 0.1, e.new_history(steps), 0)
        X = topk_csr(*e.result_topk(k), V)
        e.release()
        _trained[key] = X
    return _trained[key]


def assert_within_chain_bound(got, X, S, where):
    """|got - ref| <= gamma_n sum |p s| per element, n = entries of the spot (n = 0: exactly 0)."""
    X64, S64 = X.astype(np.float64), np.asarray(S, dtype=np.float64)
    ref = np.asarray(X64.T @ S64)
    mag = np.asarray(abs(X64).T @ np.abs(S64))
    n = np.bincount(X.indices, minlength=X.shape[1]).astype(np.float64)
    gamma = (n * U / (1.0 - n * U))[:, None]
    err = np.abs(got.astype(np.float64) - ref)
    worst = np.unravel_index(np.argmax(err - gamma * mag), err.shape)
    print(f"{where}: max |err| {err.max():.3e}, max err / (gamma * mag) {np.nanmax(np.where(mag > 0, err / np.maximum(gamma * mag, 1e-300), 0)):.3f}")
    assert (err <= gamma * mag).all(), f"{where}: element {worst}: |err| {err[worst]:.3e} > bound {(gamma * mag)[worst]:.3e}"


def float_S(C, n_genes, seed):
    return np.random.default_rng(seed).standard_normal((C, n_genes)).astype(np.float32)


def check_general_floats(device, C, V):
    from tangram_amd import project_sparse
    X = trained_topk(device, C, V)
    S = float_S(C, 37, C + V)
    assert (S < 0).any()
    got = _np(project_sparse(X, S, device=device))
    assert got.shape == (V, 37) and got.dtype == np.float32
    assert_within_chain_bound(got, X, S, f"general floats C{C} V{V}")


def check_bit_reproducibility(device, C=300, V=257):
    from tangram_amd import SparseMap, project_sparse
    X = trained_topk(device, C, V)
    S = float_S(C, REPRO_GENES, 11)
    dev = torch.device(device)
    St = torch.as_tensor(S, device=dev)
    a, b = SparseMap(X, device), SparseMap(X, device)
    first = _np(a.project(St))
    assert_within_chain_bound(first, X, S, "bit reproducibility: the reference run")
    np.testing.assert_array_equal(_bits(_np(a.project(St))), _bits(first), err_msg="two calls in a row")
    np.testing.assert_array_equal(_bits(_np(b.project(St))), _bits(first), err_msg="two independently built images")
    for x, y in zip(a.image(), b.image()):
        np.testing.assert_array_equal(_np(x).view(np.uint8), _np(y).view(np.uint8), err_msg="the two images")
    out = torch.full((V, REPRO_GENES), float("nan"), dtype=torch.float32, device=dev)
    edges = (0,) + SPLITS + (REPRO_GENES,)
    for lo, hi in zip(edges[:-1], edges[1:]):
        a.project_into(St[:, lo:hi], out[:, lo:hi])
    np.testing.assert_array_equal(_bits(_np(out)), _bits(first), err_msg=f"the gene range split at columns {SPLITS}")
    # the same matrix with the entries of every row shuffled: canonicalised on a copy, the caller's arrays unchanged
    rng = np.random.default_rng(3)
    indices, data = X.indices.copy(), X.data.copy()
    for c in range(C):
        perm = rng.permutation(X.indptr[c + 1] - X.indptr[c]) + X.indptr[c]
        indices[X.indptr[c]:X.indptr[c + 1]], data[X.indptr[c]:X.indptr[c + 1]] = X.indices[perm], X.data[perm]
    shuffled = sp.csr_matrix((data, indices, X.indptr.copy()), shape=X.shape)
    assert not shuffled.has_sorted_indices
    keep = [shuffled.indptr.copy(), shuffled.indices.copy(), shuffled.data.copy()]
    np.testing.assert_array_equal(_bits(_np(project_sparse(shuffled, S, device=device))), _bits(first), err_msg="rows shuffled")
    for before, after in zip(keep, (shuffled.indptr, shuffled.indices, shuffled.data)):
        np.testing.assert_array_equal(before, after, err_msg="the caller's matrix was modified")


def check_pipeline_tie(device, C, K, V, k=8, n_genes=50):
    """T, the sparse projection of result_topk(k), against D, the dense projection of the same engine (fp32, 3 steps, S >= 0):
    T <= D elementwise, and per gene sum_v (D - T) = sum_c (1 - mass_c) S[c, g]; both to relFro(P^T S) <= 1e-4 of ||D||."""
    from tangram_amd import project_sparse
    from tangram_amd.engine import HipMapperEngine
    from tests import parity_common as pc
    S, G, d, M0 = pc.validation_problem(C, K, V, C + V)
    e = HipMapperEngine(S, G, M0, d=d, device=device, precision="fp32", lambdas=LAM)
    e.step(3, 0.1, e.new_history(3), 0)
    S_all = np.abs(float_S(C, n_genes, 5))
    D = _np(e.project_genes(S_all)).astype(np.float64)
    X = topk_csr(*e.result_topk(k), V)
    e.release()
    T = _np(project_sparse(X, S_all, device=device)).astype(np.float64)
    tol = pc.TOL["fp32"]["ghat"] * np.linalg.norm(D)
    mass = np.asarray(X.astype(np.float64).sum(axis=1)).ravel()
    assert (mass > 0).all() and (mass <= 1 + 1e-6).all() and mass.min() < 0.999, "the truncation must drop visible mass"
    lost = (1.0 - mass) @ S_all.astype(np.float64)
    gap = (D - T).sum(axis=0)
    print(f"pipeline tie C{C} V{V}: ||D|| {np.linalg.norm(D):.4e}, tol {tol:.3e}, max (T - D) {np.max(T - D):.3e}, "
          f"||gap - lost|| {np.linalg.norm(gap - lost):.3e}, ||lost|| {np.linalg.norm(lost):.3e}")
    assert (T <= D + tol).all(), f"T exceeds D by {np.max(T - D):.3e} > {tol:.3e}"
    assert np.linalg.norm(gap - lost) <= tol, f"||sum_v (D - T) - sum_c (1 - mass_c) S|| = {np.linalg.norm(gap - lost):.3e} > {tol:.3e}"
    assert np.linalg.norm(lost) > 10 * tol, "the lost mass must be far above the tolerance for the identity to say anything"


def _map(device, **kw):
    import tangram_amd as tg
    from tests.test_map_cells_to_space import _adatas
    ad_sc, ad_sp = _adatas()
    return tg.map_cells_to_space(ad_sc, ad_sp, mode="cells", device=device, num_epochs=4, random_state=42, verbose=False, **kw)


def check_public_surface(device):
    import tangram_amd as tg
    from tangram_amd.anndata_lite import AnnDataLite
    from tests.test_map_cells_to_space import _adatas
    import pandas as pd
    dense = _map(device)
    top = _map(device, top_k=4)
    assert sp.issparse(top.X)
    ge = tg.project_genes(top, _adatas()[0], truncated=True, device=device)
    ge_dense = tg.project_genes(dense, _adatas()[0], device=device)
    S = np.asarray(_adatas()[0].X, dtype=np.float32)
    got = np.asarray(ge.X)
    assert got.shape == (top.X.shape[1], S.shape[1]) == np.asarray(ge_dense.X).shape
    np.testing.assert_array_equal(_bits(got), _bits(_np(tg.project_sparse(top.X, S, device=device))))
    assert_within_chain_bound(got, top.X.tocsr(), S, "project_genes(truncated=True)")
    assert ge.obs.equals(ge_dense.obs) and ge.var.equals(ge_dense.var) and ge.var["is_training"].sum() == 12
    assert set(ge.uns) == set(ge_dense.uns)
    # ... after the mapper was released
    kept = _map(device, top_k=4, keep_mapper=True)
    kept._tangram_amd_mapper.release()
    np.testing.assert_array_equal(_bits(np.asarray(tg.project_genes(kept, _adatas()[0], truncated=True, device=device).X)), _bits(got))
    # ... on a CSR built by hand from a thresholded dense mapping: rows that do not sum to one, no renormalisation
    P = np.asarray(dense.X, dtype=np.float32).copy()
    P[P < 0.05] = 0.0
    hand = AnnDataLite(sp.csr_matrix(P), obs=dense.obs, var=dense.var, uns=dense.uns)
    assert np.abs(P.sum(axis=1) - 1).max() > 1e-3
    ge_hand = np.asarray(tg.project_genes(hand, _adatas()[0], truncated=True, device=device).X)
    assert_within_chain_bound(ge_hand, hand.X, S, "a thresholded dense mapping")
    # ... a sparse adata_sc.X of 1 030 genes: two blocks of the expansion, the same bits as the dense S in one call
    rng = np.random.default_rng(8)
    wide = (rng.random((S.shape[0], 1030)) < 0.2) * rng.integers(1, 9, size=(S.shape[0], 1030))
    wide[0] = 1
    wide = wide.astype(np.float32)
    ad_wide = AnnDataLite(sp.csr_matrix(wide), obs=_adatas()[0].obs, var=pd.DataFrame(index=[f"g{i}" for i in range(1030)]))
    ge_wide = tg.project_genes(top, ad_wide, truncated=True, device=device)
    assert np.asarray(ge_wide.X).shape == (top.X.shape[1], 1030) and ge_wide.var["is_training"].sum() == 12
    np.testing.assert_array_equal(_bits(np.asarray(ge_wide.X)), _bits(_np(tg.project_sparse(top.X, wide, device=device))))
    assert_within_chain_bound(np.asarray(ge_wide.X), top.X.tocsr(), wide, "sparse adata_sc.X, 1 030 genes")
    # ... and what is refused: before anything runs on the device
    with pytest.raises(ValueError, match="sparse adata_map.X"):
        tg.project_genes(dense, _adatas()[0], truncated=True, device=device)
    with pytest.raises(ValueError, match="mapper="):
        tg.project_genes(top, _adatas()[0], truncated=True, mapper=kept._tangram_amd_mapper, device=device)
    with pytest.raises(ValueError, match=r"mapper=adata_map\._tangram_amd_mapper"):
        tg.project_genes(top, _adatas()[0], device=device)                     # the default is unchanged
    X = top.X.tocsr()
    bad = sp.csr_matrix((X.data.copy(), X.indices.copy(), X.indptr.copy()), shape=X.shape)
    bad.indices[5] = X.shape[1]
    with pytest.raises(ValueError, match="spot index outside"):
        tg.project_genes(AnnDataLite(bad, obs=top.obs, var=top.var, uns=top.uns), _adatas()[0], truncated=True, device=device)
    with pytest.raises(ValueError, match="spot index outside"):
        tg.project_sparse(bad, S, device=device)
    with pytest.raises(ValueError, match="rows for"):
        tg.project_sparse(X[:-1], S, device=device)
    short = AnnDataLite(X[:-1], obs=top.obs.iloc[:-1], var=top.var, uns=top.uns)
    with pytest.raises(ValueError):
        tg.project_genes(short, _adatas()[0], truncated=True, device=device)
    broken = sp.csr_matrix((X.data.copy(), X.indices.copy(), X.indptr.copy()), shape=X.shape)
    broken.indptr[3] = broken.indptr[4] + 1
    with pytest.raises(ValueError, match="indptr"):
        tg.project_sparse(broken, S, device=device)


def check_argument_errors(device):
    """Every invalid combination returns TG_ERR_INVALID -> ValueError with the library's message; a valid call afterwards is exact."""
    from tangram_amd import SparseMap
    from tangram_amd.preprocess import _stream
    lib = _capi.lib()
    p = ("k", 40, 65, 4)
    X = make_pattern(p)
    sm = SparseMap(X, device)
    dev = sm.device
    C, V, nnz, n = 40, 65, int(X.nnz), 8
    st = _stream(dev)
    ws = sm.workspace.data_ptr()
    S = torch.zeros((C, n), dtype=torch.float32, device=dev)
    out = torch.zeros((V, n), dtype=torch.float32, device=dev)
    ip, ix, dt = (t.data_ptr() for t in sm._csr_dev)
    nbytes = ct.c_size_t()

    def refused(msg, fn, *args):
        with pytest.raises(ValueError, match=msg):
            _capi.check(fn(*args))

    refused("NULL", lib.tg_sparse_map_query_bytes, C, V, nnz, None)
    for bad in ((-1, V, nnz), (C, -1, nnz), (C, V, -1)):
        refused("negative size", lib.tg_sparse_map_query_bytes, *bad, ct.byref(nbytes))
        refused("negative size", lib.tg_sparse_map_build, ip, ix, dt, *bad, ws, st)
        refused("negative size", lib.tg_sparse_map_project, ws, *bad, S.data_ptr(), n, n, out.data_ptr(), n, st)
    for bad in ((2 ** 31, V, nnz), (C, 2 ** 31 - 1, nnz), (2 ** 20, 2 ** 20, 2 ** 31)):
        refused("32-bit", lib.tg_sparse_map_query_bytes, *bad, ct.byref(nbytes))
        refused("32-bit", lib.tg_sparse_map_build, ip, ix, dt, *bad, ws, st)
        refused("32-bit", lib.tg_sparse_map_project, ws, *bad, S.data_ptr(), n, n, out.data_ptr(), n, st)
    refused("do not fit", lib.tg_sparse_map_build, ip, ix, dt, 2, 3, 7, ws, st)
    for args in ((None, ix, dt), (ip, None, dt), (ip, ix, None)):
        refused("null argument", lib.tg_sparse_map_build, *args, C, V, nnz, ws, st)
    refused("null argument", lib.tg_sparse_map_build, ip, ix, dt, C, V, nnz, None, st)
    for w, s_, o_ in ((None, S.data_ptr(), out.data_ptr()), (ws, None, out.data_ptr()), (ws, S.data_ptr(), None)):
        refused("null argument", lib.tg_sparse_map_project, w, C, V, nnz, s_, n, n, o_, n, st)
    for ng, lds, ldo in ((0, n, n), (-3, n, n), (n, n - 1, n), (n, n, n - 1)):
        refused("n_genes", lib.tg_sparse_map_project, ws, C, V, nnz, S.data_ptr(), lds, ng, out.data_ptr(), ldo, st)
    _capi.check(lib.tg_sparse_map_query_bytes(C, V, nnz, ct.byref(nbytes)))
    assert nbytes.value == sm.workspace.numel() >= 8 * (V + 1) + 8 * nnz
    _capi.check(lib.tg_sparse_map_query_bytes(0, 0, 0, ct.byref(nbytes)))
    assert nbytes.value > 0
    project_exact(sm, X, 65, False, "after the refused calls")
    project_exact(SparseMap(X, device), X, 64, True, "a new image after the refused calls")
