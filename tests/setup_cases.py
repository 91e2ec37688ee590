"""Case tables and checks for the kernels that run once before the first step (tangram_amd/csrc/tg_setup.h): tg_csr_gather_cols,
tg_csr_cols_to_dense, tg_row_sums, tg_normalize_total, tg_cluster_sums, tg_s_exact_check and tg_init_normal, each against a plain
high-precision reference of the same operation at every boundary of its loops.

Shared by the emulator suite (tests/test_setup_kernels.py, device "cpu") and the GPU suite (tests/test_gpu_setup_kernels.py): every
`check_*` takes a device string first, like tests/test_preprocess.py::check_preprocessing.  No test lives here.

Loop boundaries the tables are built around:
  tg_csr_gather_cols, tg_csr_cols_to_dense   256 threads zero the output row (`k += 256`) and walk the stored values (`i += 256`)
  tg_row_sums                                 one wave of 64 lanes per row (`k += 64` / `i += 64`), four rows per block
  tg_normalize_total                          one block of 1024 threads (`i += 1024`)
  tg_cluster_sums                             column blocks of 256 threads, members summed in the order they are listed
  tg_s_exact_check                            C * (K + 1 + T) elements: S, the d_source column, the cell-type columns
  tg_init_normal                              four columns per thread, at most 16 384 blocks of 256 threads, then a grid stride
"""
import ctypes as ct
import functools
import math

import numpy as np
import scipy.sparse as sp
import torch

SENTINEL = -7.0                # pre-fill of every padded output: the columns past `ncols` must still hold it afterwards
HALF_ULP = 0.5 + 1e-6          # "the fp64 result rounded once": double accumulation of <= 5000 fp32 values is off by < 1e-12 relative


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def ulp32(x):
    """float32 unit in the last place at the magnitude of the EXACT (fp64) value x: 2^(floor(log2 |x|) - 23), denormals 2^-149."""
    _, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def ulp_error(got, exact):
    """|got - exact| in float32 ulps of `exact`, elementwise; where exact == 0 the result must be 0 too (inf otherwise)."""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    err = np.abs(got - exact) / ulp32(exact)
    return np.where(exact == 0, np.where(got == 0, 0.0, np.inf), err)


def fsum_rows(X):
    return np.array([math.fsum(row) for row in np.asarray(X, dtype=np.float64)], dtype=np.float64).reshape(len(X))


def make_values(kind, shape, rng):
    if kind == "counts":
        return (rng.negative_binomial(2, 0.4, size=shape) + 1).astype(np.float32)
    if kind == "decades":                       # positive, spread over 8 decades: an fp32 accumulator is a whole ulp off on these
        return (np.abs(rng.standard_normal(shape)) * np.exp(rng.uniform(-10, 10, shape))).astype(np.float32)
    raise KeyError(kind)


def _device(device):
    from tangram_amd import preprocess as pre
    return pre._check_device(device)


def _up(a, device):
    return torch.as_tensor(np.ascontiguousarray(a), device=_device(device))


def _call(device, name, *args):
    """One call of the C ABI on `device`'s current stream (what tangram_amd.preprocess does), for the arguments its wrappers never
    pass: a row pitch wider than the column count, a column offset, a member list in any order."""
    from tangram_amd import _capi, preprocess as pre
    dev = _device(device)
    pre._call(dev, getattr(_capi.lib(), name), *args, pre._stream(dev))


def _padded(nrows, ncols, pad, device):
    return torch.full((nrows, ncols + pad), SENTINEL, dtype=torch.float32, device=_device(device))


def _split_padded(out, ncols, what):
    """The [:, :ncols] part of a padded output as NumPy, after checking that nothing was written past it."""
    a = out.cpu().numpy()
    assert (a[:, ncols:] == np.float32(SENTINEL)).all(), f"{what}: wrote past column {ncols} of a row of pitch {a.shape[1]}"
    return a[:, :ncols]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. CSR gather
# ---------------------------------------------------------------------------------------------------------------------------------
CSR_NCOLS = 701
LONG_ROWS = (0, 1, 255, 256, 257, 512, 513, 700, 0)          # stored values per row; the empty row is the first and the last
ROW_257, ROW_700 = 4, 7
HOLE_700 = 5                                                  # the one column the 700-value row does not store
CSR_MATRICES = {"long-rows": LONG_ROWS, "one-row": (300,)}


@functools.lru_cache(maxsize=None)
def csr_matrix_case(name):
    """(scipy CSR, dense float32) with exactly CSR_MATRICES[name] stored values per row, the pattern built explicitly."""
    rng = np.random.default_rng(11)
    indptr, indices = [0], []
    for n in CSR_MATRICES[name]:
        if n == 700:
            cols = np.delete(np.arange(CSR_NCOLS), HOLE_700)
        else:
            cols = np.sort(rng.choice(CSR_NCOLS, size=n, replace=False))
        indices.append(cols)
        indptr.append(indptr[-1] + n)
    indices = np.concatenate(indices).astype(np.int32)
    data = (rng.random(len(indices)) + 0.5).astype(np.float32)                 # no stored zero, all different
    m = sp.csr_matrix((data, indices, np.asarray(indptr, dtype=np.int64)), shape=(len(CSR_MATRICES[name]), CSR_NCOLS))
    assert m.has_canonical_format and tuple(np.diff(m.indptr)) == CSR_MATRICES[name]
    return m, m.toarray().astype(np.float32)


def last_stored_column(name):
    m, _ = csr_matrix_case(name)
    row = ROW_257 if name == "long-rows" else 0
    return int(m.indices[m.indptr[row + 1] - 1])


def column_selection(matrix, sel):
    kind, _, n = sel.partition("-")
    if kind == "perm":
        return np.random.default_rng(int(n)).permutation(CSR_NCOLS)[:int(n)]
    if kind == "identity":
        return np.arange(int(n))
    if sel == "skip-last-stored":                 # every column but the one that holds a row's last stored value
        return np.delete(np.arange(CSR_NCOLS), last_stored_column(matrix))
    raise KeyError(sel)


OUT_COLS = (1, 255, 256, 257, 700)
SELECTIONS = [f"perm-{n}" for n in OUT_COLS] + [f"identity-{n}" for n in OUT_COLS] + ["skip-last-stored"]
PADS = (0, 5)
GATHER_CASES = [("long-rows", s, p) for s in SELECTIONS for p in PADS] + \
               [("one-row", s, p) for s in ("perm-257", "identity-700", "skip-last-stored") for p in PADS]
BLOCK_WIDTHS = (256, 300)                          # both tile the 701 columns with a short last block (189 and 101 columns)
BLOCK_CASES = [(m, w, p) for m in CSR_MATRICES for w in BLOCK_WIDTHS for p in PADS]
BOUNDARY_BLOCK = (256, 256)                        # (col0, ncols): columns 255, 256, 511 and 512 are all stored in the 700-value row


def _csr_on(device, m):
    from tangram_amd import preprocess as pre
    return pre.DeviceCSR(m, device)


def check_csr_gather(device, matrix, sel, pad):
    """tg_csr_gather_columns == X[:, cols] of the dense matrix, value for value."""
    from tangram_amd import preprocess as pre
    m, dense = csr_matrix_case(matrix)
    cols = column_selection(matrix, sel)
    want = dense[:, cols]
    if sel == "skip-last-stored":
        assert dense[:, last_stored_column(matrix)].any() and len(cols) == CSR_NCOLS - 1
    if pad == 0:                                   # the product's own wrapper: ld_out == ncols
        got = pre.gather_training_genes(m, cols, device).cpu().numpy()
    else:
        csr = _csr_on(device, m)
        colmap = np.full(CSR_NCOLS, -1, dtype=np.int32)
        colmap[cols] = np.arange(len(cols), dtype=np.int32)
        colmap_d = _up(colmap, device)
        out = _padded(m.shape[0], len(cols), pad, device)
        _call(device, "tg_csr_gather_columns", csr.indptr.data_ptr(), csr.indices.data_ptr(), csr.data.data_ptr(), m.shape[0],
              colmap_d.data_ptr(), len(cols), out.data_ptr(), len(cols) + pad)
        got = _split_padded(out, len(cols), "tg_csr_gather_columns")
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} elements differ, first at {np.argwhere(got != want)[:3].tolist()}"


def column_blocks(width):
    return [(c0, min(width, CSR_NCOLS - c0)) for c0 in range(0, CSR_NCOLS, width)]


def check_csr_blocks(device, matrix, width, pad):
    """tg_csr_columns_to_dense on blocks (col0, ncols) that tile the columns: every block == dense[:, col0:col0 + ncols], and the
    blocks side by side == the dense matrix."""
    m, dense = csr_matrix_case(matrix)
    csr = _csr_on(device, m)
    blocks = column_blocks(width)
    assert blocks[-1][1] < width and sum(n for _, n in blocks) == CSR_NCOLS
    if matrix == "long-rows" and BOUNDARY_BLOCK in blocks:     # both sides of `c >= 0 && c < ncols` hold a stored value in one row
        c0, n = BOUNDARY_BLOCK
        assert dense[ROW_700, [c0 - 1, c0, c0 + n - 1, c0 + n]].all()
    parts = []
    for c0, n in blocks:
        out = _padded(m.shape[0], n, pad, device)
        _call(device, "tg_csr_columns_to_dense", csr.indptr.data_ptr(), csr.indices.data_ptr(), csr.data.data_ptr(), m.shape[0],
              c0, n, out.data_ptr(), n + pad)
        got = _split_padded(out, n, f"tg_csr_columns_to_dense block ({c0}, {n})")
        assert np.array_equal(got, dense[:, c0:c0 + n]), f"block ({c0}, {n}): {int((got != dense[:, c0:c0 + n]).sum())} elements differ"
        parts.append(got)
    assert np.array_equal(np.concatenate(parts, axis=1), dense)


PROJECT_SHAPE = (200, 30, 90, 77)                  # C, K, V and 77 genes to project: blocks of 30, 30 and 17 columns


def check_project_genes_sparse(device):
    """HipMapperEngine.project_genes(csr) == project_genes(dense) with a gene count that is no multiple of the handle's K."""
    from oracle import tangram_oracle as orc
    from tangram_amd.engine import HipMapperEngine
    C, K, V, n = PROJECT_SHAPE
    assert n % K
    data = orc.make_synthetic(C, K, V, seed=5)
    e = HipMapperEngine(data["S"], data["G"], orc.reference_init_M(C, V, 2), d=data["d"], device=device, precision="bf16x3",
                        lambdas=dict(lambda_d=1.0))
    e.step(2, 0.1, e.new_history(2))
    rng = np.random.default_rng(0)
    dense = (rng.gamma(1.0, 2.0, size=(C, n)) * (rng.random((C, n)) < 0.3)).astype(np.float32)
    dense[:, n - 1] = rng.gamma(1.0, 2.0, size=C).astype(np.float32)           # the last column of the short block is full
    a = e.project_genes(sp.csr_matrix(dense)).cpu().numpy()
    b = e.project_genes(dense).cpu().numpy()
    np.testing.assert_array_equal(a, b)
    assert a.shape == (V, n) and np.isfinite(a).all() and (a.max(axis=0) > 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. row sums and density
# ---------------------------------------------------------------------------------------------------------------------------------
LONG_SUM = 5000                                    # values per row at which an fp32 running sum is a whole ulp off
ROW_SUM_NCOLS = (1, 63, 64, 65, 129, 1000)
ROW_SUM_NROWS = (1, 3, 4, 5, 1027)
ROW_SUM_PADS = (0, 3)
ROW_SUM_DENSE_CASES = [(r, c, p) for c in ROW_SUM_NCOLS for r in ROW_SUM_NROWS for p in ROW_SUM_PADS] + \
                      [(6, LONG_SUM, p) for p in ROW_SUM_PADS]
ROW_SUM_CSR_CASES = {"short-rows": (0, 1, 63, 64, 65, 200), "long-rows": (LONG_SUM, 0, LONG_SUM, LONG_SUM, LONG_SUM, LONG_SUM, LONG_SUM)}
VALUE_KINDS = ("counts", "decades")
DENSITY_N = (1, 2, 1023, 1024, 1025, 5000, 20000)
DENSITY_NCOLS = 11


def _running_sum_f32(X):
    """What a plain float32 accumulator gives: s += x, left to right."""
    return np.cumsum(np.asarray(X, dtype=np.float32), axis=1, dtype=np.float32)[:, -1]


def check_row_sums_dense(device, nrows, ncols, pad):
    """tg_row_sums on a dense [nrows, ncols] matrix of row pitch ncols + pad == math.fsum of the row, rounded once."""
    from tangram_amd import preprocess as pre
    worst = {}
    for kind in VALUE_KINDS:
        rng = np.random.default_rng(1000 * nrows + ncols)
        X = make_values(kind, (nrows, ncols + pad), rng)
        X[:, ncols:] = 1e30                                                     # a column of padding read by mistake shows at once
        exact = fsum_rows(X[:, :ncols])
        Xd = _up(X, device)[:, :ncols]
        assert Xd.stride(0) == ncols + pad
        got = pre.row_sums(Xd, device).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (nrows,)
        worst[kind] = float(ulp_error(got, exact).max())
        assert worst[kind] <= HALF_ULP, f"{kind}: {worst[kind]:.4f} ulp from the exactly rounded sum"
        if kind == "decades" and ncols == LONG_SUM:
            # the case says something about the accumulator only if a float32 running sum of the same rows MISSES the bound
            naive = float(ulp_error(_running_sum_f32(X[:, :ncols]), exact).max())
            assert naive > HALF_ULP, f"a float32 running sum meets the bound too ({naive:.4f} ulp): the rows prove nothing"
            worst["float32 running sum"] = naive
    return worst


@functools.lru_cache(maxsize=None)
def row_sum_csr_case(name, kind):
    lengths = ROW_SUM_CSR_CASES[name]
    rng = np.random.default_rng(len(lengths) + 17)
    ncols = max(lengths) + 40
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(ncols, size=n, replace=False)) for n in lengths]).astype(np.int32)
    data = make_values(kind, len(indices), rng)
    assert (data != 0).all()
    m = sp.csr_matrix((data, indices, indptr), shape=(len(lengths), ncols))
    exact = np.array([math.fsum(data[indptr[i]:indptr[i + 1]].astype(np.float64)) for i in range(len(lengths))])
    return m, exact


def check_row_sums_csr(device, name):
    """tg_row_sums on CSR input (indptr, data) == math.fsum of the stored values of the row, rounded once; an empty row sums to 0."""
    from tangram_amd import preprocess as pre
    worst = {}
    for kind in VALUE_KINDS:
        m, exact = row_sum_csr_case(name, kind)
        got = pre.row_sums(m, device).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (m.shape[0],)
        worst[kind] = float(ulp_error(got, exact).max())
        assert worst[kind] <= HALF_ULP, f"{kind}: {worst[kind]:.4f} ulp from the exactly rounded sum"
        empty = np.diff(m.indptr) == 0
        assert empty.any() and (got[empty] == 0).all()
        if kind == "decades" and name == "long-rows":
            rows = [m.data[m.indptr[i]:m.indptr[i + 1]] for i in np.nonzero(~empty)[0]]
            naive = float(ulp_error(_running_sum_f32(np.stack(rows)), exact[~empty]).max())
            assert naive > HALF_ULP, f"a float32 running sum meets the bound too ({naive:.4f} ulp): the rows prove nothing"
            worst["float32 running sum"] = naive
    return worst


def check_density(device, n):
    """tg_row_sums(normalize=1), the density prior `X.sum(axis=1) / X.sum()` over n spots.  With r = the float32 row sums and the
    total taken in double, d = r / sum(r) rounded ONCE (<= 0.5 ulp).  Against the exact rowsum / total there are two roundings:
    r is off by a relative 2^-24 at most, which is at most 1 ulp of the quotient, and the quotient is rounded (0.5 ulp) -> 1.5 ulp
    (the total of the rounded row sums is off by the AVERAGE of their rounding errors, which is far below one of them)."""
    from tangram_amd import preprocess as pre
    rng = np.random.default_rng(n)
    X = (np.abs(rng.standard_normal((n, DENSITY_NCOLS))) * np.exp(rng.uniform(-3, 3, (n, DENSITY_NCOLS)))).astype(np.float32)
    X *= (rng.random(X.shape) < 0.6)
    X[:, 0] = np.maximum(X[:, 0], np.float32(0.25))                             # no empty spot: the CSR and the dense form agree
    rowsum = fsum_rows(X)
    exact = rowsum / math.fsum(rowsum)
    out = {}
    for form, M in (("dense", X), ("csr", sp.csr_matrix(X))):
        r64 = pre.row_sums(M, device).cpu().numpy().astype(np.float64)
        d = pre.rna_count_density(M, device).cpu().numpy()
        assert d.dtype == np.float32 and d.shape == (n,)
        once = float(ulp_error(d, r64 / math.fsum(r64)).max())
        twice = float(ulp_error(d, exact).max())
        assert once <= HALF_ULP, f"{form}: {once:.4f} ulp from r / sum(r) rounded once"
        assert twice <= 1.5, f"{form}: {twice:.4f} ulp from the exact rowsum / total"
        assert abs(d.sum(dtype=np.float64) - 1.0) < n * 2.0 ** -24
        if n == 1:
            assert d[0] == np.float32(1.0)
        out[form] = (once, twice)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. cluster aggregation
# ---------------------------------------------------------------------------------------------------------------------------------
CLUSTER_NCOLS = (1, 255, 256, 257, 513)
CLUSTER_BIG = 3000
CLUSTER_REV = 10
CLUSTER_ROWS = CLUSTER_BIG + 1 + CLUSTER_REV
# name -> member rows in the order the kernel is to add them; "ghost" is a label of unique_labels that no row carries
CLUSTER_LAYOUTS = {
    "four-labels": ("one", "big", "ghost", "rev"),
    "all-in-one": ("all",),
}
CLUSTER_CASES = [("four-labels", c, p) for c in CLUSTER_NCOLS for p in ((0, 0), (3, 5))] + [("all-in-one", 257, (0, 0)), ("all-in-one", 257, (3, 5))]


def cluster_members(label):
    if label == "one":
        return np.array([CLUSTER_BIG], dtype=np.int32)
    if label == "big":
        return np.arange(CLUSTER_BIG, dtype=np.int32)
    if label == "rev":                                                          # listed in DECREASING row order
        return np.arange(CLUSTER_ROWS - 1, CLUSTER_BIG, -1, dtype=np.int32)
    if label == "ghost":
        return np.zeros(0, dtype=np.int32)
    if label == "all":
        return np.arange(CLUSTER_ROWS, dtype=np.int32)
    raise KeyError(label)


@functools.lru_cache(maxsize=None)
def cluster_case(layout, ncols):
    """(X, members per label, exact fp64 sums [n_labels, ncols]): fsum over the members of every column."""
    rng = np.random.default_rng(ncols)
    X = make_values("decades", (CLUSTER_ROWS, ncols), rng)
    members = [cluster_members(l) for l in CLUSTER_LAYOUTS[layout]]
    X64 = X.astype(np.float64)
    sums = np.array([[math.fsum(X64[rows, k]) for k in range(ncols)] for rows in members], dtype=np.float64).reshape(len(members), ncols)
    return X, members, sums


def check_cluster_aggregate(device, layout, ncols, pads):
    """tg_cluster_aggregate, sum and mean, == the fp64 sum / mean per label rounded once; the label nobody carries sums to exactly 0
    and its mean is NaN (0 / 0, as NumPy's mean of nothing).  pads = (input pitch - ncols, output pitch - ncols)."""
    from tangram_amd import preprocess as pre
    X, members, sums = cluster_case(layout, ncols)
    labels = CLUSTER_LAYOUTS[layout]
    counts = np.array([len(r) for r in members], dtype=np.float64)
    pad_in, pad_out = pads
    Xp = np.full((CLUSTER_ROWS, ncols + pad_in), 1e30, dtype=np.float32)
    Xp[:, :ncols] = X
    Xd = _up(Xp, device)
    indptr_d = _up(np.concatenate([[0], np.cumsum([len(r) for r in members])]).astype(np.int32), device)
    rows_d = _up(np.concatenate(members).astype(np.int32), device)
    worst = {}
    for mean in (0, 1):
        out = _padded(len(members), ncols, pad_out, device)
        _call(device, "tg_cluster_aggregate", Xd.data_ptr(), ncols + pad_in, ncols, indptr_d.data_ptr(), rows_d.data_ptr(), len(members),
              mean, out.data_ptr(), ncols + pad_out)
        got = _split_padded(out, ncols, "tg_cluster_aggregate")
        _check_clusters(got, sums, counts, labels, mean, worst)
    if pads == (0, 0):
        # the product's wrapper builds the member lists itself from labels / unique_labels (rows in increasing order)
        lab = np.empty(CLUSTER_ROWS, dtype=object)
        for l, rows in zip(labels, members):
            lab[rows] = l
        for mean in (0, 1):
            got = pre.cluster_expression(_up(X, device), lab, list(labels), scale=not mean).cpu().numpy()
            _check_clusters(got, sums, counts, labels, mean, worst)
    return worst


def _check_clusters(got, sums, counts, labels, mean, worst):
    assert got.dtype == np.float32 and got.shape == sums.shape
    for i, l in enumerate(labels):
        if counts[i] == 0:
            assert np.isnan(got[i]).all() if mean else (got[i] == 0).all(), (l, mean, got[i][:4])
            continue
        exact = sums[i] / counts[i] if mean else sums[i]
        w = float(ulp_error(got[i], exact).max())
        worst[(l, mean)] = max(worst.get((l, mean), 0.0), w)
        assert w <= HALF_ULP, f"label {l!r} ({int(counts[i])} rows), {'mean' if mean else 'sum'}: {w:.4f} ulp from the exactly rounded result"


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. bf16-exactness check
# ---------------------------------------------------------------------------------------------------------------------------------
SX_SHAPE = (131, 37, 53)                           # C, K, V: two cell tiles of 128, nothing a multiple of anything
SX_TILE, SX_STEPS, SX_TYPES = 128, 3, 3
GENERAL, TWO_PRODUCTS = "bf16x3", "bf16x3 (S exact: 2 products)"
_C, _K, _V = SX_SHAPE
BF16_MAX = 3.3895314e38
# (id, where, value, verdict or None): `where` = ("S", row, column) | ("d_source", row) | ("ct", row, column)
SX_POSITION_CASES = [
    ("S-first-element", ("S", 0, 0), 257.0, GENERAL),
    ("S-last-element", ("S", _C - 1, _K - 1), 257.0, GENERAL),
    ("S-last-row-first-column", ("S", _C - 1, 0), 257.0, GENERAL),
    ("d_source-last-row", ("d_source", _C - 1), 257.0, GENERAL),
    ("ct-last-row-last-column", ("ct", _C - 1, SX_TYPES - 1), 1.0 / 3.0, GENERAL),
]
SX_EXACT_VALUES = (256.0, 65536.0, -3.0, 0.5, -0.0, 2.0 ** -20, BF16_MAX)
SX_INEXACT_VALUES = (257.0, 255.5, 65537.0, 1.0 + 2.0 ** -8, float(np.float32(3.4028235e38)))
SX_UNPINNED_VALUES = (2.0 ** -133, 2.0 ** -140, float("inf"))
SX_VALUE_AT = ("S", 77, 19)
SX_CASES = SX_POSITION_CASES + \
    [("exact-d_source-column", ("d_source", None), 2.0 ** -7, TWO_PRODUCTS), ("exact-one-hot-cell-types", ("ct", None, None), 1.0, TWO_PRODUCTS)] + \
    [(f"exact-{v!r}", SX_VALUE_AT, v, TWO_PRODUCTS) for v in SX_EXACT_VALUES] + \
    [(f"inexact-{v!r}", SX_VALUE_AT, v, GENERAL) for v in SX_INEXACT_VALUES] + \
    [(f"unpinned-{v!r}", SX_VALUE_AT, v, None) for v in SX_UNPINNED_VALUES]


@functools.lru_cache(maxsize=None)
def _sx_base():
    from oracle import tangram_oracle as orc
    C, K, V = SX_SHAPE
    data = orc.make_synthetic(C, K, V, seed=3, n_types=SX_TYPES)
    assert data["S"].max() < 256 and (data["S"] == np.round(data["S"])).all()          # counts: bf16-exact
    return data, orc.reference_init_M(C, V, 42), orc.grid_graph(V, standardized=False, self_inclusion=False)


def _sx_run(device, S, G, d, M0, s_exact, lam, kw):
    from tangram_amd.engine import HipMapperEngine
    e = HipMapperEngine(S, G, M0, d=d, device=device, precision="bf16x3", lambdas=lam, tile_size=SX_TILE, s_exact=s_exact, **kw)
    h = e.new_history(SX_STEPS)
    e.step(SX_STEPS, 0.1, h)
    M, m1, m2, _ = e.logits()
    out = dict(P=e.result().cpu().numpy(), h=h.cpu().numpy(), M=M.cpu().numpy().copy(), m1=m1.cpu().numpy().copy(),
               m2=m2.cpu().numpy().copy(), eff=e.effective_precision)
    e.release()
    return out


def check_s_exact(device, where, value, verdict):
    """One element of what the S images are built from is set to `value`: the handle made with s_exact="auto" must compute what the
    one made with s_exact=False computes (P, history, logits and both Adam moments EQUAL), whatever its verdict; and the verdict
    read from effective_precision is the pinned one."""
    data, M0, graph = _sx_base()
    C, K, V = SX_SHAPE
    S = data["S"].copy()
    lam, kw = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5), {}
    if where[0] == "S":
        S[where[1], where[2]] = np.float32(value)
    elif where[0] == "d_source":
        ds = np.full(C, 2.0 ** -7, dtype=np.float32)                             # exact everywhere ...
        if where[1] is not None:
            ds[where[1]] = np.float32(value)                                     # ... but here
        kw = dict(d_source=ds)
    elif where[0] == "ct":
        E = data["ct_encode"].copy()
        if where[1] is not None:
            E[where[1], where[2]] = np.float32(value)
        lam = dict(lambda_g1=1.0, lambda_d=1.0, lambda_ct_islands=0.17)
        kw = dict(neighborhood_filter=graph, ct_encode=E)
    else:
        raise KeyError(where)
    a = _sx_run(device, S, data["G"], data["d"], M0, False, lam, kw)
    b = _sx_run(device, S, data["G"], data["d"], M0, "auto", lam, kw)
    assert a["eff"] == GENERAL
    # A value above the largest bf16 (+inf, FLT_MAX) has the hi part +inf and the lo part x - inf on the GENERAL path already: NaN
    # in every result of both runs, compared as equal.  Everywhere else the results are finite and compared with plain ==.
    nan_ok = not abs(float(np.float32(value))) <= BF16_MAX
    for k in ("P", "M", "m1", "m2"):
        assert nan_ok or np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k], equal_nan=nan_ok), f"{k}: {int((a[k] != b[k]).sum())} elements differ between s_exact=False and 'auto' ({b['eff']})"
    used = ~np.isnan(a["h"]).all(axis=0)                                         # (the columns of the terms that are off stay NaN)
    assert nan_ok or (used[:2].all() and used.sum() >= 3)                        # total, main and at least one more term were recorded
    assert np.array_equal(a["h"][:, used], b["h"][:, used], equal_nan=nan_ok), "history"
    assert np.array_equal(np.isnan(a["h"]), np.isnan(b["h"]))
    if verdict is not None:
        assert b["eff"] == verdict, f"value {value!r} at {where}: the library took {b['eff']!r}"
    return b["eff"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. device initialiser
# ---------------------------------------------------------------------------------------------------------------------------------
MASK64 = (1 << 64) - 1
INIT_TOL = 1e-5        # the kernel takes the logarithm, the square root, the angle and the cosine in fp32: radius <= 5.9, angle error
#                        <= 7.5e-7 -> about 5e-6 absolute.  A wrong constant, shift or index gives differences of order 1.
GRID_CAP_QUADS = 16384 * 256
INIT_DIRECT = dict(shape=(300, 501), seeds=(42, 43), stream_ids=(0, 1))
INIT_NARROW_CASES = [(n, col0, 3) for n in (1, 2, 3, 5) for col0 in (0, 3)]       # (n_cols, col0, pad) of a 7 x 11 plane
INIT_NARROW_PLANE = (7, 11)
INIT_WIDE = dict(n_rows=86000, n_cols=8, col0=49990, n_cols_total=50000, last_rows=5)
INIT_PLANES = {"gpu": (4200, 4100), "cpu": (300, 410)}                          # the emulator's is far below the grid cap: see the check


def mixed_seed(seed, stream_id):
    """device_init.device_normal's own seed mixing"""
    return (int(seed) * 0x9E3779B1 + int(stream_id) * 0x85EBCA77) & MASK64


def counter_bits(seed64, idx):
    """tg_counter_normal's integer part in exact 64-bit arithmetic (Python ints masked to 64 bits): the two 24-bit fields."""
    z = (idx * 0x9E3779B97F4A7C15 + ((seed64 ^ 0xD1B54A32D192ED03) * 0xBF58476D1CE4E5B9)) & MASK64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z >> 40, z & 0xFFFFFF


def counter_normal_ref(seed64, indices):
    """tg_counter_normal at the given global indices (an iterable of Python ints), float64.  The two uniforms are the float32 numbers
    the formula defines them as, (float(bits) + 0.5f) * 2^-24 -- the addition rounds once bits >= 2^23 --, and the Box-Muller
    transform of them is taken in fp64."""
    bits = np.array([counter_bits(seed64, int(i)) for i in indices], dtype=np.int64).reshape(-1, 2)
    u = (bits.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    assert u.dtype == np.float32 and (u > 0).all() and (u <= 1).all()
    u = u.astype(np.float64)
    return np.sqrt(-2.0 * np.log(u[:, 0])) * np.cos(2.0 * math.pi * u[:, 1])


def plane_ref(seed64, rows, cols, n_cols_total):
    """Reference block for the given global rows and columns -> [len(rows), len(cols)] float64"""
    idx = [int(r) * int(n_cols_total) + int(c) for r in rows for c in cols]
    return counter_normal_ref(seed64, idx).reshape(len(rows), len(cols))


def check_init_direct(device, seed, stream_id):
    """device_normal(300, 501) against the formula, element for element."""
    from tangram_amd.device_init import device_normal
    R, Cn = INIT_DIRECT["shape"]
    got = device_normal(R, Cn, device, seed=seed, stream_id=stream_id).cpu().numpy()
    ref = plane_ref(mixed_seed(seed, stream_id), range(R), range(Cn), Cn)
    err = float(np.abs(got - ref).max())
    assert got.dtype == np.float32 and err <= INIT_TOL, f"seed {seed}, stream {stream_id}: max |got - ref| = {err:.3e}"
    return err


def check_init_narrow(device, n_cols, col0, pad):
    """Blocks narrower than, as wide as and wider than one quad of columns, at an even and an odd first column, written into rows of
    pitch n_cols + pad through the C ABI."""
    R, total = INIT_NARROW_PLANE
    seed64 = mixed_seed(7, 0)
    out = _padded(R, n_cols, pad, device)
    _call(device, "tg_init_logits_normal", out.data_ptr(), R, n_cols, n_cols + pad, ct.c_uint64(seed64), col0, total)
    got = _split_padded(out, n_cols, "tg_init_logits_normal")
    ref = plane_ref(seed64, range(R), range(col0, col0 + n_cols), total)
    err = float(np.abs(got - ref).max())
    assert err <= INIT_TOL, f"{n_cols} columns at {col0}: max |got - ref| = {err:.3e}"
    return err


def check_init_index_above_2_32(device):
    """The block BASELINE config 4's last rank draws: global indices r * 50 000 + column pass 2^32 at row 85 900."""
    from tangram_amd.device_init import device_normal
    w = INIT_WIDE
    got = device_normal(w["n_rows"], w["n_cols"], device, seed=42, col0=w["col0"], n_cols_total=w["n_cols_total"]).cpu().numpy()
    rows = range(w["n_rows"] - w["last_rows"], w["n_rows"])
    cols = range(w["col0"], w["col0"] + w["n_cols"])
    assert min(rows) * w["n_cols_total"] + min(cols) > 2 ** 32                  # every index compared needs more than 32 bits
    assert (w["n_rows"] - 1) * w["n_cols_total"] + max(cols) > 2 ** 32
    ref = plane_ref(mixed_seed(42, 0), rows, cols, w["n_cols_total"])
    err = float(np.abs(got[-w["last_rows"]:] - ref).max())
    assert np.isfinite(got).all() and err <= INIT_TOL, f"max |got - ref| = {err:.3e}"
    # the rows below 2^32 of the same block, so that a truncated index cannot pass by accident of the comparison either
    ref0 = plane_ref(mixed_seed(42, 0), range(2), cols, w["n_cols_total"])
    assert float(np.abs(got[:2] - ref0).max()) <= INIT_TOL
    return err


def check_init_plane(device, plane):
    """A whole plane: 2000 elements chosen at random and the last row against the formula, a 3-column block drawn alone against the
    same columns of the plane, every value finite.  plane "gpu" (4200 x 4100 = 4.3 M quads, 69 MB) is above the cap of 16 384 blocks
    x 256 threads, so every thread makes a second trip of the grid-stride loop; plane "cpu" is the emulator's, which walks a plane
    thread by thread and CANNOT reach the cap in the time a test has: it runs the same comparisons below the cap."""
    from tangram_amd.device_init import device_normal
    R, Cn = INIT_PLANES[plane]
    quads = R * ((Cn + 3) // 4)
    assert (quads > GRID_CAP_QUADS) == (plane == "gpu")
    full = device_normal(R, Cn, device, seed=42)
    c0 = 1000 if Cn > 1003 else 100
    blk = device_normal(R, 3, device, seed=42, col0=c0, n_cols_total=Cn)
    assert torch.equal(full[:, c0:c0 + 3], blk)
    assert bool(torch.isfinite(full).all())
    seed64 = mixed_seed(42, 0)
    rng = np.random.default_rng(5)
    rr, cc = rng.integers(0, R, 2000), rng.integers(0, Cn, 2000)
    got = full[torch.as_tensor(rr, device=full.device), torch.as_tensor(cc, device=full.device)].cpu().numpy()
    ref = counter_normal_ref(seed64, [int(r) * Cn + int(c) for r, c in zip(rr, cc)])
    last = full[R - 1].cpu().numpy()
    ref_last = plane_ref(seed64, [R - 1], range(Cn), Cn)[0]
    err = max(float(np.abs(got - ref).max()), float(np.abs(last - ref_last).max()))
    assert err <= INIT_TOL, f"max |got - ref| = {err:.3e}"
    return err


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables keep every boundary
# ---------------------------------------------------------------------------------------------------------------------------------
def check_case_tables():
    # 1. CSR gather
    assert set(LONG_ROWS) >= {0, 1, 255, 256, 257, 512, 513} and max(LONG_ROWS) >= 700 and LONG_ROWS[0] == 0 and LONG_ROWS[-1] == 0
    assert {len(v) for v in CSR_MATRICES.values()} >= {1, len(LONG_ROWS)} and max(CSR_MATRICES["one-row"]) > 256
    for matrix in CSR_MATRICES:
        sels = {s for m, s, _ in GATHER_CASES if m == matrix}
        assert {p for m, _, p in GATHER_CASES if m == matrix} == {0, 5} and "skip-last-stored" in sels
        assert any(s.startswith("perm-") for s in sels) and any(s.startswith("identity-") for s in sels)
    long_sels = {s for m, s, _ in GATHER_CASES if m == "long-rows"}
    assert {len(column_selection("long-rows", s)) for s in long_sels if s.startswith("perm-")} >= {1, 255, 256, 257, 700}
    assert {len(column_selection("long-rows", s)) for s in long_sels if s.startswith("identity-")} >= {1, 255, 256, 257, 700}
    assert all((m, s, 5 - p) in GATHER_CASES for m, s, p in GATHER_CASES)
    assert {(m, p) for m, _, p in BLOCK_CASES} == {(m, p) for m in CSR_MATRICES for p in (0, 5)}
    assert all(column_blocks(w)[-1][1] < w for _, w, _ in BLOCK_CASES) and any(BOUNDARY_BLOCK in column_blocks(w) for m, w, _ in BLOCK_CASES if m == "long-rows")
    assert PROJECT_SHAPE[3] % PROJECT_SHAPE[1] and PROJECT_SHAPE[3] > 2 * PROJECT_SHAPE[1]
    # 2. row sums and density
    assert {c for _, c, _ in ROW_SUM_DENSE_CASES} >= {1, 63, 64, 65, 129, 1000, 5000}
    assert {r for r, _, _ in ROW_SUM_DENSE_CASES} >= {1, 3, 4, 5, 1027}
    assert all((r, c, 3 - p) in ROW_SUM_DENSE_CASES for r, c, p in ROW_SUM_DENSE_CASES) and {p for _, _, p in ROW_SUM_DENSE_CASES} == {0, 3}
    assert set(ROW_SUM_CSR_CASES["short-rows"]) >= {0, 1, 63, 64, 65, 200} and set(ROW_SUM_CSR_CASES["long-rows"]) == {0, 5000}
    assert set(VALUE_KINDS) == {"counts", "decades"}
    assert set(DENSITY_N) >= {1, 2, 1023, 1024, 1025, 5000, 20000}
    # 3. clusters
    assert {c for l, c, _ in CLUSTER_CASES if l == "four-labels"} >= {1, 255, 256, 257, 513}
    assert {p for l, _, p in CLUSTER_CASES if l == "four-labels"} == {(0, 0), (3, 5)} and any(l == "all-in-one" for l, _, _ in CLUSTER_CASES)
    assert set(CLUSTER_LAYOUTS["four-labels"]) == {"one", "big", "ghost", "rev"} and CLUSTER_LAYOUTS["all-in-one"] == ("all",)
    assert len(cluster_members("one")) == 1 and len(cluster_members("big")) == 3000 and len(cluster_members("ghost")) == 0
    assert (np.diff(cluster_members("rev")) < 0).all() and len(cluster_members("all")) == CLUSTER_ROWS
    # 4. exactness check
    C, K, V = SX_SHAPE
    assert SX_SHAPE == (131, 37, 53) and (SX_TILE, SX_STEPS) == (128, 3)
    ids = [c[0] for c in SX_CASES]
    assert len(set(ids)) == len(ids)
    pos = {c[1]: c for c in SX_POSITION_CASES}
    assert set(pos) == {("S", 0, 0), ("S", C - 1, K - 1), ("S", C - 1, 0), ("d_source", C - 1), ("ct", C - 1, SX_TYPES - 1)}
    assert all(c[3] == GENERAL for c in SX_POSITION_CASES) and all(c[2] == 257.0 for c in SX_POSITION_CASES if c[1][0] != "ct")
    by_verdict = {v: {c[2] for c in SX_CASES if c[3] == v and c[1] == SX_VALUE_AT} for v in (TWO_PRODUCTS, GENERAL, None)}
    assert by_verdict[TWO_PRODUCTS] == {256.0, 65536.0, -3.0, 0.5, 0.0, 2.0 ** -20, 3.3895314e38} and any(math.copysign(1, v) < 0 and v == 0 for v in SX_EXACT_VALUES)
    assert by_verdict[GENERAL] == {257.0, 255.5, 65537.0, 1.0 + 2.0 ** -8, float(np.float32(3.4028235e38))}
    assert by_verdict[None] == {2.0 ** -133, 2.0 ** -140, float("inf")}
    assert np.float32(2.0 ** -133) != 0 and np.float32(2.0 ** -140) != 0 and np.float32(BF16_MAX).view(np.uint32) & 0xFFFF == 0
    # 5. initialiser
    assert INIT_DIRECT == dict(shape=(300, 501), seeds=(42, 43), stream_ids=(0, 1))
    assert {n for n, _, _ in INIT_NARROW_CASES} >= {1, 2, 3, 5} and any(c0 % 2 for _, c0, _ in INIT_NARROW_CASES) and all(p == 3 for _, _, p in INIT_NARROW_CASES)
    assert all(c0 + n <= INIT_NARROW_PLANE[1] for n, c0, _ in INIT_NARROW_CASES)
    assert INIT_WIDE == dict(n_rows=86000, n_cols=8, col0=49990, n_cols_total=50000, last_rows=5)
    R, Cn = INIT_PLANES["gpu"]
    assert R * ((Cn + 3) // 4) > GRID_CAP_QUADS and R * Cn * 4 < 70e6
    R, Cn = INIT_PLANES["cpu"]
    assert R * ((Cn + 3) // 4) < GRID_CAP_QUADS
