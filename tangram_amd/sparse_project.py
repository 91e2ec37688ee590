"""Genes projected from a SPARSE mapping on the device: `X.T @ S` for a cells x spots scipy matrix X with a few entries per row --
the `adata_map.X` of `map_cells_to_space(..., top_k=k)`, the same matrix written to disk and reloaded, a dense mapping the user
thresholded -- and the single-cell matrix S.  No mapper, no logits and no cells x spots plane are involved (csrc/tg_sparse.h):

  SparseMap         the spot-major image of X, built once on the device (tg_sparse_map_build): per spot its (cell, value)
                    entries in ascending cell order, a pure function of X; `.project(S)` any number of times
  project_sparse    X.T @ S -> [n_spots, n_genes] float32 device tensor; S dense (host array or device tensor: one call) or
                    scipy-sparse (uploaded once as a preprocess.DeviceCSR, expanded 1 024 genes at a time)

Every output element is one fp32 fmaf chain from 0 over the entries of its spot in that order: the same bits on every call, for every
alignment of S and for every split of the gene range.  The host checks the matrix (shape, index range, indptr) before anything is
uploaded; the device code trusts what it is given.  Everything goes through the C ABI; torch only owns the memory.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np
import torch

from . import _capi
from ._device import call, check_device, pitch, stream, workspace
from .preprocess import DeviceCSR

GENE_BLOCK = 1024           # genes of a sparse S expanded at a time (there is no mapper K to borrow here)


def canonical_csr(X, n_cells=None):
    """X as a canonical scipy CSR matrix (sorted indices, no duplicates), checked: ValueError for a wrong number of rows, an index
    outside [0, n_spots), an indptr that is not monotone from 0 to nnz.  The caller's matrix is never modified: canonicalisation
    works on a copy."""
    import scipy.sparse as sp
    if not sp.issparse(X):
        raise ValueError("the mapping must be a scipy.sparse matrix (cells x spots)")
    csr = X.tocsr()
    if n_cells is not None and csr.shape[0] != n_cells:
        raise ValueError(f"the sparse mapping has {csr.shape[0]} rows for {n_cells} cells")
    indptr, indices = np.asarray(csr.indptr), np.asarray(csr.indices)
    nnz = int(indices.shape[0])
    if indptr.shape[0] != csr.shape[0] + 1 or int(indptr[0]) != 0 or int(indptr[-1]) != nnz or np.asarray(csr.data).shape[0] != nnz \
            or (np.diff(indptr) < 0).any():
        raise ValueError("the sparse mapping's indptr is not monotone from 0 to the number of entries")
    if nnz and (int(indices.min()) < 0 or int(indices.max()) >= csr.shape[1]):
        raise ValueError(f"the sparse mapping holds a spot index outside [0, {csr.shape[1]})")
    if not csr.has_canonical_format:                 # (`tocsr()` of a CSR matrix is the caller's own object)
        csr = csr.copy()
        csr.sum_duplicates()
    return csr


class SparseMap:
    """The spot-major image of a cells x spots sparse mapping on `device`."""

    def __init__(self, X, device="cuda:0", n_cells=None):
        self.device = check_device(device)
        csr = canonical_csr(X, n_cells)
        self.n_cells, self.n_spots = (int(n) for n in csr.shape)
        self.nnz = int(csr.nnz)
        lib = _capi.lib()
        self.workspace = workspace(lib.tg_sparse_map_query_bytes, self.n_cells, self.n_spots, self.nnz, device=self.device)
        up = DeviceCSR(csr, self.device)
        call(self.device, lib.tg_sparse_map_build, up.indptr.data_ptr(), up.indices.data_ptr() or None, up.data.data_ptr() or None,
             self.n_cells, self.n_spots, self.nnz, self.workspace.data_ptr(), stream(self.device))
        self._csr_dev = (up.indptr, up.indices, up.data)      # (kept until the build has run: same stream as every later use)

    def image(self):
        """(spot_ptr int64 [n_spots + 1], cell int32 [nnz], val float32 [nnz]): views of the workspace, no copy."""
        off = (ct.c_int64 * 5)()
        _capi.check(_capi.lib().tg_debug_sparse_map_layout(self.n_spots, self.nnz, off))
        ws = self.workspace
        return (ws[off[0]:off[0] + 8 * (self.n_spots + 1)].view(torch.int64), ws[off[1]:off[1] + 4 * self.nnz].view(torch.int32),
                ws[off[2]:off[2] + 4 * self.nnz].view(torch.float32))

    def project_into(self, S, out):
        """out[:, :n] = X.T @ S for 2-D float32 device tensors with unit column stride (views with a pitch are taken as they are);
        columns of `out`'s storage outside the view are not touched."""
        for t, rows, name in ((S, self.n_cells, "S"), (out, self.n_spots, "out")):
            if t.dim() != 2 or t.shape[0] != rows or t.dtype != torch.float32 or t.device != self.device or (t.shape[1] > 1 and t.stride(1) != 1):
                raise ValueError(f"{name} must be a float32 [{rows}, n_genes] tensor on {self.device} with unit column stride")
        if S.shape[1] != out.shape[1]:
            raise ValueError("S and out differ in their number of genes")
        call(self.device, _capi.lib().tg_sparse_map_project, self.workspace.data_ptr(), self.n_cells, self.n_spots, self.nnz,
             S.data_ptr() or None, pitch(S), int(S.shape[1]), out.data_ptr() or None, pitch(out), stream(self.device))
        return out

    def project(self, S_all):
        """X.T @ S_all -> [n_spots, n_genes] float32 tensor on the device.  S_all: [n_cells, n_genes] device tensor or host array
        (one call), or a scipy.sparse matrix (CSR uploaded once, expanded GENE_BLOCK genes at a time)."""
        if hasattr(S_all, "tocsr") and not isinstance(S_all, torch.Tensor):
            return self._project_csr(S_all.tocsr())
        S_all = torch.as_tensor(S_all)
        if S_all.dim() != 2 or S_all.shape[0] != self.n_cells:
            raise ValueError("S_all must be [n_cells, n_genes] with the mapping's cells")
        S_all = S_all.to(device=self.device, dtype=torch.float32)
        if S_all.shape[1] > 1 and S_all.stride(1) != 1:
            S_all = S_all.contiguous()
        out = torch.empty((self.n_spots, int(S_all.shape[1])), dtype=torch.float32, device=self.device)
        if out.numel() == 0:
            return out
        return self.project_into(S_all, out)

    def _project_csr(self, csr):
        if csr.shape[0] != self.n_cells:
            raise ValueError("S_all must be [n_cells, n_genes] with the mapping's cells")
        n = int(csr.shape[1])
        out = torch.empty((self.n_spots, n), dtype=torch.float32, device=self.device)
        if out.numel() == 0:
            return out
        csr = DeviceCSR(csr, self.device)
        block = torch.empty((self.n_cells, min(GENE_BLOCK, n)), dtype=torch.float32, device=self.device)
        for k0 in range(0, n, GENE_BLOCK):
            kc = min(GENE_BLOCK, n - k0)
            csr.columns_into(k0, kc, block)
            self.project_into(block[:, :kc], out[:, k0:k0 + kc])
        return out


def project_sparse(X_csr, S_all, device="cuda:0"):
    """`X_csr.T @ S_all` -> [n_spots, n_genes] float32 tensor on `device`, of exactly the sparse cells x spots matrix passed in (no
    renormalisation of truncated rows).  The spot-major image is built once per call; hold a `SparseMap` to project repeatedly."""
    return SparseMap(X_csr, device, n_cells=int(S_all.shape[0])).project(S_all)
