"""Thin owner of one `tg_mapper` handle: device buffers come from torch (plumbing), every
computation goes through the C ABI of libtangram_hip.so."""
from __future__ import annotations

import ctypes as ct

import numpy as np
import torch

from . import _capi, _device
from .preprocess import DeviceCSR


def _csr_pair(mat, n, device):
    """(CSR of mat, CSR of mat^T) as int32/float32 device tensors; `mat` is a dense array/matrix or scipy.sparse."""
    import scipy.sparse as sp
    m = mat if sp.issparse(mat) else sp.csr_matrix(np.asarray(mat, dtype=np.float32))
    m = m.tocsr().astype(np.float32)
    if m.shape != (n, n):
        raise ValueError(f"spot graph must be {n} x {n}, got {m.shape}")
    out = []
    for a in (m, m.T.tocsr()):
        a.sort_indices()
        out.append((torch.as_tensor(a.indptr.astype(np.int32), device=device),
                    torch.as_tensor(a.indices.astype(np.int32), device=device),
                    torch.as_tensor(a.data.astype(np.float32), device=device)))
    return out[0], out[1], int(m.nnz)


def _as_dev_f32(x, device):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.float32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float32)), device=device)


class HipMapperEngine:
    """State + workspace of one mapping problem (or one spot-shard of it) on one GPU."""

    def __init__(self, S, G, M0, d=None, d_source=None, F0=None, *, mode="mapper", device="cuda:0",
                 precision="bf16x3", lambdas=None, n_spots_total=None, n_ranks=0, fwd_splits=0, tile_size=0, pipeline_bands=0,
                 bwd_tile=0, spot_offset=0, s_exact=False,
                 target_count=0.0, betas=(0.9, 0.999), eps=1e-8,
                 voxel_weights=None, neighborhood_filter=None, ct_encode=None, spatial_weights=None):
        self.device = _device.check_device(device)
        if precision not in _capi.PRECISIONS:
            raise ValueError(f"gemm precision must be one of {sorted(_capi.PRECISIONS)}")
        self._lib = _capi.lib()
        lam = dict(lambda_g1=1.0, lambda_d=0.0, lambda_g2=0.0, lambda_r=0.0, lambda_l1=0.0, lambda_l2=0.0,
                   lambda_count=1.0, lambda_f_reg=1.0, lambda_neighborhood_g1=0.0, lambda_ct_islands=0.0,
                   lambda_getis_ord=0.0, lambda_moran=0.0, lambda_geary=0.0)
        lam.update(lambdas or {})
        S = _as_dev_f32(S, self.device)
        G = _as_dev_f32(G, self.device)
        M0 = _as_dev_f32(M0, self.device)
        d = _as_dev_f32(d, self.device)
        d_source = _as_dev_f32(d_source, self.device)
        F0 = _as_dev_f32(F0, self.device)
        self.C, self.K = S.shape
        self.V = G.shape[0]
        if G.shape[1] != self.K:
            raise ValueError("S and G must have the same number of genes")
        if tuple(M0.shape) != (self.C, self.V):
            raise ValueError("M0 must be [n_cells, n_spots]")
        cfg = _capi.TgConfig()
        cfg.abi_version = _capi.TG_ABI_VERSION
        cfg.mode = _capi.TG_MODE_CONSTRAINED if mode == "constrained" else _capi.TG_MODE_MAPPER
        cfg.precision = _capi.PRECISIONS[precision]
        cfg.n_cells, cfg.n_genes, cfg.n_spots = self.C, self.K, self.V
        cfg.n_spots_total = int(n_spots_total or self.V)
        cfg.n_ranks = int(n_ranks)
        cfg.has_density = int(d is not None)
        cfg.has_d_source = int(d_source is not None)
        cfg.fwd_splits = int(fwd_splits)
        cfg.tile_size = int(tile_size)
        cfg.pipeline_bands = int(pipeline_bands)
        cfg.bwd_tile = int(bwd_tile)
        cfg.spot_offset = int(spot_offset)
        # any falsy value (False, 0, numpy.False_, None): the general three-product path; "auto": the library checks S once.  True was
        # accepted as "check" before round 5 and is again, with a warning -- nobody can CLAIM exactness, the library always checks.
        if isinstance(s_exact, str):
            if s_exact != "auto":
                raise ValueError("s_exact must be False (always the general three-product path) or 'auto' (check S once at construction)")
            s_exact = True
        elif s_exact:
            import warnings
            warnings.warn("s_exact=True is treated as s_exact='auto': the library checks S itself", DeprecationWarning, stacklevel=3)
        cfg.s_exact_mode = 1 if s_exact else 0
        for k, v in lam.items():
            setattr(cfg, k, float(v))
        cfg.target_count = float(target_count)
        cfg.beta1, cfg.beta2, cfg.eps = float(betas[0]), float(betas[1]), float(eps)
        self.cfg = cfg
        self.precision = precision
        inp = _capi.TgInputs()
        inp.S_dev, inp.G_dev, inp.M0_dev = S.data_ptr(), G.data_ptr(), M0.data_ptr()
        inp.d_dev = d.data_ptr() if d is not None else None
        inp.d_source_dev = d_source.data_ptr() if d_source is not None else None
        inp.F0_dev = F0.data_ptr() if F0 is not None else None
        keep = []                                   # keep the CSR tensors alive until create() has copied them
        if lam["lambda_neighborhood_g1"] > 0:
            if voxel_weights is None:
                raise ValueError("lambda_neighborhood_g1 > 0 needs voxel_weights")
            w, wt, cfg.nnz_w = _csr_pair(voxel_weights, cfg.n_spots_total, self.device)
            keep += [w, wt]
            inp.w_indptr, inp.w_indices, inp.w_data = (x.data_ptr() for x in w)
            inp.wt_indptr, inp.wt_indices, inp.wt_data = (x.data_ptr() for x in wt)
        if lam["lambda_getis_ord"] > 0 or lam["lambda_moran"] > 0 or lam["lambda_geary"] > 0:
            if spatial_weights is None:
                raise ValueError("lambda_getis_ord / lambda_moran / lambda_geary > 0 need spatial_weights")
            ws, wst, cfg.nnz_s = _csr_pair(spatial_weights, cfg.n_spots_total, self.device)
            keep += [ws, wst]
            inp.s_indptr, inp.s_indices, inp.s_data = (x.data_ptr() for x in ws)
            inp.st_indptr, inp.st_indices, inp.st_data = (x.data_ptr() for x in wst)
        if lam["lambda_ct_islands"] > 0:
            if neighborhood_filter is None or ct_encode is None:
                raise ValueError("lambda_ct_islands > 0 needs neighborhood_filter and ct_encode")
            nn, nt, cfg.nnz_n = _csr_pair(neighborhood_filter, cfg.n_spots_total, self.device)
            E = _as_dev_f32(ct_encode, self.device)
            if E.shape[0] != self.C:
                raise ValueError("ct_encode must have one row per cell")
            cfg.n_cell_types = int(E.shape[1])
            keep += [nn, nt, E]
            inp.n_indptr, inp.n_indices, inp.n_data = (x.data_ptr() for x in nn)
            inp.nt_indptr, inp.nt_indices, inp.nt_data = (x.data_ptr() for x in nt)
            inp.ct_encode_dev = E.data_ptr()
        self._keepalive = keep
        sizes = _capi.TgSizes()
        _capi.check(self._lib.tg_query_sizes(ct.byref(cfg), ct.byref(sizes)))
        self.sizes = sizes
        self.state = torch.empty(sizes.state_bytes, dtype=torch.uint8, device=self.device)
        self.workspace = torch.empty(sizes.workspace_bytes, dtype=torch.uint8, device=self.device)
        handle = ct.c_void_p()
        # the stream every call of this handle is enqueued on (the library binds to it at create())
        self._torch_stream = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None
        self._hip_stream = _device.stream(self.device)
        self._call(self._lib.tg_mapper_create, ct.byref(cfg), ct.byref(inp), self.state.data_ptr(),
                   self.workspace.data_ptr(), self._hip_stream, ct.byref(handle))
        self._h = handle
        self._sync()            # inputs were only borrowed for the duration of create()
        # The precision the handle really computes in.  Clusters-mode problems (<= 32 rows of M, one GPU, no spatial terms,
        # tile_size not pinned) train on the library's exact-fp32 clusters-mode kernels whatever `gemm_precision` says, and the
        # library then also validates / projects such a handle in fp32 (tg_make_layout): `precision` is what was asked for,
        # `effective_precision` what runs.
        # `bf16x3` on a bf16-exact S (raw counts, one-hot columns): two matrix-core products per element instead of three, the
        # same results (`s_exact="auto"`: the default of Mapper / MapperConstrained / map_cells_to_space; this low-level class
        # defaults to the general path, `s_exact=False`) -> "bf16x3 (S exact: 2 products)".
        self.effective_precision = {0: "fp32", 1: "bf16", 2: "bf16x3", 3: "bf16x3 (S exact: 2 products)"}.get(
            int(self._lib.tg_mapper_effective_precision(self._h)), precision)
        self._scratch_row = torch.zeros(_capi.H_NTERMS, dtype=torch.float32, device=self.device)

    # -- plumbing ---------------------------------------------------------------------------------
    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def _call(self, fn, *args, tensors=()):
        """One C-ABI call with this mapper's GPU as the current HIP device (the library enqueues on the stream it was created
        with; HIP rejects a stream that does not belong to the current device).

        The caller may be on ANOTHER torch stream than the one the handle was created on (torch streams are non-blocking):
        the creation stream first waits for the caller's stream (allocations / uploads issued there), and the caller's
        stream waits for the library's work afterwards, so reads such as `.cpu()` see finished results.  `tensors`: buffers
        allocated on the caller's stream that the library touches (kept from being recycled early by the caching allocator)."""
        if self.device.type != "cuda":
            return _capi.check(fn(*args))
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            foreign = cur != self._torch_stream
            if foreign:
                self._torch_stream.wait_stream(cur)
                for t in tensors:
                    if t is not None:
                        t.record_stream(self._torch_stream)
            try:
                return _capi.check(fn(*args))
            finally:
                if foreign:
                    cur.wait_stream(self._torch_stream)

    def close(self):
        if getattr(self, "_h", None):
            self._sync()
            self._lib.tg_mapper_destroy(self._h)
            self._h = None

    def release(self):
        """Destroy the handle and drop the state / workspace buffers (>= 16 bytes per cell x spot) right away."""
        self.close()
        self.state = self.workspace = self._keepalive = self._scratch_row = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the hot path -------------------------------------------------------------------------------
    def new_history(self, n_rows):
        return torch.full((n_rows, _capi.H_NTERMS), float("nan"), dtype=torch.float32, device=self.device)

    def step(self, n_steps, lr, history=None, first_row=0):
        hp = history.data_ptr() if history is not None else None
        self._call(self._lib.tg_mapper_step, self._h, int(n_steps), float(lr), hp, int(first_row), tensors=(history,))

    def attach_comm(self, comm_handle):
        """Spot shard: bind a `tg_comm` (tangram_amd.sharded builds it); collective -- performs the set-up exchanges."""
        self._call(self._lib.tg_mapper_attach_comm, self._h, comm_handle)

    def workspace_view(self, ptr, n_floats):
        """float32 torch view (no copy) of `n_floats` at device address `ptr` inside this handle's workspace."""
        off = int(ptr) - self.workspace.data_ptr()
        if off < 0 or off + 4 * n_floats > self.workspace.numel():
            raise ValueError("pointer outside the workspace")
        return self.workspace[off:off + 4 * n_floats].view(torch.float32)

    def result(self, with_filter=False):
        P = torch.empty((self.C, self.V), dtype=torch.float32, device=self.device)
        F = torch.empty((self.C,), dtype=torch.float32, device=self.device) if with_filter else None
        self._call(self._lib.tg_mapper_result, self._h, P.data_ptr(), F.data_ptr() if with_filter else None, tensors=(P, F))
        return (P, F) if with_filter else P

    def filter_values(self):
        """Constrained mode: sigmoid(F) [C] alone (tg_mapper_result without its dense plane)."""
        F = torch.empty((self.C,), dtype=torch.float32, device=self.device)
        self._call(self._lib.tg_mapper_result, self._h, None, F.data_ptr(), tensors=(F,))
        return F

    def result_topk(self, k):
        """Each cell's k most probable spots of this handle's spots: (values [C, k] float32, indices [C, k] int32) device tensors,
        value descending, equal values by ascending spot; the values are the bits `result()` holds at those places, the indices are
        global (spot_offset + column); rows of a shard with fewer than k spots end in (0, -1).  One pass over the logits
        (tg_mapper_result_topk): no C x V plane is written.  Constrained mode: softmax(M) without the filter, like adata_map.X."""
        k = int(k)
        val = torch.empty((self.C, max(k, 1)), dtype=torch.float32, device=self.device)
        idx = torch.empty((self.C, max(k, 1)), dtype=torch.int32, device=self.device)
        self._call(self._lib.tg_mapper_result_topk, self._h, k, val.data_ptr(), idx.data_ptr(), tensors=(val, idx))
        return val, idx

    def topk_merge(self, val, idx, k):
        """Best k of every row of the candidate lists val / idx [n_rows, n_in] (index -1 = pad), same order (tg_topk_merge)."""
        val = val.to(device=self.device, dtype=torch.float32)
        idx = idx.to(device=self.device, dtype=torch.int32)
        if val.dim() != 2 or val.shape != idx.shape or val.stride(1) != 1 or idx.stride(1) != 1 or val.stride(0) != idx.stride(0):
            val, idx = val.contiguous(), idx.contiguous()
        n_rows, n_in = val.shape
        k = int(k)
        out_v = torch.empty((n_rows, max(k, 1)), dtype=torch.float32, device=self.device)
        out_i = torch.empty((n_rows, max(k, 1)), dtype=torch.int32, device=self.device)
        self._call(self._lib.tg_topk_merge, val.data_ptr(), idx.data_ptr(), n_rows, n_in, int(val.stride(0)), k, out_v.data_ptr(),
                   out_i.data_ptr(), self._hip_stream, tensors=(val, idx, out_v, out_i))
        return out_v, out_i

    def result_spot_topk(self, k, min_filter=None, colsum=False, slab_rows=0):
        """Each spot's k most probable cells of this handle's spots -- the column reading of the mapping: (values [V, k] float32,
        cells [V, k] int32[, column sums [V] float32]) device tensors, value descending, equal values by ascending cell; the values
        are the bits `result()` holds at those places; 1 <= k <= 32 (_capi.SPOT_TOPK_MAX); a spot with fewer admitted cells than k
        ends in (0, -1).  One pass over the logits (tg_mapper_result_spot_topk): no C x V plane is written.  `min_filter`
        (constrained mode only): only cells whose filter value is > min_filter take part; None admits every cell.  `colsum=True`:
        also each spot's sum over the admitted cells (fp64 accumulation, rounded once).  `slab_rows`: 0 = the library cuts the cells
        into slabs; a value >= 8 forces the slab height (the lists do not depend on it)."""
        k, slab_rows = int(k), int(slab_rows)
        thr = -1.0 if min_filter is None else float(min_filter)
        nbytes = ct.c_size_t()
        self._call(self._lib.tg_mapper_spot_topk_query_bytes, self._h, k, slab_rows, ct.byref(nbytes))
        scratch = torch.empty((max(nbytes.value, 8) + 7) // 8, dtype=torch.int64, device=self.device)
        val = torch.empty((self.V, k), dtype=torch.float32, device=self.device)
        cell = torch.empty((self.V, k), dtype=torch.int32, device=self.device)
        total = torch.empty((self.V,), dtype=torch.float32, device=self.device) if colsum else None
        self._call(self._lib.tg_mapper_result_spot_topk, self._h, k, thr, slab_rows, scratch.data_ptr(), val.data_ptr(), cell.data_ptr(),
                   total.data_ptr() if colsum else None, tensors=(scratch, val, cell, total))
        return (val, cell, total) if colsum else (val, cell)

    def project(self):
        Gh = torch.empty((self.V, self.K), dtype=torch.float32, device=self.device)
        self._call(self._lib.tg_mapper_project, self._h, Gh.data_ptr(), tensors=(Gh,))
        return Gh

    def project_genes(self, S_all, unfiltered=True):
        """softmax(M)^T S_all for ANY gene set -> [V, K_all] device tensor; the C x V mapping never leaves the GPU
        (reference: `adata_map.X.T @ adata_sc.X`, utils.py:366-368).  S_all: [C, K_all] float32 on this device, a host array,
        or a scipy.sparse matrix -- then the CSR arrays are uploaded once and every block of genes is expanded on the device
        (preprocess.DeviceCSR.columns_into) instead of `adata_sc.X.toarray()` on the host (utils.py:364-365)."""
        if hasattr(S_all, "tocsr") and not isinstance(S_all, torch.Tensor):
            return self._project_genes_csr(S_all.tocsr(), unfiltered)
        S_all = torch.as_tensor(S_all)
        if S_all.dim() != 2 or S_all.shape[0] != self.C:
            raise ValueError("S_all must be [n_cells, n_genes] with the mapper's cells")
        S_all = S_all.to(device=self.device, dtype=torch.float32)
        if S_all.stride(1) != 1:
            S_all = S_all.contiguous()
        n = int(S_all.shape[1])
        out = torch.empty((self.V, n), dtype=torch.float32, device=self.device)
        self._call(self._lib.tg_mapper_project_genes, self._h, S_all.data_ptr(), int(S_all.stride(0)), n, out.data_ptr(), n,
                   1 if unfiltered else 0, tensors=(S_all, out))
        return out

    def _project_genes_csr(self, csr, unfiltered):
        if csr.shape[0] != self.C:
            raise ValueError("S_all must be [n_cells, n_genes] with the mapper's cells")
        csr = DeviceCSR(csr, self.device)
        n = int(csr.shape[1])
        out = torch.empty((self.V, n), dtype=torch.float32, device=self.device)
        block = torch.empty((self.C, min(self.K, n)), dtype=torch.float32, device=self.device)
        expand = lambda fn, *args: self._call(fn, *args, self._hip_stream, tensors=(csr.indptr, csr.indices, csr.data, block))  # noqa: E731
        for k0 in range(0, n, self.K):
            kc = min(self.K, n - k0)
            csr.columns_into(k0, kc, block, launch=expand)
            self._call(self._lib.tg_mapper_project_genes, self._h, block.data_ptr(), int(block.stride(0)), kc,
                       out.data_ptr() + 4 * k0, n, 1 if unfiltered else 0, tensors=(block, out))
        return out

    def validate(self):
        """(expression_sim, gv_sim, sparsity-weighted gv_sim, entropy) of the current mapping; one D2H copy."""
        out = torch.empty(4, dtype=torch.float32, device=self.device)
        self._call(self._lib.tg_mapper_validate, self._h, out.data_ptr(), tensors=(out,))
        return [float(x) for x in out.cpu().numpy()]

    def validate_into(self, out):
        """The same four numbers into `out` (4 float32 on the device), enqueued on the handle's stream: no copy, no synchronisation
        (a batch of mappings validated every epoch reads all its rows back once, at the end)."""
        self._call(self._lib.tg_mapper_validate, self._h, out.data_ptr(), tensors=(out,))

    def logits(self):
        """Views of M / Adam m / Adam v ([C, pitch] float32, columns >= V are padding)."""
        pm, p1, p2 = ct.c_void_p(), ct.c_void_p(), ct.c_void_p()
        pitch, step = ct.c_int32(), ct.c_int64()
        self._call(self._lib.tg_mapper_state, self._h, ct.byref(pm), ct.byref(p1), ct.byref(p2), ct.byref(pitch),
                                              ct.byref(step))
        out = []
        for p in (pm, p1, p2):
            off = p.value - self.state.data_ptr()
            out.append(self.state[off:off + 4 * self.C * pitch.value].view(torch.float32).view(self.C, pitch.value))
        return out[0], out[1], out[2], int(step.value)

    def filter_state(self):
        """Constrained mode: [3, pitch] view of the filter logits F and their two Adam moments (columns >= C are padding)."""
        pf, pitch = ct.c_void_p(), ct.c_int32()
        self._call(self._lib.tg_mapper_filter_state, self._h, ct.byref(pf), ct.byref(pitch))
        off = pf.value - self.state.data_ptr()
        return self.state[off:off + 4 * 3 * pitch.value].view(torch.float32).view(3, pitch.value)

    def set_step(self, step):
        self._call(self._lib.tg_mapper_set_step, self._h, int(step))

    def profile(self, enable=True):
        self._call(self._lib.tg_mapper_profile, self._h, int(bool(enable)))

    def profile_read(self):
        """[(kernel name, total ms, launches)] since profile(True); synchronises the stream."""
        names = ct.create_string_buffer(4096)
        ms = (ct.c_float * 64)()
        cnt = (ct.c_int * 64)()
        n = ct.c_int()
        self._call(self._lib.tg_mapper_profile_read, self._h, names, 4096, ms, cnt, 64, ct.byref(n))
        ks = names.value.decode().split(";") if n.value else []
        return [(k, float(ms[i]), int(cnt[i])) for i, k in enumerate(ks)]
