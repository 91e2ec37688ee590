"""
Device-side `project_genes` (reference: tangram/utils.py:338-375).  The reference multiplies the C x V mapping by the
full single-cell matrix on the host (`adata_map.X.T @ adata_sc.X`, utils.py:368; 2*C*V*K_all flop, K_all ~ 26k genes
in the tutorial); here the product runs in the forward GEMM kernel of the training loop (tg_mapper_project_genes),
block of genes by block of genes, with the mapping resident in HBM.

Same argument meaning, `ValueError` condition and result contract (`X` = spots x genes, `obs` = adata_map.var,
`var` = adata_sc.var + `is_training`, `uns` = adata_sc.uns).  scanpy is not imported: the gene filter
`sc.pp.filter_genes(min_cells=1)` (:357) and `var_names_make_unique` (:354) are restated on the duck-typed inputs.
"""
from __future__ import annotations

import numpy as np
import pandas as pd
import torch

from . import mapping_utils as mu
from .anndata_lite import AnnDataLite
from .engine import HipMapperEngine


def _make_unique(names):
    """anndata's `var_names_make_unique` rule: later duplicates get -1, -2, ... appended."""
    seen, out = {}, []
    taken = set(names)
    for n in names:
        if n not in seen:
            seen[n] = 0
            out.append(n)
            continue
        while True:
            seen[n] += 1
            cand = "{}-{}".format(n, seen[n])
            if cand not in taken:
                break
        taken.add(cand)
        out.append(cand)
    return out


def _result(X, obs, var, uns):
    try:
        import anndata
        return anndata.AnnData(X=X, obs=obs, var=var, uns=uns)
    except Exception:
        return AnnDataLite(X, obs=obs, var=var, uns=uns)


def _projection_engine(adata_map, device, gemm_precision):
    """A mapper whose softmax reproduces a GIVEN mapping matrix `adata_map.X`: logits = log P, so softmax(logits) =
    P / rowsum(P).  Returns (engine, row sums): a mapping whose rows do not sum to one (filtered / edited by the caller)
    is projected exactly by scaling the rows of the single-cell matrix with the row sums."""
    P = torch.as_tensor(np.asarray(adata_map.X), dtype=torch.float32, device=device)
    rows = P.sum(dim=1).cpu().numpy().astype(np.float64)
    M0 = torch.log(P).clamp_(min=-1.0e30)
    C, V = P.shape
    S1 = torch.ones((C, 1), dtype=torch.float32, device=device)
    G1 = torch.ones((V, 1), dtype=torch.float32, device=device)
    return HipMapperEngine(S1, G1, M0, device=device, precision=gemm_precision, lambdas=dict(lambda_g1=1.0)), rows


def _prepare_sc(adata_map, adata_sc, cluster_label, scale):
    """What project_genes does to `adata_sc` before the product (reference utils.py:351-365) -> (the prepared adata_sc, its matrix:
    scipy-sparse as it is, or dense float32)."""
    adata_sc.var.index = [g.lower() for g in adata_sc.var.index]                     # :351
    adata_sc.var.index = _make_unique(list(adata_sc.var.index))                      # :354
    X = adata_sc.X
    n_cells = np.asarray((X != 0).sum(axis=0)).reshape(-1)                           # :357 filter_genes(min_cells=1)
    keep = n_cells >= 1
    if not keep.all():
        adata_sc = adata_sc[:, list(adata_sc.var.index[keep])]
    adata_sc.var["n_cells"] = n_cells[keep]
    if cluster_label:                                                                # :359-360
        adata_sc = mu.adata_to_cluster_expression(adata_sc, cluster_label, scale=scale)
    if not adata_map.obs.index.equals(adata_sc.obs.index):                           # :362-363
        raise ValueError("The two AnnDatas need to have same `obs` index.")
    X_sc = adata_sc.X                                                                # :364-365: sparse stays sparse, the gene blocks
    S_all = X_sc if hasattr(X_sc, "tocsr") else np.ascontiguousarray(mu._dense(X_sc), dtype=np.float32)   # are expanded on the device
    return adata_sc, S_all


def project_genes(adata_map, adata_sc, cluster_label=None, scale=True, *, mapper=None, device="cuda:0",
                  gemm_precision="bf16x3", truncated=False):
    """Transfer gene expression from the single cell data onto space (reference utils.py:338-375).

    Like the reference, the projection is `adata_map.X.T @ adata_sc.X` of the mapping matrix the caller passes in (which
    may have been edited or filtered since training): `adata_map.X` is uploaded once and multiplied on the device.
    Extra keywords: `mapper` -- pass the trained `Mapper`/`MapperConstrained` EXPLICITLY (e.g. the
    `adata_map._tangram_amd_mapper` of `map_cells_to_space(..., keep_mapper=True)`) to project with the mapping that is
    still resident in HBM instead (required when `adata_map.X` is the sparse top-k matrix of `top_k=`: ValueError otherwise); `device`, `gemm_precision` as in `map_cells_to_space`.
    `truncated=True` -- project a SPARSE `adata_map.X` as it is: the result is `adata_map.X.T @ adata_sc.X` of exactly the matrix
    passed in (the reference's definition, utils.py:366-368), computed on `device` by the sparse kernels (tangram_amd.sparse_project)
    without a mapper, logits or a cells x spots plane -- so it works on a top-k result that was saved and reloaded, mapped in another
    process, or whose mapper was released, and on a dense mapping thresholded into a sparse matrix.  The flag is explicit because
    this is NOT the dense mapping's projection: a top-k matrix keeps only part of each cell's probability mass
    (`adata_map.obs["top_k_mass"]`), nothing is renormalised, and every projected value is at most the dense one for non-negative
    expression.  ValueError with a dense `adata_map.X` or together with `mapper=`.
    Unlike the reference (`sc.pp.filter_genes`, `var_names_make_unique` mutate the caller's AnnData in place, :351-357),
    only `adata_sc.var.index` is rewritten in place; the gene filter and `n_cells` land on a view."""
    adata_sc, S_all = _prepare_sc(adata_map, adata_sc, cluster_label, scale)
    route = _Route(adata_map, S_all.shape[0], mapper, truncated, device, gemm_precision)
    try:
        X_space = route.project(S_all).cpu().numpy()                                 # :366  (adata_map.X.T @ adata_sc.X)
    finally:
        route.release()
    adata_ge = _result(X_space, adata_map.var, adata_sc.var, adata_sc.uns)           # :367-369
    training_genes = adata_map.uns["train_genes_df"].index.values                    # :370-371
    adata_ge.var["is_training"] = adata_ge.var.index.isin(training_genes)
    return adata_ge


_MISSING_SP = "Missing tangram parameters. Run `pp_adatas()`."
_MISSING_GE = "Missing tangram parameters. Use `project_genes()` to get adata_ge."
_TANGRAM_KEYS = {"training_genes", "overlap_genes"}


def _check_score_inputs(uns_ge, adata_sp, genes):
    """The checks compare_spatial_geneexp runs before it computes anything (reference utils.py:394-408) -> the genes to score."""
    if not _TANGRAM_KEYS.issubset(set(adata_sp.uns.keys())):
        raise ValueError(_MISSING_SP)
    if not _TANGRAM_KEYS.issubset(set(uns_ge.keys())):
        raise ValueError(_MISSING_GE)
    assert list(adata_sp.uns["overlap_genes"]) == list(uns_ge["overlap_genes"])
    return list(uns_ge["overlap_genes"] if genes is None else genes)


def _columns_of(var, genes, what):
    idx = var.index.get_indexer(genes)
    if (idx < 0).any():
        raise KeyError(f"genes missing from {what}: {[g for g, i in zip(genes, idx) if i < 0][:5]}")
    return idx


def _score_frame(scores, overlap_genes, var_ge, adata_sp, adata_sc, genes):
    """The DataFrame of compare_spatial_geneexp from the per-gene scores (reference utils.py:428-463)."""
    df_g = pd.DataFrame(np.asarray(scores, dtype=np.float64), overlap_genes, columns=["score"])
    for var in (var_ge, adata_sp.var):
        if "is_training" in var.keys():
            df_g["is_training"] = var["is_training"]
    df_g["sparsity_sp"] = adata_sp.var.loc[overlap_genes, "sparsity"]
    if adata_sc is not None:
        if not _TANGRAM_KEYS.issubset(set(adata_sc.uns.keys())):
            raise ValueError(_MISSING_SP)
        assert list(adata_sc.uns["overlap_genes"]) == list(adata_sp.uns["overlap_genes"])
        mu.annotate_gene_sparsity(adata_sc)
        df_g = df_g.merge(pd.DataFrame(adata_sc.var.loc[overlap_genes, "sparsity"]), left_index=True, right_index=True)
        df_g.rename({"sparsity": "sparsity_sc"}, inplace=True, axis="columns")
        df_g["sparsity_diff"] = df_g["sparsity_sp"] - df_g["sparsity_sc"]
    if genes is not None:
        df_g = df_g.loc[genes]
    return df_g.sort_values(by="score", ascending=False)


def compare_spatial_geneexp(adata_ge, adata_sp, adata_sc=None, genes=None, *, device="cuda:0", gene_block=1024):
    """Compares generated spatial data with the true spatial data (reference utils.py:377-463): a DataFrame indexed by gene with the
    columns `score` (cosine similarity of the gene's projected and measured expression over the spots), `is_training` (when
    `adata_ge.var` or `adata_sp.var` has it), `sparsity_sp`, and -- only when `adata_sc` is passed -- `sparsity_sc` and `sparsity_diff`
    (= sparsity_sp - sparsity_sc); subset and ordered by `genes` when given, then sorted by descending score.  Same argument
    meaning, ValueError conditions and assertions as the reference; like it, the call writes `var["sparsity"]` of adata_sp (and
    adata_sc).  The scored columns of `adata_ge.X` and `adata_sp.X` (dense or scipy-sparse: uploaded once as CSR, expanded on the
    device) go to `device` in blocks of `gene_block` genes and are reduced there (tg_gene_scores): products and sums in float64 of the
    float32 values, where the reference takes NumPy norms in the matrices' own precision.  The root logger is left alone."""
    from .gene_score import GeneBlocks, GeneScorer
    overlap_genes = _check_score_inputs(adata_ge.uns, adata_sp, genes)
    mu.annotate_gene_sparsity(adata_sp)
    if adata_ge.X.shape[0] != adata_sp.X.shape[0]:
        raise ValueError(f"adata_ge has {adata_ge.X.shape[0]} spots, adata_sp has {adata_sp.X.shape[0]}")
    n_spots, n = int(adata_sp.X.shape[0]), len(overlap_genes)
    dev = torch.device(device)
    ge = GeneBlocks(adata_ge.X, _columns_of(adata_ge.var, overlap_genes, "adata_ge"), dev)
    sp_ = GeneBlocks(adata_sp.X, _columns_of(adata_sp.var, overlap_genes, "adata_sp"), dev)
    dev = ge.device
    kb = max(1, min(int(gene_block), n))
    scores = torch.empty(n, dtype=torch.float64, device=dev)
    if n:
        scorer = GeneScorer(n_spots, kb, dev)
        pred, meas = (torch.empty((n_spots, kb), dtype=torch.float32, device=dev) for _ in range(2))
        for k0 in range(0, n, kb):
            kc = min(kb, n - k0)
            scorer.score_into(ge.fill(k0, kc, pred), sp_.fill(k0, kc, meas), scores[k0:k0 + kc])
    return _score_frame(scores.cpu().numpy(), overlap_genes, adata_ge.var, adata_sp, adata_sc, genes)


class _Route:
    """The route `project_genes` and `score_genes` take from their keywords, stated once: the mapping resident in HBM (`mapper=`, on
    a spot-sharded run gathered across the ranks), a dense `adata_map.X` through an engine of its own, or the sparse `adata_map.X`
    itself (`truncated=True`).  `project(S)` -> [n_spots, n_genes] float32 device tensor for S [n_cells, n_genes]: a host array, a
    scipy-sparse matrix or a device block; `device`, `n_spots`; `release()` frees the engine made for a dense `adata_map.X`."""

    def __init__(self, adata_map, n_cells, mapper, truncated, device, gemm_precision):
        self._rows = self._engine = None
        if truncated:
            if mapper is not None:
                raise ValueError("truncated=True projects the sparse adata_map.X itself: it cannot be combined with mapper=")
            if not hasattr(adata_map.X, "tocsr"):
                raise ValueError("truncated=True needs a sparse adata_map.X (the top_k= result); a dense mapping is projected without it")
            from .sparse_project import SparseMap
            sm = SparseMap(adata_map.X, device, n_cells=n_cells)                      # :366, no renormalisation
            self.device, self.n_spots, self._project, self._sm, self._out = sm.device, sm.n_spots, self._truncated, sm, None
            return
        if mapper is None:
            if hasattr(adata_map.X, "tocsr"):
                raise ValueError("adata_map.X is sparse (map_cells_to_space(..., top_k=k) keeps each cell's k most probable spots only): "
                                 "project with the trained mapping instead -- map with keep_mapper=True and pass "
                                 "mapper=adata_map._tangram_amd_mapper -- or project the truncated matrix itself with truncated=True")
            engine, rows = _projection_engine(adata_map, torch.device(device), gemm_precision)
            self._engine = engine
            if np.abs(rows - 1.0).max() > 1e-6:                                       # not row-stochastic: P^T S = (P / r)^T (r S)
                self._rows = rows
            self._project = lambda S: engine.project_genes(S, unfiltered=True)
        else:
            # the trained mapper projects through its own seam: on a spot-sharded run that gathers every rank's block of spots
            # (mapper._engine alone is only the LOCAL shard); MapperConstrained: softmax(M) without the filter, like adata_map.X
            from .mapping_optimizer import MapperConstrained
            engine = mapper._engine
            kw = dict(unfiltered=True) if isinstance(mapper, MapperConstrained) else {}
            self._project = lambda S: mapper.project_genes_device(S, **kw)
        self.device, self.n_spots = engine.device, engine.V
        if engine.C != n_cells:
            self.release()
            raise ValueError("The two AnnDatas need to have same `obs` index.")

    def project(self, S):
        if self._rows is not None:                       # the float32 value times the float64 row sum, rounded to float32 once
            if hasattr(S, "tocsr") and not isinstance(S, torch.Tensor):
                import scipy.sparse as sp
                S = (sp.diags(self._rows) @ S.tocsr()).tocsr()
            else:
                S = torch.as_tensor(S).to(device=self.device, dtype=torch.float32)
                S = (S.double() * torch.as_tensor(self._rows, device=self.device)[:, None]).float()
        return self._project(S)

    def _truncated(self, S):
        sm = self._sm
        if not (isinstance(S, torch.Tensor) and S.device == sm.device):
            return sm.project(S)
        kc = int(S.shape[1])                             # a device block (score_genes): the scratch is reused
        if self._out is None or self._out.shape[1] < kc:
            self._out = torch.empty((sm.n_spots, kc), dtype=torch.float32, device=sm.device)
        return sm.project_into(S, self._out[:, :kc])

    def release(self):
        if self._engine is not None:
            self._engine.release()
            self._engine = None


class _ShardRoute:
    """The route of `score_genes(..., distributed=True)`: `project(S)` is THIS rank's block of spots only, [hi - lo, n_genes]
    (the engine's `project_genes` on the rank's own logits; nothing is gathered); `rows` = (lo, hi) of `shard_bounds`, `n_spots` the
    total, `comm` the mapper's communicator."""

    def __init__(self, mapper, n_cells):
        from .sharded import shard_bounds
        sh = mapper._sharded
        engine = sh.eng
        self.device, self.n_spots, self.comm = engine.device, int(sh.n_spots_total), sh.pycomm
        self.rows = shard_bounds(self.n_spots, sh.world, sh.rank, sh.spatial)
        if engine.C != n_cells:
            raise ValueError("The two AnnDatas need to have same `obs` index.")
        sh.checked()
        self._project = lambda S: engine.project_genes(S, unfiltered=True)      # softmax(M) without the filter, like adata_map.X

    def project(self, S):
        return self._project(S)

    def release(self):
        pass


def score_genes(adata_map, adata_sc, adata_sp, cluster_label=None, scale=True, genes=None, *, mapper=None, truncated=False,
                device="cuda:0", gemm_precision="bf16x3", gene_block=1024, distributed=False):
    """`compare_spatial_geneexp(project_genes(adata_map, adata_sc, cluster_label, scale, ...), adata_sp, adata_sc, genes)` without the
    projected plane: the same DataFrame (index, columns, `is_training`, sparsities, order), but no spots x genes array ever exists on
    the host and none wider than `gene_block` genes on the device.  `adata_sc` is prepared as project_genes prepares it; only the
    scored genes -- `adata_sc.uns["overlap_genes"]`, or `genes` -- are projected: block by block their columns of the single-cell
    matrix are gathered on the device (a dense matrix is uploaded once; a scipy-sparse one as CSR), projected by the route the
    keywords select exactly as in project_genes (`mapper=`: the mapping resident in HBM; a dense `adata_map.X`; `truncated=True`: the
    sparse `adata_map.X` itself; the same ValueErrors), and scored against the same genes of `adata_sp.X` (tg_gene_scores), the
    scratch reused.  A spot-sharded mapper is refused with a ValueError unless `distributed=True`.
    `distributed=True` (the keyword of `Mapper` and `map_cells_to_space`; collective: every rank makes the same call with the same
    full `adata_sc` / `adata_sp` and its own spot-sharded `mapper`): per block of genes a rank projects onto its OWN spots only,
    scores them against its own rows `lo:hi` of `adata_sp.X` (`shard_bounds`), and the ranks exchange `[3, gene_block]` doubles -- the
    local dot products and squared norms, summed in rank order on every rank (tg_gene_scores_merge).  Every rank returns the same
    DataFrame; no rank holds a plane taller than its own spots.  ValueError with a mapper that is not spot-sharded or with
    `truncated=True`."""
    from . import preprocess as pre
    from .gene_score import GeneBlocks, GeneScorer, ShardedGeneScorer
    adata_sc_p, S_all = _prepare_sc(adata_map, adata_sc, cluster_label, scale)
    n_cells = int(S_all.shape[0])
    sharded = mapper is not None and getattr(mapper, "_sharded", None) is not None
    if distributed:
        if truncated or not sharded:
            raise ValueError("score_genes(distributed=True) scores over the spot shards of a mapper made with distributed=True: pass that "
                             "mapper as mapper=, without truncated=True")
        route = _ShardRoute(mapper, n_cells)
    else:
        if sharded and not truncated:
            raise ValueError("score_genes does not take a spot-sharded mapper without distributed=True: every rank holds the moments of its "
                             "own spots only; pass distributed=True on every rank (the ranks then exchange the moments), or project "
                             "with project_genes and score with compare_spatial_geneexp")
        route = _Route(adata_map, n_cells, mapper, truncated, device, gemm_precision)
    dev, n_spots = route.device, route.n_spots
    lo, hi = route.rows if distributed else (0, n_spots)
    try:
        overlap_genes = _check_score_inputs(adata_sc_p.uns, adata_sp, genes)
        mu.annotate_gene_sparsity(adata_sp)
        if n_spots != adata_sp.X.shape[0]:
            raise ValueError(f"the mapping has {n_spots} spots, adata_sp has {adata_sp.X.shape[0]}")
        var_ge = adata_sc_p.var.copy()
        var_ge["is_training"] = var_ge.index.isin(adata_map.uns["train_genes_df"].index.values)
        idx_sc = _columns_of(var_ge, overlap_genes, "adata_sc")
        X_sp = adata_sp.X[lo:hi] if distributed else adata_sp.X                      # a shard measures against its own rows only
        sp_ = GeneBlocks(X_sp, _columns_of(adata_sp.var, overlap_genes, "adata_sp"), dev)
        n = len(overlap_genes)
        kb = max(1, min(int(gene_block), n))
        scores = torch.empty(n, dtype=torch.float64, device=dev)
        if n:
            sparse_s = hasattr(S_all, "tocsr")
            S_dev = pre.DeviceCSR(S_all, dev) if sparse_s else torch.as_tensor(S_all).to(device=dev, dtype=torch.float32)
            scorer = ShardedGeneScorer(hi - lo, kb, route.comm, dev) if distributed else GeneScorer(n_spots, kb, dev)
            meas = torch.empty((hi - lo, kb), dtype=torch.float32, device=dev)
            for k0 in range(0, n, kb):
                kc = min(kb, n - k0)
                cols = idx_sc[k0:k0 + kc]
                if sparse_s:
                    S_blk = pre.gather_training_genes(S_dev, cols, dev)
                else:
                    S_blk = S_dev.index_select(1, torch.as_tensor(cols, dtype=torch.int64, device=dev))
                scorer.score_into(route.project(S_blk), sp_.fill(k0, kc, meas), scores[k0:k0 + kc])
        scores = scores.cpu().numpy()
    finally:
        route.release()
    return _score_frame(scores, overlap_genes, var_ge, adata_sp, adata_sc, genes)
