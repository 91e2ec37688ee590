"""Per-gene cosine scores of a predicted against a measured spots x genes plane on the device (csrc/tg_score.h, tg_gene_scores):
what `compare_spatial_geneexp` computes with one `np.linalg.norm` pair per gene on the host (reference tangram/utils.py:424-426).

  gene_scores     score[j] = <pred[:, j], meas[:, j]> / (|pred[:, j]| |meas[:, j]|) for two planes of equal shape, float64; optionally the
                  three moments (dot, |pred|^2, |meas|^2) they are made of
  GeneScorer      the workspace and outputs of planes of one height, reused block of genes by block of genes
  gene_scores_sharded / ShardedGeneScorer   the same over planes whose spots are spread over the ranks of a communicator: local
                  moments, one all-gather of [3, n_genes] doubles, a merge in rank order (tg_gene_scores_merge)
  GeneBlocks      selected gene columns of an AnnData matrix (dense or scipy-sparse) as dense float32 device blocks

Every element is converted to double, products and sums are fp64 in an order that depends on the number of spots alone: a column
gives the same bits in any block of any call.  Everything goes through the C ABI; torch only owns the memory.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from ._device import call, check_device, pitch, stream, workspace
from .preprocess import DeviceCSR


def _plane(x, device, name):
    x = torch.as_tensor(x) if not isinstance(x, torch.Tensor) else x
    if x.dim() != 2:
        raise ValueError(f"{name} must be a [n_spots, n_genes] matrix")
    x = x.to(device=device, dtype=torch.float32)
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    return x


class GeneScorer:
    """Scores planes of `n_spots` rows and at most `max_genes` columns on `device`; nothing is allocated per call."""

    def __init__(self, n_spots, max_genes, device):
        self.device = check_device(device)
        self.n_spots, self.max_genes = int(n_spots), int(max_genes)
        self.workspace = workspace(_capi.lib().tg_gene_scores_query_bytes, self.n_spots, self.max_genes, device=self.device)

    def score_into(self, pred, meas, score=None, moments=None):
        """pred, meas: float32 [n_spots, n] device tensors with unit column stride (views with a pitch are taken as they are);
        score: float64 [n] or None, moments: contiguous float64 [3, n] or None (not both None), written in place."""
        n = int(pred.shape[1])
        if pred.shape != meas.shape:
            raise ValueError(f"the predicted plane is {tuple(pred.shape)}, the measured one {tuple(meas.shape)}")
        if int(pred.shape[0]) != self.n_spots or n > self.max_genes:
            raise ValueError(f"this scorer takes planes of {self.n_spots} spots x at most {self.max_genes} genes")
        for t, name in ((pred, "pred"), (meas, "meas")):
            if t.dtype != torch.float32 or t.device != self.device or (n > 1 and t.stride(1) != 1):
                raise ValueError(f"{name} must be a float32 tensor on {self.device} with unit column stride")
        for t, shape, name in ((score, (n,), "score"), (moments, (3, n), "moments")):
            if t is not None and (t.dtype != torch.float64 or t.device != self.device or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float64 tensor of shape {shape} on {self.device}")
        call(self.device, _capi.lib().tg_gene_scores, pred.data_ptr() or None, pitch(pred), meas.data_ptr() or None, pitch(meas),
             self.n_spots, n, self.workspace.data_ptr(), moments.data_ptr() if moments is not None else None,
             score.data_ptr() if score is not None else None, stream(self.device))


def gene_scores(pred, meas, *, moments=False, device=None):
    """Cosine score of every gene column of `pred` against the same column of `meas` -> float64 tensor [n_genes] on the device;
    `moments=True`: (scores, moments [3, n_genes] = dot, sum pred^2, sum meas^2).  pred, meas: device tensors or host arrays of equal
    shape [n_spots, n_genes] (taken as float32; views with a row pitch are read in place).  A gene whose predicted or measured column
    is all zero scores NaN, as in the reference.  `device`: default the device of a tensor argument, else cuda:0."""
    if device is None:
        device = next((t.device for t in (pred, meas) if isinstance(t, torch.Tensor) and t.device.type == "cuda"), None)
        if device is None:
            device = next((t.device for t in (pred, meas) if isinstance(t, torch.Tensor)), torch.device("cuda:0"))
    device = check_device(device)
    if tuple(pred.shape) != tuple(meas.shape):
        raise ValueError(f"pred is {tuple(pred.shape)}, meas is {tuple(meas.shape)}: the two planes must have the same shape")
    pred, meas = _plane(pred, device, "pred"), _plane(meas, device, "meas")
    n_spots, n = (int(s) for s in pred.shape)
    scorer = GeneScorer(n_spots, n, device)
    score = torch.empty(n, dtype=torch.float64, device=device)
    mom = torch.empty((3, n), dtype=torch.float64, device=device) if moments else None
    scorer.score_into(pred, meas, score, mom)
    return (score, mom) if moments else score


class ShardedGeneScorer:
    """GeneScorer over spot shards (collective: every rank of `comm` makes the same calls with planes of the same width): this rank
    holds `n_spots_local` rows of both planes.  Per call the rank reduces its rows to moments (tg_gene_scores), the [3, n] doubles of
    all ranks are gathered once through `comm.all_gather(outs, t)`, and every rank merges them in rank order (tg_gene_scores_merge):
    the same bits on every rank, no plane taller than the rank's own spots anywhere."""

    def __init__(self, n_spots_local, max_genes, comm, device):
        self.local = GeneScorer(n_spots_local, max_genes, device)
        self.device, self.max_genes, self.comm, self.world = self.local.device, int(max_genes), comm, int(comm.world)
        self._mine = torch.empty(3 * self.max_genes, dtype=torch.float64, device=self.device)
        self._every = torch.empty(self.world * 3 * self.max_genes, dtype=torch.float64, device=self.device)

    def score_into(self, pred, meas, score=None, moments=None):
        """As GeneScorer.score_into on this rank's rows; `score` [n] and `moments` [3, n] are those of ALL spots."""
        n = int(pred.shape[1])
        if n < 1 or n > self.max_genes:
            raise ValueError(f"this scorer takes planes of 1 to {self.max_genes} genes, not {n} (the same width on every rank)")
        for t, shape, name in ((score, (n,), "score"), (moments, (3, n), "moments")):
            if t is not None and (t.dtype != torch.float64 or t.device != self.device or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float64 tensor of shape {shape} on {self.device}")
        if score is None and moments is None:
            raise ValueError("score and moments are both None")
        mine = self._mine[:3 * n].view(3, n)
        self.local.score_into(pred, meas, None, mine)
        every = self._every[:self.world * 3 * n].view(self.world, 3, n)
        self.comm.all_gather(list(every.unbind(0)), mine)
        call(self.device, _capi.lib().tg_gene_scores_merge, every.data_ptr(), self.world, n, moments.data_ptr() if moments is not None else None,
             score.data_ptr() if score is not None else None, stream(self.device))


def gene_scores_sharded(pred_local, meas_local, comm, moments=False, *, device=None):
    """`gene_scores` of planes whose rows (spots) are spread over the ranks of `comm` (anything with `world` and
    `all_gather(outs, t)`: a ShardedMapperEngine's `pycomm`); collective.  pred_local, meas_local: this rank's rows
    [n_spots_local, n_genes], the same genes on every rank.  Returns on every rank the same float64 device tensor [n_genes] of the
    scores over ALL spots; `moments=True`: (scores, moments [3, n_genes]), each moment the ranks' sums added in rank order."""
    if device is None:
        device = next((t.device for t in (pred_local, meas_local) if isinstance(t, torch.Tensor) and t.device.type == "cuda"), None)
        if device is None:
            device = next((t.device for t in (pred_local, meas_local) if isinstance(t, torch.Tensor)), torch.device("cuda:0"))
    device = check_device(device)
    if tuple(pred_local.shape) != tuple(meas_local.shape):
        raise ValueError(f"pred is {tuple(pred_local.shape)}, meas is {tuple(meas_local.shape)}: the two planes must have the same shape")
    pred, meas = _plane(pred_local, device, "pred"), _plane(meas_local, device, "meas")
    n_spots, n = (int(s) for s in pred.shape)
    scorer = ShardedGeneScorer(n_spots, n, comm, device)
    score = torch.empty(n, dtype=torch.float64, device=device)
    mom = torch.empty((3, n), dtype=torch.float64, device=device) if moments else None
    scorer.score_into(pred, meas, score, mom)
    return (score, mom) if moments else score


class GeneBlocks:
    """The gene columns `idx` (in that order) of the matrix X [n_obs, n_vars] -- dense, or scipy-sparse: then the selection is uploaded
    once as CSR and every block is expanded on the device (DeviceCSR.columns_into).  `fill(k0, kc, out)` writes the columns
    k0 .. k0 + kc of the selection into the float32 device tensor `out[:, :kc]`."""

    def __init__(self, X, idx, device):
        self.device = check_device(device)
        self.idx = np.asarray(idx, dtype=np.int64)
        self.csr = self.dense = None
        if hasattr(X, "tocsr") and not isinstance(X, torch.Tensor):
            self.csr = DeviceCSR(X.tocsr()[:, self.idx], self.device)          # the columns are selected on the host, before the upload
        else:
            self.dense = X

    def fill(self, k0, kc, out):
        view = out[:, :kc]
        if self.dense is not None:
            cols = self.idx[k0:k0 + kc]
            if isinstance(self.dense, torch.Tensor):
                view.copy_(self.dense[:, torch.as_tensor(cols, device=self.dense.device)])
            else:
                view.copy_(torch.as_tensor(np.ascontiguousarray(np.asarray(self.dense)[:, cols], dtype=np.float32)))
        else:
            self.csr.columns_into(k0, kc, out)
        return view
