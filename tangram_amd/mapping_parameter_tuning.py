"""
The tuning trial of `tangram.mapping_parameter_tuning` (reference: tangram/mapping_parameter_tuning.py:42-139) on the device.

A trial trains `n_runs` mappings of one problem from different seeds and reports how well they agree:

    cell_map_consistency    mean pairwise Pearson correlation of the mapping matrices
    cell_map_agreement      1 - mean normalized vote entropy (do the runs send a cell to the same spot?)
    cell_map_certainty      1 - mean normalized consensus entropy (how peaked is the mean mapping of a cell?)
    gene_expr_consistency   mean pairwise Pearson correlation of the projected validation genes
    gene_expr_correctness   mean validation gene score of the runs

The reference stacks the `n_runs` C x V mapping matrices on the host and runs NumPy over the cube.  Here the logits of all runs are
still resident when the question is asked: one pass over them (tg_mapper_consistency, csrc/tg_consist.h) gives the correlations,
the votes and both entropies per cell; nothing C x V is written or copied.  The three metric functions keep the reference's
names, arguments and return shapes and run through the same kernel on plain planes (tg_planes_consistency).

Spot-sharded mappers (all of one group) are answered from per-rank packets merged in rank order (tg_mapper_consistency_shard,
tg_consistency_merge): collective, the same bits on every rank, nothing cells x spots gathered.

Differences to the reference, all of them documented where they occur: values are float32 on the device (a float64 cube is
cast), `pearson_corr` of a single run raises instead of returning an empty array, and `train_multiple_Mapper` RETURNS the metrics
(the reference hands them to `ray.train.report`; wrap the call for a ray trial).
"""
from __future__ import annotations

import ctypes as ct

import numpy as np
import torch

from . import _capi
from ._device import call, check_device, stream, workspace

METRICS = ("cell_map_consistency", "cell_map_agreement", "cell_map_certainty", "gene_expr_consistency", "gene_expr_correctness")
_FLAT_COLS = 8192          # row length `pearson_corr` re-cuts narrow contiguous planes to (a row is one workgroup's work)


def _device_of(x, device):
    if device is not None:
        return torch.device(device)
    for t in (x if isinstance(x, (list, tuple)) else [x]):
        if isinstance(t, torch.Tensor):
            return t.device
    return torch.device("cpu" if _capi.is_emulated() else "cuda:0")


def _planes(cube, device):
    """`cube` (r, i, j) -- a host array, a device tensor or a list of r planes -- as r float32 device tensors [i, j] with unit
    column stride and one common row pitch."""
    dev = check_device(_device_of(cube, device))
    if isinstance(cube, (list, tuple)):
        planes = [p if isinstance(p, torch.Tensor) else torch.as_tensor(np.asarray(p, dtype=np.float32)) for p in cube]
    else:
        if not isinstance(cube, torch.Tensor):
            cube = torch.as_tensor(np.ascontiguousarray(np.asarray(cube, dtype=np.float32)))
        if cube.dim() != 3:
            raise ValueError("cube must be (runs, i, j)")
        cube = cube.to(device=dev, dtype=torch.float32)
        planes = [cube[r] for r in range(cube.shape[0])]
    if not planes:
        raise ValueError("cube holds no run")
    planes = [p.detach().to(device=dev, dtype=torch.float32) for p in planes]
    if any(p.dim() != 2 or p.shape != planes[0].shape for p in planes):
        raise ValueError("the planes of a cube must be two-dimensional and of one shape")
    if any(p.stride(1) != 1 or p.stride(0) != planes[0].stride(0) or p.stride(0) < p.shape[1] for p in planes):
        planes = [p.contiguous() for p in planes]
    return planes, dev


def planes_consistency(planes, pearson=True, vote=True, consensus=True, votes=False, device=None, _max_parts=None):
    """One pass of tg_planes_consistency over r planes [i, j] (see `_planes` for what a cube may be).  Returns a dict of device
    tensors: "pearson" float64 [r (r - 1) / 2] (pairs in the order of np.tril_indices(r, -1); absent when r = 1), "vote_entropy" and
    "consensus_entropy" float32 [i], "votes" int32 [r, i] -- those that were asked for.  (`_max_parts`, for the tests: the same pass with at
    most that many workgroups, tg_debug_planes_consistency.)"""
    planes, dev = _planes(planes, device)
    lib = _capi.lib()
    r = len(planes)
    n_rows, n_cols = (int(x) for x in planes[0].shape)
    ws = workspace(lib.tg_consistency_query_bytes, r, n_rows, device=dev, min_bytes=8)
    out = {}
    if pearson and r > 1:
        out["pearson"] = torch.empty(r * (r - 1) // 2, dtype=torch.float64, device=dev)
    if vote:
        out["vote_entropy"] = torch.empty(n_rows, dtype=torch.float32, device=dev)
    if consensus:
        out["consensus_entropy"] = torch.empty(n_rows, dtype=torch.float32, device=dev)
    if votes:
        out["votes"] = torch.empty((r, n_rows), dtype=torch.int32, device=dev)
    ptr = lambda k: out[k].data_ptr() if k in out else None
    arr = (ct.c_void_p * r)(*[p.data_ptr() for p in planes])
    fn, tail = (lib.tg_planes_consistency, ()) if _max_parts is None else (lib.tg_debug_planes_consistency, (int(_max_parts),))
    call(dev, fn, arr, r, n_rows, n_cols, int(planes[0].stride(0)), ws.data_ptr(), ptr("pearson"), ptr("vote_entropy"),
         ptr("consensus_entropy"), ptr("votes"), stream(dev), *tail)
    return out


def _flat(planes):
    """Contiguous planes of few columns re-cut into rows of up to `_FLAT_COLS` elements: the rows do not matter to a correlation of
    the flattened planes, and a row is what one workgroup streams.  Planes whose element count has no such divisor stay as they are;
    one-column planes (a single validation gene), which the kernel does not take, then become ONE row of all their elements --
    correct for any count the library accepts, slow for a large one (a single workgroup streams it)."""
    i, j = (int(x) for x in planes[0].shape)
    n = i * j
    if j >= _FLAT_COLS:
        return planes
    if not all(p.is_contiguous() for p in planes):
        if j >= 2:
            return planes
        planes = [p.contiguous() for p in planes]
    for cols in range(min(n, _FLAT_COLS), max(j, 2), -1):
        if n % cols == 0:
            return [p.view(n // cols, cols) for p in planes]
    return planes if j >= 2 else [p.view(1, n) for p in planes]


def pearson_corr(cube, device=None):
    """All pairwise Pearson correlations of the runs of `cube` (r, n, j), each run flattened: float64 ndarray [r (r - 1) / 2] in the
    order of np.tril_indices(r, -1), like the reference (:42-53).  Moments and sums are fp64 on the device; the values are the
    float32 of the cube.  r = 1 has no pair: ValueError (the reference returns an empty array, whose mean is NaN)."""
    planes, dev = _planes(cube, device)
    if len(planes) < 2:
        raise ValueError("pearson_corr needs at least two runs")
    out = planes_consistency(_flat(planes), pearson=True, vote=False, consensus=False, device=dev)
    return out["pearson"].cpu().numpy()


def vote_entropy(pred_probs_cube, device=None):
    """Normalized vote entropy across the last axis of `pred_probs_cube` (r, i, j): float64 ndarray [i] (:55-69)."""
    out = planes_consistency(pred_probs_cube, pearson=False, vote=True, consensus=False, device=device)
    return out["vote_entropy"].cpu().numpy().astype(np.float64)


def consensus_entropy(pred_probs_cube, device=None):
    """Normalized entropy of the mean over the runs across the last axis of `pred_probs_cube` (r, i, j): float64 ndarray [i] (:71-82)."""
    out = planes_consistency(pred_probs_cube, pearson=False, vote=False, consensus=True, device=device)
    return out["consensus_entropy"].cpu().numpy().astype(np.float64)


def _engine_of(m):
    if getattr(m, "_sharded", None) is not None:
        return m._sharded.eng
    return getattr(m, "_engine", m)


def _shard_group(mappers):
    """None for mappers that hold every spot; the first mapper's ShardedMapperEngine when ALL are spot shards.  Mixed: ValueError."""
    if not mappers:
        raise ValueError("no mapper")
    sharded = [getattr(m, "_sharded", None) for m in mappers]
    if all(s is None for s in sharded):
        return None
    if any(s is None for s in sharded):
        raise ValueError("mapping_consistency takes mappers that are all spot-sharded over one group or all unsharded, not a mixture")
    s0 = sharded[0]
    if any(s.world != s0.world or s.rank != s0.rank or s.n_spots_total != s0.n_spots_total for s in sharded):
        raise ValueError("spot-sharded mappers must be shards of one group: the same world, rank and total number of spots")
    return s0


def _gather_packets(sh, packet):
    """The ranks' packets (int64 device tensors of one length) side by side, in rank order: [world, len]."""
    every = torch.empty((sh.world, packet.numel()), dtype=torch.int64, device=packet.device)
    sh.pycomm.all_gather(list(every.unbind(0)), packet)
    return every


def _merge(lib, dev, every, r, n_rows, n_cols_total, n_elem, out):
    ptr = lambda k: out[k].data_ptr() if k in out else None
    call(dev, lib.tg_consistency_merge, every.data_ptr(), int(every.shape[0]), r, n_rows, int(every.stride(0)) * 8, int(n_cols_total), int(n_elem),
         ptr("pearson"), ptr("vote_entropy"), ptr("consensus_entropy"), ptr("votes"), stream(dev))
    return out


def _sharded_mapper_consistency(sh, engines, votes):
    """Collective: every rank reduces its own block of spots to a packet (tg_mapper_consistency_shard), the packets are gathered once
    through the group's Python communicator, and every rank merges them in rank order (tg_consistency_merge)."""
    e0 = engines[0]
    lib, dev, r, C = e0._lib, e0.device, len(engines), int(e0.C)
    sh.checked()
    ws = workspace(lib.tg_consistency_query_bytes, r, C, device=dev, min_bytes=8)
    nbytes = ct.c_size_t()
    _capi.check(lib.tg_consistency_packet_bytes(r, C, ct.byref(nbytes)))
    packet = torch.empty(nbytes.value // 8, dtype=torch.int64, device=dev)
    arr = (ct.c_void_p * r)(*[e._h for e in engines])
    e0._call(lib.tg_mapper_consistency_shard, arr, r, ws.data_ptr(), packet.data_ptr(), tensors=(ws, packet))
    every = _gather_packets(sh, packet)
    out = {"vote_entropy": torch.empty(C, dtype=torch.float32, device=dev),
           "consensus_entropy": torch.empty(C, dtype=torch.float32, device=dev)}
    if r > 1:
        out["pearson"] = torch.empty(r * (r - 1) // 2, dtype=torch.float64, device=dev)
    if votes:
        out["votes"] = torch.empty((r, C), dtype=torch.int32, device=dev)
    V = int(sh.n_spots_total)
    return _merge(lib, dev, every, r, C, V, C * V, out)


def sharded_planes_pearson(planes_local, comm_owner, n_rows_total):
    """Pairwise Pearson correlations of r planes whose ROWS are spread over the ranks (collective): planes_local are this rank's
    [rows_local, j] blocks; the moments of the flattened planes are additive over row blocks, so every rank reduces its block
    (tg_planes_consistency_shard, moments only), the sums are gathered and merged in rank order -> float64 device tensor
    [r (r - 1) / 2], the same bits on every rank.  `comm_owner`: a ShardedMapperEngine (its `pycomm`, `world`)."""
    planes, dev = _planes(planes_local, None)
    r = len(planes)
    if r < 2:
        raise ValueError("pearson_corr needs at least two runs")
    lib = _capi.lib()
    j = int(planes[0].shape[1])
    planes = _flat(planes)
    n_rows, n_cols = (int(x) for x in planes[0].shape)
    ws = workspace(lib.tg_consistency_query_bytes, r, n_rows, device=dev, min_bytes=8)
    nbytes = ct.c_size_t()
    _capi.check(lib.tg_consistency_packet_bytes(r, 0, ct.byref(nbytes)))
    packet = torch.empty(nbytes.value // 8, dtype=torch.int64, device=dev)
    arr = (ct.c_void_p * r)(*[p.data_ptr() for p in planes])
    call(dev, lib.tg_planes_consistency_shard, arr, r, n_rows, n_cols, int(planes[0].stride(0)) if n_rows > 1 else max(int(planes[0].stride(0)), n_cols),
         max(j, 2), 0, 0, ws.data_ptr(), packet.data_ptr(), stream(dev))
    every = _gather_packets(comm_owner, packet)
    out = {"pearson": torch.empty(r * (r - 1) // 2, dtype=torch.float64, device=dev)}
    return _merge(lib, dev, every, r, 0, max(j, 2), int(n_rows_total) * j, out)["pearson"]


def mapper_consistency(mappers, votes=False):
    """tg_mapper_consistency over trained mappers (or engines) whose logits are resident: dict of device tensors like
    `planes_consistency`, of the mappings softmax(M) -- the bits `result()` would hold, which is never formed.
    Mappers that all carry `_sharded` from one group (spot shards): collective, every rank gets the same outputs for ALL spots, votes as
    global spot indices; no rank reads anything but its own logits.  Mixing sharded and unsharded mappers raises ValueError."""
    mappers = list(mappers)
    sh = _shard_group(mappers)
    engines = [_engine_of(m) for m in mappers]
    if sh is not None:
        return _sharded_mapper_consistency(sh, engines, votes)
    e0 = engines[0]
    lib, dev, r = e0._lib, e0.device, len(engines)
    ws = workspace(lib.tg_consistency_query_bytes, r, e0.C, device=dev, min_bytes=8)
    out = {"vote_entropy": torch.empty(e0.C, dtype=torch.float32, device=dev),
           "consensus_entropy": torch.empty(e0.C, dtype=torch.float32, device=dev)}
    if r > 1:
        out["pearson"] = torch.empty(r * (r - 1) // 2, dtype=torch.float64, device=dev)
    if votes:
        out["votes"] = torch.empty((r, e0.C), dtype=torch.int32, device=dev)
    ptr = lambda k: out[k].data_ptr() if k in out else None
    arr = (ct.c_void_p * r)(*[e._h for e in engines])
    e0._call(lib.tg_mapper_consistency, arr, r, ws.data_ptr(), ptr("pearson"), ptr("vote_entropy"), ptr("consensus_entropy"), ptr("votes"),
             tensors=(ws,) + tuple(out.values()))
    return out


def mapping_consistency(mappers, S_val=None):
    """The consistency metrics of trained mappers of one problem (created on one stream, logits resident):

        cell_map_consistency = mean(pearson), cell_map_agreement = 1 - mean(vote entropy), cell_map_certainty = 1 - mean(consensus
        entropy) -- one pass over the logits; the means are taken in float64 on the host from the small outputs;
        gene_expr_consistency (with `S_val` [n_cells, n_val], host or device): mean pairwise Pearson correlation of the runs'
        projections softmax(M)^T S_val ([n_spots, n_val], `engine.project_genes`, at the mapper's gemm precision).

    Nothing of size cells x spots is written or copied.  A single mapper has no pair: its consistencies are NaN.
    Spot-sharded mappers (all of them, one group; collective): the same numbers on every rank; `gene_expr_consistency` from each
    rank's own [local_spots, n_val] projections, nothing gathered but a few sums."""
    mappers = list(mappers)
    out = mapper_consistency(mappers)
    sh = _shard_group(mappers)
    nan = float("nan")
    res = {"cell_map_consistency": float(out["pearson"].cpu().numpy().mean()) if "pearson" in out else nan,
           "cell_map_agreement": float(1.0 - out["vote_entropy"].cpu().numpy().astype(np.float64).mean()),
           "cell_map_certainty": float(1.0 - out["consensus_entropy"].cpu().numpy().astype(np.float64).mean())}
    if S_val is not None:
        engines = [_engine_of(m) for m in mappers]
        if len(engines) > 1:
            S_val = S_val if hasattr(S_val, "tocsr") else torch.as_tensor(S_val).to(device=engines[0].device, dtype=torch.float32)
            proj = [e.project_genes(S_val) for e in engines]
            if sh is not None:
                res["gene_expr_consistency"] = float(sharded_planes_pearson(proj, sh, sh.n_spots_total).cpu().numpy().mean())
            else:
                res["gene_expr_consistency"] = float(pearson_corr(proj).mean())
        else:
            res["gene_expr_consistency"] = nan
    return res


def _train_together(mappers, num_epochs, learning_rate):
    """Advance all mappers `num_epochs` steps: in one `MapperBatch` when they can share one, else one after the other.  No per-epoch
    validation, no result: the logits stay where they are."""
    from .batched import MapperBatch, _batch_key
    keys = [_batch_key(m) for m in mappers]
    if len(mappers) > 1 and keys[0] is not None and all(k == keys[0] for k in keys):
        try:
            batch = MapperBatch(mappers)
        except (RuntimeError, ValueError):          # refused by tg_batch_create: nothing has been stepped
            batch = None
        if batch is not None:
            batch.step(num_epochs, learning_rate, batch.new_histories(max(num_epochs, 1)), 0)
            batch.close()
            return
    for m in mappers:
        e = m._engine
        e.step(num_epochs, learning_rate, e.new_history(max(num_epochs, 1)), 0)


def train_multiple_Mapper(config, data, n_runs=3):
    """One tuning trial (:86-139): `n_runs` Mappers of the problem in `data`, seeds 0 .. n_runs - 1, trained with the hyperparameters
    in `config`; returns {metric: float} for the five METRICS.

    data:   the reference's 12-tuple (S, G, d_source, d, device, print_each, voxel_weights, ct_encode, neighborhood_filter,
            spatial_weights, train_genes_idx, val_genes_idx); `print_each` is ignored (nothing is printed per epoch).
    config: any of lambda_d, lambda_g1, lambda_g2, lambda_neighborhood_g1, lambda_r, lambda_l1, lambda_l2, lambda_ct_islands,
            lambda_getis_ord, plus learning_rate (default 0.1) and num_epochs (default 1000), as in the reference.

    The mappers are built one after the other on the calling thread (`random_state=run` seeds NumPy's global stream; seed 0 is
    "unseeded" as in the reference) and trained together in a `MapperBatch` where they can share one.  The reference validates
    every epoch and reads the last value only: validation is a function of the logits, so ONE validation per run after the last
    step gives `val_gene_sim[-1]`, bit for bit.  No dense mapping is formed and nothing C x V reaches the host."""
    from .mapping_optimizer import Mapper
    S, G, d_source, d, device, print_each, voxel_weights, ct_encode, neighborhood_filter, spatial_weights, train_genes_idx, val_genes_idx = data
    hyperparameters = {"d_source": d_source}
    for param in ("lambda_d", "lambda_g1", "lambda_g2", "lambda_neighborhood_g1", "lambda_r", "lambda_l1", "lambda_l2", "lambda_ct_islands",
                  "lambda_getis_ord"):
        if param in config:
            hyperparameters[param] = config[param]
    learning_rate = config.get("learning_rate", 0.1)
    num_epochs = int(config.get("num_epochs", 1000))
    mappers = []
    try:
        for run in range(int(n_runs)):
            mappers.append(Mapper(S=S, G=G, d=d, train_genes_idx=train_genes_idx, val_genes_idx=val_genes_idx, voxel_weights=voxel_weights,
                                  neighborhood_filter=neighborhood_filter, ct_encode=ct_encode, spatial_weights=spatial_weights,
                                  device=device, random_state=run, **hyperparameters))
        _train_together(mappers, num_epochs, learning_rate)
        val_gene_scores = [m._engine.validate()[1] for m in mappers]                    # val_gene_sim of the trained mapping
        S_all = S if isinstance(S, torch.Tensor) else np.asarray(S, dtype=np.float32)
        S_val = S_all if val_genes_idx is None else S_all[:, val_genes_idx]
        res = mapping_consistency(mappers, S_val)
        res["gene_expr_correctness"] = float(np.array(val_gene_scores).mean())
    finally:
        for m in mappers:
            m.release()
    return {k: res[k] for k in METRICS}
