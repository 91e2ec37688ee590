"""Genes projected from a sparse top-k mapping (tg_sparse.h) at the BASELINE config-2 shape, 30 000 cells x 10 000 spots, k = 8, the
matrix taken from `result_topk` of a mapper after a few trained steps; dense S of 1 000 and of 26 496 genes.  Prints ONE JSON line:

    build_ms / project_ms            device time of tg_sparse_map_build / tg_sparse_map_project into preallocated buffers (HIP events,
                                     min and median after warm-up)
    copy_ceiling_fraction            (4 nnz n_genes + 4 V n_genes) bytes over the median projection time, against the 6.29 TB/s copy
                                     ceiling of DESIGN.md
    dense_project_ms                 tg_mapper_project_genes of the same genes with the mapper resident, same run
    sparse_end_to_end_ms             wall clock: upload of the CSR arrays + build + projection, S resident on the device, synchronised
    sparse_from_host_ms              ... + the upload of S and the copy of the result to a NumPy array (what project_genes pays)
    host_scipy_ms                    wall clock of `X.T @ S` in scipy on the host

    python scripts/bench_sparse_project.py [--cells 30000] [--spots 10000] [--train-genes 1000] [--k 8] [--genes 1000 26496]
                                           [--reps 10] [--out profiles/sparse_project/bench_sparse_project.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tangram_amd import _capi                               # noqa: E402
from tangram_amd.device_init import device_normal          # noqa: E402
from tangram_amd.engine import HipMapperEngine             # noqa: E402
from tangram_amd.sparse_project import SparseMap           # noqa: E402

COPY_CEILING = 6.29e12                                      # bytes / s


def device_ms(fn, dev, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize(dev)
        ms.append(t0.elapsed_time(t1))
    return round(min(ms), 4), round(statistics.median(ms), 4)


def wall_ms(fn, dev, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ms.append(1e3 * (time.perf_counter() - t0))
    return round(min(ms), 3), round(statistics.median(ms), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=30000)
    ap.add_argument("--spots", type=int, default=10000)
    ap.add_argument("--train-genes", type=int, default=1000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--genes", type=int, nargs="+", default=[1000, 26496])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    C, V, K, k = a.cells, a.spots, a.train_genes, a.k
    g = torch.Generator(device="cpu").manual_seed(1)
    S_train = torch.rand((C, K), generator=g).to(dev)
    G = torch.rand((V, K), generator=g).to(dev)
    eng = HipMapperEngine(S_train, G, device_normal(C, V, dev, 7), device=dev, precision="bf16x3")
    eng.step(a.steps, 0.1)
    val, idx = (x.cpu().numpy() for x in eng.result_topk(k))
    order = np.argsort(idx, axis=1)
    X = sp.csr_matrix((np.take_along_axis(val, order, 1).ravel(), np.take_along_axis(idx, order, 1).ravel().astype(np.int32),
                       np.arange(0, C * k + 1, k, dtype=np.int64)), shape=(C, V))
    nnz = int(X.nnz)
    per_spot = np.bincount(X.indices, minlength=V)
    lib = _capi.lib()
    sm = SparseMap(X, dev)
    indptr, indices, data = sm._csr_dev
    stream = eng._hip_stream
    build = lambda: _capi.check(lib.tg_sparse_map_build(indptr.data_ptr(), indices.data_ptr(), data.data_ptr(), C, V, nnz,      # noqa: E731
                                                        sm.workspace.data_ptr(), stream))
    out = dict(cells=C, spots=V, k=k, nnz=nnz, entries_per_spot_median=int(np.median(per_spot)), entries_per_spot_max=int(per_spot.max()),
               steps=a.steps, reps=a.reps, device=torch.cuda.get_device_name(dev), mapper_genes=K)
    out["build_ms_min"], out["build_ms"] = device_ms(build, dev, a.warmup, a.reps)
    for n in a.genes:
        S_host = np.random.default_rng(n).random((C, n), dtype=np.float32)
        S = torch.as_tensor(S_host, device=dev)
        res = torch.empty((V, n), dtype=torch.float32, device=dev)
        r = {}
        r["project_ms_min"], r["project_ms"] = device_ms(lambda: sm.project_into(S, res), dev, a.warmup, a.reps)
        nbytes = 4 * nnz * n + 4 * V * n
        r["algorithmic_bytes"] = nbytes
        r["copy_ceiling_fraction"] = round(nbytes / (1e-3 * r["project_ms"]) / COPY_CEILING, 4)
        dense_out = torch.empty((V, n), dtype=torch.float32, device=dev)
        dense = lambda: eng._call(lib.tg_mapper_project_genes, eng._h, S.data_ptr(), int(S.stride(0)), n, dense_out.data_ptr(), n, 1)  # noqa: E731
        r["dense_project_ms_min"], r["dense_project_ms"] = device_ms(dense, dev, 1, a.reps)
        r["sparse_end_to_end_ms_min"], r["sparse_end_to_end_ms"] = wall_ms(lambda: SparseMap(X, dev).project_into(S, res), dev, 1, a.reps)
        r["sparse_from_host_ms_min"], r["sparse_from_host_ms"] = wall_ms(lambda: SparseMap(X, dev).project(S_host).cpu().numpy(), dev, 1,
                                                                         a.host_reps)
        ms = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            ref = X.T @ S_host
            ms.append(1e3 * (time.perf_counter() - t0))
        r["host_scipy_ms_min"], r["host_scipy_ms"] = round(min(ms), 3), round(statistics.median(ms), 3)
        r["device_path_faster_than_host"] = bool(r["sparse_from_host_ms"] < r["host_scipy_ms"])
        got = sm.project(S).cpu().numpy()
        r["max_abs_diff_vs_host"] = float(np.abs(got - ref).max())
        r["max_dense_minus_sparse"] = float((dense_out.cpu().numpy() - got).max())
        out[f"genes_{n}"] = r
        del S, res, dense_out, got, ref, S_host
        torch.cuda.empty_cache()
    eng.release()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
