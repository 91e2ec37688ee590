"""Which cells sit in a spot: each spot's k most probable cells from the logits (tg_spot_topk + tg_topk_merge_rows, V x k pairs)
against the dense result plus a column sort on the host, at the BASELINE config-2 shape, 30 000 cells x 10 000 spots, k = 8.
Prints ONE JSON line:

    spot_topk_device_ms / spot_topk_colsum_device_ms   device time of one call into preallocated buffers, without / with the fp64
                                                       column sums (HIP events, median after warm-up)
    result_device_ms / topk_device_ms                  tg_softmax_out (reads AND writes the plane) and tg_row_topk in the same run
    slab_sweep                                         the call at forced slab heights: {slab_rows: device ms}; "0" is the library's rule
    k_sweep                                            the call at k = 1, 4, 8, 16, 32 ({k: device ms})
    floor_ms, ratio_to_floor                           4 C Vp + 16 V k slabs + 8 V k bytes at 6.29 TB/s, and the call against it
    spot_topk_to_host_ms / host_sort_route_ms          end to end to NumPy arrays: the call + copies, against result() + copy + a stable
                                                       argsort of every column on the host
    lists_equal_host_route / values_equal_host_route   the two routes agree (cells equal, values bit for bit)

    python scripts/bench_spot_topk.py [--cells 30000] [--spots 10000] [--genes 64] [--k 8] [--reps 10] [--out profiles/spot_topk/bench_spot_topk.json]
"""
import argparse
import ctypes as ct
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tangram_amd.device_init import device_normal          # noqa: E402
from tangram_amd.engine import HipMapperEngine             # noqa: E402

COPY_CEILING = 6.29e12                                      # bytes / s: the copy ceiling DESIGN.md section 7 measures against


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
    return round(statistics.median(ms), 4), round(min(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=30000)
    ap.add_argument("--spots", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=64)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", default="304,600,1200,2400,4800,30000")
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    C, V, K, k = a.cells, a.spots, a.genes, a.k
    g = torch.Generator(device="cpu").manual_seed(1)
    S = torch.rand((C, K), generator=g).to(dev)
    G = torch.rand((V, K), generator=g).to(dev)
    eng = HipMapperEngine(S, G, device_normal(C, V, dev, 7), device=dev, precision="bf16x3")
    eng.step(2, 0.1)                                        # the row statistics as the update kernel leaves them
    lib = eng._lib
    Vp = int(eng.logits()[0].shape[1])
    P = torch.empty((C, V), dtype=torch.float32, device=dev)
    rval = torch.empty((C, k), dtype=torch.float32, device=dev)
    ridx = torch.empty((C, k), dtype=torch.int32, device=dev)
    val = torch.empty((V, max(k, 32)), dtype=torch.float32, device=dev)      # (room for the largest k of the sweep)
    cell = torch.empty((V, max(k, 32)), dtype=torch.int32, device=dev)
    total = torch.empty((V,), dtype=torch.float32, device=dev)

    def spot_call(slab_rows, colsum, k=k):
        n = ct.c_size_t()
        eng._call(lib.tg_mapper_spot_topk_query_bytes, eng._h, k, slab_rows, ct.byref(n))
        scratch = torch.empty(n.value // 8 + 1, dtype=torch.int64, device=dev)
        return lambda: eng._call(lib.tg_mapper_result_spot_topk, eng._h, k, -1.0, slab_rows, scratch.data_ptr(), val.data_ptr(),
                                 cell.data_ptr(), total.data_ptr() if colsum else None, tensors=(scratch,))

    out = dict(cells=C, spots=V, pitch=Vp, k=k, reps=a.reps, device=torch.cuda.get_device_name(dev))
    calls = {"result": lambda: eng._call(lib.tg_mapper_result, eng._h, P.data_ptr(), None),
             "topk": lambda: eng._call(lib.tg_mapper_result_topk, eng._h, k, rval.data_ptr(), ridx.data_ptr()),
             "spot_topk": spot_call(0, False), "spot_topk_colsum": spot_call(0, True)}
    for name, fn in calls.items():
        out[name + "_device_ms"], out[name + "_device_ms_min"] = device_ms(fn, dev, a.warmup, a.reps)
    limits = (ct.c_int32 * 4)()
    lib.tg_debug_spot_topk_limits(C, V, limits)
    rows = int(limits[3])
    n_slabs = -(-C // rows)
    out["slab_rows"], out["slabs"], out["workgroups"] = rows, n_slabs, -(-V // int(limits[1])) * n_slabs
    out["slab_sweep"] = {"0": out["spot_topk_device_ms"]}
    for r in [int(x) for x in a.sweep.split(",") if x]:
        out["slab_sweep"][str(r)] = device_ms(spot_call(r, False), dev, 2, max(3, a.reps // 2))[0]
    # the list length: k = 1 keeps one entry and hardly ever shifts -- what the pass costs without the insertions
    out["k_sweep"] = {str(kk): device_ms(spot_call(0, False, kk), dev, 2, max(3, a.reps // 2))[0] for kk in (1, 4, 8, 16, 32)}
    floor_bytes = 4 * C * Vp + 16 * V * k * n_slabs + 8 * V * k
    out["floor_bytes"], out["floor_ms"] = floor_bytes, round(1e3 * floor_bytes / COPY_CEILING, 4)
    out["ratio_to_floor"] = round(out["spot_topk_device_ms"] / out["floor_ms"], 3)
    out["ratio_to_floor_colsum"] = round(out["spot_topk_colsum_device_ms"] / out["floor_ms"], 3)
    out["ratio_to_softmax_out"] = round(out["spot_topk_device_ms"] / out["result_device_ms"], 3)

    def spot_to_host():
        return tuple(x.cpu().numpy() for x in eng.result_spot_topk(k))

    def host_route():
        Pt = np.ascontiguousarray(eng.result().cpu().numpy().T)             # [V, C]: a column of the mapping per row
        order = np.argsort(-Pt, axis=1, kind="stable")[:, :k]                # value descending, equal values by ascending cell
        return np.take_along_axis(Pt, order, 1), order.astype(np.int32)

    for _ in range(2):
        spot_to_host()
    ms = []
    for _ in range(max(3, a.reps // 2)):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        got = spot_to_host()
        ms.append(1e3 * (time.perf_counter() - t0))
    out["spot_topk_to_host_ms"] = round(statistics.median(ms), 3)
    if not a.no_host_route:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        hv, hc = host_route()
        out["host_sort_route_ms"] = round(1e3 * (time.perf_counter() - t0), 1)          # (one run: tens of seconds)
        out["lists_equal_host_route"] = bool(np.array_equal(got[1], hc))
        out["values_equal_host_route"] = bool(np.array_equal(got[0].view(np.uint32), hv.view(np.uint32)))
    out["dense_bytes"], out["spot_topk_bytes"] = C * V * 4, V * k * 8
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
