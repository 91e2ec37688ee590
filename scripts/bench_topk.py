"""Getting the answer out: the dense result (tg_softmax_out, C x V floats) against each cell's k most probable spots (tg_row_topk,
C x k pairs) at the BASELINE config-2 shape, 30 000 cells x 10 000 spots, k = 8.  Prints ONE JSON line:

    result_device_ms / topk_device_ms          device time of one call into preallocated buffers (HIP events, median after warm-up)
    result_to_host_ms / topk_to_host_ms        the call + the copy to NumPy arrays (wall clock, synchronised)

    python scripts/bench_topk.py [--cells 30000] [--spots 10000] [--genes 64] [--k 8] [--reps 10] [--out profiles/topk/bench_topk.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tangram_amd.device_init import device_normal          # noqa: E402
from tangram_amd.engine import HipMapperEngine             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=30000)
    ap.add_argument("--spots", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=64)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
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
    P = torch.empty((C, V), dtype=torch.float32, device=dev)
    val = torch.empty((C, k), dtype=torch.float32, device=dev)
    idx = torch.empty((C, k), dtype=torch.int32, device=dev)
    calls = {"result": lambda: eng._call(lib.tg_mapper_result, eng._h, P.data_ptr(), None),
             "topk": lambda: eng._call(lib.tg_mapper_result_topk, eng._h, k, val.data_ptr(), idx.data_ptr())}
    to_host = {"result": lambda: eng.result().cpu().numpy(),
               "topk": lambda: tuple(x.cpu().numpy() for x in eng.result_topk(k))}
    out = dict(cells=C, spots=V, k=k, reps=a.reps, device=torch.cuda.get_device_name(dev))
    for name, fn in calls.items():
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize(dev)
            ms.append(t0.elapsed_time(t1))
        out[name + "_device_ms"] = round(statistics.median(ms), 4)
        out[name + "_device_ms_min"] = round(min(ms), 4)
    for name, fn in to_host.items():
        for _ in range(2):
            fn()
        ms = []
        for _ in range(max(3, a.reps // 2)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ms.append(1e3 * (time.perf_counter() - t0))
        out[name + "_to_host_ms"] = round(statistics.median(ms), 3)
    ref = eng.result()
    tv, ti = eng.result_topk(k)
    rv, ri = torch.topk(ref, k, dim=1)                      # (a check of the run, not the order test: ties are tests/topk_cases.py)
    out["values_equal_dense"] = bool(torch.equal(tv, rv))
    out["dense_bytes"], out["topk_bytes"] = C * V * 4, C * k * 8
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
