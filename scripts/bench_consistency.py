"""Scoring repeated mappings: the five-metric question of a tuning trial answered from the resident logits (tg_mapper_consistency,
one pass over R planes of logits) against the host route of the reference (R dense results copied to the host, NumPy over the cube),
at the BASELINE config-2 shape, 30 000 cells x 10 000 spots, R = 3 untrained seeded mappings.  Prints ONE JSON line:

    consistency_device_ms / _min     device time of one tg_mapper_consistency call (HIP events, mean and minimum of --reps after warm-up)
    consistency_no_pearson_device_ms the same call with the correlations not asked for: votes and both entropies only, no fp64 moment is
                                     formed -- the difference is what the moments cost over the read
    floor_ms, ratio_to_floor         R * C * pitch * 4 bytes at the 6.29 TB/s copy ceiling, and mean / floor
    softmax_out_device_ms            tg_softmax_out of ONE plane in the same run (reads one plane, writes one)
    host_route_s                     the host route, timed once: R x result().cpu() + np.corrcoef / vote / consensus entropy in NumPy
                                     (needs ~12 GB of host memory: --skip-host leaves it out)
    pearson_equal_host, votes_equal_host     the device's correlations (within 1e-9) and votes (exactly) against that route

    python scripts/bench_consistency.py [--cells 30000] [--spots 10000] [--genes 64] [--runs 3] [--reps 10] [--skip-host]
                                        [--out profiles/consistency/bench_consistency.json]
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
from tangram_amd import mapping_parameter_tuning as mpt     # noqa: E402
from tangram_amd.device_init import device_normal          # noqa: E402
from tangram_amd.engine import HipMapperEngine             # noqa: E402

COPY_CEILING = 6.29e12          # bytes / s, the measured device-to-device copy rate (README)


def host_metrics(cube):
    """The reference's three functions (mapping_parameter_tuning.py:42-82), one run at a time where they allow it."""
    import scipy.stats
    r = cube.shape[0]
    pearson = np.corrcoef(np.reshape(cube, (r, -1)))[np.tril_indices(r, -1)]
    votes = cube.argmax(axis=2)
    enc = np.zeros(cube.shape)
    for run in range(r):
        enc[run, np.arange(cube.shape[1]), votes[run]] = 1
    vote = scipy.stats.entropy(enc.mean(axis=0), axis=1) / np.log(cube.shape[2])
    del enc
    cons = scipy.stats.entropy(cube.mean(axis=0), axis=1) / np.log(cube.shape[2])
    return pearson, votes, vote, cons


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=30000)
    ap.add_argument("--spots", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "consistency",
                                                  "bench_consistency.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    C, V, K, R = a.cells, a.spots, a.genes, a.runs
    g = torch.Generator(device="cpu").manual_seed(1)
    S = torch.rand((C, K), generator=g).to(dev)
    G = torch.rand((V, K), generator=g).to(dev)
    engines = [HipMapperEngine(S, G, device_normal(C, V, dev, 7 + r), device=dev, precision="bf16x3") for r in range(R)]
    e0 = engines[0]
    lib, pitch = e0._lib, int(e0.sizes.m_pitch)
    P = torch.empty((C, V), dtype=torch.float32, device=dev)
    nbytes = ct.c_size_t()
    lib.tg_consistency_query_bytes(R, C, ct.byref(nbytes))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)          # everything preallocated: the events time the two kernels
    pear = torch.empty(max(R * (R - 1) // 2, 1), dtype=torch.float64, device=dev)
    vote, cons = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(2))
    votes = torch.empty((R, C), dtype=torch.int32, device=dev)
    handles = (ct.c_void_p * R)(*[e._h for e in engines])
    calls = {"consistency": lambda: e0._call(lib.tg_mapper_consistency, handles, R, ws.data_ptr(), pear.data_ptr(), vote.data_ptr(), cons.data_ptr(),
                                             votes.data_ptr()),
             "consistency_no_pearson": lambda: e0._call(lib.tg_mapper_consistency, handles, R, ws.data_ptr(), None, vote.data_ptr(), cons.data_ptr(),
                                                        votes.data_ptr()),
             "softmax_out": lambda: e0._call(lib.tg_mapper_result, e0._h, P.data_ptr(), None)}
    out = dict(cells=C, spots=V, pitch=pitch, runs=R, reps=a.reps, device=torch.cuda.get_device_name(dev))
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
        out[name + "_device_ms"] = round(statistics.mean(ms), 4)
        out[name + "_device_ms_min"] = round(min(ms), 4)
    out["logit_bytes"] = R * C * pitch * 4
    out["floor_ms"] = round(1e3 * out["logit_bytes"] / COPY_CEILING, 4)
    out["ratio_to_floor"] = round(out["consistency_device_ms"] / out["floor_ms"], 3)
    out["ratio_to_softmax_out_x_runs"] = round(out["consistency_device_ms"] / (R * out["softmax_out_device_ms"]), 3)
    got = {k: v.cpu().numpy() for k, v in mpt.mapper_consistency(engines, votes=True).items()}
    t0 = time.perf_counter()
    m = mpt.mapping_consistency(engines)
    torch.cuda.synchronize(dev)
    out["mapping_consistency_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    out.update({k: float(v) for k, v in m.items()})
    if not a.skip_host:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        cube = np.stack([e.result().cpu().numpy() for e in engines])
        out["host_copy_s"] = round(time.perf_counter() - t0, 3)
        host_pearson, host_votes, host_vote, host_cons = host_metrics(cube)
        out["host_route_s"] = round(time.perf_counter() - t0, 3)
        out["pearson_equal_host"] = bool(np.abs(host_pearson - got["pearson"]).max() <= 1e-9)
        out["votes_equal_host"] = bool(np.array_equal(host_votes, got["votes"]))
        out["vote_entropy_max_dev_host"] = float(np.abs(host_vote - got["vote_entropy"]).max())
        out["consensus_entropy_max_dev_host"] = float(np.abs(host_cons - got["consensus_entropy"]).max())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
