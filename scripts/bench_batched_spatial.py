"""Three seeds of one mapping problem WITH spatial terms (the tuning trial, mapping_parameter_tuning.py:86-139): stepped one after
the other -- what the library did before a tg_batch admitted spatial terms, reproduced here by stepping the handles solo -- against
the same three handles in ONE tg_batch.  Both figures come from the same run, on the same handles, in alternating windows.

Data: tangram_amd/synthetic.py (seeded, generated on the device); graph: hexagonal grid, 6 neighbours; terms: those of BASELINE
config 5b (lambda_neighborhood_g1 = 0.96, lambda_ct_islands = 0.17, 18 cell types) plus lambda_getis_ord.

Per shape: device ms per iteration of the three seeds (HIP events around `--steps` iterations, median and spread of `--reps`
alternating windows after a warm-up), the wall time of train_multiple_Mapper with the batch and with batching disabled, and the
kernel launches of one iteration both ways (counted from the step's launch list, tg_capi.hip: tg_one_step / tg_batch_step_impl).
Writes profiles/batched_spatial/bench_batched_spatial.json and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tangram_amd as tg  # noqa: E402
import tangram_amd.mapping_optimizer as mo  # noqa: E402
from tangram_amd import batched  # noqa: E402
from tangram_amd.batched import MapperBatch  # noqa: E402
from tangram_amd.synthetic import cell_type_encoding, hex_grid_graph, make_workload  # noqa: E402

LAM = dict(lambda_d=1.0, lambda_g1=1.0, lambda_neighborhood_g1=0.96, lambda_ct_islands=0.17, lambda_getis_ord=0.5)
N_TYPES = 18
SHAPES = ((2000, 249, 2000), (4200, 500, 1100), (8000, 500, 4000))


def launches_per_step(n_mappings, n_groups):
    """Kernel launches of one iteration with nb + ct + Getis-Ord on: forward, Ghat reduce, gene reduce | W Ghat, column statistics,
    their reduce | mask, its gradient | loss | W^T product | Ws product, two statistics stages with a reduce each, finalize, gradient,
    its reduce, Ws^T product | emitter, backward, update.  Solo: per mapping.  Batch: per GROUP of mappings (tg_batch_groups)."""
    per_step = 3 + 3 + 2 + 1 + 1 + 9 + 3
    return {"sequential": per_step * n_mappings, "batch": per_step * n_groups, "batch_groups": n_groups}


def problem(C, K, V, dev):
    w = make_workload(C, K, V, dev, seed=1)
    N, W = hex_grid_graph(V)
    import scipy.sparse as sp
    Ws = (W - sp.identity(V, dtype=np.float32, format="csr")).tocsr()             # row-standardised, no self loops (spatial_weights.py)
    Ws.eliminate_zeros()
    return dict(S=w["S"].cpu().numpy(), G=w["G"].cpu().numpy(), d=w["d"].cpu().numpy(), voxel_weights=W, neighborhood_filter=N,
                spatial_weights=Ws, ct_encode=cell_type_encoding(w["assign"].cpu().numpy(), V, N_TYPES))


def device_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def measure(C, K, V, dev, steps, reps, warmup, epochs):
    p = problem(C, K, V, dev)
    kw = dict(S=p["S"], G=p["G"], d=p["d"], voxel_weights=p["voxel_weights"], neighborhood_filter=p["neighborhood_filter"],
              ct_encode=p["ct_encode"], spatial_weights=p["spatial_weights"], device=dev, **LAM)
    mappers = [mo.Mapper(random_state=seed, **kw) for seed in (1, 2, 3)]
    engines = [m._engine for m in mappers]
    batch = MapperBatch(mappers)

    def sequential():
        for e in engines:
            e.step(steps, 0.1)

    def together():
        batch.step(steps, 0.1)

    for e in engines:
        e.step(warmup, 0.1)
    batch.step(warmup, 0.1)
    torch.cuda.synchronize()
    seq, bat = [], []
    for _ in range(reps):                                   # alternating windows on the same handles (they stay at one step count)
        seq.append(device_ms(sequential, steps))
        bat.append(device_ms(together, steps))
    groups = 3                                              # tg_batch_groups(3): one mapping per group
    batch.close()
    for m in mappers:
        m.release()
    out = {"shape": [C, K, V], "cells_x_spots": C * V, "steps_per_window": steps, "windows": reps,
           "sequential_ms_per_iter": {"median": statistics.median(seq), "min": min(seq), "max": max(seq)},
           "batch_ms_per_iter": {"median": statistics.median(bat), "min": min(bat), "max": max(bat)},
           "batch_speedup_median": statistics.median(seq) / statistics.median(bat),
           "launches_per_iter": launches_per_step(3, groups)}
    # the trial end to end (construction of the three mappers, training, validation, the consistency metrics)
    pack = [p["S"], p["G"], None, p["d"], dev, None, p["voxel_weights"], p["ct_encode"], p["neighborhood_filter"], p["spatial_weights"],
            np.arange(0, K - 10), np.arange(K - 10, K)]
    config = dict(num_epochs=epochs, learning_rate=0.1, **LAM)

    def trial(batching):
        made, init, key = [], batched.MapperBatch.__init__, batched._batch_key

        def spy(self, ms):
            init(self, ms)
            made.append(len(self.mappers))

        batched.MapperBatch.__init__ = spy
        if not batching:
            batched._batch_key = lambda m: None
        try:
            np.random.seed(7)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = tg.train_multiple_Mapper(config, pack)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res, made
        finally:
            batched.MapperBatch.__init__, batched._batch_key = init, key

    trial(True)                                             # warm-up of everything the trial touches
    t_seq, r_seq, made_seq = trial(False)
    t_bat, r_bat, made_bat = trial(True)
    out["train_multiple_Mapper"] = {"epochs": epochs, "sequential_s": t_seq, "batch_s": t_bat, "speedup": t_seq / t_bat,
                                    "batches_created": {"sequential": made_seq, "batch": made_bat},
                                    "metrics_bit_identical": all(np.float64(r_seq[k]).tobytes() == np.float64(r_bat[k]).tobytes() for k in r_seq)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="iterations per timed window")
    ap.add_argument("--reps", type=int, default=7, help="alternating windows per route")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--epochs", type=int, default=300, help="epochs of the train_multiple_Mapper trials")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched_spatial", "bench_batched_spatial.json"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batched_spatial.py measures on the GPU: no device found")
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "lambdas": LAM, "cell_types": N_TYPES, "graph": "hex grid, 6 neighbours",
           "seeds": 3, "shapes": [measure(C, K, V, dev, opt.steps, opt.reps, opt.warmup, opt.epochs) for C, K, V in SHAPES]}
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
