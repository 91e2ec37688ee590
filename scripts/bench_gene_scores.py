"""Scoring every gene against the measured spatial data: the per-gene cosine score of compare_spatial_geneexp computed on the device
(tg_gene_scores, score_genes) against the host route of the reference (project_genes to a host array, one np.linalg.norm pair per
gene), at the tutorial's shape: 26 431 cells x 9 852 spots, 18 000 scored genes, a Mapper trained for a few epochs.  Prints ONE JSON line:

    block_device_ms / _min           device time of one tg_gene_scores call on a block of --gene-block genes (HIP events, mean and
                                     minimum of --reps after warm-up), 16-byte path; block_scalar_device_ms: an odd pitch
    block_floor_ms, block_ratio_to_floor   2 * spots * block * 4 bytes at the 6.29 TB/s copy ceiling, and mean / floor
    plane_device_ms, plane_ratio_to_floor  the same for ONE call over all scored genes (the kernel away from its launch overheads)
    score_genes_s                    score_genes(mapper=...) end to end: preparation of adata_sc, gather, projection and scoring of every
                                     block, the DataFrame
    host_route_s                     project_genes(mapper=...) to host arrays + the reference's per-gene NumPy loop (utils.py:424-426),
                                     in the same run; host_project_s / host_loop_s: its two parts
    scores_max_abs_diff, scores_agree      the two routes' scores against each other (agree: within 1e-4, the split-bf16 tolerance of the
                                     projection; the host loop runs in float32 like the reference)

    python scripts/bench_gene_scores.py [--cells 26431] [--spots 9852] [--genes 18000] [--train 249] [--gene-block 1024] [--reps 20]
                                        [--skip-host] [--out profiles/gene_scores/bench_gene_scores.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tangram_amd as tg                                    # noqa: E402
from tangram_amd.anndata_lite import AnnDataLite           # noqa: E402
from tangram_amd.gene_score import GeneScorer              # noqa: E402

COPY_CEILING = 6.29e12          # bytes / s, the measured device-to-device copy rate (README)


def host_scores(X_1, X_2):
    """The reference's loop (utils.py:424-426)."""
    cos_sims = []
    for v1, v2 in zip(X_1.T, X_2.T):
        norm_sq = np.linalg.norm(v1) * np.linalg.norm(v2)
        cos_sims.append((v1 @ v2) / norm_sq)
    return np.asarray(cos_sims, dtype=np.float64)


def counts(shape, density, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand(shape, generator=g, device=dev)
    return (torch.floor(x / density * 6 + 1) * (x < density)).cpu().numpy()      # integers 1 .. 6 at `density`, else 0


def timed(fn, dev, warmup, reps):
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
    return round(statistics.mean(ms), 4), round(min(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=26431)
    ap.add_argument("--spots", type=int, default=9852)
    ap.add_argument("--genes", type=int, default=18000)
    ap.add_argument("--train", type=int, default=249)
    ap.add_argument("--gene-block", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gene_scores",
                                                  "bench_gene_scores.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    C, V, N, kb = a.cells, a.spots, a.genes, a.gene_block
    out = dict(cells=C, spots=V, genes=N, train_genes=a.train, gene_block=kb, reps=a.reps, device=torch.cuda.get_device_name(dev))

    # ---- the kernel alone: one block, one whole plane
    g = torch.Generator(device=dev).manual_seed(1)
    pred = torch.rand((V, N), generator=g, device=dev)
    meas = torch.rand((V, N), generator=g, device=dev)
    scorer = GeneScorer(V, N, dev)
    score = torch.empty(N, dtype=torch.float64, device=dev)
    pb, mb = pred[:, :kb].contiguous(), meas[:, :kb].contiguous()
    po, mo = (torch.empty((V, kb + 1), dtype=torch.float32, device=dev)[:, :kb].copy_(x) for x in (pb, mb))
    assert pb.data_ptr() % 16 == 0 and kb % 4 == 0 and po.stride(0) % 2 == 1
    out["block_device_ms"], out["block_device_ms_min"] = timed(lambda: scorer.score_into(pb, mb, score[:kb]), dev, a.warmup, a.reps)
    out["block_scalar_device_ms"], out["block_scalar_device_ms_min"] = timed(lambda: scorer.score_into(po, mo, score[:kb]), dev, a.warmup, a.reps)
    out["plane_device_ms"], out["plane_device_ms_min"] = timed(lambda: scorer.score_into(pred, meas, score), dev, a.warmup, a.reps)
    out["block_floor_ms"] = round(1e3 * 2 * V * kb * 4 / COPY_CEILING, 4)
    out["plane_floor_ms"] = round(1e3 * 2 * V * N * 4 / COPY_CEILING, 4)
    out["block_ratio_to_floor"] = round(out["block_device_ms"] / out["block_floor_ms"], 3)
    out["plane_ratio_to_floor"] = round(out["plane_device_ms"] / out["plane_floor_ms"], 3)
    del pred, meas, pb, mb, po, mo, scorer

    # ---- the two routes end to end on one trained mapper
    genes = [f"g{i}" for i in range(N)]
    S, G = counts((C, N), 0.1, dev, 2), counts((V, N), 0.2, dev, 3)
    S[0], G[0] = 1.0, 1.0                                              # (no all-zero gene)

    def adatas():
        ad_sc = AnnDataLite(S, obs=pd.DataFrame(index=[f"c{i}" for i in range(C)]), var=pd.DataFrame(index=genes))
        ad_sp = AnnDataLite(G, obs=pd.DataFrame(index=[f"s{i}" for i in range(V)]), var=pd.DataFrame(index=genes))
        for ad in (ad_sc, ad_sp):
            ad.uns["training_genes"], ad.uns["overlap_genes"] = genes[:a.train], genes
        return ad_sc, ad_sp

    ad_sc, ad_sp = adatas()
    ad_map = tg.map_cells_to_space(ad_sc, ad_sp, device=dev, num_epochs=a.epochs, density_prior=None, random_state=42, verbose=False,
                                   keep_mapper=True, top_k=4)
    mapper = ad_map._tangram_amd_mapper
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    df = tg.score_genes(ad_map, ad_sc, ad_sp, mapper=mapper, device=dev, gene_block=kb)
    torch.cuda.synchronize(dev)
    out["score_genes_s"] = round(time.perf_counter() - t0, 3)
    if not a.skip_host:
        ad_sc, ad_sp = adatas()
        t0 = time.perf_counter()
        ad_ge = tg.project_genes(ad_map, ad_sc, mapper=mapper, device=dev)
        t1 = time.perf_counter()
        host = host_scores(np.asarray(ad_ge.X), G)
        t2 = time.perf_counter()
        out["host_project_s"], out["host_loop_s"], out["host_route_s"] = round(t1 - t0, 3), round(t2 - t1, 3), round(t2 - t0, 3)
        d = float(np.abs(df.loc[genes, "score"].to_numpy() - host).max())
        out["scores_max_abs_diff"], out["scores_agree"] = d, bool(d <= 1e-4)
        out["speedup_end_to_end"] = round(out["host_route_s"] / out["score_genes_s"], 2)
    mapper.release()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
