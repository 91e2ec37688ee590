"""The validation metrics of Mapper._val_loss_fn (tg_mapper_validate: val_total_loss, val_gene_sim, val_sp_sparsity_weighted_sim,
val_entropy) on every kernel path against the fp64 formula oracle.tangram_oracle.validation_metrics, on the HIP emulator (CPU; the GPU
run of the same table is tests/test_gpu_validation_metrics.py).  The formula itself is pinned to the reference's recorded
_val_loss_fn history in tests/test_oracle_golden.py::test_validation_metrics_fp64.

tg_mapper_validate runs code no training step runs: a forced whole forward pass, tg_ghat_reduce with the per-spot statistics forced
on, tg_row_entropy (256 threads stride over the spots of a row; reads the row constants the last update kernel left),
tg_val_finalize (1 024 threads stride over spots, genes and cells; alone, `partial` = 1 and read-back on spot shards), and the
non-zero fractions tg_prep_g / tg_colsum_parts build at set-up.  The table (parity_common.validation_cases) holds one case per edge
of those loops and per path that leads to them; every id names its edge, test_case_table_covers_every_edge ties them together.

Every case (parity_common.validation_case): validate() before any step, after one step and after three, each of the four numbers
within TOL[precision]["loss"] absolute of the fp64 formula at the oracle's logits -- 1e-5 in fp32 / bf16x3 (and for clusters-mode
handles, which compute in fp32 whatever is asked), 1e-3 in bf16.  The inputs are conditioned: the same formula in NumPy float32
is within a third of 1e-5 of its fp64 value at every such point (largest over the table: 1.6e-7).  The path is asserted
(tg_debug_layout, the effective precision, profile_read of the first step).

Largest |library - fp64 formula| measured over this table on the emulator (MI355X: tests/test_gpu_validation_metrics.py):
    precision                bound   total     gene_sim  weighted  entropy
    fp32 (+ clusters mode)   1e-5    9.6e-8    4.3e-8    5.1e-8    1.2e-7
    bf16x3 (+ two products)  1e-5    4.5e-7    2.0e-7    3.3e-7    3.0e-7
    bf16                     1e-3    1.7e-4    1.1e-4    1.0e-4    4.4e-5
    spot shards (bf16x3)     1e-5    4.5e-8    2.7e-8    3.0e-8    7.8e-8
"""
import pytest

from tests import parity_common as pc
from tests.hipsim.build_sim import build_sim


@pytest.fixture(scope="module")
def sim():
    from tangram_amd import _capi
    path = build_sim()
    if path is None:
        pytest.skip("host clang not available to build the emulator")
    _capi._install_library_for_tests(path)
    yield path
    _capi._install_library_for_tests(None)


CASES = pc.validation_cases(False)


def _is_clusters(c):
    return c["C"] <= pc.TG_SC_MAXC and not c.get("tile") and c["V"] <= pc.ROWPASS_MAX_V


def test_case_table_covers_every_edge():
    """Both tables (emulator and GPU) hold, under an id that names it, every edge the validation kernels have."""
    from tests.test_gpu_validation_metrics import CASES as GPU_CASES
    for table in (CASES, GPU_CASES):
        ids = [c["id"] for c in table]
        assert len(set(ids)) == len(ids)
        by_id = {c["id"]: c for c in table}

        def has(cid, **want):
            assert cid in by_id, cid
            for k, v in want.items():
                assert by_id[cid].get(k, 0) == v, (cid, k)
            return by_id[cid]
        # the three strided loops, one value below / at / above the stride and one on the third trip
        for V in (255, 256, 257, 513):
            has(f"spots-{V}-row-entropy-stride-256", V=V)
        for V in (1023, 1024, 1025, 2050):
            has(f"spots-{V}-finalize-stride-1024", V=V)
        for K in (1023, 1024, 1025):
            has(f"genes-{K}-finalize-stride-1024", K=K)
        for C in (1023, 1025):
            has(f"cells-{C}-finalize-stride-1024", C=C)
        # nky: K + 1 below, at and above TG_GH_COLS on both tiles, and three parts
        for tile in (128, 256):
            for K, nky in ((254, 1), (255, 1), (256, 2), (300, 2)):
                assert pc.val_nky(K, tile) == nky
                has(f"genes-{K}-tile{tile}-nky{nky}", K=K, tile=tile)
        assert pc.val_nky(600, 0) == 3
        has("genes-600-nky3", K=600)
        # lambda_g2 = 0 on both paths
        assert not _is_clusters(has("lambda-g2-0-gemm-path", lambda_g2=0.0)) and _is_clusters(has("lambda-g2-0-clusters-path", lambda_g2=0.0))
        assert all(c.get("lambda_g2", 0.5) == 0.5 for c in table if not c["id"].startswith("lambda-g2-0"))
        # row blocks of TG_RB spots with genes that are zero in (almost) every spot; the tall gene reduce
        for V in (15, 16, 17, 33):
            assert has(f"spots-{V}-row-block-of-16-sparse-genes", V=V)["zero_genes"] > 0
        tall = has("spots-8200-tall-gene-reduce-sparse-genes", V=8200)
        assert -(-tall["V"] // pc.TG_RB) > 512 and tall["zero_genes"] > 0 and not _is_clusters(tall)
        assert all(-(-c["V"] // pc.TG_RB) <= 512 for c in table if c["V"] < 8200)
        # the update families whose row constants tg_row_entropy reads
        kinds = {}
        for c in table:
            if not _is_clusters(c) and not c.get("pipeline_bands"):
                k = pc.update_instantiation(c["C"], c["V"], c["precision"], "plain")
                kinds.setdefault((k[0], k[4]), []).append(c["id"])
        assert "spots-4000-after-rowpass-256-threads" in kinds[("tg_adam_rowpass", 256)]
        assert "spots-4100-after-rowpass-512-threads" in kinds[("tg_adam_rowpass", 512)]
        assert "spots-16400-cells-40-after-adam-update-1024-threads" in kinds[("tg_adam_update", 1024)]
        assert "spots-16400-cells-70-after-adam-update-256-threads" in kinds[("tg_adam_update", 256)]
        # both paths: clusters mode at 1, 18 and 32 cells, the first GEMM-path C, both K and both V; bf16 asked once; tile pinned once
        cl = [c for c in table if _is_clusters(c)]
        assert {c["C"] for c in cl} >= {1, 18, 32} and {c["K"] for c in cl} >= {9, 250} and {c["V"] for c in cl} >= {70, 1300}
        assert not _is_clusters(has("cells-33-first-gemm-path", C=33))
        assert _is_clusters(has("clusters-18-cells-bf16-asked-fp32-runs", C=18)) and by_id["clusters-18-cells-bf16-asked-fp32-runs"]["precision"] == "bf16"
        pinned, default = has("clusters-18-cells-tile128-pins-gemm-path", C=18, tile=128), has("clusters-18-cells-default-path", C=18)
        assert not _is_clusters(pinned) and _is_clusters(default)
        assert {k: v for k, v in pinned.items() if k not in ("id", "tile")} == {k: v for k, v in default.items() if k != "id"}
        for b in (2, 3):
            has(f"pipeline-bands-{b}", C=420, K=16, V=150, pipeline_bands=b)
        for K in (6015, 6016, 6200):
            has(f"genes-{K}-all-genes-width", K=K)
        assert has("sharpened-logits-x30-spots-300", V=300)["sharpen"] == 30.0
        # precisions: everything in bf16x3, a third of the GEMM-path cases in fp32 and in bf16, two cases on the two-product path
        x3 = [c for c in table if c["precision"] == "bf16x3" and not c.get("s_exact")]
        gemm = [c for c in x3 if not _is_clusters(c) and c["K"] != 5888 and (table is GPU_CASES or c["V"] < 8000)]
        for p in ("fp32", "bf16"):
            n = sum(1 for c in table if c["precision"] == p and not _is_clusters(c))
            assert 3 * n >= len(gemm) - 3, (p, n, len(gemm))
            assert {c["id"][:-len(p) - 1] for c in table if c["id"].endswith("-" + p)} <= set(by_id)
        assert sum(1 for c in table if c.get("s_exact")) == 2
    assert any(c["K"] == 5888 and c.get("tile") == 256 for c in GPU_CASES), "the 256-tile all-genes width of tests/test_gpu_wide_genes.py"


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_emulated_validation_metrics(sim, case):
    pc.run_validation_case("cpu", case)


UNDISTURBED = [
    ("clusters-path", dict(C=18, K=20, V=70)),
    ("rowpass-256-threads", dict(C=40, K=8, V=300)),
    ("rowpass-512-threads", dict(C=40, K=8, V=4100)),
    ("adam-update", dict(C=40, K=8, V=16400, calls=(1, 1))),          # (two steps here, 25 s each on the emulator; four on the GPU)
    ("lambda-g2-0", dict(C=40, K=8, V=300, lambda_g2=0.0)),
    ("pipeline-bands-3", dict(C=420, K=16, V=150, pipeline_bands=3)),
    ("pipeline-bands-3-two-steps-per-call", dict(C=420, K=16, V=150, pipeline_bands=3, calls=(2, 2))),
]


@pytest.mark.parametrize("kw", [k for _, k in UNDISTURBED], ids=[i for i, _ in UNDISTURBED])
def test_emulated_validation_leaves_training_alone(sim, kw):
    pc.validation_undisturbed_case("cpu", **kw)


def test_emulated_constrained_handle_refuses_validation(sim):
    pc.validation_refused_case("cpu")


# (world, K, rank whose block holds no spot of gene 0): 1 010 spots are ragged on 2 and on 3 shards; 300 genes are two voxstat parts
SHARDS = [(2, 48, None), (3, 300, None), (3, 48, 1),
          # nine and sixteen shards: the second trip of the eight-wide per-rank loops (tests/many_rank_cases.py); the rank without a
          # spot of gene 0 is one of the second trip
          (9, 300, None), (16, 300, 11)]


@pytest.mark.parametrize("world,K,empty", SHARDS, ids=[f"world{w}-genes{K}" + ("-gene-empty-on-a-shard" if e is not None else "") for w, K, e in SHARDS])
def test_emulated_validation_on_spot_shards(sim, world, K, empty):
    pc.validation_shards_case("cpu", "bf16x3", world, 40, K, 1010, empty_gene_on_rank=empty)
