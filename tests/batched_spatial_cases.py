"""Batches of mappings that carry spatial terms (tg_batch over handles with has_nb / has_ct / has_ac): the cases shared by
tests/test_batched_spatial.py (CPU emulator) and tests/test_gpu_batched_spatial.py (device).

The contract of a batch: a mapping trained in a batch has the BITS of the same mapping trained alone -- every history column of
every epoch, the logits and both Adam moments (tg_mapper_state).  Each case trains B mappings alone on fresh handles, then the same
B mappings (fresh handles again, same seeds) in one `MapperBatch` for STEPS steps, and compares bits.

Shapes: the smallest at which the batched twins of the spatial kernels can go wrong.
  SMALL = 40 cells x 12 genes x 70 spots, 3 cell types: 70 spots are 4 blocks of 16 and a block of 6 (tg_colstats_b, tg_ac_*_b), the
          irregular graph is weighted and asymmetric, spot 0 has no neighbour (an empty CSR row in every graph, an empty column too)
          and cell type 2 has no cell (a zero column of ct_encode).
  WIDE  = 40 x 130 x 257: 257 spots cross a block boundary by one spot, 130 genes + 1 + 3 pad to 256 columns, i.e. two operand
          column blocks of 128 for the emitter and a second 64-gene block of tg_gene_reduce_b.
Batch sizes 2 and 3 are one mapping per group; 5 is three groups of 1, 2 and 2 mappings (tg_batch_groups), so that the last
group's offset into every argument array is 3.
Reference loop being replaced: mapping_parameter_tuning.py:86-139 (three seeds of one problem, one after the other)."""
import contextlib
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests.parity_common import ALL_FIVE, SPATIAL_TERMS, spatial_graphs, spatial_problem

STEPS = 4
LR = 0.1
SMALL = (40, 12, 70, 3)
WIDE = (40, 130, 257, 3)
SEED = 5

# name -> (terms, extra lambdas).  lambda_g2 is on unless a set says otherwise: the per-spot statistics then feed tg_loss_finalize_b.
TERM_SETS = {
    "nb": (("nb",), {}),
    "ct": (("ct",), {}),
    "getis": (("getis",), {}),
    "moran+geary": (("moran", "geary"), {}),
    "all5": (ALL_FIVE, {}),
    "all5-full": (ALL_FIVE, dict(lambda_r=1e-3, lambda_l1=1e-4, lambda_l2=1e-5)),          # L.full: regulariser row sums, tg_hist_regs_b
    "all5-g2-0": (ALL_FIVE, dict(lambda_g2=0.0)),
}


def case_table(gpu):
    """(id, shape, term set, B, precision, vary).  `vary`: None, "lambda" (every mapping its own lambda values) or "graph" (every
    mapping its own spot graphs).  Every term set at B = 2 and B = 3 in fp32 and bf16x3 (alternating), B = 5 on both shapes, and
    plain bf16 on the device only."""
    out = []
    for i, name in enumerate(TERM_SETS):
        out.append((f"small-{name}-B{2 + i % 2}-fp32", SMALL, name, 2 + i % 2, "fp32", None))
        out.append((f"small-{name}-B{3 - i % 2}-bf16x3", SMALL, name, 3 - i % 2, "bf16x3", None))
    out.append(("small-all5-B5-fp32", SMALL, "all5", 5, "fp32", None))
    out.append(("small-all5-full-B5-bf16x3", SMALL, "all5-full", 5, "bf16x3", None))
    out.append(("wide-all5-B2-fp32", WIDE, "all5", 2, "fp32", None))
    out.append(("wide-all5-full-B3-bf16x3", WIDE, "all5-full", 3, "bf16x3", None))
    out.append(("wide-all5-B5-bf16x3", WIDE, "all5", 5, "bf16x3", None))
    out.append(("small-all5-own-lambdas-B3-fp32", SMALL, "all5", 3, "fp32", "lambda"))
    out.append(("small-all5-own-graphs-B3-bf16x3", SMALL, "all5", 3, "bf16x3", "graph"))
    out.append(("wide-all5-own-graphs-B5-fp32", WIDE, "all5", 5, "fp32", "graph"))
    if gpu:
        out.append(("small-all5-B3-bf16", SMALL, "all5", 3, "bf16", None))
        out.append(("wide-all5-full-B2-bf16", WIDE, "all5-full", 2, "bf16", None))
        out.append(("small-all5-own-lambdas-B5-bf16", SMALL, "all5", 5, "bf16", "lambda"))
    return out


@functools.lru_cache(maxsize=None)
def _problem(shape, name, graph_seed):
    """(data, lambdas, graph keywords) of one term set on one shape; the graphs from `graph_seed` (the data never change)."""
    C, K, V, T = shape
    terms, extra = TERM_SETS[name]
    data, _, lam, kw = spatial_problem(C, K, V, T, "irregular", terms, SEED)
    lam = dict(lam, lambda_g2=0.5)
    lam.update(extra)
    if graph_seed != SEED:
        g = spatial_graphs("irregular", V, graph_seed)
        kw = {k: (g[k] if k in g else v) for k, v in kw.items()}
    if "ct_encode" in kw:                                       # cell type T - 1 has no cell: its cells join type 0
        E = kw["ct_encode"].copy()
        E[:, 0] += E[:, T - 1]
        E[:, T - 1] = 0
        assert (E.sum(axis=1) == 1).all() and not E[:, T - 1].any() and E[:, 0].any()
        kw = dict(kw, ct_encode=E)
    for k, W in kw.items():
        if k != "ct_encode":
            off = W - np.diag(np.diag(W))
            assert not off[0].any(), f"{k}: spot 0 must have no neighbour"          # (voxel_weights keeps its self loop)
    return data, lam, kw


def mapping_spec(shape, name, i, vary):
    """The i-th mapping of a case: (data, M0, lambdas, graphs)."""
    from oracle import tangram_oracle as orc
    C, K, V, T = shape
    data, lam, kw = _problem(shape, name, SEED + 3 * i if vary == "graph" else SEED)
    if vary == "lambda":                                        # same terms on, other values: 1, 1.25, 1.5, ... times the table's
        spatial = {v[0] for v in SPATIAL_TERMS.values()}
        lam = {k: (v * (1.0 + 0.25 * i) if k in spatial else v) for k, v in lam.items()}
        lam["lambda_g2"] = 0.5 + 0.1 * i
    return data, orc.reference_init_M(C, V, 100 + i), lam, kw


def make_engine(device, precision, spec, **kw):
    from tangram_amd.engine import HipMapperEngine
    data, M0, lam, graphs = spec
    return HipMapperEngine(data["S"], data["G"], M0, d=data["d"], device=device, precision=precision, lambdas=lam, **graphs, **kw)


def bits(t):
    return t.detach().cpu().numpy().copy().view(np.uint32)          # (a copy: on the emulator .cpu() is the live buffer itself)


def state_bits(e):
    M, m1, m2, step = e.logits()
    return bits(M), bits(m1), bits(m2), step


_SOLO = {}


def solo_bits(device, precision, shape, name, i, vary):
    """History and state of mapping i trained alone for STEPS steps: computed once per (device, precision, mapping), shared by the
    cases that contain that mapping, never modified."""
    key = (str(device), precision, shape, name, i, vary if (vary and i) else None)      # (mapping 0 is the same with every `vary`)
    if key not in _SOLO:
        e = make_engine(device, precision, mapping_spec(shape, name, i, vary))
        h = e.new_history(STEPS)
        e.step(STEPS, LR, h, 0)
        out = (bits(h),) + state_bits(e)
        e.release()
        for a in out[:4]:
            a.setflags(write=False)
        _SOLO[key] = out
    return _SOLO[key]


def as_mappers(engines):
    return [SimpleNamespace(_engine=e) for e in engines]


def assert_same_bits(got, ref, what):
    for g, r, part in zip(got, ref, ("history", "M", "Adam m", "Adam v", "step")):
        if part == "step":
            assert g == r, (what, part, g, r)
        else:
            assert g.shape == r.shape and np.array_equal(g, r), f"{what}: {part} differs in {int((g != r).sum())} of {g.size} words"


def run_case(device, case):
    """One row of case_table: B mappings in one MapperBatch against the same mappings trained alone."""
    from tangram_amd import _capi
    from tangram_amd.batched import MapperBatch
    cid, shape, name, B, precision, vary = case
    ref = [solo_bits(device, precision, shape, name, i, vary) for i in range(B)]
    engines = [make_engine(device, precision, mapping_spec(shape, name, i, vary)) for i in range(B)]
    batch = MapperBatch(as_mappers(engines))
    hists = batch.new_histories(STEPS)
    batch.step(1, LR, hists, 0)                         # two calls: the second one starts at a history row other than 0
    batch.step(STEPS - 1, LR, hists, 1)
    batch.close()
    terms = TERM_SETS[name][0]
    for i, e in enumerate(engines):
        h = hists[i].cpu().numpy()
        for t in terms:                                 # the enabled terms really ran: their history columns are numbers
            assert np.isfinite(h[:, getattr(_capi, SPATIAL_TERMS[t][2])]).all(), (cid, i, t)
        assert np.isfinite(h[:, _capi.H_TOTAL]).all()
        assert_same_bits((bits(hists[i]),) + state_bits(e), ref[i], f"{cid}: mapping {i}")
        e.release()
    if vary:                                            # the mappings of such a batch are really different problems
        assert any(not np.array_equal(ref[0][0], ref[i][0]) for i in range(1, B))


# ---- refusals: the message names the reason, nothing is written, the handles go on alone with the solo bits -------------------------
def _refused(device, precision, engines, match, after=None):
    """MapperBatch(engines) raises with `match`; the handles' logits, moments and step count are untouched."""
    from tangram_amd.batched import MapperBatch
    before = [state_bits(e) for e in engines]
    before = [tuple(x.copy() if hasattr(x, "copy") else x for x in b) for b in before]
    with pytest.raises((RuntimeError, ValueError), match=match):
        MapperBatch(as_mappers(engines))
    for e, b in zip(engines, before):
        no_hist = (np.zeros(1, np.uint32),)
        assert_same_bits(no_hist + state_bits(e), no_hist + b, "after the refusal")


def _then_alone(e, ref, what):
    h = e.new_history(STEPS)
    e.step(STEPS, LR, h, 0)
    assert_same_bits((bits(h),) + state_bits(e), ref, what)
    e.release()


def refusal_mixed_spatial_and_plain(device, precision="fp32"):
    from oracle import tangram_oracle as orc
    C, K, V, T = SMALL
    sp = make_engine(device, precision, mapping_spec(SMALL, "nb", 0, None))
    data, M0, lam, _ = mapping_spec(SMALL, "nb", 1, None)
    base = {k: v for k, v in lam.items() if k in ("lambda_g1", "lambda_d", "lambda_g2")}
    plain = make_engine(device, precision, (data, M0, base, {}))
    for order in ((sp, plain), (plain, sp)):
        _refused(device, precision, list(order), "set of spatial terms")
    plain.release()
    _then_alone(sp, solo_bits(device, precision, SMALL, "nb", 0, None), "nb mapping after the refusal")


def refusal_mixed_term_sets(device, precision="fp32"):
    """nb with nb + ct (the latter has cell-type columns in its operand layout)."""
    a = make_engine(device, precision, mapping_spec(SMALL, "nb", 0, None))
    data, M0, lam, kw = mapping_spec(SMALL, "ct", 1, None)
    _, _, lam_nb, kw_nb = mapping_spec(SMALL, "nb", 1, None)
    b = make_engine(device, precision, (data, M0, dict(lam_nb, **lam), dict(kw_nb, **kw)))
    assert b.cfg.lambda_neighborhood_g1 > 0 and b.cfg.lambda_ct_islands > 0
    _refused(device, precision, [a, b], "set of spatial terms")
    b.release()
    _then_alone(a, solo_bits(device, precision, SMALL, "nb", 0, None), "nb mapping after the refusal")


def refusal_band_pipeline(device, precision="fp32"):
    """pipeline_bands > 1 needs two cell tiles to take effect: 130 cells."""
    shape = (130,) + SMALL[1:]
    specs = [mapping_spec(shape, "nb", i, None) for i in range(2)]
    engines = [make_engine(device, precision, s, pipeline_bands=2) for s in specs]
    _refused(device, precision, engines, "band pipeline")
    alone = make_engine(device, precision, specs[0], pipeline_bands=2)
    h = alone.new_history(STEPS)
    alone.step(STEPS, LR, h, 0)
    ref = (bits(h),) + state_bits(alone)
    alone.release()
    engines[1].release()
    _then_alone(engines[0], ref, "banded mapping after the refusal")


def refusal_spot_shard(device, precision="fp32"):
    """Spatial handles of a spot-sharded run (one rank: the shard holds every spot, the handle still gathers Ghat)."""
    from tangram_amd.sharded import make_sharded
    from tests.local_comm import run_ranks

    def rank_fn(comm):
        def shard(i):
            data, M0, lam, kw = mapping_spec(SMALL, "all5", i, None)
            return make_sharded(data["S"], data["G"], M0, d=data["d"], device=device, precision=precision, lambdas=lam, comm=comm, **kw)

        def run(sh):
            h = sh.eng.new_history(STEPS)
            sh.run(STEPS, LR, h)
            out = (bits(h),) + state_bits(sh.eng)
            sh.release()
            return out

        ref = run(shard(0))
        a, b = shard(0), shard(1)
        _refused(device, precision, [a.eng, b.eng], "spot shard")
        b.release()
        assert_same_bits(run(a), ref, "sharded mapping after the refusal")

    run_ranks(1, rank_fn)


REFUSALS = {"spatial-with-plain": refusal_mixed_spatial_and_plain, "nb-with-nb+ct": refusal_mixed_term_sets,
            "spot-shard": refusal_spot_shard, "band-pipeline": refusal_band_pipeline}


# ---- through the top: the tuning trial ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def batches_created():
    """Sizes of the MapperBatch objects that were really created (a refusal raises inside __init__ and is not counted)."""
    from tangram_amd import batched
    made, inner = [], batched.MapperBatch.__init__

    def spy(self, mappers):
        inner(self, mappers)
        made.append(len(self.mappers))

    batched.MapperBatch.__init__ = spy
    try:
        yield made
    finally:
        batched.MapperBatch.__init__ = inner


def tuning_trial_case(device, epochs=4):
    """train_multiple_Mapper with the three hyperparameters the tuner exists for: the three seeds go through ONE MapperBatch, and the
    five metrics are those of the same trial with batching disabled, bit for bit."""
    import tangram_amd as tg
    from tangram_amd import batched
    C, K, V, T = SMALL
    data, lam, kw = _problem(SMALL, "all5", SEED)
    tr, va = np.arange(0, K - 3), np.arange(K - 3, K)
    config = dict(num_epochs=epochs, learning_rate=LR, lambda_d=1.0, lambda_g1=1.0, lambda_g2=0.5,
                  lambda_neighborhood_g1=SPATIAL_TERMS["nb"][1], lambda_ct_islands=SPATIAL_TERMS["ct"][1], lambda_getis_ord=SPATIAL_TERMS["getis"][1])
    pack = [data["S"], data["G"], None, data["d"], device, None, kw["voxel_weights"], kw["ct_encode"], kw["neighborhood_filter"],
            kw["spatial_weights"], tr, va]

    def trial():
        np.random.seed(77)                              # (run 0 is "unseeded": it draws from the global stream)
        with batches_created() as made:
            return tg.train_multiple_Mapper(config, pack), made

    got, made = trial()
    assert made == [3], f"the three seeds must go through one MapperBatch, batches created: {made}"
    key = batched._batch_key
    batched._batch_key = lambda m: None                 # batching disabled: _train_together steps the seeds one after the other
    try:
        ref, made = trial()
    finally:
        batched._batch_key = key
    assert made == []
    assert list(got) == list(tg.mapping_parameter_tuning.METRICS)
    for k in got:
        assert np.isfinite(got[k]), k
        assert np.float64(got[k]).tobytes() == np.float64(ref[k]).tobytes(), (k, got[k], ref[k])
