"""Batches of mappings with spatial terms on the device: the cases of tests/batched_spatial_cases.py (plain bf16 included), and
one batched spatial step captured into a HIP graph."""
import numpy as np
import pytest

from tests import batched_spatial_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", cases.case_table(True), ids=lambda c: c[0])
def test_spatial_batch_has_the_bits_of_each_mapping_alone(case):
    cases.run_case("cuda:0", case)


@pytest.mark.parametrize("name", sorted(cases.REFUSALS))
def test_spatial_batch_refusals(name):
    cases.REFUSALS[name]("cuda:0")


def test_tuning_trial_with_spatial_terms_goes_through_one_batch():
    cases.tuning_trial_case("cuda:0")


def test_batched_spatial_step_captured_into_a_graph():
    """One batched step with all five terms captured after a priming step and replayed twice, against three uncaptured steps.  The
    step index (Adam's bias corrections) and the history row are launch arguments (TgStepVar), so a replay repeats the captured
    step: the uncaptured side issues its second and third step at the same step index and history row (tg_mapper_set_step), which
    is the only way two programs can issue the launches a replay issues.  B = 5: three groups, i.e. a graph with parallel branches."""
    import torch
    from tangram_amd.batched import MapperBatch
    B, precision = 5, "bf16x3"
    specs = [cases.mapping_spec(cases.SMALL, "all5-full", i, None) for i in range(B)]

    def second_step_twice(batch, hists, how):
        batch.step(1, cases.LR, hists, 0)                          # priming step: uploads the argument arrays for THESE histories
        graph = None
        for rep in range(2):
            for e in batch.engines:
                e.set_step(1)
            if how == "eager":
                batch.step(1, cases.LR, hists, 1)
            else:
                if graph is None:
                    s.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
                        batch.step(1, cases.LR, hists, 1)          # captured, not executed
                    assert all(np.isnan(h[1].cpu().numpy()).all() for h in hists), "capturing must not execute the step"
                graph.replay()
        s.synchronize()
        return [(cases.bits(h),) + cases.state_bits(e)[:3] for h, e in zip(hists, batch.engines)]

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                                     # the handles bind to the stream that is current at construction
        out = {}
        for how in ("eager", "graph"):
            engines = [cases.make_engine("cuda:0", precision, sp) for sp in specs]
            batch = MapperBatch(cases.as_mappers(engines))
            out[how] = second_step_twice(batch, batch.new_histories(2), how)
            batch.close()
            for e in engines:
                e.release()
    for i in range(B):
        assert np.isfinite(out["eager"][i][0].view(np.float32)[:, 0]).all()
        cases.assert_same_bits(out["graph"][i], out["eager"][i], f"mapping {i}")
