"""Tables and checks of the consistency metrics of repeated mappings (tg_consist.h: tg_consist_rows, tg_consist_finish;
tg_mapper_consistency / tg_planes_consistency; tangram_amd.mapping_parameter_tuning), shared by tests/test_consistency.py
(emulator, device "cpu") and tests/test_gpu_consistency.py (MI355X).

The oracle is an fp64 NumPy statement of the three definitions, applied to the dense `result()` planes of the same handles on the
same backend -- the p bits are identical, so the votes are exact:

    pearson             np.corrcoef of the flattened planes in fp64, pairs in the order of np.tril_indices(R, -1)
    vote entropy        -sum_s (n_s / R) log(n_s / R) / log(V) over the distinct columns s = argmax of a run's row (n_s votes each)
    consensus entropy   -sum_v m_v log m_v / log(V), m_v the mean of the runs' p_v, a term with m = 0 counts 0

Bounds (none of them fitted to what the kernel gives):
    votes        exact.
    pearson      1e-9: every term is fp64, at most n = 5e5 of them per plane pair here; the worst-case summation error n 2^-53 =
                 5.5e-11 is relative to sum |x_a x_b| <= N sqrt(var_a var_b) (Cauchy-Schwarz), three such errors (cov, two variances)
                 plus NumPy's own leave a margin of 5x.  fp32 accumulation (1e-4 and worse at these sizes) does not pass.
    vote entropy 1e-6: at most 8 terms, each the logarithm of a small rational within a few fp32 ulp.
    consensus    1.5e-6 = 8x the 1.8e-7 by which the reference's own arithmetic (fp32 mean, scipy.stats.entropy) leaves fp64 (measured
                 over V in {2, 63, 1000, 8193, 16387}, scales 0, 1, 8, 48 rows each).  Largest deviation seen with these tables:
                 emulator 1.1e-7, MI355X 1.7e-7 (every table; the MI355X's largest in PLANE_ROW_CASES; also in DESIGN.md, f-7).
    gene_expr_consistency (public surface)  the projection runs at the mapper's gemm precision, so the number is measured, not
                 derived: deviation from the fp64 oracle on the emulator 8.96e-9 at (C, K, V) = (20, 40, 130) and 2.72e-9 at
                 (1500, 40, 900) (3 seeds, 4 epochs, bf16x3); asserted: GENE_EXPR_BOUND = 4 x the larger = 3.6e-8.  The margin is for
                 the device's exponential, which differs from the emulator's in the last place (seen on the MI355X at the first
                 shape: 3.3e-9).
"""
import ctypes as ct
import os
import re

import numpy as np
import pytest
import torch

from tangram_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "tangram_amd", "csrc", "tg_consist.h")


def _header_int(name):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, open(HEADER).read(), flags=re.M)
    assert m, f"{name} is not a plain integer in tg_consist.h"
    return int(m.group(1))


CHUNK = _header_int("TG_CONSIST_CHUNK")
MAX_RUNS = _header_int("TG_CONSIST_MAX_RUNS")
MAX_PARTS = _header_int("TG_CONSIST_MAX_PARTS")
LAM = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5)
PEARSON_BOUND, VOTE_BOUND, CONSENSUS_BOUND = 1e-9, 1e-6, 1.5e-6
GENE_EXPR_BOUND = 4 * 8.96e-9

FAMILIES = ("iid1", "iid8", "shared", "half", "trained")
# (C, V, R, family): row lengths around the wave and the chunk boundary (3 rows: a few hundred KB of logits), 1 / 3 / 257 rows (257 = a
# second trip of the finish kernel's stride over the workgroups' partials), 1 / 2 / 3 / 8 runs
KERNEL_CASES = [(3, 2, 3, "iid1"), (3, 3, 3, "iid8"), (3, 63, 3, "shared"), (3, 64, 3, "half"), (3, 65, 3, "trained"),
                (3, CHUNK - 1, 3, "iid1"), (3, CHUNK, 2, "iid8"), (3, CHUNK + 1, 3, "shared"), (3, 2 * CHUNK + 3, 3, "half"),
                (1, 65, 3, "iid8"), (257, 65, 3, "iid1"), (257, 130, 2, "trained"),
                (40, 257, 1, "iid1"), (40, 257, 2, "shared"), (40, 257, 8, "half"), (3, CHUNK + 1, 8, "iid1")]
# The row loop of tg_consist_rows: the grid stops growing at MAX_PARTS workgroups, workgroup b takes the rows b, b + grid, ... -- the
# moments carried in registers over its rows, the per-row LDS words alternating between two copies (both used again from the third
# trip on).  ROW_LOOP_CASES (n_rows, most workgroups, n_cols, ld, offset, R) walk it on the emulator and the GPU with a handful of rows
# through tg_debug_planes_consistency: 1 .. 9 trips, workgroups of unequal trip counts, both plain loaders, a second chunk, R = 8.
# (The plane entry point: the two plain loaders.  The logits loader is walked by the row loop only on the GPU, in GRID_CASES.)
ROW_LOOP_CASES = [(7, 2, 65, 68, 0, 3), (5, 1, 37, 39, 1, 2), (9, 4, CHUNK + 1, CHUNK + 4, 0, 3), (8, 3, 130, 130, 0, 8), (9, 1, 64, 64, 0, 1),
                  (300, 257, 5, 8, 0, 3)]
# GRID_CASES (C, V, R, family) and PLANE_ROW_CASES (n_rows, n_cols, ld, offset, R) are the shipped launch beyond MAX_PARTS rows, logits
# flavour and values flavour (scalar and 16-byte loads): two trips for one workgroup only, and three trips for four workgroups, two for
# the rest.  On the GPU only: a case costs the emulator, which switches fibers at every wave shuffle of 2 048 workgroups, 20 - 50 s.
GRID_CASES = [(MAX_PARTS + 1, 65, 3, "half"), (2 * MAX_PARTS + 4, 64, 3, "iid1")]
# (n_cols, ld, offset in floats of the first plane's base, R): the values flavour on planes that are not the logits of anybody
PLANE_CASES = [(2, 2, 0, 3), (5, 8, 0, 3), (5, 7, 0, 2), (1000, 1000, 0, 3), (1000, 1004, 0, 3), (1000, 1001, 0, 3), (1000, 1000, 1, 3),
               (1000, 1004, 1, 8), (CHUNK + 1, CHUNK + 4, 0, 2), (5, 5, 0, 1)]
# (n_rows, n_cols, ld, offset, R): the values flavour beyond MAX_PARTS rows, scalar loads (odd pitch, base off by one float) and 16-byte loads
PLANE_ROW_CASES = [(2 * MAX_PARTS + 4, 37, 39, 1, 3), (MAX_PARTS + 1, 64, 68, 0, 2)]
TIE_ROWS = ("equal-logits", "across-the-chunk-boundary", "one-p-from-two-logits", "same-chunk")


def check_case_tables():
    assert {V for _, V, _, _ in KERNEL_CASES} >= {2, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3}
    assert {C for C, _, _, _ in KERNEL_CASES} >= {1, 3, 257} and {R for _, _, R, _ in KERNEL_CASES} >= {1, 2, 3, 8}
    assert {f for *_, f in KERNEL_CASES} == set(FAMILIES)
    assert all(C * V <= 500000 for C, V, _, _ in KERNEL_CASES)
    # the row loop of tg_consist_rows: one trip, two trips, three trips (the per-row LDS words alternate between two copies)
    assert {C for C, _, _, _ in GRID_CASES} >= {MAX_PARTS + 1, 2 * MAX_PARTS + 4} and all(C * V <= 500000 for C, V, _, _ in GRID_CASES)
    trips = {-(-(C - b) // min(C, parts)) for C, parts, *_ in ROW_LOOP_CASES for b in range(min(C, parts))}
    assert trips >= {1, 2, 3, 4, 5, 9} and all(parts < C for C, parts, *_ in ROW_LOOP_CASES)
    assert any(ld % 4 or o for _, _, _, ld, o, _ in ROW_LOOP_CASES) and any(ld % 4 == 0 and o == 0 for _, _, _, ld, o, _ in ROW_LOOP_CASES)
    assert any(n > CHUNK for _, _, n, *_ in ROW_LOOP_CASES) and {R for *_, R in ROW_LOOP_CASES} >= {1, 3, 8}
    assert any(parts > 256 for _, parts, *_ in ROW_LOOP_CASES)            # (and the finish kernel's second trip behind such a launch)
    assert any(C > 2 * MAX_PARTS and ld % 4 for C, _, ld, _, _ in PLANE_ROW_CASES) and any(C > MAX_PARTS and ld % 4 == 0 and o == 0 for C, _, ld, o, _ in PLANE_ROW_CASES)
    assert all(C * n <= 500000 for C, n, _, _, _ in PLANE_ROW_CASES)
    assert {n for n, _, _, _ in PLANE_CASES} >= {2, 5, 1000}
    assert any(ld > n for n, ld, _, _ in PLANE_CASES) and any(ld % 2 == 1 for _, ld, _, _ in PLANE_CASES) and any(o == 1 for _, _, o, _ in PLANE_CASES)
    assert MAX_RUNS == _capi.CONSIST_MAX_RUNS == 8


def check_limits():
    out = (ct.c_int32 * 3)()
    assert _capi.lib().tg_debug_consist_limits(out) == 0
    assert (out[0], out[1], out[2]) == (MAX_RUNS, CHUNK, MAX_PARTS) and MAX_PARTS >= 257


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def oracle_pearson(cube):
    cube = np.asarray(cube, dtype=np.float64)
    if cube.shape[0] < 2:
        return np.zeros(0)
    return np.corrcoef(cube.reshape(cube.shape[0], -1))[np.tril_indices(cube.shape[0], -1)]


def oracle_votes(cube):
    return np.argmax(np.asarray(cube), axis=2)


def oracle_vote_entropy(cube):
    R, C, V = np.asarray(cube).shape
    votes = oracle_votes(cube)
    out = np.zeros(C)
    for c in range(C):
        _, n = np.unique(votes[:, c], return_counts=True)
        f = n.astype(np.float64) / R
        out[c] = -(f * np.log(f)).sum() / np.log(V)
    return out


def oracle_consensus_entropy(cube):
    m = np.asarray(cube, dtype=np.float64).mean(axis=0)
    t = np.zeros_like(m)
    np.multiply(m, np.log(m, where=m > 0, out=np.zeros_like(m)), out=t)
    return -t.sum(axis=1) / np.log(m.shape[1])


def _np(t):
    return t.detach().cpu().numpy()


def _bits(x):
    x = np.ascontiguousarray(_np(x) if isinstance(x, torch.Tensor) else x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def assert_same_bits(a, b, where):
    assert set(a) == set(b), where
    for k in a:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{where}: {k}")


def assert_against_oracle(out, cube, where, spot_offset=0):
    """Every output in `out` against the fp64 statement on the dense planes `cube` (R, C, V); returns the deviations."""
    R, C, V = cube.shape
    dev = {}
    if "votes" in out:
        votes = _np(out["votes"])
        assert votes.shape == (R, C) and votes.dtype == np.int32
        np.testing.assert_array_equal(votes, oracle_votes(cube) + spot_offset, err_msg=f"{where}: votes (a vote >= {V} is a padding column)")
    if R > 1 and "pearson" in out:
        r = _np(out["pearson"])
        assert r.dtype == np.float64 and r.shape == (R * (R - 1) // 2,)
        dev["pearson"] = float(np.abs(r - oracle_pearson(cube)).max())
    else:
        assert "pearson" not in out
    if "vote_entropy" in out:
        dev["vote"] = float(np.abs(_np(out["vote_entropy"]).astype(np.float64) - oracle_vote_entropy(cube)).max())
    if "consensus_entropy" in out:
        dev["consensus"] = float(np.abs(_np(out["consensus_entropy"]).astype(np.float64) - oracle_consensus_entropy(cube)).max())
    print(f"consistency-dev {where}: " + " ".join(f"{k}={v:.3e}" for k, v in dev.items()))
    assert dev.get("pearson", 0.0) <= PEARSON_BOUND, (where, dev)
    assert dev.get("vote", 0.0) <= VOTE_BOUND, (where, dev)
    assert dev.get("consensus", 0.0) <= CONSENSUS_BOUND, (where, dev)
    return dev


# ---- handles --------------------------------------------------------------------------------------------------------------------
def _problem(C, K, V, seed):
    from tests import parity_common as pc
    return pc.validation_problem(C, K, V, seed)


def family_logits(family, R, C, V, seed):
    """R initial logit planes: independent N(0, 1) at scale 1 / 8 (r ~ 0), a shared plane plus 0.05 noise (r > 0.99), a shared plane
    plus 0.7 noise (r ~ 0.5 between the exponentials: (e - 1) / (e^1.49 - 1)); "trained" starts from independent planes and is stepped by the caller."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((C, V))
    scale = {"iid1": 1.0, "iid8": 8.0, "trained": 1.0}.get(family)
    if scale is not None:
        return [(scale * rng.standard_normal((C, V))).astype(np.float32) for _ in range(R)]
    noise = 0.05 if family == "shared" else 0.7
    return [(base + noise * rng.standard_normal((C, V))).astype(np.float32) for _ in range(R)]


def make_engines(device, C, V, logits, K=5, steps=None, seed=None):
    from tangram_amd.engine import HipMapperEngine
    S, G, d, _ = _problem(C, K, V, C + V if seed is None else seed)
    engines = [HipMapperEngine(S, G, M0, d=d, device=device, precision="bf16x3", lambdas=LAM) for M0 in logits]
    for e, n in zip(engines, steps or ()):
        if n:
            e.step(n, 0.1, e.new_history(n), 0)
    return engines


def _cube_of(engines):
    return np.stack([_np(e.result()) for e in engines])


def check_handles(engines, where):
    """tg_mapper_consistency of `engines`: against the oracle on their dense results, the same bits from tg_planes_consistency on
    those planes (the values flavour), and the same bits from a second call."""
    from tangram_amd import mapping_parameter_tuning as mpt
    out = mpt.mapper_consistency(engines, votes=True)
    cube = _cube_of(engines)
    dev = assert_against_oracle(out, cube, where)
    planes = mpt.planes_consistency(torch.as_tensor(cube, device=engines[0].device), votes=True)
    assert_same_bits(out, planes, f"{where}: logits flavour vs values flavour on the result planes")
    assert_same_bits(out, mpt.mapper_consistency(engines, votes=True), f"{where}: second call")
    return dev, cube


def check_kernel_case(device, C, V, R, family):
    steps = [3] * R if family == "trained" else None
    engines = make_engines(device, C, V, family_logits(family, R, C, V, 7 * C + V + R), steps=steps)
    dev, _ = check_handles(engines, f"C{C} V{V} R{R} {family}")
    for e in engines:
        e.release()
    return dev


def check_pearson_span(device, C=40, V=257):
    """The input families put the correlations at r ~ 0, r ~ 0.5 and r > 0.99."""
    from tangram_amd import mapping_parameter_tuning as mpt
    got = {}
    for family in ("iid1", "half", "shared"):
        engines = make_engines(device, C, V, family_logits(family, 3, C, V, 5))
        got[family] = _np(mpt.mapper_consistency(engines)["pearson"])
        for e in engines:
            e.release()
    assert np.abs(got["iid1"]).max() < 0.1 and (got["shared"] > 0.99).all() and ((got["half"] > 0.3) & (got["half"] < 0.7)).all(), got


def check_steps_and_modes(device):
    """Handles standing at different steps (0, 1, 4), and a constrained pair: softmax(M) without the filter."""
    from tangram_amd.engine import HipMapperEngine
    from oracle import tangram_oracle as orc
    C, V = 40, 130
    engines = make_engines(device, C, V, family_logits("shared", 3, C, V, 3), steps=[0, 1, 4])
    assert [e.logits()[3] for e in engines] == [0, 1, 4]
    check_handles(engines, "steps 0 / 1 / 4")
    for e in engines:
        e.release()
    C, K, V = 40, 12, 100
    data = orc.make_synthetic(C, K, V, seed=5)
    lam = dict(lambda_g1=1.0, lambda_d=1.0, lambda_g2=0.5, lambda_count=1.0, lambda_f_reg=1.0)
    engines = []
    for seed in (6, 7):
        M0, F0 = orc.reference_init_MF_constrained(C, V, seed)
        engines.append(HipMapperEngine(data["S"], data["G"], M0, d=data["d"], F0=F0, mode="constrained", device=device, lambdas=lam, target_count=20.0))
        engines[-1].step(3, 0.1, engines[-1].new_history(3), 0)
    _, cube = check_handles(engines, "constrained")
    np.testing.assert_array_equal(cube[0], _np(engines[0].result(with_filter=True)[0]))
    for e in engines:
        e.release()


def tie_logits():
    """(M0 [4, V] of run 0, expected votes of run 0): rows a comparison of logits, or of values without the column, gets wrong."""
    V = CHUNK + 70
    M = np.full((4, V), -4.0, dtype=np.float32)
    M[0] = 0.25                                                          # all equal: column 0
    M[1, CHUNK - 3] = M[1, CHUNK + 5] = 3.0                              # the maximum on both sides of the chunk boundary
    M[2] = -30.0                                                         # two different logits, ONE p (1e-9 vanishes against the row shift):
    M[2, 7], M[2, 3] = 1e-9, 0.0                                         # the larger logit sits at the higher column
    M[3, 5] = M[3, 700] = M[3, 1030] = 3.0                               # one chunk, three threads (column 1030 is thread 1's second quad)
    return M, [0, CHUNK - 3, 3, 5]


def check_ties(device):
    from tangram_amd import mapping_parameter_tuning as mpt
    M0, expect = tie_logits()
    C, V = M0.shape
    other = np.ascontiguousarray(M0[:, ::-1])                             # run 1: the mirrored rows
    engines = make_engines(device, C, V, [M0, other])
    _, cube = check_handles(engines, "ties")
    assert cube[0][2, 3] == cube[0][2, 7] and M0[2, 7] > M0[2, 3], "row 2 must hold one p from two logits"
    assert len(np.unique(cube[0][0])) == 1
    votes = _np(mpt.mapper_consistency(engines, votes=True)["votes"])
    assert votes[0].tolist() == expect, votes[0].tolist()
    assert votes[1].tolist() == [0, V - 1 - (CHUNK + 5), V - 1 - 7, V - 1 - 1030], votes[1].tolist()
    assert (votes < V).all() and (votes >= 0).all()
    for e in engines:
        e.release()


# ---- plain planes -----------------------------------------------------------------------------------------------------------------
def check_plane_case(device, n_cols, ld, offset, R, C=6):
    """The values flavour on planes cut out of one buffer at pitch `ld`, the first one `offset` floats off a 16-byte boundary, the
    columns behind n_cols and the gaps between the planes filled with 1e30: the oracle, and the bits of the same values in
    contiguous aligned planes."""
    from tangram_amd import mapping_parameter_tuning as mpt
    dev = torch.device(device)
    rng = np.random.default_rng(n_cols * 31 + ld + offset + R)
    vals = rng.random((R, C, n_cols)).astype(np.float32)
    vals /= vals.sum(axis=2, keepdims=True)
    vals[:, 0, :] = vals[0, 0, :]                                        # a row every run agrees on
    if n_cols >= 5:
        vals[:, 1, 1] = vals[:, 1, 4] = 0.9                              # a duplicated maximum: column 1
    plane_floats = C * ld + 4 + offset                                   # (the next plane starts 16-byte aligned again, + offset)
    plane_floats += (-plane_floats) % 4
    buf = torch.full((R * plane_floats + 8,), 1e30, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    planes = []
    for r in range(R):
        p = buf[r * plane_floats + offset: r * plane_floats + offset + C * ld].view(C, ld)[:, :n_cols]
        p.copy_(torch.as_tensor(vals[r]))
        planes.append(p)
        assert p.data_ptr() % 16 == (4 * offset) % 16 and p.stride(0) == ld
    where = f"planes n{n_cols} ld{ld} off{offset} R{R}"
    out = mpt.planes_consistency(planes, votes=True)
    assert_against_oracle(out, vals, where)
    assert_same_bits(out, mpt.planes_consistency(torch.as_tensor(vals, device=dev), votes=True), f"{where}: against contiguous aligned planes")
    assert_same_bits(out, mpt.planes_consistency(planes, votes=True), f"{where}: second call")
    assert (_np(out["votes"]) < n_cols).all()
    assert float(buf[R * plane_floats:].min()) == float(buf.max()) == float(np.float32(1e30))      # the inputs are read only


def check_row_loop_case(device, n_rows, max_parts, n_cols, ld, offset, R):
    """The pass with at most `max_parts` workgroups against the oracle, and against the shipped launch of the same planes (one row per
    workgroup here): votes and entropies are per-row results, the same bits; the correlations sum the same moments in another
    order, each within the bound of the oracle."""
    from tangram_amd import mapping_parameter_tuning as mpt
    dev = torch.device(device)
    assert max_parts < n_rows <= MAX_PARTS
    rng = np.random.default_rng(n_rows * 131 + max_parts * 17 + n_cols)
    vals = rng.random((R, n_rows, n_cols)).astype(np.float32) ** 4          # (peaked rows: the votes differ from row to row)
    vals /= vals.sum(axis=2, keepdims=True)
    buf = torch.full((R, n_rows * ld + 4), 1e30, dtype=torch.float32, device=dev)
    planes = [buf[r, offset: offset + n_rows * ld].view(n_rows, ld)[:, :n_cols] for r in range(R)]
    for p, v in zip(planes, vals):
        p.copy_(torch.as_tensor(v))
    where = f"row loop rows{n_rows} parts{max_parts} n{n_cols} ld{ld} off{offset} R{R}"
    out = mpt.planes_consistency(planes, votes=True, _max_parts=max_parts)
    assert_against_oracle(out, vals, where)
    assert_same_bits(out, mpt.planes_consistency(planes, votes=True, _max_parts=max_parts), f"{where}: second call")
    full = mpt.planes_consistency(planes, votes=True)
    assert_against_oracle(full, vals, where + " (one row per workgroup)")
    per_row = ("votes", "vote_entropy", "consensus_entropy")
    assert_same_bits({k: out[k] for k in per_row}, {k: full[k] for k in per_row}, f"{where}: against one row per workgroup")
    for bad in (0, MAX_PARTS + 1):
        with pytest.raises(ValueError, match="workgroups"):
            mpt.planes_consistency(planes, _max_parts=bad)


# ---- state, errors -----------------------------------------------------------------------------------------------------------------
def _state_of(e):
    M, m1, m2, step = e.logits()
    return [_np(x).copy() for x in (M, m1, m2)] + [step]


def check_undisturbed(device, C=40, V=257):
    """2 steps, the consistency call, 2 steps == 4 steps on a twin that was never scored: history, logits, both Adam moments."""
    from tangram_amd import mapping_parameter_tuning as mpt
    logits = family_logits("iid1", 2, C, V, 11)
    res = []
    for ask in (True, False):
        engines = make_engines(device, C, V, logits)
        hists = [e.new_history(4) for e in engines]
        for e, h in zip(engines, hists):
            e.step(2, 0.1, h, 0)
        if ask:
            mpt.mapper_consistency(engines, votes=True)
        for e, h in zip(engines, hists):
            e.step(2, 0.1, h, 2)
        res.append([[_np(h).copy()] + _state_of(e) for e, h in zip(engines, hists)])
        for e in engines:
            e.release()
    for r in range(2):
        for name, x, y in zip(("history", "M", "exp_avg", "exp_avg_sq", "step"), res[0][r], res[1][r]):
            np.testing.assert_array_equal(x, y, err_msg=f"run {r}: {name}")


def check_argument_errors(device):
    """Every refusal reaches Python as ValueError (TG_ERR_INVALID) or RuntimeError with the library's message, writes nothing and
    leaves the handles usable."""
    from tangram_amd import mapping_parameter_tuning as mpt
    from tangram_amd.engine import HipMapperEngine
    lib = _capi.lib()
    dev = torch.device(device)
    C, V = 40, 70
    logits = family_logits("iid1", 2, C, V, 1)
    engines = make_engines(device, C, V, logits)
    e0 = engines[0]
    S, G, d, _ = _problem(C, 5, V, C + V)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    pear = torch.full((28,), 7.0, dtype=torch.float64, device=dev)
    ent = torch.full((C,), 7.0, dtype=torch.float32, device=dev)

    def handles(*es):
        return (ct.c_void_p * len(es))(*[e._h if e is not None else None for e in es])

    def call_m(arr, n, w=ws.data_ptr(), p=pear.data_ptr(), v=ent.data_ptr()):
        e0._call(lib.tg_mapper_consistency, arr, n, w, p, v, None, None)

    with pytest.raises(ValueError, match="NULL"):
        call_m(None, 2)
    with pytest.raises(ValueError, match="handle 1 is NULL"):
        call_m(handles(e0, None), 2)
    for n in (0, -1, 9):
        with pytest.raises(ValueError, match="outside"):
            call_m(handles(*([e0] * 9)), n)
    with pytest.raises(ValueError, match="workspace"):
        call_m(handles(*engines), 2, w=None)
    with pytest.raises(ValueError, match="every output is NULL"):
        call_m(handles(*engines), 2, p=None, v=None)
    other = make_engines(device, C, V + 1, family_logits("iid1", 1, C, V + 1, 2))[0]           # another n_spots (same pitch)
    with pytest.raises(ValueError, match="handle 1 is"):
        call_m(handles(e0, other), 2)
    other.release()
    other = make_engines(device, C + 1, V, family_logits("iid1", 1, C + 1, V, 2))[0]           # another n_cells
    with pytest.raises(ValueError, match="handle 1 is"):
        call_m(handles(e0, other), 2)
    other.release()
    other = make_engines(device, C, 64, family_logits("iid1", 1, C, 64, 2))[0]                 # (64 and 70 spots: pitches 64 and 128)
    with pytest.raises(ValueError, match="pitch"):
        call_m(handles(e0, other), 2)
    other.release()
    one = make_engines(device, C, 1, family_logits("iid1", 2, C, 1, 2))                        # one spot: log(1) = 0
    with pytest.raises(ValueError, match="two columns"):
        mpt.mapper_consistency(one)
    for e in one:
        e.release()
    shard = HipMapperEngine(S, G, logits[1], d=d, device=device, precision="bf16x3", lambdas=LAM, n_ranks=1)
    with pytest.raises(RuntimeError, match="spot shard") as ei:
        mpt.mapper_consistency([e0, shard])
    assert not isinstance(ei.value, ValueError)
    shard.release()
    if dev.type == "cuda":                                                                     # (the emulator has one stream)
        with torch.cuda.stream(torch.cuda.Stream(device=dev)):
            foreign = HipMapperEngine(S, G, logits[1], d=d, device=device, precision="bf16x3", lambdas=LAM)
        torch.cuda.synchronize(dev)
        with pytest.raises(ValueError, match="same stream"):
            mpt.mapper_consistency([e0, foreign])
        foreign.release()
    # plain planes
    x = torch.rand((2, 6, 8), dtype=torch.float32, device=dev)
    planes = (ct.c_void_p * 2)(x[0].data_ptr(), x[1].data_ptr())
    stream = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None

    def call_p(arr=planes, n=2, rows=6, cols=8, ld=8, w=ws.data_ptr(), p=pear.data_ptr()):
        _capi.check(lib.tg_planes_consistency(arr, n, rows, cols, ld, w, p, ent.data_ptr(), None, None, stream))

    with pytest.raises(ValueError, match="NULL"):
        call_p(arr=None)
    with pytest.raises(ValueError, match="plane 1 is NULL"):
        call_p(arr=(ct.c_void_p * 2)(x[0].data_ptr(), None))
    for n in (0, 9):
        with pytest.raises(ValueError, match="outside"):
            call_p(n=n)
    with pytest.raises(ValueError, match="two columns"):
        call_p(cols=1)
    with pytest.raises(ValueError, match="at least one row"):
        call_p(rows=0)
    with pytest.raises(ValueError, match="pitch"):
        call_p(ld=7)
    for rows, cols in ((1 << 31, 8), (6, (1 << 31) - 1)):
        with pytest.raises(ValueError, match="32-bit"):
            call_p(rows=rows, cols=cols, ld=max(cols, 8))
    with pytest.raises(ValueError, match="workspace"):
        call_p(w=None)
    nbytes = ct.c_size_t(7)
    for n, rows in ((0, 5), (9, 5), (3, 0), (3, 1 << 31)):
        with pytest.raises(ValueError, match="outside"):
            _capi.check(lib.tg_consistency_query_bytes(n, rows, ct.byref(nbytes)))
    with pytest.raises(ValueError, match="NULL"):
        _capi.check(lib.tg_consistency_query_bytes(3, 5, None))
    assert nbytes.value == 7
    with pytest.raises(ValueError, match="at least two runs"):
        mpt.pearson_corr(x[:1])
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    assert float(pear.min()) == 7.0 and float(ent.min()) == 7.0 and int(ws.max()) == 0, "a refused call wrote something"
    check_handles(engines, "after the refused calls")
    # R = 1: no pair, pearson_out is not touched
    e0._call(lib.tg_mapper_consistency, handles(e0), 1, ws.data_ptr(), pear.data_ptr(), ent.data_ptr(), None, None)
    assert float(pear.min()) == 7.0 and float(ent.max()) < 7.0
    for e in engines:
        e.release()


# ---- the public surface ----------------------------------------------------------------------------------------------------------
def tuning_problem(C, K, V, n_val=5, seed=21):
    from oracle import tangram_oracle as orc
    data = orc.make_synthetic(C, K, V, seed=seed)
    tr, va = np.arange(0, K - n_val), np.arange(K - n_val, K)
    return data, tr, va


def oracle_trial(device, data, tr, va, config, n_runs=3, seed0=77):
    """The five metrics the reference's way: `train_many(val_each=1)`, the dense mappings on the host, NumPy in fp64."""
    import tangram_amd as tg
    import tangram_amd.mapping_optimizer as mo
    lam = {k: v for k, v in config.items() if k.startswith("lambda_")}
    np.random.seed(seed0)                                                 # (run 0 is "unseeded": it draws from the global stream)
    builders = [(lambda run=run: mo.Mapper(S=data["S"], G=data["G"], d=data["d"], train_genes_idx=tr, val_genes_idx=va, device=device,
                                           random_state=run, **lam)) for run in range(n_runs)]
    res, mappers = tg.train_many(builders, config["num_epochs"], config.get("learning_rate", 0.1), device=device, val_each=1)
    cube = np.stack([P for P, _ in res])
    S_val = data["S"][:, va].astype(np.float64)
    genes = np.stack([S_val.T @ P.astype(np.float64) for P, _ in res])
    for m in mappers:
        m.release()
    return {"cell_map_consistency": oracle_pearson(cube).mean(), "cell_map_agreement": 1 - oracle_vote_entropy(cube).mean(),
            "cell_map_certainty": 1 - oracle_consensus_entropy(cube).mean(), "gene_expr_consistency": oracle_pearson(genes).mean(),
            "gene_expr_correctness": np.array([h["val_gene_sim"][-1] for _, h in res]).mean()}, cube


def trial_deviation(device, C, K, V, epochs=4, seed0=77):
    """(train_multiple_Mapper's dict, the oracle's dict, the dense cube) of one trial."""
    import tangram_amd as tg
    data, tr, va = tuning_problem(C, K, V)
    config = dict(num_epochs=epochs, learning_rate=0.1, lambda_d=1, lambda_g1=1, lambda_g2=0.5)
    ref, cube = oracle_trial(device, data, tr, va, config, seed0=seed0)
    np.random.seed(seed0)
    pack = [data["S"], data["G"], None, data["d"], device, None, None, None, None, None, tr, va]
    got = tg.train_multiple_Mapper(config, pack)
    return got, ref, cube


def check_public_surface(device):
    import tangram_amd as tg
    got, ref, cube = trial_deviation(device, 20, 40, 130)
    assert list(got) == list(tg.mapping_parameter_tuning.METRICS) and all(isinstance(v, float) for v in got.values())
    print("consistency-dev trial: " + " ".join(f"{k}={abs(got[k] - ref[k]):.3e}" for k in got))
    assert got["gene_expr_correctness"] == ref["gene_expr_correctness"], "ONE final validation must be val_gene_sim[-1], bit for bit"
    assert abs(got["cell_map_consistency"] - ref["cell_map_consistency"]) <= PEARSON_BOUND
    assert abs(got["cell_map_agreement"] - ref["cell_map_agreement"]) <= VOTE_BOUND
    assert abs(got["cell_map_certainty"] - ref["cell_map_certainty"]) <= CONSENSUS_BOUND
    assert abs(got["gene_expr_consistency"] - ref["gene_expr_consistency"]) <= GENE_EXPR_BOUND
    # the three cube functions: host array, device tensor, list of planes -- the same answers, the reference's shapes and dtypes
    dev = torch.device(device)
    t = torch.as_tensor(cube, device=dev)
    for fn, orc_fn, bound, shape in ((tg.pearson_corr, oracle_pearson, PEARSON_BOUND, (3,)), (tg.vote_entropy, oracle_vote_entropy, VOTE_BOUND, (20,)),
                                     (tg.consensus_entropy, oracle_consensus_entropy, CONSENSUS_BOUND, (20,))):
        a, b, c = fn(cube, device=device), fn(t), fn([t[0], t[1], t[2]])
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == shape
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
        assert np.abs(a - orc_fn(cube)).max() <= bound, fn.__name__
    # narrow planes are re-cut into long rows: the same correlation
    narrow = np.random.default_rng(3).random((3, 900, 7)).astype(np.float32)
    assert np.abs(tg.pearson_corr(narrow, device=device) - oracle_pearson(narrow)).max() <= PEARSON_BOUND
    # one-column planes (a single validation gene) whose element count, a prime, cannot be re-cut: one row of all elements
    column = np.random.default_rng(4).random((3, 8209, 1)).astype(np.float32)
    assert np.abs(tg.pearson_corr(column, device=device) - oracle_pearson(column)).max() <= PEARSON_BOUND
    assert np.abs(tg.pearson_corr(torch.as_tensor(column, device=dev)[:, ::2], device=device) - oracle_pearson(column[:, ::2])).max() <= PEARSON_BOUND
    with pytest.raises(ValueError, match="at least two runs"):
        tg.pearson_corr(cube[:1], device=device)


# ---- the oracle against the reference's own functions (CPU only; skipped without the reference tree) -----------------------------------
def reference_source():
    """The reference's tuning module next to the hot-path module oracle/make_ref.py stages (the test is skipped when the reference tree is absent)."""
    from oracle import make_ref
    return os.path.join(os.path.dirname(make_ref.REF_SRC), "mapping_parameter_tuning.py")


def reference_functions():
    """pearson_corr, vote_entropy, consensus_entropy of the reference, taken out of its source at run time (the module itself pulls
    scanpy in): only those three `def`s are executed, with np and scipy in scope."""
    import ast
    import scipy
    import scipy.stats  # noqa: F401
    src = reference_source()
    tree = ast.parse(open(src).read())
    names = ("pearson_corr", "vote_entropy", "consensus_entropy")
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(defs) == 3
    scope = {"np": np, "scipy": scipy}
    exec(compile(ast.Module(body=defs, type_ignores=[]), src, "exec"), scope)
    return [scope[n] for n in names]


def check_oracle_against_reference():
    ref_p, ref_v, ref_c = reference_functions()
    rng = np.random.default_rng(0)
    for R, C, V, scale in ((3, 7, 63, 1.0), (2, 5, 1000, 8.0), (8, 4, 130, 0.0)):
        M = scale * rng.standard_normal((R, C, V))
        M[:, 0, :] = M[0, 0, :]                                          # a row every run agrees on; scale 0: uniform rows, all votes 0
        e = np.exp(M - M.max(axis=2, keepdims=True))
        cube64 = e / e.sum(axis=2, keepdims=True)
        cube = cube64.astype(np.float32)
        if scale:
            assert np.abs(oracle_pearson(cube) - ref_p(cube)).max() <= 1e-12
            assert np.abs(oracle_pearson(cube64) - ref_p(cube64)).max() <= 1e-12
        assert np.abs(oracle_vote_entropy(cube) - ref_v(cube)).max() <= 1e-12
        # scipy.stats.entropy divides by the row sum first: on rows that sum to 1 in fp64 the two statements agree to rounding ...
        assert np.abs(oracle_consensus_entropy(cube64) - ref_c(cube64)).max() <= 1e-12
        # ... and on the float32 cube the reference takes the mean and the entropy in fp32: its own noise, bounded like the device's
        assert np.abs(oracle_consensus_entropy(cube) - ref_c(cube)).max() <= CONSENSUS_BOUND
