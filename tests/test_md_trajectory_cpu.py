"""The host side of the trajectory recorder, without a GPU: the spacing policies of timewarp_amd/simulation.py against the
report steps the reference's own policies give (tests/golden/spacing_steps.npz, written by tools/gen_spacing_golden.py),
`report_steps`, the refusal of bad report steps by `LangevinDynamics.trajectory`, the launch planner of
`simulate_trajectory`, and the float64 restatement tests/trajectory_oracle.py against tests/langevin_oracle.py."""
import os

import numpy as np
import pytest
import torch

from tests import langevin_oracle as lo
from tests import trajectory_oracle as to
from timewarp_amd import simulation as S

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "spacing_steps.npz")
KINDS = ["regular", "logarithmic", "windowed"]


def build(kind, args):
    if kind == "regular":
        return S.RegularSpacing(*args)
    if kind == "logarithmic":
        return S.LogarithmicSpacing(*args)
    interval, window, subsamples, seed = args
    return S.UniformWindowedSpacing(interval, spacing_window=window, subsamples=subsamples, seed=seed)


def golden_cases():
    z = np.load(GOLDEN)
    for key in sorted(z.files):
        if key.endswith("__params"):
            p = [int(v) for v in z[key]]
            yield key[:-len("__params")], KINDS[p[0]], p[3:], p[1], p[2], z[key[:-len("__params")] + "__steps"]


def test_every_policy_reproduces_the_reference_report_steps():
    """All three policies, exactly; the windowed cases walk through three windows and more with fixed seeds."""
    seen = set()
    for name, kind, args, start, stop, want in golden_cases():
        got = S.report_steps(build(kind, args), start, stop)
        assert got.dtype == np.int64 and want.dtype == np.int64
        assert np.array_equal(got, want), (name, got[:10], want[:10])
        assert len(want) >= 5
        seen.add(kind)
    assert seen == set(KINDS)


def test_windowed_golden_cases_cross_three_windows():
    for name, kind, args, start, stop, want in golden_cases():
        if kind == "windowed":
            interval = args[0]
            centres = [c for c in range(0, stop + 1, interval) if start < c <= stop and c in want]
            assert len(centres) >= 3, (name, centres)
            assert len(set(want.tolist())) == len(want) and np.all(np.diff(want) > 0)


def test_logarithmic_spacing_docstring_example():
    """npzreporter.py:48-53: interval 10000, factor 10 -> 10000, 10001, 10010, 10100, 11000, 20000, 20001, ..."""
    got = S.report_steps(S.LogarithmicSpacing(10000, 10), 10000, 30000)
    assert got.tolist() == [10001, 10010, 10100, 11000, 20000, 20001, 20010, 20100, 21000, 30000]
    with pytest.raises(ValueError):
        S.LogarithmicSpacing(100, 1)


@pytest.mark.parametrize("kind,args", [("regular", (5,)), ("regular", (1,)), ("logarithmic", (10, 3)), ("logarithmic", (16, 2)),
                                       ("windowed", (20, 4, 3, 1))])
def test_report_steps_excludes_start_and_includes_stop(kind, args):
    """(start, stop]: `start` is never returned, even when it is a report step; `stop` is whenever it is one."""
    full = S.report_steps(build(kind, args), 0, 200)
    assert len(full) > 10 and np.all(np.diff(full) > 0) and full[0] > 0
    for start in (0, int(full[2]), int(full[2]) + 1, int(full[5])):
        for stop in (int(full[7]), int(full[7]) + 1, int(full[9]), start):
            got = S.report_steps(build(kind, args), start, stop)
            assert start not in got
            if kind != "windowed":     # (a windowed policy draws its windows as it is asked: another start is another sequence)
                assert np.array_equal(got, full[(full > start) & (full <= stop)])
                assert (stop in got) == (stop in full and stop > start)
            assert np.all(got > start) and np.all(got <= stop)
    # a windowed policy always keeps the multiples of its interval
    if kind == "windowed":
        assert all(c in full for c in (20, 40, 200))
        assert full[-1] == 200


def test_windowed_spacing_refuses_steps_that_go_back():
    sp = S.UniformWindowedSpacing(20, 4, 3, seed=0)
    sp.steps_until_next_report(10)
    with pytest.raises(ValueError):
        sp.steps_until_next_report(10)


# ---------------------------------------------------------------------------------------------
# LangevinDynamics.trajectory refuses bad report steps before anything reaches the device
# ---------------------------------------------------------------------------------------------
def _dynamics(V=3):
    from tests.test_langevin_cpu import bond_only_tables
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from timewarp_amd.md import LangevinDynamics

    return LangevinDynamics(AmberPotentialEnergyTorch(bond_only_tables()), torch.ones(2), seed=1)


@pytest.mark.parametrize("steps,num_steps,why", [([3, 2], None, "unordered"), ([0, 2, 2, 5], None, "repeated"), ([-1, 2], None, "negative"),
                                                 ([1, 6], 5, "beyond num_steps"), ([0, 1, 5, 4], 5, "unordered"), ([[1, 2]], None, "not flat"),
                                                 ([1.5], None, "not whole"), ([], None, "no num_steps"), ([1], -1, "negative num_steps"),
                                                 ([1], 2 ** 31, "int32")])
def test_trajectory_refuses_bad_report_steps(steps, num_steps, why):
    md = _dynamics()
    x = torch.zeros(1, 2, 3)      # CPU tensors: a list that passed would fail later, with RuntimeError ("no CPU fallback")
    with pytest.raises(ValueError):
        md.trajectory(x, x, steps, num_steps=num_steps)
    assert md.steps_done == 0


def test_good_report_steps_pass_the_check():
    from timewarp_amd.md import check_report_steps

    r, n = check_report_steps([0, 1, 5, 13])
    assert r.dtype == np.int32 and r.tolist() == [0, 1, 5, 13] and n == 13
    assert check_report_steps([], 7)[1] == 7 and check_report_steps(np.array([0]), 0)[1] == 0
    assert check_report_steps([2.0, 3.0], 9)[0].tolist() == [2, 3]
    md = _dynamics()
    with pytest.raises(RuntimeError, match="no CPU fallback|MI355X"):     # past the check, stopped by the missing device
        md.trajectory(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), [0, 1])


# ---------------------------------------------------------------------------------------------
# the launch planner
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 10 ** 6])
@pytest.mark.parametrize("burn_in,sampling,spacing", [(3, 24, ("logarithmic", (10, 3))), (0, 50, ("regular", (7,))), (13, 0, ("regular", (1,))),
                                                      (20, 100, ("windowed", (40, 8, 3, 5))), (5, 5, ("regular", (100,)))])
def test_launch_plan_covers_the_run_once_and_places_every_report(chunk, burn_in, sampling, spacing):
    reports = S.report_steps(build(*spacing), burn_in, burn_in + sampling)
    plan = S.plan_launches(burn_in, sampling, reports, chunk)
    # the chunks tile [0, burn_in + sampling) in order, none empty or longer than asked, burn-in and sampling not mixed
    at = 0
    placed = []
    for first, n_steps, rel in plan:
        assert first == at and 1 <= n_steps <= chunk
        assert first + n_steps <= burn_in or first >= burn_in
        assert rel.dtype == np.int64 and np.all(rel >= 1) and np.all(rel <= n_steps) and np.all(np.diff(rel) > 0)
        if first < burn_in:
            assert rel.size == 0
        placed += [first + int(r) for r in rel]
        at += n_steps
    assert at == burn_in + sampling
    assert placed == reports.tolist()        # every report once, in order, at its own step
    if chunk >= 10 ** 6:
        assert len(plan) == (burn_in > 0) + (sampling > 0)
    # same plan twice: a pure function
    again = S.plan_launches(burn_in, sampling, reports, chunk)
    assert [(a, b, c.tolist()) for a, b, c in plan] == [(a, b, c.tolist()) for a, b, c in again]


def test_launch_plan_refuses_reports_outside_the_sampling():
    for bad in ([3], [2], [28], [5, 5], [9, 8]):
        with pytest.raises(ValueError):
            S.plan_launches(3, 24, bad, 7)
    with pytest.raises(ValueError):
        S.plan_launches(3, 24, [4], 0)


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
def test_the_restated_recorder_is_the_restated_integrator(scheme):
    """A frame at step r holds what `lo.langevin_steps` returns after r steps; frames do not depend on which other steps
    are reported; E_kin is 1/2 sum m v^2; force-free forces and energies are 0."""
    rng = np.random.default_rng(5)
    V, n = 5, 2
    m = (1.0 + 0.37 * np.arange(V)).astype(np.float32)
    x, v = rng.standard_normal((n, V, 3)).astype(np.float32), rng.standard_normal((n, V, 3)).astype(np.float32)
    args = (0.0005, 50.0, 2.5, scheme, 99, 1000003)
    full = to.record(lo.no_forces, m, x, v, list(range(14)), 13, *args)
    some = to.record(lo.no_forces, m, x, v, [0, 1, 5, 13], 13, *args)
    assert full["positions"].shape == (n, 14, V, 3) and full["energies"].shape == (n, 14, 2)
    for k, r in enumerate([0, 1, 5, 13]):
        wx, wv, _ = lo.langevin_steps(lo.no_forces, m, x, v, r, *args)
        for got in (full["positions"][:, r], some["positions"][:, k]):
            assert np.array_equal(got, wx)
        for got in (full["velocities"][:, r], some["velocities"][:, k]):
            assert np.array_equal(got, wv)
        assert np.array_equal(full["energies"][:, r], some["energies"][:, k])
    assert np.array_equal(full["positions"][:, 0], x) and np.array_equal(some["final_x"], full["positions"][:, 13])
    ek = 0.5 * (m.astype(np.float64)[None, None, :, None] * full["velocities"].astype(np.float64) ** 2).sum(axis=(2, 3))
    assert np.all(np.abs(full["energies"][..., 1] - ek) <= 2.0 ** -22 * ek)
    assert np.count_nonzero(full["forces"]) == 0 and np.count_nonzero(full["energies"][..., 0]) == 0
    none = to.record(lo.no_forces, m, x, v, [], 13, *args)
    assert none["positions"].shape == (n, 0, V, 3) and np.array_equal(none["final_v"], full["final_v"])
