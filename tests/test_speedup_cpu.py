"""The host side of the speed-up report (timewarp_amd/analysis.py `coverage_distance` ... `speedup_report`, timewarp_amd/speedup.py):
the restatement tests/coverage_oracle.py against the notebook's literal scipy expression, the first-zero ESS against the notebook's
formula, the loaders, and the report driver with the torch route standing in for the kernel (it needs no GPU)."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from tests import coverage_oracle as co
from tests.conftest import ROOT
from timewarp_amd import analysis as an
from timewarp_amd import sample_trajectory as st
from timewarp_amd import speedup


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_ref,n_cloud", [(1, 1), (37, 300), (513, 770)])
def test_restatement_matches_the_notebook_expression(n_ref, n_cloud):
    from scipy.spatial import distance

    A, B = co.random_case(n_ref, n_cloud, 2)
    notebook = distance.cdist(A, B).min(axis=1).max()
    _, worst, arg = co.random_truth(n_ref, n_cloud, 2, 1)
    bound = 2.0 * co.worst_bound(2)          # the restatement's side and cdist's own rounding (module docstring of the oracle)
    assert abs(np.longdouble(notebook) - worst[0]) <= bound * worst[0], (notebook, float(worst[0]))
    assert int(arg[0]) == int(np.argmax(distance.cdist(A, B).min(axis=1)))


def test_restatement_groups_ties_and_empty_groups():
    ref = np.array([[0.0, 0.0], [5.0, 0.0], [0.0, 5.0], [5.0, 0.0]])
    cloud = np.array([[0.0, 0.0], [5.0, 0.0], [9.0, 9.0], [0.0, 1.0], [5.0, 0.0]])    # groups: rows (0, 3), (1, 4), (2)
    m, w, a = co.coverage(ref, cloud, 3)
    assert m[0].tolist() == [0.0, 25.0, 16.0, 25.0] and m[1].tolist() == [25.0, 0.0, 50.0, 0.0] and m[2].tolist() == [162.0, 97.0, 97.0, 97.0]
    assert w[0] == 5.0 and w[1] == np.sqrt(np.longdouble(50.0)) and a.tolist() == [1, 2, 0]      # the tie goes to row 1, not 3
    m, w, a = co.coverage(ref, cloud[:2], 3)                                            # group 2 has no rows
    assert np.isinf(m[2]).all() and np.isinf(w[2]) and a[2] == 0 and np.isfinite(m[:2]).all()
    m0, w0, a0 = co.coverage(ref, np.zeros((0, 2)), 1)
    assert np.isinf(m0).all() and np.isinf(w0[0]) and a0.tolist() == [0]
    assert co.EXTENDED or co.SLACK == 2.0


# ---- coverage_distance, torch route -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_groups", [1, 3])
def test_torch_route_matches_the_restatement(n_groups):
    A, B = co.random_case(130, 1001, 3)
    exact_m, exact_w, exact_a = co.random_truth(130, 1001, 3, n_groups)
    worst, arg, min_d = an.coverage_distance(A, B, dims=3, n_groups=n_groups, normalise=False, return_min=True, route="torch", chunk=64)
    assert isinstance(worst, np.ndarray) and worst.dtype == np.float64 and arg.dtype == np.int64 and min_d.shape == (n_groups, 130)
    bound = 2.0 * co.worst_bound(3)
    assert (np.abs(worst.astype(co.LD) - exact_w) <= bound * exact_w).all()
    assert (np.abs(min_d.astype(co.LD) - np.sqrt(exact_m)) <= bound * np.sqrt(exact_m)).all()
    co.check_arg(arg, exact_m, exact_a, 3)
    # tensors in, tensors out; two results without return_min
    out = an.coverage_distance(torch.as_tensor(A), torch.as_tensor(B), dims=3, n_groups=n_groups, normalise=False, route="torch")
    assert len(out) == 2 and isinstance(out[0], torch.Tensor) and np.array_equal(out[0].numpy(), worst)


def test_coverage_distance_normalises_by_the_reference_ranges_and_refuses():
    A, B = co.random_case(37, 300, 2)
    A3 = np.concatenate([A, np.ones((37, 1))], axis=1)           # a third column that dims=2 must ignore
    w_n, a_n = an.coverage_distance(A3, np.concatenate([B, np.zeros((300, 1))], axis=1), route="torch")
    ranges = np.abs(A).max(0)
    w_ref, a_ref = an.coverage_distance(A / ranges, B / ranges, normalise=False, route="torch")
    assert np.array_equal(w_n, w_ref) and np.array_equal(a_n, a_ref)
    # an empty group: +inf and arg 0
    w, a = an.coverage_distance(A, B[:2], n_groups=3, route="torch")
    assert np.isinf(w[2]) and a[2] == 0 and np.isfinite(w[:2]).all()
    flat = A.copy()
    flat[:, 1] = 0.0
    with pytest.raises(ValueError, match="zero range in TIC 1"):
        an.coverage_distance(flat, B, route="torch")
    for bad in (np.nan, np.inf):
        broken = B.copy()
        broken[7, 0] = bad
        with pytest.raises(ValueError, match="cloud_tics holds non-finite"):
            an.coverage_distance(A, broken, route="torch")
        with pytest.raises(ValueError, match="ref_tics holds non-finite"):
            an.coverage_distance(broken, A, route="torch")
    with pytest.raises(ValueError, match="dims 9"):
        an.coverage_distance(np.zeros((3, 9)), np.zeros((3, 9)), dims=9, route="torch")
    with pytest.raises(ValueError, match="n_groups 0"):
        an.coverage_distance(A, B, n_groups=0, route="torch")
    with pytest.raises(ValueError, match="route"):
        an.coverage_distance(A, B, route="host")
    assert an.DEFAULT_COVERAGE_ROUTE in an.COVERAGE_ROUTES


# ---- first-zero ESS ----------------------------------------------------------------------------------------------------------------

def ar1(T, phi, seed):
    rng = np.random.default_rng(seed)
    e = rng.normal(size=T)
    s = np.zeros(T)
    for t in range(1, T):
        s[t] = phi * s[t - 1] + e[t]
    return s


@pytest.mark.parametrize("phi,seed", [(0.9, 0), (0.5, 1), (-0.4, 2)])
def test_first_zero_ess_is_the_notebook_formula(phi, seed):
    x = ar1(1500, phi, seed)
    rho = co.autocorr(x)
    k = int(np.where(rho <= 0)[0][0])
    assert abs(rho[k]) > 1e-6 and abs(rho[k - 1]) > 1e-6         # a decisive crossing: the cut cannot flip on rounding
    want = co.notebook_ess(rho)
    assert float(an.first_zero_ess(rho)) == pytest.approx(want, rel=1e-12)
    # from the series: `autocorrelation` on one chain is that definition (FFT against direct sums)
    got = an.ess_per_sample(x)
    assert got.shape == () and float(got) == pytest.approx(want, rel=1e-9)
    two = an.ess_per_sample(np.stack([x, ar1(1500, 0.2, seed + 10)], axis=1))
    assert two.shape == (2,) and float(two[0]) == pytest.approx(want, rel=1e-9)
    assert float(an.ess_per_sample(x, estimator="geyer")) == pytest.approx(float(an.effective_sample_size(x[None, :, None])[0]) / 1500)


def test_first_zero_ess_refuses_a_sequence_that_never_crosses():
    rho = np.stack([np.linspace(1.0, 0.1, 50), np.linspace(1.0, -1.0, 50)], axis=1)
    with pytest.raises(ValueError, match=r"md TIC 0 never reaches zero within 50 lags"):
        an.first_zero_ess(rho, names=["md TIC 0", "md TIC 1"])
    with pytest.raises(ValueError, match=r"observable 0 never"):
        an.first_zero_ess(rho[:, 0])
    with pytest.raises(IndexError):
        co.notebook_ess(rho[:, 0])
    assert float(an.first_zero_ess(rho[:, 1])) == pytest.approx(co.notebook_ess(rho[:, 1]), rel=1e-12)
    with pytest.raises(ValueError, match="estimator"):
        an.ess_per_sample(np.arange(10.0), estimator="arviz")


# ---- loaders -----------------------------------------------------------------------------------------------------------------------

def test_loaders(tmp_path):
    rng = np.random.default_rng(3)
    segments = [rng.normal(size=(4 + i, 5, 3)).astype(np.float32) for i in range(3)]
    for i, seg in enumerate(segments):
        np.savez(st.segment_path(str(tmp_path), "SAEL", i), positions=seg, time=1.5 + i)     # sample_trajectory's call
    np.savez(st.segment_path(str(tmp_path), "RYDT", 0), positions=segments[0], time=9.0)      # another protein's: not read
    pos, sec = an.load_model_chain(str(tmp_path), "SAEL")
    assert np.array_equal(pos, np.concatenate(segments)) and sec.tolist() == [1.5, 2.5, 3.5]
    pos, sec = an.load_model_chain(str(tmp_path), "SAEL", drop_last=True)
    assert np.array_equal(pos, np.concatenate(segments[:2])) and sec.tolist() == [1.5, 2.5]
    pos, _ = an.load_model_chain(str(tmp_path), "SAEL", stride=2)
    assert np.array_equal(pos, np.concatenate([s[::2] for s in segments]))
    with pytest.raises(FileNotFoundError, match="not a directory"):
        an.load_model_chain(str(tmp_path / "absent"), "SAEL")
    with pytest.raises(FileNotFoundError, match="no segments"):
        an.load_model_chain(str(tmp_path), "ABCD")
    with pytest.raises(FileNotFoundError, match="after dropping the last"):
        an.load_model_chain(str(tmp_path), "RYDT", drop_last=True)
    path = tmp_path / "SAEL_exploration.npz"
    np.savez(path, positions=segments[1], time=12.25)
    pos, seconds = an.load_exploration(str(path))
    assert np.array_equal(pos, segments[1]) and seconds == 12.25


def test_acceptance_from_thinned():
    x = np.zeros((50, 4, 3), dtype=np.float32)
    x[:, 0, 0] = np.repeat(np.arange(10), 5)                      # 50 frames, 9 moves between them
    assert an.acceptance_from_thinned(x) == pytest.approx(9 / 50 / 10)
    assert an.acceptance_from_thinned(x, thin=1) == pytest.approx(9 / 50)
    assert "not the chain's own counter" in " ".join(an.acceptance_from_thinned.__doc__.split())


# ---- the report driver ---------------------------------------------------------------------------------------------------------------

REPORT = dict(lag=10, dim=2, md_seconds_per_frame=2.0, route="torch")


def test_report_full_cloud_and_time_scaling():
    md, model = co.four_state_md(), co.four_state_model()
    r = an.speedup_report(md, model, model_seconds_per_frame=0.5, **REPORT)
    assert r.all_states_found and r.coverage < 0.3 and r.threshold == 0.3 and r.covered_fraction == 1.0
    assert r.speedup_tic0 > 0 and r.speedup_tic1 > 0 and r.acceptance is None and r.n_groups == 1
    assert r.ess_md.shape == (2,) and r.ess_model.shape == (2,) and r.eigenvalues.shape == (2,) and r.timescales.shape == (2,)
    assert r.speedup_tic0 == pytest.approx((r.ess_model[0] / 0.5) / (r.ess_md[0] / 2.0), rel=1e-12)
    # the fast chain decorrelates sooner than the slow one, and the first eigenvalue is that of the slow chain (0.95 per frame)
    assert r.ess_model[0] > r.ess_md[0] and r.eigenvalues[0] == pytest.approx(0.95 ** 10, abs=0.08)
    half = an.speedup_report(md, model, model_seconds_per_frame=0.25, **REPORT)
    assert half.speedup_tic0 == pytest.approx(2 * r.speedup_tic0, rel=1e-12) and half.speedup_tic1 == pytest.approx(2 * r.speedup_tic1, rel=1e-12)
    assert half.coverage == r.coverage and half.coverage_arg == r.coverage_arg
    # the notebook's thinning is a choice, not the default
    thin = an.speedup_report(md, model, model_seconds_per_frame=0.5, md_stride=10, cloud_stride=10, **REPORT)
    assert thin.coverage != r.coverage and thin.all_states_found
    doc = " ".join(an.speedup_report.__doc__.split())
    assert "md_stride=10, cloud_stride=10 reproduces that" in doc


def test_report_missing_state_gives_zero_speedups():
    md, model = co.four_state_md(), co.four_state_model(allowed=(0, 1, 2))
    r = an.speedup_report(md, model, model_seconds_per_frame=0.5, **REPORT)
    assert not r.all_states_found and r.coverage > 0.3
    assert r.speedup_tic0 == 0.0 and r.speedup_tic1 == 0.0
    # the MD frame farthest from every model sample is one of the missing state, and about a sixth of the MD points is uncovered
    tail = np.linalg.norm(md[r.coverage_arg] - co.CENTRES[3])
    assert tail < 6 * co.SIGMA
    assert 0.6 < r.covered_fraction < 0.95


def test_report_grouped_form_picks_the_planted_explorer():
    md = co.four_state_md()
    for P, best in ((3, 1), (5, 4)):
        r = an.speedup_report(md, co.explorers(P, best), model_seconds_per_frame=0.5, n_groups=P, **REPORT)
        assert r.n_groups == P and r.best_group == best and r.threshold == 0.1
        assert r.group_coverage.shape == (P,) and r.coverage == r.group_coverage[best] == r.group_coverage.min()
        assert (np.delete(r.group_coverage, best) > 0.3).all() and r.coverage < 0.3
        assert r.speedup_tic1 == 0.0 and np.isnan(r.ess_model[1])
        assert r.all_states_found == (r.coverage < 0.1)
        loose = an.speedup_report(md, co.explorers(P, best), model_seconds_per_frame=0.5, n_groups=P, threshold=0.3, **REPORT)
        assert loose.all_states_found and loose.speedup_tic0 == pytest.approx((loose.ess_model[0] / 0.5) / (loose.ess_md[0] / 2.0))
    with pytest.raises(ValueError, match="not a multiple"):
        an.speedup_report(md, co.explorers(3, 1)[:-1], model_seconds_per_frame=0.5, n_groups=3, **REPORT)
    with pytest.raises(ValueError, match="route='torch' takes features"):
        an.speedup_report(np.zeros((20, 4, 3)), np.zeros((20, 4, 3)), topology=([], [], []), model_seconds_per_frame=1.0, **REPORT)


# ---- binding and command line --------------------------------------------------------------------------------------------------------

def test_entry_point_is_declared_and_bound():
    from timewarp_amd import _lib

    header = open(os.path.join(ROOT, "include", "timewarp_hip.h")).read()
    assert re.search(r"#define TW_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8
    for name, n_args in (("tw_cloud_coverage_workspace_bytes", 4), ("tw_cloud_coverage", 12)):
        assert re.search(r"\b%s\(" % name, header), name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    assert "k ASCENDING" in header and "#define TW_COVERAGE_MAX_DIM 8" in header
    assert [f.name for f in dataclasses.fields(an.SpeedupReport)][:5] == ["coverage", "coverage_arg", "covered_fraction", "threshold",
                                                                           "all_states_found"]


def test_cli_arguments():
    base = ["--md", "SAEL-traj-arrays.npz", "--pdb", "SAEL-traj-state0.pdb", "--md-seconds-per-step", "1e-4", "--md-steps-per-frame", "10000"]
    a = speedup.parse_args(base + ["--model-dir", "chains", "--protein", "SAEL"])
    assert (a.lag, a.dim, a.threshold, a.md_stride, a.cloud_stride, a.no_koopman, a.explorers) == (100, 40, None, 1, 1, False, None)
    a = speedup.parse_args(base + ["--exploration", "SAEL_exploration.npz", "--explorers", "100", "--threshold", "0.2", "--md-stride", "10",
                                   "--cloud-stride", "10", "--no-koopman", "--lag", "50", "--dim", "4", "--out", "x.npz"])
    assert (a.explorers, a.threshold, a.md_stride, a.cloud_stride, a.no_koopman, a.lag, a.dim, a.out) == (100, 0.2, 10, 10, True, 50, 4, "x.npz")
    refused = [base + ["--model-dir", "chains", "--protein", "SAEL", "--exploration", "e.npz", "--explorers", "3"],   # both sources
               base,                                                                                               # neither
               base + ["--model-dir", "chains"],                                                                   # no --protein
               base + ["--exploration", "e.npz"],                                                                  # no --explorers
               base[2:] + ["--model-dir", "chains", "--protein", "SAEL"],                                          # no --md
               base[:4] + ["--model-dir", "chains", "--protein", "SAEL"]]                                          # no MD wall time
    for argv in refused:
        with pytest.raises(SystemExit):
            speedup.parse_args(argv)
    assert speedup.output_path("/d/SAEL-traj-arrays.npz") == "/d/SAEL-speedup.npz"
