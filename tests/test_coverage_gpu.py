"""`tw_cloud_coverage` (csrc/tw_analysis.hip) through the C ABI, and the drivers built on it (`coverage_distance`, `speedup_report`),
against the extended-precision restatement tests/coverage_oracle.py, whose docstring derives every bound used here.

Shapes sit on each side of every boundary the kernel has (the constants below restate csrc/tw_analysis.hip once):
  n_ref    1, REF_BLOCK - 1 / REF_BLOCK / REF_BLOCK + 1, two blocks plus one, and REDUCE_CHUNK + 1 (two chunks of the reduction);
  n_cloud  0, 1, n_groups - 1 (an empty group), TILE - 1 / TILE / TILE + 1 per group, and FIRST_SPLIT - 1 / FIRST_SPLIT /
           FIRST_SPLIT + 1 per group: the first size at which the cloud axis is split over workgroups;
  dim 1, 2, 3, 8; n_groups 1, 3, 100 with n_cloud not a multiple of n_groups.  The largest case is 1025 x 4100 points.
Random fp64 inputs are held to the derived bounds; integer-grid inputs, where every operation is exact, bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import coverage_oracle as co
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

REF_BLOCK = 512                # reference points per workgroup (kCovThreads x kCovRefPerLane)
TILE = 256                     # cloud points per LDS tile (kCovTile)
MIN_TILES_PER_SPLIT = 2        # kCovMinTilesPerSplit: two ranges need four tiles
FIRST_SPLIT = (2 * MIN_TILES_PER_SPLIT - 1) * TILE + 1    # 769 cloud points in the largest group
REDUCE_CHUNK = 2048            # reference points per workgroup of the reduction (kCovRedChunk)
POISON = -7.25e300             # no result is negative
REPORTED = {}                  # output -> worst error / bound seen (printed by the last random case)


def dev():
    return torch.device("cuda", 0)


def bits(t):
    return t.contiguous().view(torch.int64)


def raw(ref, cloud, groups, want_min=True, guard=64, ws_bytes=None, **override):
    """One tw_cloud_coverage call on poisoned, over-allocated buffers.  Returns (status, min_d2 [G, M] or None, worst [G], arg [G],
    clean) - `clean`: nothing outside the stated extents of the outputs and of the workspace was written."""
    from timewarp_amd import _lib

    lib = _lib.load()
    ref = torch.as_tensor(np.ascontiguousarray(ref, dtype=np.float64)).to(dev())
    cloud = torch.as_tensor(np.ascontiguousarray(cloud, dtype=np.float64)).to(dev())
    M, dim = ref.shape
    N = cloud.shape[0]
    G = groups
    a = dict(n_ref=M, n_cloud=N, dim=dim, n_groups=G)
    a.update(override)                                                   # what the call is told, where it differs from the buffers
    need = int(lib.tw_cloud_coverage_workspace_bytes(M, N, dim, G))
    have = max(need, 8) if ws_bytes is None else ws_bytes
    out_min = torch.full((G * M + 2 * guard,), POISON, dtype=torch.float64, device=dev())
    worst = torch.full((G + 2 * guard,), POISON, dtype=torch.float64, device=dev())
    arg = torch.full((G + 2 * guard,), -77, dtype=torch.int64, device=dev())
    ws = torch.full((max(need, 8) // 8 + 2 * guard,), POISON, dtype=torch.float64, device=dev())
    status = lib.tw_cloud_coverage(ref.data_ptr(), cloud.data_ptr() if N else None, a["n_ref"], a["n_cloud"], a["dim"], a["n_groups"],
                                   out_min[guard:].data_ptr() if want_min else None, worst[guard:].data_ptr(), arg[guard:].data_ptr(),
                                   ws[guard:].data_ptr(), have, _lib.stream_ptr(dev()))
    torch.cuda.synchronize()
    untouched = lambda t, n, p: bool((t[:guard] == p).all()) and bool((t[guard + n:] == p).all())
    clean = untouched(out_min, G * M, POISON) and untouched(worst, G, POISON) and untouched(arg, G, -77) and \
        untouched(ws, max(need, 8) // 8, POISON)
    if not want_min:
        clean = clean and bool((out_min == POISON).all())
    return (status, out_min[guard:guard + G * M].reshape(G, M).cpu() if want_min else None, worst[guard:guard + G].cpu(),
            arg[guard:guard + G].cpu(), clean)


def splits(n_ref, n_cloud, dim, n_groups):
    """The number of ranges the cloud axis is cut into, read off the workspace size (header: splits x n_groups x n_ref partial minima
    and two words per group and chunk of the reduction)."""
    from timewarp_amd import _lib

    words = int(_lib.load().tw_cloud_coverage_workspace_bytes(n_ref, n_cloud, dim, n_groups)) // 8
    chunks = -(-n_ref // REDUCE_CHUNK)
    s, rest = divmod(words - 2 * n_groups * chunks, n_groups * n_ref)
    assert rest == 0
    return s


# (n_ref, n_cloud, dim, n_groups)
N_REF_CASES = [(m, 300, 2, 1) for m in (1, REF_BLOCK - 1, REF_BLOCK, REF_BLOCK + 1, 2 * REF_BLOCK + 1)] + [(REDUCE_CHUNK + 1, 10, 2, 1)]
N_CLOUD_CASES = [(37, n, 2, 1) for n in (0, 1, TILE - 1, TILE, TILE + 1, FIRST_SPLIT - 1, FIRST_SPLIT, FIRST_SPLIT + 1)] + \
                [(37, n, 2, 3) for n in (2, 3 * TILE - 1, 3 * TILE, 3 * TILE + 1, 3 * (FIRST_SPLIT - 1), 3 * (FIRST_SPLIT - 1) + 1,
                                         3 * (FIRST_SPLIT - 1) + 2)] + \
                [(5, n, 2, 100) for n in (99, 100 * TILE - 1, 100 * TILE + 1)]
DIM_CASES = [(REF_BLOCK + 1, 1000, d, 3) for d in (1, 2, 3, 8)]
LARGEST = [(2 * REF_BLOCK + 1, 4100, 2, 1), (2 * REF_BLOCK + 1, 4100, 8, 3)]
CASES = N_REF_CASES + N_CLOUD_CASES + DIM_CASES + LARGEST


def test_the_cloud_axis_splits_where_the_constants_say():
    for G in (1, 3):
        assert splits(37, G * (FIRST_SPLIT - 1), 2, G) == 1
        assert splits(37, G * (FIRST_SPLIT - 1) + 1, 2, G) == 2          # one group now has FIRST_SPLIT points
    assert splits(2 * REF_BLOCK + 1, 4100, 2, 1) > 2 and splits(5, 100 * TILE + 1, 2, 100) == 1
    assert splits(37, 0, 2, 1) == 1


@pytest.mark.parametrize("n_ref,n_cloud,dim,n_groups", CASES)
def test_random_inputs_meet_the_derived_bounds(n_ref, n_cloud, dim, n_groups):
    ref, cloud = co.random_case(n_ref, n_cloud, dim)
    exact_m, exact_w, exact_a = co.random_truth(n_ref, n_cloud, dim, n_groups)
    status, m, w, a, clean = raw(ref, cloud, n_groups)
    assert status == 0 and clean
    e_m = co.check_min_d2(m.numpy(), exact_m, dim)
    e_w = co.check_worst(w.numpy(), exact_w, dim)
    print(f"error / bound: out_min_d2 {e_m:.3f}, out_worst {e_w:.3f}")
    REPORTED["out_min_d2"], REPORTED["out_worst"] = max(REPORTED.get("out_min_d2", 0.0), e_m), max(REPORTED.get("out_worst", 0.0), e_w)
    co.check_arg(a.numpy(), exact_m, exact_a, dim)
    if n_cloud < n_groups:                                               # the empty groups: +inf, +inf, 0
        assert torch.isinf(m[n_cloud:]).all() and torch.isinf(w[n_cloud:]).all() and (a[n_cloud:] == 0).all()
    if (n_ref, n_cloud, dim, n_groups) == CASES[-1]:
        print("worst error / bound over the random cases:", REPORTED)


GRID_CASES = [(2 * REF_BLOCK + 1, 4 * TILE + 1, 2, 1), (REF_BLOCK + 1, 3 * FIRST_SPLIT + 1, 3, 3), (REDUCE_CHUNK + 1, 50, 2, 1),
              (REF_BLOCK, 1001, 8, 3), (7, 99, 1, 100), (1, 1, 2, 1)]


@pytest.mark.parametrize("n_ref,n_cloud,dim,n_groups", GRID_CASES)
def test_integer_grid_inputs_bit_for_bit(n_ref, n_cloud, dim, n_groups):
    ref, cloud, far = co.grid_case(n_ref, n_cloud, dim, n_groups)
    exact_m, exact_w, exact_a = co.grid_truth(n_ref, n_cloud, dim, n_groups)
    status, m, w, a, clean = raw(ref, cloud, n_groups)
    assert status == 0 and clean
    assert np.array_equal(m.numpy().view(np.int64), exact_m.view(np.int64))
    assert np.array_equal(w.numpy().view(np.int64), exact_w.view(np.int64))
    assert a.tolist() == exact_a.tolist()
    filled = min(n_cloud, n_groups)
    assert (a[:filled] == far[0]).all() and (m[:filled, far[0]] == m[:filled, far[1]]).all()     # the planted tie: the smaller index
    if n_ref > 1 and far[0] != 1:
        assert float(m[0, 1]) == 0.0                                     # reference row 1 is cloud row 0


def test_output_hygiene():
    n_ref, n_cloud, dim, G = 2 * REF_BLOCK + 1, 3 * FIRST_SPLIT + 2, 3, 3
    ref, cloud = co.random_case(n_ref, n_cloud, dim)
    status, m, w, a, clean = raw(ref, cloud, G)
    assert status == 0 and clean
    # out_min_d2 = NULL: the same worst and arg, and nothing stored
    status, none, w2, a2, clean = raw(ref, cloud, G, want_min=False)
    assert status == 0 and clean and none is None and torch.equal(bits(w2), bits(w)) and torch.equal(a2, a)
    # the same call twice: the same bits
    status, m3, w3, a3, clean = raw(ref, cloud, G)
    assert status == 0 and clean and torch.equal(bits(m3), bits(m)) and torch.equal(bits(w3), bits(w)) and torch.equal(a3, a)
    # a reference point's minimum does not depend on the blocks of reference points after it (the plan, and with it the split of the
    # cloud axis, does change: min is exact)
    for keep in (REF_BLOCK, REF_BLOCK + 1, 1):
        status, mk, _, _, clean = raw(ref[:keep], cloud, G)
        assert status == 0 and clean and torch.equal(bits(mk), bits(m[:, :keep]))
    # nor on the other groups: group g alone is the single-group call on its rows
    for g in range(G):
        status, mg, wg, ag, clean = raw(ref, cloud[g::G], 1)
        assert status == 0 and clean and torch.equal(bits(mg[0]), bits(m[g])) and torch.equal(bits(wg), bits(w[g:g + 1])) and ag[0] == a[g]


def test_refusals_name_the_argument_and_write_nothing():
    from timewarp_amd import _lib

    lib = _lib.load()
    ref, cloud = co.random_case(37, 300, 2)
    untouched = lambda m, w, a: bool((m == POISON).all()) and bool((w == POISON).all()) and bool((a == -77).all())
    for override, name in ((dict(dim=0), "dim"), (dict(dim=9), "dim"), (dict(n_ref=0), "n_ref"), (dict(n_cloud=-1), "n_cloud"),
                           (dict(n_groups=0), "n_groups")):
        status, m, w, a, clean = raw(ref, cloud, 1, **override)
        assert status != 0 and clean and untouched(m, w, a), override
        message = lib.tw_last_error().decode()
        assert "tw_cloud_coverage" in message and name + ":" in message, message
        args = dict(n_ref=37, n_cloud=300, dim=2, n_groups=1)
        args.update(override)
        assert lib.tw_cloud_coverage_workspace_bytes(args["n_ref"], args["n_cloud"], args["dim"], args["n_groups"]) == -1
    need = int(lib.tw_cloud_coverage_workspace_bytes(37, 300, 2, 1))
    assert need > 0
    status, m, w, a, clean = raw(ref, cloud, 1, ws_bytes=need - 8)
    assert status != 0 and clean and untouched(m, w, a)
    assert "workspace too small" in lib.tw_last_error().decode()
    status, m, w, a, clean = raw(ref, cloud, 1, ws_bytes=need)           # exactly enough is enough
    assert status == 0 and clean


def test_coverage_distance_against_the_torch_route():
    from timewarp_amd import analysis as an

    A, B = co.random_case(REF_BLOCK + 1, 1000, 3)
    for normalise in (True, False):
        for G in (1, 3):
            kw = dict(dims=3, n_groups=G, normalise=normalise, return_min=True)
            w, a, m = an.coverage_distance(torch.as_tensor(A).to(dev()), torch.as_tensor(B).to(dev()), route="kernel", **kw)
            assert w.is_cuda and a.is_cuda and m.is_cuda and w.dtype == torch.float64 and a.dtype == torch.int64 and m.shape == (G, len(A))
            wt, at, mt = an.coverage_distance(torch.as_tensor(A).to(dev()), torch.as_tensor(B).to(dev()), route="torch", chunk=300, **kw)
            # both routes round a d2 within gamma and a square root: twice the bound of out_worst apart at the most
            bound = 2.0 * co.worst_bound(3)
            assert bool(((w - wt).abs() <= bound * wt).all()) and bool(((m - mt).abs() <= bound * mt).all())
            scale = np.abs(A).max(0) if normalise else 1.0
            exact_m, exact_w, exact_a = co.coverage(A / scale, B / scale, G)
            co.check_worst(w.cpu().numpy(), exact_w, 3)
            co.check_arg(a.cpu().numpy(), exact_m, exact_a, 3), co.check_arg(at.cpu().numpy(), exact_m, exact_a, 3)
            # numpy in, numpy out, the same bits; two results without return_min
            wn, an_ = an.coverage_distance(A, B, dims=3, n_groups=G, normalise=normalise)
            assert isinstance(wn, np.ndarray) and np.array_equal(wn, w.cpu().numpy()) and np.array_equal(an_, a.cpu().numpy())
    with pytest.raises(ValueError, match="non-finite"):
        an.coverage_distance(np.array([[0.0, np.nan]]), B[:, :2])
    with pytest.raises(ValueError, match="zero range"):
        an.coverage_distance(np.zeros((4, 2)), B[:, :2])


# ---- speedup_report on the device -----------------------------------------------------------------------------------------------------

# tests/test_analysis_cpu.py:168 holds `autocorrelation` to its direct-sum restatement at 1e-10; the ESS, a function of that
# autocorrelation alone, is held at the same figure, relative
RHO_TOL = 1e-10
MD_FRAMES = 4000               # of the four-state chain: the restatement walks every MD point against every model point


def device_tics(md, model, topology, lag, dim):
    """The device's own TICs (numpy fp64) of both inputs: the fit and the projections `speedup_report` makes, made again."""
    from timewarp_amd import analysis as an

    tica = an.run_tica(md[None], lagtime=lag, dim=dim, topology=topology, koopman=True)
    return np.asarray(tica.transform(md)), np.asarray(tica.transform(model))


def oracle_ess(series):
    rho = co.autocorr(series, max_lag=1500)
    k = int(np.where(rho <= 0)[0][0])
    assert abs(rho[k]) > 1e-6 and abs(rho[k - 1]) > 1e-6, (k, rho[k - 1], rho[k])      # a decisive crossing
    return co.notebook_ess(rho)


def check_report(r, tics_md, tics_model, threshold, ess_columns=(0, 1)):
    """A single-group report against the restatement fed the device's own TICs."""
    ranges = np.abs(tics_md[:, :2]).max(0)
    exact_m, exact_w, exact_a = co.coverage(tics_md[:, :2] / ranges, tics_model[:, :2] / ranges, 1)
    co.check_worst(np.array([r.coverage]), exact_w, 2)
    co.check_arg(np.array([r.coverage_arg]), exact_m, exact_a, 2)
    d = np.sqrt(exact_m[0])
    b = co.worst_bound(2)
    assert (d < threshold * (1 - b)).mean() <= r.covered_fraction <= (d < threshold * (1 + b)).mean()
    assert r.all_states_found == (r.coverage < threshold) and r.threshold == threshold
    for k in ess_columns:
        assert r.ess_md[k] == pytest.approx(oracle_ess(tics_md[:, k]), rel=RHO_TOL)
        assert r.ess_model[k] == pytest.approx(oracle_ess(tics_model[:, k]), rel=RHO_TOL)


def test_report_on_the_four_state_features():
    from timewarp_amd import analysis as an

    md = co.four_state_md(T=MD_FRAMES)
    kw = dict(lag=10, dim=2, md_seconds_per_frame=2.0, model_seconds_per_frame=0.5)
    for allowed, found in (((0, 1, 2, 3), True), ((0, 1, 2), False)):
        model = co.four_state_model(T=1500, allowed=allowed)
        r = an.speedup_report(md, model, **kw)
        assert r.all_states_found == found
        check_report(r, *device_tics(md, model, None, 10, 2), 0.3)
        if found:
            assert r.speedup_tic0 == pytest.approx((r.ess_model[0] / 0.5) / (r.ess_md[0] / 2.0), rel=1e-12) and r.speedup_tic1 > 0
        else:
            assert r.speedup_tic0 == 0.0 and r.speedup_tic1 == 0.0 and r.coverage > 0.3
    # device tensors in: the same report
    rt = an.speedup_report(torch.as_tensor(md).to(dev()), torch.as_tensor(model).to(dev()), **kw)
    assert rt.coverage == r.coverage and rt.coverage_arg == r.coverage_arg and np.array_equal(rt.ess_md, r.ess_md)


@functools.lru_cache(maxsize=None)
def alanine_frames():
    """(md [4000, 22, 3], model [1500, 22, 3] float32, topology): alanine dipeptide displaced along two fixed directions by the
    four-state chains' 2-D emissions (0.01 nm per unit) - slow hops for the MD, fast ones for the model."""
    from timewarp_amd import forcefield as ffm

    z = np.load(os.path.join(GOLDEN, "ad_topology.npz"))
    rid = {"ACE": 1, "ALA": 2, "NME": 3}
    topo = (list(z["atom_names"]), ffm.AD_RESIDUES, [rid[r] for r in ffm.AD_RESIDUES])
    rng = np.random.default_rng(41)
    directions = rng.normal(size=(2, 22, 3))
    frames = lambda e: (z["coords_nm"][None] + 0.01 * np.einsum("tk,kvd->tvd", e.astype(np.float64), directions)).astype(np.float32)
    return frames(co.four_state_md(T=4000, seed=43)), frames(co.four_state_model(T=1500, seed=47)), topo


def test_report_on_coordinates():
    from timewarp_amd import analysis as an

    md, model, topo = alanine_frames()
    r = an.speedup_report(md, model, topology=topo, lag=10, dim=4, md_seconds_per_frame=1.0, model_seconds_per_frame=1.0)
    check_report(r, *device_tics(md, model, topo, 10, 4), 0.3, ess_columns=(0,))
    assert r.acceptance == pytest.approx(an.acceptance_from_thinned(model)) and r.eigenvalues.shape == (4,)


@pytest.mark.parametrize("P,best", [(3, 1), (100, 42)])
def test_grouped_report_equals_separate_single_group_calls(P, best):
    from timewarp_amd import analysis as an

    md = co.four_state_md(T=MD_FRAMES)
    model = co.explorers(P, best, T=2000 if P == 3 else 300)
    r = an.speedup_report(md, model, lag=10, dim=2, md_seconds_per_frame=2.0, model_seconds_per_frame=0.5, n_groups=P)
    assert r.best_group == best and r.n_groups == P and r.threshold == 0.1 and r.group_coverage.shape == (P,)
    tics_md, tics_model = device_tics(md, model, None, 10, 2)
    for g in range(P):
        w, a = an.coverage_distance(tics_md, tics_model[g::P])
        assert w[0] == r.group_coverage[g], g                             # bit for bit
        if g == best:
            assert a[0] == r.coverage_arg and w[0] == r.coverage
    check_report(r, tics_md, tics_model[best::P], 0.1, ess_columns=())      # coverage, arg and covered_fraction are the best explorer's
    assert r.ess_model[0] == pytest.approx(oracle_ess(tics_model[best::P, 0]), rel=RHO_TOL) and np.isnan(r.ess_model[1])
    assert r.speedup_tic1 == 0.0



def test_command_line_on_both_model_sources(tmp_path):
    """`python -m timewarp_amd.speedup` in process: the sampler's segments, then the same frames read as three explorers."""
    from timewarp_amd import analysis as an
    from timewarp_amd import sample_trajectory as st
    from timewarp_amd import speedup

    md, model, (names, residues, ids) = alanine_frames()
    np.savez(tmp_path / "ad-traj-arrays.npz", positions=md, step=np.arange(len(md)))
    pdb = tmp_path / "ad-traj-state0.pdb"
    with open(pdb, "w") as f:
        for i, (a, r, k) in enumerate(zip(names, residues, ids)):
            x, y, z = md[0, i] * 10.0
            f.write(f"ATOM  {i + 1:5d} {a:<4s} {r:>3s} A{int(k):4d}    {x:8.3f}{y:8.3f}{z:8.3f}  1.00  0.00\n")
        f.write("END\n")
    chains = tmp_path / "chains"
    chains.mkdir()
    for i in range(3):
        np.savez(st.segment_path(str(chains), "ad", i), positions=model[500 * i:500 * (i + 1)], time=2.0 + i)
    base = ["--md", str(tmp_path / "ad-traj-arrays.npz"), "--pdb", str(pdb), "--md-seconds-per-step", "1e-3", "--md-steps-per-frame", "100",
            "--lag", "10", "--dim", "4"]
    out = speedup.main(base + ["--model-dir", str(chains), "--protein", "ad"])
    assert out == str(tmp_path / "ad-speedup.npz")
    z = np.load(out)
    r = an.speedup_report(md, model, topology=str(pdb), lag=10, dim=4, md_seconds_per_frame=0.1, model_seconds_per_frame=9.0 / 1500)
    assert float(z["coverage"]) == r.coverage and int(z["coverage_arg"]) == r.coverage_arg and bool(z["all_states_found"]) == r.all_states_found
    assert float(z["speedup_tic0"]) == r.speedup_tic0 and np.array_equal(z["ess_model"], r.ess_model) and float(z["acceptance"]) == r.acceptance
    np.savez(tmp_path / "ad_exploration.npz", positions=model, time=6.0)
    out = speedup.main(base + ["--exploration", str(tmp_path / "ad_exploration.npz"), "--explorers", "3", "--out", str(tmp_path / "e.npz")])
    z = np.load(out)
    r = an.speedup_report(md, model, topology=str(pdb), lag=10, dim=4, md_seconds_per_frame=0.1, model_seconds_per_frame=6.0 / 500, n_groups=3)
    assert int(z["n_groups"]) == 3 and int(z["best_group"]) == r.best_group and np.array_equal(z["group_coverage"], r.group_coverage)
    assert float(z["threshold"]) == 0.1 and float(z["speedup_tic0"]) == r.speedup_tic0 and "acceptance" not in z.files
