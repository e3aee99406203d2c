"""`evaluate.joint_histograms` on its torch route, `analysis.ramachandran_histograms` and `tica_report` without a GPU, against the
numpy restatement tests/joint_histogram_oracle.py (np.histogramdd on float64 casts): every comparison of counts is integer
EQUALITY.  The kernel route runs in tests/test_joint_histogram_gpu.py against the same oracle."""
import numpy as np
import pytest
import torch

from tests import joint_histogram_oracle as jo
from timewarp_amd import analysis, evaluate as ev, tica_report as tr

LO, HI = -1.25, 3.5


def dyadic(bins):
    """A range whose np.linspace edges are float32 numbers: planted values sit EXACTLY on them."""
    return -0.5, -0.5 + bins / 64.0


def matrix(T, C, bins, seed, lo=LO, hi=HI):
    rng = np.random.default_rng(seed)
    return np.stack([jo.planted(lo, hi, bins, rng, T) for _ in range(C)], axis=1)


def check(X, pairs, bins, lo=LO, hi=HI, **kw):
    bx, by = (bins, bins) if np.isscalar(bins) else bins
    P = len(pairs)
    h = ev.joint_histograms(X, pairs, bins=bins, range=((lo, hi), (lo, hi)), route="torch", **kw)
    ex, ey = jo.linspace_tables(lo, hi, bx, P), jo.linspace_tables(lo, hi, by, P)
    counts, outside = jo.joint_pairs(X, pairs, ex, ey)
    assert h.counts.dtype == np.int64 and h.counts.shape == (P, bx, by) and h.outside.shape == (P, 3)
    assert (h.edges_x == ex).all() and (h.edges_y == ey).all()
    assert (h.counts == counts).all() and (h.outside == outside).all()
    assert (h.counts.sum(axis=(1, 2)) + h.outside.sum(axis=1) == len(X)).all()
    return h


@pytest.mark.parametrize("bins", [100, (7, 5), (1, 1), (5, 64)])
def test_torch_route_equals_histogramdd_with_values_on_edges(bins):
    bx, by = (bins, bins) if np.isscalar(bins) else bins
    X = np.stack([jo.planted(LO, HI, bx, np.random.default_rng(1), 3000), jo.planted(LO, HI, by, np.random.default_rng(2), 3000),
                  jo.planted(LO, HI, bx, np.random.default_rng(3), 3000)], axis=1)
    h = check(X, [[0, 1], [2, 1], [0, 1]], bins)
    assert (h.counts[0] == h.counts[2]).all() and h.outside[:, :2].min() > 0
    # edges that ARE float32 numbers: the planted values sit exactly on them, in x and in y
    lo, hi = dyadic(max(bx, by))
    X = matrix(3000, 2, max(bx, by), seed=4, lo=lo, hi=hi)
    e32 = np.linspace(lo, hi, max(bx, by) + 1).astype(np.float32)
    assert (e32.astype(np.float64) == np.linspace(lo, hi, max(bx, by) + 1)).all() and np.isin(e32, X[:, 0]).all() and np.isin(e32, X[:, 1]).all()
    if bx == by:
        check(X, [[0, 1], [1, 0]], bins, lo=lo, hi=hi)
    assert (np.histogram2d(X[:, 0].astype(np.float64), X[:, 1].astype(np.float64), bins=(bx, by), range=((LO, HI), (LO, HI)))[0]
            == ev.joint_histograms(X, [[0, 1]], bins=bins, range=((LO, HI), (LO, HI)), route="torch").counts[0]).all()


def test_nan_and_infinities_go_to_the_three_outside_counters():
    X = matrix(500, 2, 10, seed=5)
    inside = np.float32(1.0)
    X[:12, 0] = [np.nan, inside, np.nan, np.inf, -np.inf, inside, inside, np.inf, np.nan, np.inf, np.float32(LO - 1), inside]
    X[:12, 1] = [inside, np.nan, np.nan, inside, inside, np.inf, -np.inf, np.inf, np.inf, np.nan, np.float32(HI + 1), np.float32(HI + 1)]
    h = check(X, [[0, 1]], 10)
    base = check(X[12:], [[0, 1]], 10)
    # NaN in either wins; then x outside (whatever y is); then y outside
    assert (h.outside[0] - base.outside[0]).tolist() == [4, 3, 5] and (h.counts == base.counts).all()
    with pytest.raises(ValueError, match=r"joint_histograms: column 0 holds 7 non-finite"):
        ev.joint_histograms(X, [[0, 0]], route="torch")
    X[:12, 0] = inside
    assert ev.joint_histograms(X, [[0, 0]], route="torch").counts.sum() == 500          # column 1 is not named: its NaN do not matter


def test_constant_column_same_column_and_empty_inputs():
    X = matrix(400, 3, 10, seed=6)
    X[:, 2] = np.float32(0.75)
    h = ev.joint_histograms(X, [[2, 0], [1, 1]], bins=(4, 6), route="torch")
    assert (h.edges_x[0] == np.linspace(0.25, 1.25, 5)).all()                          # numpy's widened empty range
    ref = np.histogram2d(X[:, 2].astype(np.float64), X[:, 0].astype(np.float64), bins=(4, 6))
    assert (h.counts[0] == ref[0]).all() and (h.edges_y[0] == ref[2]).all() and h.outside.sum() == 0
    same = ev.joint_histograms(X, [[1, 1]], bins=8, route="torch")
    assert (same.counts[0] == np.diag(np.diag(same.counts[0]))).all() and same.counts.sum() == 400
    assert (np.diag(same.counts[0]) == np.histogram(X[:, 1].astype(np.float64), bins=8)[0]).all()
    empty = ev.joint_histograms(X[:0], [[0, 1]], bins=3, route="torch")
    assert empty.counts.shape == (1, 3, 3) and empty.counts.sum() == 0 and (empty.edges_x[0] == np.linspace(0, 1, 4)).all()
    none = ev.joint_histograms(X, np.zeros((0, 2), dtype=int), bins=3, route="torch")
    assert none.counts.shape == (0, 3, 3) and none.outside.shape == (0, 3)
    assert isinstance(ev.joint_histograms(torch.as_tensor(X), [[0, 1]], route="torch").counts, np.ndarray)


def test_caller_edges_and_refusals_by_name():
    rng = np.random.default_rng(7)
    bx, by, P = 9, 13, 2
    ex = np.sort(rng.uniform(LO, HI, size=(P, bx + 1)), axis=1).astype(np.float32).astype(np.float64)
    ey = (LO + (HI - LO) * np.linspace(0, 1, by + 1) ** 3)[None].repeat(P, axis=0).astype(np.float32).astype(np.float64)
    X = matrix(2000, 2, 10, seed=8)
    inf = np.float32(np.inf)
    e32 = ex[0].astype(np.float32)
    X[:3 * (bx + 1), 0] = np.concatenate([e32, np.nextafter(e32, -inf), np.nextafter(e32, inf)])
    e32 = ey[0].astype(np.float32)
    X[100:100 + 3 * (by + 1), 1] = np.concatenate([e32, np.nextafter(e32, -inf), np.nextafter(e32, inf)])
    pairs = [[0, 1], [1, 1]]
    ex[1] = ey[1][:bx + 1]
    h = ev.joint_histograms(X, pairs, bins=(bx, by), edges=(ex, ey), route="torch")
    counts, outside = jo.joint_pairs(X, pairs, ex, ey)
    assert (h.counts == counts).all() and (h.outside == outside).all() and (h.edges_x == ex).all()
    bad = ex.copy()
    bad[1, 3] = bad[1, 2]
    with pytest.raises(ValueError, match="edges of column 1 are not strictly increasing"):
        ev.joint_histograms(X, pairs, bins=(bx, by), edges=(bad, ey), route="torch")
    bad = ey.copy()
    bad[0, 0] = np.inf
    with pytest.raises(ValueError, match="edges of column 0 hold non-finite"):
        ev.joint_histograms(X, pairs, bins=(bx, by), edges=(ex, bad), route="torch")
    with pytest.raises(ValueError, match=r"edges \(2, 10\): expected"):
        ev.joint_histograms(X, pairs, bins=(bx, by), edges=(ex, ex), route="torch")
    for p, msg in (([[0, 2]], r"pairs: entries must be in 0 \.\. 1, got 0 \.\. 2"), ([[-1, 0]], r"pairs: entries must be in 0 \.\. 1"),
                   ([[0, 1, 1]], r"pairs: expected \[n_pairs, 2\]")):
        with pytest.raises(ValueError, match=msg):
            ev.joint_histograms(X, p, route="torch")
    for bins, msg in ((0, "bins 0"), ((4, 4097), "bins 4097"), ((2048, 1024), "at most 2\\^20")):
        with pytest.raises(ValueError, match=msg):
            ev.joint_histograms(X, pairs, bins=bins, route="torch")
    with pytest.raises(ValueError, match="route 'fused'"):
        ev.joint_histograms(X, pairs, route="fused")
    with pytest.raises(ValueError, match="max must be larger than min"):
        ev.joint_histograms(X, pairs, range=((1.0, 0.0), (0.0, 1.0)), route="torch")
    assert ev.DEFAULT_JOINT_ROUTE in ev.JOINT_ROUTES


def test_chunks_accumulate_density_and_marginals():
    X = matrix(3000, 3, 100, seed=9)
    pairs = [[0, 1], [2, 0], [1, 1]]
    whole = ev.joint_histograms(X, pairs, bins=(30, 20), route="torch")
    parts = ev.joint_histograms(X, pairs, bins=(30, 20), route="torch", chunk_rows=701)
    for f in ("counts", "outside", "edges_x", "edges_y"):
        assert (getattr(whole, f) == getattr(parts, f)).all(), f
    assert whole.outside.sum() == 0                                                    # own ranges: nothing is outside
    dens = whole.density()
    for p, (i, j) in enumerate(pairs):
        ref = np.histogram2d(X[:, i].astype(np.float64), X[:, j].astype(np.float64), bins=(30, 20), density=True)[0]
        assert (dens[p] == ref).all()                                                  # bit-equal: numpy's order of operations
    # with nothing outside the marginals are the 1-D histograms on the same edges
    cols = ev.column_histograms(X[:, [0, 2, 1]], bins=30, route="torch", edges=whole.edges_x)
    assert (whole.marginal_x() == cols.counts).all()
    cols = ev.column_histograms(X[:, [1, 0, 1]], bins=20, route="torch", edges=whole.edges_y)
    assert (whole.marginal_y() == cols.counts).all()
    fe = whole.free_energy()
    h = whole.counts[0].astype(np.float64)
    with np.errstate(divide="ignore"):
        assert np.array_equal(fe[0], -np.log(h / h.max())) and fe[0].min() == 0 and np.isinf(fe[0]).any()


def test_ramachandran_histograms_all_residues_in_one_call():
    rng = np.random.default_rng(10)
    T = 2000
    phi = rng.uniform(-np.pi, np.pi, size=(T, 3)).astype(np.float32)
    psi = rng.uniform(-np.pi, np.pi, size=(T, 2)).astype(np.float32)
    phi[:4, 0] = [np.float32(np.pi), -np.float32(np.pi), 0.0, np.nan]                # float32 pi is inside: it is the last edge
    rp = [(0, 0), (2, 1), (1, 0)]
    h = analysis.ramachandran_histograms(phi, psi, rp, bins=24, route="torch")
    p = float(np.float32(np.pi))
    e = jo.linspace_tables(-p, p, 24, 3)
    for k, (i, j) in enumerate(rp):
        counts, outside = jo.joint_counts(phi[:, i], psi[:, j], e[k], e[k])
        assert (h.counts[k] == counts).all() and (h.outside[k] == outside).all()
    assert h.outside.tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 0]] and (h.edges_x == e).all()
    with pytest.raises(ValueError, match="residue_pairs"):
        analysis.ramachandran_histograms(phi, psi, [(3, 0)], route="torch")
    # away from the edges the old per-residue function counts the same
    old = analysis.ramachandran_histogram(phi[4:, 1], psi[4:, 0], 24).numpy()
    assert (analysis.ramachandran_histograms(phi[4:], psi[4:], [(1, 0)], bins=24, route="torch").counts[0] == old).all()


# ---- the report --------------------------------------------------------------------------------------------------------------------------

def four_state_chain(T, seed, F=5, rate=0.01):
    """features [T, F] float32 of a chain hopping between four wells, and (phi, psi) [T, 2] float32 that follow the state."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(4, F)) * 2
    state = np.zeros(T, dtype=np.int64)
    for t in range(1, T):
        state[t] = rng.integers(4) if rng.random() < rate else state[t - 1]
    feats = (centres[state] + 0.3 * rng.normal(size=(T, F))).astype(np.float32)
    wells = np.array([[-1.2, 2.5], [-1.2, -0.8], [1.0, 0.8], [-2.6, 2.9]])
    ang = wells[state][:, None, :] + 0.25 * rng.normal(size=(T, 2, 2))
    ang = ((ang + np.pi) % (2 * np.pi) - np.pi).astype(np.float32)
    return feats, (ang[:, :, 0].copy(), ang[:, :, 1].copy())


def chain_inputs():
    md, md_t = four_state_chain(4000, 0)
    model, model_t = four_state_chain(1500, 1, rate=0.05)
    expl, expl_t = four_state_chain(900, 2, rate=0.2)
    return md, model, expl, {"md": md_t, "model": model_t, "exploration": expl_t}


def numpy_autocorrelation(x):
    z = x.astype(np.float64) - x.astype(np.float64).mean()
    T = len(z)
    gamma = np.array([np.dot(z[:T - k], z[k:]) / T for k in range(min(T, 1500))])
    return gamma / gamma[0]


@pytest.mark.parametrize("edges", ["md", "own"])
def test_tica_report_fields_are_the_numpy_expressions(edges, tmp_path):
    md, model, expl, tors = chain_inputs()
    bins, lag = 20, 10
    r = tr.tica_report(md, model, exploration=expl, torsions=tors, lag=lag, dim=3, bins=bins, edges=edges, route="torch",
                       seconds_per_frame={"md": 0.5, "model": 0.02}, strides={"md": 7}, chunk_rows=997)
    tica = analysis._run_tica_torch(torch.as_tensor(md)[None], lag, 3, True, 16384)
    assert np.array_equal(r.eigenvalues, tica.eigenvalues.numpy()) and r.lag == lag and list(r.runs) == ["md", "model", "exploration"]
    tics = {k: ((torch.as_tensor(f).double() - tica.mean) @ tica.projection).to(torch.float32).numpy()
            for k, f in (("md", md), ("model", model), ("exploration", expl))}
    f64 = lambda a: a.astype(np.float64)
    md_range = [(f64(tics["md"][:, d]).min(), f64(tics["md"][:, d]).max()) for d in (0, 1)]
    for name, t in tics.items():
        run = r.runs[name]
        own = [(f64(t[:, d]).min(), f64(t[:, d]).max()) for d in (0, 1)]
        rng_ = md_range if edges == "md" else own
        ref = np.histogram2d(f64(t[:, 0]), f64(t[:, 1]), bins=bins, range=rng_)
        assert (run.tic01.counts[0] == ref[0]).all() and (run.tic01.edges_x[0] == ref[1]).all() and (run.tic01.edges_y[0] == ref[2]).all()
        ex, ey = np.linspace(*rng_[0], bins + 1), np.linspace(*rng_[1], bins + 1)
        assert (run.tic01.outside[0] == jo.joint_counts(t[:, 0], t[:, 1], ex, ey)[1]).all()
        assert run.tic01.counts.sum() + run.tic01.outside.sum() == len(t) == run.n_frames
        if edges == "own" or name == "md":
            assert run.tic01.outside.sum() == 0
        for d in (0, 1):                                                          # plot_free_energy2
            hist, e = np.histogram(f64(t[:, d]), bins=bins)
            dens = np.histogram(f64(t[:, d]), bins=bins, density=True)[0]
            assert (run.projections.counts[d] == hist).all() and (run.projections.edges[d] == e).all()
            assert np.array_equal(run.centres[d], 0.5 * (e[1:] + e[:-1]))
            with np.errstate(divide="ignore"):
                fe = -np.log(dens / dens.max())
            assert np.array_equal(np.isinf(run.free_energy[d]), np.isinf(fe))
            assert np.allclose(run.free_energy[d][~np.isinf(fe)], fe[~np.isinf(fe)], rtol=0, atol=1e-12)
        rho = numpy_autocorrelation(t[:, 0])
        k = int(np.flatnonzero(rho <= 0)[0])
        assert len(run.autocorrelation) == k and np.allclose(run.autocorrelation, rho[:k], rtol=0, atol=1e-9)
        ess = 1.0 / (-1.0 + 2.0 * np.abs(rho[:k]).sum())
        assert abs(run.ess_per_sample - ess) < 1e-9 * ess
        stride = 7 if name == "md" else 100
        assert run.series_stride == stride and np.array_equal(run.tic0_series, t[::stride, 0])
        phi, psi = tors[name]
        p = float(np.float32(np.pi))
        e = np.linspace(-p, p, bins + 1)
        for i in range(2):
            counts, outside = jo.joint_counts(phi[:, i], psi[:, i], e, e)
            assert (run.ramachandran.counts[i] == counts).all() and (run.ramachandran.outside[i] == outside).all()
    assert abs(r.runs["md"].ess_per_second - r.runs["md"].ess_per_sample / 0.5) < 1e-15 and r.runs["exploration"].ess_per_second is None
    assert r.residue_pairs.tolist() == [[0, 0], [1, 1]]
    back = ev.load_report(r.save(str(tmp_path / "report.npz")))
    arrays = r.arrays()
    assert set(back) == set(arrays) and "exploration_ess_per_second" not in back and "model_ramachandran_counts" in back
    for k, v in arrays.items():
        assert np.array_equal(back[k], v, equal_nan=np.asarray(v).dtype.kind == "f"), k
    assert back["md_tic01_counts"].shape == (bins, bins) and str(back["edges_mode"]) == edges


def test_tica_report_refusals():
    md, model, expl, tors = chain_inputs()
    with pytest.raises(ValueError, match="edges 'shared'"):
        tr.tica_report(md, model, edges="shared", route="torch")
    with pytest.raises(ValueError, match="route 'fused'"):
        tr.tica_report(md, model, route="fused")
    with pytest.raises(ValueError, match="model: expected features"):
        tr.tica_report(md, model[None], route="torch")
    r = tr.tica_report(md, model, lag=10, dim=2, bins=10, route="torch")
    assert r.runs["md"].ramachandran is None and "md_ramachandran_counts" not in r.arrays() and len(r.residue_pairs) == 0


def test_command_line_in_process(tmp_path):
    from tests.test_evaluate_cpu import cli_files

    mdf, chain, pdb, z, frames, steps = cli_files(tmp_path)
    expl = tmp_path / "nnqq_exploration.npz"
    np.savez(expl, positions=frames[::-1].copy(), time=3.0)
    out = str(tmp_path / "tica.npz")
    got = tr.main(["--md", mdf, "--model-dir", chain, "--protein", "nnqq", "--pdb", pdb, "--exploration", str(expl), "--lag", "2",
                   "--dim", "2", "--bins", "12", "--route", "torch", "--md-seconds-per-frame", "0.25", "--out", out])
    assert got == out
    back = ev.load_report(out)
    md_x = z["positions"][:len(steps)]
    direct = tr.tica_report(md_x, frames, exploration=frames[::-1].copy(), topology=pdb, lag=2, dim=2, bins=12, route="torch",
                            seconds_per_frame={"md": 0.25, "model": 2.0 / 30, "exploration": 0.1}).arrays()
    assert set(back) == set(direct)
    for k, v in direct.items():
        assert np.array_equal(back[k], v, equal_nan=np.asarray(v).dtype.kind == "f"), k
    assert back["md_tic01_counts"].sum() == len(md_x) and back["model_tic01_counts"].sum() + back["model_tic01_outside"].sum() == 30
    assert back["md_ramachandran_counts"].shape == (len(back["residue_pairs"]), 12, 12) and len(back["residue_pairs"]) == 2   # the two inner residues of the tetrapeptide have both angles
    assert back["md_ramachandran_counts"].sum() == 2 * len(md_x) and "exploration_ess_per_second" in back
    with pytest.raises(SystemExit):
        tr.build_parser().parse_args(["--md", mdf])
