"""`tw_project`, `tw_lagged_moments_weighted` and the drivers built on them (`frame_weights`, weighted `lagged_moments`, `run_tica`,
the command line's --koopman) against the float64 restatement tests/koopman_oracle.py.

Tolerances are derived, not measured.  `tw_project`: per term one rounding of X - m and one of the fma, plus the rounding of the
running sum, so (F + 2) 2^-52 (|b| + sum |X - m| |P|).  Weighted moments: a term is rnd(a w) b, one rounding more than the
unweighted call's exact products, so (n + 2) 2^-52 sum |w| |a| |b| over the n pairs, and the same form for sum w.  End to end the
issue's absolute figures hold: eigenvalues 1e-9, mean and frame weights 1e-12 (the features are 0 / 1 and the weights O(1)).

Shapes: F 1 .. 260 (below, at and above the 64-feature slice of `tw_project` and the 128-feature tile of the moments, scalar and
vector loads), k 1 .. 64 (one column, fewer columns than waves, an uneven split, all 16 columns of every wave), rows 1 / 65 / 257."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import koopman_oracle as ko
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

EPS64 = 2.0 ** -52
KEYS = ("sum_x", "sum_y", "c_xx", "c_xy", "c_yy")


def dev():
    return torch.device("cuda", 0)


def bits(t):
    return t.contiguous().view(torch.int64)


# ---- tw_project ---------------------------------------------------------------------------------------------------------------------

def raw_project(Xd, P, m=None, b=None, n_rows=None, F=None, k=None):
    """(status, out) of one tw_project call on the device tensor Xd; the shape arguments default to the tensors' own."""
    from timewarp_amd import _lib

    lib = _lib.load()
    up = lambda a: None if a is None else torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dev())
    Pd, md, bd = up(P), up(m), up(b)
    n_rows = Xd.shape[0] if n_rows is None else n_rows
    F = Xd.shape[1] if F is None else F
    k = Pd.shape[1] if k is None else k
    out = torch.full((max(n_rows, 1), max(k, 1)), float("nan"), dtype=torch.float64, device=dev())
    status = lib.tw_project(Xd.data_ptr(), None if md is None else md.data_ptr(), Pd.data_ptr(), None if bd is None else bd.data_ptr(),
                            out.data_ptr(), n_rows, F, k, _lib.stream_ptr(dev()))
    torch.cuda.synchronize()
    return status, out


@pytest.mark.parametrize("k", [1, 2, 16, 17, 64])
@pytest.mark.parametrize("F", [1, 63, 64, 65, 130, 260])
def test_project_matches_the_restatement(F, k):
    rng = np.random.default_rng(100 * F + k)
    X = (rng.normal(size=(257, F)) + rng.normal(size=F)).astype(np.float32)
    P, m, b = rng.normal(size=(F, k)), rng.normal(size=F), rng.normal(size=k)
    worst = 0.0
    for n_rows in (1, 65, 257):
        Xd = torch.as_tensor(X[:n_rows]).to(dev())
        for mm, bb in ((None, None), (m, b), (m, None), (None, b)):
            status, out = raw_project(Xd, P, mm, bb)
            ref, mag = ko.project(X[:n_rows], P, mm, bb)
            err, bound = np.abs(out.cpu().numpy() - ref), (F + 2) * EPS64 * mag
            worst = max(worst, float((err / bound).max()))
            assert status == 0 and (err <= bound).all(), (n_rows, mm is None, bb is None, float(err.max()))
    print(f"F {F} k {k}: worst error / bound {worst}")


@pytest.mark.parametrize("F,k", [(65, 1), (130, 17), (260, 64)])
def test_project_is_row_local(F, k):
    rng = np.random.default_rng(F + k)
    X = torch.as_tensor(rng.normal(size=(257, F)).astype(np.float32)).to(dev())
    P, m, b = rng.normal(size=(F, k)), rng.normal(size=F), rng.normal(size=k)
    _, whole = raw_project(X, P, m, b)
    _, head = raw_project(X[:65].contiguous(), P, m, b)
    _, tail = raw_project(X[190:].contiguous(), P, m, b)              # the same rows at other positions in other blocks
    assert torch.equal(bits(whole[:65]), bits(head)) and torch.equal(bits(whole[190:]), bits(tail))


def test_project_refusals_and_the_empty_call():
    from timewarp_amd import _lib

    lib = _lib.load()
    X = torch.zeros(4, 8, device=dev())
    P = np.zeros((8, 64))
    for F, k, word in ((8, 0, b"k"), (8, 65, b"k"), (1025, 1, b"n_features"), (0, 1, b"n_features")):
        status, out = raw_project(X, P, n_rows=4, F=F, k=k)
        assert status == -1 and word in lib.tw_last_error(), (F, k, lib.tw_last_error())
        assert bool(torch.isnan(out).all())
    status, out = raw_project(X, P, n_rows=0, F=8, k=64)
    assert status == 0 and bool(torch.isnan(out).all())               # nothing launched, nothing written


def test_project_driver_shapes_and_numpy():
    from timewarp_amd import analysis as an

    rng = np.random.default_rng(7)
    X = rng.normal(size=(2, 33, 20)).astype(np.float32)
    P, m = rng.normal(size=(20, 3)), rng.normal(size=20)
    got_np = an.project(X, P, m)
    got_dev = an.project(torch.as_tensor(X).to(dev()), torch.as_tensor(P), torch.as_tensor(m).to(dev()))
    assert isinstance(got_np, np.ndarray) and got_np.shape == (2, 33, 3) and got_np.dtype == np.float64 and got_dev.is_cuda
    assert (got_dev.cpu().numpy() == got_np).all()
    ref, mag = ko.project(X, P, m)
    assert (np.abs(got_np - ref) <= 22 * EPS64 * mag).all()
    with pytest.raises(ValueError):
        an.project(X, P[:19], m)


# ---- tw_lagged_moments_weighted -----------------------------------------------------------------------------------------------------

def raw_weighted(Xd, Wd, lag, acc=None):
    """One tw_lagged_moments_weighted call; (acc, count, workspace, sum_w) accumulate when given."""
    from timewarp_amd import analysis as an

    if acc is None:
        acc = an.moments_accumulator(Xd.shape[-1], Xd.device) + (torch.zeros(1, dtype=torch.float64, device=Xd.device),)
    an.accumulate_moments_weighted(Xd, Wd, lag, acc[0], acc[1], acc[3], acc[2])
    return acc


def split_acc(acc, F):
    a = acc.cpu().numpy()
    FF = F * F
    return dict(sum_x=a[:F], sum_y=a[F:2 * F], c_xx=a[2 * F:2 * F + FF].reshape(F, F), c_xy=a[2 * F + FF:2 * F + 2 * FF].reshape(F, F),
                c_yy=a[2 * F + 2 * FF:].reshape(F, F))


def assert_weighted(got, sum_w, ref, what=""):
    n = ref["n_pairs"]
    worst = 0.0
    for key, bound_key in (("sum_x", "abs_x"), ("sum_y", "abs_y"), ("c_xx", "abs_xx"), ("c_xy", "abs_xy"), ("c_yy", "abs_yy")):
        err = np.abs(np.asarray(got[key]) - ref[key])
        bound = (n + 2) * EPS64 * ref[bound_key]
        ok = err <= bound
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        assert ok.all(), (what, key, float(err.max()), np.argwhere(~ok)[:4].tolist())
    err_w, bound_w = abs(sum_w - ref["sum_w"]), (n + 2) * EPS64 * ref["abs_w"]
    print(what, "worst error / bound", worst, "sum w error", err_w, "bound", bound_w)
    assert err_w <= bound_w, (what, "sum_w", err_w, bound_w)


def make_X(n_chains, T, F, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n_chains, T, F)) + rng.normal(size=F)).astype(np.float32)


def make_W(n_chains, T, seed):
    """normal(1, 1) - about one in six negative - with a few exact zeros"""
    rng = np.random.default_rng(seed + 1000)
    w = rng.normal(1.0, 1.0, size=(n_chains, T))
    w.reshape(-1)[:: 11] = 0.0
    return w


@pytest.mark.parametrize("n_chains", [1, 3])
@pytest.mark.parametrize("T,lag", [(200, 1), (200, 7), (200, 199), (2, 1), (8, 7)])
@pytest.mark.parametrize("F", [1, 63, 64, 65, 130])
def test_weighted_moments_match_the_restatement(F, T, lag, n_chains):
    X, W = make_X(n_chains, T, F, F + T + lag), make_W(n_chains, T, F + T + lag)
    acc, count, _, sum_w = raw_weighted(torch.as_tensor(X).to(dev()), torch.as_tensor(W).to(dev()), lag)
    ref = ko.weighted_moments(X, lag, W)
    assert int(count.item()) == ref["n_pairs"] == n_chains * (T - lag)
    assert_weighted(split_acc(acc, F), float(sum_w.item()), ref, f"F {F} T {T} lag {lag} chains {n_chains}")


def test_weighted_moments_vector_path_three_tiles():
    F, T, lag = 260, 96, 5
    X, W = make_X(2, T, F, 11), make_W(2, T, 11)
    assert (W < 0).any() and (W == 0).any()
    acc, count, _, sum_w = raw_weighted(torch.as_tensor(X).to(dev()), torch.as_tensor(W).to(dev()), lag)
    assert_weighted(split_acc(acc, F), float(sum_w.item()), ko.weighted_moments(X, lag, W), "F 260")


@pytest.mark.parametrize("F,T,lag,n_chains", [(260, 96, 5, 2), (63, 200, 7, 3), (64, 8, 7, 1), (130, 200, 199, 3), (1, 2, 1, 1)])
def test_all_ones_reproduce_the_unweighted_call(F, T, lag, n_chains):
    from timewarp_amd import analysis as an

    Xd = torch.as_tensor(make_X(n_chains, T, F, 21)).to(dev())
    plain = an.moments_accumulator(F, dev())
    an.accumulate_moments(Xd, lag, *plain)
    acc, count, _, sum_w = raw_weighted(Xd, torch.ones(n_chains, T, dtype=torch.float64, device=dev()), lag)
    assert torch.equal(bits(acc), bits(plain[0])) and int(count.item()) == int(plain[1].item()) == n_chains * (T - lag)
    assert float(sum_w.item()) == float(n_chains * (T - lag))


def test_weighted_moments_are_reproducible_and_accumulate():
    F, T, lag = 65, 200, 7
    X, W = make_X(3, T, F, 14), make_W(3, T, 14)
    Xd, Wd = torch.as_tensor(X).to(dev()), torch.as_tensor(W).to(dev())
    a, b = raw_weighted(Xd, Wd, lag), raw_weighted(Xd.clone(), Wd.clone(), lag)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[3]), bits(b[3]))
    Y, V = torch.as_tensor(make_X(2, 96, 260, 15)).to(dev()), torch.as_tensor(make_W(2, 96, 15)).to(dev())        # the vector path
    c, d = raw_weighted(Y, V, 5), raw_weighted(Y, V, 5)
    assert torch.equal(bits(c[0]), bits(d[0])) and torch.equal(bits(c[3]), bits(d[3]))
    # two overlapping halves: pairs whose first frame is 0 .. 99, then 100 .. 192
    ref = ko.weighted_moments(X, lag, W)
    acc = raw_weighted(Xd[:, : 100 + lag].contiguous(), Wd[:, : 100 + lag].contiguous(), lag)
    acc = raw_weighted(Xd[:, 100:].contiguous(), Wd[:, 100:].contiguous(), lag, acc)
    assert int(acc[1].item()) == ref["n_pairs"]
    assert_weighted(split_acc(acc[0], F), float(acc[3].item()), ref, "two halves")
    # the last `lag` weights of a chain pair with nothing: they are never read
    Wh = W.copy()
    Wh[:, T - lag:] = 1.0e300
    h = raw_weighted(Xd, torch.as_tensor(Wh).to(dev()), lag)
    assert torch.equal(bits(h[0]), bits(a[0])) and torch.equal(bits(h[3]), bits(a[3]))


def test_weighted_moments_never_pair_across_chains():
    """The marker of the unweighted test - in the last `lag` frames of chain 0 and the first `lag` frames of chain 1 - with every
    weight 2 (exact): were a pair to cross the boundary, x y^T would hold marker x marker.  A second call gives chain 1 the weight
    3: the weights are indexed by (chain, frame), not by the pair's number."""
    F, T, lag, big = 5, 40, 7, 1.0e6
    X = np.ones((2, T, F), dtype=np.float32)
    X[0, T - lag:, 0] = big
    X[1, :lag, 0] = big
    W = np.full((2, T), 2.0)
    acc, count, _, sum_w = raw_weighted(torch.as_tensor(X).to(dev()), torch.as_tensor(W).to(dev()), lag)
    got = split_acc(acc, F)
    assert int(count.item()) == 2 * (T - lag) and float(sum_w.item()) == 4.0 * (T - lag)
    assert got["c_xy"][0, 0] < big * big
    assert got["c_xy"][0, 0] == 2.0 * ((T - lag - lag) * 2 * 1.0 + 2 * lag * big)
    assert_weighted(got, float(sum_w.item()), ko.weighted_moments(X, lag, W), "marker")
    W[1] = 3.0
    acc, _, _, sum_w = raw_weighted(torch.as_tensor(X).to(dev()), torch.as_tensor(W).to(dev()), lag)
    assert float(sum_w.item()) == 5.0 * (T - lag)
    assert split_acc(acc, F)["c_xy"][0, 0] == 2.0 * ((T - 2 * lag) + lag * big) + 3.0 * ((T - 2 * lag) + lag * big)


def test_weighted_moments_refuse_what_is_not_supported():
    from timewarp_amd import _lib

    lib = _lib.load()
    s = _lib.stream_ptr(dev())
    X = torch.zeros(1, 8, 4, device=dev())
    W = torch.ones(1, 8, dtype=torch.float64, device=dev())
    acc = torch.zeros(2 * 4 + 3 * 16, dtype=torch.float64, device=dev())
    sw = torch.zeros(1, dtype=torch.float64, device=dev())
    ws = torch.empty(int(lib.tw_lagged_moments_workspace_len(4)), dtype=torch.float64, device=dev())
    call = lambda T, F, lag, w=W.data_ptr(): lib.tw_lagged_moments_weighted(X.data_ptr(), w, 1, T, F, lag, acc.data_ptr(), None,
                                                                            sw.data_ptr(), ws.data_ptr(), s)
    assert call(8, 4, 8) == -1 and b"lag" in lib.tw_last_error()
    assert call(8, 4, 9) == -1 and call(8, 4, 0) == -1
    assert call(8, 1025, 1) == -1 and b"n_features" in lib.tw_last_error()
    assert call(8, 4, 1, None) == -1 and b"weights" in lib.tw_last_error()
    assert call(8, 4, 7) == 0          # the largest lag that is supported; NULL pair count is allowed
    torch.cuda.synchronize()
    assert float(acc.abs().sum()) == 0.0 and float(sw.item()) == 1.0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

LAG = 5


@functools.lru_cache(maxsize=None)
def markov():
    """(X float32 [2000, 40, 3], the oracle's run_tica on it, reweighted and plain) - computed once, never modified"""
    X = ko.one_hot(ko.markov_states(0))
    X.setflags(write=False)
    return X, ko.run_tica(X, LAG, 3, reweight=True), ko.run_tica(X, LAG, 3, reweight=False)


def moments_dict(m):
    return {k: np.asarray(getattr(m, k).cpu() if isinstance(getattr(m, k), torch.Tensor) else getattr(m, k)) for k in KEYS}


def test_run_tica_on_the_markov_chain():
    from timewarp_amd import analysis as an

    X, ref, ref_plain = markov()
    Xd = torch.as_tensor(np.array(X)).to(dev())
    model = an.run_tica(Xd, lagtime=LAG, dim=3)
    ev, mean = model.eigenvalues.cpu().numpy(), model.mean.cpu().numpy()
    w = an.frame_weights(Xd, model.koopman)
    assert w.shape == (2000, 40) and w.dtype == torch.float64 and model.projection.shape == (3, 3)
    print("eigenvalues", ev, "oracle", ref["eigenvalues"], "mean error", np.abs(mean - ref["mean"]).max(), "weight error",
          np.abs(w.cpu().numpy() - ref["weights"]).max(), "largest |weight|", np.abs(ref["weights"]).max())
    assert np.abs(ev - ref["eigenvalues"]).max() < 1e-9
    assert np.abs(mean - ref["mean"]).max() < 1e-12
    assert np.abs(w.cpu().numpy() - ref["weights"]).max() < 1e-12
    assert np.abs(model.timescales.cpu().numpy() + LAG / np.log(np.abs(ref["eigenvalues"]))).max() < 1e-6
    # what the CPU test asks of the oracle holds for the device result
    assert abs(model.koopman.eigenvalue - 1.0) < 1e-9 and abs(float(w[:, : 40 - LAG].mean()) - 1.0) < 1e-9
    plain = an.run_tica(Xd, lagtime=LAG, dim=3, koopman=False)
    assert plain.koopman is None
    assert np.abs(plain.mean.cpu().numpy() - ko.MARKOV_PI[:3]).max() > 0.15 and np.abs(mean - ko.MARKOV_PI[:3]).max() < 0.05
    assert abs(ev[0] - 0.95 ** LAG) < 0.02 and float(plain.eigenvalues[0]) < 0.74
    assert np.abs(plain.eigenvalues.cpu().numpy() - ref_plain["eigenvalues"]).max() < 1e-9
    # transform goes through tw_project
    tics = model.transform(Xd)
    tref, mag = ko.project(X, model.projection.cpu().numpy(), model.mean.cpu().numpy())
    assert tics.shape == (2000, 40, 3) and (np.abs(tics.cpu().numpy() - tref) <= (3 + 2) * EPS64 * mag).all()
    # koopman=False is lagged_moments + tica_from_moments, bit for bit
    for got, want in zip((plain.eigenvalues, plain.projection, plain.mean), an.tica_from_moments(an.lagged_moments(Xd, LAG), 3)):
        assert torch.equal(bits(got), bits(want))


def test_run_tica_chunks_and_numpy_input():
    from timewarp_amd import analysis as an

    X, ref, _ = markov()
    Xd = torch.as_tensor(np.array(X)).to(dev())
    km = an.koopman_from_moments(an.lagged_moments(Xd, LAG))
    w = an.frame_weights(Xd, km)
    rw = w.cpu().numpy()
    mref = ko.weighted_moments(X, LAG, rw)                              # the device's own weights: the bound is about the sums
    for what, m in (("whole, model", an.lagged_moments(Xd, LAG, chunk_frames=1 << 20, weights=km)),
                    ("chunks of 16, model", an.lagged_moments(Xd, LAG, chunk_frames=16, weights=km)),
                    ("chunks of 64, model", an.lagged_moments(Xd, LAG, chunk_frames=64, weights=km)),
                    ("chunks of 16, tensor", an.lagged_moments(Xd, LAG, chunk_frames=16, weights=w)),
                    ("chunks of 16, array", an.lagged_moments(Xd, LAG, chunk_frames=16, weights=rw)),
                    ("torch route", an.lagged_moments(Xd, LAG, chunk_frames=16, weights=w, route="torch"))):
        assert m.n_pairs == 2000 * 35 and m.sum_w is not None, what
        assert_weighted(moments_dict(m), m.sum_w, mref, what)
    # numpy in, numpy out, the same bits
    a, b = an.run_tica(Xd, lagtime=LAG, dim=3, chunk_frames=16), an.run_tica(np.array(X), lagtime=LAG, dim=3, chunk_frames=16)
    assert isinstance(b.eigenvalues, np.ndarray) and isinstance(b.koopman.u, np.ndarray) and a.eigenvalues.is_cuda
    for key in ("eigenvalues", "projection", "mean", "timescales"):
        assert (getattr(a, key).cpu().numpy() == getattr(b, key)).all(), key
    assert (a.koopman.u.cpu().numpy() == b.koopman.u).all() and a.koopman.const == b.koopman.const
    wa, wb = an.frame_weights(Xd, a.koopman), an.frame_weights(np.array(X), b.koopman)
    assert isinstance(wb, np.ndarray) and (wa.cpu().numpy() == wb).all()
    assert (a.transform(Xd).cpu().numpy() == b.transform(np.array(X))).all()
    with pytest.raises(ValueError):
        an.lagged_moments(Xd, LAG, weights=w[:, :39])


@functools.lru_cache(maxsize=None)
def nnqq():
    z = np.load(os.path.join(GOLDEN, "energy_kat_2olx.npz"))
    return z, (list(z["atom_names"]), list(z["residue_names"]), list(z["residue_ids"]))


def test_run_tica_from_coordinates():
    from timewarp_amd import analysis as an

    z, topo = nnqq()
    frames = np.ascontiguousarray(z["positions"], dtype=np.float32)
    coords = np.ascontiguousarray(frames[np.arange(200) % len(frames)]).reshape(2, 100, 65, 3)
    coords = coords + np.float32(1e-3) * np.random.default_rng(15).normal(size=coords.shape).astype(np.float32)
    cd = torch.as_tensor(coords).to(dev())
    model = an.run_tica(cd, lagtime=7, dim=5, topology=topo, chunk_frames=32)
    feats = an.tica_features(cd, topo)
    assert model.koopman is not None and model.eigenvalues.shape == (5,) and model.projection.shape == (feats.shape[-1], 5)
    assert abs(model.koopman.eigenvalue - 1.0) < 1e-9
    w_coords = an.frame_weights(cd, model.koopman, topology=topo, chunk_frames=32)
    w_feats = an.frame_weights(feats, model.koopman)
    assert w_coords.shape == (2, 100) and torch.equal(bits(w_coords), bits(w_feats))
    assert torch.equal(bits(model.transform(cd, chunk_frames=32)), bits(an.project(feats, model.projection, model.mean)))


def write_pdb(path, z):
    with open(path, "w") as f:
        for i, (a, r, k) in enumerate(zip(z["atom_names"], z["residue_names"], z["residue_ids"])):
            name = f" {a:<3s}" if len(a) < 4 else str(a)
            x, y, zz = z["positions"][0][i] * 10.0
            f.write(f"ATOM  {i + 1:5d} {name} {r:>3s} A{int(k):4d}    {x:8.3f}{y:8.3f}{zz:8.3f}  1.00  0.00\n")
        f.write("END\n")
    return str(path)


def test_cli_with_and_without_koopman(tmp_path):
    from timewarp_amd import analysis as an

    z, _ = nnqq()
    rng = np.random.default_rng(17)
    pos = (z["positions"][np.arange(60) % 40] + 1e-3 * rng.normal(size=(60, 65, 3))).astype(np.float32)
    traj = tmp_path / "nnqq-traj-arrays.npz"
    np.savez(traj, positions=pos, step=np.arange(60))
    pdb = write_pdb(tmp_path / "nnqq-traj-state0.pdb", z)
    common = [str(traj), "--pdb", pdb, "--lag", "5", "--dim", "4", "--max-lag", "20", "--chunk-frames", "16"]
    with_k = dict(np.load(an.main(common + ["--koopman", "--out", str(tmp_path / "k.npz")])))
    without = dict(np.load(an.main(common)))
    today = {f for fam in an.FAMILIES for f in (fam, fam + "_indices", "ess_" + fam)} | {
        "tica_eigenvalues", "tica_projection", "tica_mean", "tics", "lag", "n_pairs"}
    new = {"koopman_u", "koopman_const", "koopman_mean", "frame_weights", "tica_timescales"}
    assert set(without) == today and set(with_k) == today | new
    F = without["tica_mean"].shape[0]
    assert with_k["koopman_u"].shape == (F,) and with_k["koopman_mean"].shape == (F,) and with_k["koopman_const"].shape == ()
    assert with_k["frame_weights"].shape == (60,) and with_k["frame_weights"].dtype == np.float64
    assert with_k["tica_timescales"].shape == with_k["tica_eigenvalues"].shape == (4,) and with_k["tics"].shape == (60, 2)
    assert int(with_k["n_pairs"]) == int(without["n_pairs"]) == 55
    # the unflagged run is today's: lagged_moments + tica_from_moments on the same trajectory
    cd = torch.as_tensor(pos).to(dev())[None]
    ev, proj, mean = an.tica_from_moments(an.lagged_moments(cd, 5, chunk_frames=16, topology=pdb), 4)
    assert (without["tica_eigenvalues"] == ev.cpu().numpy()).all() and (without["tica_projection"] == proj.cpu().numpy()).all()
    assert (without["tica_mean"] == mean.cpu().numpy()).all()
