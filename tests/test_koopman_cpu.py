"""The Koopman reweighting without a GPU: the float64 restatement (tests/koopman_oracle.py) on a Markov chain whose stationary
distribution and eigenvalues are known, the host algebra of timewarp_amd/analysis.py (`koopman_from_moments`, `tica_from_moments`
with weighted moments) against that restatement, and the command line's new flag.

Tolerances: the oracle and the package do the same float64 algebra with different LAPACK drivers, so they agree to 1e-10 relative
to the largest entry.  The statistical bounds of the Markov-chain test (0.15 / 0.05 on the mean, 0.02 / 0.74 on the eigenvalue)
stand well clear of what 2000 chains of 40 frames give: 0.20 against at most 0.021, and 0.724 .. 0.729 against 0.770 .. 0.782."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import koopman_oracle as ko
from timewarp_amd import analysis as an

LAG = 5
TRUE_EIGENVALUE = 0.95 ** LAG


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_recovers_the_stationary_chain(seed):
    X = ko.one_hot(ko.markov_states(seed))
    assert X.shape == (2000, 40, 3) and X.dtype == np.float32
    plain, rew = ko.run_tica(X, LAG, 3, reweight=False), ko.run_tica(X, LAG, 3, reweight=True)
    eigenvalue = rew["model"][3]
    mean_weight = rew["weights"][:, : 40 - LAG].mean()
    off_plain = np.abs(plain["mean"] - ko.MARKOV_PI[:3]).max()
    off_rew = np.abs(rew["mean"] - ko.MARKOV_PI[:3]).max()
    print("eigenvalue of K - 1", eigenvalue - 1.0, "mean weight - 1", mean_weight - 1.0, "mean off pi: plain", off_plain, "reweighted",
          off_rew, "leading eigenvalue: plain", plain["eigenvalues"][0], "reweighted", rew["eigenvalues"][0])
    assert abs(eigenvalue - 1.0) < 1e-9 and abs(mean_weight - 1.0) < 1e-9
    assert off_plain > 0.15 and off_rew < 0.05
    assert abs(rew["eigenvalues"][0] - TRUE_EIGENVALUE) < 0.02 and plain["eigenvalues"][0] < 0.74


def hand_built(weighted, numpy_fields=False, seed=3, F=6):
    """(Moments, the oracle's sums) of a smooth random series; `weighted`: with weights around 1, some negative."""
    rng = np.random.default_rng(seed)
    X = np.cumsum(rng.normal(size=(4, 120, F)), axis=1).astype(np.float32) * np.float32(0.1) + rng.normal(size=F).astype(np.float32)
    w = rng.normal(1.0, 0.6, size=(4, 120)) if weighted else None
    m = ko.weighted_moments(X, 3, w)
    conv = (lambda a: a.copy()) if numpy_fields else torch.as_tensor
    fields = [conv(m[k]) for k in ("sum_x", "sum_y", "c_xx", "c_xy", "c_yy")]
    return an.Moments(m["n_pairs"], 3, *fields, sum_w=m["sum_w"] if weighted else None), m


def close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(what, "relative error", err)
    assert got.shape == ref.shape and err < 1e-10, (what, err)


@pytest.mark.parametrize("numpy_fields", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_host_algebra_matches_the_oracle(weighted, numpy_fields):
    moments, m = hand_built(weighted, numpy_fields)
    assert moments.normaliser == (m["sum_w"] if weighted else m["n_pairs"])
    model = an.koopman_from_moments(moments)
    u, const, mean_0, eigenvalue = ko.koopman(m)
    assert isinstance(model.u, np.ndarray if numpy_fields else torch.Tensor)
    close(model.u, u, "u")
    close(model.mean_0, mean_0, "mean_0")
    assert abs(model.const - const) < 1e-10 and abs(model.eigenvalue - eigenvalue) < 1e-10 and abs(model.eigenvalue - 1.0) < 1e-9
    ev, proj, mean = an.tica_from_moments(moments, 4)
    rev, rproj, rmean = ko.tica(m, 4)
    close(ev, rev, "eigenvalues")
    close(mean, rmean, "mean")
    sign = np.sign((proj.numpy() * rproj).sum(0))                     # an eigenvector's sign is free
    close(proj.numpy() * sign, rproj, "projection")


def test_unweighted_tica_keeps_its_bits():
    moments, _ = hand_built(False)
    old_style = an.Moments(moments.n_pairs, moments.lag, moments.sum_x, moments.sum_y, moments.c_xx, moments.c_xy, moments.c_yy)
    assert old_style.sum_w is None and dataclasses.fields(an.Moments)[-1].name == "sum_w"
    # the estimator as it was before `sum_w` existed
    n = float(moments.n_pairs)
    mean = (moments.sum_x + moments.sum_y) / (2.0 * n)
    mm = torch.outer(mean, mean)
    c0 = (moments.c_xx + moments.c_yy) / (2.0 * n) - mm
    ct = (moments.c_xy + moments.c_xy.T) / (2.0 * n) - mm
    lam, u = torch.linalg.eigh(0.5 * (c0 + c0.T))
    w = u[:, lam > 1e-6 * lam.max()] / torch.sqrt(lam[lam > 1e-6 * lam.max()])
    k = w.T @ ct @ w
    ev, v = torch.linalg.eigh(0.5 * (k + k.T))
    order = torch.argsort(ev, descending=True)[:4]
    before = (ev[order], w @ v[:, order], mean)
    for m in (moments, old_style, dataclasses.replace(moments, sum_w=None)):
        for got, ref in zip(an.tica_from_moments(m, 4), before):
            assert torch.equal(got.view(torch.int64), ref.view(torch.int64))
    # a weight sum equal to the pair count is the same normaliser
    for got, ref in zip(an.tica_from_moments(dataclasses.replace(moments, sum_w=float(moments.n_pairs)), 4), before):
        assert torch.equal(got.view(torch.int64), ref.view(torch.int64))


def test_rank_deficient_features_lose_a_direction():
    X = ko.one_hot(ko.markov_states(0, n_chains=200), n_columns=4)           # the four columns add up to one
    m = ko.weighted_moments(X, LAG)
    moments = an.Moments(m["n_pairs"], LAG, *(torch.as_tensor(m[k]) for k in ("sum_x", "sum_y", "c_xx", "c_xy", "c_yy")))
    model = an.koopman_from_moments(moments)
    assert abs(model.eigenvalue - 1.0) < 1e-9 and bool(torch.isfinite(model.u).all())
    w = ko.frame_weights(X, (model.u.numpy(), model.const, model.mean_0.numpy(), model.eigenvalue))
    assert abs(w[:, : 40 - LAG].mean() - 1.0) < 1e-9
    ev, proj, _ = an.tica_from_moments(moments, 4)
    assert ev.shape == (3,) and proj.shape == (4, 3) and bool(torch.isfinite(proj).all())
    mw = ko.weighted_moments(X, LAG, w)
    weighted = an.Moments(mw["n_pairs"], LAG, *(torch.as_tensor(mw[k]) for k in ("sum_x", "sum_y", "c_xx", "c_xy", "c_yy")),
                          sum_w=mw["sum_w"])
    ev, proj, _ = an.tica_from_moments(weighted, 4)
    assert ev.shape == (3,) and proj.shape == (4, 3)


def test_cli_parses_koopman_and_keeps_its_defaults():
    p = an.build_parser()
    a = p.parse_args(["x-traj-arrays.npz", "--pdb", "s.pdb"])
    assert (a.lag, a.dim, a.max_lag, a.chunk_frames, a.out, a.koopman) == (500, 10, None, 16384, None, False)
    assert sorted(vars(a)) == ["chunk_frames", "dim", "koopman", "lag", "max_lag", "out", "pdb", "trajectory"]
    assert p.parse_args(["x.npz", "--pdb", "s.pdb", "--koopman"]).koopman is True


def test_run_tica_signature():
    import inspect

    sig = inspect.signature(an.run_tica)
    got = {k: v.default for k, v in sig.parameters.items() if v.kind is not inspect.Parameter.VAR_KEYWORD}
    assert got == dict(features_or_coords=inspect.Parameter.empty, lagtime=500, dim=40, topology=None, koopman=True, chunk_frames=16384)
    assert inspect.signature(an.lagged_moments).parameters["weights"].default is None
