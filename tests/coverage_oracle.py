"""Restatements for the speed-up report of timewarp_amd/analysis.py: the cloud coverage distance `tw_cloud_coverage` computes, the
notebooks' first-zero ESS, and the inputs of their tests.  TEST INFRASTRUCTURE ONLY.  Written from the text of
include/timewarp_hip.h and of the docstrings; it reads nothing from the package.

The coverage restatement is brute force over all pairs, in the header's order (k ascending), in numpy.longdouble.  Where that type
is the x87 extended format (epsilon 2^-63 < 2^-60, `EXTENDED`) its own error, about dim 2^-63 relative, is 2^-10 of the bounds
below and is neglected; where longdouble is only a double, the restatement is as inexact as the kernel, and every bound is
doubled (`SLACK` = 2).

Bounds, from u = 2^-53 (one fp64 rounding, |delta| <= u).  All terms of d2 = sum_k (r_k - c_k)^2 are non-negative, so every rounding
is relative to a partial sum that is at most the result:
    t_k = rnd(r_k - c_k) = (r_k - c_k)(1 + delta)                          one rounding
    term 0: rnd(t_0 t_0) = (r_0 - c_0)^2 (1 + delta)^3                      three
    term k, fused: fma(t_k, t_k, s) = (s + (r_k - c_k)^2 (1 + delta)^2)(1 + delta): the new term carries three, and s one more
    term k, not fused: rnd(s + rnd(t_k t_k)): the same count
so after dim terms the first term has collected 3 + (dim - 1) = dim + 2 factors and every other fewer:
    |d2^ - d2| <= gamma d2,   gamma = gamma(dim) = (dim + 2) u / (1 - (dim + 2) u)        (`d2_bound`; out_min_d2)
min and max are exact and monotone, so max_a min_j d2^ is within gamma of max_a min_j d2.  The square root halves a relative
error (sqrt(1 + gamma) <= 1 + gamma / 2, sqrt(1 - gamma) >= 1 - gamma / 2 - gamma^2) and rounds once:
    |worst^ - worst| <= (gamma / 2 + u + gamma^2) worst                                  (`worst_bound`; out_worst)
out_arg: the kernel's index a^ has the largest COMPUTED minimum, v^(a^) >= v^(a) for all a, hence for the exact minima
v(a^)(1 + gamma) >= v_max (1 - gamma).  If the second largest exact minimum is below v_max (1 - gamma) / (1 + gamma) only the arg-max
itself passes that test and the index is compared exactly; otherwise the kernel's index must hold a value at or above that line
(`check_arg`).  Integer-grid inputs make every operation exact; there everything, ties included, is compared bit for bit.

cdist's own rounding (the CPU test against the notebook's expression): scipy computes sqrt(sum_k (a_k - b_k)^2) in fp64 in some
order, i.e. a d2 within gamma(dim) and a square root: the `worst_bound` again.  The two sides then differ by at most
worst_bound (restatement -> exact is negligible) + worst_bound (cdist), relative.
"""
import functools

import numpy as np

from tests.koopman_oracle import MARKOV_P

U = 2.0 ** -53
LD = np.longdouble
EXTENDED = float(np.finfo(LD).eps) < 2.0 ** -60
SLACK = 1.0 if EXTENDED else 2.0


def d2_bound(dim):
    return SLACK * (dim + 2) * U / (1.0 - (dim + 2) * U)


def worst_bound(dim):
    g = d2_bound(dim) / SLACK
    return SLACK * (g / 2.0 + U + g * g)


# ---- restatements -----------------------------------------------------------------------------------------------------------------

def coverage(ref, cloud, n_groups=1):
    """(min_d2 [G, M] longdouble, worst [G] longdouble, arg [G] int64) of ref [M, dim], cloud [N, dim]: cloud row j belongs to group
    j % n_groups; an empty group gives +inf, +inf, 0; arg is the smallest index that attains the maximum."""
    ref, cloud = np.asarray(ref, dtype=LD), np.asarray(cloud, dtype=LD).reshape(-1, np.shape(ref)[1])
    M, dim = ref.shape
    out = np.full((n_groups, M), np.inf, dtype=LD)
    for g in range(n_groups):
        rows = cloud[g::n_groups]
        if len(rows) == 0:
            continue
        for a in range(0, M, 128):
            d2 = np.zeros((len(ref[a:a + 128]), len(rows)), dtype=LD)
            for k in range(dim):                                  # k ascending, as the header states
                t = ref[a:a + 128, k, None] - rows[None, :, k]
                d2 += t * t
            out[g, a:a + 128] = d2.min(axis=1)
    worst2 = out.max(axis=1)
    arg = np.array([int(np.flatnonzero(out[g] == worst2[g])[0]) for g in range(n_groups)], dtype=np.int64)
    return out, np.sqrt(worst2), arg


def check_min_d2(got, exact, dim, what=""):
    """got [G, M] float64 against the longdouble minima; returns the worst error over the bound."""
    got, exact = np.asarray(got), np.asarray(exact)
    assert got.shape == exact.shape, (what, got.shape, exact.shape)
    inf = np.isinf(exact)
    assert (np.isinf(got) == inf).all() and (got[inf] > 0).all(), what
    err = np.abs(got[~inf].astype(LD) - exact[~inf])
    lim = d2_bound(dim) * exact[~inf]
    assert (err <= lim).all(), (what, float((err / np.where(lim > 0, lim, 1)).max()))
    return float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0


def check_worst(got, exact, dim, what=""):
    got, exact = np.asarray(got), np.asarray(exact)
    inf = np.isinf(exact)
    assert (np.isinf(got) == inf).all(), what
    err = np.abs(got[~inf].astype(LD) - exact[~inf])
    lim = worst_bound(dim) * exact[~inf]
    assert (err <= lim).all(), (what, got, exact)
    return float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0


def check_arg(got, exact_min_d2, exact_arg, dim, what=""):
    """The rule of the module docstring, per group."""
    g_ = d2_bound(dim)
    line = (1.0 - g_) / (1.0 + g_)
    for g, a in enumerate(np.asarray(got).tolist()):
        v = exact_min_d2[g]
        assert 0 <= a < len(v), (what, g, a)
        top = v.max()
        if np.isinf(top):
            assert a == int(exact_arg[g]), (what, g, a)          # inf is exact: the smallest index that holds it
            continue
        rest = np.delete(v, int(exact_arg[g]))
        if len(rest) == 0 or rest.max() < top * line:
            assert a == int(exact_arg[g]), (what, g, a, int(exact_arg[g]))
        else:
            assert v[a] >= top * line, (what, g, a)


def notebook_ess(autocorrelations, spacing=1):
    """The notebooks' `ESS` as a formula (cut_off_at_zero=True): IndexError when the autocorrelation never reaches zero."""
    rho = np.asarray(autocorrelations, dtype=np.float64)
    k = np.where(rho <= 0)[0][0]
    return 1.0 / (-1.0 + 2.0 * spacing * np.abs(rho[:k]).sum())


def autocorr(x, max_lag=None):
    """The definition arviz documents for az.autocorr, by direct sums: the biased autocovariance of the centred series over its
    lag-0 value, for the lags 0 .. max_lag (default: all T)."""
    z = np.asarray(x, dtype=np.float64) - np.mean(x)
    T = len(z)
    gamma = np.array([np.dot(z[: T - k], z[k:]) for k in range(T if max_lag is None else min(max_lag + 1, T))]) / T
    return gamma / gamma[0]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_case(n_ref, n_cloud, dim, seed=0):
    """fp64 clouds with full mantissas, the reference cloud wider than the sample cloud (so the maximum is at the rim)."""
    rng = np.random.default_rng([seed, n_ref, n_cloud, dim])
    ref = rng.normal(size=(n_ref, dim)) * 1.5 + 0.25
    cloud = rng.normal(size=(n_cloud, dim))
    return ref, cloud


@functools.lru_cache(maxsize=None)
def random_truth(n_ref, n_cloud, dim, n_groups, seed=0):
    ref, cloud = random_case(n_ref, n_cloud, dim, seed)
    out = coverage(ref, cloud, n_groups)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def grid_case(n_ref, n_cloud, dim, n_groups, seed=0):
    """Small-integer coordinates (every difference, square and sum is exact in fp64) with planted ties: the two reference rows
    `far` = (first, last) are the same far-away point, so every group's maximum is attained at both and the smallest index must
    win; reference row 1 (when there is one) equals cloud row 0 (minimum 0 in group 0)."""
    rng = np.random.default_rng([seed, n_ref, n_cloud, dim, n_groups])
    ref = rng.integers(-8, 9, size=(n_ref, dim)).astype(np.float64)
    cloud = rng.integers(-8, 9, size=(n_cloud, dim)).astype(np.float64)
    far = (min(3, n_ref - 1), n_ref - 1)
    ref[far[0]] = ref[far[1]] = 40.0
    if n_ref > 1 and n_cloud > 0 and far[0] != 1:
        ref[1] = cloud[0]
    return ref, cloud, far


@functools.lru_cache(maxsize=None)
def grid_truth(n_ref, n_cloud, dim, n_groups, seed=0):
    ref, cloud, _ = grid_case(n_ref, n_cloud, dim, n_groups, seed)
    m, w, a = coverage(ref, cloud, n_groups)
    m64 = m.astype(np.float64)
    assert (m64.astype(LD) == m).all()                        # integers: nothing was rounded
    out = (m64, np.sqrt(m64.max(axis=1)), a)                   # IEEE square root of an exactly known integer
    for x in out:
        x.setflags(write=False)
    return out


# the four well-separated states of the report tests: 2-D Gaussians of width SIGMA around CENTRES, a Markov chain hopping between them
CENTRES = np.array([[-3.0, -1.0], [-1.0, 1.0], [1.0, -1.0], [3.0, 1.0]])
SIGMA = 0.08
FAST_P = np.array([[.5, .5, 0, 0], [.25, .5, .25, 0], [0, .25, .5, .25], [0, 0, .5, .5]])    # the "sampler": the same stationary law


def chain_states(P, T, seed, start=0, allowed=(0, 1, 2, 3)):
    """int [T]: one chain of the transition matrix P restricted to `allowed` (rows renormalised)."""
    allowed = list(allowed)
    Q = P[np.ix_(allowed, allowed)]
    cum = np.cumsum(Q / Q.sum(axis=1, keepdims=True), axis=1)
    rng = np.random.default_rng(seed)
    u = rng.random(T)
    s = np.zeros(T, dtype=np.int64)
    s[0] = allowed.index(start) if start in allowed else 0
    for t in range(1, T):
        s[t] = min(int((u[t] >= cum[s[t - 1]]).sum()), len(allowed) - 1)
    return np.asarray(allowed)[s]


def emit(states, seed):
    """float32 [T, 2]: a Gaussian of width SIGMA around each state's centre."""
    rng = np.random.default_rng(seed)
    return (CENTRES[states] + SIGMA * rng.normal(size=(len(states), 2))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def four_state_md(T=20000, seed=11):
    x = emit(chain_states(MARKOV_P, T, seed), seed + 1)
    return x


@functools.lru_cache(maxsize=None)
def four_state_model(T=6000, seed=21, allowed=(0, 1, 2, 3)):
    x = emit(chain_states(FAST_P, T, seed, allowed=allowed), seed + 1)
    return x


@functools.lru_cache(maxsize=None)
def explorers(P, best, T=3000, seed=31):
    """float32 [T * P, 2]: P interleaved explorers (explorer i in rows i::P); all miss state 3 but explorer `best`."""
    rows = [emit(chain_states(FAST_P, T, seed + 7 * i, allowed=(0, 1, 2, 3) if i == best else (0, 1, 2)), seed + 7 * i + 1)
            for i in range(P)]
    x = np.ascontiguousarray(np.stack(rows, axis=1).reshape(T * P, 2))
    return x
