"""Float64 numpy restatements of the Koopman reweighting and of what goes with it in timewarp_amd/analysis.py: weighted lagged
moments with their summation bounds, the affine projection with its bound, the Koopman weights, the symmetrised TICA and the two
chained (`run_tica`).  TEST INFRASTRUCTURE ONLY.  Written from the text of include/timewarp_hip.h and of the docstrings; it reads
nothing from the package."""
import numpy as np

# the 4-state reversible chain of the tests: pi = (1/6, 1/3, 1/3, 1/6), second eigenvalue 0.95
MARKOV_P = np.array([[.90, .10, 0, 0], [.05, .90, .05, 0], [0, .05, .90, .05], [0, 0, .10, .90]])
MARKOV_PI = np.array([1, 2, 2, 1]) / 6.0


def markov_states(seed, n_chains=2000, T=40):
    """int [n_chains, T]: chains of MARKOV_P, all started in state 0."""
    rng = np.random.default_rng(seed)
    cum = np.cumsum(MARKOV_P, axis=1)
    s = np.zeros((n_chains, T), dtype=np.int64)
    for t in range(1, T):
        s[:, t] = np.minimum((rng.random(n_chains)[:, None] >= cum[s[:, t - 1]]).sum(1), 3)
    return s


def one_hot(states, n_columns=3):
    """float32 [..., n_columns]: the indicator of the states 0 .. n_columns - 1 (with 3 of the 4 states the features are not
    collinear with the constant)."""
    return (states[..., None] == np.arange(n_columns)).astype(np.float32)


def weighted_moments(X, lag, w=None):
    """The sums over x = X[c, t], y = X[c, t + lag] with the weight w[c, t] (None: ones), and for each sum the matching sum of
    |w| |a| |b| that its summation bound is made from."""
    X = np.asarray(X)
    assert X.dtype == np.float32
    n_chains, T, F = X.shape
    x = X[:, : T - lag].astype(np.float64).reshape(-1, F)
    y = X[:, lag:].astype(np.float64).reshape(-1, F)
    w = np.ones((n_chains, T)) if w is None else np.asarray(w, dtype=np.float64)
    w = w[:, : T - lag].reshape(-1, 1)
    ax, ay, aw = np.abs(x), np.abs(y), np.abs(w)
    return dict(n_pairs=x.shape[0], sum_w=float(w.sum()), abs_w=float(aw.sum()),
                sum_x=(w * x).sum(0), sum_y=(w * y).sum(0), c_xx=(w * x).T @ x, c_xy=(w * x).T @ y, c_yy=(w * y).T @ y,
                abs_x=(aw * ax).sum(0), abs_y=(aw * ay).sum(0), abs_xx=(aw * ax).T @ ax, abs_xy=(aw * ax).T @ ay,
                abs_yy=(aw * ay).T @ ay)


def project(X, P, m=None, b=None):
    """(out, magnitude): out = b + (X - m) @ P in float64 and |b| + |X - m| @ |P|, what the bound of `tw_project` is made from."""
    d = np.asarray(X).astype(np.float64) - (0.0 if m is None else np.asarray(m, dtype=np.float64))
    P = np.asarray(P, dtype=np.float64)
    b = np.zeros(P.shape[1]) if b is None else np.asarray(b, dtype=np.float64)
    return b + d @ P, np.abs(b) + np.abs(d) @ np.abs(P)


def _whitening(c, eps):
    lam, v = np.linalg.eigh(0.5 * (c + c.T))
    keep = lam > eps * lam.max()
    return v[:, keep] / np.sqrt(lam[keep])


def koopman(m, eps=1e-6):
    """(u, const, mean_0, eigenvalue) from the sums `m` (a dict as `weighted_moments` gives), normalised by m['sum_w']."""
    n = m["sum_w"]
    mean_0, mean_t = m["sum_x"] / n, m["sum_y"] / n
    c00 = m["c_xx"] / n - np.outer(mean_0, mean_0)
    c0t = m["c_xy"] / n - np.outer(mean_0, mean_t)
    R = _whitening(c00, eps)
    r = R.shape[1]
    K = np.zeros((r + 1, r + 1))
    K[:r, :r] = R.T @ c0t @ R
    K[r, :r] = (mean_t - mean_0) @ R
    K[r, r] = 1.0
    ev, vec = np.linalg.eig(K.T)
    i = int(np.argmin(np.abs(ev - 1.0)))
    uh = np.real(vec[:, i] / vec[r, i])
    return R @ uh[:r], float(uh[r]), mean_0, float(np.real(ev[i]))


def frame_weights(X, model):
    u, const, mean_0, _ = model
    return (np.asarray(X).astype(np.float64) - mean_0) @ u + const


def tica(m, dim, eps=1e-6):
    """(eigenvalues descending, projection, mean) of the symmetrised estimator on the sums `m`, normalised by m['sum_w']."""
    n = m["sum_w"]
    mean = (m["sum_x"] + m["sum_y"]) / (2.0 * n)
    mm = np.outer(mean, mean)
    c0 = (m["c_xx"] + m["c_yy"]) / (2.0 * n) - mm
    ct = (m["c_xy"] + m["c_xy"].T) / (2.0 * n) - mm
    W = _whitening(c0, eps)
    k = W.T @ ct @ W
    ev, v = np.linalg.eigh(0.5 * (k + k.T))
    order = np.argsort(-ev)[:dim]
    return ev[order], W @ v[:, order], mean


def run_tica(X, lag, dim, reweight=True):
    """dict(eigenvalues, projection, mean, model, weights, moments): plain moments -> Koopman weights -> weighted moments -> TICA;
    reweight=False: the plain symmetrised estimator."""
    plain = weighted_moments(X, lag)
    if not reweight:
        ev, proj, mean = tica(plain, dim)
        return dict(eigenvalues=ev, projection=proj, mean=mean, model=None, weights=None, moments=plain)
    model = koopman(plain)
    w = frame_weights(X, model)
    m = weighted_moments(X, lag, w)
    ev, proj, mean = tica(m, dim)
    return dict(eigenvalues=ev, projection=proj, mean=mean, model=model, weights=w, moments=m)
