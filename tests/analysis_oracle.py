"""Float64 numpy restatements of what timewarp_amd/analysis.py computes on the device (csrc/tw_analysis.hip).  TEST
INFRASTRUCTURE ONLY.  Written from the text of include/timewarp_hip.h, not from the kernels: the dihedral formula, the feature
vector, the lagged moments with the summation bound that goes with them, and the direct O(T L) autocovariance."""
import numpy as np


def dihedrals(coords, quads):
    """[n_rows, n_quads] float64: b1 = x1-x0, b2 = x2-x1, b3 = x3-x2, c1 = b2 x b3, c2 = b1 x b2, atan2((b1.c1) |b2|, c1.c2)."""
    x = np.asarray(coords, dtype=np.float64)
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    p0, p1, p2, p3 = (x[:, q[:, k]] for k in range(4))
    b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
    c1, c2 = np.cross(b2, b3), np.cross(b1, b2)
    y = (b1 * c1).sum(-1) * np.sqrt((b2 * b2).sum(-1))
    return np.arctan2(y, (c1 * c2).sum(-1))


def place_fourth(p0, p1, p2, angle, bond=0.15, bend=np.deg2rad(110.0)):
    """A fourth point whose dihedral about p1-p2 is `angle` in the IUPAC convention: 0 = cis (eclipsing p0), positive = clockwise
    rotation of the far bond when looking from p1 to p2.  Built from the definition, not from the formula above."""
    p0, p1, p2 = (np.asarray(p, dtype=np.float64) for p in (p0, p1, p2))
    axis = (p2 - p1) / np.linalg.norm(p2 - p1)
    u = (p0 - p1) - np.dot(p0 - p1, axis) * axis     # the direction of p0 seen down the axis
    u /= np.linalg.norm(u)
    w = np.cross(axis, u)                            # u turned by +90 degrees clockwise seen from p1 to p2 (right-handed about axis)
    radial = np.cos(angle) * u + np.sin(angle) * w
    return p2 + bond * (np.sin(bend) * radial - np.cos(bend) * axis)


def features(coords, atom_sel, families):
    """[n_rows, F] float64: pair distances of the selected atoms in np.triu_indices(n, k=1) order, then per family (a list of
    [n, 4] quad tables) the sines of its angles and the cosines of its angles."""
    x = np.asarray(coords, dtype=np.float64)
    sel = np.asarray(atom_sel, dtype=np.int64).reshape(-1)
    cols = []
    if len(sel) > 1:
        i, j = np.triu_indices(len(sel), k=1)
        d = x[:, sel[i]] - x[:, sel[j]]
        cols.append(np.sqrt((d * d).sum(-1)))
    for quads in families:
        a = dihedrals(x, quads)
        cols += [np.sin(a), np.cos(a)]
    return np.concatenate(cols, axis=1) if cols else np.zeros((x.shape[0], 0))


def lagged_moments(X, lag):
    """The sums over x = X[c, t], y = X[c, t + lag], 0 <= t < T - lag, in float64 from the float32 values, and for each [F, F] sum
    the matching sum of |x_i| |y_j| - what the summation bound N 2^-52 sum |x_i y_j| is made from."""
    X = np.asarray(X)
    assert X.dtype == np.float32
    n_chains, T, F = X.shape
    x = X[:, : T - lag].astype(np.float64).reshape(-1, F)
    y = X[:, lag:].astype(np.float64).reshape(-1, F)
    ax, ay = np.abs(x), np.abs(y)
    return dict(n_pairs=x.shape[0], sum_x=x.sum(0), sum_y=y.sum(0), c_xx=x.T @ x, c_xy=x.T @ y, c_yy=y.T @ y,
                abs_x=ax.sum(0), abs_y=ay.sum(0), abs_xx=ax.T @ ax, abs_xy=ax.T @ ay, abs_yy=ay.T @ ay)


def autocovariance(series, max_lag):
    """gamma [max_lag + 1, n_obs]: chains centred on the pooled mean, (1 / T) sum_t z_t z_{t+k} per chain by direct sums, averaged
    over chains."""
    s = np.asarray(series, dtype=np.float64)
    n_chains, T, _ = s.shape
    z = s - s.mean(axis=(0, 1), keepdims=True)
    return np.stack([np.mean([(z[c, : T - k] * z[c, k:]).sum(0) / T for c in range(n_chains)], axis=0) for k in range(max_lag + 1)])
