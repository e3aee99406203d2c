"""A float64 restatement of the constrained Langevin integrator (csrc/tw_md.hip `langevin_constrained_kernel` behind
`tw_langevin_trajectory_constrained`, and `apply_constraints_kernel` behind `tw_apply_constraints`).  TEST INFRASTRUCTURE ONLY.

Written from the text of include/timewarp_hip.h, vectorised over rows AND clusters: a cluster is (c; h_1 .. h_k), k <= 3, with
inverse masses w = 1 / m and reference vectors r_a = xref_c - xref_{h_a}.

    P(x; xref)  SHAKE sweeps, Gauss-Seidel over a = 1 .. k:  s = x_c - x_{h_a};  delta = d_a^2 - s.s;  where |delta| > tol d_a^2:
                g = delta / (2 (r_a.s) (w_c + w_{h_a}));  x_c += g w_c r_a;  x_{h_a} -= g w_{h_a} r_a.  A cluster stops after its first
                sweep that changed nothing (that sweep is counted) or after max_sweeps.  residual = max_a |d_a^2 - s.s| / d_a^2 at the end.
    Q(v; r)     A_ab = (r_a.r_b) w_c + [a = b] (r_a.r_a) w_{h_a};  b_a = (v_c - v_{h_a}).r_a;  A lambda = b by Gaussian elimination
                without pivoting;  v_c -= lambda_a w_c r_a (a in order);  v_{h_a} += lambda_a w_{h_a} r_a.
    scheme 0    v += dt F/m;  Q(v; r from x);  xref = x;  x += dt/2 v;  v <- a v + sigma N;  x += dt/2 v  (x_u);  P(x; xref);
                v += (x - x_u) / dt on the cluster atoms
    scheme 1    xref = x;  v <- a v + fscale F/m + sigma N;  x += dt v  (x_u);  P(x; xref);  v += (x - x_u) / dt on the cluster atoms

Unused hydrogen slots are handled as rows of the identity in Q (lambda = 0) and skipped in P, which is the k x k computation.  The
noise is `langevin_oracle.md_normal` with the unchanged key; with zero clusters every line is `langevin_oracle.langevin_steps`'s.
`wrong=` switches on one of four deliberately wrong variants, for the tests that show the comparison can tell them apart.
"""
import numpy as np

from tests import langevin_oracle as lo

WRONG = ("no_velocity_projection", "no_inverse_dt", "reference_from_new", "masses_swapped")


class Clusters:
    """atoms [C, 4] (centre, h1, h2, h3; -1 unused), lengths [C, 3], masses [V] -> index and weight arrays for the projections"""

    def __init__(self, atoms, lengths, masses, swap_masses=False):
        atoms = np.asarray(atoms, dtype=np.int64).reshape(-1, 4)
        self.n = atoms.shape[0]
        self.used = atoms[:, 1:] >= 0                                   # [C, 3]
        self.c = atoms[:, 0]                                            # [C]
        self.h = np.where(self.used, atoms[:, 1:], atoms[:, :1])        # [C, 3]; unused -> the centre (never written through)
        m = np.asarray(masses, dtype=np.float32).astype(np.float64).reshape(-1)
        self.wc = 1.0 / m[self.c] if self.n else np.zeros(0)            # [C]
        self.wh = np.where(self.used, 1.0 / m[self.h], 0.0) if self.n else np.zeros((0, 3))
        if swap_masses and self.n:                                       # WRONG on purpose: centre and hydrogen masses exchanged
            wc = self.wc
            self.wc = np.where(self.used[:, 0], 1.0 / m[self.h[:, 0]], wc)
            self.wh = np.where(self.used, wc[:, None], 0.0)
        self.d2 = np.where(self.used, np.asarray(lengths, dtype=np.float64).reshape(-1, 3) ** 2, 0.0)
        self.n_constraints = int(self.used.sum())


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def refvec(cl, xref):
    """[N, C, 3(a), 3]: r_a = xref_c - xref_{h_a}; exactly 0 in unused slots"""
    return xref[:, cl.c][:, :, None, :] - xref[:, cl.h]


def project_positions(cl, x, xref, tol, max_sweeps):
    """-> (x, sweeps [N, C] int, residual [N, C]); x is a new array"""
    x = x.copy()
    n = x.shape[0]
    if cl.n == 0:
        return x, np.zeros((n, 0), dtype=np.int64), np.zeros((n, 0))
    r = refvec(cl, xref)
    xc = x[:, cl.c]                         # [N, C, 3]   local copies, as the lane holds them
    xh = x[:, cl.h]                         # [N, C, 3, 3]
    active = np.ones((n, cl.n), dtype=bool)
    sweeps = np.zeros((n, cl.n), dtype=np.int64)
    for _ in range(int(max_sweeps)):
        if not active.any():
            break
        sweeps += active
        changed = np.zeros((n, cl.n), dtype=bool)
        for a in range(3):
            s = xc - xh[:, :, a]
            delta = cl.d2[None, :, a] - _dot(s, s)
            move = active & cl.used[None, :, a] & (np.abs(delta) > tol * cl.d2[None, :, a])
            with np.errstate(divide="ignore", invalid="ignore"):
                g = delta / (2.0 * _dot(r[:, :, a], s) * (cl.wc[None] + cl.wh[None, :, a]))
            g = np.where(move, g, 0.0)
            xc = np.where(move[..., None], xc + (g * cl.wc[None])[..., None] * r[:, :, a], xc)
            xh[:, :, a] = np.where(move[..., None], xh[:, :, a] - (g * cl.wh[None, :, a])[..., None] * r[:, :, a], xh[:, :, a])
            changed |= move
        active &= changed
    resid = np.zeros((n, cl.n))
    for a in range(3):
        s = xc - xh[:, :, a]
        with np.errstate(divide="ignore", invalid="ignore"):
            ra = np.abs(cl.d2[None, :, a] - _dot(s, s)) / cl.d2[None, :, a]
        resid = np.maximum(resid, np.where(cl.used[None, :, a], ra, 0.0))
    x[:, cl.c] = xc
    for a in range(3):
        u = cl.used[:, a]
        x[:, cl.h[u, a]] = xh[:, u, a]
    return x, sweeps, resid


def project_velocities(cl, v, r):
    """Q(v; r) with r = refvec(...) -> new v"""
    v = v.copy()
    if cl.n == 0:
        return v
    vc, vh = v[:, cl.c], v[:, cl.h]
    A = np.empty(r.shape[:2] + (3, 3))
    b = np.empty(r.shape[:2] + (3,))
    for a in range(3):
        for c in range(3):
            A[..., a, c] = _dot(r[:, :, a], r[:, :, c]) * cl.wc[None]
        A[..., a, a] += _dot(r[:, :, a], r[:, :, a]) * cl.wh[None, :, a]
        A[..., a, a] = np.where(cl.used[None, :, a], A[..., a, a], 1.0)
        b[..., a] = _dot(vc - vh[:, :, a], r[:, :, a])
    m10, m20 = A[..., 1, 0] / A[..., 0, 0], A[..., 2, 0] / A[..., 0, 0]
    A[..., 1, 1] -= m10 * A[..., 0, 1]
    A[..., 1, 2] -= m10 * A[..., 0, 2]
    b[..., 1] -= m10 * b[..., 0]
    A[..., 2, 1] -= m20 * A[..., 0, 1]
    A[..., 2, 2] -= m20 * A[..., 0, 2]
    b[..., 2] -= m20 * b[..., 0]
    m21 = A[..., 2, 1] / A[..., 1, 1]
    A[..., 2, 2] -= m21 * A[..., 1, 2]
    b[..., 2] -= m21 * b[..., 1]
    lam = np.empty_like(b)
    lam[..., 2] = b[..., 2] / A[..., 2, 2]
    lam[..., 1] = (b[..., 1] - A[..., 1, 2] * lam[..., 2]) / A[..., 1, 1]
    lam[..., 0] = (b[..., 0] - A[..., 0, 1] * lam[..., 1] - A[..., 0, 2] * lam[..., 2]) / A[..., 0, 0]
    for a in range(3):
        vc = vc - (lam[..., a] * cl.wc[None])[..., None] * r[:, :, a]
        vh[:, :, a] = vh[:, :, a] + (lam[..., a] * cl.wh[None, :, a])[..., None] * r[:, :, a]
    v[:, cl.c] = vc
    for a in range(3):
        u = cl.used[:, a]
        v[:, cl.h[u, a]] = vh[:, u, a]
    return v


def cluster_atoms(cl):
    """indices of all atoms that sit in a cluster"""
    return np.concatenate([cl.c, cl.h[cl.used]]) if cl.n else np.zeros(0, dtype=np.int64)


def apply_constraints(cl, x, v, tol, max_sweeps):
    """tw_apply_constraints in float64: x <- P(x; x), v <- Q(v; r from the projected x) -> (x, v or None, residual [N])"""
    x = np.asarray(x, dtype=np.float64)
    x2, _, resid = project_positions(cl, x, x, tol, max_sweeps)
    v2 = None if v is None else project_velocities(cl, np.asarray(v, dtype=np.float64), refvec(cl, x2))
    return x2, v2, (resid.max(axis=1) if cl.n else np.zeros(x.shape[0]))


def constrained_steps64(force_fn, masses, x, v, n_steps, dt, friction, kbT, scheme, seed, first_step, atoms, lengths, tol, max_sweeps,
                        conformations=None, wrong=None, on_step=None):
    """`n_steps` constrained steps of a float64 state -> (x, v, e, worst_sweeps [N], worst_residual [N]), all float64: the carry of
    state64.  `on_step(s, x, v, e, f)` is called with the state BEFORE step s and its energy / forces (what a frame at s records).
    `wrong`: None or one of WRONG."""
    assert wrong is None or wrong in WRONG, wrong
    x, v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
    n, V, _ = x.shape
    m = np.asarray(masses, dtype=np.float32).astype(np.float64).reshape(1, V, 1)
    cl = Clusters(atoms, lengths, masses, swap_masses=(wrong == "masses_swapped"))
    members = cluster_atoms(cl)
    conf = (np.arange(n) if conformations is None else np.asarray(conformations)).reshape(n, 1, 1)
    comp = np.arange(3 * V).reshape(1, V, 3)
    if friction > 0.0:
        a = np.exp(-friction * dt)
        fscale = (1.0 - a) / friction
        sigma = np.sqrt(1.0 - a * a) * np.sqrt(kbT / m)
    else:
        a, fscale, sigma = 1.0, dt, None
    e = np.zeros(n)
    worst_sweeps, worst_resid = np.zeros(n, dtype=np.int64), np.zeros(n)
    for s in range(int(n_steps)):
        e, f = force_fn(x)
        if on_step is not None:
            on_step(s, x, v, e, f)
        kick = sigma * lo.md_normal(seed, conf, int(first_step) + s, comp) if sigma is not None else 0.0
        xref = x
        if scheme == 0:
            v = v + dt * f / m
            if wrong != "no_velocity_projection":
                v = project_velocities(cl, v, refvec(cl, x))
            x = x + 0.5 * dt * v
            v = a * v + kick
            x = x + 0.5 * dt * v
        else:
            v = a * v + fscale * f / m + kick
            x = x + dt * v
        xu = x
        x, sweeps, resid = project_positions(cl, xu, xu if wrong == "reference_from_new" else xref, tol, max_sweeps)
        if cl.n:
            v = v.copy()
            v[:, members] += (x[:, members] - xu[:, members]) / (1.0 if wrong == "no_inverse_dt" else dt)
            worst_sweeps = np.maximum(worst_sweeps, sweeps.max(axis=1))
            worst_resid = np.maximum(worst_resid, resid.max(axis=1))
    return x, v, np.asarray(e, dtype=np.float64), worst_sweeps, worst_resid


def constrained_steps(force_fn, masses, x, v, n_steps, dt, friction, kbT, scheme, seed, first_step, atoms, lengths, tol, max_sweeps,
                      conformations=None, wrong=None):
    """The call without state64: inputs rounded to float32 on entry, the result rounded to float32 once on exit, as
    `langevin_oracle.langevin_steps` -> (x, v, e, worst_sweeps, worst_residual)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    x, v, e, sw, res = constrained_steps64(force_fn, masses, x, v, n_steps, dt, friction, kbT, scheme, seed, first_step, atoms, lengths,
                                           tol, max_sweeps, conformations, wrong)
    return x.astype(np.float32), v.astype(np.float32), e, sw, res
