"""A float64 numpy restatement of the device energy minimiser (csrc/tw_md.hip `minimize_kernel` behind `tw_minimize` /
`timewarp_amd.md.minimize_energy`).  TEST INFRASTRUCTURE ONLY.

Written from the algorithm in the comment of `tw_minimize` in include/timewarp_hip.h: limited-memory BFGS (two-loop
recursion, initial scaling gamma = s.y / y.y of the newest pair, a ring of `history` pairs), first trial step 1 with a
history and min(1, max_displacement / max |d_i|) without, capped so that no coordinate moves by more than
`max_displacement`, Armijo backtracking (c1 = 1e-4, halving, 21 trials), the history dropped when the direction is no
descent direction or when 21 trials were rejected, status 0 converged / 1 budget used up / 2 stalled / 3 not finite at the
input.  Convergence: sqrt(g.g / 3V) <= tolerance on entry and after every accepted step.

One conformation per call.  `force_fn(x [N,V,3]) -> (E [N], F [N,V,3])` as in tests/langevin_oracle.py.  `reverse=True`
sums every reduction in the opposite index order: the distance between the two runs is the restatement's own sensitivity
to the order of summation, which is what the device's tree of partial sums differs from numpy's by."""
import numpy as np

C1 = 1e-4
TRIALS = 21
CURVATURE = 1e-10


def quadratic_forces(A, b):
    """force_fn of E(x) = 1/2 x.A x - b.x over the flattened coordinates (A symmetric [3V,3V])"""
    def force_fn(x):
        n = x.shape[0]
        f = x.reshape(n, -1)
        return 0.5 * np.einsum("ni,ij,nj->n", f, A, f) - f @ b, (-(f @ A) + b).reshape(x.shape)

    return force_fn


def bond_forces(r0, k):
    """analytic force_fn of two atoms joined by one harmonic bond, E = 1/2 k (|x0 - x1| - r0)^2"""
    def force_fn(x):
        d = x[:, 0] - x[:, 1]
        r = np.sqrt((d * d).sum(-1))
        g = (-k * (r - r0) / r)[:, None] * d      # force on atom 0
        return 0.5 * k * (r - r0) ** 2, np.stack([g, -g], axis=1)

    return force_fn


def minimize(force_fn, x, tolerance, n_iterations, history, max_displacement, reverse=False):
    """x [V,3] -> (x [V,3] float64, E, rms, iterations, evaluations, status, trace): `trace` lists E at the start and after
    every accepted step."""
    x = np.array(x, dtype=np.float64)
    shape, N = x.shape, x.size
    dot = (lambda a, b: float(np.sum((a * b)[::-1]))) if reverse else (lambda a, b: float(np.sum(a * b)))
    flat = lambda a: np.asarray(a, dtype=np.float64).reshape(-1)

    def evaluate(xf):
        e, f = force_fn(xf.reshape((1,) + shape))
        return float(e[0]), -flat(f[0])

    x = flat(x)
    E, g = evaluate(x)
    evaluations, iterations = 1, 0
    gg = dot(g, g)
    trace = [E]
    pairs = []      # oldest first: (s, y, rho)
    if not (np.isfinite(E) and np.isfinite(gg)):
        status = 3
    else:
        status = 0 if np.sqrt(gg / N) <= tolerance else 1
    for _ in range(int(n_iterations)):
        if status != 1:
            break
        for attempt in range(2):
            q = g.copy()
            alphas = []
            for s, y, rho in reversed(pairs):
                a = rho * dot(s, q)
                alphas.append(a)
                q = q - a * y
            if pairs:
                s, y, _ = pairs[-1]
                q = q * (dot(s, y) / dot(y, y))
            for (s, y, rho), a in zip(pairs, reversed(alphas)):
                b = rho * dot(y, q)
                q = q + (a - b) * s
            d = -q
            gd = dot(g, d)
            if pairs and not gd < 0.0:
                pairs = []
                d = -g
                gd = dot(g, d)
            dmax = float(np.abs(d).max())
            with np.errstate(divide="ignore"):
                t = 1.0 if pairs else min(1.0, max_displacement / dmax)
                t = min(t, max_displacement / dmax)
            accepted = False
            for _trial in range(TRIALS):
                xt = x + t * d
                Et, gt = evaluate(xt)
                evaluations += 1
                ggt = dot(gt, gt)
                if np.isfinite(Et) and np.isfinite(ggt) and Et <= E + C1 * t * gd:
                    accepted = True
                    break
                t *= 0.5
            if accepted:
                s, y = xt - x, gt - g
                sy, yy = dot(s, y), dot(y, y)
                if history > 0 and sy > CURVATURE * yy:
                    pairs.append((s, y, 1.0 / sy))
                    pairs = pairs[-history:]
                x, g, E, gg = xt, gt, Et, ggt
                iterations += 1
                trace.append(E)
                if np.sqrt(gg / N) <= tolerance:
                    status = 0
                break
            if pairs:
                pairs = []
            else:
                status = 2
                break
    return x.reshape(shape), E, float(np.sqrt(gg / N)), iterations, evaluations, status, np.array(trace)
