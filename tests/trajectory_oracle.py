"""A float64 restatement of the recording Langevin kernel (csrc/tw_md.hip `langevin_trajectory_kernel` behind
`tw_langevin_trajectory` / `LangevinDynamics.trajectory`).  TEST INFRASTRUCTURE ONLY.

Built on tests/langevin_oracle.py: the state is stepped from report step to report step with the update of
`lo.langevin_steps` and the noise of `lo.md_normal`, but - as the kernel does within a launch - it stays in float64 from
one report step to the next (`lo.langevin_steps` rounds to float32 when it returns, so it is called one segment at a time
only to CHECK the segment: `segment` below is its loop body, and `record` asserts that both give the same float32 state
whenever the segment started from float32 values).  At every report step: the force function's forces and energy at the
float64 positions, 1/2 sum m v^2 of the float64 velocities, and the float32 casts of positions and velocities.
"""
import numpy as np

from tests import langevin_oracle as lo


def segment(force_fn, m, x, v, n_steps, dt, friction, kbT, scheme, seed, first_step, conf):
    """`n_steps` steps of float64 x, v [N,V,3] without any rounding: the loop of `lo.langevin_steps`"""
    n, V, _ = x.shape
    comp = np.arange(3 * V).reshape(1, V, 3)
    if friction > 0.0:
        a = np.exp(-friction * dt)
        fscale = (1.0 - a) / friction
        sigma = np.sqrt(1.0 - a * a) * np.sqrt(kbT / m)
    else:
        a, fscale, sigma = 1.0, dt, None
    for s in range(int(n_steps)):
        _, f = force_fn(x)
        kick = sigma * lo.md_normal(seed, conf, int(first_step) + s, comp) if sigma is not None else 0.0
        if scheme == 0:
            v = v + dt * f / m
            x = x + 0.5 * dt * v
            v = a * v + kick
            x = x + 0.5 * dt * v
        else:
            v = a * v + fscale * f / m + kick
            x = x + dt * v
    return x, v


def record(force_fn, masses, x, v, report_steps, n_steps, dt, friction, kbT, scheme, seed, first_step, conformations=None):
    """x, v [N,V,3] (rounded to float32 on entry) -> dict: positions / velocities float32 [N,T,V,3], forces float64 [N,T,V,3],
    energies float64 [N,T,2] = (E_pot, E_kin) at the report steps (counted from the start, 0 = the input state), and
    final_x / final_v float32 [N,V,3] after `n_steps` steps."""
    x32, v32 = np.asarray(x, dtype=np.float32), np.asarray(v, dtype=np.float32)
    x, v = x32.astype(np.float64), v32.astype(np.float64)
    n, V, _ = x.shape
    m = np.asarray(masses, dtype=np.float32).astype(np.float64).reshape(1, V, 1)
    conf = (np.arange(n) if conformations is None else np.asarray(conformations)).reshape(n, 1, 1)
    args = (dt, friction, kbT, scheme, seed)
    pos, vel, frc, ene = [], [], [], []
    done = 0
    for r in list(report_steps) + [None]:
        target = int(n_steps) if r is None else int(r)
        assert target >= done
        x, v = segment(force_fn, m, x, v, target - done, *args, first_step + done, conf)
        if done == 0 and target > 0:   # the first segment starts from float32 values: it IS lo.langevin_steps
            wx, wv, _ = lo.langevin_steps(force_fn, masses, x32, v32, target, *args, first_step, conformations=conformations)
            assert np.array_equal(wx, x.astype(np.float32)) and np.array_equal(wv, v.astype(np.float32))
        done = target
        if r is not None:
            e, f = force_fn(x)
            pos.append(x.astype(np.float32))
            vel.append(v.astype(np.float32))
            frc.append(np.asarray(f, dtype=np.float64))
            ene.append(np.stack([np.asarray(e, dtype=np.float64), 0.5 * (m * v * v).sum(axis=(1, 2))], axis=-1))
    T = len(pos)
    stack = lambda a, tail, dt_: np.stack(a, axis=1) if T else np.zeros((n, 0) + tail, dtype=dt_)
    return {"positions": stack(pos, (V, 3), np.float32), "velocities": stack(vel, (V, 3), np.float32),
            "forces": stack(frc, (V, 3), np.float64), "energies": stack(ene, (2,), np.float64),
            "final_x": x.astype(np.float32), "final_v": v.astype(np.float32)}
