"""A float64 restatement of the device Langevin integrator (csrc/tw_md.hip `langevin_kernel` behind `tw_langevin_steps` /
timewarp_amd/md.py).  TEST INFRASTRUCTURE ONLY.

Written from the formulas of include/timewarp_hip.h:

    scheme 0  LangevinMiddleIntegrator  v += dt F/m;  x += dt/2 v;  v <- a v + sqrt(1 - a^2) sqrt(kT/m) N(0,1);  x += dt/2 v
    scheme 1  LangevinIntegrator        v <- a v + (1 - a)/friction F/m + sqrt(kT (1 - a^2)/m) N(0,1);  x += dt v
    a = exp(-friction dt);  friction 0 = plain leapfrog (a = 1, (1 - a)/friction -> dt, no noise)

and, for the noise, from the definition of `md_normal`: with `mix` one output step of splitmix64 from state z,

    k  = mix(seed ^ mix(conformation * 0x100000001B3 + step) ^ mix(0xD6E8FEB86659FD93 * (component + 1)))     (mod 2^64)
    u1 = ((k >> 11) + 1) / 2^53,  u2 = (mix(k) >> 11) / 2^53,  N = sqrt(-2 ln u1) cos(2 pi u2)

`step` = first_step + s is a 64-bit value, `component` = 3 * atom + axis.  The kernel reads float32 coordinates,
velocities and masses, keeps x and v in float64 between the steps of one call and rounds them to float32 once when it
returns; so does `langevin_steps`.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle.fake_sim import _State  # the Simulation-shaped shell of the other stand-in

MASK64 = (1 << 64) - 1
THREADS = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))


def _u64(a):
    """integers (Python ints of any sign, int64 / uint64 arrays) -> uint64 array, two's complement"""
    if isinstance(a, (int, np.integer)):
        return np.array(int(a) & MASK64, dtype=np.uint64)
    a = np.asarray(a)
    if a.dtype == np.uint64:
        return a
    if a.dtype == object:
        return np.array([int(v) & MASK64 for v in a.ravel()], dtype=np.uint64).reshape(a.shape)
    return a.astype(np.int64).view(np.uint64)


def md_mix(z):
    """one output of splitmix64 whose state is `z` before the increment (uint64 arithmetic wraps)"""
    with np.errstate(over="ignore"):
        z = _u64(z) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def md_key(seed, conformation, step, component):
    with np.errstate(over="ignore"):
        inner = _u64(conformation) * np.uint64(0x100000001B3) + _u64(step)
        comp = np.uint64(0xD6E8FEB86659FD93) * (_u64(component) + np.uint64(1))
        return md_mix(_u64(seed) ^ md_mix(inner) ^ md_mix(comp))


def md_normal(seed, conformation, step, component):
    """the standard normal of (seed, conformation, step, component); the arguments broadcast"""
    k = md_key(seed, conformation, step, component)
    k2 = md_mix(k)
    u1 = ((k >> np.uint64(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740993.0)   # (0, 1]; the constant rounds to 2^53
    u2 = (k2 >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def no_forces(x):
    return np.zeros(x.shape[0]), np.zeros_like(x)


def fd_forces(tables, h):
    """force_fn of `langevin_steps`: the C oracle's energy and its central differences with step `h` (nm), the 6V
    displaced copies of every row in ONE oracle call"""
    from tests import helpers as H

    def force_fn(x):
        n, V, _ = x.shape
        d = np.zeros((6 * V, V, 3))
        i = np.arange(3 * V)
        d[2 * i, i // 3, i % 3] = h
        d[2 * i + 1, i // 3, i % 3] = -h
        batch = np.concatenate([x, (x[:, None] + d[None]).reshape(-1, V, 3)])
        if len(batch) * V * V < 10 ** 7:
            e, _ = H.oracle_energy(tables, batch, dtype=np.float64)
        else:   # the protein: the C call releases the interpreter lock
            with ThreadPoolExecutor(THREADS) as pool:
                e = np.concatenate(list(pool.map(lambda c: H.oracle_energy(tables, c, dtype=np.float64)[0], np.array_split(batch, 4 * THREADS))))
        ed = e[n:].reshape(n, 3 * V, 2)
        return e[:n], (-(ed[:, :, 0] - ed[:, :, 1]) / (2.0 * h)).reshape(n, V, 3)

    return force_fn


def langevin_steps(force_fn, masses, x, v, n_steps, dt, friction, kbT, scheme, seed, first_step, conformations=None):
    """x, v [N,V,3] -> (x, v, e): `n_steps` steps in float64 of inputs rounded to float32 on entry, rounded to float32
    once on exit; e [N] is the potential energy at the positions of the LAST force evaluation (those before the last
    update).  `force_fn(x) -> (E [N], F [N,V,3])`.  Row r is conformation r of the noise key unless `conformations` names
    others."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    n, V, _ = x.shape
    m = np.asarray(masses, dtype=np.float32).astype(np.float64).reshape(1, V, 1)
    conf = (np.arange(n) if conformations is None else np.asarray(conformations)).reshape(n, 1, 1)
    comp = np.arange(3 * V).reshape(1, V, 3)
    if friction > 0.0:
        a = np.exp(-friction * dt)
        fscale = (1.0 - a) / friction
        sigma = np.sqrt(1.0 - a * a) * np.sqrt(kbT / m)
    else:
        a, fscale, sigma = 1.0, dt, None
    e = np.zeros(n)
    for s in range(int(n_steps)):
        e, f = force_fn(x)
        kick = sigma * md_normal(seed, conf, int(first_step) + s, comp) if sigma is not None else 0.0
        if scheme == 0:
            v = v + dt * f / m
            x = x + 0.5 * dt * v
            v = a * v + kick
            x = x + 0.5 * dt * v
        else:
            v = a * v + fscale * f / m + kick
            x = x + dt * v
    return x.astype(np.float32), v.astype(np.float32), np.asarray(e, dtype=np.float64)


class _Context:
    def __init__(self):
        self.pos = self.vel = None

    def setPositions(self, p):
        self.pos = np.array(p, dtype=np.float64)
        assert self.pos.ndim == 2 and self.pos.shape[1] == 3, self.pos.shape

    def setVelocities(self, v):
        self.vel = np.array(v, dtype=np.float64)
        assert self.vel.shape == self.pos.shape

    def getState(self, getPositions=False, getVelocities=False, **kwargs):
        return _State(self.pos, self.vel)


class RestatedSimulation:
    """`langevin_steps` behind the five calls `openmm_step` makes (context.setPositions, context.setVelocities, step,
    context.getState, state.getPositions / getVelocities - the shape of oracle/fake_sim.FakeSimulation), counting its
    steps as `LangevinDynamics.steps_done` does: one conformation, the noise key's conformation 0."""

    def __init__(self, force_fn, masses, dt, friction, kbT, scheme, seed):
        self.context = _Context()
        self.force_fn, self.masses = force_fn, masses
        self.dt, self.friction, self.kbT, self.scheme, self.seed = dt, friction, kbT, scheme, seed
        self.steps_done = 0
        self.calls = 0

    def step(self, n):
        c = self.context
        x, v, _ = langevin_steps(self.force_fn, self.masses, c.pos[None], c.vel[None], n, self.dt, self.friction, self.kbT,
                                 self.scheme, self.seed, self.steps_done)
        c.pos, c.vel = x[0].astype(np.float64), v[0].astype(np.float64)
        self.steps_done += int(n)
        self.calls += 1
