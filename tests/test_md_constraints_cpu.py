"""Hydrogen-bond constraints without a GPU: the cluster finder of timewarp_amd/forcefield.py `hbond_constraints`, the float64
restatement tests/constraint_oracle.py checked by itself (SHAKE residual, the velocity projection, momentum, zero clusters = the
unconstrained restatement bit for bit, the sweep bound, the temperature of force-free stars), the finite-difference error `u` and
the tolerance error `u_tol` of the restatement that tests/test_md_constraints_gpu.py holds the kernel to, and the host side:
fingerprint, command line, and where the driver projects.

`star_case`, `star_tolerance_error`, `constrained_case`, `crestated`, `star_temperature` are shared with the GPU tests."""
import dataclasses
import functools
import types

import numpy as np
import pytest
import torch

from tests import amber_oracle as ao
from tests import constraint_oracle as co
from tests import langevin_oracle as lo
from tests.test_langevin_cpu import FD_H, KBT, PRESET_KICK, REAL_CASES, REAL_RUNS, _cached_forces, real_case
from timewarp_amd import simulation as S
from timewarp_amd.forcefield import HBondConstraints, hbond_constraints

DT = 0.002            # ps: the step constraints are for
TOL = 1e-10           # the tolerance of every comparison with the kernel
TOL_FINE = 1e-13      # u_tol: the restatement at TOL against the restatement at TOL_FINE
SWEEPS = 32


# ---------------------------------------------------------------------------------------------
# the cluster finder
# ---------------------------------------------------------------------------------------------
def test_alanine_dipeptide_has_six_clusters_and_twelve_constraints():
    tables, masses, _, _ = real_case("ad")
    c = hbond_constraints(tables, masses)
    assert c.n_clusters == 6 and c.n_constraints == 12
    assert [(int((row[1:] >= 0).sum())) for row in c.atoms] == [3, 1, 1, 3, 1, 3]
    assert c.atoms.dtype == np.int32 and c.lengths.dtype == np.float64 and c.tolerance == 1e-8 and c.max_sweeps == 32
    assert list(c.atoms[:, 0]) == sorted(c.atoms[:, 0])                      # ordered by centre
    assert all(list(r[1:][r[1:] >= 0]) == sorted(r[1:][r[1:] >= 0]) for r in c.atoms)     # hydrogens ascending
    # lengths are the r0 of that bond: C-H 0.109, N-H 0.101 nm
    bonds = {tuple(sorted(b)): p[0] for b, p in zip(tables.bond_idx.tolist(), tables.bond_par.tolist())}
    for row, d in zip(c.atoms, c.lengths):
        for a in range(3):
            assert d[a] == (bonds[tuple(sorted((int(row[0]), int(row[1 + a]))))] if row[1 + a] >= 0 else 0.0)
    assert sorted(set(np.round(c.lengths[c.lengths > 0], 4))) == [0.101, 0.109]
    # the tables are not touched
    assert S.tables_digest(tables) == S.tables_digest(real_case("ad")[0])


@pytest.mark.parametrize("mol", ["nnqq", "1hgv"])
def test_every_hydrogen_of_the_committed_molecules_sits_in_exactly_one_cluster(mol):
    from tests.test_energy_kat import kat, protein

    tables, masses, _, _ = real_case(mol)
    z = kat() if mol == "nnqq" else protein()
    elements = [str(e) for e in z["elements"]] if "elements" in z.files else [next(ch for ch in str(n) if ch.isalpha()) for n in z["atom_names"]]
    c = hbond_constraints(tables, masses)
    hydrogens = [i for i, e in enumerate(elements) if e == "H"]
    assert c.n_constraints == len(hydrogens) > 0
    assert sorted(c.atoms[:, 1:][c.atoms[:, 1:] >= 0].tolist()) == hydrogens
    assert not set(c.atoms[:, 0].tolist()) & set(hydrogens)
    print(f"{mol}: {c.n_clusters} clusters, {c.n_constraints} constraints, sizes {np.bincount((c.atoms[:, 1:] >= 0).sum(1))[1:].tolist()}")


def methane_tables():
    from timewarp_amd.forcefield import ForceFieldTables

    z = lambda w, t=np.float64: np.zeros((0, w), dtype=t)
    return ForceFieldTables(bond_idx=np.array([[2, 0], [2, 1], [2, 3], [4, 2]], dtype=np.int32), bond_par=np.array([[0.109, 3e5]] * 4),
                            angle_idx=z(3, np.int32), angle_par=z(2), torsion_idx=z(4, np.int32), torsion_par=z(3), exc_idx=z(2, np.int32),
                            exc_par=z(3), atom_par=np.array([[0.0, 0.3, 0.0, 0.15, 0.8]] * 5), has_gbsa=0)


def test_a_centre_with_four_hydrogens_is_refused_by_name():
    with pytest.raises(ValueError, match=r"atom 2 carries 4 hydrogens"):
        hbond_constraints(methane_tables(), [1.008, 1.008, 12.01, 1.008, 1.008])
    # three of them and a heavy neighbour: fine; H-H (no heavy partner) is no constraint
    c = hbond_constraints(methane_tables(), [1.008, 1.008, 12.01, 1.008, 14.01])
    assert c.atoms.tolist() == [[2, 0, 1, 3]]
    assert hbond_constraints(methane_tables(), [1.008] * 5).n_clusters == 0
    with pytest.raises(ValueError, match="one mass per atom"):
        hbond_constraints(methane_tables(), [1.0] * 4)


def test_check_refuses_by_field_name():
    good = HBondConstraints(np.array([[2, 0, 1, -1], [4, 3, -1, -1]], dtype=np.int32), np.array([[0.1, 0.11, 0.0], [0.1, 0.0, 0.0]]), 5)
    assert good.check() is good and good.n_constraints == 3

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            dataclasses.replace(good, **kw).check()

    a = good.atoms
    bad("^atoms: index out of range", atoms=np.array([[2, 0, 5, -1], [4, 3, -1, -1]], dtype=np.int32))
    bad("^atoms: index out of range", atoms=np.array([[-1, 0, 1, -1], [4, 3, -1, -1]], dtype=np.int32))
    bad("^atoms: atom 0 is in two clusters", atoms=np.array([[2, 0, 1, -1], [4, 0, -1, -1]], dtype=np.int32))
    bad("^atoms: atom 2 is in two clusters", atoms=np.array([[2, 0, 1, -1], [4, 2, -1, -1]], dtype=np.int32))
    bad("^atoms: every cluster has at least one hydrogen", atoms=np.array([[2, -1, 1, -1], [4, 3, -1, -1]], dtype=np.int32))
    bad("^atoms: expected an integer array", atoms=a.astype(np.float64))
    bad("^lengths: every constrained bond needs a finite positive length", lengths=np.array([[0.1, 0.0, 0.0], [0.1, 0.0, 0.0]]))
    bad("^lengths: every constrained bond", lengths=np.array([[0.1, np.nan, 0.0], [0.1, 0.0, 0.0]]))
    bad("^lengths: expected a float array", lengths=np.zeros((2, 2)))
    for t in (0.0, -1e-8, np.inf, np.nan):
        bad("^tolerance:", tolerance=t)
    for s in (0, 65, -1, 2.5):
        bad("^max_sweeps:", max_sweeps=s)
    assert dataclasses.replace(good, max_sweeps=1).check() and dataclasses.replace(good, max_sweeps=64).check()


# ---------------------------------------------------------------------------------------------
# force-free stars (shared with the GPU tests)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def star_case(V, rows, seed=0):
    """(masses float32 [V], atoms, lengths, x float32, v float32): V < 5: one cluster (0; 1 .. V - 1); otherwise V / 4 stars of three
    hydrogens, atoms (4 i; 4 i + 1, 4 i + 2, 4 i + 3), centres 0.6 nm apart on a grid.  Distinct masses and lengths; the float32 state
    is the rounding of a float64 state that meets the constraints and whose velocities are projected."""
    rng = np.random.default_rng(7000 * V + rows + seed)
    if V < 5:
        atoms = np.array([[0] + list(range(1, V)) + [-1] * (4 - V)], dtype=np.int32)
    else:
        assert V % 4 == 0
        atoms = np.array([[4 * i, 4 * i + 1, 4 * i + 2, 4 * i + 3] for i in range(V // 4)], dtype=np.int32)
    C = atoms.shape[0]
    used = atoms[:, 1:] >= 0
    lengths = np.where(used, 0.096 + 0.001 * (np.arange(3 * C).reshape(C, 3) % 17), 0.0)
    masses = np.zeros(V, dtype=np.float32)
    masses[atoms[:, 0]] = 12.0 + 0.37 * np.arange(C)
    masses[atoms[:, 1:][used]] = 1.0 + 0.011 * np.arange(int(used.sum()))
    side = int(np.ceil(C ** (1.0 / 3.0)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:C] * 0.6
    x = np.zeros((rows, V, 3))
    x[:, atoms[:, 0]] = grid[None] + 0.05 * rng.standard_normal((rows, C, 3))
    for a in range(3):
        u = used[:, a]
        d = rng.standard_normal((rows, int(u.sum()), 3))
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        x[:, atoms[u, 1 + a]] = x[:, atoms[u, 0]] + lengths[u, a][None, :, None] * d
    v = rng.standard_normal((rows, V, 3)) * np.sqrt(KBT / masses.astype(np.float64))[None, :, None]
    cl = co.Clusters(atoms, lengths, masses)
    x, v, _ = co.apply_constraints(cl, x, v, 1e-14, 64)
    return masses, atoms, lengths, x.astype(np.float32), v.astype(np.float32)


STAR_SEED, STAR_FIRST_STEP = 0x9E3779B97F4A7C15 ^ 4242, 1000003


def star_run(V, rows, steps, friction, scheme, tol=TOL, dt=DT):
    masses, atoms, lengths, x, v = star_case(V, rows)
    return co.constrained_steps64(lo.no_forces, masses, x.astype(np.float64), v.astype(np.float64), steps, dt, friction, KBT, scheme, STAR_SEED,
                                  STAR_FIRST_STEP, atoms, lengths, tol, SWEEPS)


@functools.lru_cache(maxsize=None)
def star_tolerance_error(V, rows, steps, friction, scheme):
    """(u_tol_x, u_tol_v, run at TOL): the largest float64 difference between the restatement at TOL and at TOL_FINE"""
    a, b = star_run(V, rows, steps, friction, scheme, TOL), star_run(V, rows, steps, friction, scheme, TOL_FINE)
    return float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max()), a


def _momentum(masses, y):
    return (masses.astype(np.float64)[None, :, None] * y).sum(axis=1)


@pytest.mark.parametrize("V", [2, 3, 4, 64, 68])
def test_projections_of_the_restatement(V):
    """After SHAKE the residual is within the tolerance; after the velocity projection no constrained bond changes length to first
    order; both conserve each cluster's momentum (clusters are disjoint, so the total is the sum) to rounding; atoms outside are not
    touched."""
    masses, atoms, lengths, x, v = star_case(V, 3)
    rng = np.random.default_rng(V)
    cl = co.Clusters(atoms, lengths, masses)
    x = x.astype(np.float64) * (1.0 + 0.02 * rng.standard_normal(x.shape))       # bonds some 2 % off
    v = v.astype(np.float64) + rng.standard_normal(v.shape)
    for tol in (1e-6, 1e-10, 1e-13):
        x2, sweeps, resid = co.project_positions(cl, x, x, tol, 64)
        assert resid.max() <= tol and 2 <= sweeps.max() < 64
        assert np.abs(_momentum(masses, x2 - x)).max() <= 1e-13 * np.abs(_momentum(masses, np.abs(x))).max()
    d2 = ((x2[:, cl.c][:, :, None] - x2[:, cl.h]) ** 2).sum(-1)
    assert np.all(np.abs(d2 - cl.d2[None])[:, cl.used] <= 1e-13 * cl.d2[cl.used])
    r = co.refvec(cl, x2)
    v2 = co.project_velocities(cl, v, r)
    rel = ((v2[:, cl.c][:, :, None] - v2[:, cl.h]) * r).sum(-1)
    scale = np.linalg.norm(v, axis=-1).max() * np.sqrt(cl.d2.max())
    assert np.abs(rel[:, cl.used]).max() <= 1e-12 * scale
    assert np.abs(_momentum(masses, v2 - v)).max() <= 1e-13 * np.abs(_momentum(masses, np.abs(v))).max()
    assert np.abs(v2 - v).max() > 0.1
    # one sweep allowed: the residual says that it did not suffice
    _, sweeps, resid = co.project_positions(cl, x, x, 1e-10, 1)
    assert sweeps.max() == 1 and resid.max() > 1e-10


@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("friction", [0.0, 0.3])
def test_zero_clusters_is_the_unconstrained_restatement_bit_for_bit(scheme, friction):
    tables, masses, x0, v0 = real_case("ad")
    fn = lambda x: tuple(t.numpy() for t in ao.energy_and_forces(tables, x))
    want = lo.langevin_steps(fn, masses, x0[:2], v0[:2], 5, DT / 4, friction, KBT, scheme, 9, 11)
    got = co.constrained_steps(fn, masses, x0[:2], v0[:2], 5, DT / 4, friction, KBT, scheme, 9, 11, np.zeros((0, 4), dtype=np.int32),
                               np.zeros((0, 3)), TOL, SWEEPS)
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], want)) and got[3].max() == 0 and got[4].max() == 0.0


@functools.lru_cache(maxsize=None)
def constrained_case(mol):
    """`real_case` with the constraint set and a start that meets it: (tables, masses, atoms, lengths, x0 float32, v0 float32) - the
    committed conformations projected in float64 (positions, then the thermal velocities) and rounded to float32."""
    tables, masses, x0, v0 = real_case(mol)
    c = hbond_constraints(tables, masses)
    cl = co.Clusters(c.atoms, c.lengths, masses)
    x0 = x0.astype(np.float64)
    if mol == "1hgv":
        # The unconstrained case uses the one committed frame with no pair of atoms within 3 h of the 2 nm cutoff (a central
        # difference across the cutoff is wrong, and after the first step the whole row would have to be left out).  The projection
        # moves 572 of the 691 atoms and brings some twenty atoms into that window, as in every other frame.  So the frame is
        # scaled by 1 + 2e-5 k before it is projected - every distance near the cutoff moves by 4e-5 k nm, about the width of the
        # window - for the smallest k = 0, 1, 2, ... at which the projected float32 start has no such pair (k stays below 1000: under
        # 2 % on every length, which the projection takes back on the X-H bonds).  Both rows start there, as in the unconstrained case.
        for k in range(1000):
            xs = co.apply_constraints(cl, x0[:1] * (1.0 + 2e-5 * k), None, 1e-14, 64)[0].astype(np.float32).astype(np.float64)
            d = np.linalg.norm(xs[0, :, None] - xs[0, None], axis=-1)
            if not (np.abs(d - tables.cutoff) < 3 * FD_H).any():
                break
        else:
            raise AssertionError("no scaling of the frame keeps every pair out of the cutoff window")
        x0 = np.repeat(xs, x0.shape[0], axis=0)
    x, v, resid = co.apply_constraints(cl, x0, v0.astype(np.float64), 1e-14, 64)
    assert resid.max() <= 1e-14
    return tables, masses, c.atoms, c.lengths, x.astype(np.float32), v.astype(np.float32)


def oracle_forces(mol):
    tables = real_case(mol)[0]
    return lambda x: tuple(t.numpy() for t in ao.energy_and_forces(tables, x))


def test_sweep_bound_on_alanine_dipeptide():
    """2 rows, 50 steps of 2 fs at tolerance 1e-10 with the autograd forces: never more than 16 sweeps, half the default bound."""
    tables, masses, atoms, lengths, x0, v0 = constrained_case("ad")
    out = co.constrained_steps64(oracle_forces("ad"), masses, x0[:2].astype(np.float64), v0[:2].astype(np.float64), 50, DT, 1.0, KBT, 0, 5, 0,
                                 atoms, lengths, TOL, SWEEPS)
    print(f"alanine dipeptide, 50 steps of 2 fs, tol 1e-10: worst sweeps {out[3].max()}, worst residual {out[4].max():.2e}")
    assert out[3].max() <= 16 and out[4].max() <= TOL and np.isfinite(out[0]).all()


class CRestated:
    """The constrained restatement of one case of tests/test_langevin_cpu.py REAL_CASES at 2 fs and tolerance 1e-10, with central
    differences of step h and h / 2: what is compared, the finite-difference error u and the tolerance error u_tol."""

    def __init__(self, mol, scheme, friction, h=FD_H):
        tables, masses, atoms, lengths, x0, v0 = constrained_case(mol)
        rows, steps = REAL_RUNS[mol]
        # The seed is arbitrary.  On the protein the share of components left out at the cutoff depends on it - whole clusters are left
        # out, since the projections hand a wrong force on within a step: 3.3 .. 6.0 % for LangevinMiddle over the seeds 4321, 4323, ..,
        # 4335 and 2.9 .. 4.4 % for Langevin over 4322 .. 4336, measured on the restatement alone - and the 5 % condition below is
        # asserted for the one used.
        self.steps, self.seed, self.first_step = steps, 4325 + scheme, 23
        self.args = (masses, x0, v0, steps, DT, friction, KBT, scheme, self.seed, self.first_step, atoms, lengths)
        run = lambda hh, tol=TOL, n=steps: co.constrained_steps64(_cached_forces(mol, hh), masses, x0.astype(np.float64), v0.astype(np.float64),
                                                                   n, DT, friction, KBT, scheme, self.seed, self.first_step, atoms, lengths, tol,
                                                                   SWEEPS)
        coarse, fine, finer_tol = run(h), run(h / 2), run(h / 2, TOL_FINE)
        self.fine64 = fine
        self.fine = (fine[0].astype(np.float32), fine[1].astype(np.float32), fine[2])
        keep = np.ones(x0.shape, dtype=bool)
        if mol == "1hgv":      # atoms with a partner within 3 h of the cutoff at a force evaluation (tests/test_langevin_cpu.py Restated)
            evals = [(0, x0.astype(np.float64))] + ([(steps - 1, run(h / 2, TOL, steps - 1)[0])] if steps > 1 else [])
            for s, x in evals:
                d = np.linalg.norm(x[:, :, None] - x[:, None], axis=-1)
                near = (np.abs(d - tables.cutoff) < 3 * h).any(axis=2)
                # the projections hand a wrong force on to the other atoms of the cluster within the same step
                cl = co.Clusters(atoms, lengths, masses)
                members = np.concatenate([cl.c[:, None], cl.h], axis=1)                   # [C, 4]; unused slots repeat the centre
                hit = near[:, members].any(axis=2)                                          # [N, C]
                for j in range(4):
                    near[:, members[:, j]] |= hit
                keep[near] = False
                if s < steps - 1:
                    keep[near.any(axis=1)] = False
        self.keep, self.left_out = keep, 1.0 - keep.mean()
        f32 = lambda a: a.astype(np.float32).astype(np.float64)
        self.u_x = float(np.abs(f32(coarse[0]) - f32(fine[0]))[keep].max())
        self.u_v = float(np.abs(f32(coarse[1]) - f32(fine[1]))[keep].max())
        self.u_tol_x = float(np.abs(fine[0] - finer_tol[0])[keep].max())
        self.u_tol_v = float(np.abs(fine[1] - finer_tol[1])[keep].max())
        self.sweeps, self.residual = int(fine[3].max()), float(fine[4].max())

    def bounds(self):
        """|kernel - out(h / 2)| <= 4 u + 1 ulp32 (tests/test_langevin_cpu.py Restated.bounds)"""
        return (4 * self.u_x + np.spacing(np.abs(self.fine[0])), 4 * self.u_v + np.spacing(np.abs(self.fine[1])))


@functools.lru_cache(maxsize=None)
def crestated(mol, scheme, friction):
    return CRestated(mol, scheme, friction)


@pytest.mark.parametrize("mol,scheme,friction", REAL_CASES)
def test_finite_difference_and_tolerance_error_of_the_constrained_restatement(mol, scheme, friction):
    """u = max |out(h) - out(h / 2)| of the constrained restatement at 2 fs (float32 results, as compared with the kernel), and
    u_tol = max |out(tol 1e-10) - out(tol 1e-13)| in float64.  Conditions on the restatement alone: 100 u is at most one
    thermostat kick on a hydrogen at the preset (for coordinates: that kick over one 2 fs step of this run), at most 5 % of the components are
    left out at the cutoff; u_tol is printed and is far below one float32 ulp of the results.

    Measured (u_x nm, u_v nm/ps; u_tol_x nm, u_tol_v nm/ps; 6 sweeps and a residual of 9.9e-11 .. 1.0e-10 in every case):
      ad    u_x 1.5e-8 .. 6.0e-8, u_v 2.4e-7;            u_tol 4.2e-12 .. 4.6e-12 / 2.1e-9 .. 3.4e-9;  nothing left out
      nnqq  u_x 6.0e-8 .. 1.2e-7, u_v 2.4e-7 .. 1.1e-6;  u_tol 2.5e-11 .. 3.7e-11 / 3.7e-9 .. 4.6e-9;  nothing left out
      1hgv  u_x 1.2e-7, u_v 4.8e-7 / 1.1e-6;             u_tol 1.1e-10 .. 1.2e-10 / 5.3e-8 .. 6.0e-8;  3.84 % / 3.69 % left out
    - u is one to four float32 ulp of the results, 2e4 times below the kick of 0.0277 nm/ps; u_tol is below a tenth of an ulp."""
    r = crestated(mol, scheme, friction)
    print(f"{mol} scheme {scheme} friction {friction} at 2 fs: u_x {r.u_x:.3e} nm, u_v {r.u_v:.3e} nm/ps, u_tol_x {r.u_tol_x:.3e}, "
          f"u_tol_v {r.u_tol_v:.3e}, sweeps {r.sweeps}, residual {r.residual:.2e}, left out {100 * r.left_out:.2f} %")
    assert 100.0 * r.u_v <= PRESET_KICK and 100.0 * r.u_x <= PRESET_KICK * DT      # how far that kick carries a hydrogen in one step of this run
    assert r.left_out <= 0.05
    assert r.sweeps <= 16 and r.residual <= TOL
    _, _, _, _, x0, v0 = constrained_case(mol)
    assert np.abs(r.fine[1] - v0)[r.keep].max() > 1000 * (4 * r.u_v + 1e-7)


# ---------------------------------------------------------------------------------------------
# energy conservation of the restatement (the yardstick of the GPU test)
# ---------------------------------------------------------------------------------------------
def total_energy(masses, atoms, lengths, x, v, f, e_pot, dt):
    """[T]: E_pot + the kinetic energy of the frames' velocities moved to the full step - v + (dt/2) F / m - and projected onto the
    constraints at the frame's positions (the stored velocities of a leapfrog live half a step earlier: their kinetic energy
    oscillates in first order of dt).  x, v, f [T, V, 3] of one row, any float type."""
    m = np.asarray(masses, dtype=np.float64)[None, :, None]
    x, v, f = (np.asarray(a, dtype=np.float64) for a in (x, v, f))
    cl = co.Clusters(atoms, lengths, masses)
    w = co.project_velocities(cl, v + 0.5 * dt * f / m, co.refvec(cl, x))
    return np.asarray(e_pot, dtype=np.float64) + 0.5 * (m * w * w).sum(axis=(1, 2))


def oracle_energy_excursion(dt=DT, steps=1000, every=10):
    """max |E(t) - E(0)| of the float64 restatement with autograd forces: alanine dipeptide, row 0 of `constrained_case`, friction 0,
    frames every `every` steps (the run of the GPU test)."""
    tables, masses, atoms, lengths, x0, v0 = constrained_case("ad")
    frames = []

    def on_step(s, x, v, e, f):
        if s % every == 0:
            frames.append((x[0].copy(), v[0].copy(), f[0].copy(), float(e[0])))

    fn = oracle_forces("ad")
    x, v, _, _, _ = co.constrained_steps64(fn, masses, x0[:1].astype(np.float64), v0[:1].astype(np.float64), steps, dt, 0.0, KBT, 0, 1, 0, atoms,
                                           lengths, TOL, SWEEPS, on_step=on_step)
    e, f = fn(x)
    frames.append((x[0], v[0], f[0], float(e[0])))
    en = total_energy(masses, atoms, lengths, *(np.stack([fr[i] for fr in frames]) for i in range(3)), np.array([fr[3] for fr in frames]), dt)
    return float(np.abs(en - en[0]).max())


# kJ/mol: oracle_energy_excursion() over 1000 steps of 2 fs, measured once (profiles/md_constraints.txt); a tenth of the run is
# repeated by test_the_recorded_energy_excursion_is_the_restatements
AD_EXCURSION_2FS = 3.7310
AD_EXCURSION_2FS_100_STEPS = 2.9765      # the first 100 of those steps


def test_the_recorded_energy_excursion_is_the_restatements():
    got = oracle_energy_excursion(DT, 100, 10)
    print(f"total-energy excursion of the restatement over the first 100 steps of 2 fs: {got:.4f} kJ/mol")
    assert abs(got - AD_EXCURSION_2FS_100_STEPS) <= 1e-3


# ---------------------------------------------------------------------------------------------
# temperature of force-free stars
# ---------------------------------------------------------------------------------------------
STAR_T_ROWS, STAR_T_STEPS, STAR_T_FRICTION = 4096, 2000, 10.0


@functools.lru_cache(maxsize=None)
def star_temperature():
    """(relative deviation of the mean kinetic temperature from the target, mean T / target): 4096 rows of one 3-hydrogen star, no
    forces, friction 10 / ps, 2 fs, LangevinMiddle; the stored velocities after every step of the second half of 2000 steps; 9
    degrees of freedom per row."""
    masses, atoms, lengths, x, v = star_case(4, STAR_T_ROWS)
    m = masses.astype(np.float64)[None, :, None]
    x, v = x.astype(np.float64), v.astype(np.float64)
    total, count = 0.0, 0
    for s in range(STAR_T_STEPS):
        x, v, _, _, _ = co.constrained_steps64(lo.no_forces, masses, x, v, 1, DT, STAR_T_FRICTION, KBT, 0, STAR_SEED, s, atoms, lengths, 1e-8, SWEEPS)
        if s >= STAR_T_STEPS // 2:
            total += float((m * v * v).sum() / STAR_T_ROWS)
            count += 1
    ratio = total / count / (9.0 * KBT)
    return abs(ratio - 1.0), ratio


def test_force_free_stars_hold_their_temperature():
    dev, ratio = star_temperature()
    print(f"force-free 3-hydrogen stars, 4096 rows, friction 10 / ps, 2 fs: <T_kin> / T = {ratio:.5f} (9 degrees of freedom per row)")
    assert dev <= 0.005


# ---------------------------------------------------------------------------------------------
# host side: fingerprint, command line, where the driver projects
# ---------------------------------------------------------------------------------------------
from tests.test_md_checkpoint_cpu import FakeDynamics, system      # noqa: E402

FAKE_ATOMS = np.array([[0, 1, -1, -1], [2, 4, -1, -1]], dtype=np.int32)      # masses 12.01, 1.008, 14.01, 16.0, 1.008
FAKE_LENGTHS = np.array([[0.03, 0.0, 0.0], [0.025, 0.0, 0.0]])


class ConstrainedFake(FakeDynamics):
    """FakeDynamics with a constraint set and the restated `apply_constraints`; every call is written into `events`"""

    def __init__(self, masses, constraints, events, **kw):
        super().__init__(masses, **kw)
        self.constraints, self.events, self.constraint_residual = constraints, events, None

    def apply_constraints(self, coords, velocs=None, state=None):
        assert coords is None and state is not None
        cl = co.Clusters(self.constraints.atoms, self.constraints.lengths, self.masses.numpy())
        x, v, resid = co.apply_constraints(cl, state[:, 0].numpy(), state[:, 1].numpy(), self.constraints.tolerance, self.constraints.max_sweeps)
        state[:, 0], state[:, 1] = torch.from_numpy(x), torch.from_numpy(v)
        self.constraint_residual = torch.from_numpy(resid)
        self.events.append(("apply", self.steps_done))
        return state[:, 0].float(), state[:, 1].float()

    def trajectory(self, coords, velocs, report_steps, num_steps=None, state=None, velocities="stored"):
        self.events.append(("launch", self.steps_done, state.clone()))
        return super().trajectory(coords, velocs, report_steps, num_steps=num_steps, state=state, velocities=velocities)


def fake_constraints(**kw):
    return HBondConstraints(FAKE_ATOMS, FAKE_LENGTHS, 5, **kw)


def test_fingerprint_knows_the_constraints():
    energy, masses, x, v = system()
    kw = dict(burn_in=3, sampling=24, seed=4, reports=[5, 9], velocities="stored", redraw_velocities=False, minimize=False, min_tol=2.0)
    plain = S.run_fingerprint(energy, FakeDynamics(masses), x, v, **kw)
    assert S.FINGERPRINT_FIELDS[-1] == "constraints" and plain["constraints"] is None
    # an unconstrained run's fingerprint is what it was in every other field, and an old file without the key compares equal
    old = {k: val for k, val in plain.items() if k != "constraints"}
    assert sorted(old) == sorted(S.FINGERPRINT_FIELDS[:-1])
    assert S.first_difference(old, plain) is None and S.first_difference(plain, old) is None
    on = S.run_fingerprint(energy, ConstrainedFake(masses, fake_constraints(), []), x, v, **kw)
    assert sorted(on["constraints"]) == ["max_sweeps", "tables", "tolerance"] and on["constraints"]["tolerance"] == 1e-8
    assert {k: val for k, val in on.items() if k != "constraints"} == old
    for other in (fake_constraints(tolerance=1e-9), fake_constraints(max_sweeps=16),
                  HBondConstraints(FAKE_ATOMS, FAKE_LENGTHS * 1.01, 5), HBondConstraints(FAKE_ATOMS[:1], FAKE_LENGTHS[:1], 5)):
        fp = S.run_fingerprint(energy, ConstrainedFake(masses, other, []), x, v, **kw)
        assert S.first_difference(on, fp) == "constraints"
    assert S.first_difference(plain, on) == "constraints" and S.first_difference(old, on) == "constraints"


def test_a_checkpoint_with_other_constraints_is_refused(tmp_path):
    energy, masses, x, v = system()
    run = lambda md, **kw: S.simulate_trajectory(energy, masses, x, v, burn_in=3, sampling=24, spacing=S.LogarithmicSpacing(10, 3), integrator=md,
                                                 steps_per_launch=7, out_dir=str(tmp_path), name="fake", seed=4,
                                                 checkpoint=str(tmp_path / "ck"), **kw)
    assert run(ConstrainedFake(masses, fake_constraints(), []), max_steps=10) is None
    with pytest.raises(ValueError, match="`constraints`"):
        run(ConstrainedFake(masses, fake_constraints(tolerance=1e-9), []))
    with pytest.raises(ValueError, match="`constraints`"):
        run(FakeDynamics(masses))
    whole = S.simulate_trajectory(energy, masses, x, v, burn_in=3, sampling=24, spacing=S.LogarithmicSpacing(10, 3),
                                  integrator=ConstrainedFake(masses, fake_constraints(), []), steps_per_launch=5, seed=4)
    rest = run(ConstrainedFake(masses, fake_constraints(), []))
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(whole, rest) for k in a)


def test_cli_flags_parse():
    p = S.build_parser()
    d = p.parse_args(["--out", "o"])
    assert d.constraints == "none" and d.constraint_tolerance is None and d.timestep_fs is None
    a = p.parse_args(["--out", "o", "--constraints", "h-bonds", "--constraint-tolerance", "1e-9", "--timestep-fs", "2"])
    assert a.constraints == "h-bonds" and a.constraint_tolerance == 1e-9 and a.timestep_fs == 2.0
    with pytest.raises(SystemExit):
        p.parse_args(["--out", "o", "--constraints", "all-bonds"])


def test_the_driver_projects_after_minimise_and_after_the_redraw(monkeypatch):
    """Order of events of a constrained run with minimisation and a velocity redraw: minimise, project (positions and the drawn
    velocities), burn-in launches, redraw + project, sampling launches - and the states the launches start from meet the
    constraints in both halves."""
    import timewarp_amd.md as md_module

    energy, masses, x, v = system()
    events = []

    def fake_minimize(energy_, coords, tolerance=10.0, **kw):
        events.append(("minimize",))
        return types.SimpleNamespace(status=torch.zeros(coords.shape[0], dtype=torch.int32), coords=coords * 1.25)

    monkeypatch.setattr(md_module, "minimize_energy", fake_minimize)
    cons = fake_constraints(tolerance=1e-12)
    md = ConstrainedFake(masses, cons, events)
    rows = S.simulate_trajectory(energy, masses, x, None, burn_in=6, sampling=10, spacing=S.RegularSpacing(5), integrator=md, steps_per_launch=4,
                                 seed=4, minimize=True, redraw_velocities=True)
    kinds = [(e[0],) + ((e[1],) if e[0] != "minimize" else ()) for e in events]
    assert kinds == [("minimize",), ("apply", 0), ("launch", 0), ("launch", 4), ("apply", 6), ("launch", 6), ("launch", 10), ("launch", 14)]
    cl = co.Clusters(cons.atoms, cons.lengths, masses.numpy())
    first, sampling = events[2][2].numpy(), events[5][2].numpy()
    for st in (first, sampling):
        r = co.refvec(cl, st[:, 0])
        assert np.all(np.abs((r * r).sum(-1) - cl.d2[None])[:, cl.used] <= 1e-12 * cl.d2[cl.used])
        rel = ((st[:, 1][:, cl.c][:, :, None] - st[:, 1][:, cl.h]) * r).sum(-1)
        assert np.abs(rel[:, cl.used]).max() <= 1e-12
    # the minimiser's coordinates were projected, not the input's: atom 3 (in no cluster) is where the minimiser left it
    assert np.array_equal(first[:, 0, 3].astype(np.float32), (x * 1.25)[:, 3].numpy())
    # the redraw replaced the velocities (atom 3 again: no projection touches it) and left the positions alone
    before_redraw = events[3][2]
    assert not np.array_equal(sampling[:, 1, 3], before_redraw[:, 1, 3].numpy())
    assert len(rows) == 2 and rows[0]["step"].tolist() == [10, 15]


def test_a_residual_above_the_tolerance_stops_the_run_naming_the_row(tmp_path):
    energy, masses, x, v = system()

    class Failing(ConstrainedFake):
        def trajectory(self, *a, **kw):
            out = super().trajectory(*a, **kw)
            self.constraint_residual = torch.tensor([0.0, 3e-5 if self.steps_done > 7 else 0.0], dtype=torch.float64)
            return out

    run = lambda **kw: S.simulate_trajectory(energy, masses, x, v, burn_in=3, sampling=24, spacing=S.LogarithmicSpacing(10, 3),
                                             integrator=Failing(masses, fake_constraints(), []), steps_per_launch=7, seed=4, **kw)
    with pytest.raises(RuntimeError, match=r"row 1 residual 3\.000e-05"):
        run()
    with pytest.raises(RuntimeError, match=r"row 1 residual"):
        run(checkpoint=str(tmp_path / "ck"), checkpoint_steps=1, out_dir=str(tmp_path))
    saved = S.read_checkpoint(S.checkpoint_path(str(tmp_path / "ck")))
    assert saved["steps_done"] <= 7       # the state after the failing launch was never written


def test_constraints_argument_needs_an_integrator_that_has_them():
    energy, masses, x, v = system()
    with pytest.raises(ValueError, match="constraints= builds the default integrator"):
        S.simulate_trajectory(energy, masses, x, v, burn_in=0, sampling=5, spacing=S.RegularSpacing(5), integrator=FakeDynamics(masses),
                              constraints="h-bonds")
    with pytest.raises(ValueError, match="constraint_tolerance needs constraints="):
        S.simulate_trajectory(energy, masses, x, v, burn_in=0, sampling=5, spacing=S.RegularSpacing(5), integrator=FakeDynamics(masses),
                              constraint_tolerance=1e-9)
