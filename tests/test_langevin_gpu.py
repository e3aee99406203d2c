"""The device Langevin integrator (csrc/tw_md.hip `langevin_kernel<W>` behind `tw_langevin_steps` / timewarp_amd/md.py) step for
step against its float64 restatement, tests/langevin_oracle.py - the update formulas, `(1 - a) / friction`, the noise
scale, the mass of every atom, the key of the noise stream (seed, conformation, first_step + step, component) and the
meaning of `out_energy`, none of which the statistical tests of tests/test_md_gpu.py can see.

Force-free tables make every component a linear recursion in the noise, so the restatement needs no forces and the
agreement is limited by the final float32 rounding alone.  On the real force field the restatement takes its forces
from central differences of the C oracle's energy, and the bound is measured between two difference steps - on the
reference, not the kernel (tests/test_langevin_cpu.py)."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import langevin_oracle as lo
from tests.test_langevin_cpu import FD_H, KBT, REAL_CASES, _cached_forces, real_case, restated

pytestmark = pytest.mark.gpu

GAS_CONSTANT = 8.314462618e-3
TEMPERATURE = 297.3456789        # a float64 temperature, passed through `temperature=`
FIRST_STEP = 1000003
SCHEMES = ["LangevinMiddleIntegrator", "LangevinIntegrator"]


def free_tables(V):
    """Tables whose forces vanish identically: no bonded term, no exception, zero charges and LJ depths, no GBSA."""
    from timewarp_amd.forcefield import ForceFieldTables

    z = lambda w, t=np.float64: np.zeros((0, w), dtype=t)
    atom_par = np.tile(np.array([[0.0, 0.3, 0.0, 0.15, 0.8]]), (V, 1))
    return ForceFieldTables(bond_idx=z(2, np.int32), bond_par=z(2), angle_idx=z(3, np.int32), angle_par=z(2), torsion_idx=z(4, np.int32),
                            torsion_par=z(3), exc_idx=z(2, np.int32), exc_par=z(3), atom_par=atom_par, has_gbsa=0)


_ENERGIES = {}


def free_energy(V):
    from timewarp_amd.energy import AmberPotentialEnergyTorch

    if V not in _ENERGIES:
        _ENERGIES[V] = AmberPotentialEnergyTorch(free_tables(V))
    return _ENERGIES[V]


def real_energy(mol):
    from timewarp_amd.energy import AmberPotentialEnergyTorch

    if mol not in _ENERGIES:
        _ENERGIES[mol] = AmberPotentialEnergyTorch(real_case(mol)[0])
    return _ENERGIES[mol]


def free_state(V, rows, seed=0):
    """atoms 0.5 nm apart on a cubic grid (jittered), velocities of thermal size; masses all distinct"""
    rng = np.random.default_rng(1000 * V + rows + seed)
    side = int(np.ceil(V ** (1.0 / 3.0)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:V] * 0.5
    x = (grid[None] + 0.05 * rng.standard_normal((rows, V, 3))).astype(np.float32)
    v = rng.standard_normal((rows, V, 3)).astype(np.float32)
    masses = (1.0 + 0.37 * np.arange(V)).astype(np.float32)
    return masses, x, v


def dynamics(energy, masses, dt, friction, scheme, seed, first_step=0, temperature=TEMPERATURE):
    from timewarp_amd.md import LangevinDynamics

    md = LangevinDynamics(energy, torch.from_numpy(np.asarray(masses)), timestep_ps=dt, friction_per_ps=friction, integrator=SCHEMES[scheme],
                          seed=seed, temperature=temperature)
    md.steps_done = first_step
    return md


def device_steps(md, x, v, n_steps, want_energy=False):
    out = md.step(torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda(), n_steps, want_energy=want_energy)
    return tuple(o.cpu().numpy() for o in out)


def worst_in_ulps(got, want, floor=1e-12):
    """max of (|got - want| - floor) / ulp32(want): <= 1 is the force-free tolerance |got - want| <= spacing(float32(want)) + 1e-12 -
    one float32 ulp for the device / numpy log, cos and exp differing in the last double bit, plus an absolute floor where x
    cancels to near zero"""
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return float(((np.abs(got.astype(np.float64) - want.astype(np.float64)) - floor) / ulp).max())


def free_cases():
    cases = [(V, 3, 2, 50.0, 0.0005) for V in (1, 2, 22, 63, 64, 65, 128, 691)]
    cases += [(V, rows, steps, 0.3, 0.0005) for V in (22, 65) for rows in (1, 3, 257) for steps in (1, 2, 37)]
    cases += [(V, 3, 2, friction, dt) for V in (22, 65) for friction in (0.3, 50.0, 4.0e4) for dt in (0.0005, 0.001)]
    cases += [(691, 257, 37, 50.0, 0.001), (64, 257, 37, 4.0e4, 0.0005), (1, 257, 37, 0.3, 0.001), (128, 257, 2, 4.0e4, 0.001),
              (63, 257, 1, 4.0e4, 0.0005), (691, 1, 1, 4.0e4, 0.0005), (2, 3, 37, 50.0, 0.001)]
    return list(dict.fromkeys(cases))


# ---------------------------------------------------------------------------------------------
# force-free tables
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 2, 22, 63, 64, 65, 128, 691])
def test_force_kernel_returns_exactly_zero_on_force_free_tables(V):
    """Empty term lists run (the loops of tw_md.hip and tw_energy.hip are guarded by their counts), and energy and forces
    are exactly 0."""
    _, x, _ = free_state(V, 3)
    e, f = free_energy(V).energy_and_forces(torch.from_numpy(x).cuda())
    assert e.shape == (3,) and f.shape == (3, V, 3)
    assert torch.count_nonzero(e) == 0 and torch.count_nonzero(f) == 0
    e2, _ = free_energy(V).energy_and_terms(torch.from_numpy(x).cuda())
    assert torch.count_nonzero(e2) == 0


@pytest.mark.parametrize("scheme", [0, 1])
def test_force_free_trajectories_match_the_restatement_to_one_float32_ulp(scheme):
    """Every size (one wave up to 64 atoms, sixteen above; 691 atoms need the 160 KiB LDS opt-in), 1 / 3 / 257 rows,
    1 / 2 / 37 steps, friction 0.3 / 50 / 4e4 per ps at 0.5 and 1 fs (at 4e4 / ps a ~ 2e-9: the velocity that comes back IS the
    scaled noise - the bit-level check of md_normal on the device), distinct masses, a non-zero first step, a float64
    temperature."""
    kbT = GAS_CONSTANT * TEMPERATURE
    report = []
    for V, rows, steps, friction, dt in free_cases():
        masses, x, v = free_state(V, rows)
        seed = 0x9E3779B97F4A7C15 ^ (V * 7919 + rows)      # a seed with its top bit set
        md = dynamics(free_energy(V), masses, dt, friction, scheme, seed, FIRST_STEP)
        gx, gv, ge = device_steps(md, x, v, steps, want_energy=True)
        wx, wv, _ = lo.langevin_steps(lo.no_forces, masses, x, v, steps, dt, friction, kbT, scheme, seed, FIRST_STEP)
        report.append((worst_in_ulps(gx, wx), worst_in_ulps(gv, wv), V, rows, steps, friction, dt))
        assert md.steps_done == FIRST_STEP + steps and np.count_nonzero(ge) == 0
        assert np.abs(gv - v).max() > 1e-3      # the thermostat acted
    print(f"scheme {scheme}: {len(report)} force-free cases, worst distance in float32 ulps: x {max(r[0] for r in report):.3f}, "
          f"v {max(r[1] for r in report):.3f}")
    bad = [r for r in report if max(r[:2]) > 1.0]
    assert not bad, bad


@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("V", [22, 65])
def test_steps_done_advances_the_key(scheme, V):
    """step(x, v, 3) then step(., ., 2): the second call is the restatement started at step 3 from what the first returned;
    one call of 5 agrees within two ulp - one of the result, one where the hand-off rounds to float32 once more."""
    kbT = GAS_CONSTANT * TEMPERATURE
    masses, x, v = free_state(V, 3, seed=1)
    md = dynamics(free_energy(V), masses, 0.0005, 50.0, scheme, 77, FIRST_STEP)
    ax, av = device_steps(md, x, v, 3)
    bx, bv = device_steps(md, ax, av, 2)
    w3 = lo.langevin_steps(lo.no_forces, masses, x, v, 3, 0.0005, 50.0, kbT, scheme, 77, FIRST_STEP)
    w2 = lo.langevin_steps(lo.no_forces, masses, ax, av, 2, 0.0005, 50.0, kbT, scheme, 77, FIRST_STEP + 3)
    w5 = lo.langevin_steps(lo.no_forces, masses, x, v, 5, 0.0005, 50.0, kbT, scheme, 77, FIRST_STEP)
    assert max(worst_in_ulps(ax, w3[0]), worst_in_ulps(av, w3[1])) <= 1.0
    assert max(worst_in_ulps(bx, w2[0]), worst_in_ulps(bv, w2[1])) <= 1.0
    # "two ulp", each where its rounding happens: one of the result (as above), and the half ulp of the float32 hand-off of x and
    # v after step 3, which reaches the result with a coefficient <= 1 (v: a^2; x: 1, and 2 dt for the hand-off's v)
    ulp = lambda t: np.spacing(np.abs(t).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(bv.astype(np.float64) - w5[1]) <= ulp(w5[1]) + 0.5 * ulp(av) + 1e-12)
    assert np.all(np.abs(bx.astype(np.float64) - w5[0]) <= ulp(w5[0]) + 0.5 * ulp(ax) + 0.0005 * ulp(av) + 1e-12)
    # a second call that started the key at FIRST_STEP again would be far off
    stale = lo.langevin_steps(lo.no_forces, masses, ax, av, 2, 0.0005, 50.0, kbT, scheme, 77, FIRST_STEP)
    assert worst_in_ulps(bv, stale[1]) > 100.0


@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("V", [22, 65])
def test_a_row_does_not_depend_on_its_neighbours(scheme, V):
    """Row r of a 257-row call is the restatement of that row alone as conformation r, and is not what the device gives
    the same state as row 0 of a call of its own."""
    kbT = GAS_CONSTANT * TEMPERATURE
    masses, x, v = free_state(V, 257, seed=2)
    gx, gv = device_steps(dynamics(free_energy(V), masses, 0.001, 50.0, scheme, 31, FIRST_STEP), x, v, 4)
    for r in (0, 1, 100, 256):
        wx, wv, _ = lo.langevin_steps(lo.no_forces, masses, x[r:r + 1], v[r:r + 1], 4, 0.001, 50.0, kbT, scheme, 31, FIRST_STEP, conformations=[r])
        assert max(worst_in_ulps(gx[r:r + 1], wx), worst_in_ulps(gv[r:r + 1], wv)) <= 1.0, r
    ox, ov = device_steps(dynamics(free_energy(V), masses, 0.001, 50.0, scheme, 31, FIRST_STEP), x[100:101], v[100:101], 4)
    assert worst_in_ulps(ov, gv[100:101]) > 100.0
    ox, ov = device_steps(dynamics(free_energy(V), masses, 0.001, 50.0, scheme, 31, FIRST_STEP), x[:1], v[:1], 4)
    assert np.array_equal(ox, gx[:1]) and np.array_equal(ov, gv[:1])


@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("V", [22, 65])
@pytest.mark.parametrize("first_step", [2 ** 32 + 3, 2 ** 31 - 1])
def test_the_step_enters_the_key_as_64_bits(scheme, V, first_step):
    """include/timewarp_hip.h: `int64_t first_step`, a stream keyed on first_step + step.  2^32 + 3 is not step 3 again, and
    three steps from 2^31 - 1 cross the sign change of a 32-bit step.  (Below 2^31 a 32-bit and a 64-bit step are the same
    key: no earlier stream moves.)"""
    kbT = GAS_CONSTANT * TEMPERATURE
    masses, x, v = free_state(V, 3, seed=3)
    gx, gv = device_steps(dynamics(free_energy(V), masses, 0.0005, 50.0, scheme, 5, first_step), x, v, 3)
    wx, wv, _ = lo.langevin_steps(lo.no_forces, masses, x, v, 3, 0.0005, 50.0, kbT, scheme, 5, first_step)
    print(f"first_step {first_step}: distance to the restatement x {worst_in_ulps(gx, wx):.3g} ulp, v {worst_in_ulps(gv, wv):.3g} ulp")
    if first_step >= 2 ** 32:
        dx, dv = device_steps(dynamics(free_energy(V), masses, 0.0005, 50.0, scheme, 5, first_step % 2 ** 32), x, v, 3)
        assert not np.array_equal(gv, dv), "the device replays the noise of first_step mod 2^32"
    assert max(worst_in_ulps(gx, wx), worst_in_ulps(gv, wv)) <= 1.0


# ---------------------------------------------------------------------------------------------
# deliberately wrong restatements: the comparisons are not vacuous
# ---------------------------------------------------------------------------------------------
def mutant_steps(mutant, force_fn, masses, x, v, n_steps, dt, friction, kbT, scheme, seed, first_step):
    """`langevin_oracle.langevin_steps` with one slip each.  These live here, never in the library."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    n, V, _ = x.shape
    m = np.asarray(masses, dtype=np.float32).astype(np.float64)
    if mutant == "mass of atom i % 64":
        m = m[np.arange(V) % 64]
    m = m.reshape(1, V, 1)
    conf = np.arange(n).reshape(n, 1, 1) * (0 if mutant == "key without the conformation" else 1)
    comp = np.arange(3 * V).reshape(1, V, 3)
    a = np.exp(-friction * dt)
    fscale = dt if mutant == "dt for (1 - a) / friction" else (1.0 - a) / friction
    sigma = np.sqrt((1.0 - a) if mutant == "noise scale sqrt(1 - a)" else (1.0 - a * a)) * np.sqrt(kbT / m)
    for s in range(n_steps):
        _, f = force_fn(x)
        kick = sigma * lo.md_normal(seed, conf, first_step + s, comp)
        if scheme == 0 and mutant == "kick after the half drift":
            x = x + 0.5 * dt * v
            v = v + dt * f / m
            v = a * v + kick
            x = x + 0.5 * dt * v
        elif scheme == 0:
            v = v + dt * f / m
            x = x + 0.5 * dt * v
            v = a * v + kick
            x = x + 0.5 * dt * v
        else:
            v = a * v + fscale * f / m + kick
            x = x + dt * v
    return x.astype(np.float32), v.astype(np.float32)


@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("mutant", ["noise scale sqrt(1 - a)", "mass of atom i % 64", "key without the conformation"])
def test_wrong_noise_restatements_miss_by_a_hundred_tolerances(mutant, scheme):
    """Force-free, 128 atoms (sixteen waves), 3 rows, 2 steps at friction 50 / ps: the kernel is within one ulp of the
    restatement and at least 100 ulp from each slip in the noise term."""
    kbT = GAS_CONSTANT * TEMPERATURE
    V, rows, steps, friction, dt = 128, 3, 2, 50.0, 0.0005
    masses, x, v = free_state(V, rows)
    gx, gv = device_steps(dynamics(free_energy(V), masses, dt, friction, scheme, 41, FIRST_STEP), x, v, steps)
    wx, wv, _ = lo.langevin_steps(lo.no_forces, masses, x, v, steps, dt, friction, kbT, scheme, 41, FIRST_STEP)
    same = mutant_steps(None, lo.no_forces, masses, x, v, steps, dt, friction, kbT, scheme, 41, FIRST_STEP)
    assert np.array_equal(same[0], wx) and np.array_equal(same[1], wv)     # without a slip the mutant code IS the restatement
    mx, mv = mutant_steps(mutant, lo.no_forces, masses, x, v, steps, dt, friction, kbT, scheme, 41, FIRST_STEP)
    assert max(worst_in_ulps(gx, wx), worst_in_ulps(gv, wv)) <= 1.0
    miss = worst_in_ulps(gv, mv)
    print(f"{mutant}, scheme {scheme}: the kernel misses it by {miss:.3g} ulp")
    assert miss >= 100.0


@pytest.mark.parametrize("mutant,scheme", [("kick after the half drift", 0), ("dt for (1 - a) / friction", 1)])
def test_wrong_force_restatements_miss_by_a_hundred_tolerances(mutant, scheme):
    """The two slips that need forces to show, on alanine dipeptide at friction 50 / ps: the velocity kick after the half drift in
    LangevinMiddle (the positions move by dt^2 F / 2m), and dt where (1 - a) / friction belongs in Langevin (1.2 % of the force
    term there; 7.5e-5 of it at the preset's 0.3 / ps).  The kernel is at least 100 bounds away from each."""
    r = restated("ad", scheme, 50.0)
    tables, masses, x0, v0 = real_case("ad")
    md = dynamics(real_energy("ad"), masses, 0.0005, 50.0, scheme, r.seed, r.first_step, temperature=310.0)
    gx, gv = device_steps(md, x0, v0, r.steps)
    fn = _cached_forces("ad", FD_H / 2)
    same = mutant_steps(None, fn, masses, x0, v0, r.steps, 0.0005, 50.0, KBT, scheme, r.seed, r.first_step)
    assert np.array_equal(same[0], r.fine[0]) and np.array_equal(same[1], r.fine[1])
    mx, mv = mutant_steps(mutant, fn, masses, x0, v0, r.steps, 0.0005, 50.0, KBT, scheme, r.seed, r.first_step)
    bx, bv = r.bounds()
    miss = max((np.abs(gx.astype(np.float64) - mx) / bx).max(), (np.abs(gv.astype(np.float64) - mv) / bv).max())
    print(f"{mutant}: the kernel misses it by {miss:.3g} bounds")
    assert miss >= 100.0


# ---------------------------------------------------------------------------------------------
# the real force field
# ---------------------------------------------------------------------------------------------
def _compare(r, mol, scheme, friction):
    tables, masses, x0, v0 = real_case(mol)
    md = dynamics(real_energy(mol), masses, 0.0005, friction, scheme, r.seed, r.first_step, temperature=310.0)
    gx, gv, ge = device_steps(md, x0, v0, r.steps, want_energy=True)
    bx, bv = r.bounds()
    ex, ev = np.abs(gx.astype(np.float64) - r.fine[0]), np.abs(gv.astype(np.float64) - r.fine[1])
    de = np.abs(ge - r.fine[2]) / np.abs(r.fine[2])
    e_out, _ = H.oracle_energy(tables, r.fine[0].astype(np.float64), dtype=np.float64)
    print(f"{mol} scheme {scheme} friction {friction}: u_x {r.u_x:.3e} u_v {r.u_v:.3e}; kernel to out(h/2): x {ex[r.keep].max():.3e} nm "
          f"({(ex / bx)[r.keep].max():.2f} of the bound), v {ev[r.keep].max():.3e} nm/ps ({(ev / bv)[r.keep].max():.2f} of the bound); "
          f"energy {de.max():.2e} of |E|; left out {100 * r.left_out:.2f} %")
    assert r.left_out <= 0.05
    assert np.all(ex[r.keep] <= bx[r.keep]) and np.all(ev[r.keep] <= bv[r.keep])
    assert de.max() < 1e-6
    assert (np.abs(ge - e_out) / np.abs(e_out)).max() > 100 * 1e-6     # (a single row may sit at a turning point of its energy)


@pytest.mark.parametrize("mol,scheme,friction", REAL_CASES)
def test_real_force_field_steps_match_the_restatement(mol, scheme, friction):
    """Alanine dipeptide (22 atoms, one wave) and NNQQ (65, sixteen waves): 8 rows, 10 steps, both schemes at 0.3 and 50 / ps;
    the 691-atom protein: 2 rows, 2 steps, LangevinMiddle at 0.3 / ps and Langevin at 50 / ps (the other two combinations are
    dropped there: one step is 4146 oracle energies per row).  Thermal velocities, dt 0.5 fs, 310 K.

    Bound: the kernel within 4 u + 1 ulp32 of out(h / 2), u = max |out(h) - out(h / 2)| of the restatement with central
    differences of step h = 1e-5 nm (tests/test_langevin_cpu.py measures u and checks its conditions without a GPU).
    `want_energy`: the C oracle's energy at the restated positions BEFORE the last update, to 1e-6 of |E| (the bar of
    test_hip_kernels_on_segments_of_the_protein); the energy at the returned positions is more than 100 times that away.

    Measured (u from the restatement alone; then the kernel's largest distance from out(h / 2), in nm and nm/ps):
      every case: u_x 1.2e-10 .. 6.0e-8 nm, u_v 2.4e-7 or 4.8e-7 nm/ps (one or two float32 ulp of the results: the finite differences
      themselves agree below the output rounding)
      alanine dipeptide  x <= 3.0e-8 (0.20 of the bound), v 2.4e-7 (0.20);  energy 1.4e-8 of |E|
      NNQQ               x <= 6.0e-8 (0.67 of the bound), v 2.4e-7 (0.20);  energy 6.2e-10 of |E|
      1hgv               x <= 2.7e-12 (0.01 of the bound), v 4.8e-7 (0.20); energy 5.0e-11 of |E|; 1.2 % / 1.9 % of the components left out
      friction 0 (test_friction_zero_through_the_restatement): x 3.0e-8 (0.11), v 2.4e-7 (0.11)"""
    _compare(restated(mol, scheme, friction), mol, scheme, friction)


@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("mol", ["ad", "nnqq"])
def test_friction_zero_through_the_restatement(mol, scheme):
    """The no-noise leapfrog of either scheme, 10 steps, same bound (u measured for this run)."""
    r = restated(mol, scheme, 0.0)
    _compare(r, mol, scheme, 0.0)
    other = restated(mol, 1 - scheme, 0.0)      # both schemes are the same leapfrog then
    bx, bv = r.bounds()
    assert np.all(np.abs(other.fine[0].astype(np.float64) - r.fine[0]) <= bx) and np.all(np.abs(other.fine[1].astype(np.float64) - r.fine[1]) <= bv)
