"""Hydrogen-bond constraints on the device (csrc/tw_md.hip `langevin_constrained_kernel<W>` behind
`tw_langevin_trajectory_constrained`, `apply_constraints_kernel` behind `tw_apply_constraints`, `LangevinDynamics(constraints=)`,
`simulate_trajectory(constraints=)`) against the float64 restatement tests/constraint_oracle.py, whose own errors - the
finite-difference error u, the tolerance error u_tol, the temperature of force-free stars - tests/test_md_constraints_cpu.py
measures without a GPU.  Every test goes through one of the new entry points or the `constraints=` argument."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import constraint_oracle as co
from tests.test_langevin_cpu import FD_H, KBT, REAL_CASES, _cached_forces, real_case
from tests.test_langevin_gpu import free_energy, real_energy, worst_in_ulps
from tests.test_md_checkpoint_cpu import same_files, same_rows
from tests.test_md_constraints_cpu import (DT, STAR_FIRST_STEP, STAR_SEED, STAR_T_FRICTION, STAR_T_ROWS, STAR_T_STEPS, SWEEPS, TOL,
                                           constrained_case, crestated, oracle_energy_excursion, star_case, star_temperature,
                                           star_tolerance_error, total_energy, AD_EXCURSION_2FS)
from timewarp_amd import simulation as S
from timewarp_amd.forcefield import HBondConstraints, hbond_constraints

pytestmark = pytest.mark.gpu
SCHEMES = ["LangevinMiddleIntegrator", "LangevinIntegrator"]


def dynamics(energy, masses, dt, friction, scheme, seed, first_step=0, constraints=None, temperature=310.0):
    from timewarp_amd.md import LangevinDynamics

    md = LangevinDynamics(energy, torch.from_numpy(np.asarray(masses)), timestep_ps=dt, friction_per_ps=friction, integrator=SCHEMES[scheme],
                          seed=seed, temperature=temperature, constraints=constraints)
    md.steps_done = first_step
    return md


def no_clusters(V):
    return HBondConstraints(np.zeros((0, 4), dtype=np.int32), np.zeros((0, 3)), V)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---------------------------------------------------------------------------------------------
# zero clusters: the new entry point IS tw_langevin_trajectory_opts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("mol", ["ad", "nnqq"])
def test_zero_clusters_equal_the_unconstrained_kernel_bit_for_bit(mol, scheme):
    """Alanine dipeptide (one wave) and NNQQ (sixteen waves): frames, returned state and state64 of 9 steps at friction 0.3 / ps,
    and of friction 0."""
    _, masses, x0, v0 = real_case(mol)
    V = x0.shape[1]
    for friction in (0.3, 0.0):
        outs = []
        for cons in (None, no_clusters(V)):
            md = dynamics(real_energy(mol), masses, 0.0005, friction, scheme, 77, 1000, constraints=cons)
            state = md.new_state(cuda(x0[:4]), cuda(v0[:4]))
            x, v, f = md.trajectory(None, None, [0, 1, 4, 9], num_steps=9, state=state)
            outs.append((x, v, state, f.positions, f.velocities, f.forces, f.energies))
            if cons is not None:
                assert md.constraint_residual.abs().max().item() == 0.0 and md.constraint_sweeps.abs().max().item() == 0
        assert all(same_bits(a, b) for a, b in zip(*outs)), (mol, scheme, friction)
        assert not torch.equal(outs[0][3][:, 0], outs[0][3][:, -1])
    # and through `step`: the float32 hand-off of tw_langevin_steps
    a = dynamics(real_energy(mol), masses, 0.0005, 0.3, scheme, 77, 5).step(cuda(x0[:4]), cuda(v0[:4]), 6)
    b = dynamics(real_energy(mol), masses, 0.0005, 0.3, scheme, 77, 5, constraints=no_clusters(V)).step(cuda(x0[:4]), cuda(v0[:4]), 6)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


# ---------------------------------------------------------------------------------------------
# force-free stars
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("V", [2, 3, 4, 64, 68])
def test_force_free_stars_match_the_restatement(V, scheme):
    """One cluster of 1, 2, 3 hydrogens; 16 stars (one wave, full); 17 stars on sixteen waves.  1 / 3 / 257 rows, 1 and 37 steps of
    2 fs, friction 0 and 1 / ps, tolerance 1e-10, distinct masses and lengths.  Bound: one float32 ulp (the final rounding) plus
    u_tol, what the restatement itself moves by between tolerance 1e-10 and 1e-13 - a sweep more or less at the threshold."""
    report = []
    for rows in (1, 3, 257):
        masses, atoms, lengths, x, v = star_case(V, rows)
        cons = HBondConstraints(atoms, lengths, V, TOL, SWEEPS)
        for steps in (1, 37):
            for friction in (0.0, 1.0):
                md = dynamics(free_energy(V), masses, DT, friction, scheme, STAR_SEED, STAR_FIRST_STEP, constraints=cons)
                gx, gv = (t.cpu().numpy() for t in md.step(cuda(x), cuda(v), steps))
                ux, uv, want = star_tolerance_error(V, rows, steps, friction, scheme)
                wx, wv = want[0].astype(np.float32), want[1].astype(np.float32)
                sweeps, resid = md.constraint_sweeps.cpu().numpy(), md.constraint_residual.cpu().numpy()
                report.append((worst_in_ulps(gx, wx, 1e-12 + ux), worst_in_ulps(gv, wv, 1e-12 + uv), rows, steps, friction, ux, uv,
                               int(sweeps.max()), float(resid.max())))
                assert resid.max() <= TOL and np.all(sweeps >= 1) and np.all(np.abs(sweeps - want[3]) <= 1), (rows, steps, friction)
                assert np.abs(gv - v).max() > 1e-4 or friction == 0.0
                assert np.abs(gx - x).max() > 1e-4
    print(f"V {V} scheme {scheme}: worst distance in float32 ulps x {max(r[0] for r in report):.3f}, v {max(r[1] for r in report):.3f}; "
          f"u_tol x <= {max(r[5] for r in report):.2e}, v <= {max(r[6] for r in report):.2e}; sweeps <= {max(r[7] for r in report)}, "
          f"residual <= {max(r[8] for r in report):.2e}")
    bad = [r for r in report if max(r[:2]) > 1.0]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# the real force field
# ---------------------------------------------------------------------------------------------
def _device_real(mol, scheme, friction, r):
    tables, masses, atoms, lengths, x0, v0 = constrained_case(mol)
    cons = HBondConstraints(atoms, lengths, x0.shape[1], TOL, SWEEPS)
    md = dynamics(real_energy(mol), masses, DT, friction, scheme, r.seed, r.first_step, constraints=cons)
    gx, gv = (t.cpu().numpy() for t in md.step(cuda(x0), cuda(v0), r.steps))
    return gx, gv, md


@pytest.mark.parametrize("mol,scheme,friction", REAL_CASES)
def test_real_force_field_steps_match_the_constrained_restatement(mol, scheme, friction):
    """The cases of tests/test_langevin_gpu.py at 2 fs with the X-H bonds constrained (tolerance 1e-10): alanine dipeptide and NNQQ
    8 rows x 10 steps, both schemes, friction 0.3 and 50 / ps; the protein 2 rows x 2 steps, the diagonal.  Bound: 4 u + 1 ulp32 of
    the restatement with central-difference forces (u: tests/test_md_constraints_cpu.py)."""
    r = crestated(mol, scheme, friction)
    gx, gv, md = _device_real(mol, scheme, friction, r)
    bx, bv = r.bounds()
    ex, ev = np.abs(gx.astype(np.float64) - r.fine[0]), np.abs(gv.astype(np.float64) - r.fine[1])
    print(f"{mol} scheme {scheme} friction {friction}: u_x {r.u_x:.3e} u_v {r.u_v:.3e}; kernel to out(h/2): x {ex[r.keep].max():.3e} nm "
          f"({(ex / bx)[r.keep].max():.2f} of the bound), v {ev[r.keep].max():.3e} nm/ps ({(ev / bv)[r.keep].max():.2f} of the bound); "
          f"sweeps {int(md.constraint_sweeps.max())} (restatement {r.sweeps}), residual {float(md.constraint_residual.max()):.2e}")
    assert r.left_out <= 0.05
    assert np.all(ex[r.keep] <= bx[r.keep]) and np.all(ev[r.keep] <= bv[r.keep])
    assert float(md.constraint_residual.max()) <= TOL and int(md.constraint_sweeps.max()) <= 16


@pytest.mark.parametrize("wrong,scheme", [("no_velocity_projection", 0), ("no_inverse_dt", 0), ("reference_from_new", 1), ("masses_swapped", 1)])
def test_wrong_restatements_miss_by_a_hundred_bounds(wrong, scheme):
    """Alanine dipeptide at friction 0.3 / ps: the kernel is at least 100 bounds away from each of four slips - no velocity
    projection (LangevinMiddle only has one), the velocity correction without 1 / dt, reference vectors from the new positions,
    centre and hydrogen masses exchanged."""
    r = crestated("ad", scheme, 0.3)
    gx, gv, _ = _device_real("ad", scheme, 0.3, r)
    mx, mv, _, _, _ = co.constrained_steps(_cached_forces("ad", FD_H / 2), *r.args, TOL, SWEEPS, wrong=wrong)
    bx, bv = r.bounds()
    miss = max((np.abs(gx.astype(np.float64) - mx) / bx).max(), (np.abs(gv.astype(np.float64) - mv) / bv).max())
    print(f"{wrong}, scheme {scheme}: the kernel misses it by {miss:.3g} bounds")
    assert miss >= 100.0
    same = co.constrained_steps(_cached_forces("ad", FD_H / 2), *r.args, TOL, SWEEPS)
    assert np.array_equal(same[0], r.fine[0]) and np.array_equal(same[1], r.fine[1])


# ---------------------------------------------------------------------------------------------
# the constraints hold
# ---------------------------------------------------------------------------------------------
def _bond_errors(x, atoms, lengths):
    """relative errors of the squared lengths, [N, ..., constraints]"""
    cl = co.Clusters(atoms, lengths, np.ones(int(atoms.max()) + 1))
    d2 = ((x[..., cl.c, None, :] - x[..., cl.h, :]) ** 2).sum(-1)
    return (np.abs(d2 - cl.d2) / np.where(cl.used, cl.d2, 1.0))[..., cl.used]


def test_constraints_hold_over_two_hundred_steps():
    """Alanine dipeptide, 64 rows, 200 steps of 2 fs at 1 / ps, a frame every step."""
    tables, masses, atoms, lengths, x0, v0 = constrained_case("ad")
    cons = HBondConstraints(atoms, lengths, 22, TOL, SWEEPS)
    md = dynamics(real_energy("ad"), masses, DT, 1.0, 0, 3, 0, constraints=cons)
    state = md.new_state(cuda(np.tile(x0, (8, 1, 1))), cuda(np.tile(v0, (8, 1, 1))))
    md.apply_constraints(None, state=state)
    _, _, f = md.trajectory(None, None, np.arange(1, 201), num_steps=200, state=state)
    resid, sweeps = md.constraint_residual.cpu().numpy(), md.constraint_sweeps.cpu().numpy()
    print(f"64 rows x 200 steps: residual <= {resid.max():.2e}, sweeps {sweeps.min()} .. {sweeps.max()}")
    assert resid.shape == (64,) and resid.max() <= TOL and resid.min() > 0.0 and 1 <= sweeps.min() and sweeps.max() <= 16
    final = state[:, 0].cpu().numpy()
    assert _bond_errors(final, atoms, lengths).max() <= TOL
    pos = f.positions.cpu().numpy().astype(np.float64)
    assert np.isfinite(pos).all() and np.abs(pos[:, -1] - pos[:, 0]).max() > 0.01
    # float32 frames: each coordinate is off by at most half an ulp of max |x|; a squared length by 4 eps32 max|x| / d relatively
    bound = 4.0 * np.finfo(np.float32).eps * np.abs(pos).max() / lengths[lengths > 0].min()
    assert _bond_errors(pos, atoms, lengths).max() <= bound
    # unconstrained, the same run stretches its X-H bonds by far more
    free = dynamics(real_energy("ad"), masses, DT / 4, 1.0, 0, 3, 0)
    fx, _ = free.step(cuda(x0), cuda(v0), 40)
    assert _bond_errors(fx.cpu().numpy().astype(np.float64), atoms, lengths).max() > 1e4 * bound


def test_apply_constraints_projects_a_state_that_is_off():
    tables, masses, atoms, lengths, x0, v0 = constrained_case("nnqq")
    V = x0.shape[1]
    cons = HBondConstraints(atoms, lengths, V, TOL, SWEEPS)
    md = dynamics(real_energy("nnqq"), masses, DT, 1.0, 0, 3, 0, constraints=cons)
    rng = np.random.default_rng(5)
    cl = co.Clusters(atoms, lengths, masses)
    x = x0.astype(np.float64)
    hyd = cl.h[cl.used]
    x[:, hyd] += 0.02 * (x[:, hyd] - x[:, np.repeat(cl.c, cl.used.sum(1))]) * rng.uniform(-1, 1, (x.shape[0], hyd.size, 1))
    v = v0.astype(np.float64) + rng.standard_normal(v0.shape)
    assert _bond_errors(x, atoms, lengths).max() > 1e-2
    state = torch.stack([cuda(x), cuda(v)], dim=1).contiguous()
    before = state.clone()
    x32, v32 = md.apply_constraints(None, state=state)
    got = state.cpu().numpy()
    wx, wv, wres = co.apply_constraints(cl, x, v, TOL, SWEEPS)
    assert _bond_errors(got[:, 0], atoms, lengths).max() <= TOL and float(md.constraint_residual.max()) <= TOL
    assert np.abs(got[:, 0] - wx).max() <= 1e-11 and np.abs(got[:, 1] - wv).max() <= 1e-11 * np.abs(wv).max() + 1e-12
    outside = np.setdiff1d(np.arange(V), co.cluster_atoms(cl))
    assert outside.size > 0 and torch.equal(state[:, :, outside], before[:, :, outside])
    assert torch.equal(x32, state[:, 0].float()) and torch.equal(v32, state[:, 1].float())
    rel = ((got[:, 1][:, cl.c][:, :, None] - got[:, 1][:, cl.h]) * co.refvec(cl, got[:, 0])).sum(-1)
    assert np.abs(rel[:, cl.used]).max() <= 1e-12
    # float32 arrays: the casts of the same projection; velocities optional
    cx, cv = md.apply_constraints(cuda(x.astype(np.float32)), cuda(v.astype(np.float32)))
    wx32, wv32, _ = co.apply_constraints(cl, x.astype(np.float32).astype(np.float64), v.astype(np.float32).astype(np.float64), TOL, SWEEPS)
    assert worst_in_ulps(cx.cpu().numpy(), wx32.astype(np.float32)) <= 1.0 and worst_in_ulps(cv.cpu().numpy(), wv32.astype(np.float32)) <= 1.0
    only_x, none = md.apply_constraints(cuda(x.astype(np.float32)))
    assert none is None and torch.equal(only_x, cx)
    with pytest.raises(ValueError, match="no constraints"):
        dynamics(real_energy("nnqq"), masses, DT, 1.0, 0, 3).apply_constraints(cuda(x.astype(np.float32)))


# ---------------------------------------------------------------------------------------------
# cuts, rows, checkpoints
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("mol", ["ad", "nnqq"])
def test_cutting_a_constrained_run_changes_no_bit(mol, scheme):
    """40 steps in one launch against 7 + 13 + 20 with the fp64 carry: frames and state bit for bit."""
    tables, masses, atoms, lengths, x0, v0 = constrained_case(mol)
    cons = HBondConstraints(atoms, lengths, x0.shape[1], TOL, SWEEPS)
    reports = np.array([0, 3, 7, 8, 19, 20, 33, 40])
    one = dynamics(real_energy(mol), masses, DT, 0.3, scheme, 9, 100, constraints=cons)
    s1 = one.new_state(cuda(x0[:3]), cuda(v0[:3]))
    _, _, f1 = one.trajectory(None, None, reports, num_steps=40, state=s1)
    cut = dynamics(real_energy(mol), masses, DT, 0.3, scheme, 9, 100, constraints=cons)
    s2 = cut.new_state(cuda(x0[:3]), cuda(v0[:3]))
    parts, at, worst = [], 0, 0.0
    for n in (7, 13, 20):
        lower = reports > at if at else reports >= 0      # step `at` itself was the last frame of the launch before
        mine = reports[lower & (reports <= at + n)] - at
        _, _, f = cut.trajectory(None, None, mine, num_steps=n, state=s2)
        parts.append(f)
        at += n
        worst = max(worst, float(cut.constraint_residual.max()))
    assert same_bits(s1, s2) and cut.steps_done == one.steps_done == 140
    for key in ("positions", "velocities", "forces", "energies"):
        assert same_bits(getattr(f1, key), torch.cat([getattr(p, key) for p in parts], dim=1)), key
    assert float(one.constraint_residual.max()) == worst <= TOL


def test_a_constrained_row_does_not_depend_on_its_neighbours():
    tables, masses, atoms, lengths, x0, v0 = constrained_case("ad")
    cons = HBondConstraints(atoms, lengths, 22, TOL, SWEEPS)
    x, v = np.tile(x0, (33, 1, 1))[:257], np.tile(v0, (33, 1, 1))[:257]
    many = dynamics(real_energy("ad"), masses, DT, 0.3, 0, 9, 100, constraints=cons).step(cuda(x), cuda(v), 10)
    alone = dynamics(real_energy("ad"), masses, DT, 0.3, 0, 9, 100, constraints=cons).step(cuda(x[:1]), cuda(v[:1]), 10)
    assert same_bits(many[0][:1], alone[0]) and same_bits(many[1][:1], alone[1])
    assert not torch.equal(many[1][0], many[1][8])      # the same start as row 0, another row of the noise key


def test_a_constrained_run_resumes_bit_for_bit(tmp_path):
    from timewarp_amd.md import LangevinDynamics

    _, masses, x0, v0 = real_case("ad")
    energy = real_energy("ad")

    def run(out, **kw):
        md = LangevinDynamics(energy, torch.from_numpy(masses), DT, 0.3, "LangevinMiddleIntegrator", seed=11, constraints="h-bonds",
                              constraint_tolerance=TOL)
        return S.simulate_trajectory(energy, torch.from_numpy(masses), cuda(x0[:2]), None, burn_in=6, sampling=24, spacing=S.LogarithmicSpacing(10, 3),
                                     integrator=md, out_dir=str(out), name="ad", seed=4, redraw_velocities=True, **kw)

    want = run(tmp_path / "a", steps_per_launch=7)
    base = str(tmp_path / "ck" / "ad")
    assert run(tmp_path / "b", steps_per_launch=7, checkpoint=base, max_steps=4) is None
    ck = S.read_checkpoint(S.checkpoint_path(base))
    assert ck["fingerprint"]["constraints"]["tolerance"] == TOL and ck["steps_done"] == 4
    assert run(tmp_path / "b", steps_per_launch=5, checkpoint=base, max_steps=13, segment_frames=2) is None
    got = run(tmp_path / "b", steps_per_launch=5, checkpoint=base, segment_frames=3)
    assert same_rows(got, want) and same_files(tmp_path / "a", tmp_path / "b")
    cons = hbond_constraints(energy.tables, masses)
    assert _bond_errors(want[0]["positions"].astype(np.float64), cons.atoms, cons.lengths).max() <= 1e-5
    with pytest.raises(ValueError, match="`constraints`"):
        S.simulate_trajectory(energy, torch.from_numpy(masses), cuda(x0[:2]), None, burn_in=6, sampling=24, spacing=S.LogarithmicSpacing(10, 3),
                              integrator=LangevinDynamics(energy, torch.from_numpy(masses), DT, 0.3, "LangevinMiddleIntegrator", seed=11),
                              out_dir=str(tmp_path / "c"), name="ad", seed=4, redraw_velocities=True,
                              checkpoint=_leave_a_checkpoint(run, tmp_path))


def test_the_command_line_runs_a_constrained_trajectory(tmp_path, capsys):
    """`--constraints h-bonds --timestep-fs 2 --minimize --redraw-velocities`: the minimised start is projected, the frames hold the
    X-H lengths to float32 rounding and the time axis is in steps of 2 fs; without the flags the same command leaves them free."""
    tables, masses, _, _ = real_case("ad")
    cons = hbond_constraints(tables, masses)
    common = ["--burn-in", "20", "--sampling", "60", "--spacing", "20", "--spacing-approach", "regular", "--seed", "3"]
    assert S.main(common + ["--out", str(tmp_path / "c"), "--constraints", "h-bonds", "--timestep-fs", "2", "--constraint-tolerance", "1e-10",
                            "--minimize", "--redraw-velocities"]) == 0
    assert S.main(common + ["--out", str(tmp_path / "f")]) == 0
    capsys.readouterr()
    c = np.load(tmp_path / "c" / "alanine-dipeptide-traj-arrays.npz")
    f = np.load(tmp_path / "f" / "alanine-dipeptide-traj-arrays.npz")
    assert c["step"].tolist() == f["step"].tolist() == [40, 60, 80]
    assert np.allclose(c["time"], c["step"] * 0.002) and np.allclose(f["time"], f["step"] * 0.0005)
    bound = 4.0 * np.finfo(np.float32).eps * np.abs(c["positions"]).max() / cons.lengths[cons.lengths > 0].min()
    assert _bond_errors(c["positions"].astype(np.float64), cons.atoms, cons.lengths).max() <= bound
    assert _bond_errors(f["positions"].astype(np.float64), cons.atoms, cons.lengths).max() > 1e3 * bound


def _leave_a_checkpoint(run, tmp_path):
    base = str(tmp_path / "ck2" / "ad")
    assert run(tmp_path / "d", steps_per_launch=7, checkpoint=base, max_steps=4) is None
    return base


# ---------------------------------------------------------------------------------------------
# physics
# ---------------------------------------------------------------------------------------------
def _device_excursion(dt, steps, every):
    tables, masses, atoms, lengths, x0, v0 = constrained_case("ad")
    cons = HBondConstraints(atoms, lengths, 22, TOL, SWEEPS)
    md = dynamics(real_energy("ad"), masses, dt, 0.0, 0, 1, 0, constraints=cons)
    state = md.new_state(cuda(x0[:1]), cuda(v0[:1]))
    _, _, f = md.trajectory(None, None, np.arange(0, steps + 1, every), num_steps=steps, state=state)
    e = total_energy(masses, atoms, lengths, f.positions[0].cpu().numpy(), f.velocities[0].cpu().numpy(), f.forces[0].cpu().numpy(),
                     f.energies[0, :, 0].cpu().numpy(), dt)
    return float(np.abs(e - e[0]).max()), float(md.constraint_residual.max())


def test_energy_is_conserved_as_well_as_the_restatement_conserves_it():
    """Friction 0, alanine dipeptide, 2 ps: the total energy (E_pot + the kinetic energy of the full-step velocities, projected;
    `total_energy`) leaves its starting value by at most twice what the float64 restatement with autograd forces shows for the same
    start (AD_EXCURSION_2FS, profiles/md_constraints.txt; the factor covers the chaotic divergence of two fp64 runs over 2 ps), and
    at 1 fs by 2.5 to 6 times less (second order: 4)."""
    ex2, res2 = _device_excursion(DT, 1000, 10)
    ex1, res1 = _device_excursion(DT / 2, 2000, 20)
    print(f"total-energy excursion over 2 ps: {ex2:.4f} kJ/mol at 2 fs (restatement {AD_EXCURSION_2FS:.4f}), {ex1:.4f} at 1 fs: ratio {ex2 / ex1:.2f}")
    assert max(res1, res2) <= TOL
    assert ex2 <= 2.0 * AD_EXCURSION_2FS
    assert 2.5 <= ex2 / ex1 <= 6.0


def test_force_free_stars_hold_their_temperature_on_the_device():
    """The run of tests/test_md_constraints_cpu.py `star_temperature` on the device: within the restatement's own deviation from the
    target plus three standard errors of the mean (from the spread of the 4096 rows' means)."""
    dev_oracle, _ = star_temperature()
    masses, atoms, lengths, x, v = star_case(4, STAR_T_ROWS)
    cons = HBondConstraints(atoms, lengths, 4, 1e-8, SWEEPS)
    md = dynamics(free_energy(4), masses, DT, STAR_T_FRICTION, 0, STAR_SEED, 0, constraints=cons, temperature=KBT / 8.314462618e-3)
    state = md.new_state(cuda(x), cuda(v))
    half = STAR_T_STEPS // 2
    md.trajectory(None, None, [], num_steps=half, state=state)
    row_sum = torch.zeros(STAR_T_ROWS, dtype=torch.float64, device="cuda")
    for _ in range(10):      # frames of steps half + 1 .. 2000: the stored velocities after every step of the second half
        _, _, f = md.trajectory(None, None, np.arange(1, half // 10 + 1), num_steps=half // 10, state=state)
        row_sum += f.energies[:, :, 1].sum(dim=1)
    t_rows = (2.0 * row_sum / half / (9.0 * KBT)).cpu().numpy()
    ratio, sem = float(t_rows.mean()), float(t_rows.std(ddof=1) / np.sqrt(STAR_T_ROWS))
    print(f"device: <T_kin> / T = {ratio:.5f} +- {sem:.5f}; the restatement deviates by {dev_oracle:.5f}")
    assert abs(ratio - 1.0) <= dev_oracle + 3.0 * sem


# ---------------------------------------------------------------------------------------------
# refusals before launch: nothing is written
# ---------------------------------------------------------------------------------------------
def test_refusals_come_before_the_launch_and_write_nothing():
    from timewarp_amd import _lib
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from tests.test_langevin_gpu import free_tables

    tables, masses, atoms, lengths, x0, v0 = constrained_case("ad")
    energy = real_energy("ad")
    lib, dev = _lib.load(), torch.device("cuda")
    ff = energy._device_ff(dev)
    good = HBondConstraints(atoms, lengths, 22, TOL, SWEEPS).to_device(dev)
    m = cuda(masses)
    x, v = cuda(x0[:2]), cuda(v0[:2])
    state = torch.stack([x, v], dim=1).double().contiguous()
    steps = torch.tensor([1, 2], dtype=torch.int32, device=dev)
    bufs = [torch.full((2, 2, 22, 3), 7.0, dtype=torch.float32, device=dev) for _ in range(3)] + [torch.full((2, 2, 2), 7.0, dtype=torch.float64, device=dev)]
    res = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    sw = torch.full((2,), 7, dtype=torch.int32, device=dev)
    everything = [x, v, state, res, sw] + bufs
    before = [t.clone() for t in everything]

    def call(flags=0, cons=good.struct, ffs=ff.struct, n_steps=2):
        rc = lib.tw_langevin_trajectory_constrained(C.byref(ffs), m.data_ptr(), x.data_ptr(), v.data_ptr(), state.data_ptr(), n_steps, DT, 0.3, KBT, 0,
                                                    5, 0, steps.data_ptr(), 2, *[b.data_ptr() for b in bufs], 2, flags, C.byref(cons),
                                                    res.data_ptr(), sw.data_ptr(), _lib.stream_ptr(dev))
        torch.cuda.synchronize()
        return rc, lib.tw_last_error().decode()

    def with_(**kw):
        s = _lib.Constraints(good.struct.n_clusters, good.struct.max_sweeps, good.struct.tolerance, good.struct.atoms, good.struct.lengths)
        for k, val in kw.items():
            setattr(s, k, val)
        return s

    refused = [(call(flags=2), "record_flags 0x2"), (call(flags=_lib.TW_RECORD_FULL_STEP_VELOCITIES), "TW_RECORD_FULL_STEP_VELOCITIES is not available with constraints"),
               (call(cons=with_(max_sweeps=0)), "max_sweeps 0"), (call(cons=with_(max_sweeps=65)), "max_sweeps 65"),
               (call(cons=with_(tolerance=0.0)), "tolerance must be finite and positive"), (call(cons=with_(tolerance=-1e-8)), "tolerance must be"),
               (call(cons=with_(tolerance=float("nan"))), "tolerance must be"), (call(cons=with_(n_clusters=-1)), "n_clusters -1"),
               (call(cons=with_(atoms=None)), "NULL pointer")]
    for (rc, msg), want in refused:
        assert rc != 0 and want in msg, (rc, msg, want)
    # 770 atoms: the unconstrained carve fits 160 KiB, the constrained kernel's (3 V doubles more) does not
    big = AmberPotentialEnergyTorch(free_tables(770))
    with pytest.raises(RuntimeError, match="constrained Langevin kernel: 770 atoms need"):
        dynamics(big, np.ones(770, dtype=np.float32), DT, 0.3, 0, 1, constraints=no_clusters(770)).step(
            torch.zeros((1, 770, 3), device=dev), torch.zeros((1, 770, 3), device=dev), 1)
    rc = lib.tw_apply_constraints(C.byref(with_(max_sweeps=0)), m.data_ptr(), 22, x.data_ptr(), v.data_ptr(), None, res.data_ptr(), 2, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc != 0 and "max_sweeps 0" in lib.tw_last_error().decode()
    assert all(torch.equal(a, b) for a, b in zip(everything, before))
    # the python layer refuses full-step velocities through the same message, and the good call runs
    md = dynamics(energy, masses, DT, 0.3, 0, 5, constraints=HBondConstraints(atoms, lengths, 22, TOL, SWEEPS))
    with pytest.raises(RuntimeError, match="not available with constraints"):
        md.trajectory(x, v, [1], velocities="full-step")
    assert md.n_dof == 66 - 12 and dynamics(energy, masses, DT, 0.3, 0, 5).n_dof == 66
    rc, msg = call()
    assert rc == 0 and float(res.max()) <= TOL and int(sw.max()) <= 16 and not torch.equal(bufs[0], before[5])
