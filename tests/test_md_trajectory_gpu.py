"""The device trajectory recorder (csrc/tw_md.hip `langevin_trajectory_kernel<W>` behind `tw_langevin_trajectory`,
`LangevinDynamics.trajectory`, timewarp_amd/simulation.py): the same stream as `LangevinDynamics.step`, frames that do not
depend on which steps are reported or on where a run is cut into launches (fp64 carry), frame contents against the float64
restatement tests/trajectory_oracle.py and against the force kernel / the C oracle, and the driver's files.

Shapes: 1, 22, 64 and 65 atoms (64 | 65: one wave | sixteen), 1 and 3 rows, at most 37 steps, both schemes, friction 0.3 and
50 / ps, first step 1000003, one 691-atom case of 3 steps.  Force-free tables and the real force field (alanine dipeptide, NNQQ)
are those of tests/test_langevin_gpu.py; the tolerances are that file's."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import langevin_oracle as lo
from tests import trajectory_oracle as to
from tests.test_langevin_cpu import FD_H, KBT, _cached_forces, real_case, restated
from tests.test_langevin_gpu import (FIRST_STEP, GAS_CONSTANT, TEMPERATURE, dynamics, free_energy, free_state, real_energy,
                                     worst_in_ulps)

pytestmark = pytest.mark.gpu

SIZES = [1, 22, 64, 65]
FRAME_KEYS = ("positions", "velocities", "forces", "energies")


def record(md, x, v, report_steps, num_steps=None, state=None):
    """-> (x, v, frames as a dict of numpy arrays + step / time)"""
    gx, gv, f = md.trajectory(torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda(), report_steps, num_steps=num_steps, state=state)
    frames = {k: getattr(f, k).cpu().numpy() for k in FRAME_KEYS}
    frames["step"], frames["time"] = f.step, f.time
    return gx.cpu().numpy(), gv.cpu().numpy(), frames


def same_frames(a, b, rows=slice(None)):
    return all(np.array_equal(a[k][rows], b[k][rows]) for k in FRAME_KEYS)


def free_runs():
    """(V, rows, friction): every size with 1 and 3 rows, the two frictions alternating so that each size sees both"""
    return [(V, rows, (0.3, 50.0)[(i + j) % 2]) for i, V in enumerate(SIZES) for j, rows in enumerate((1, 3))] + [(22, 3, 0.3), (65, 3, 50.0)]


def real_md(mol, scheme, friction, seed=4321, first_step=FIRST_STEP):
    _, masses, x0, v0 = real_case(mol)
    return dynamics(real_energy(mol), masses, 0.0005, friction, scheme, seed, first_step, temperature=310.0), x0, v0


# ---------------------------------------------------------------------------------------------
# a. the same stream as `step`
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
def test_one_frame_at_the_end_is_what_step_returns(scheme):
    """No carry, report_steps = [n]: coords / velocs come back bit for bit as `step(n)` returns them from the same inputs, and
    the single frame's positions / velocities are those values.  Force-free tables at every size, and the real force field:
    alanine dipeptide, NNQQ, and the 691-atom protein for 3 steps."""
    runs = [("free", V, rows, friction, 37) for V, rows, friction in free_runs()]
    runs += [("ad", 22, 3, 0.3, 13), ("nnqq", 65, 3, 50.0, 13), ("1hgv", 691, 2, 0.3, 3), ("ad", 22, 1, 50.0, 1)]
    for kind, V, rows, friction, n in runs:
        if kind == "free":
            masses, x, v = free_state(V, rows)
            make = lambda: dynamics(free_energy(V), masses, 0.0005, friction, scheme, 77 + V, FIRST_STEP)
        else:
            x, v = real_case(kind)[2][:rows], real_case(kind)[3][:rows]
            make = lambda: real_md(kind, scheme, friction)[0]
        md = make()
        sx, sv = (o.cpu().numpy() for o in md.step(torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda(), n))
        md2 = make()
        gx, gv, f = record(md2, x, v, [n])
        assert md2.steps_done == md.steps_done == FIRST_STEP + n
        assert np.array_equal(gx, sx) and np.array_equal(gv, sv), (kind, V, rows, friction)
        assert f["positions"].shape == (rows, 1, V, 3) and f["energies"].shape == (rows, 1, 2)
        assert np.array_equal(f["positions"][:, 0], sx) and np.array_equal(f["velocities"][:, 0], sv), (kind, V, rows, friction)
        assert f["step"].tolist() == [FIRST_STEP + n] and f["time"][0] == (FIRST_STEP + n) * 0.0005
        assert np.abs(sv - v).max() > 1e-4      # the run did something


# ---------------------------------------------------------------------------------------------
# b. spacing independence
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
def test_frames_do_not_depend_on_which_steps_are_reported(scheme):
    """Frames at steps {0, 1, 5, 13} of one launch equal, bit for bit, the same steps of a launch that reports 0 .. 13 -
    positions, velocities, forces and energies."""
    some = [0, 1, 5, 13]
    runs = [("free", V, rows, friction) for V, rows, friction in free_runs()] + [("ad", 22, 3, 0.3), ("nnqq", 65, 3, 50.0), ("nnqq", 65, 1, 0.3)]
    for kind, V, rows, friction in runs:
        if kind == "free":
            masses, x, v = free_state(V, rows)
            make = lambda: dynamics(free_energy(V), masses, 0.0005, friction, scheme, 5, FIRST_STEP)
        else:
            x, v = real_case(kind)[2][:rows], real_case(kind)[3][:rows]
            make = lambda: real_md(kind, scheme, friction)[0]
        ax, av, full = record(make(), x, v, list(range(14)))
        bx, bv, part = record(make(), x, v, some)
        assert np.array_equal(ax, bx) and np.array_equal(av, bv)
        for key in FRAME_KEYS:
            assert np.array_equal(full[key][:, some], part[key]), (kind, V, rows, key)
        assert np.array_equal(full["positions"][:, 0], x) and np.array_equal(full["velocities"][:, 0], v)   # frame 0 is the input
        assert part["step"].tolist() == [FIRST_STEP + s for s in some]
        if kind != "free":
            assert np.abs(full["forces"]).max() > 10.0 and not np.array_equal(full["forces"][:, 0], full["forces"][:, 13])


# ---------------------------------------------------------------------------------------------
# c. chunk invariance
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
def test_launches_with_the_fp64_carry_are_one_launch(scheme):
    """5 + 7 + 1 steps with the carry give the frames and the final state of one launch of 13, bit for bit (frames at 0, 1, 5,
    6, 12, 13: the first and last step of every launch).  Without the carry the state is rounded to float32 at 5 and 12 and the
    result may differ: it does differ on at least one case, so the carry is not being ignored."""
    reports = [0, 1, 5, 6, 12, 13]
    chunks = [(5, [0, 1, 5]), (7, [1, 7]), (1, [1])]
    runs = [("free", V, rows, friction) for V, rows, friction in free_runs()] + [("ad", 22, 3, 0.3), ("nnqq", 65, 3, 50.0)]
    differs = 0
    for kind, V, rows, friction in runs:
        if kind == "free":
            masses, x, v = free_state(V, rows)
            make = lambda: dynamics(free_energy(V), masses, 0.0005, friction, scheme, 5, FIRST_STEP)
        else:
            x, v = real_case(kind)[2][:rows], real_case(kind)[3][:rows]
            make = lambda: real_md(kind, scheme, friction)[0]
        wx, wv, want = record(make(), x, v, reports)
        for carry in (True, False):
            md = make()
            state = md.new_state(torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda()) if carry else None
            cx, cv, got = x, v, []
            for n, rel in chunks:
                cx, cv, f = record(md, cx, cv, rel, num_steps=n, state=state)
                got.append(f)
            assert md.steps_done == FIRST_STEP + 13
            cat = {k: np.concatenate([f[k] for f in got], axis=1) for k in FRAME_KEYS}
            assert np.concatenate([f["step"] for f in got]).tolist() == [FIRST_STEP + r for r in reports]
            same = same_frames(cat, want) and np.array_equal(cx, wx) and np.array_equal(cv, wv)
            if carry:
                assert same, (kind, V, rows, friction)
                assert np.array_equal(state[:, 0].cpu().numpy().astype(np.float32), wx) and np.array_equal(state[:, 1].cpu().numpy().astype(np.float32), wv)
            else:
                differs += not same
                assert np.array_equal(cat["positions"][:, :3], want["positions"][:, :3])     # the first launch is the same launch
    assert differs >= 1


# ---------------------------------------------------------------------------------------------
# d. force-free tables against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
def test_force_free_frames_match_the_restatement(scheme):
    """Positions / velocities of every frame within one float32 ulp of tests/trajectory_oracle.py (`worst_in_ulps <= 1`, the bound of
    tests/test_langevin_gpu.py); forces and E_pot exactly 0; E_kin within 2^-22 relative of 1/2 sum m v^2 of the recorded float32
    velocities (each velocity is rounded by <= 2^-24 relative, its square by ~2^-23; a sum of positives keeps that; a factor 2 of
    margin).  Every size, 1 and 3 rows, 37 steps, both frictions; 691 atoms for 3 steps."""
    kbT = GAS_CONSTANT * TEMPERATURE
    runs = [(V, rows, friction, 37, [0, 1, 2, 17, 36, 37]) for V, rows, friction in free_runs()] + [(691, 3, 50.0, 3, [0, 1, 3])]
    report = []
    for V, rows, friction, n, reports in runs:
        masses, x, v = free_state(V, rows)
        seed = 0x9E3779B97F4A7C15 ^ (V * 7919 + rows)
        gx, gv, f = record(dynamics(free_energy(V), masses, 0.0005, friction, scheme, seed, FIRST_STEP), x, v, reports, num_steps=n)
        w = to.record(lo.no_forces, masses, x, v, reports, n, 0.0005, friction, kbT, scheme, seed, FIRST_STEP)
        ulps = (worst_in_ulps(f["positions"], w["positions"]), worst_in_ulps(f["velocities"], w["velocities"]),
                worst_in_ulps(gx, w["final_x"]), worst_in_ulps(gv, w["final_v"]))
        ek = 0.5 * (masses.astype(np.float64)[None, None, :, None] * f["velocities"].astype(np.float64) ** 2).sum(axis=(2, 3))
        ek_err = float((np.abs(f["energies"][..., 1] - ek) / ek).max())
        report.append((max(ulps), ek_err, V, rows, friction))
        assert np.count_nonzero(f["forces"]) == 0 and np.count_nonzero(f["energies"][..., 0]) == 0, (V, rows)
        assert ek.min() > 0.0 and np.abs(f["velocities"][:, -1] - v).max() > 1e-3
    print(f"scheme {scheme}: worst distance {max(r[0] for r in report):.3f} ulp, E_kin off by {max(r[1] for r in report):.2e} relative (bound {2.0 ** -22:.2e})")
    assert not [r for r in report if r[0] > 1.0 or r[1] > 2.0 ** -22], report


# ---------------------------------------------------------------------------------------------
# e. real force field, frame 0
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mol", ["ad", "nnqq", "1hgv"])
def test_frame_zero_holds_the_forces_and_energy_of_the_input(mol):
    """report_steps = [0], n_steps = 0.  Forces: within one float32 ulp of the conformation's largest force component of
    `energy_and_forces` on the same coords (the same fp64 device function on identical input: only contraction order can differ,
    far below a float32 ulp, so at most one rounding flips).  E_pot: within 1e-6 |E| of the C oracle's energy (the bound
    tests/test_langevin_gpu.py holds `out_energy` to).  The state comes back unchanged and no step is counted."""
    tables, masses, x0, v0 = real_case(mol)
    md, _, _ = real_md(mol, 0, 0.3)
    gx, gv, f = record(md, x0, v0, [0], num_steps=0)
    assert md.steps_done == FIRST_STEP and np.array_equal(gx, x0) and np.array_equal(gv, v0)
    assert np.array_equal(f["positions"][:, 0], x0) and np.array_equal(f["velocities"][:, 0], v0)
    _, want = real_energy(mol).energy_and_forces(torch.from_numpy(x0).cuda())
    want = want.cpu().numpy()
    largest = np.abs(want).max(axis=(1, 2), keepdims=True)
    ulp = np.spacing(largest.astype(np.float32)).astype(np.float64)
    err = np.abs(f["forces"][:, 0].astype(np.float64) - want)
    e_ref, _ = H.oracle_energy(tables, x0.astype(np.float64), dtype=np.float64)
    de = np.abs(f["energies"][:, 0, 0] - e_ref) / np.abs(e_ref)
    ek = 0.5 * (masses.astype(np.float64)[None, :, None] * v0.astype(np.float64) ** 2).sum(axis=(1, 2))
    print(f"{mol}: forces off by {(err / ulp).max():.3f} ulp of the largest component ({largest.max():.1f}), E_pot by {de.max():.2e} of |E|")
    assert np.all(err <= ulp)
    assert de.max() < 1e-6
    assert np.all(np.abs(f["energies"][:, 0, 1] - ek) <= 2.0 ** -22 * ek)      # exact float32 inputs: far inside
    assert largest.min() > 100.0


# ---------------------------------------------------------------------------------------------
# f. real force field, later frames
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mol,scheme,friction", [(m, s, f) for m in ("ad", "nnqq") for s in (0, 1) for f in (0.3, 50.0)])
def test_real_force_field_frames_match_the_restatement(mol, scheme, friction):
    """Frames at steps 0, 1, 4 and 10 of the 10-step runs of test_real_force_field_steps_match_the_restatement (8 rows): recorded
    positions / velocities within 4 u + 1 ulp32 of tests/trajectory_oracle.py on central differences of step h / 2, u the
    finite-difference error tests/test_langevin_cpu.py measures for that run.  With the chunk invariance and frame 0 above this
    covers the forces of later frames: frame r is frame 0 of a launch that starts there.  E_pot of later frames is printed here,
    not asserted: what would catch an energy (or a force) taken from the wrong force evaluation under the real force field is
    test b above, whose bitwise comparison includes `energies` and `forces` of steps 1, 5 and 13 against the launch that reports
    every step, together with test c (frame r of one launch = frame 0 of the launch that starts at r) and test e (frame 0)."""
    r = restated(mol, scheme, friction)
    tables, masses, x0, v0 = real_case(mol)
    reports = [0, 1, 4, r.steps]
    md = dynamics(real_energy(mol), masses, 0.0005, friction, scheme, r.seed, r.first_step, temperature=310.0)
    gx, gv, f = record(md, x0, v0, reports)
    w = to.record(_cached_forces(mol, FD_H / 2), masses, x0, v0, reports, r.steps, 0.0005, friction, KBT, scheme, r.seed, r.first_step)
    assert np.array_equal(w["final_x"], r.fine[0]) and np.array_equal(w["final_v"], r.fine[1])     # the restated run of that test
    assert r.keep.all()
    wx, wv = w["positions"].astype(np.float64), w["velocities"].astype(np.float64)
    # one float32 ulp of the restated value, as Restated.bounds() takes it (the spacing of the float32 array)
    bx, bv = 4 * r.u_x + np.spacing(np.abs(w["positions"])), 4 * r.u_v + np.spacing(np.abs(w["velocities"]))
    ex, ev = np.abs(f["positions"].astype(np.float64) - wx), np.abs(f["velocities"].astype(np.float64) - wv)
    de = np.abs(f["energies"][..., 0] - w["energies"][..., 0]) / np.abs(w["energies"][..., 0])
    print(f"{mol} scheme {scheme} friction {friction}: x {(ex / bx).max():.2f} of the bound, v {(ev / bv).max():.2f}; E_pot {de.max():.2e} of |E| "
          "(printed only: the energy of a frame is held by frame 0 and the chunk invariance)")
    assert np.all(ex <= bx) and np.all(ev <= bv)
    assert np.array_equal(f["positions"][:, -1], gx) and np.array_equal(f["velocities"][:, -1], gv)


# ---------------------------------------------------------------------------------------------
# g. rows are independent
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("V", [22, 65])
def test_a_row_of_a_trajectory_does_not_depend_on_its_neighbours(scheme, V):
    """Row 1 of a 3-row launch equals, bit for bit, the same state run as conformation 1 with other neighbours (another row 0, no
    row 2); it is the restatement of that row alone under conformation index 1; and it is NOT what the state gives as row 0 of a
    launch of its own (the row is the conformation of the noise key)."""
    kbT = GAS_CONSTANT * TEMPERATURE
    reports = [0, 2, 4]
    masses, x, v = free_state(V, 3, seed=2)
    make = lambda: dynamics(free_energy(V), masses, 0.001, 50.0, scheme, 31, FIRST_STEP)
    gx, gv, f = record(make(), x, v, reports)
    _, x2, v2 = free_state(V, 3, seed=9)
    ox, ov, o = record(make(), np.stack([x2[0], x[1]]), np.stack([v2[0], v[1]]), reports)
    assert same_frames(f, o, rows=slice(1, 2)) and np.array_equal(gx[1], ox[1]) and np.array_equal(gv[1], ov[1])
    assert not np.array_equal(f["velocities"][0], o["velocities"][0])
    w = to.record(lo.no_forces, masses, x[1:2], v[1:2], reports, 4, 0.001, 50.0, kbT, scheme, 31, FIRST_STEP, conformations=[1])
    assert max(worst_in_ulps(f["positions"][1:2], w["positions"]), worst_in_ulps(f["velocities"][1:2], w["velocities"])) <= 1.0
    ax, av, alone = record(make(), x[1:2], v[1:2], reports)
    assert worst_in_ulps(alone["velocities"][:, 1:], f["velocities"][1:2, 1:]) > 100.0
    assert np.array_equal(alone["velocities"][:, 0], f["velocities"][1:2, 0])        # frame 0 is the input either way


# ---------------------------------------------------------------------------------------------
# h. the driver
# ---------------------------------------------------------------------------------------------
def test_simulate_trajectory_writes_the_reference_file_format(tmp_path):
    """Alanine dipeptide, 2 replicas, burn-in 3, sampling 24, LogarithmicSpacing(10, 3), 7 steps per launch: two files with the
    reporter's keys, dtypes and shapes (where the committed reference-format file tests/golden/energy_kat_1hgv.npz has the key:
    as there), step = report_steps(spacing, 3, 27), time = step * dt, and the arrays of ONE direct `trajectory` call."""
    import os

    from timewarp_amd import simulation as S
    from timewarp_amd.md import LangevinDynamics

    _, masses, x0, v0 = real_case("ad")
    energy = real_energy("ad")
    x, v = torch.from_numpy(x0[:2]).cuda(), torch.from_numpy(v0[:2]).cuda()
    make = lambda: LangevinDynamics(energy, torch.from_numpy(masses), 0.0005, 0.3, "LangevinMiddleIntegrator", seed=11)
    rows = S.simulate_trajectory(energy, torch.from_numpy(masses), x, v, burn_in=3, sampling=24, spacing=S.LogarithmicSpacing(10, 3),
                                 integrator=make(), steps_per_launch=7, out_dir=str(tmp_path), name="ad")
    want_steps = S.report_steps(S.LogarithmicSpacing(10, 3), 3, 27)
    assert want_steps.tolist() == [9, 10, 11, 13, 19, 20, 21, 23]
    assert sorted(os.listdir(tmp_path)) == ["ad-0-traj-arrays.npz", "ad-1-traj-arrays.npz"]
    md = make()
    _, _, direct = md.trajectory(x, v, want_steps, num_steps=27)
    assert md.steps_done == 27
    kat = np.load(os.path.join(os.path.dirname(__file__), "golden", "energy_kat_1hgv.npz"))
    T, V = len(want_steps), 22
    layout = {"step": (np.int64, (T,)), "time": (np.float64, (T,)), "energies": (np.float64, (T, 2)), "positions": (np.float32, (T, V, 3)),
              "velocities": (np.float32, (T, V, 3)), "forces": (np.float32, (T, V, 3))}
    for row in range(2):
        z = np.load(tmp_path / f"ad-{row}-traj-arrays.npz")
        assert sorted(z.files) == sorted(layout)
        for key, (dtype, shape) in layout.items():
            assert z[key].dtype == dtype and z[key].shape == shape, key
            assert np.array_equal(z[key], rows[row][key])
        for key in ("positions", "forces"):      # [frames, atoms, 3] float32, as the reference's own file has them
            assert z[key].dtype == kat[key].dtype and z[key].ndim == kat[key].ndim and z[key].shape[2:] == kat[key].shape[2:]
        assert z["energies"].dtype == kat["energies"].dtype
        assert np.array_equal(z["step"], want_steps) and np.array_equal(z["time"], want_steps * 0.0005)
        for key in FRAME_KEYS:
            assert np.array_equal(z[key], getattr(direct, key)[row].cpu().numpy()), key
        assert np.abs(z["forces"]).max() > 100.0 and z["energies"][:, 1].min() > 0.0
    # one replica: the name without a row number; missing velocities are drawn at temperature
    S.simulate_trajectory(energy, torch.from_numpy(masses), x[:1], burn_in=0, sampling=4, spacing=S.RegularSpacing(2), seed=3,
                          out_dir=str(tmp_path / "one"), name="solo")
    z = np.load(tmp_path / "one" / "solo-traj-arrays.npz")
    assert z["step"].tolist() == [2, 4] and 1.0 < z["energies"][0, 1] < 400.0     # 66 degrees of freedom at 310 K: ~85 kJ/mol
