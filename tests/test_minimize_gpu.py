"""The device energy minimiser (csrc/tw_md.hip `minimize_kernel<W>` behind `tw_minimize`, `timewarp_amd.md.minimize_energy`,
`simulate_trajectory(minimize=, redraw_velocities=)`): status codes, the iterates against the float64 restatement
tests/minimize_oracle.py on the one-bond molecule, the minimum against the C oracle's energy and its finite-difference
forces on the real force field, and the invariances - a row does not depend on its batch, nor on where the iterations are
cut into launches - bit for bit.

Shapes: 1 and 2 atoms, alanine dipeptide (22 atoms, one wave), NNQQ (65 atoms, sixteen waves), three iterations of the
691-atom protein (the 160 KiB LDS opt-in)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import langevin_oracle as lo
from tests import minimize_oracle as mo

pytestmark = pytest.mark.gpu

HISTORY = 8
MAX_DISP = 0.01
FD_H = 1e-5     # nm, the difference step of the Langevin tests; the second run uses h / 2


def free_tables(V):
    """(the tables of tests/test_langevin_gpu.py: forces vanish identically)"""
    from timewarp_amd.forcefield import ForceFieldTables

    z = lambda w, t=np.float64: np.zeros((0, w), dtype=t)
    atom_par = np.tile(np.array([[0.0, 0.3, 0.0, 0.15, 0.8]]), (V, 1))
    return ForceFieldTables(bond_idx=z(2, np.int32), bond_par=z(2), angle_idx=z(3, np.int32), angle_par=z(2), torsion_idx=z(4, np.int32),
                            torsion_par=z(3), exc_idx=z(2, np.int32), exc_par=z(3), atom_par=atom_par, has_gbsa=0)


def bond_only_tables(r0=0.1, k=3.0e5):
    """(the tables of tests/test_langevin_cpu.py: two atoms, one harmonic bond, nothing else)"""
    from timewarp_amd.forcefield import ForceFieldTables

    z = lambda w, t=np.float64: np.zeros((0, w), dtype=t)
    return ForceFieldTables(bond_idx=np.array([[0, 1]], dtype=np.int32), bond_par=np.array([[r0, k]]), angle_idx=z(3, np.int32),
                            angle_par=z(2), torsion_idx=z(4, np.int32), torsion_par=z(3), exc_idx=z(2, np.int32), exc_par=z(3),
                            atom_par=np.array([[0.0, 0.3, 0.0, 0.15, 0.8]] * 2), has_gbsa=0)


def bond_start(length):
    u = np.array([2.0, -1.0, 0.5]) / np.sqrt(5.25)
    a = np.array([0.02, 0.01, -0.03])
    return np.stack([a, a + length * u]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def system(mol):
    """(energy object, tables, masses tensor or None, start float32 [V,3])"""
    from timewarp_amd import synthetic
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from tests.test_energy_kat import kat, kat_tables, protein, protein_tables

    if mol == "ad":
        energy = AmberPotentialEnergyTorch.alanine_dipeptide()
        _, coords, masses = synthetic.alanine_dipeptide_state()
        return energy, energy.tables, masses, coords.numpy().astype(np.float32)
    z = kat() if mol == "nnqq" else protein()
    tables = kat_tables(z) if mol == "nnqq" else protein_tables(z)
    return AmberPotentialEnergyTorch(tables), tables, None, np.ascontiguousarray(z["positions"][0], dtype=np.float32)


def raw(energy, x, ws, fresh, n_iterations, tolerance, history=HISTORY, max_disp=MAX_DISP):
    """One `tw_minimize` call on the float32 cuda tensor x [n,V,3] (updated in place) and the workspace `ws` (None: a new one,
    filled with NaN first so that anything the kernel leaves uninitialised shows).  -> (ws, dict of numpy outputs)"""
    from timewarp_amd import _lib

    lib = _lib.load()
    n, V = x.shape[0], energy.tables.n_atoms
    if ws is None:
        ws = torch.full((n, lib.tw_minimize_workspace_len(V, history)), float("nan"), dtype=torch.float64, device=x.device)
    ff = energy._device_ff(x.device)
    e, rms = (torch.empty(n, dtype=torch.float64, device=x.device) for _ in range(2))
    it, ev, st = (torch.empty(n, dtype=torch.int32, device=x.device) for _ in range(3))
    _lib.check(lib.tw_minimize(C.byref(ff.struct), x.data_ptr(), ws.data_ptr(), int(fresh), history, int(n_iterations), float(tolerance),
                               float(max_disp), e.data_ptr(), rms.data_ptr(), it.data_ptr(), ev.data_ptr(), st.data_ptr(), n,
                               _lib.stream_ptr(x.device)), "tw_minimize")
    out = {"x": x.cpu().numpy().copy(), "energy": e.cpu().numpy(), "rms": rms.cpu().numpy(), "iterations": it.cpu().numpy(),
           "evaluations": ev.cpu().numpy(), "status": st.cpu().numpy()}
    return ws, out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_outputs(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(same_bits(a[k][rows_a], b[k][rows_b]) for k in a)


def result_dict(r):
    return {k: getattr(r, k).cpu().numpy() for k in ("coords", "coords64", "energy", "rms_force", "iterations", "evaluations", "status", "converged")}


def minimized(mol, x, **kw):
    from timewarp_amd.md import minimize_energy

    return minimize_energy(system(mol)[0], torch.from_numpy(np.ascontiguousarray(x)).cuda(), **kw)


# ---------------------------------------------------------------------------------------------
# 1, 2: the smallest molecules
# ---------------------------------------------------------------------------------------------
def test_force_free_atom_is_converged_at_once():
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from timewarp_amd.md import minimize_energy

    x = torch.tensor([[[0.3, -1.7, 2.9]], [[1e-3, 5.0, -0.25]]], dtype=torch.float32).cuda()
    r = minimize_energy(AmberPotentialEnergyTorch(free_tables(1)), x, tolerance=2.0)
    assert r.status.tolist() == [0, 0] and r.iterations.tolist() == [0, 0] and r.evaluations.tolist() == [1, 1]
    assert r.converged.tolist() == [True, True] and r.converged.dtype == torch.bool
    assert same_bits(r.coords.cpu().numpy(), x.cpu().numpy()) and r.coords.shape == x.shape and r.coords.dtype == torch.float32
    assert torch.equal(r.coords64, x.to(torch.float64)) and r.energy.tolist() == [0.0, 0.0] and r.rms_force.tolist() == [0.0, 0.0]


def test_one_bond_matches_the_restatement_iteration_by_iteration():
    """Two rows, the bond stretched to 0.13 nm and compressed to 0.08 nm (r0 = 0.1 nm, k = 3e5), tolerance 2.  The device's
    per-iteration energies (one iteration per call on one workspace) and its final state against the restatement with
    analytic forces.

    Bound.  u = the restatement's own distance between its run and the run with every reduction summed in the opposite
    order.  Coordinates: 4 u_x + 1 ulp32 (the float32 cast), the fp64 state 4 u_x + 8 eps64 |x|.  Energies: 4 u_E plus the
    rounding of E = 1/2 k (r - r0)^2 itself: r carries dr = 8 eps64 r of error, so E moves by k |r - r0| dr + 1/2 k dr^2
    (both orders of the expansion: where the restatement lands on r = r0 exactly, E = 0 and only the second is left), plus
    8 eps64 E.
    Measured on an MI355X (profiles/minimize.txt): both rows 2 iterations, 3 evaluations; u_x 0, u_E 0 (six terms: the order of
    summation does not show).  Stretched: x64 identical to the restatement, x32 1.7e-9 nm off (0.49 of the bound), E 2.9e-29
    kJ/mol off at the last iterate, where the restatement's E is exactly 0.  Compressed: x64 1.4e-17 nm (0.26), x32 1.7e-9
    (0.45), E 1.2e-14 (0.06)."""
    from timewarp_amd.energy import AmberPotentialEnergyTorch

    r0, k, tol, V = 0.1, 3.0e5, 2.0, 2
    energy = AmberPotentialEnergyTorch(bond_only_tables(r0, k))
    starts = np.stack([bond_start(0.13), bond_start(0.08)])
    x = torch.from_numpy(starts.copy()).cuda()
    ws, out = raw(energy, x, None, 1, 0, tol)
    traces, outs = [out["energy"].copy()], [out]
    for _ in range(40):
        if not (outs[-1]["status"] == 1).any():
            break
        ws, out = raw(energy, x, ws, 0, 1, tol)
        traces.append(out["energy"].copy())
        outs.append(out)
    final = outs[-1]
    assert final["status"].tolist() == [0, 0]
    eps = np.finfo(np.float64).eps
    worst = {"x": 0.0, "x64": 0.0, "E": 0.0}
    for row in range(2):
        fwd = mo.minimize(mo.bond_forces(r0, k), starts[row], tol, 100, HISTORY, MAX_DISP)
        rev = mo.minimize(mo.bond_forces(r0, k), starts[row], tol, 100, HISTORY, MAX_DISP, reverse=True)
        assert fwd[5] == 0 and fwd[3:6] == rev[3:6]
        assert (int(final["iterations"][row]), int(final["evaluations"][row])) == (fwd[3], fwd[4])
        trace = np.array([t[row] for t in traces])[:fwd[3] + 1]
        assert len(trace) == len(fwd[6])
        u_x = np.abs(fwd[0] - rev[0]).max()
        u_E = np.abs(fwd[6] - rev[6])
        x64 = ws[row, 8:8 + 3 * V].cpu().numpy().reshape(V, 3)
        bx = 4 * u_x + np.spacing(np.abs(fwd[0]).astype(np.float32)).astype(np.float64)
        bx64 = 4 * u_x + 8 * eps * np.abs(fwd[0])
        dr = 8 * eps * 0.13      # the error of r
        bE = 4 * u_E + k * np.sqrt(2 * fwd[6] / k) * dr + 0.5 * k * dr ** 2 + 8 * eps * fwd[6]
        ex, ex64, eE = np.abs(final["x"][row] - fwd[0]), np.abs(x64 - fwd[0]), np.abs(trace - fwd[6])
        worst = {"x": max(worst["x"], (ex / bx).max()), "x64": max(worst["x64"], (ex64 / bx64).max()), "E": max(worst["E"], (eE / bE).max())}
        print(f"row {row}: {fwd[3]} iterations, {fwd[4]} evaluations; u_x {u_x:.2e} nm, u_E <= {u_E.max():.2e}; device to restatement: "
              f"x32 {ex.max():.2e} ({(ex / bx).max():.2f} of the bound), x64 {ex64.max():.2e} ({(ex64 / bx64).max():.2f}), "
              f"E {eE.max():.2e} ({(eE / bE).max():.2f})")
        assert np.all(ex <= bx) and np.all(ex64 <= bx64) and np.all(eE <= bE)
        # as in the CPU test: |r| = r0 and E within tolerance^2 3V / (2k) of zero
        r = np.linalg.norm(x64[0] - x64[1])
        assert 0.0 <= final["energy"][row] <= tol ** 2 * 3 * V / (2 * k) and abs(r - r0) <= np.sqrt(2.0 * (tol ** 2 * 3 * V / (2 * k)) / k)
        assert np.all(np.diff(trace) < 0.0) and abs(final["rms"][row] - fwd[2]) <= 4 * abs(fwd[2] - rev[2]) + 1e-6


# ---------------------------------------------------------------------------------------------
# 3 - 5: the real force field
# ---------------------------------------------------------------------------------------------
def ad_rows():
    x0 = system("ad")[3]
    rng = np.random.default_rng(31)
    pert = (x0 + 0.005 * rng.standard_normal(x0.shape)).astype(np.float32)
    return np.stack([x0, pert, x0])


@functools.lru_cache(maxsize=None)
def ad_batch():
    return minimized("ad", ad_rows(), tolerance=2.0)


def check_minimum(mol, start, r, tol):
    """the properties of a converged run of test 3 / 5, for every row of `start`"""
    energy, tables = system(mol)[:2]
    d = result_dict(r)
    V = tables.n_atoms
    assert d["status"].tolist() == [0] * len(start) and d["converged"].all() and (d["rms_force"] <= tol).all()
    e0 = energy.energy_and_forces(torch.from_numpy(start).cuda())[0].cpu().numpy()
    assert np.all(d["energy"] < e0), (d["energy"], e0)
    # the C oracle at the fp64 state
    e_c, _ = H.oracle_energy(tables, d["coords64"], dtype=np.float64)
    rel = np.abs(d["energy"] - e_c) / np.abs(e_c)
    assert rel.max() <= 1e-6, rel
    # the oracle's central-difference forces there
    rms_fd = lambda h: np.sqrt((lo.fd_forces(tables, h)(d["coords64"])[1] ** 2).sum((1, 2)) / (3 * V))
    coarse, fine = rms_fd(FD_H), rms_fd(FD_H / 2)
    e_fd = 4 * np.abs(coarse - fine)
    # the force kernel at the float32 coordinates that are handed on
    _, f32 = energy.energy_and_forces(r.coords)
    rms32 = f32.pow(2).sum((1, 2)).div(3 * V).sqrt().cpu().numpy()
    k_max = float(tables.bond_par[:, 1].max())
    b32 = k_max * float(np.spacing(np.float32(np.abs(d["coords"]).max())))
    print(f"{mol}: iterations {d['iterations'].tolist()}, evaluations {d['evaluations'].tolist()}, E {e0.round(3).tolist()} -> {d['energy'].round(3).tolist()}, "
          f"rms {d['rms_force'].round(4).tolist()}; |E - oracle| / |E| {rel.max():.1e}; finite-difference rms {fine.round(4).tolist()} (e_fd {e_fd.max():.1e}); "
          f"rms at the float32 coordinates off by {np.abs(rms32 - d['rms_force']).max():.2e} (bound {b32:.2e})")
    assert np.all(fine <= tol + e_fd)
    assert np.all(np.abs(rms32 - d["rms_force"]) <= b32)
    assert same_bits(d["coords"], d["coords64"].astype(np.float32))


def test_alanine_dipeptide_minimum():
    """Ideal geometry, the same plus N(0, 0.005 nm), and a copy of row 0, to 2 kJ/mol/nm."""
    start = ad_rows()
    r = ad_batch()
    check_minimum("ad", start, r, 2.0)
    d = result_dict(r)
    assert all(same_bits(d[k][2], d[k][0]) for k in d)
    assert same_bits(r.workspace[2].cpu().numpy(), r.workspace[0].cpu().numpy())
    assert not same_bits(d["coords"][1], d["coords"][0])
    solo = minimized("ad", start[1:2], tolerance=2.0)
    assert same_outputs(result_dict(solo), d, rows_b=slice(1, 2)) and same_bits(solo.workspace[0].cpu().numpy(), r.workspace[1].cpu().numpy())


def test_cut_invariance():
    """40 iterations in one call, in four calls of 10 on one workspace, and through minimize_energy(iterations_per_launch=7,
    max_iterations=40): the whole workspace and every output bit for bit.  (Tolerance 1e-6: the run is still going after 40.)"""
    energy = system("ad")[0]
    start = ad_rows()[:2]
    tol = 1e-6
    xa = torch.from_numpy(start.copy()).cuda()
    wa, a = raw(energy, xa, None, 1, 40, tol)
    xb = torch.from_numpy(start.copy()).cuda()
    wb, b = raw(energy, xb, None, 1, 10, tol)
    for _ in range(3):
        wb, b = raw(energy, xb, wb, 0, 10, tol)
    assert a["iterations"].tolist() == [40, 40] and a["status"].tolist() == [1, 1]
    assert same_outputs(a, b) and same_bits(wa.cpu().numpy(), wb.cpu().numpy())
    assert not np.isnan(wa.cpu().numpy()).any()      # the NaN fill is gone: a fresh call initialises every entry
    # seven per launch: 7 * 5 + 5
    r = minimized("ad", start, tolerance=tol, max_iterations=40, iterations_per_launch=7, history=HISTORY, max_displacement=MAX_DISP)
    d = result_dict(r)
    assert same_bits(r.workspace.cpu().numpy(), wa.cpu().numpy())
    assert same_bits(d["coords"], a["x"]) and same_bits(d["energy"], a["energy"]) and same_bits(d["rms_force"], a["rms"])
    assert same_bits(d["iterations"], a["iterations"]) and same_bits(d["evaluations"], a["evaluations"]) and same_bits(d["status"], a["status"])
    # ... and the uncut default run ends where the chain of sevens ends
    full = minimized("ad", start, tolerance=2.0)
    sevens = minimized("ad", start, tolerance=2.0, iterations_per_launch=7)
    assert same_outputs(result_dict(full), result_dict(sevens)) and same_bits(full.workspace.cpu().numpy(), sevens.workspace.cpu().numpy())


def test_nnqq_minimum_on_the_sixteen_wave_path():
    start = system("nnqq")[3][None]
    check_minimum("nnqq", start, minimized("nnqq", start, tolerance=10.0), 10.0)


def test_three_iterations_of_the_protein():
    energy, tables, _, x0 = system("1hgv")
    tol = 2.0
    xa = torch.from_numpy(x0[None].copy()).cuda()
    wa, a = raw(energy, xa, None, 1, 3, tol)
    e0, _ = energy.energy_and_forces(torch.from_numpy(x0[None]).cuda())
    assert a["status"].tolist() == [1] and a["iterations"].tolist() == [3] and a["energy"][0] < float(e0[0])
    xb = torch.from_numpy(x0[None].copy()).cuda()
    wb, b = raw(energy, xb, None, 1, 1, tol)
    wb, b = raw(energy, xb, wb, 0, 2, tol)
    assert same_outputs(a, b) and same_bits(wa.cpu().numpy(), wb.cpu().numpy())
    xc = torch.from_numpy(x0[None].copy()).cuda()
    wc, c = raw(energy, xc, None, 1, 0, tol)
    f0 = energy.energy_and_forces(torch.from_numpy(x0[None]).cuda())[1]
    assert same_bits(c["energy"], e0.cpu().numpy()) and same_bits(c["x"], x0[None])
    assert c["evaluations"].tolist() == [1] and c["iterations"].tolist() == [0] and c["status"].tolist() == [1]
    assert abs(c["rms"][0] - float(f0.pow(2).sum().div(3 * tables.n_atoms).sqrt())) <= 1e-12 * c["rms"][0]     # (another order of summation)


# ---------------------------------------------------------------------------------------------
# 7, 8: a bad row, the budget
# ---------------------------------------------------------------------------------------------
def test_a_bad_row_stops_alone():
    from timewarp_amd import simulation as S

    energy, _, masses, x0 = system("ad")
    bad = x0.copy()
    bad[5] = bad[4]      # two atoms at one point
    start = np.stack([bad, ad_rows()[1]])
    r = minimized("ad", start, tolerance=2.0)
    d = result_dict(r)
    assert d["status"].tolist() == [3, 0] and d["converged"].tolist() == [False, True]
    assert d["iterations"][0] == 0 and d["evaluations"][0] == 1 and same_bits(d["coords"][0], bad)
    solo = result_dict(ad_batch())
    assert all(same_bits(d[k][1], solo[k][1]) for k in d)
    with pytest.raises(RuntimeError, match=r"row\(s\) 0 "):
        S.simulate_trajectory(energy, masses, torch.from_numpy(start).cuda(), burn_in=0, sampling=4, spacing=S.RegularSpacing(2), minimize=True)


def test_budget_and_continuation():
    start = ad_rows()[:2]
    cut = minimized("ad", start, tolerance=2.0, max_iterations=2)
    assert cut.status.tolist() == [1, 1] and cut.converged.tolist() == [False, False] and cut.iterations.tolist() == [2, 2]
    go_on = minimized("ad", start, tolerance=2.0, workspace=cut.workspace)
    full, d = result_dict(ad_batch()), result_dict(go_on)
    assert d["status"].tolist() == [0, 0]
    assert all(same_bits(d[k], full[k][:2]) for k in d) and same_bits(go_on.workspace.cpu().numpy(), ad_batch().workspace[:2].cpu().numpy())


# ---------------------------------------------------------------------------------------------
# 9: the driver
# ---------------------------------------------------------------------------------------------
def load_rows(path, name, n):
    from timewarp_amd import simulation as S

    return [dict(np.load(S.trajectory_path(str(path), name, r, n))) for r in range(n)]


def same_rows(a, b):
    return len(a) == len(b) and all(set(x) == set(y) and all(same_bits(x[k], y[k]) for k in x) for x, y in zip(a, b))


def test_driver_minimises_first(tmp_path):
    from timewarp_amd import simulation as S

    energy, _, masses, _ = system("ad")
    start = torch.from_numpy(ad_rows()[:2]).cuda()
    kw = dict(burn_in=5, sampling=12, spacing=S.RegularSpacing(4), seed=11, steps_per_launch=6)
    log = []
    S.simulate_trajectory(energy, masses, start, out_dir=str(tmp_path / "a"), name="m", minimize=True, min_tol=2.0, minimization_log=log, **kw)
    res = minimized("ad", ad_rows()[:2], tolerance=2.0)
    S.simulate_trajectory(energy, masses, res.coords, out_dir=str(tmp_path / "b"), name="m", **kw)
    S.simulate_trajectory(energy, masses, start, out_dir=str(tmp_path / "c"), name="m", **kw)
    a, b, c = (load_rows(tmp_path / d, "m", 2) for d in "abc")
    assert same_rows(a, b) and not same_rows(a, c)
    assert len(log) == 1 and same_bits(log[0][0].coords.cpu().numpy(), res.coords.cpu().numpy()) and np.all(log[0][1].cpu().numpy() > res.energy.cpu().numpy())
    assert a[0]["step"].tolist() == [8, 12, 16]


def test_driver_redraws_velocities(tmp_path):
    from timewarp_amd import simulation as S
    from timewarp_amd.md import LangevinDynamics

    energy, _, masses, _ = system("ad")
    x = ad_batch().coords[:2].clone()
    kw = dict(burn_in=5, sampling=12, spacing=S.RegularSpacing(4), seed=11, steps_per_launch=6)
    with_redraw = S.simulate_trajectory(energy, masses, x, redraw_velocities=True, **kw)
    without = S.simulate_trajectory(energy, masses, x, **kw)
    # by hand: the initial draw, the burn-in, the documented redraw, the sampling
    first, again = S.velocity_seeds(11)
    md = LangevinDynamics.for_energy(energy, masses, seed=11)
    gen = torch.Generator(device=x.device)
    gen.manual_seed(first)
    v = S.thermal_velocities(md.masses, md.kbT, x, gen)
    state = md.new_state(x, v)
    md.trajectory(None, None, [], num_steps=5, state=state)
    gen = torch.Generator(device=x.device)
    gen.manual_seed(again)
    state[:, 1] = S.thermal_velocities(md.masses, md.kbT, x, gen).to(torch.float64)
    _, _, f = md.trajectory(None, None, [3, 7, 11], num_steps=12, state=state)
    hand = [S.frame_arrays([f], r) for r in range(2)]
    for r in range(2):
        for k in ("positions", "velocities", "forces", "energies"):
            assert same_bits(with_redraw[r][k], hand[r][k]), (r, k)
        assert with_redraw[r]["step"].tolist() == [8, 12, 16] == without[r]["step"].tolist()
        assert not same_bits(with_redraw[r]["velocities"], without[r]["velocities"])
    assert first != again
