"""Cost of the device minimiser (`md.minimize_energy` -> `tw_minimize`) on alanine dipeptide (22 atoms, one wave per row), NNQQ
(65 atoms, frame 0 of tests/golden/energy_kat_2olx.npz, sixteen waves) and the 691-atom protein of energy_kat_1hgv.npz, to the
reference's tolerance of 2 kJ/mol/nm: iterations, force evaluations, wall time, ms per force evaluation - and, in the same run
on the same rows, the ms per step of `LangevinDynamics.step`, whose step is one force evaluation plus a trivial update.  The
ratio of the two is what the L-BFGS bookkeeping (two-loop recursion, reductions, workspace traffic) costs per evaluation.
The figures behind `md.default_iterations_per_launch` (profiles/minimize.txt).  `python tools/time_minimize.py`"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timewarp_amd import simulation as S, synthetic
from timewarp_amd.energy import AmberPotentialEnergyTorch
from timewarp_amd.forcefield import ELEMENT_MASSES, amber99sbildn_obc_tables
from timewarp_amd.md import LangevinDynamics, default_iterations_per_launch, minimize_energy

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
dev = torch.device("cuda")
TOLERANCE = 2.0


def kat_system(file, order=None):
    z = np.load(os.path.join(GOLDEN, file))
    names = [str(n) for n in z["atom_names"]]
    kw = {"improper_neighbour_order": order} if order else {}
    tables = amber99sbildn_obc_tables(names, [str(r) for r in z["residue_names"]], [int(i) for i in z["residue_ids"]], **kw)
    masses = torch.tensor([ELEMENT_MASSES[next(ch for ch in n if ch.isalpha())] for n in names], dtype=torch.float32)
    return AmberPotentialEnergyTorch(tables), masses, torch.from_numpy(z["positions"][0].astype(np.float32))


def systems():
    _, coords, masses = synthetic.alanine_dipeptide_state()
    yield "alanine dipeptide (22 atoms)", AmberPotentialEnergyTorch.alanine_dipeptide(), masses, coords.to(torch.float32), 2000
    yield ("NNQQ (65 atoms)",) + kat_system("energy_kat_2olx.npz") + (1000,)
    yield ("1hgv (691 atoms)",) + kat_system("energy_kat_1hgv.npz", "pyset") + (50,)


def wall(fn):
    """seconds of one call, host clock around a synchronised device, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


for label, energy, masses, coords, n_steps in systems():
    V = coords.shape[0]
    for rows in (1, 256):      # one workgroup per row: one row, and one row per CU
        x = coords.to(dev)[None].repeat(rows, 1, 1).contiguous()
        md = LangevinDynamics.for_energy(energy, masses, seed=1)
        v = S.thermal_velocities(md.masses, md.kbT, x)
        t_md, _ = wall(lambda: md.step(x, v, n_steps))
        ms_step = t_md / n_steps * 1e3
        print(f"{label} x {rows} rows: LangevinDynamics.step, {n_steps} steps in one launch: {ms_step:9.4f} ms per step", flush=True)
        for per_launch in (default_iterations_per_launch(V), 1000000):
            t, r = wall(lambda: minimize_energy(energy, x, tolerance=TOLERANCE, iterations_per_launch=per_launch))
            it, ev = int(r.iterations.max()), int(r.evaluations.max())
            ms_eval = t / ev * 1e3
            what = "one launch" if per_launch == 1000000 else f"{per_launch} iterations per launch ({-(-it // per_launch)} launches)"
            print(f"{label} x {rows} rows: minimize_energy to {TOLERANCE} kJ/mol/nm, {what}: status {sorted(set(r.status.tolist()))}, "
                  f"{it} iterations, {ev} evaluations, E {float(energy.energy_and_forces(x)[0][0]):.2f} -> {float(r.energy[0]):.2f} kJ/mol, "
                  f"rms {float(r.rms_force[0]):.3f}; {t * 1e3:9.2f} ms = {ms_eval:9.4f} ms per evaluation = {ms_eval / ms_step:5.2f} x a Langevin step",
                  flush=True)
