"""Per-step time of the constrained Langevin kernel (`LangevinDynamics(constraints="h-bonds")` -> `tw_langevin_trajectory_constrained`)
against the unconstrained one (`tw_langevin_trajectory`) on alanine dipeptide (22 atoms, one wave per row), NNQQ (65 atoms) and the
691-atom protein 1hgv (sixteen waves per row), with the method of tools/time_md_trajectory.py: the fp64 carry, no frame, HIP events
around one launch, median of five after a warm-up.  From that: simulated ns per day at 0.5 fs unconstrained against 2 fs
constrained, the SHAKE sweeps and residuals of the timed launches, and the registers and scratch of the kernels of csrc/tw_md.hip
(tools/resource_usage.py; needs hipcc, no GPU).  The figures of profiles/md_constraints.txt.

    python tools/time_md_constraints.py [--skip-timing] [--skip-resources] [--out profiles/md_constraints.txt]"""
import argparse, os, subprocess, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from timewarp_amd import simulation as S, synthetic
from timewarp_amd.energy import AmberPotentialEnergyTorch
from timewarp_amd.forcefield import ELEMENT_MASSES, amber99sbildn_obc_tables
from timewarp_amd.md import LangevinDynamics

GOLDEN = os.path.join(ROOT, "tests", "golden")
TOLERANCE = 1e-8      # the default of forcefield.hbond_constraints


def systems():
    _, coords, masses = synthetic.alanine_dipeptide_state()
    yield "alanine dipeptide (22 atoms)", AmberPotentialEnergyTorch.alanine_dipeptide(), masses, coords, 2000
    z = np.load(os.path.join(GOLDEN, "energy_kat_2olx.npz"))
    tables = amber99sbildn_obc_tables([str(n) for n in z["atom_names"]], [str(r) for r in z["residue_names"]], [int(i) for i in z["residue_ids"]])
    masses = torch.tensor([ELEMENT_MASSES[str(e)] for e in z["elements"]], dtype=torch.float32)
    yield "NNQQ (65 atoms)", AmberPotentialEnergyTorch(tables), masses, torch.from_numpy(z["positions"][0].astype(np.float32)), 1000
    z = np.load(os.path.join(GOLDEN, "energy_kat_1hgv.npz"))
    names = [str(n) for n in z["atom_names"]]
    tables = amber99sbildn_obc_tables(names, [str(r) for r in z["residue_names"]], [int(i) for i in z["residue_ids"]], improper_neighbour_order="pyset")
    masses = torch.tensor([ELEMENT_MASSES[next(ch for ch in n if ch.isalpha())] for n in names], dtype=torch.float32)
    yield "1hgv (691 atoms)", AmberPotentialEnergyTorch(tables), masses, torch.from_numpy(z["positions"][1].astype(np.float32)), 100


def timed(fn, repeats=5):
    """median and minimum over `repeats` calls, ms, HIP events on the launch stream, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def timing(emit):
    dev = torch.device("cuda")
    emit("# us per step: one launch of n steps, fp64 carry, no frame; median (min) of 5.  ns/day = timestep x 86400 s / time per step, per row.")
    for label, energy, masses, coords, n in systems():
        for rows in (1, 256):      # one workgroup per row: a single row, and one row per CU
            x = coords.to(dev)[None].repeat(rows, 1, 1).contiguous()
            result = {}
            for kind, dt_fs, kw in (("unconstrained", 0.5, {}), ("h-bonds", 2.0, dict(constraints="h-bonds", constraint_tolerance=TOLERANCE))):
                md = LangevinDynamics.for_energy(energy, masses, seed=1, timestep_ps=1e-3 * dt_fs, **kw)
                v = S.thermal_velocities(md.masses, md.kbT, x)
                state = md.new_state(x, v)      # the carry moves on from call to call
                if md.constraints is not None:
                    md.apply_constraints(None, state=state)
                med, best = timed(lambda: md.trajectory(None, None, [], num_steps=n, state=state))
                us = med / n * 1e3
                result[(kind, dt_fs)] = us
                extra = ""
                if md.constraints is not None:
                    extra = (f"  sweeps <= {int(md.constraint_sweeps.max())}, residual <= {float(md.constraint_residual.max()):.2e} "
                             f"(tolerance {TOLERANCE:.0e}; {md.constraints.n_clusters} clusters, {md.constraints.n_constraints} constraints)")
                emit(f"{label} x {rows} rows, {n} steps per launch, {kind:13s} {dt_fs} fs: {us:9.2f} us per step (min {best / n * 1e3:9.2f})  "
                     f"= {dt_fs * 86.4 / us:9.3f} ns/day{extra}")
            a, c = result[("unconstrained", 0.5)], result[("h-bonds", 2.0)]
            emit(f"{label} x {rows} rows: constraint phases cost {100.0 * (c - a) / a:+.1f} % per step; simulated time per day x {4.0 * a / c:.2f} (2 fs constrained / 0.5 fs unconstrained)")


def resources(emit):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), os.path.join(ROOT, "timewarp_amd", "csrc", "tw_md.hip")],
                         stdout=subprocess.PIPE, text=True, check=True)
    emit("# registers and scratch of every kernel of csrc/tw_md.hip (tools/resource_usage.py)")
    for line in res.stdout.splitlines():
        emit(line)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--skip-resources", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "md_constraints.txt"))
    args = ap.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    if not args.skip_timing:
        timing(emit)
    if not args.skip_resources:
        resources(emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
