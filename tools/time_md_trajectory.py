"""Per-step time of the recording Langevin kernel (`LangevinDynamics.trajectory` -> `tw_langevin_trajectory`) on alanine dipeptide
(22 atoms, one wave per row) and on the reference's 691-atom test protein (1hgv: topology and a frame from
tests/golden/energy_kat_1hgv.npz, sixteen waves per row), against `LangevinDynamics.step` on the same state, and what the cut into
launches costs `simulate_trajectory`.  The figures behind the default `steps_per_launch` (profiles/md_trajectory.txt).
`python tools/time_md_trajectory.py`"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timewarp_amd import simulation as S, synthetic
from timewarp_amd.energy import AmberPotentialEnergyTorch
from timewarp_amd.forcefield import ELEMENT_MASSES, amber99sbildn_obc_tables
from timewarp_amd.md import LangevinDynamics

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
dev = torch.device("cuda")


def systems():
    _, coords, masses = synthetic.alanine_dipeptide_state()
    yield "alanine dipeptide (22 atoms)", AmberPotentialEnergyTorch.alanine_dipeptide(), masses, coords, 2000
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


for label, energy, masses, coords, n in systems():
    for rows in (1, 256, 512):      # one workgroup per row: up to one row per CU (256), then twice that
        md = LangevinDynamics.for_energy(energy, masses, seed=1)
        x = coords.to(dev)[None].repeat(rows, 1, 1).contiguous()
        v = S.thermal_velocities(md.masses, md.kbT, x)
        state = md.new_state(x, v)      # the carry moves on from call to call, so the trajectory cases continue from it (None, None)
        cases = [("step (no frames, float32 state)", lambda: md.step(x, v, n)),
                 ("trajectory, fp64 carry, no frame", lambda: md.trajectory(None, None, [], num_steps=n, state=state)),
                 ("trajectory, fp64 carry, 5 frames", lambda: md.trajectory(None, None, [1, 10, n // 2, n - 1, n], num_steps=n, state=state)),
                 ("trajectory, fp64 carry, a frame every step", lambda: md.trajectory(None, None, np.arange(1, n + 1), num_steps=n, state=state))]
        for what, fn in cases:
            med, best = timed(fn)
            print(f"{label} x {rows} rows, {n} steps per launch: {what:44s} median {med:9.3f} ms  min {best:9.3f} ms  = {med / n * 1e3:9.2f} us per step", flush=True)

# what the cut into launches costs the driver: alanine dipeptide, 20000 sampling steps, logarithmic spacing of 1000
_, coords, masses = synthetic.alanine_dipeptide_state()
energy = AmberPotentialEnergyTorch.alanine_dipeptide()
x = coords.to(dev)[None].contiguous()
for per_launch in (10, 100, 1000, 10000):
    def run():
        S.simulate_trajectory(energy, masses, x, burn_in=0, sampling=20000, spacing=S.LogarithmicSpacing(1000, 10), seed=2, steps_per_launch=per_launch)
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"simulate_trajectory, alanine dipeptide x 1 row, 20000 steps, steps_per_launch {per_launch:5d}: {dt * 1e3:9.1f} ms = {dt / 20000 * 1e6:7.2f} us per step", flush=True)
