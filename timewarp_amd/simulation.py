"""Plain MD trajectories on the device in the reference's `*-traj-arrays.npz` frame format: the stand-in for
simulation/simulate_trajectory.py (burn-in, then `--sampling` steps, :198-250) with the NPZReporter of
simulation/npzreporter.py:196-293, both of which go through OpenMM.  Here the integration and the recording are one HIP
kernel (`LangevinDynamics.trajectory` -> `tw_langevin_trajectory`): a frame of positions, velocities, forces and
[E_pot, E_kin] at every report step of a spacing policy, no host round trip per frame, and - the fp64 state is carried
between launches - a trajectory that does not depend on where the launches or the frames fall.

Opt-in, as the reference does them around that run: `minimize=True` relaxes every replica on the device before anything
moves (`md.minimize_energy` -> `tw_minimize`, to an RMS force of `min_tol` = 2 kJ/mol/nm, the reference's `--min-tol`;
simulate_trajectory.py:186-191 - it stops by OpenMM's rule and does not reproduce OpenMM's iterates), and
`redraw_velocities=True` draws the velocities again between burn-in and sampling (:204-205).  Both default to off: a caller
who passes a relaxed state (a frame of an existing trajectory, a conformation of a dataset) gets exactly the run of before.

What is NOT built: checkpointing (the reference's `--resume`).  And the reference's burn-in is one step short
(`simulation.step(burnin_steps - 1)`, :201), so with a burn-in its sampling starts at `currentStep` = burn_in - 1 and its
report steps are those of (burn_in - 1, burn_in - 1 + sampling]; here the burn-in runs `burn_in` steps and the report
steps are those of (burn_in, burn_in + sampling] - pass a burn-in one shorter for the reference's own steps.  For
LangevinMiddleIntegrator the recorded velocities (and E_kin) are the integrator's stored half-step velocities, not the
full-step ones OpenMM's getState reports (include/timewarp_hip.h).

    python -m timewarp_amd.simulation --preset alanine-dipeptide --burn-in 2000 --sampling 20000 --spacing 1000 \\
        --spacing-approach logarithmic --replicas 4 --minimize --redraw-velocities --out runs/ad
"""
from __future__ import annotations

import argparse
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

# ---------------------------------------------------------------------------------------------
# spacing policies: "how many steps from step c to the next report" (simulation/npzreporter.py:17-193)
# ---------------------------------------------------------------------------------------------


class Spacing:
    """A policy answers `steps_until_next_report(current_step)` >= 1 (npzreporter.py:17-21); OpenMM asks it again at every
    report, so the report steps after `start` are start + d(start), then that + d(that), ..."""

    def steps_until_next_report(self, current_step: int) -> int:
        raise NotImplementedError


class RegularSpacing(Spacing):
    """Every multiple of `report_interval` (npzreporter.py:24-41): from step c the next report is the next multiple above c."""

    def __init__(self, report_interval: int):
        if report_interval < 1:
            raise ValueError("report_interval must be at least 1")
        self.report_interval = int(report_interval)

    def steps_until_next_report(self, current_step: int) -> int:
        return self.report_interval - int(current_step) % self.report_interval


class LogarithmicSpacing(Spacing):
    """Within every block of `report_interval` steps the offsets 0, 1, f, f^2, ... below the interval, f = `space_factor`
    (npzreporter.py:44-87): with 10000 and 10 the steps 10000, 10001, 10010, 10100, 11000, 20000, 20001, ...  From offset o
    of a block the next report is at the smallest power of f above o, or at the start of the next block if that comes first."""

    def __init__(self, report_interval: int, space_factor: int = 10):
        if space_factor <= 1:
            raise ValueError("space_factor must be larger than one")
        if report_interval < 1:
            raise ValueError("report_interval must be at least 1")
        self.report_interval, self.space_factor = int(report_interval), int(space_factor)

    def steps_until_next_report(self, current_step: int) -> int:
        offset = int(current_step) % self.report_interval
        power = 1
        while power <= offset:
            power *= self.space_factor
        return min(power, self.report_interval) - offset


class UniformWindowedSpacing(Spacing):
    """Around every multiple of `report_interval` the multiple itself and `subsamples` distinct steps drawn uniformly from
    the window [-spacing_window, spacing_window) around it (npzreporter.py:90-193).  Stateful, like the reference's: each
    window's offsets are drawn when the previous window is used up - `numpy.random.RandomState(seed).choice` over the
    2 * spacing_window offsets with offset 0 given weight zero, 0 appended, sorted - and queries must come with increasing
    steps.  With the same seed it reports the reference's steps on the walk a simulation takes - asked at the start and then
    at every step it reported, which is what `report_steps` does and what tests/golden/spacing_steps.npz pins.  Other query
    sequences are not promised to match: the reference compares each query with the previous one AFTER wrapping that one
    into its window (npzreporter.py:147-151), this class compares the steps themselves, so a sequence can be refused by
    one and answered by the other."""

    def __init__(self, report_interval: int, spacing_window: int = 100, subsamples: int = 10, seed: Optional[int] = None):
        self.report_interval, self.spacing_window, self.subsamples = int(report_interval), int(spacing_window), int(subsamples)
        if not self.subsamples < 2 * self.spacing_window:
            raise ValueError("subsamples must be fewer than the 2 * spacing_window steps of a window")
        if not self.report_interval >= 2 * self.spacing_window:
            raise ValueError("windows of neighbouring report steps must not overlap: report_interval >= 2 * spacing_window")
        self.rng = np.random.RandomState(seed)
        self._weights = np.ones(2 * self.spacing_window)
        self._weights[self.spacing_window] = 0.0      # offset 0 is always kept, never drawn
        self._weights /= self._weights.sum()
        self._offsets = self._draw()
        self._last_query = None
        self._ahead = False       # the offsets are already those of the NEXT window while steps of this one are still asked about

    def _draw(self) -> np.ndarray:
        drawn = self.rng.choice(2 * self.spacing_window, self.subsamples, replace=False, p=self._weights) - self.spacing_window
        return np.sort(np.concatenate((drawn, np.array([0], dtype=int))))

    def steps_until_next_report(self, current_step: int) -> int:
        current_step = int(current_step)
        if self._last_query is not None and current_step <= self._last_query:
            raise ValueError("UniformWindowedSpacing must be asked about increasing steps")
        self._last_query = current_step
        interval, half = self.report_interval, self.report_interval // 2
        rel = (current_step + half) % interval - half      # position relative to the nearest multiple: [-half, interval - half)
        if rel > 0 and self._ahead:
            # past the centre of a window whose successor is drawn already: the next report is the first of the successor
            return int(self._offsets[0]) - (rel - interval)
        self._ahead = False
        i = int(np.searchsorted(self._offsets, rel, side="left"))
        if i < len(self._offsets) and self._offsets[i] == rel:
            i += 1                                           # standing on a kept step: the one after it
        if i >= len(self._offsets):
            self._offsets = self._draw()
            self._ahead = True
            return int(self._offsets[0]) - (rel - interval)
        return int(self._offsets[i]) - rel


def report_steps(spacing: Spacing, start: int, stop: int) -> np.ndarray:
    """The absolute report steps in (start, stop] of a simulation that stands at step `start` and runs to `stop`, asking
    the policy after every report as OpenMM's Simulation does (describeNextReport, npzreporter.py:235-237).  `start`
    itself is never reported; `stop` is when the policy names it.  int64."""
    out, c = [], int(start)
    while True:
        d = int(spacing.steps_until_next_report(c))
        if d < 1:
            raise ValueError(f"{type(spacing).__name__} answered {d} steps at step {c}")
        c += d
        if c > stop:
            return np.asarray(out, dtype=np.int64)
        out.append(c)


def make_spacing(approach: str, interval: int, seed: Optional[int] = None) -> Spacing:
    """The policies as simulate_trajectory.py:208-232 builds them (factor 10; window 200 with 10 subsamples), plus "regular"."""
    if approach == "regular":
        return RegularSpacing(interval)
    if approach == "logarithmic":
        return LogarithmicSpacing(interval, 10)
    if approach == "windowed":
        return UniformWindowedSpacing(interval, spacing_window=200, subsamples=10, seed=seed)
    raise ValueError(f"spacing approach {approach!r}: expected regular, logarithmic or windowed")


# ---------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------
def plan_launches(burn_in: int, sampling: int, reports, steps_per_launch: int) -> List[Tuple[int, int, np.ndarray]]:
    """The launches of a run of `burn_in` + `sampling` steps as (first step, number of steps, report steps relative to the
    first step).  `reports`: absolute report steps in (burn_in, burn_in + sampling], increasing.  Burn-in launches report
    nothing; the sampling starts a launch of its own; a launch over steps (a, b] gets the reports in (a, b], each in
    exactly one launch.  No launch is longer than `steps_per_launch`.  A pure function."""
    burn_in, sampling, steps_per_launch = int(burn_in), int(sampling), int(steps_per_launch)
    if burn_in < 0 or sampling < 0 or steps_per_launch < 1:
        raise ValueError("burn_in and sampling must not be negative, steps_per_launch at least 1")
    reports = np.asarray(reports, dtype=np.int64).reshape(-1)
    total = burn_in + sampling
    if reports.size and (np.any(np.diff(reports) <= 0) or reports[0] <= burn_in or reports[-1] > total):
        raise ValueError("report steps must increase within (burn_in, burn_in + sampling]")
    plan = []
    for begin, end in ((0, burn_in), (burn_in, total)):
        a = begin
        while a < end:
            b = min(a + steps_per_launch, end)
            mine = reports[(reports > a) & (reports <= b)] - a
            plan.append((a, b - a, mine))
            a = b
    return plan


def thermal_velocities(masses: torch.Tensor, kbT: float, like: torch.Tensor, generator: Optional[torch.Generator] = None):
    """Maxwell-Boltzmann velocities (nm/ps) shaped like `like`: what `openmm_step` draws when it is given none
    (utils/evaluation_utils.py, setVelocitiesToTemperature)."""
    m = masses.to(device=like.device, dtype=like.dtype)
    noise = torch.randn(like.shape, dtype=like.dtype, device=like.device, generator=generator)
    return noise * (kbT / m).sqrt()[None, :, None]


def frame_arrays(frames: List, row: int) -> dict:
    """Row `row` of the frames of consecutive `trajectory` calls as the arrays the reference's reporter saves
    (npzreporter.py:275-293): step int64 [T], time float64 [T], energies float64 [T, 2], positions / velocities / forces
    float32 [T, V, 3]."""
    cat = lambda name: torch.cat([getattr(f, name)[row] for f in frames]).cpu().numpy()
    return {"step": np.concatenate([f.step for f in frames]).astype(np.int64),
            "time": np.concatenate([f.time for f in frames]).astype(np.float64),
            "energies": cat("energies").astype(np.float64),
            "positions": cat("positions").astype(np.float32),
            "velocities": cat("velocities").astype(np.float32),
            "forces": cat("forces").astype(np.float32)}


def velocity_seeds(seed: int) -> Tuple[int, int]:
    """The seeds of the two torch generators `simulate_trajectory` draws velocities from: (initial draw, redraw after the
    burn-in) = (seed mod 2^63, (seed XOR 0x9E3779B97F4A7C15) mod 2^63).  The constant's low bits are set, so the two differ
    for every seed."""
    return int(seed) & (2 ** 63 - 1), (int(seed) ^ 0x9E3779B97F4A7C15) & (2 ** 63 - 1)


def simulate_trajectory(energy, masses, coords, velocs=None, *, burn_in: int, sampling: int, spacing: Spacing, integrator=None,
                        seed: int = 0, steps_per_launch: int = 50, out_dir: Optional[str] = None, name: str = "traj",
                        minimize: bool = False, min_tol: float = 2.0, redraw_velocities: bool = False, minimization_log=None):
    """`burn_in` unrecorded steps, then `sampling` steps with a frame at every report step of `spacing` - the steps
    `report_steps(spacing, burn_in, burn_in + sampling)`, counted from the start of the run as the reference's
    `simulation.currentStep` is (its burn-in is one step short, so its steps are one lower: module docstring).  ValueError
    before anything runs if that is no step at all.  coords [N, V, 3] (nm, on the GPU): N independent replicas that share one seed and differ
    by their conformation index in the noise key.  Missing velocities are drawn at the energy's temperature (seeded by
    `seed`).  `integrator`: a `LangevinDynamics`, default the energy's own (`LangevinDynamics.for_energy`).

    The run is cut into launches of at most `steps_per_launch` steps with the fp64 state carried between them, so the
    frames do not depend on the cut - `steps_per_launch` only bounds how long one launch holds the device.  The default of
    50 keeps a launch of the 691-atom protein at 0.2 s (3.9 ms per step of the recording kernel measured on it) and costs
    alanine dipeptide (32 us per step) about 3 % against an uncut run (profiles/md_trajectory.txt).  That holds up to one
    replica per CU (256); a row is a workgroup, so more replicas of a large molecule take proportionally longer per launch.

    Returns a list of N dicts of numpy arrays in the reporter's layout (`frame_arrays`).  With `out_dir` each is also
    saved with `np.savez_compressed` as `<name>-traj-arrays.npz` (one row) or `<name>-<row>-traj-arrays.npz`.

    `minimize`: the replicas are first minimised to an RMS force of `min_tol` kJ/mol/nm (`md.minimize_energy` with its
    defaults otherwise) and the run starts from the float32 coordinates it returns - exactly the run of calling
    `minimize_energy` oneself and passing `result.coords`.  A row that stalled or whose start is not finite (status 2, 3)
    raises RuntimeError naming the rows before a single MD step runs.  The initial velocities are drawn after the
    minimisation, as the reference does.  `minimization_log`: a list that receives (result, starting energies [N]).
    `redraw_velocities`: between the last burn-in launch and the first sampling launch the velocity half of the fp64 state is
    overwritten with `thermal_velocities` (float32, like the initial draw) from a generator seeded with
    `velocity_seeds(seed)[1]`; the initial draw uses `velocity_seeds(seed)[0]`.  It happens with `burn_in=0` too, as in the
    reference.  Without `minimize` no minimisation happens: pass a relaxed state.  Checkpointing is not built."""
    from .md import LangevinDynamics, minimize_energy

    reports = report_steps(spacing, burn_in, burn_in + sampling)
    if reports.size == 0:       # known before the first launch: do not integrate a run that records nothing
        raise ValueError(f"the spacing policy reports no step in ({burn_in}, {burn_in + sampling}]: nothing would be recorded")
    md = integrator if integrator is not None else LangevinDynamics.for_energy(energy, masses, seed=seed)
    V = energy.tables.n_atoms
    x = coords.reshape(-1, V, 3).to(torch.float32)
    if minimize:
        e0 = energy.energy_and_forces(x)[0] if minimization_log is not None else None
        res = minimize_energy(energy, x, tolerance=min_tol)
        bad = [(r, int(st)) for r, st in enumerate(res.status.tolist()) if st in (2, 3)]
        if bad:
            raise RuntimeError("energy minimisation failed for row(s) " + ", ".join(
                f"{r} ({'stalled' if st == 2 else 'energy or forces not finite at the start'})" for r, st in bad) + "; no MD step was run")
        if minimization_log is not None:
            minimization_log.append((res, e0))
        x = res.coords.reshape(-1, V, 3)
    if velocs is None:
        gen = torch.Generator(device=x.device)
        gen.manual_seed(velocity_seeds(seed)[0])
        v = thermal_velocities(md.masses, md.kbT, x, gen)
    else:
        v = velocs.reshape(-1, V, 3).to(torch.float32)
    n = x.shape[0]
    start = md.steps_done
    state = md.new_state(x, v)
    frames = []
    redrawn = not redraw_velocities
    for first, n_steps, rel in plan_launches(burn_in, sampling, reports, steps_per_launch):
        if not redrawn and first >= burn_in:      # the first sampling launch
            gen = torch.Generator(device=x.device)
            gen.manual_seed(velocity_seeds(seed)[1])
            state[:, 1] = thermal_velocities(md.masses, md.kbT, x, gen).to(torch.float64)
            redrawn = True
        _, _, f = md.trajectory(None, None, rel, num_steps=n_steps, state=state)      # from the carry alone: no comparison, no wait
        if rel.size:
            f.step = f.step - start          # steps of THIS run, whatever the integrator had done before
            f.time = f.step.astype(np.float64) * md.dt
            frames.append(f)
    rows = [frame_arrays(frames, r) for r in range(n)]
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        for r, arrays in enumerate(rows):
            np.savez_compressed(trajectory_path(out_dir, name, r, n), **arrays)
    return rows


def trajectory_path(out_dir: str, name: str, row: int, n_rows: int) -> str:
    return os.path.join(out_dir, f"{name}-traj-arrays.npz" if n_rows == 1 else f"{name}-{row}-traj-arrays.npz")


# ---------------------------------------------------------------------------------------------
# command line (the reference's docopt interface is not reproduced)
# ---------------------------------------------------------------------------------------------
def preset_system(preset: str):
    """(energy, masses [V], starting coords [V, 3]) of a built-in system.  Only alanine dipeptide ships with tables and a
    conformation: the ideal-geometry coordinates of `synthetic.alanine_dipeptide_state()`, which are NOT minimised.  With
    `--minimize` (`simulate_trajectory(minimize=True)`) they are relaxed on the device first; without it the burn-in does the
    relaxing, and the command line's default of 2000 steps is there for that.  Other systems go through `simulate_trajectory`
    with the caller's own tables and state."""
    from . import synthetic
    from .energy import AmberPotentialEnergyTorch

    if preset != "alanine-dipeptide":
        raise SystemExit(f"--preset {preset}: only 'alanine-dipeptide' ships with tables and a starting conformation; call "
                         "timewarp_amd.simulation.simulate_trajectory with your own energy, masses and state for other systems")
    _, coords, masses = synthetic.alanine_dipeptide_state()
    return AmberPotentialEnergyTorch.alanine_dipeptide(), masses, coords


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m timewarp_amd.simulation", description=__doc__.split("\n\n")[0])
    ap.add_argument("--preset", default="alanine-dipeptide")
    ap.add_argument("--burn-in", type=int, default=2000)
    ap.add_argument("--sampling", type=int, default=20000)
    ap.add_argument("--spacing", type=int, default=1000, help="report interval in steps")
    ap.add_argument("--spacing-approach", choices=["regular", "logarithmic", "windowed"], default="logarithmic")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--replicas", type=int, default=1)
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--minimize", action="store_true", help="minimise the energy of every replica before the run (off by default)")
    ap.add_argument("--min-tol", type=float, default=2.0, help="RMS force at which the minimisation stops, kJ/mol/nm")
    ap.add_argument("--redraw-velocities", action="store_true", help="draw the velocities again between burn-in and sampling")
    return ap


def main(argv=None, device="cuda") -> int:
    """`device`: where the replicas are put; anything but a GPU is refused by the integrator (there is no CPU path)."""
    args = build_parser().parse_args(argv)
    if args.replicas < 1:
        raise SystemExit("--replicas must be at least 1")
    energy, masses, coords = preset_system(args.preset)
    x = coords.to(torch.float32).to(device)[None].repeat(args.replicas, 1, 1)
    log = []
    rows = simulate_trajectory(energy, masses, x, burn_in=args.burn_in, sampling=args.sampling,
                               spacing=make_spacing(args.spacing_approach, args.spacing, args.seed), seed=args.seed,
                               out_dir=args.out, name=args.preset, minimize=args.minimize, min_tol=args.min_tol,
                               redraw_velocities=args.redraw_velocities, minimization_log=log)
    for res, e0 in log:
        for r in range(len(res.status)):
            print(f"minimised replica {r}: {int(res.iterations[r])} iterations, {int(res.evaluations[r])} force evaluations, "
                  f"E {float(e0[r]):.3f} -> {float(res.energy[r]):.3f} kJ/mol, RMS force {float(res.rms_force[r]):.3f} kJ/mol/nm")
    for r, arrays in enumerate(rows):
        e = arrays["energies"]
        print(f"{trajectory_path(args.out, args.preset, r, len(rows))}: {len(arrays['step'])} frames, steps {arrays['step'][0]} .. "
              f"{arrays['step'][-1]}, <E_pot> {e[:, 0].mean():.2f} <E_kin> {e[:, 1].mean():.2f} kJ/mol")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
