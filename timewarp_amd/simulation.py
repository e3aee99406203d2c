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

Checkpoint and resume (the reference's simulation/checkpointing.py, `--cpmins`, default 5 minutes there; off by default
here so that the default call writes what it always wrote): `simulate_trajectory(checkpoint=BASE, ...)` writes the frames out
in segments, keeps a checkpoint of the fp64 state, the integrator's absolute step (the noise key) and the report steps, and a
call that finds the checkpoint continues from it - in another process, with other launch and segment sizes - to the files of
the uninterrupted run, bit for bit.  `max_steps` / `max_seconds` (`--max-steps`, `--max-minutes`) stop a run cleanly for a job
with a time limit; the command line then exits with 3 and the same command continues.  Checkpoints fall between launches;
there is no background thread, and the minimiser is not checkpointed mid-run.

The reference's burn-in is one step short (`simulation.step(burnin_steps - 1)`, :201), so with a burn-in its sampling starts
at `currentStep` = burn_in - 1 and its report steps are those of (burn_in - 1, burn_in - 1 + sampling]; here the burn-in runs
`burn_in` steps and the report steps are those of (burn_in, burn_in + sampling] - pass a burn-in one shorter for the
reference's own steps.  For LangevinMiddleIntegrator the recorded velocities (and E_kin) are by default the integrator's stored
half-step velocities; `velocities="full-step"` (`--full-step-velocities`) records v + (dt/2) F / m of the frame's own forces,
the shift OpenMM's getState applies before it reports (include/timewarp_hip.h; not compared with OpenMM, which is not
available here).  `constraints="h-bonds"` (`--constraints h-bonds`, usually with `--timestep-fs 2`) holds the bonds to hydrogen
fixed (`LangevinDynamics(constraints=)`): off by default, part of the fingerprint, not available with full-step velocities.  `--pdb FILE --force-field NAME` starts from a PDB file instead of the built-in alanine dipeptide.

    python -m timewarp_amd.simulation --preset alanine-dipeptide --burn-in 2000 --sampling 20000 --spacing 1000 \\
        --spacing-approach logarithmic --replicas 4 --minimize --redraw-velocities --out runs/ad
    python -m timewarp_amd.simulation --pdb 1hgv-traj-state0.pdb --burn-in 2000000 --sampling 20000000 --spacing 10000 \\
        --checkpoint-minutes 5 --max-minutes 55 --segment-frames 1000 --full-step-velocities --out runs/1hgv    # again until it exits 0
    python -m timewarp_amd.simulation --preset alanine-dipeptide --constraints h-bonds --timestep-fs 2 --minimize --burn-in 500 \\
        --sampling 5000 --out runs/ad-2fs
"""
from __future__ import annotations

import argparse
import glob
import hashlib
import json
import os
import time
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


# ---------------------------------------------------------------------------------------------
# checkpoints and segments
# ---------------------------------------------------------------------------------------------
CHECKPOINT_VERSION = 1
VELOCITIES = ("stored", "full-step")
# the fields of a run's fingerprint in the order they are compared: everything the frames depend on, nothing they do not
# (steps_per_launch, segment_frames and the checkpoint interval are free to change between the parts of a run)
FINGERPRINT_FIELDS = ("burn_in", "sampling", "seed", "noise_seed", "scheme", "dt", "friction", "kbT", "n_rows", "n_atoms", "force_field",
                      "masses", "start", "report_steps", "velocities", "redraw_velocities", "minimize", "min_tol", "constraints")


def checkpoint_path(base: str) -> str:
    return f"{base}.checkpoint.npz"


def segment_path(base: str, index: int) -> str:
    return f"{base}.segment-{int(index):06d}.npz"


def _digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def tables_digest(tables) -> str:
    """sha256 over every field of the force-field tables in name order: arrays with dtype and shape, scalars by their repr."""
    h = hashlib.sha256()
    for key in sorted(vars(tables)):
        value = vars(tables)[key]
        h.update(key.encode())
        if isinstance(value, (np.ndarray, torch.Tensor)):
            h.update(_digest(value.detach().cpu().numpy() if isinstance(value, torch.Tensor) else value).encode())
        else:
            h.update(repr(value).encode())
    return h.hexdigest()


def run_fingerprint(energy, md, x, velocs, *, burn_in, sampling, seed, reports, velocities, redraw_velocities, minimize, min_tol) -> dict:
    """Everything that defines a run's frames (`FINGERPRINT_FIELDS`).  `start` is a hash of the float32 state the caller
    passed in - the coordinates before any minimisation, and the velocities when they were given.  `constraints` is None for
    an unconstrained run (and for integrators that know nothing of constraints), else tolerance, max_sweeps and a digest of the
    cluster tables."""
    cons = getattr(md, "constraints", None)
    start = [x.detach().cpu().numpy()] + ([] if velocs is None else [velocs.detach().cpu().numpy()])
    return {"burn_in": int(burn_in), "sampling": int(sampling), "seed": int(seed), "noise_seed": int(md.seed), "scheme": int(md.scheme),
            "dt": float(md.dt), "friction": float(md.friction), "kbT": float(md.kbT), "n_rows": int(x.shape[0]),
            "n_atoms": int(x.shape[1]), "force_field": tables_digest(energy.tables),
            "masses": _digest(md.masses.detach().cpu().numpy()), "start": _digest(*start),
            "report_steps": [int(r) for r in reports], "velocities": str(velocities),
            "redraw_velocities": bool(redraw_velocities), "minimize": bool(minimize), "min_tol": float(min_tol) if minimize else None,
            "constraints": None if cons is None else cons.fingerprint()}


def _write_atomically(path: str, **arrays) -> None:
    """The arrays as an uncompressed npz under a temporary name, moved into place with `os.replace`: a reader finds the old
    file or the new one under `path`, never part of one."""
    tmp = f"{path}.tmp"
    try:
        with open(tmp, "wb") as f:
            np.savez(f, **arrays)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def write_checkpoint(path: str, fingerprint: dict, *, steps_done: int, integrator_step: int, state: np.ndarray, redrawn: bool,
                     n_segments: int, start_coords: np.ndarray) -> None:
    fp = dict(fingerprint)
    reports = np.asarray(fp.pop("report_steps"), dtype=np.int64)
    _write_atomically(path, version=np.int64(CHECKPOINT_VERSION), fingerprint=np.array(json.dumps(fp, sort_keys=True)),
                      steps_done=np.int64(steps_done), integrator_step=np.int64(integrator_step),
                      state=np.ascontiguousarray(state, dtype=np.float64), redrawn=np.bool_(redrawn), n_segments=np.int64(n_segments),
                      report_steps=reports, start_coords=np.ascontiguousarray(start_coords, dtype=np.float32))


def read_checkpoint(path: str) -> dict:
    """-> dict with `fingerprint` (report_steps included again), steps_done, integrator_step, state [N, 2, V, 3] float64,
    redrawn, n_segments, report_steps int64, start_coords [N, V, 3] float32.  ValueError for another format version."""
    with np.load(path) as z:
        version = int(z["version"])
        if version != CHECKPOINT_VERSION:
            raise ValueError(f"{path}: checkpoint format version {version}, this code reads version {CHECKPOINT_VERSION}")
        fp = json.loads(str(z["fingerprint"]))
        reports = z["report_steps"].astype(np.int64)
        fp["report_steps"] = [int(r) for r in reports]
        return {"fingerprint": fp, "steps_done": int(z["steps_done"]), "integrator_step": int(z["integrator_step"]),
                "state": z["state"], "redrawn": bool(z["redrawn"]), "n_segments": int(z["n_segments"]), "report_steps": reports,
                "start_coords": z["start_coords"]}


def first_difference(saved: dict, now: dict) -> Optional[str]:
    """The first field of `FINGERPRINT_FIELDS` in which two fingerprints differ, or None."""
    for key in FINGERPRINT_FIELDS:
        if saved.get(key) != now.get(key):
            return key
    return None


def write_segment(path: str, frames: List) -> int:
    """The buffered frames of all rows as one file: `step` [T] and, per row r, `positions_r`, `velocities_r`, `forces_r`
    float32 [T, V, 3] and `energies_r` float64 [T, 2] - a member per row, so that assembling a row reads that row only."""
    step = np.concatenate([f.step for f in frames]).astype(np.int64)
    arrays = {"step": step}
    for key in ("positions", "velocities", "forces", "energies"):
        host = torch.cat([getattr(f, key) for f in frames], dim=1).cpu().numpy()      # one copy per key: [N, T, ...]
        for r in range(host.shape[0]):
            arrays[f"{key}_{r}"] = host[r]
    _write_atomically(path, **arrays)
    return int(step.size)


def assemble_row(base: str, n_segments: int, row: int, dt: float) -> dict:
    """Row `row` of segments 0 .. n_segments - 1 in the reporter's layout: what `frame_arrays` gives for the same frames."""
    parts = {k: [] for k in ("step", "energies", "positions", "velocities", "forces")}
    for i in range(n_segments):
        with np.load(segment_path(base, i)) as z:
            parts["step"].append(z["step"])
            for key in ("energies", "positions", "velocities", "forces"):
                parts[key].append(z[f"{key}_{row}"])
    step = np.concatenate(parts["step"]).astype(np.int64)
    return {"step": step, "time": step.astype(np.float64) * dt,
            "energies": np.concatenate(parts["energies"]).astype(np.float64),
            "positions": np.concatenate(parts["positions"]).astype(np.float32),
            "velocities": np.concatenate(parts["velocities"]).astype(np.float32),
            "forces": np.concatenate(parts["forces"]).astype(np.float32)}


def next_launch(done: int, burn_in: int, total: int, reports: np.ndarray, steps_per_launch: int, stop_at: Optional[int] = None,
                room: Optional[int] = None) -> Tuple[int, np.ndarray]:
    """The launch that follows `done` steps as (number of steps, report steps relative to `done`): up to `steps_per_launch`
    steps, never across the burn-in / sampling boundary, never beyond `stop_at`, and - with `room` >= 1 - cut at the step of
    its `room`-th frame so that it records no more than that.  From step 0 without `stop_at` and `room` it walks the launches
    of `plan_launches`.  A pure function."""
    end = burn_in if done < burn_in else total
    b = min(done + steps_per_launch, end)
    if stop_at is not None:
        b = min(b, stop_at)
    mine = reports[(reports > done) & (reports <= b)]
    if room is not None and mine.size > room:
        mine = mine[:room]
        b = int(mine[-1])
    return b - done, mine - done


def simulate_trajectory(energy, masses, coords, velocs=None, *, burn_in: int, sampling: int, spacing: Optional[Spacing], integrator=None,
                        seed: int = 0, steps_per_launch: int = 50, out_dir: Optional[str] = None, name: str = "traj",
                        minimize: bool = False, min_tol: float = 2.0, redraw_velocities: bool = False, minimization_log=None,
                        velocities: str = "stored", checkpoint: Optional[str] = None, checkpoint_steps: Optional[int] = None,
                        checkpoint_seconds: Optional[float] = None, segment_frames: Optional[int] = None,
                        max_steps: Optional[int] = None, max_seconds: Optional[float] = None, keep_segments: bool = False,
                        stats: Optional[dict] = None, constraints=None, constraint_tolerance: Optional[float] = None):
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
    reference.  Without `minimize` no minimisation happens: pass a relaxed state.

    `velocities`: "stored" (the frames of before) or "full-step" (`LangevinDynamics.trajectory(velocities=)`).

    Checkpoint and resume.  With every argument below at its default nothing new is written and the call is the call of
    before.  `checkpoint`: a path base; the run keeps `<base>.checkpoint.npz` and `<base>.segment-NNNNNN.npz` beside it.
      segments   At most `segment_frames` frames per replica are held on the device (launches are cut at the frame that fills
                 the buffer); a full buffer is copied to the host and written as a segment, all rows in one file.  Without
                 `segment_frames` the buffer is flushed at checkpoints only.  Segments go to the checkpoint base, or without
                 one to `<out_dir>/<name>`.  At completion the rows are assembled from the segments one row at a time: the
                 arrays, and the files, of the same run made without segments, bit for bit.
      checkpoint every `checkpoint_steps` steps and / or `checkpoint_seconds` of wall time, between launches, and whenever
                 `max_steps` / `max_seconds` stop the run.  The frame buffer is flushed as a segment first; then one file: format
                 version, fingerprint, steps done, the integrator's absolute step (the noise key), the fp64 state
                 [N, 2, V, 3], whether the velocity redraw has happened, the number of segments, the report steps computed
                 before the first launch (so a stateful policy never has to be restored) and the coordinates the run
                 started from.  Every file is written under a temporary name and moved into place with `os.replace`.  A
                 state that is not finite is never written: RuntimeError names the replicas and the previous checkpoint stays.
      resume     a call that finds `<base>.checkpoint.npz` continues from it: no minimisation, no initial draw, no second
                 redraw; `spacing` may then be None.  The fingerprint (`FINGERPRINT_FIELDS`: burn-in, sampling, seeds,
                 scheme, dt, friction, kbT, rows, atoms, hashes of tables, masses and the passed-in state, the report steps,
                 `velocities`, `redraw_velocities`, `minimize`, `min_tol`) must be the saved one: otherwise ValueError names
                 the first field that differs and nothing is touched.  `steps_per_launch`, `segment_frames` and the
                 intervals may change.  Segment files numbered at or beyond the checkpoint's count are leftovers of an
                 interrupted write and are overwritten.  Without a checkpoint file the run starts at step 0.
      `max_steps` / `max_seconds`: run at most that many further steps / stop after the launch that passes that wall time,
                 checkpoint, and return None (they need `checkpoint`).
      completion the final files are written, then checkpoint and segments are removed unless `keep_segments`.
    `constraints`: None (the default: the run of before), "h-bonds" or a `forcefield.HBondConstraints` - the default integrator is
    then built with them (`LangevinDynamics(constraints=, constraint_tolerance=)`); an `integrator` passed in brings its own.
    Constrained dynamics samples another ensemble (X-H lengths fixed) and usually runs at 2 fs.  The fp64 state is projected onto
    the constraints (`apply_constraints`) once before the first launch - positions after the optional minimisation, velocities
    after the draw - and the velocities again after the redraw.  Wherever the driver waits for the device anyway (a segment
    flush, a checkpoint, the end) the largest residual any launch since then reported is compared with the tolerance: a row
    above it raises RuntimeError naming row and residual, and such a state is never checkpointed.  The constraints are part of
    the fingerprint: a checkpoint of a run with others is refused as `constraints`.  Full-step velocities are not available.
    `stats`: a dict that receives `max_buffered_frames` (the most frames per replica the device buffer ever held, from the
    buffers' shapes), `segments`, `checkpoints`, `resumed_at` (step or None), `steps_done`, `start_coords` ([N, V, 3] float32:
    where the MD started, after the minimisation when there was one)."""
    from .md import LangevinDynamics, minimize_energy

    if velocities not in VELOCITIES:
        raise ValueError(f"velocities {velocities!r}: expected one of {list(VELOCITIES)}")
    if (max_steps is not None or max_seconds is not None) and checkpoint is None:
        raise ValueError("max_steps / max_seconds stop a run to be continued later: they need checkpoint=")
    if max_steps is not None and max_steps < 0:
        raise ValueError("max_steps must not be negative")
    if segment_frames is not None and segment_frames < 1:
        raise ValueError("segment_frames must be at least 1")
    if checkpoint_steps is not None and checkpoint_steps < 1:
        raise ValueError("checkpoint_steps must be at least 1")
    segmented = checkpoint is not None or segment_frames is not None
    base = checkpoint if checkpoint is not None else (os.path.join(out_dir, name) if out_dir is not None else None)
    if segmented and base is None:
        raise ValueError("segment_frames needs somewhere to write the segments: checkpoint= or out_dir=")
    saved = read_checkpoint(checkpoint_path(checkpoint)) if checkpoint is not None and os.path.exists(checkpoint_path(checkpoint)) else None
    if spacing is None and saved is None:
        raise ValueError("spacing may be None only when the run continues from a checkpoint")
    reports = report_steps(spacing, burn_in, burn_in + sampling) if spacing is not None else saved["report_steps"]
    if reports.size == 0:       # known before the first launch: do not integrate a run that records nothing
        raise ValueError(f"the spacing policy reports no step in ({burn_in}, {burn_in + sampling}]: nothing would be recorded")
    if integrator is not None and constraints is not None and getattr(integrator, "constraints", None) is None:
        raise ValueError("constraints= builds the default integrator with them; an integrator= passed in brings its own "
                         "(LangevinDynamics(..., constraints=))")
    if constraint_tolerance is not None and constraints is None:
        raise ValueError("constraint_tolerance needs constraints=")
    if integrator is not None:
        md = integrator
    elif constraints is not None:
        md = LangevinDynamics.for_energy(energy, masses, seed=seed, constraints=constraints, constraint_tolerance=constraint_tolerance)
    else:
        md = LangevinDynamics.for_energy(energy, masses, seed=seed)
    cons = getattr(md, "constraints", None)
    worst_residual = None       # [N] on the device: the largest residual of any launch since the last look
    V = energy.tables.n_atoms
    x = coords.reshape(-1, V, 3).to(torch.float32)
    n = x.shape[0]
    total = burn_in + sampling
    fingerprint = None
    if checkpoint is not None:
        fingerprint = run_fingerprint(energy, md, x, None if velocs is None else velocs.reshape(-1, V, 3).to(torch.float32), burn_in=burn_in,
                                      sampling=sampling, seed=seed, reports=reports, velocities=velocities,
                                      redraw_velocities=redraw_velocities, minimize=minimize, min_tol=min_tol)
    if saved is not None:
        field = first_difference(saved["fingerprint"], fingerprint)
        if field is not None:
            show = (lambda v: f"{len(v)} steps {v[:4]}..." if isinstance(v, list) and len(v) > 4 else repr(v))
            raise ValueError(f"{checkpoint_path(checkpoint)} belongs to another run: `{field}` was {show(saved['fingerprint'].get(field))} and is "
                             f"now {show(fingerprint.get(field))}; nothing was changed")
        done, n_segments, redrawn = saved["steps_done"], saved["n_segments"], saved["redrawn"]
        start_coords = saved["start_coords"]
        state = torch.from_numpy(saved["state"]).to(x.device).contiguous()
        start = saved["integrator_step"] - done
        if hasattr(md, "continued_at"):
            md.continued_at(saved["integrator_step"])
        else:
            md.steps_done = saved["integrator_step"]
    else:
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
        start = md.steps_done
        state = md.new_state(x, v)
        if cons is not None:        # positions (after the minimisation) and the drawn velocities onto the constraints, in fp64
            md.apply_constraints(None, state=state)
            worst_residual = md.constraint_residual
            x = state[:, 0].to(torch.float32)
        done, n_segments, redrawn = 0, 0, not redraw_velocities
        start_coords = None
    if stats is not None:
        stats.update(max_buffered_frames=0, segments=0, checkpoints=0, resumed_at=None if saved is None else done, steps_done=done)
    stop_at = total if max_steps is None else min(total, done + int(max_steps))
    frames, buffered = [], 0
    began = last_time = time.monotonic()
    last_step = done

    def check_constraints():
        nonlocal worst_residual
        if cons is None or worst_residual is None:
            return
        res = worst_residual.cpu().numpy()
        worst_residual = None
        bad = np.flatnonzero(~(res <= cons.tolerance))
        if bad.size:
            raise RuntimeError(f"constraints not met after {done} steps: " + ", ".join(f"row {r} residual {res[r]:.3e}" for r in bad) +
                               f" (tolerance {cons.tolerance:.3e}, max_sweeps {cons.max_sweeps}); nothing was written for this state")

    def flush():
        nonlocal frames, buffered, n_segments
        if frames:
            check_constraints()
            os.makedirs(os.path.dirname(os.path.abspath(base)), exist_ok=True)
            write_segment(segment_path(base, n_segments), frames)
            n_segments += 1
            frames, buffered = [], 0
            if stats is not None:
                stats["segments"] += 1

    def save_checkpoint():
        nonlocal last_time, last_step
        check_constraints()
        finite = torch.isfinite(state).reshape(n, -1).all(dim=1).cpu().numpy()
        if not finite.all():
            raise RuntimeError(f"the state of replica(s) {', '.join(str(r) for r in np.flatnonzero(~finite))} is not finite after {done} steps: "
                               "no checkpoint was written" + (" and the previous one is left in place" if os.path.exists(checkpoint_path(checkpoint)) else ""))
        flush()
        os.makedirs(os.path.dirname(os.path.abspath(checkpoint)), exist_ok=True)
        write_checkpoint(checkpoint_path(checkpoint), fingerprint, steps_done=done, integrator_step=md.steps_done, state=state.cpu().numpy(),
                         redrawn=redrawn, n_segments=n_segments, start_coords=start_coords)
        last_time, last_step = time.monotonic(), done
        if stats is not None:
            stats["checkpoints"] += 1

    while done < stop_at:
        room = None if segment_frames is None else segment_frames - buffered
        n_steps, rel = next_launch(done, burn_in, total, reports, steps_per_launch, stop_at, room)
        if not redrawn and done >= burn_in:      # the first sampling launch
            gen = torch.Generator(device=x.device)
            gen.manual_seed(velocity_seeds(seed)[1])
            state[:, 1] = thermal_velocities(md.masses, md.kbT, x, gen).to(torch.float64)
            if cons is not None:
                md.apply_constraints(None, state=state)
            redrawn = True
        kind = {} if velocities == "stored" else {"velocities": velocities}
        _, _, f = md.trajectory(None, None, rel, num_steps=n_steps, state=state, **kind)      # from the carry alone: no comparison, no wait
        done += n_steps
        if cons is not None and getattr(md, "constraint_residual", None) is not None:
            worst_residual = md.constraint_residual if worst_residual is None else torch.maximum(worst_residual, md.constraint_residual)
        if start_coords is None and segmented:      # the first launch has been accepted: from here on files may appear
            start_coords = x.cpu().numpy()
        if rel.size:
            f.step = f.step - start          # steps of THIS run, whatever the integrator had done before
            f.time = f.step.astype(np.float64) * md.dt
            frames.append(f)
            buffered += int(f.positions.shape[1])
            if stats is not None:
                stats["max_buffered_frames"] = max(stats["max_buffered_frames"], sum(int(g.positions.shape[1]) for g in frames))
        if stats is not None:
            stats["steps_done"] = done
        if segment_frames is not None and buffered >= segment_frames:
            flush()
        if checkpoint is not None and done < total:
            now = time.monotonic()
            out_of_time = max_seconds is not None and now - began >= max_seconds
            if out_of_time or done >= stop_at or (checkpoint_steps is not None and done - last_step >= checkpoint_steps) or \
                    (checkpoint_seconds is not None and now - last_time >= checkpoint_seconds):
                save_checkpoint()
            if out_of_time:
                return None
    if done < total:       # stopped by max_steps
        if checkpoint is not None and last_step != done:
            save_checkpoint()
        return None
    check_constraints()
    if stats is not None:
        stats["start_coords"] = x.cpu().numpy() if start_coords is None else start_coords
    if segmented:
        flush()
        rows = [assemble_row(base, n_segments, r, md.dt) for r in range(n)]
    else:
        rows = [frame_arrays(frames, r) for r in range(n)]
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        for r, arrays in enumerate(rows):
            np.savez_compressed(trajectory_path(out_dir, name, r, n), **arrays)
    if segmented and not keep_segments:
        leftovers = glob.glob(glob.escape(base) + ".segment-*.npz")
        for path in leftovers + ([checkpoint_path(checkpoint)] if checkpoint is not None else []):
            if os.path.exists(path):
                os.remove(path)
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


def pdb_system(path: str, force_field: str = "amber99-implicit"):
    """(energy, masses [V], starting coords [V, 3] in nm, the file's ATOM / HETATM lines) of a PDB file - one of the reference's own
    `*-traj-state0.pdb` files, say.  Topology: `forcefield.read_pdb_topology`; coordinates: the fixed columns 31-54 in angstrom,
    times 0.1; masses: `forcefield.ELEMENT_MASSES` by the element column (77-78) or, where that is empty, the first letter of the
    atom name; energy: `AmberPotentialEnergyTorch.from_preset(force_field, ...)`, `force_field` a key of
    `forcefield.PRESET_FAMILY`.  SystemExit names what cannot be simulated: an unknown force field, a residue without a
    template, atoms that do not match their residue's template (a file without hydrogens), an element without a mass."""
    from .energy import AmberPotentialEnergyTorch
    from .forcefield import ELEMENT_MASSES, PRESET_FAMILY, read_pdb_topology

    if force_field not in PRESET_FAMILY:
        raise SystemExit(f"--force-field {force_field}: expected one of {sorted(PRESET_FAMILY)}")
    try:
        names, residues, ids = read_pdb_topology(path)
    except (OSError, ValueError) as e:
        raise SystemExit(f"--pdb {path}: {e}")
    if not names:
        raise SystemExit(f"--pdb {path}: no ATOM or HETATM record")
    lines, xyz, masses = [], [], []
    with open(path) as f:
        for line in f:
            if line.startswith(("ATOM", "HETATM")):
                lines.append(line.rstrip("\n"))
                try:
                    xyz.append([0.1 * float(line[30:38]), 0.1 * float(line[38:46]), 0.1 * float(line[46:54])])
                except ValueError:
                    raise SystemExit(f"--pdb {path}: no coordinates in columns 31-54 of {line.rstrip()!r}")
                element = line[76:78].strip().capitalize() or line[12:16].strip()[:1]
                if element not in ELEMENT_MASSES:
                    raise SystemExit(f"--pdb {path}: atom {line[12:16].strip()} of residue {line[17:20].strip()} {line[22:26].strip()}: no mass "
                                     f"for element {element!r} (have {sorted(ELEMENT_MASSES)})")
                masses.append(ELEMENT_MASSES[element])
    try:
        energy = AmberPotentialEnergyTorch.from_preset(force_field, names, residues, ids)
    except NotImplementedError as e:       # a residue without a template: the message names it
        raise SystemExit(f"--pdb {path}: {e}")
    except ValueError as e:                # atoms that are not the template's - missing hydrogens, most often
        raise SystemExit(f"--pdb {path}: {e}; the file must hold every atom of the force field's residue templates, hydrogens included")
    return energy, torch.tensor(masses, dtype=torch.float32), torch.tensor(xyz, dtype=torch.float32), lines


def write_state0_pdb(path: str, atom_lines: List[str], coords_nm, remark: str) -> None:
    """The input's ATOM / HETATM records with the coordinates `coords_nm` [V, 3] in columns 31-54 (angstrom), after a REMARK
    that says which state they are: the topology file `python -m timewarp_amd.analysis --pdb` takes.  Written atomically."""
    xyz = np.asarray(coords_nm, dtype=np.float64).reshape(-1, 3) * 10.0
    if len(atom_lines) != xyz.shape[0]:
        raise ValueError("one coordinate triple per ATOM record")
    tmp = f"{path}.tmp"
    with open(tmp, "w") as f:
        f.write(f"REMARK   {remark}\n")
        for line, (a, b, c) in zip(atom_lines, xyz):
            line = line.ljust(54)
            f.write(f"{line[:30]}{a:8.3f}{b:8.3f}{c:8.3f}{line[54:]}\n")
        f.write("END\n")
    os.replace(tmp, path)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m timewarp_amd.simulation", description=__doc__.split("\n\n")[0])
    ap.add_argument("--preset", default="alanine-dipeptide")
    ap.add_argument("--pdb", default=None, help="start from this PDB file (all atoms, hydrogens included) instead of a preset")
    ap.add_argument("--force-field", default="amber99-implicit", help="with --pdb: a dataset or preset name of forcefield.PRESET_FAMILY")
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
    ap.add_argument("--full-step-velocities", action="store_true", help="record velocities moved to the full step: v + (dt/2) F / m")
    ap.add_argument("--checkpoint-minutes", type=float, default=0.0,
                    help="checkpoint every M minutes of wall time; 0 (the default) = off (the reference's --cpmins defaults to 5)")
    ap.add_argument("--max-minutes", type=float, default=None, help="stop cleanly with a checkpoint after M minutes; the same command continues")
    ap.add_argument("--max-steps", type=int, default=None, help="stop cleanly with a checkpoint after K further steps; the same command continues")
    ap.add_argument("--constraints", choices=["none", "h-bonds"], default="none",
                    help="hold the bonds to hydrogen at their equilibrium lengths (off by default; usually with --timestep-fs 2)")
    ap.add_argument("--constraint-tolerance", type=float, default=None, help="relative to the squared bond length (default 1e-8)")
    ap.add_argument("--timestep-fs", type=float, default=None, help="integration step in fs (default: the preset's 0.5)")
    ap.add_argument("--segment-frames", type=int, default=None, help="hold at most F frames per replica on the device, write the rest out as segments")
    return ap


def main(argv=None, device="cuda") -> int:
    """`device`: where the replicas are put; anything but a GPU is refused by the integrator (there is no CPU path).

    Returns 0 when the run is complete and 3 when `--max-minutes` / `--max-steps` stopped it with a checkpoint (one line says at
    which step; the same command continues it).  A checkpoint `<out>/<name>.checkpoint.npz` is kept when any of
    `--checkpoint-minutes`, `--max-minutes`, `--max-steps` is given; `--checkpoint-minutes` defaults to 0 = off so that the
    default command writes what it always wrote (the reference's default is 5 minutes).  With `--pdb` the name is the file's
    stem and `<name>-traj-state0.pdb` is written at completion: the input's ATOM records with the coordinates the MD started
    from - after the minimisation when there was one -, the topology file `python -m timewarp_amd.analysis --pdb` takes.  Which
    state the reference writes into its own `*-traj-state0.pdb` was not checked."""
    args = build_parser().parse_args(argv)
    if args.replicas < 1:
        raise SystemExit("--replicas must be at least 1")
    if args.checkpoint_minutes < 0 or (args.max_minutes is not None and args.max_minutes < 0) or (args.max_steps is not None and args.max_steps < 0):
        raise SystemExit("--checkpoint-minutes, --max-minutes and --max-steps must not be negative")
    atom_lines = None
    if args.pdb is not None:
        energy, masses, coords, atom_lines = pdb_system(args.pdb, args.force_field)
        name = os.path.splitext(os.path.basename(args.pdb))[0]
    else:
        energy, masses, coords = preset_system(args.preset)
        name = args.preset
    x = coords.to(torch.float32).to(device)[None].repeat(args.replicas, 1, 1)
    log, stats, extra = [], {}, {}
    if args.full_step_velocities:
        extra["velocities"] = "full-step"
    if args.segment_frames is not None:
        extra["segment_frames"] = args.segment_frames
    if args.checkpoint_minutes > 0 or args.max_minutes is not None or args.max_steps is not None:
        extra["checkpoint"] = os.path.join(args.out, name)
        if args.checkpoint_minutes > 0:
            extra["checkpoint_seconds"] = 60.0 * args.checkpoint_minutes
        if args.max_minutes is not None:
            extra["max_seconds"] = 60.0 * args.max_minutes
        if args.max_steps is not None:
            extra["max_steps"] = args.max_steps
    if atom_lines is not None or "checkpoint" in extra:
        extra["stats"] = stats
    if args.timestep_fs is not None and not args.timestep_fs > 0:
        raise SystemExit("--timestep-fs must be positive")
    if args.constraint_tolerance is not None and args.constraints == "none":
        raise SystemExit("--constraint-tolerance needs --constraints h-bonds")
    if args.timestep_fs is not None or args.constraints != "none":
        from .md import LangevinDynamics

        kw = {} if args.timestep_fs is None else {"timestep_ps": 1e-3 * args.timestep_fs}
        if args.constraints != "none":
            kw.update(constraints=args.constraints, constraint_tolerance=args.constraint_tolerance)
        extra["integrator"] = LangevinDynamics.for_energy(energy, masses, seed=args.seed, **kw)
    rows = simulate_trajectory(energy, masses, x, burn_in=args.burn_in, sampling=args.sampling,
                               spacing=make_spacing(args.spacing_approach, args.spacing, args.seed), seed=args.seed,
                               out_dir=args.out, name=name, minimize=args.minimize, min_tol=args.min_tol,
                               redraw_velocities=args.redraw_velocities, minimization_log=log, **extra)
    for res, e0 in log:
        for r in range(len(res.status)):
            print(f"minimised replica {r}: {int(res.iterations[r])} iterations, {int(res.evaluations[r])} force evaluations, "
                  f"E {float(e0[r]):.3f} -> {float(res.energy[r]):.3f} kJ/mol, RMS force {float(res.rms_force[r]):.3f} kJ/mol/nm")
    if rows is None:
        print(f"stopped after step {stats.get('steps_done', '?')} of {args.burn_in + args.sampling} with a checkpoint at "
              f"{checkpoint_path(extra['checkpoint'])}: the same command continues the run")
        return 3
    if atom_lines is not None and "start_coords" in stats:
        write_state0_pdb(os.path.join(args.out, f"{name}-traj-state0.pdb"), atom_lines, stats["start_coords"][0],
                         "the state the MD run started from" + (f": after the energy minimisation to an RMS force of {args.min_tol} kJ/mol/nm"
                                                                if args.minimize else " (the input coordinates; no minimisation)"))
    for r, arrays in enumerate(rows):
        e = arrays["energies"]
        print(f"{trajectory_path(args.out, name, r, len(rows))}: {len(arrays['step'])} frames, steps {arrays['step'][0]} .. "
              f"{arrays['step'][-1]}, <E_pot> {e[:, 0].mean():.2f} <E_kin> {e[:, 1].mean():.2f} kJ/mol")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
