"""Langevin dynamics on the HIP force kernel: the device-side stand-in for the `openmm.app.Simulation` the reference's
hybrid moves drive (`openmm_step`, utils/evaluation_utils.py:439-466; integrators of simulation/md.py:213-231 with the
preset parameters of md.py:75-93: 310 K, friction 0.3 / ps, time step 0.5 fs, LangevinMiddleIntegrator - LangevinIntegrator
for the oldest datasets).

`sample_with_model(..., openmm_on_current / openmm_on_proposal, num_openmm_steps=n, sim=LangevinDynamics(...))` - or
`sim="device"` with an `AmberPotentialEnergyTorch` energy, for which the chain builds one (the preset's integrator, a seed
drawn from the chain's noise; `sim=None` turns the options off, as in the reference) - advances states on the GPU without
the host round trip an OpenMM Simulation costs per iteration.  The integration schemes are OpenMM's; the Gaussian noise is
this library's own counter-based stream, so trajectories agree with OpenMM's statistically (temperature, energy
conservation without friction), not step for step.  The stream is keyed on (seed, conformation, steps_done + step, component), the
step count as 64 bits; tests/langevin_oracle.py restates generator and schemes in float64.  There is no CPU path.

`LangevinDynamics.trajectory` records frames on the device while it steps (`tw_langevin_trajectory`): positions, velocities,
forces and [E_pot, E_kin] at chosen steps of one launch - the data the reference's NPZReporter collects through OpenMM
(simulation/npzreporter.py:244-273).  timewarp_amd/simulation.py builds the reference's trajectory files on it.

`minimize_energy` relaxes conformations on the device before dynamics (`tw_minimize`, an L-BFGS on the same force kernels): the
stand-in for `simulation.minimizeEnergy` (simulate_trajectory.py:186-191).  It stops by OpenMM's rule - RMS force at or below
the tolerance - and does not reproduce OpenMM's iterates (include/timewarp_hip.h).

`LangevinDynamics(constraints="h-bonds")` holds the bonds to hydrogen at their equilibrium lengths (OpenMM's `constraints=HBonds`,
which the reference's md.py:182 leaves at None), so that the step can be 2 fs: `step` and `trajectory` then run
`tw_langevin_trajectory_constrained` - SHAKE for the positions, a direct projection for the velocities, one lane per X-H star -
and `apply_constraints` projects a state onto the constraints first.  Off by default: it samples another ensemble than the flow's.
tests/constraint_oracle.py restates it in float64."""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional

import numpy as np
import torch

from . import _lib
from .energy import AmberPotentialEnergyTorch

SCHEMES = {"LangevinMiddleIntegrator": 0, "LangevinIntegrator": 1}
VELOCITY_KINDS = {"stored": 0, "full-step": _lib.TW_RECORD_FULL_STEP_VELOCITIES}     # -> record_flags of tw_langevin_trajectory_opts

# ---------------------------------------------------------------------------------------------
# energy minimisation
# ---------------------------------------------------------------------------------------------
MIN_CONVERGED, MIN_CONTINUE, MIN_STALLED, MIN_NONFINITE = 0, 1, 2, 3     # the status codes of tw_minimize
MIN_WS_HEADER = 8               # doubles before x in a workspace row (include/timewarp_hip.h)
MIN_HISTORY = 8                 # pairs of the L-BFGS ring: the usual 3 .. 20; 8 rows of 3V doubles stay in cache for any molecule here
# nm: no coordinate moves further in one trial step.  A length scale of the force field, not a tuned number: a tenth of the shortest
# equilibrium bond length in the AMBER tables (X-H, 0.096 .. 0.109 nm).  Inside it the stiffest term, a bond of k ~ 5e5 kJ/mol/nm^2,
# is still near its harmonic range, so the first steepest-descent trial from a strained start cannot throw an atom through a neighbour.
MIN_MAX_DISPLACEMENT = 0.01
MIN_LAUNCH_SECONDS = 0.2        # what a worst-case launch should take: the aim of simulation.simulate_trajectory's steps_per_launch
MIN_WORST_EVALUATIONS = 42      # per iteration: 21 trials with a history, 21 more as steepest descent


def default_iterations_per_launch(n_atoms: int) -> int:
    """Iterations per launch such that a launch in which EVERY iteration runs its worst case (42 force evaluations) stays near
    0.2 s.  The time of one evaluation inside the minimiser is interpolated from what tools/time_minimize.py measured on an
    MI355X (profiles/minimize.txt), bookkeeping included: 46 us on the one-wave path (alanine dipeptide, up to 64 atoms), and
    on the sixteen-wave path 0.14 ms at 65 atoms (NNQQ) rising with the pair terms' V^2 to 2.9 ms at 691 atoms (1hgv).  That
    gives 103 iterations for alanine dipeptide, 34 for NNQQ and 1 for the protein.  A typical iteration takes 1.02 evaluations,
    so a typical launch is some forty times shorter than the bound; the cut costs nothing measurable (same file)."""
    if n_atoms <= 64:
        seconds = 46e-6
    else:
        seconds = 0.14e-3 + (2.9e-3 - 0.14e-3) * (n_atoms ** 2 - 65 ** 2) / (691 ** 2 - 65 ** 2)
    return max(1, int(MIN_LAUNCH_SECONDS / (MIN_WORST_EVALUATIONS * seconds)))


@dataclasses.dataclass
class MinimizationResult:
    """What `minimize_energy` returns, N rows.  `status`: 0 converged, 1 stopped by `max_iterations` (pass `workspace` back to go on),
    2 stalled (no step of the line search lowered the energy), 3 energy or forces not finite at the start (coordinates unchanged)."""

    coords: torch.Tensor        # float32, shaped like the input: the float32 cast of coords64
    coords64: torch.Tensor      # [N, V, 3] float64: the accepted state
    energy: torch.Tensor        # [N] float64 kJ/mol at coords64
    rms_force: torch.Tensor     # [N] float64 kJ/mol/nm: sqrt(sum F^2 / 3V) at coords64
    iterations: torch.Tensor    # [N] int32: accepted steps
    evaluations: torch.Tensor   # [N] int32: force evaluations
    status: torch.Tensor        # [N] int32
    converged: torch.Tensor     # [N] bool: status == 0
    workspace: torch.Tensor     # [N, tw_minimize_workspace_len] float64: the state `minimize_energy(..., workspace=)` continues from
    history: int


@torch.no_grad()
def minimize_energy(energy: AmberPotentialEnergyTorch, coords: torch.Tensor, tolerance: float = 10.0, max_iterations: int = 0,
                    history: int = MIN_HISTORY, iterations_per_launch: Optional[int] = None,
                    max_displacement: float = MIN_MAX_DISPLACEMENT, workspace: Optional[torch.Tensor] = None) -> MinimizationResult:
    """Local minimisation of every conformation in `coords` [..., V, 3] (nm, on the GPU) until the RMS of all force components
    is at or below `tolerance` (kJ/mol/nm): signature and defaults of OpenMM's `Simulation.minimizeEnergy(tolerance=10,
    maxIterations=0)`, `max_iterations=0` meaning "until every row has stopped".  L-BFGS with `history` pairs and a backtracking
    line search in fp64 on the device (include/timewarp_hip.h has the algorithm); rows are independent and a row's result does
    not depend on the batch it is in, on `iterations_per_launch` or on `max_iterations` cuts.

    The run is a chain of launches of at most `iterations_per_launch` iterations (default: `default_iterations_per_launch`) on
    one workspace; the status vector is read back after each launch - one host wait per launch - and the chain ends when no row
    has status 1 or `max_iterations` iterations were launched.  `workspace`: that of an earlier result of the same rows and
    `history`, to continue a run `max_iterations` stopped (`coords` then only gives the shape)."""
    V = energy.tables.n_atoms
    x = _lib.require_gpu_tensor(coords.reshape(-1, V, 3), torch.float32, "coords").clone()
    n, dev = x.shape[0], x.device
    history, max_iterations = int(history), int(max_iterations)
    if max_iterations < 0:
        raise ValueError("max_iterations must not be negative (0: until every row has stopped)")
    per_launch = default_iterations_per_launch(V) if iterations_per_launch is None else int(iterations_per_launch)
    if per_launch < 1:
        raise ValueError("iterations_per_launch must be at least 1")
    lib = _lib.load()
    ws_len = int(lib.tw_minimize_workspace_len(V, history))
    if ws_len < 0:
        raise ValueError(f"history {history}: expected 0 .. 64 pairs")
    fresh = workspace is None
    if fresh:
        workspace = torch.empty((n, ws_len), dtype=torch.float64, device=dev)
    elif workspace.dtype != torch.float64 or tuple(workspace.shape) != (n, ws_len) or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError(f"workspace: expected the contiguous float64 [{n}, {ws_len}] workspace of an earlier result on {dev}")
    ff = energy._device_ff(dev)
    e = torch.empty(n, dtype=torch.float64, device=dev)
    rms = torch.empty(n, dtype=torch.float64, device=dev)
    iters = torch.empty(n, dtype=torch.int32, device=dev)
    evals = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    launched = 0
    while True:
        k = per_launch if max_iterations == 0 else min(per_launch, max_iterations - launched)
        with torch.cuda.device(dev):
            _lib.check(lib.tw_minimize(C.byref(ff.struct), x.data_ptr(), workspace.data_ptr(), int(fresh), history, k, float(tolerance),
                                       float(max_displacement), e.data_ptr(), rms.data_ptr(), iters.data_ptr(), evals.data_ptr(),
                                       status.data_ptr(), n, _lib.stream_ptr(dev)), "tw_minimize")
        fresh = False
        launched += k
        if n == 0 or not bool((status == MIN_CONTINUE).any().item()) or (max_iterations and launched >= max_iterations):
            break
    x64 = workspace[:, MIN_WS_HEADER:MIN_WS_HEADER + 3 * V].reshape(n, V, 3).clone()
    return MinimizationResult(x.reshape(coords.shape), x64, e, rms, iters, evals, status, status == MIN_CONVERGED, workspace, history)



@dataclasses.dataclass
class TrajectoryFrames:
    """The frames one `LangevinDynamics.trajectory` call recorded, T frames of N rows.  A frame is the state after `step` steps:
    positions (nm), velocities (nm/ps) - float32 casts of the fp64 state -, the forces at those positions (kJ/mol/nm, float32) and
    energies[..., 0] = E_pot at those positions, energies[..., 1] = E_kin = 1/2 sum m v^2 of those velocities (kJ/mol, float64).
    `velocity_kind` says which velocities: "stored" - the integrator's own, which for LangevinMiddleIntegrator live at the half step
    (the ones `step` returns), not the full-step ones OpenMM's getState reports - or "full-step": stored + (dt/2) F / m with the
    frame's own forces (`trajectory(velocities="full-step")`, include/timewarp_hip.h), E_kin of those."""

    positions: torch.Tensor    # [N, T, V, 3] float32, on the device
    velocities: torch.Tensor   # [N, T, V, 3] float32
    forces: torch.Tensor       # [N, T, V, 3] float32
    energies: torch.Tensor     # [N, T, 2] float64
    step: np.ndarray           # [T] int64: absolute step count (steps_done at the call + report step)
    time: np.ndarray           # [T] float64: step * timestep, ps
    velocity_kind: str = "stored"    # "stored" or "full-step"


def check_report_steps(report_steps, num_steps=None):
    """`report_steps` as an int32 array and the step count of the launch (default: the last report step).  ValueError unless the
    steps are integers, strictly increasing and within 0 .. num_steps - the kernel walks the list with one running index and
    trusts it."""
    r = np.asarray(report_steps)
    if r.ndim != 1:
        raise ValueError(f"report_steps: expected a flat list of steps, got shape {r.shape}")
    if r.size and not (np.issubdtype(r.dtype, np.integer) or np.array_equal(r, np.round(r))):
        raise ValueError("report_steps: steps are whole numbers")
    r = r.astype(np.int64)
    if num_steps is None:
        if r.size == 0:
            raise ValueError("num_steps is needed when no step is reported")
        num_steps = int(r[-1])
    num_steps = int(num_steps)
    if not 0 <= num_steps < 2 ** 31:
        raise ValueError(f"num_steps {num_steps}: expected 0 .. 2^31 - 1")
    if r.size and r.min() < 0:
        raise ValueError(f"report_steps: negative step {int(r.min())}")
    if r.size and r.max() > num_steps:
        raise ValueError(f"report_steps: step {int(r.max())} is beyond the {num_steps} steps of the launch")
    if np.any(np.diff(r) <= 0):
        raise ValueError("report_steps: steps must be strictly increasing (no step twice)")
    return r.astype(np.int32), num_steps


class LangevinDynamics:
    def __init__(self, energy: AmberPotentialEnergyTorch, masses: torch.Tensor, timestep_ps: float = 0.0005,
                 friction_per_ps: float = 0.3, integrator: str = "LangevinMiddleIntegrator", seed: int = 0,
                 temperature: Optional[float] = None, constraints=None, constraint_tolerance: Optional[float] = None):
        """`constraints`: None (the default: today's kernels and calls, unchanged), "h-bonds" (the X-H bonds of the energy's tables,
        `forcefield.hbond_constraints`) or an `HBondConstraints`.  With constraints `step` and `trajectory` run the constrained
        kernel (`tw_langevin_trajectory_constrained`, include/timewarp_hip.h): the state passed in must satisfy the constraints -
        `apply_constraints` makes it so.  `constraint_tolerance` (relative to the squared length) replaces the set's own."""
        if integrator not in SCHEMES:
            raise ValueError(f"integrator {integrator!r}: expected one of {sorted(SCHEMES)}")
        self.energy = energy
        self.masses = masses.detach().to(torch.float32).reshape(-1).contiguous()
        if self.masses.numel() != energy.tables.n_atoms:
            raise ValueError("one mass per atom")
        self.dt, self.friction, self.scheme = float(timestep_ps), float(friction_per_ps), SCHEMES[integrator]
        self.integrator = integrator
        self.kbT = energy.kbT if temperature is None else 8.314462618e-3 * float(temperature)
        self.seed = int(seed) & (2 ** 64 - 1)
        self.steps_done = 0
        self._m = {}
        self.constraints = self._make_constraints(constraints, constraint_tolerance)
        self._c = {}
        self.constraint_residual = None     # [N] float64 / [N] int32 on the device: the last constrained launch's worst residual
        self.constraint_sweeps = None       # and SHAKE sweeps per row

    def _make_constraints(self, constraints, tolerance):
        from .forcefield import HBondConstraints, hbond_constraints

        if constraints is None or constraints == "none":
            if tolerance is not None:
                raise ValueError("constraint_tolerance needs constraints=")
            return None
        if isinstance(constraints, str):
            if constraints != "h-bonds":
                raise ValueError(f"constraints {constraints!r}: expected None, 'h-bonds' or an HBondConstraints")
            cons = hbond_constraints(self.energy.tables, self.masses)
        elif isinstance(constraints, HBondConstraints):
            cons = constraints
        else:
            raise ValueError(f"constraints {constraints!r}: expected None, 'h-bonds' or an HBondConstraints")
        if tolerance is not None:
            cons = dataclasses.replace(cons, tolerance=float(tolerance))
        if cons.n_atoms != self.energy.tables.n_atoms:
            raise ValueError(f"constraints: made for {cons.n_atoms} atoms, the energy has {self.energy.tables.n_atoms}")
        return cons.check()

    @property
    def n_dof(self) -> int:
        """Degrees of freedom of one conformation: 3 V minus the constraints (the centre of mass is not removed)."""
        return 3 * self.energy.tables.n_atoms - (0 if self.constraints is None else self.constraints.n_constraints)

    def _constraints_on(self, device):
        key = str(device)
        if key not in self._c:
            self._c[key] = self.constraints.to_device(device)
        return self._c[key]

    @torch.no_grad()
    def apply_constraints(self, coords: torch.Tensor, velocs: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None):
        """Project a state onto the constraints (`tw_apply_constraints`): positions by SHAKE against themselves, then velocities
        (when given) so that no constrained bond changes length to first order.  With `state` (the fp64 carry of `new_state`)
        both halves are projected in place in float64 and the float32 casts are returned; otherwise `coords` (and `velocs`) are
        read, projected in float64 and returned as float32 casts.  Returns (coords, velocs) - velocs None when none were given -
        and leaves the rows' residuals in `constraint_residual`.  Atoms outside the clusters are not touched."""
        if self.constraints is None:
            raise ValueError("apply_constraints: this integrator has no constraints")
        V = self.energy.tables.n_atoms
        lib = _lib.load()
        if state is not None:
            if state.dtype != torch.float64 or state.dim() != 4 or tuple(state.shape[1:]) != (2, V, 3) or not state.is_contiguous():
                raise ValueError(f"state: expected the contiguous float64 [N, 2, {V}, 3] tensor of new_state()")
            _lib.require_gpu_tensor(state, torch.float64, "state")
            n, dev = state.shape[0], state.device
            x = v = None
        else:
            x = _lib.require_gpu_tensor(coords.reshape(-1, V, 3), torch.float32, "coords").clone()
            v = None if velocs is None else _lib.require_gpu_tensor(velocs.reshape(-1, V, 3), torch.float32, "velocs").clone()
            n, dev = x.shape[0], x.device
        cons = self._constraints_on(dev)
        res = torch.zeros(n, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.tw_apply_constraints(C.byref(cons.struct), self._masses_on(dev).data_ptr(), V, _lib.ptr(x), _lib.ptr(v),
                                                _lib.ptr(state), res.data_ptr(), n, _lib.stream_ptr(dev)), "tw_apply_constraints")
        self.constraint_residual = res
        if state is not None:
            return state[:, 0].to(torch.float32), state[:, 1].to(torch.float32)
        return x.reshape(coords.shape).to(coords.dtype), None if v is None else v.reshape(velocs.shape).to(velocs.dtype)

    def _constrained_launch(self, x, v, state, num_steps, steps_dev, T, bufs, flags, n, dev):
        cons = self._constraints_on(dev)
        ff = self.energy._device_ff(dev)
        res = torch.zeros(n, dtype=torch.float64, device=dev)
        sweeps = torch.zeros(n, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().tw_langevin_trajectory_constrained(
                C.byref(ff.struct), self._masses_on(dev).data_ptr(), x.data_ptr(), v.data_ptr(), _lib.ptr(state), int(num_steps), self.dt,
                self.friction, self.kbT, self.scheme, self.seed, self.steps_done, _lib.ptr(steps_dev), T,
                *[b.data_ptr() if T else None for b in bufs], n, int(flags), C.byref(cons.struct), res.data_ptr(), sweeps.data_ptr(),
                _lib.stream_ptr(dev)), "tw_langevin_trajectory_constrained")
        self.constraint_residual, self.constraint_sweeps = res, sweeps

    def _masses_on(self, device):
        key = str(device)
        if key not in self._m:
            self._m[key] = self.masses.to(device)
        return self._m[key]

    @torch.no_grad()
    def step(self, coords: torch.Tensor, velocs: torch.Tensor, num_steps: int = 1, want_energy: bool = False):
        """`num_steps` steps of every conformation: coords (nm), velocs (nm/ps) [..., V, 3] -> new (coords, velocs) like the
        inputs (and, with `want_energy`, the potential energy [N] at the last force evaluation: the positions before the last update)."""
        V = self.energy.tables.n_atoms
        x = _lib.require_gpu_tensor(coords.reshape(-1, V, 3), torch.float32, "coords").clone()
        v = _lib.require_gpu_tensor(velocs.reshape(-1, V, 3), torch.float32, "velocs").clone()
        n, dev = x.shape[0], x.device
        if self.constraints is not None:
            if want_energy:
                raise ValueError("step(want_energy=True) is not available with constraints: record a frame with `trajectory`")
            self._constrained_launch(x, v, None, num_steps, None, 0, (None,) * 4, 0, n, dev)
            self.steps_done += int(num_steps)
            return x.reshape(coords.shape).to(coords.dtype), v.reshape(velocs.shape).to(velocs.dtype)
        ff = self.energy._device_ff(dev)
        e = torch.empty(n, dtype=torch.float64, device=dev) if want_energy else None
        with torch.cuda.device(dev):
            _lib.check(_lib.load().tw_langevin_steps(
                C.byref(ff.struct), self._masses_on(dev).data_ptr(), x.data_ptr(), v.data_ptr(), int(num_steps), self.dt,
                self.friction, self.kbT, self.scheme, self.seed, self.steps_done, _lib.ptr(e), n, _lib.stream_ptr(dev)),
                "tw_langevin_steps")
        self.steps_done += int(num_steps)
        out = (x.reshape(coords.shape).to(coords.dtype), v.reshape(velocs.shape).to(velocs.dtype))
        return out + (e,) if want_energy else out

    def new_state(self, coords: torch.Tensor, velocs: torch.Tensor) -> torch.Tensor:
        """The fp64 carry of `trajectory`: [N, 2, V, 3] float64 = (x, v) per row on the device of `coords`, from the float32 values
        a launch without carry would start from."""
        V = self.energy.tables.n_atoms
        x = _lib.require_gpu_tensor(coords.reshape(-1, V, 3), torch.float32, "coords")
        v = _lib.require_gpu_tensor(velocs.reshape(-1, V, 3), torch.float32, "velocs")
        return torch.stack([x, v], dim=1).to(torch.float64).contiguous()

    @torch.no_grad()
    def trajectory(self, coords: torch.Tensor, velocs: torch.Tensor, report_steps, num_steps: Optional[int] = None,
                   state: Optional[torch.Tensor] = None, velocities: str = "stored"):
        """`num_steps` steps (default: the last report step) of every conformation in ONE launch, recording a frame at each of
        `report_steps` - strictly increasing step counts from the start of this call, 0 (the input state) .. num_steps.
        Returns (coords, velocs, frames): the final state like `step` returns it and a `TrajectoryFrames`.  A frame does not
        depend on which other steps are reported.  `state` (from `new_state`, updated in place) carries x and v between calls in
        float64: the launch then starts from it, not from `coords` / `velocs`, and a run cut into several calls is bit for bit
        the run of one; without it the state is rounded to float32 between calls, as with `step`.  With `state`, `coords` and
        `velocs` may be None (the shapes are the state's; [N, V, 3] float32 comes back); when they are given they must be the
        float32 cast of the state - what `new_state` was made from, or what the previous call returned - and a pair that is
        not (a fresh x, v beside a stale state) is refused with ValueError.  That comparison waits for the device, so a loop
        of many short launches passes None.  An empty `report_steps` is plain stepping with the carry.

        `velocities`: "stored" (the default: the call of before, `tw_langevin_trajectory`) or "full-step": the frames' velocities
        are the stored ones plus (dt/2) F / m of the frame's own forces and E_kin is theirs (`tw_langevin_trajectory_opts` with
        TW_RECORD_FULL_STEP_VELOCITIES).  Positions, forces, E_pot, the returned state and `state` do not depend on it."""
        if velocities not in VELOCITY_KINDS:
            raise ValueError(f"velocities {velocities!r}: expected one of {sorted(VELOCITY_KINDS)}")
        r, num_steps = check_report_steps(report_steps, num_steps)
        V = self.energy.tables.n_atoms
        if (coords is None) != (velocs is None) or (coords is None and state is None):
            raise ValueError("coords and velocs: both, or neither and a `state` to start from")
        if coords is None:
            if state.dtype != torch.float64 or state.dim() != 4 or tuple(state.shape[1:]) != (2, V, 3) or not state.is_contiguous():
                raise ValueError(f"state: expected the contiguous float64 [N, 2, {V}, 3] tensor of new_state()")
            _lib.require_gpu_tensor(state, torch.float64, "state")
            x, v = state[:, 0].to(torch.float32).contiguous(), state[:, 1].to(torch.float32).contiguous()
            shape_x, shape_v, dtype_x, dtype_v = x.shape, v.shape, torch.float32, torch.float32
        else:
            x = _lib.require_gpu_tensor(coords.reshape(-1, V, 3), torch.float32, "coords").clone()
            v = _lib.require_gpu_tensor(velocs.reshape(-1, V, 3), torch.float32, "velocs").clone()
            shape_x, shape_v, dtype_x, dtype_v = coords.shape, velocs.shape, coords.dtype, velocs.dtype
        n, dev, T = x.shape[0], x.device, int(r.size)
        if state is not None and (state.dtype != torch.float64 or tuple(state.shape) != (n, 2, V, 3) or state.device != dev
                                  or not state.is_contiguous()):
            raise ValueError(f"state: expected the contiguous float64 [{n}, 2, {V}, 3] tensor of new_state() on {dev}")
        if state is not None and coords is not None:
            same = lambda a, b: torch.equal(a.to(torch.float32).contiguous().view(torch.int32), b.view(torch.int32))
            if not (same(state[:, 0], x) and same(state[:, 1], v)):
                raise ValueError("state: coords / velocs are not the float32 cast of `state` - the launch would start from the state and "
                                 "ignore them; make a new_state(coords, velocs), or pass None for both to continue from the state")
        ff = self.energy._device_ff(dev)
        steps_dev = torch.from_numpy(r).to(dev) if T else None
        f32 = lambda: torch.empty((n, T, V, 3), dtype=torch.float32, device=dev)
        pos, vel, frc = f32(), f32(), f32()
        ene = torch.empty((n, T, 2), dtype=torch.float64, device=dev)
        args = (C.byref(ff.struct), self._masses_on(dev).data_ptr(), x.data_ptr(), v.data_ptr(), _lib.ptr(state), num_steps, self.dt,
                self.friction, self.kbT, self.scheme, self.seed, self.steps_done, _lib.ptr(steps_dev), T,
                pos.data_ptr() if T else None, vel.data_ptr() if T else None, frc.data_ptr() if T else None,
                ene.data_ptr() if T else None, n)
        with torch.cuda.device(dev):
            if self.constraints is not None:      # full-step velocities are refused by the library, by name
                self._constrained_launch(x, v, state, num_steps, steps_dev, T, (pos, vel, frc, ene), VELOCITY_KINDS[velocities], n, dev)
            elif velocities == "stored":
                _lib.check(_lib.load().tw_langevin_trajectory(*args, _lib.stream_ptr(dev)), "tw_langevin_trajectory")
            else:
                _lib.check(_lib.load().tw_langevin_trajectory_opts(*args, VELOCITY_KINDS[velocities], _lib.stream_ptr(dev)),
                           "tw_langevin_trajectory_opts")
        step = self.steps_done + r.astype(np.int64)
        self.steps_done += num_steps
        frames = TrajectoryFrames(pos, vel, frc, ene, step, step.astype(np.float64) * self.dt, velocities)
        return x.reshape(shape_x).to(dtype_x), v.reshape(shape_v).to(dtype_v), frames

    def continued_at(self, steps_done: int) -> "LangevinDynamics":
        """This integrator standing at absolute step `steps_done`: the noise is keyed on (seed, row, absolute step), so a run
        that is resumed from a saved fp64 state must also restore the step count to draw the noise the uninterrupted run drew.
        Returns self."""
        steps_done = int(steps_done)
        if steps_done < 0:
            raise ValueError("steps_done must not be negative")
        self.steps_done = steps_done
        return self

    @classmethod
    def from_preset(cls, energy: AmberPotentialEnergyTorch, masses: torch.Tensor, preset: str = "amber14-implicit", seed: int = 0, **kwargs):
        """simulation/md.py:75-93: both presets run 310 K, 0.3 / ps, 0.5 fs; "amber99-implicit-old" uses LangevinIntegrator,
        everything else (the other presets, energies of unknown origin) LangevinMiddleIntegrator (md.py:213-231)."""
        integ = "LangevinIntegrator" if preset == "amber99-implicit-old" else "LangevinMiddleIntegrator"
        return cls(energy, masses, kwargs.pop("timestep_ps", 0.0005), 0.3, integ, seed, **kwargs)

    @classmethod
    def for_energy(cls, energy: AmberPotentialEnergyTorch, masses: torch.Tensor, seed: int = 0, **kwargs):
        """The integrator of the energy object: the scheme, step size and friction of the OpenMM integrator it was built with
        (`AmberPotentialEnergyTorch.from_openmm(system, integrator)`), else its dataset preset's.  `kwargs`: `timestep_ps` (instead
        of that step size), `constraints`, `constraint_tolerance` as in the constructor."""
        if getattr(energy, "md_integrator", None) is not None:
            name, dt, friction = energy.md_integrator
            return cls(energy, masses, kwargs.pop("timestep_ps", dt), friction, name, seed, **kwargs)
        return cls.from_preset(energy, masses, preset=energy.md_preset, seed=seed, **kwargs)
