"""Full-step velocities in the recording Langevin kernel (csrc/tw_md.hip `langevin_trajectory_kernel<W, FULL>` behind
`tw_langevin_trajectory_opts`, `LangevinDynamics.trajectory(velocities="full-step")`): with `record_flags == 0` the new entry
point is the old one bit for bit; with TW_RECORD_FULL_STEP_VELOCITIES only the frames' velocities and E_kin change, and they
change by (dt/2) F / m of the frame's own forces.

Shapes: alanine dipeptide (22 atoms, one wave, 3 rows) and NNQQ (65 atoms, sixteen waves, 2 rows) of tests/test_langevin_gpu.py, both
schemes, 10 steps with frames at 0, 1, 4 and 10 (the input state, and the last step's own branch of the kernel), first step 1000003."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_langevin_cpu import real_case
from tests.test_langevin_gpu import FIRST_STEP, dynamics, free_energy, free_state
from tests.test_md_trajectory_gpu import FRAME_KEYS, real_md, record

pytestmark = pytest.mark.gpu

REPORTS = [0, 1, 4, 10]
ROWS = {"ad": 3, "nnqq": 2}
CASES = [(mol, scheme) for mol in ("ad", "nnqq") for scheme in (0, 1)]


def launch_opts(md, x, v, reports, flags, num_steps, state=None, prefill=None):
    """`tw_langevin_trajectory_opts` through the ctypes table, with the buffers `LangevinDynamics.trajectory` makes ->
    (return code, x, v, frames as numpy arrays).  `prefill`: the value the four frame buffers hold before the call."""
    from timewarp_amd import _lib

    x, v = torch.from_numpy(x).cuda().clone(), torch.from_numpy(v).cuda().clone()
    n, V, T = x.shape[0], x.shape[1], len(reports)
    steps = torch.tensor(reports, dtype=torch.int32, device="cuda")
    make = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda") if prefill is None else torch.full(shape, prefill, dtype=dtype, device="cuda")
    pos, vel, frc = (make((n, T, V, 3), torch.float32) for _ in range(3))
    ene = make((n, T, 2), torch.float64)
    ff = md.energy._device_ff(x.device)
    rc = _lib.load().tw_langevin_trajectory_opts(
        C.byref(ff.struct), md._masses_on(x.device).data_ptr(), x.data_ptr(), v.data_ptr(), _lib.ptr(state), num_steps, md.dt, md.friction,
        md.kbT, md.scheme, md.seed, md.steps_done, steps.data_ptr(), T, pos.data_ptr(), vel.data_ptr(), frc.data_ptr(), ene.data_ptr(), n,
        flags, _lib.stream_ptr(x.device))
    torch.cuda.synchronize()
    frames = {"positions": pos.cpu().numpy(), "velocities": vel.cpu().numpy(), "forces": frc.cpu().numpy(), "energies": ene.cpu().numpy()}
    return rc, x.cpu().numpy(), v.cpu().numpy(), frames


_RUNS = {}


def runs(mol, scheme):
    """The stored and the full-step launch of one case, each with an fp64 carry, computed once: (x, v, frames, state)."""
    if (mol, scheme) not in _RUNS:
        x0, v0 = real_case(mol)[2][:ROWS[mol]], real_case(mol)[3][:ROWS[mol]]
        out = {}
        for kind in ("stored", "full-step"):
            md = real_md(mol, scheme, 0.3)[0]
            state = md.new_state(torch.from_numpy(x0).cuda(), torch.from_numpy(v0).cuda())
            gx, gv, f = md.trajectory(torch.from_numpy(x0).cuda(), torch.from_numpy(v0).cuda(), REPORTS, state=state, velocities=kind)
            assert f.velocity_kind == kind and md.steps_done == FIRST_STEP + 10
            frames = {k: getattr(f, k).cpu().numpy() for k in FRAME_KEYS}
            out[kind] = (gx.cpu().numpy(), gv.cpu().numpy(), frames, state.cpu().numpy())
        _RUNS[mol, scheme] = out
    return _RUNS[mol, scheme]


@pytest.mark.parametrize("mol,scheme", CASES)
def test_flags_zero_is_the_old_call(mol, scheme):
    """`trajectory()` as every caller of before makes it (`tw_langevin_trajectory`), `trajectory(velocities="stored")` and
    `tw_langevin_trajectory_opts` with record_flags = 0 give the same bits in every frame key, in the returned state and in the
    fp64 carry."""
    from timewarp_amd import _lib

    x0, v0 = real_case(mol)[2][:ROWS[mol]], real_case(mol)[3][:ROWS[mol]]
    sx, sv, stored, sstate = runs(mol, scheme)["stored"]
    md = real_md(mol, scheme, 0.3)[0]
    state = md.new_state(torch.from_numpy(x0).cuda(), torch.from_numpy(v0).cuda())
    ox, ov, old = record(md, x0, v0, REPORTS, state=state)                    # no `velocities` argument at all
    md2 = real_md(mol, scheme, 0.3)[0]
    state2 = md2.new_state(torch.from_numpy(x0).cuda(), torch.from_numpy(v0).cuda())
    rc, nx, nv, new = launch_opts(md2, x0, v0, REPORTS, 0, 10, state=state2)
    assert rc == 0, _lib.load().tw_last_error()
    for key in FRAME_KEYS:
        assert np.array_equal(old[key], stored[key]) and np.array_equal(old[key], new[key]), (mol, scheme, key)
    assert np.array_equal(ox, sx) and np.array_equal(ov, sv) and np.array_equal(ox, nx) and np.array_equal(ov, nv)
    assert np.array_equal(state.cpu().numpy(), sstate) and np.array_equal(state2.cpu().numpy(), sstate)
    assert np.abs(old["forces"]).max() > 100.0 and not np.array_equal(old["positions"][:, 0], old["positions"][:, 3])
    # without the carry too (coords / velocs alone)
    _, _, plain = record(real_md(mol, scheme, 0.3)[0], x0, v0, REPORTS)
    rc, _, _, plain_new = launch_opts(real_md(mol, scheme, 0.3)[0], x0, v0, REPORTS, 0, 10)
    assert rc == 0 and all(np.array_equal(plain[k], plain_new[k]) for k in FRAME_KEYS)


@pytest.mark.parametrize("mol,scheme", CASES)
def test_only_velocities_and_kinetic_energy_change(mol, scheme):
    (sx, sv, S, sstate), (fx, fv, F, fstate) = runs(mol, scheme)["stored"], runs(mol, scheme)["full-step"]
    assert np.array_equal(S["positions"], F["positions"]) and np.array_equal(S["forces"], F["forces"])
    assert np.array_equal(S["energies"][..., 0], F["energies"][..., 0])
    assert np.array_equal(sx, fx) and np.array_equal(sv, fv) and np.array_equal(sstate, fstate)
    assert not np.array_equal(S["velocities"], F["velocities"]) and not np.array_equal(S["energies"][..., 1], F["energies"][..., 1])
    # the same through the C ABI directly, flag 1
    from timewarp_amd import _lib

    x0, v0 = real_case(mol)[2][:ROWS[mol]], real_case(mol)[3][:ROWS[mol]]
    rc, _, _, direct = launch_opts(real_md(mol, scheme, 0.3)[0], x0, v0, REPORTS, _lib.TW_RECORD_FULL_STEP_VELOCITIES, 10)
    assert rc == 0 and all(np.array_equal(direct[k], F[k]) for k in FRAME_KEYS)


@pytest.mark.parametrize("mol,scheme", CASES)
def test_the_shift_is_half_a_kick_of_the_frames_own_forces(mol, scheme):
    """S: the stored run, F: the full-step run.  For every component
        |F.v - (S.v + (dt/2) S.F / m)| <= 1/2 ulp32(S.v) + (dt / 2m) 1/2 ulp32(S.F) + 1/2 ulp32(F.v),
    the right-hand side in float64 from the float32 frames: S.v and S.F are float32 roundings of the fp64 values the kernel
    combined, F.v is the float32 rounding of the result; nothing is measured.  E_kin of F within 2^-22 relative of
    1/2 sum m F.v^2 (the bound of test_force_free_frames_match_the_restatement).  The shift is far above the bound, so the factor
    1/2, the sign and the atom's own mass are all held: a hydrogen's shift with a carbon's mass is 12 times too small."""
    dt = 0.0005
    _, masses, _, _ = real_case(mol)
    S, F = runs(mol, scheme)["stored"][2], runs(mol, scheme)["full-step"][2]
    m = masses.astype(np.float64)[None, None, :, None]
    sv, sf, fv = (a.astype(np.float64) for a in (S["velocities"], S["forces"], F["velocities"]))
    half_ulp = lambda a: 0.5 * np.spacing(np.abs(a)).astype(np.float64)       # of the float32 arrays
    shift = 0.5 * dt * sf / m
    err = np.abs(fv - (sv + shift))
    bound = half_ulp(S["velocities"]) + (0.5 * dt / m) * half_ulp(S["forces"]) + half_ulp(F["velocities"])
    ek = 0.5 * (m * fv ** 2).sum(axis=(2, 3))
    ek_err = np.abs(F["energies"][..., 1] - ek) / ek
    light = masses < 2.0
    print(f"{mol} scheme {scheme}: error {(err / bound).max():.3f} of the bound; largest shift {np.abs(shift).max():.3f} nm/ps "
          f"(hydrogens {np.abs(shift[:, :, light]).max():.3f}, heavy atoms {np.abs(shift[:, :, ~light]).max():.3f}), "
          f"{(np.abs(shift) / bound).min():.0f} .. {(np.abs(shift) / bound).max():.0f} bounds; E_kin off by {ek_err.max():.2e} relative")
    assert np.all(err <= bound)
    assert np.all(ek_err <= 2.0 ** -22)
    assert light.any() and (~light).any()
    assert np.median(np.abs(shift) / bound) > 1000.0 and np.abs(shift).max() > 0.01      # the test can tell a wrong factor, sign or mass


@pytest.mark.parametrize("scheme", [0, 1])
def test_force_free_tables_shift_nothing(scheme):
    """No forces, no shift: full-step frames are the stored frames bit for bit, E_kin included - one wave and sixteen."""
    for V, rows in ((22, 3), (65, 2)):
        masses, x, v = free_state(V, rows)
        make = lambda: dynamics(free_energy(V), masses, 0.0005, 0.3, scheme, 77 + V, FIRST_STEP)
        out = {}
        for kind in ("stored", "full-step"):
            gx, gv, f = make().trajectory(torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda(), REPORTS, velocities=kind)
            out[kind] = [gx.cpu().numpy(), gv.cpu().numpy()] + [getattr(f, k).cpu().numpy() for k in FRAME_KEYS]
        assert all(np.array_equal(a, b) for a, b in zip(out["stored"], out["full-step"])), V
        assert np.count_nonzero(out["stored"][4]) == 0 and np.abs(out["stored"][3][:, -1] - v).max() > 1e-4


def test_unknown_record_flags_are_refused_before_anything_is_written():
    from timewarp_amd import _lib

    x0, v0 = real_case("ad")[2][:2], real_case("ad")[3][:2]
    for flags in (2, 3, 1 << 30, -2 ** 31, 0x100):
        md = real_md("ad", 0, 0.3)[0]
        state = md.new_state(torch.from_numpy(x0).cuda(), torch.from_numpy(v0).cuda())
        before = state.clone()
        rc, x, v, frames = launch_opts(md, x0, v0, REPORTS, flags, 10, state=state, prefill=-7.5)
        assert rc != 0 and b"record_flags" in _lib.load().tw_last_error(), flags
        assert all(np.all(frames[k] == -7.5) for k in FRAME_KEYS), flags
        assert np.array_equal(x, x0) and np.array_equal(v, v0) and torch.equal(state, before)
    with pytest.raises(ValueError, match="velocities"):
        real_md("ad", 0, 0.3)[0].trajectory(torch.from_numpy(x0).cuda(), torch.from_numpy(v0).cuda(), REPORTS, velocities="half-step")
