"""Checkpoint, resume and segments of timewarp_amd/simulation.py `simulate_trajectory` without a GPU.  The driver is run with a
duck-typed integrator (`FakeDynamics`): the float64 restatement tests/trajectory_oracle.py `segment` on CPU tensors with a harmonic
force, carrying its state in fp64 between calls as the device kernel does - so a run cut anywhere is bit for bit the run of one
call, and every comparison below is `np.array_equal`.  tests/test_md_checkpoint_gpu.py repeats the cases on the device.

Also here: the checkpoint file's round trip, the atomic write, refusals that touch nothing, a state that is not finite, the
default call's file listing, the new command-line flags, `--pdb` refusals, and `main`'s exit codes with the driver replaced."""
import os
import types

import numpy as np
import pytest
import torch

from tests import trajectory_oracle as to
from timewarp_amd import simulation as S
from timewarp_amd.md import TrajectoryFrames

V, N = 5, 2
KEYS = ("step", "time", "energies", "positions", "velocities", "forces")
SPRING = 3.0e4      # kJ/mol/nm^2: a period of some 60 steps of 0.5 fs for the masses below, so 27 steps see the force


def harmonic(x):
    return 0.5 * SPRING * (x * x).sum(axis=(1, 2)), -SPRING * x


class FakeDynamics:
    """What `simulate_trajectory` asks of a `LangevinDynamics`: masses, kbT, dt, friction, scheme, seed, steps_done,
    `new_state`, `continued_at` and `trajectory(None, None, report_steps, num_steps=, state=, velocities=)`."""

    def __init__(self, masses, seed=11, scheme=0, poison=None):
        self.masses = torch.as_tensor(masses, dtype=torch.float32)
        self.kbT, self.dt, self.friction, self.scheme, self.seed = 2.577, 0.0005, 0.3, scheme, seed
        self.steps_done = 0
        self.calls = []                 # (first absolute step, number of steps, frames) of every launch
        self.poison = poison            # (absolute step, row): the state of that row is NaN from that step on

    def new_state(self, coords, velocs):
        return torch.stack([coords, velocs], dim=1).to(torch.float64).contiguous()

    def continued_at(self, steps_done):
        self.steps_done = int(steps_done)
        return self

    def trajectory(self, coords, velocs, report_steps, num_steps=None, state=None, velocities="stored"):
        assert coords is None and velocs is None and state.dtype == torch.float64
        r = np.asarray(report_steps, dtype=np.int64)
        n = state.shape[0]
        m = self.masses.numpy().astype(np.float64).reshape(1, -1, 1)
        conf = np.arange(n).reshape(n, 1, 1)
        x, v = state[:, 0].numpy().copy(), state[:, 1].numpy().copy()
        pos, vel, frc, ene, at = [], [], [], [], 0
        for target in list(r) + [int(num_steps)]:
            x, v = to.segment(harmonic, m, x, v, int(target) - at, self.dt, self.friction, self.kbT, self.scheme, self.seed,
                              self.steps_done + at, conf)
            at = int(target)
            if len(pos) < len(r):
                e, f = harmonic(x)
                w = v + 0.5 * self.dt * f / m if velocities == "full-step" else v
                pos.append(x.astype(np.float32)), vel.append(w.astype(np.float32)), frc.append(f.astype(np.float32))
                ene.append(np.stack([e, 0.5 * (m * w * w).sum(axis=(1, 2))], axis=-1))
        self.calls.append((self.steps_done, int(num_steps), len(r)))
        step = self.steps_done + r
        self.steps_done += int(num_steps)
        if self.poison is not None and self.steps_done >= self.poison[0]:
            x[self.poison[1]] = np.nan
        state[:, 0], state[:, 1] = torch.from_numpy(x), torch.from_numpy(v)
        cat = lambda a, tail, dt: torch.from_numpy(np.stack(a, axis=1) if a else np.zeros((n, 0) + tail, dtype=dt))
        return None, None, TrajectoryFrames(cat(pos, (V, 3), np.float32), cat(vel, (V, 3), np.float32), cat(frc, (V, 3), np.float32),
                                            cat(ene, (2,), np.float64), step, step.astype(np.float64) * self.dt, velocities)


def system():
    rng = np.random.default_rng(7)
    masses = np.array([12.01, 1.008, 14.01, 16.0, 1.008], dtype=np.float32)
    energy = types.SimpleNamespace(tables=types.SimpleNamespace(n_atoms=V, spring=np.array([SPRING]), has_gbsa=0), kbT=2.577)
    x = torch.from_numpy((0.02 * rng.standard_normal((N, V, 3))).astype(np.float32))
    v = torch.from_numpy(rng.standard_normal((N, V, 3)).astype(np.float32))
    return energy, torch.from_numpy(masses), x, v


def run(tmp, *, spacing="log", burn_in=3, sampling=24, spl=7, md=None, given_velocities=True, **kw):
    energy, masses, x, v = system()
    if spacing == "log":
        spacing = S.LogarithmicSpacing(10, 3)
    md = md if md is not None else FakeDynamics(masses)
    return S.simulate_trajectory(energy, masses, x, v if given_velocities else None, burn_in=burn_in, sampling=sampling, spacing=spacing,
                                 integrator=md, steps_per_launch=spl, out_dir=str(tmp), name="fake", seed=4, **kw)


def same_rows(a, b):
    return len(a) == len(b) and all(sorted(ra) == sorted(KEYS) and all(ra[k].dtype == rb[k].dtype and np.array_equal(ra[k], rb[k]) for k in KEYS)
                                    for ra, rb in zip(a, b))


def same_files(dir_a, dir_b):
    names = sorted(os.listdir(dir_a))
    if names != sorted(os.listdir(dir_b)) or not names:
        return False
    for name in names:
        za, zb = np.load(os.path.join(dir_a, name)), np.load(os.path.join(dir_b, name))
        if sorted(za.files) != sorted(KEYS) or not all(za[k].dtype == zb[k].dtype and np.array_equal(za[k], zb[k]) for k in KEYS):
            return False
    return True


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    """A: one uninterrupted call without checkpointing - burn-in 3, sampling 24, LogarithmicSpacing(10, 3), 7 steps per launch."""
    d = tmp_path_factory.mktemp("A")
    md = FakeDynamics(system()[1])
    rows = run(d, md=md)
    assert rows[0]["step"].tolist() == [9, 10, 11, 13, 19, 20, 21, 23]
    assert [c[0] for c in md.calls] == [0, 3, 10, 17, 24]
    assert sorted(os.listdir(d)) == ["fake-0-traj-arrays.npz", "fake-1-traj-arrays.npz"]      # the default call writes what it wrote
    assert np.abs(rows[0]["forces"]).max() > 100.0 and not np.array_equal(rows[0]["positions"], rows[1]["positions"])
    return d, rows


@pytest.fixture(scope="module")
def baseline_redrawn(tmp_path_factory):
    d = tmp_path_factory.mktemp("A_redrawn")
    return d, run(d, redraw_velocities=True)


# ---------------------------------------------------------------------------------------------
# 1, 2: resume is bit-exact
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts,redraw", [((2,), False), ((3,), False), ((3,), True), ((2,), True), ((10,), False), ((12,), False), ((5, 16), False),
                                         ((5, 16), True)])
def test_resume_is_bit_exact(tmp_path, baseline, baseline_redrawn, cuts, redraw):
    """Stop with `max_steps` at every cut (inside the burn-in, on the burn-in / sampling boundary with the redraw on either side,
    on a report step, between reports, twice in one run), continue each time with a fresh integrator, 5 steps per launch and
    another `segment_frames`: rows and files equal the uninterrupted run's in every key."""
    want_dir, want = baseline_redrawn if redraw else baseline
    base = str(tmp_path / "ck" / "fake")
    done = 0
    for i, cut in enumerate(cuts):
        stats = {}
        out = run(tmp_path / "out", checkpoint=base, max_steps=cut - done, redraw_velocities=redraw, segment_frames=(2, 5)[i % 2],
                  spl=(7, 5)[i % 2], stats=stats)
        assert out is None and stats["steps_done"] == cut and stats["resumed_at"] == (done if i else None)
        ck = S.read_checkpoint(S.checkpoint_path(base))
        assert ck["steps_done"] == cut and ck["integrator_step"] == cut and ck["redrawn"] == (not redraw or cut > 3)    # no sampling launch yet at a cut <= 3
        done = cut
    stats = {}
    md = FakeDynamics(system()[1])
    got = run(tmp_path / "out", checkpoint=base, redraw_velocities=redraw, segment_frames=3, spl=5, md=md, stats=stats)
    assert stats["resumed_at"] == done and md.calls[0][0] == done and md.steps_done == 27
    assert same_rows(got, want) and same_files(tmp_path / "out", want_dir)
    assert os.listdir(tmp_path / "ck") == []      # checkpoint and segments are gone at completion


def test_the_redraw_flag_is_saved_once_it_happened(tmp_path, baseline_redrawn):
    """Cut at 10, after the first sampling launch: the checkpoint says the redraw is done and the resumed run does not repeat it."""
    base = str(tmp_path / "fake")
    assert run(tmp_path / "out", checkpoint=base, max_steps=10, redraw_velocities=True) is None
    assert S.read_checkpoint(S.checkpoint_path(base))["redrawn"] is True
    assert same_rows(run(tmp_path / "out", checkpoint=base, redraw_velocities=True, spl=5), baseline_redrawn[1])


def test_missing_velocities_are_drawn_once(tmp_path):
    want = run(tmp_path / "a", given_velocities=False)
    base = str(tmp_path / "fake")
    assert run(tmp_path / "b", given_velocities=False, checkpoint=base, max_steps=2) is None
    assert same_rows(run(tmp_path / "b", given_velocities=False, checkpoint=base, spl=5), want)


# ---------------------------------------------------------------------------------------------
# 3: the stateful windowed policy
# ---------------------------------------------------------------------------------------------
def test_windowed_policy_is_not_needed_again(tmp_path):
    make = lambda: S.UniformWindowedSpacing(20, spacing_window=4, subsamples=3, seed=5)
    want = run(tmp_path / "a", spacing=make(), burn_in=5, sampling=60)
    assert want[0]["step"].tolist() == [19, 20, 21, 22, 37, 38, 39, 40, 56, 59, 60, 62]
    base = str(tmp_path / "fake")
    assert run(tmp_path / "b", spacing=make(), burn_in=5, sampling=60, checkpoint=base, max_steps=30) is None
    assert run(tmp_path / "b", spacing=make(), burn_in=5, sampling=60, checkpoint=base, max_steps=11, spl=5) is None      # stands at 41
    assert S.read_checkpoint(S.checkpoint_path(base))["steps_done"] == 41
    got = run(tmp_path / "b", spacing=None, burn_in=5, sampling=60, checkpoint=base, spl=5)      # no policy at all
    assert same_rows(got, want) and same_files(tmp_path / "a", tmp_path / "b")
    with pytest.raises(ValueError, match="spacing may be None only"):
        run(tmp_path / "c", spacing=None, checkpoint=str(tmp_path / "c" / "fake"))


# ---------------------------------------------------------------------------------------------
# 4: segments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segment_frames", [1, 3, 8, 100])
def test_segments_bound_the_frame_buffer(tmp_path, baseline, segment_frames):
    stats = {}
    md = FakeDynamics(system()[1])
    got = run(tmp_path, segment_frames=segment_frames, md=md, stats=stats)
    assert same_rows(got, baseline[1]) and same_files(tmp_path, baseline[0])      # the listing too: no segment is left
    assert stats["max_buffered_frames"] == min(segment_frames, 8) and stats["segments"] == -(-8 // segment_frames)
    assert max(c[2] for c in md.calls) <= segment_frames and stats["checkpoints"] == 0
    kept = run(tmp_path / "kept", segment_frames=3, keep_segments=True)
    assert same_rows(kept, baseline[1])
    assert sorted(os.listdir(tmp_path / "kept")) == ["fake-0-traj-arrays.npz", "fake-1-traj-arrays.npz", "fake.segment-000000.npz",
                                                      "fake.segment-000001.npz", "fake.segment-000002.npz"]
    z = np.load(tmp_path / "kept" / "fake.segment-000001.npz")
    assert z["step"].tolist() == [13, 19, 20] and z["positions_1"].shape == (3, V, 3) and np.array_equal(z["positions_1"], baseline[1][1]["positions"][3:6])


def test_interval_checkpoints_leave_the_result_alone(tmp_path, baseline):
    stats = {}
    got = run(tmp_path / "out", checkpoint=str(tmp_path / "ck" / "fake"), checkpoint_steps=7, stats=stats)
    assert same_rows(got, baseline[1]) and stats["checkpoints"] == 3 and os.listdir(tmp_path / "ck") == []      # after 10, 17 and 24 steps
    stats = {}
    got = run(tmp_path / "out2", checkpoint=str(tmp_path / "ck2" / "fake"), checkpoint_seconds=0.0, keep_segments=True, stats=stats)
    assert same_rows(got, baseline[1]) and stats["checkpoints"] == 4      # after every launch but the last
    assert S.read_checkpoint(S.checkpoint_path(str(tmp_path / "ck2" / "fake")))["steps_done"] == 24


# ---------------------------------------------------------------------------------------------
# 5: refusals that touch nothing
# ---------------------------------------------------------------------------------------------
def snapshot(d):
    return {name: open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))}


def test_a_checkpoint_of_another_run_is_refused_and_nothing_is_touched(tmp_path, baseline):
    base = str(tmp_path / "fake")
    assert run(tmp_path, checkpoint=base, max_steps=12) is None
    before = snapshot(tmp_path)
    assert sorted(before) == ["fake.checkpoint.npz", "fake.segment-000000.npz"]
    energy, masses, x, v = system()
    others = [("velocities", dict(velocities="full-step")), ("burn_in", dict(burn_in=4, sampling=23)), ("sampling", dict(sampling=25)),
              ("redraw_velocities", dict(redraw_velocities=True)), ("minimize", dict(minimize=True)),
              ("noise_seed", dict(md=FakeDynamics(masses, seed=12))), ("scheme", dict(md=FakeDynamics(masses, scheme=1))),
              ("report_steps", dict(spacing=S.RegularSpacing(4))), ("masses", dict(md=FakeDynamics(masses * 2)))]
    for field, change in others:
        md = change.get("md") or FakeDynamics(masses)
        with pytest.raises(ValueError, match=f"`{field}`"):
            run(tmp_path, checkpoint=base, **{**change, "md": md})
        assert snapshot(tmp_path) == before and md.calls == [], field
    with pytest.raises(ValueError, match="`seed`"):
        S.simulate_trajectory(energy, masses, x, v, burn_in=3, sampling=24, spacing=S.LogarithmicSpacing(10, 3), integrator=FakeDynamics(masses),
                              steps_per_launch=7, out_dir=str(tmp_path), name="fake", seed=5, checkpoint=base)
    with pytest.raises(ValueError, match="`start`"):
        S.simulate_trajectory(energy, masses, x + 0.01, v, burn_in=3, sampling=24, spacing=S.LogarithmicSpacing(10, 3),
                              integrator=FakeDynamics(masses), steps_per_launch=7, out_dir=str(tmp_path), name="fake", seed=4, checkpoint=base)
    energy.tables.spring = np.array([SPRING + 1.0])
    with pytest.raises(ValueError, match="`force_field`"):
        S.simulate_trajectory(energy, masses, x, v, burn_in=3, sampling=24, spacing=S.LogarithmicSpacing(10, 3), integrator=FakeDynamics(masses),
                              steps_per_launch=7, out_dir=str(tmp_path), name="fake", seed=4, checkpoint=base)
    assert snapshot(tmp_path) == before
    assert same_rows(run(tmp_path, checkpoint=base, spl=5), baseline[1])      # and the run it belongs to still continues


def test_full_step_runs_resume_too(tmp_path, baseline):
    want = run(tmp_path / "a", velocities="full-step")
    assert all(np.array_equal(w[k], b[k]) for w, b in zip(want, baseline[1]) for k in ("step", "positions", "forces"))
    assert not np.array_equal(want[0]["velocities"], baseline[1][0]["velocities"])
    base = str(tmp_path / "fake")
    assert run(tmp_path / "b", velocities="full-step", checkpoint=base, max_steps=12) is None
    before = open(S.checkpoint_path(base), "rb").read()
    with pytest.raises(ValueError, match="`velocities`"):
        run(tmp_path / "b", checkpoint=base)
    assert open(S.checkpoint_path(base), "rb").read() == before
    assert same_rows(run(tmp_path / "b", velocities="full-step", checkpoint=base, spl=5, segment_frames=2), want)
    with pytest.raises(ValueError, match="velocities"):
        run(tmp_path / "c", velocities="half-step")


def test_arguments_that_make_no_sense_are_refused(tmp_path):
    for kw in (dict(max_steps=3), dict(max_seconds=1.0), dict(segment_frames=0), dict(checkpoint=str(tmp_path / "x"), checkpoint_steps=0),
               dict(checkpoint=str(tmp_path / "x"), max_steps=-1)):
        with pytest.raises(ValueError):
            run(tmp_path, **kw)
    energy, masses, x, v = system()
    with pytest.raises(ValueError, match="somewhere to write"):
        S.simulate_trajectory(energy, masses, x, v, burn_in=3, sampling=24, spacing=S.RegularSpacing(4), integrator=FakeDynamics(masses), segment_frames=2)
    assert not os.path.exists(tmp_path / "x.checkpoint.npz")


# ---------------------------------------------------------------------------------------------
# 8: a leftover segment
# ---------------------------------------------------------------------------------------------
def test_a_leftover_segment_beyond_the_count_is_overwritten(tmp_path, baseline):
    base = str(tmp_path / "fake")
    assert run(tmp_path, checkpoint=base, max_steps=12, segment_frames=2) is None
    ck = S.read_checkpoint(S.checkpoint_path(base))
    assert ck["n_segments"] == 2 and os.path.exists(S.segment_path(base, 1)) and not os.path.exists(S.segment_path(base, 2))
    for leftover in (2, 3, 7):      # what a run killed between a segment's write and its checkpoint's leaves behind
        with open(S.segment_path(base, leftover), "wb") as f:
            f.write(open(S.segment_path(base, 0), "rb").read())
    got = run(tmp_path, checkpoint=base, spl=5, segment_frames=2)
    assert same_rows(got, baseline[1]) and same_files(tmp_path, baseline[0])      # nothing of the run is left but its two files


# ---------------------------------------------------------------------------------------------
# the files themselves
# ---------------------------------------------------------------------------------------------
def test_checkpoint_file_round_trip(tmp_path):
    energy, masses, x, v = system()
    md = FakeDynamics(masses)
    reports = np.array([9, 10, 13], dtype=np.int64)
    fp = S.run_fingerprint(energy, md, x, v, burn_in=3, sampling=24, seed=4, reports=reports, velocities="stored", redraw_velocities=False,
                           minimize=True, min_tol=2.0)
    assert set(fp) == set(S.FINGERPRINT_FIELDS)
    assert not {"steps_per_launch", "segment_frames", "checkpoint_steps", "checkpoint_seconds"} & set(fp)
    state = np.random.default_rng(0).standard_normal((N, 2, V, 3))
    path = str(tmp_path / "ck.npz")
    S.write_checkpoint(path, fp, steps_done=12, integrator_step=1000015, state=state, redrawn=True, n_segments=4, start_coords=x.numpy())
    ck = S.read_checkpoint(path)
    assert ck["fingerprint"] == fp and S.first_difference(ck["fingerprint"], fp) is None
    assert (ck["steps_done"], ck["integrator_step"], ck["redrawn"], ck["n_segments"]) == (12, 1000015, True, 4)
    assert ck["state"].dtype == np.float64 and np.array_equal(ck["state"], state) and np.array_equal(ck["report_steps"], reports)
    assert np.array_equal(ck["start_coords"], x.numpy())
    assert int(np.load(path)["version"]) == S.CHECKPOINT_VERSION == 1
    assert S.first_difference(ck["fingerprint"], {**fp, "kbT": 2.5, "min_tol": 3.0}) == "kbT"      # the first in the order of the fields
    with open(path, "wb") as f:
        np.savez(f, version=np.int64(2))
    with pytest.raises(ValueError, match="version 2"):
        S.read_checkpoint(path)


def test_files_appear_whole_or_not_at_all(tmp_path, monkeypatch, baseline):
    """Every file is written under another name and moved with `os.replace`: when the move fails, nothing - old or new - is
    visible under the final name, no temporary file stays, and the earlier checkpoint is the one a later call continues from."""
    base = str(tmp_path / "fake")
    assert run(tmp_path, checkpoint=base, max_steps=10) is None
    before = snapshot(tmp_path)
    seen = []

    def refuse(src, dst):
        seen.append((os.path.basename(src), os.path.basename(dst), os.path.exists(dst)))
        raise OSError("no move today")

    monkeypatch.setattr(os, "replace", refuse)
    with pytest.raises(OSError, match="no move today"):
        run(tmp_path, checkpoint=base, max_steps=9, spl=5)      # to step 19: reports 11, 13, 19 are buffered, then a segment is due
    monkeypatch.undo()
    assert seen == [("fake.segment-000001.npz.tmp", "fake.segment-000001.npz", False)]      # the segment first; under its own name only after the move
    assert snapshot(tmp_path) == before
    assert same_rows(run(tmp_path, checkpoint=base, spl=5), baseline[1])


def test_a_state_that_is_not_finite_is_never_saved(tmp_path):
    base = str(tmp_path / "fake")
    assert run(tmp_path, checkpoint=base, max_steps=10) is None
    before = snapshot(tmp_path)
    md = FakeDynamics(system()[1], poison=(15, 1))
    with pytest.raises(RuntimeError, match=r"replica\(s\) 1 is not finite after 17 steps.*previous one is left in place"):
        run(tmp_path, checkpoint=base, checkpoint_steps=7, md=md)
    assert snapshot(tmp_path) == before
    fresh = FakeDynamics(system()[1], poison=(1, 0))
    with pytest.raises(RuntimeError, match=r"replica\(s\) 0 is not finite after 3 steps: no checkpoint was written$"):
        run(tmp_path / "new", checkpoint=str(tmp_path / "new" / "fake"), max_steps=3, md=fresh)
    assert not os.path.exists(tmp_path / "new" / "fake.checkpoint.npz")


def test_next_launch_walks_the_plan_of_before():
    reports = S.report_steps(S.LogarithmicSpacing(10, 3), 3, 27)
    for spl in (1, 4, 7, 50):
        done, walked = 0, []
        while done < 27:
            n, rel = S.next_launch(done, 3, 27, reports, spl)
            walked.append((done, n, rel.tolist()))
            done += n
        assert walked == [(a, n, rel.tolist()) for a, n, rel in S.plan_launches(3, 24, reports, spl)]
    assert S.next_launch(10, 3, 27, reports, 7, stop_at=12)[0] == 2
    n, rel = S.next_launch(10, 3, 27, reports, 7, room=1)
    assert (n, rel.tolist()) == (1, [1])
    n, rel = S.next_launch(0, 0, 27, reports, 50, room=3)
    assert (n, rel.tolist()) == (11, [9, 10, 11])


# ---------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------
def test_parser_has_the_new_flags_with_defaults_that_change_nothing():
    a = S.build_parser().parse_args(["--out", "o"])
    assert (a.pdb, a.force_field, a.full_step_velocities, a.checkpoint_minutes, a.max_minutes, a.max_steps, a.segment_frames) == \
        (None, "amber99-implicit", False, 0.0, None, None, None)
    a = S.build_parser().parse_args("--out o --pdb x.pdb --force-field amber14-implicit --full-step-velocities --checkpoint-minutes 5 "
                                    "--max-minutes 1.5 --max-steps 9 --segment-frames 100".split())
    assert (a.pdb, a.force_field, a.full_step_velocities, a.checkpoint_minutes, a.max_minutes, a.max_steps, a.segment_frames) == \
        ("x.pdb", "amber14-implicit", True, 5.0, 1.5, 9, 100)


def nnqq_pdb(path, keep=lambda name, res: True, rename=None):
    """The NNQQ peptide of tests/golden/energy_kat_2olx.npz as a PDB file: names, residues, ids and the first frame."""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "energy_kat_2olx.npz"))
    with open(path, "w") as f:
        f.write("REMARK   written by the tests\n")
        serial = 0
        for name, res, rid, el, xyz in zip(z["atom_names"], z["residue_names"], z["residue_ids"], z["elements"], z["positions"][0] * 10.0):
            name, res = str(name), str(res)
            if not keep(name, res):
                continue
            serial += 1
            res = (rename or {}).get(res, res)
            field = f" {name:<3s}" if len(name) < 4 else name
            f.write(f"ATOM  {serial:5d} {field} {res:>3s} A{int(rid):4d}    {xyz[0]:8.3f}{xyz[1]:8.3f}{xyz[2]:8.3f}  1.00  0.00          {str(el):>2s}\n")
        f.write("END\n")
    return z


def test_pdb_system_reads_topology_coordinates_and_masses(tmp_path):
    from timewarp_amd.forcefield import ELEMENT_MASSES, read_pdb_topology

    z = nnqq_pdb(tmp_path / "nnqq.pdb")
    energy, masses, coords, lines = S.pdb_system(str(tmp_path / "nnqq.pdb"))
    assert energy.tables.n_atoms == 65 and len(lines) == 65 and coords.dtype == torch.float32
    assert np.abs(coords.numpy() - z["positions"][0]).max() <= 0.5e-4 + 1e-7      # three decimals of an angstrom
    assert np.array_equal(masses.numpy(), np.array([ELEMENT_MASSES[str(e)] for e in z["elements"]], dtype=np.float32))
    S.write_state0_pdb(str(tmp_path / "state0.pdb"), lines, coords.numpy() + 0.1, "shifted by 1 angstrom")
    assert read_pdb_topology(str(tmp_path / "state0.pdb")) == read_pdb_topology(str(tmp_path / "nnqq.pdb"))
    again = S.pdb_system(str(tmp_path / "state0.pdb"))
    assert np.abs(again[2].numpy() - (coords.numpy() + 0.1)).max() <= 0.5e-4 + 1e-6
    assert open(tmp_path / "state0.pdb").readline().startswith("REMARK   shifted")


def test_pdb_files_that_cannot_be_simulated_exit_naming_the_problem(tmp_path):
    nnqq_pdb(tmp_path / "heavy.pdb", keep=lambda name, res: not name.startswith("H"))
    with pytest.raises(SystemExit, match="hydrogens"):
        S.pdb_system(str(tmp_path / "heavy.pdb"))
    nnqq_pdb(tmp_path / "odd.pdb", rename={"GLN": "XYZ"})
    with pytest.raises(SystemExit, match="XYZ"):
        S.pdb_system(str(tmp_path / "odd.pdb"))
    nnqq_pdb(tmp_path / "ok.pdb")
    with pytest.raises(SystemExit, match="amber77"):
        S.pdb_system(str(tmp_path / "ok.pdb"), "amber77")
    with pytest.raises(SystemExit, match="nowhere.pdb"):
        S.pdb_system(str(tmp_path / "nowhere.pdb"))
    with pytest.raises(SystemExit, match="alanine-dipeptide"):      # the presets are what they were
        S.preset_system("nnqq")


def test_main_returns_three_when_the_run_stopped_early(monkeypatch, tmp_path, capsys):
    nnqq_pdb(tmp_path / "nnqq.pdb")
    seen, answer = {}, {}

    def driver(energy, masses, coords, velocs=None, **kw):
        seen.clear()
        seen.update(kw, n_atoms=energy.tables.n_atoms, coords=coords)
        if "stats" in kw:
            kw["stats"].update(steps_done=9, start_coords=coords.numpy() + 0.05)
        if answer["rows"] is None:
            return None
        row = {"step": np.array([4, 8]), "time": np.array([0.002, 0.004]), "energies": np.ones((2, 2)), "positions": np.zeros((2, 65, 3), np.float32)}
        return [row] * coords.shape[0]

    monkeypatch.setattr(S, "simulate_trajectory", driver)
    out = str(tmp_path / "runs")
    os.makedirs(out)
    argv = f"--pdb {tmp_path / 'nnqq.pdb'} --burn-in 2 --sampling 12 --spacing 4 --spacing-approach regular --replicas 2 --out {out}".split()
    answer["rows"] = None
    assert S.main(argv + ["--max-steps", "9", "--checkpoint-minutes", "1", "--full-step-velocities", "--segment-frames", "4"], device="cpu") == 3
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1 and "stopped after step 9 of 14" in lines[0] and "same command continues" in lines[0] and "nnqq.checkpoint.npz" in lines[0]
    assert seen["n_atoms"] == 65 and seen["coords"].shape == (2, 65, 3) and seen["name"] == "nnqq"
    assert (seen["checkpoint"], seen["checkpoint_seconds"], seen["max_steps"], seen["velocities"], seen["segment_frames"]) == \
        (os.path.join(out, "nnqq"), 60.0, 9, "full-step", 4)
    assert os.listdir(out) == []
    answer["rows"] = "complete"
    assert S.main(argv + ["--max-minutes", "2"], device="cpu") == 0
    assert seen["max_seconds"] == 120.0 and "checkpoint_seconds" not in seen and "velocities" not in seen and "segment_frames" not in seen
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and "nnqq-1-traj-arrays.npz" in lines[1]
    assert os.listdir(out) == ["nnqq-traj-state0.pdb"]
    state0 = S.pdb_system(os.path.join(out, "nnqq-traj-state0.pdb"))
    assert np.abs(state0[2].numpy() - (seen["coords"][0].numpy() + 0.05)).max() <= 0.5e-4 + 1e-6
    # without any of the new flags the driver is called as before
    assert S.main(f"--burn-in 2 --sampling 12 --spacing 4 --spacing-approach regular --out {out}".split(), device="cpu") == 0
    assert not {"stats", "checkpoint", "velocities", "segment_frames", "max_steps", "max_seconds", "checkpoint_seconds"} & set(seen)
