"""Checkpoint, resume and segments of timewarp_amd/simulation.py `simulate_trajectory` on the device: a run that is stopped with
`max_steps` and continued - by a fresh `LangevinDynamics`, with other launch and segment sizes, by another process - writes the
files of the uninterrupted run, bit for bit in every key.  tests/test_md_checkpoint_cpu.py runs the same driver on a restated
integrator; here the state, the noise key and the frames are the kernel's.

Shapes: alanine dipeptide (22 atoms, 2 replicas, burn-in 3, sampling 24, LogarithmicSpacing(10, 3), 7 steps per launch - the run of
test_simulate_trajectory_writes_the_reference_file_format), NNQQ (65 atoms, 2 replicas, 14 steps), at most 65 steps."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_langevin_cpu import real_case
from tests.test_langevin_gpu import real_energy
from tests.test_md_checkpoint_cpu import KEYS, nnqq_pdb, same_files, same_rows
from timewarp_amd import simulation as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(tmp, mol="ad", *, spacing="log", burn_in=3, sampling=24, spl=7, md_seed=11, given_velocities=True, **kw):
    from timewarp_amd.md import LangevinDynamics

    _, masses, x0, v0 = real_case(mol)
    energy = real_energy(mol)
    x, v = torch.from_numpy(x0[:2]).cuda(), torch.from_numpy(v0[:2]).cuda()
    if spacing == "log":
        spacing = S.LogarithmicSpacing(10, 3)
    md = LangevinDynamics(energy, torch.from_numpy(masses), 0.0005, 0.3, "LangevinMiddleIntegrator", seed=md_seed)      # a fresh one every call
    return S.simulate_trajectory(energy, torch.from_numpy(masses), x, v if given_velocities else None, burn_in=burn_in, sampling=sampling,
                                 spacing=spacing, integrator=md, steps_per_launch=spl, out_dir=str(tmp), name=mol, seed=4, **kw)


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    d = tmp_path_factory.mktemp("A")
    rows = run(d)
    assert rows[0]["step"].tolist() == [9, 10, 11, 13, 19, 20, 21, 23]
    assert sorted(os.listdir(d)) == ["ad-0-traj-arrays.npz", "ad-1-traj-arrays.npz"]
    assert np.abs(rows[0]["forces"]).max() > 100.0 and not np.array_equal(rows[0]["positions"], rows[1]["positions"])
    return d, rows


@pytest.fixture(scope="module")
def baseline_redrawn(tmp_path_factory):
    d = tmp_path_factory.mktemp("A_redrawn")
    return d, run(d, redraw_velocities=True)


@pytest.mark.parametrize("cuts,redraw", [((2,), False), ((3,), False), ((3,), True), ((10,), False), ((12,), False), ((5, 16), False), ((5, 16), True)])
def test_resume_is_bit_exact(tmp_path, baseline, baseline_redrawn, cuts, redraw):
    """Cuts inside the burn-in, on the burn-in / sampling boundary (with the velocity redraw, which then falls after the cut), on a
    report step, between reports, and two cuts in one run; every continuation is a fresh LangevinDynamics with 5 steps per
    launch and another segment size."""
    want_dir, want = baseline_redrawn if redraw else baseline
    base = str(tmp_path / "ck" / "ad")
    done = 0
    for i, cut in enumerate(cuts):
        stats = {}
        assert run(tmp_path / "out", checkpoint=base, max_steps=cut - done, redraw_velocities=redraw, segment_frames=(2, 5)[i % 2],
                   spl=(7, 5)[i % 2], stats=stats) is None
        assert stats["steps_done"] == cut and stats["resumed_at"] == (done if i else None)
        done = cut
    ck = S.read_checkpoint(S.checkpoint_path(base))
    assert ck["steps_done"] == ck["integrator_step"] == done and ck["state"].shape == (2, 2, 22, 3) and ck["state"].dtype == np.float64
    got = run(tmp_path / "out", checkpoint=base, redraw_velocities=redraw, segment_frames=3, spl=5)
    assert same_rows(got, want) and same_files(tmp_path / "out", want_dir)
    assert os.listdir(tmp_path / "ck") == []
    if redraw:
        assert not np.array_equal(want[0]["velocities"], baseline[1][0]["velocities"])


def test_windowed_policy_is_not_needed_again(tmp_path):
    make = lambda: S.UniformWindowedSpacing(20, spacing_window=4, subsamples=3, seed=5)
    want = run(tmp_path / "a", spacing=make(), burn_in=5, sampling=60)
    assert want[0]["step"].tolist() == [19, 20, 21, 22, 37, 38, 39, 40, 56, 59, 60, 62]
    base = str(tmp_path / "ad")
    assert run(tmp_path / "b", spacing=make(), burn_in=5, sampling=60, checkpoint=base, max_steps=30) is None
    assert run(tmp_path / "b", spacing=make(), burn_in=5, sampling=60, checkpoint=base, max_steps=11, spl=5) is None      # stands at 41
    got = run(tmp_path / "b", spacing=None, burn_in=5, sampling=60, checkpoint=base, spl=5)      # no policy object at all
    assert same_rows(got, want) and same_files(tmp_path / "a", tmp_path / "b")


def test_segments_bound_the_frame_buffer(tmp_path, baseline):
    stats = {}
    got = run(tmp_path, segment_frames=3, stats=stats)
    assert same_rows(got, baseline[1]) and same_files(tmp_path, baseline[0])
    assert stats["max_buffered_frames"] == 3 and stats["segments"] == 3 and stats["checkpoints"] == 0


def test_full_step_runs_resume_and_do_not_mix(tmp_path, baseline):
    want = run(tmp_path / "a", velocities="full-step")
    assert all(np.array_equal(w[k], b[k]) for w, b in zip(want, baseline[1]) for k in ("step", "time", "positions", "forces"))
    assert all(np.array_equal(w["energies"][:, 0], b["energies"][:, 0]) for w, b in zip(want, baseline[1]))
    assert not np.array_equal(want[0]["velocities"], baseline[1][0]["velocities"])
    base = str(tmp_path / "ad")
    assert run(tmp_path / "b", velocities="full-step", checkpoint=base, max_steps=12) is None
    assert same_rows(run(tmp_path / "b", velocities="full-step", checkpoint=base, spl=5, segment_frames=2), want)
    # a checkpoint written with "stored" does not continue as "full-step", nor under another seed or burn-in
    assert run(tmp_path / "c", checkpoint=base, max_steps=12) is None
    before = open(S.checkpoint_path(base), "rb").read()
    for field, change in (("velocities", dict(velocities="full-step")), ("noise_seed", dict(md_seed=12)), ("burn_in", dict(burn_in=4, sampling=23))):
        with pytest.raises(ValueError, match=f"`{field}`"):
            run(tmp_path / "c", checkpoint=base, **change)
        assert open(S.checkpoint_path(base), "rb").read() == before
    assert same_rows(run(tmp_path / "c", checkpoint=base), baseline[1])


def test_the_minimiser_runs_once_across_an_interruption(tmp_path):
    log = []
    want = run(tmp_path / "a", minimize=True, given_velocities=False, minimization_log=log)
    assert len(log) == 1 and int(log[0][0].iterations.max()) > 0
    log, stats = [], {}
    base = str(tmp_path / "ad")
    assert run(tmp_path / "b", minimize=True, given_velocities=False, checkpoint=base, max_steps=2, minimization_log=log) is None
    got = run(tmp_path / "b", minimize=True, given_velocities=False, checkpoint=base, spl=5, minimization_log=log, stats=stats)
    assert len(log) == 1
    assert same_rows(got, want) and same_files(tmp_path / "a", tmp_path / "b")
    assert np.array_equal(stats["start_coords"], log[0][0].coords.cpu().numpy())      # where the MD started: the minimised state


def test_sixteen_waves_resume_too(tmp_path):
    args = dict(spacing=S.RegularSpacing(4), burn_in=2, sampling=12)
    want = run(tmp_path / "a", "nnqq", **args)
    assert want[0]["step"].tolist() == [4, 8, 12] and want[0]["positions"].shape == (3, 65, 3)
    base = str(tmp_path / "nnqq")
    assert run(tmp_path / "b", "nnqq", checkpoint=base, max_steps=7, **args) is None
    got = run(tmp_path / "b", "nnqq", checkpoint=base, spl=5, segment_frames=1, **args)
    assert same_rows(got, want) and same_files(tmp_path / "a", tmp_path / "b")


def test_a_leftover_segment_beyond_the_count_is_overwritten(tmp_path, baseline):
    base = str(tmp_path / "ad")
    assert run(tmp_path, checkpoint=base, max_steps=12, segment_frames=2) is None
    assert S.read_checkpoint(S.checkpoint_path(base))["n_segments"] == 2
    with open(S.segment_path(base, 2), "wb") as f:
        f.write(open(S.segment_path(base, 0), "rb").read())
    got = run(tmp_path, checkpoint=base, spl=5, segment_frames=2)
    assert same_rows(got, baseline[1]) and same_files(tmp_path, baseline[0])


def test_a_fresh_process_resumes(tmp_path):
    """`python -m timewarp_amd.simulation --pdb ... --max-steps 9` exits 3 with the stop line; the same command again exits 0 and
    leaves the files of an uninterrupted in-process run on the same system, the state0 PDB, and nothing else."""
    from timewarp_amd.forcefield import read_pdb_topology
    from timewarp_amd.md import LangevinDynamics

    pdb = str(tmp_path / "nnqq.pdb")
    nnqq_pdb(pdb)
    out = str(tmp_path / "runs")
    cmd = [sys.executable, "-m", "timewarp_amd.simulation", "--pdb", pdb, "--burn-in", "2", "--sampling", "12", "--spacing", "4",
           "--spacing-approach", "regular", "--replicas", "2", "--seed", "6", "--out", out, "--max-steps", "9", "--checkpoint-minutes", "1"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    first = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    assert first.returncode == 3, first.stderr[-2000:]
    assert "stopped after step 9 of 14" in first.stdout and "same command continues" in first.stdout
    assert sorted(os.listdir(out)) == ["nnqq.checkpoint.npz", "nnqq.segment-000000.npz"]
    second = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    assert second.returncode == 0, second.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["nnqq-0-traj-arrays.npz", "nnqq-1-traj-arrays.npz", "nnqq-traj-state0.pdb"]
    energy, masses, coords, _ = S.pdb_system(pdb)
    x = coords.cuda()[None].repeat(2, 1, 1)
    want = S.simulate_trajectory(energy, masses, x, burn_in=2, sampling=12, spacing=S.RegularSpacing(4), seed=6, out_dir=str(tmp_path / "direct"),
                                 name="nnqq", integrator=LangevinDynamics.for_energy(energy, masses, seed=6))
    assert want[0]["step"].tolist() == [4, 8, 12]
    for row in range(2):
        z = np.load(os.path.join(out, f"nnqq-{row}-traj-arrays.npz"))
        assert sorted(z.files) == sorted(KEYS) and all(np.array_equal(z[k], want[row][k]) and z[k].dtype == want[row][k].dtype for k in KEYS), row
    assert read_pdb_topology(os.path.join(out, "nnqq-traj-state0.pdb")) == read_pdb_topology(pdb)
    assert np.array_equal(S.pdb_system(os.path.join(out, "nnqq-traj-state0.pdb"))[2].numpy(), coords.numpy())      # no minimisation: the input
