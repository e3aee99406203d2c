"""The command line of timewarp_amd/simulation.py and the driver's refusals, without a GPU: argument parsing, `make_spacing`,
`preset_system`, `main` down to the call of `simulate_trajectory` (with the driver replaced, and with the real driver up to the
point where the integrator refuses a CPU tensor), the early refusal of a run that would record nothing, and the rules of
`LangevinDynamics.trajectory` for `coords` / `velocs` beside a `state`."""
import numpy as np
import pytest
import torch

from timewarp_amd import simulation as S


def test_parser_defaults_and_flags():
    a = S.build_parser().parse_args(["--out", "runs/x"])
    assert (a.preset, a.burn_in, a.sampling, a.spacing, a.spacing_approach, a.seed, a.replicas, a.out) == \
        ("alanine-dipeptide", 2000, 20000, 1000, "logarithmic", 0, 1, "runs/x")
    a = S.build_parser().parse_args("--preset p --burn-in 3 --sampling 24 --spacing 10 --spacing-approach windowed --seed 7 --replicas 4 --out o".split())
    assert (a.preset, a.burn_in, a.sampling, a.spacing, a.spacing_approach, a.seed, a.replicas, a.out) == ("p", 3, 24, 10, "windowed", 7, 4, "o")
    for bad in (["--sampling", "5"], ["--out", "o", "--spacing-approach", "cubic"], ["--out", "o", "--burn-in", "many"]):
        with pytest.raises(SystemExit):      # --out is required; unknown approach; not a number
            S.build_parser().parse_args(bad)


def test_make_spacing_builds_the_three_policies():
    """regular; logarithmic with factor 10; windowed with window 200 and 10 subsamples, seeded (simulate_trajectory.py:208-232)"""
    r, l, w = S.make_spacing("regular", 7), S.make_spacing("logarithmic", 1000), S.make_spacing("windowed", 1000, seed=3)
    assert isinstance(r, S.RegularSpacing) and r.report_interval == 7
    assert isinstance(l, S.LogarithmicSpacing) and (l.report_interval, l.space_factor) == (1000, 10)
    assert isinstance(w, S.UniformWindowedSpacing) and (w.report_interval, w.spacing_window, w.subsamples) == (1000, 200, 10)
    again = S.make_spacing("windowed", 1000, seed=3)
    assert np.array_equal(S.report_steps(w, 0, 5000), S.report_steps(again, 0, 5000))       # the seed reaches the policy
    with pytest.raises(ValueError):
        S.make_spacing("cubic", 10)
    with pytest.raises(ValueError):
        S.make_spacing("windowed", 399)      # windows of 2 x 200 steps would overlap


def test_preset_system_is_alanine_dipeptide_and_nothing_else():
    from timewarp_amd import synthetic

    energy, masses, coords = S.preset_system("alanine-dipeptide")
    assert energy.tables.n_atoms == 22 and masses.shape == (22,) and coords.shape == (22, 3)
    assert torch.equal(coords, synthetic.alanine_dipeptide_state()[1])      # the ideal-geometry coordinates, not a minimised state
    with pytest.raises(SystemExit, match="alanine-dipeptide"):
        S.preset_system("chignolin")


def test_main_hands_its_arguments_to_the_driver(monkeypatch, tmp_path, capsys):
    seen = {}

    def driver(energy, masses, coords, velocs=None, **kw):
        seen.update(kw, coords=coords, n_atoms=energy.tables.n_atoms)
        T = 2
        row = {"step": np.array([4, 8]), "time": np.array([0.002, 0.004]), "energies": np.ones((T, 2)), "positions": np.zeros((T, 22, 3), np.float32)}
        return [row] * coords.shape[0]

    monkeypatch.setattr(S, "simulate_trajectory", driver)
    out = str(tmp_path / "runs")
    assert S.main(f"--burn-in 3 --sampling 24 --spacing 4 --spacing-approach regular --seed 5 --replicas 3 --out {out}".split(), device="cpu") == 0
    assert seen["coords"].shape == (3, 22, 3) and seen["coords"].dtype == torch.float32 and seen["n_atoms"] == 22
    assert torch.equal(seen["coords"][0], seen["coords"][2])      # replicas start from one conformation
    assert (seen["burn_in"], seen["sampling"], seen["seed"], seen["out_dir"], seen["name"]) == (3, 24, 5, out, "alanine-dipeptide")
    assert isinstance(seen["spacing"], S.RegularSpacing) and seen["spacing"].report_interval == 4
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 3 and "alanine-dipeptide-1-traj-arrays.npz" in lines[1] and "2 frames, steps 4 .. 8" in lines[1]
    with pytest.raises(SystemExit):
        S.main(["--replicas", "0", "--out", out], device="cpu")


def test_main_reaches_the_integrator_which_has_no_cpu_path(tmp_path):
    """The real driver: parsed, preset built, velocities drawn, and then refused because the state is not on a GPU."""
    with pytest.raises(RuntimeError, match="no CPU fallback|MI355X"):
        S.main(["--burn-in", "2", "--sampling", "4", "--spacing", "2", "--spacing-approach", "regular", "--out", str(tmp_path)], device="cpu")
    assert not list(tmp_path.iterdir())


def test_a_run_that_records_nothing_is_refused_before_it_starts():
    """The report steps are known on the host: no integrator is built, no launch made (CPU tensors would raise RuntimeError)."""
    energy, masses, coords = S.preset_system("alanine-dipeptide")
    for burn_in, sampling, spacing in [(5, 5, S.RegularSpacing(100)), (13, 0, S.RegularSpacing(1))]:
        with pytest.raises(ValueError, match="nothing would be recorded"):
            S.simulate_trajectory(energy, masses, coords[None], burn_in=burn_in, sampling=sampling, spacing=spacing)


def test_trajectory_wants_coords_and_velocs_together_or_a_state():
    from timewarp_amd.md import LangevinDynamics

    energy, masses, coords = S.preset_system("alanine-dipeptide")
    md = LangevinDynamics.for_energy(energy, masses)
    x = coords[None]
    for c, v, state in [(None, None, None), (x, None, None), (None, x, None), (x, None, torch.zeros(1, 2, 22, 3, dtype=torch.float64))]:
        with pytest.raises(ValueError, match="both, or neither"):
            md.trajectory(c, v, [1], state=state)
    for state in (torch.zeros(1, 2, 22, 3), torch.zeros(1, 2, 21, 3, dtype=torch.float64), torch.zeros(2, 22, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="state: expected"):
            md.trajectory(None, None, [1], state=state)
    with pytest.raises(RuntimeError, match="no CPU fallback|MI355X"):      # a well-formed state, but not on a GPU
        md.trajectory(None, None, [1], state=torch.zeros(1, 2, 22, 3, dtype=torch.float64))
    assert md.steps_done == 0
