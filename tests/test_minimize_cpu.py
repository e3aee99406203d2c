"""The float64 restatement of the device minimiser (tests/minimize_oracle.py) checked by itself, and the host side of the
feature - the new command-line flags, what `main` hands to the driver, the refusal of CPU tensors, the declaration and the
binding of `tw_minimize` - without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import minimize_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNCAPPED = 1e30     # a max_displacement that never caps a step


def bond_only_tables(r0=0.1, k=3.0e5):
    """(the tables of tests/test_langevin_cpu.py: two atoms, one harmonic bond, nothing else)"""
    from timewarp_amd.forcefield import ForceFieldTables

    z = lambda w, t=np.float64: np.zeros((0, w), dtype=t)
    return ForceFieldTables(bond_idx=np.array([[0, 1]], dtype=np.int32), bond_par=np.array([[r0, k]]), angle_idx=z(3, np.int32),
                            angle_par=z(2), torsion_idx=z(4, np.int32), torsion_par=z(3), exc_idx=z(2, np.int32), exc_par=z(3),
                            atom_par=np.array([[0.0, 0.3, 0.0, 0.15, 0.8]] * 2), has_gbsa=0)


def bond_start(length):
    """two atoms `length` apart along a direction with three non-zero components (every reduction has six non-zero terms)"""
    u = np.array([2.0, -1.0, 0.5]) / np.sqrt(5.25)
    a = np.array([0.02, 0.01, -0.03])
    return np.stack([a, a + length * u]).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("history", [6, 10])
def test_convex_quadratic_in_six_unknowns(history):
    """E = 1/2 x.A x - b.x, A symmetric positive definite with eigenvalues 1 .. 40, steps uncapped.  The run converges, the
    energy never rises, and the distance to the exact minimum A^-1 b is within |g| / lambda_min <= tolerance sqrt(6) / 1."""
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    A = Q @ np.diag([1.0, 2.5, 7.0, 11.0, 23.0, 40.0]) @ Q.T
    A = 0.5 * (A + A.T)
    b = rng.standard_normal(6)
    x0 = rng.standard_normal((2, 3))
    tol = 1e-9
    x, E, rms, its, evals, status, trace = mo.minimize(mo.quadratic_forces(A, b), x0, tol, 200, history, UNCAPPED)
    want = np.linalg.solve(A, b)
    print(f"history {history}: {its} iterations, {evals} evaluations, |x - x*| {np.abs(x.ravel() - want).max():.2e}, rms {rms:.2e}")
    assert status == 0 and rms <= tol and its < 60
    assert np.abs(x.ravel() - want).max() <= tol * np.sqrt(6.0) / 1.0
    assert abs(E - (-0.5 * b @ want)) <= 1e-12
    assert len(trace) == its + 1 and np.all(np.diff(trace) <= 0.0) and trace[-1] == E
    assert evals >= its + 1


@pytest.mark.parametrize("length", [0.13, 0.08])
def test_one_bond_stretched_and_compressed(length):
    """Two atoms, one harmonic bond (r0 = 0.1 nm, k = 3e5 kJ/mol/nm^2), analytic forces.  At convergence each atom feels
    |F| = k |r - r0| and rms^2 = 2 F^2 / 3V, so rms <= tolerance means E = 1/2 k (r - r0)^2 <= tolerance^2 3V / (4 k), inside
    the tolerance^2 3V / (2 k) asked for; |r| - r0 is bounded by the same relation."""
    r0, k, tol, V = 0.1, 3.0e5, 2.0, 2
    x, E, rms, its, evals, status, trace = mo.minimize(mo.bond_forces(r0, k), bond_start(length), tol, 100, 8, 0.01)
    r = np.linalg.norm(x[0] - x[1])
    print(f"start {length}: {its} iterations, {evals} evaluations, r {r:.9f}, E {E:.3e}, rms {rms:.3e}")
    assert status == 0 and rms <= tol
    assert 0.0 <= E <= tol ** 2 * 3 * V / (2 * k)
    assert abs(r - r0) <= np.sqrt(2.0 * (tol ** 2 * 3 * V / (2 * k)) / k)
    assert np.all(np.diff(trace) <= 0.0)
    # the cap: in the first (steepest-descent) step the coordinate that moved furthest moved by max_displacement
    first = mo.minimize(mo.bond_forces(r0, k), bond_start(length), tol, 1, 8, 0.01)
    assert abs(np.abs(first[0] - bond_start(length)).max() - 0.01) < 1e-12


def test_reversed_reductions_are_a_different_but_close_run():
    """`reverse=True` is the same algorithm with the sums taken in the opposite order: same counts, a state within 1e-12."""
    a = mo.minimize(mo.bond_forces(0.1, 3.0e5), bond_start(0.13), 1e-6, 100, 8, 0.01)
    b = mo.minimize(mo.bond_forces(0.1, 3.0e5), bond_start(0.13), 1e-6, 100, 8, 0.01, reverse=True)
    assert a[3:6] == b[3:6] and np.abs(a[0] - b[0]).max() < 1e-12


def test_status_codes_of_the_restatement():
    f = mo.bond_forces(0.1, 3.0e5)
    # zero gradient at the input: converged with 0 iterations and the 1 evaluation that found it out
    x0 = bond_start(0.1)
    x0[1] = x0[0] + np.array([0.1, 0.0, 0.0])
    x, E, rms, its, evals, status, trace = mo.minimize(f, x0, 0.0, 50, 8, 0.01)
    assert (status, its, evals) == (0, 0, 1) and np.array_equal(x, x0) and E == 0.0 and rms == 0.0 and len(trace) == 1
    # a NaN coordinate: status 3, nothing moved, no further evaluation
    bad = bond_start(0.13)
    bad[0, 0] = np.nan
    x, E, rms, its, evals, status, _ = mo.minimize(f, bad, 2.0, 50, 8, 0.01)
    assert (status, its, evals) == (3, 0, 1) and np.array_equal(x, bad, equal_nan=True)
    # both atoms at one point: r = 0, forces 0 / 0
    x, _, _, its, evals, status, _ = mo.minimize(f, np.zeros((2, 3)), 2.0, 50, 8, 0.01)
    assert (status, its, evals) == (3, 0, 1)
    # a budget of one iteration
    x, E, rms, its, evals, status, trace = mo.minimize(f, bond_start(0.13), 2.0, 1, 8, 0.01)
    assert status == 1 and its == 1 and evals >= 2 and trace[1] < trace[0]
    # no budget at all: the input state is evaluated
    assert mo.minimize(f, bond_start(0.13), 2.0, 0, 8, 0.01)[3:6] == (0, 1, 1)


def test_a_function_that_cannot_decrease_stalls():
    """E = -|x|^2 reported with forces of the wrong sign: every trial raises the energy, 21 rejections as steepest descent."""
    f = lambda x: ((x ** 2).sum((1, 2)), 2.0 * x)
    x0 = np.ones((1, 3))
    x, E, rms, its, evals, status, _ = mo.minimize(f, x0, 1e-3, 5, 4, 0.1)
    assert (status, its, evals) == (2, 0, 1 + 21) and np.array_equal(x, x0)


# ---------------------------------------------------------------------------------------------
# the command line and the driver's keywords
# ---------------------------------------------------------------------------------------------
def test_parser_flags_and_defaults():
    from timewarp_amd import simulation as S

    a = S.build_parser().parse_args(["--out", "o"])
    assert a.minimize is False and a.min_tol == 2.0 and a.redraw_velocities is False
    a = S.build_parser().parse_args("--out o --minimize --min-tol 0.5 --redraw-velocities".split())
    assert a.minimize is True and a.min_tol == 0.5 and a.redraw_velocities is True


def test_main_hands_the_new_options_to_the_driver(monkeypatch, tmp_path):
    from timewarp_amd import simulation as S

    seen = []

    def driver(energy, masses, coords, velocs=None, **kw):
        seen.append(kw)
        row = {"step": np.array([4, 8]), "time": np.array([0.002, 0.004]), "energies": np.ones((2, 2))}
        return [row] * coords.shape[0]

    monkeypatch.setattr(S, "simulate_trajectory", driver)
    base = f"--burn-in 3 --sampling 24 --spacing 4 --spacing-approach regular --out {tmp_path}".split()
    assert S.main(base, device="cpu") == 0
    assert S.main(base + "--minimize --min-tol 1.5 --redraw-velocities".split(), device="cpu") == 0
    assert (seen[0]["minimize"], seen[0]["min_tol"], seen[0]["redraw_velocities"]) == (False, 2.0, False)
    assert (seen[1]["minimize"], seen[1]["min_tol"], seen[1]["redraw_velocities"]) == (True, 1.5, True)


def test_driver_defaults_are_off_and_the_two_seeds_differ():
    import inspect

    from timewarp_amd import simulation as S

    p = inspect.signature(S.simulate_trajectory).parameters
    assert p["minimize"].default is False and p["min_tol"].default == 2.0 and p["redraw_velocities"].default is False
    for seed in (0, 1, 5, 2 ** 63, 2 ** 64 - 1, 0x9E3779B97F4A7C15, -3):
        first, again = S.velocity_seeds(seed)
        assert first != again and 0 <= first < 2 ** 63 and 0 <= again < 2 ** 63
    assert S.velocity_seeds(5)[0] == 5      # the initial draw is seeded as before


def test_minimize_energy_refuses_cpu_tensors():
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from timewarp_amd.md import minimize_energy

    energy = AmberPotentialEnergyTorch(bond_only_tables())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        minimize_energy(energy, torch.zeros(1, 2, 3))


def test_minimize_energy_signature_follows_openmm():
    import inspect

    from timewarp_amd import md

    p = inspect.signature(md.minimize_energy).parameters
    assert list(p)[:4] == ["energy", "coords", "tolerance", "max_iterations"]
    assert p["tolerance"].default == 10.0 and p["max_iterations"].default == 0
    assert 0.0 < p["max_displacement"].default <= 0.1 * 0.1      # at most a tenth of a 0.1 nm bond
    fields = {f.name for f in __import__("dataclasses").fields(md.MinimizationResult)}
    assert {"coords", "coords64", "energy", "rms_force", "iterations", "evaluations", "status", "converged"} <= fields
    # the default launch length: worst case (42 evaluations per iteration) near 0.2 s, never below one iteration
    assert md.default_iterations_per_launch(691) >= 1 and md.default_iterations_per_launch(22) > md.default_iterations_per_launch(691)


def test_tw_minimize_is_declared_and_bound():
    from timewarp_amd import _lib

    header = open(os.path.join(ROOT, "include", "timewarp_hip.h")).read()
    assert re.search(r"int64_t\s+tw_minimize_workspace_len\(int32_t n_atoms, int32_t history\);", header)
    assert re.search(r"int\s+tw_minimize\(const tw_forcefield\* ff, float\* coords", header)
    assert "#define TW_ABI_VERSION 8" in header
    assert len(_lib.SIGNATURES["tw_minimize"][1]) == 15 and len(_lib.SIGNATURES["tw_minimize_workspace_len"][1]) == 2
    api = open(os.path.join(ROOT, "timewarp_amd", "csrc", "tw_api.hip")).read()
    assert "int tw_minimize(" in api and "int64_t tw_minimize_workspace_len(" in api
