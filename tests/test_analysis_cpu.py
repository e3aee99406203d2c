"""The host side of timewarp_amd/analysis.py: the torsion index tables, the float64 restatement the GPU tests compare against
(tests/analysis_oracle.py), TICA from hand-built moments, the FFT autocorrelation against direct sums, Geyer's truncation, the
histograms, the binding, and the command line (its run needs the GPU and is skipped without one; its parsing is not)."""
import dataclasses
import os
import re
import warnings

import numpy as np
import pytest
import torch

from tests import analysis_oracle as ao
from tests.conftest import GOLDEN, ROOT
from timewarp_amd import analysis as an
from timewarp_amd import forcefield as ffm


def npz(name):
    return np.load(os.path.join(GOLDEN, name))


# ---- index tables -----------------------------------------------------------------------------------------------------------------

def test_alanine_dipeptide_tables():
    rid = {"ACE": 1, "ALA": 2, "NME": 3}
    t = an.torsion_indices(ffm.AD_ATOM_NAMES, ffm.AD_RESIDUES, [rid[r] for r in ffm.AD_RESIDUES])
    assert t["phi"].tolist() == [[4, 6, 8, 14]] and t["psi"].tolist() == [[6, 8, 14, 16]]
    for fam in ("omega", "chi1", "chi2", "chi3", "chi4"):   # ACE and NME have no CA
        assert t[fam].shape == (0, 4), fam
    assert all(v.dtype == np.int32 for v in t.values())


def test_1hgv_phi_count_and_dataclass_fields():
    """(the two facts the reference's tests/test_torsion_utils.py pins)"""
    z = npz("energy_kat_1hgv.npz")
    t = an.torsion_indices(z["atom_names"], z["residue_names"], z["residue_ids"])
    assert t["phi"].shape == (45, 4)
    names = [f.name for f in dataclasses.fields(an.TorsionAngles)]
    assert len(names) == 14
    assert names == ["phi", "psi", "chi1", "chi2", "chi3", "chi4", "omega"] + [
        f + "_indices" for f in ("phi", "psi", "chi1", "chi2", "chi3", "chi4", "omega")]


def test_nnqq_tables_are_bonded_chains():
    z = npz("energy_kat_2olx.npz")
    t = an.torsion_indices(z["atom_names"], z["residue_names"], z["residue_ids"])
    assert {f: len(t[f]) for f in an.FAMILIES} == dict(phi=3, psi=3, omega=3, chi1=4, chi2=4, chi3=2, chi4=0)
    bonds = ffm.amber99sbildn_obc_tables(list(z["atom_names"]), list(z["residue_names"]), list(z["residue_ids"])).bond_idx
    bonded = {frozenset(b) for b in bonds.tolist()}
    for fam in an.FAMILIES:
        for q in t[fam].tolist():
            assert len(set(q)) == 4
            assert all(frozenset(q[k:k + 2]) in bonded for k in range(3)), (fam, q)
    # rows are ordered by residue
    rid = z["residue_ids"]
    for fam in an.FAMILIES:
        first = rid[t[fam][:, 1]]
        assert (np.diff(first) >= 0).all(), fam


def test_index_range_check_and_pdb_reader(tmp_path):
    with pytest.raises(ValueError, match="0 .. 21"):
        an.check_indices(np.array([[0, 1, 2, 22]]), 22, "quads")
    with pytest.raises(ValueError):
        an.check_indices(np.array([-1]), 22, "atom_sel")
    z = npz("energy_kat_2olx.npz")
    pdb = write_pdb(tmp_path / "state0.pdb", z)
    names, res, rid = ffm.read_pdb_topology(pdb)
    assert names == list(z["atom_names"]) and res == list(z["residue_names"]) and rid == list(z["residue_ids"])
    assert ffm.tables_from_pdb(pdb).bond_idx.shape == ffm.amber99sbildn_obc_tables(names, res, rid).bond_idx.shape


def test_feature_tables_column_map():
    z = npz("energy_kat_2olx.npz")
    sel, quads, cols = an.feature_tables(z)
    names = z["atom_names"]
    assert [str(names[i])[0] for i in sel] == [c for c in (str(n)[0] for n in names) if c in "CNS"]
    t = an.torsion_indices(z["atom_names"], z["residue_names"], z["residue_ids"])
    assert (quads == np.concatenate([t["phi"], t["psi"], t["omega"]])).all()
    # per family: sines then cosines
    assert cols.tolist() == [[0, 3], [1, 4], [2, 5], [6, 9], [7, 10], [8, 11], [12, 15], [13, 16], [14, 17]]
    sel, quads, cols = an.feature_tables(z, use_dihedrals=False)
    assert len(quads) == 0 and len(cols) == 0 and len(sel) > 1


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("degrees", [60.0, -60.0, 180.0, 0.0, 135.0, -1.0])
def test_restatement_has_the_iupac_sign(degrees):
    p0, p1, p2 = np.array([0.1, 0.12, -0.03]), np.array([0.0, 0.0, 0.0]), np.array([0.02, -0.01, 0.15])
    p3 = ao.place_fourth(p0, p1, p2, np.deg2rad(degrees))
    got = ao.dihedrals(np.stack([p0, p1, p2, p3])[None], [[0, 1, 2, 3]])[0, 0]
    d = (got - np.deg2rad(degrees) + np.pi) % (2 * np.pi) - np.pi
    assert abs(d) < 1e-12, (degrees, np.rad2deg(got))


def test_restatement_is_rigid_motion_invariant():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(5, 9, 3))
    quads = np.array([[0, 1, 2, 3], [3, 4, 5, 6], [8, 2, 6, 1]])
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))       # a proper rotation
    moved = x @ q.T + rng.normal(size=3)
    assert np.abs(ao.dihedrals(moved, quads) - ao.dihedrals(x, quads)).max() < 1e-12
    # a reflection flips the sign
    assert np.abs(ao.dihedrals(x * np.array([1.0, 1.0, -1.0]), quads) + ao.dihedrals(x, quads)).max() < 1e-12


# ---- TICA from moments -----------------------------------------------------------------------------------------------------------

def hand_moments(A, lam, n=1000, mean=None):
    c0, ct = A @ A.T, A @ np.diag(lam) @ A.T
    F = A.shape[0]
    m = np.zeros(F) if mean is None else mean
    mm = np.outer(m, m)
    t = torch.as_tensor
    return an.Moments(n, 7, t(n * m), t(n * m), t(n * (c0 + mm)), t(n * (ct + mm)), t(n * (c0 + mm)))


def test_tica_from_hand_built_moments():
    rng = np.random.default_rng(1)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    A = q @ np.diag([1.0, 1.5, 2.0]) @ np.linalg.qr(rng.normal(size=(3, 3)))[0]    # condition number 2
    lam = np.array([0.9, 0.5, 0.1])
    mean = np.array([0.3, -2.0, 5.0])
    ev, proj, m = an.tica_from_moments(hand_moments(A, lam, mean=mean), dim=3)
    assert np.abs(ev.numpy() - lam).max() < 1e-10
    assert np.abs(m.numpy() - mean).max() < 1e-12
    # the projection whitens C0 and diagonalises Ctau
    P = proj.numpy()
    assert np.abs(P.T @ (A @ A.T) @ P - np.eye(3)).max() < 1e-9
    assert np.abs(P.T @ (A @ np.diag(lam) @ A.T) @ P - np.diag(lam)).max() < 1e-9
    ev2, proj2, _ = an.tica_from_moments(hand_moments(A, lam), dim=2)
    assert ev2.shape == (2,) and proj2.shape == (3, 2) and np.abs(ev2.numpy() - lam[:2]).max() < 1e-10


def test_tica_rank_deficient_c0_loses_one_direction():
    rng = np.random.default_rng(2)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    A = q @ np.diag([1.0, 1.5, 2.0])
    A4 = np.concatenate([A, A[:1]], axis=0)          # feature 3 duplicates feature 0: C0 is 4 x 4 of rank 3
    lam = np.array([0.9, 0.5, 0.1])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ev, proj, _ = an.tica_from_moments(hand_moments(A4, lam), dim=4)
    assert ev.shape == (3,) and proj.shape == (4, 3)
    assert np.abs(ev.numpy() - lam).max() < 1e-9


# ---- autocorrelation and ESS -------------------------------------------------------------------------------------------------------

def ar1(n_chains, T, n_obs, phi, seed):
    rng = np.random.default_rng(seed)
    e = rng.normal(size=(n_chains, T, n_obs))
    s = np.zeros_like(e)
    s[:, 0] = e[:, 0]
    for t in range(1, T):
        s[:, t] = phi * s[:, t - 1] + e[:, t]
    return s


def test_fft_autocorrelation_matches_direct_sums():
    s = ar1(3, 257, 4, 0.8, 3) + np.array([0.0, 10.0, -3.0, 1e3])
    rho = an.autocorrelation(torch.as_tensor(s), 64)
    gamma = ao.autocovariance(s, 64)
    assert rho.shape == (65, 4) and rho.dtype == torch.float64
    assert np.abs(rho.numpy() - gamma / gamma[0]).max() < 1e-10
    assert (rho[0] == 1.0).all()
    with pytest.raises(ValueError):
        an.autocorrelation(torch.as_tensor(s), 257)


def test_geyer_truncation_on_a_hand_written_sequence():
    # pairs: (1 + 0.5) > 0, (0.2 - 0.1) > 0, (-0.3 + 0.1) <= 0 stops; the later positive pair must not be counted
    rho = torch.tensor([1.0, 0.5, 0.2, -0.1, -0.3, 0.1, 0.4, 0.4], dtype=torch.float64).reshape(-1, 1)
    assert float(an.geyer_tau(rho)) == pytest.approx(2 * (1.5 + 0.1) - 1, abs=1e-12)
    # 1 + 2 (0.5 + 0.2 - 0.1) = 2.2, the same thing
    assert float(an.geyer_tau(rho)) == pytest.approx(1 + 2 * (0.5 + 0.2 - 0.1), abs=1e-12)
    # an odd length ignores the unpaired tail; independent samples give tau = 1
    assert float(an.geyer_tau(torch.tensor([1.0, 0.0, 0.7], dtype=torch.float64).reshape(-1, 1))) == 1.0
    two = torch.tensor([[1.0, 1.0], [0.5, -0.5], [0.3, 0.3], [0.1, 0.1]], dtype=torch.float64)
    assert an.geyer_tau(two).tolist() == pytest.approx([2 * 1.9 - 1, 2 * (0.5 + 0.4) - 1])


def test_ess_of_ar1_and_of_a_constant():
    s = ar1(4, 4096, 1, 0.5, 4)
    ess = float(an.effective_sample_size(torch.as_tensor(s))[0])
    expect = 4 * 4096 * (1 - 0.5) / (1 + 0.5)         # N / tau, tau = (1 + phi) / (1 - phi)
    assert 0.8 * expect < ess < 1.25 * expect, (ess, expect)
    both = np.concatenate([s, np.full_like(s, 2.5)], axis=-1)
    with pytest.warns(RuntimeWarning, match="constant"):
        e2 = an.effective_sample_size(torch.as_tensor(both))
    assert float(e2[0]) == pytest.approx(ess) and torch.isnan(e2[1])
    # circular: the smaller of the two
    ang = torch.as_tensor(s)
    c = an.effective_sample_size(ang, circular=True)
    lo = torch.minimum(an.effective_sample_size(torch.sin(ang)), an.effective_sample_size(torch.cos(ang)))
    assert torch.equal(c, lo)


def test_histogram_and_free_energy():
    phi = torch.tensor([-np.pi, -np.pi + 1e-9, 0.0, np.pi, 1.0], dtype=torch.float64)
    psi = torch.tensor([-np.pi, -np.pi + 1e-9, 0.0, np.pi, -1.0], dtype=torch.float64)
    h = an.ramachandran_histogram(phi, psi, bins=4)
    assert h.shape == (4, 4) and int(h.sum()) == 5
    assert int(h[0, 0]) == 2 and int(h[2, 2]) == 1 and int(h[3, 3]) == 1 and int(h[2, 1]) == 1
    ref, _, _ = np.histogram2d(phi.numpy(), psi.numpy(), bins=4, range=[[-np.pi, np.pi]] * 2)
    assert (h.numpy() == ref).all()
    fe = an.free_energy(h)
    assert float(fe[0, 0]) == 0.0 and float(fe[2, 2]) == pytest.approx(np.log(2.0)) and torch.isinf(fe[0, 1])


# ---- binding and command line ------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_bound_and_built():
    from timewarp_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "timewarp_hip.h")).read()
    assert re.search(r"#define TW_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8
    for name, n_args in (("tw_dihedrals", 7), ("tw_tica_features", 11), ("tw_lagged_moments_workspace_len", 1), ("tw_lagged_moments", 9)):
        assert re.search(r"\b%s\(" % name, header), name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    assert "tw_analysis.hip" in build.SOURCES


def write_pdb(path, z):
    with open(path, "w") as f:
        for i, (a, r, k) in enumerate(zip(z["atom_names"], z["residue_names"], z["residue_ids"])):
            name = f" {a:<3s}" if len(a) < 4 else str(a)
            x, y, zz = z["positions"][0][i] * 10.0
            f.write(f"ATOM  {i + 1:5d} {name} {r:>3s} A{int(k):4d}    {x:8.3f}{y:8.3f}{zz:8.3f}  1.00  0.00\n")
        f.write("END\n")
    return str(path)


def test_cli_arguments():
    p = an.build_parser()
    a = p.parse_args(["x-traj-arrays.npz", "--pdb", "s.pdb"])
    assert (a.lag, a.dim, a.max_lag) == (500, 10, None)
    a = p.parse_args(["x.npz", "--pdb", "s.pdb", "--lag", "5", "--dim", "3", "--max-lag", "20"])
    assert (a.lag, a.dim, a.max_lag) == (5, 3, 20)
    with pytest.raises(SystemExit):
        p.parse_args(["x.npz"])                        # --pdb is required
    assert an.output_path("/d/nnqq-traj-arrays.npz") == "/d/nnqq-analysis.npz"
    assert an.output_path("run.npz") == "run-analysis.npz"


def gpu_library_usable():
    from timewarp_amd import _lib

    return torch.cuda.is_available() and os.path.exists(_lib.lib_path())


@pytest.mark.skipif(not gpu_library_usable(), reason="the command line featurises on the GPU: no GPU or no built library here")
def test_cli_on_40_frames(tmp_path):
    z = npz("energy_kat_2olx.npz")
    traj = tmp_path / "nnqq-traj-arrays.npz"
    np.savez(traj, positions=z["positions"], step=np.arange(40))
    pdb = write_pdb(tmp_path / "nnqq-traj-state0.pdb", z)
    out = an.main([str(traj), "--pdb", pdb, "--lag", "5", "--dim", "4", "--max-lag", "20", "--chunk-frames", "16"])
    assert out == str(tmp_path / "nnqq-analysis.npz")
    r = np.load(out)
    t = an.torsion_indices(z["atom_names"], z["residue_names"], z["residue_ids"])
    for fam in an.FAMILIES:
        assert r[fam].shape == (40, len(t[fam])) and (r[fam + "_indices"] == t[fam]).all() and r["ess_" + fam].shape == (len(t[fam]),)
    assert np.abs(r["phi"] - ao.dihedrals(z["positions"], t["phi"])).max() < 1e-6
    assert r["tica_eigenvalues"].shape == (4,) and r["tica_projection"].shape[1] == 4 and r["tics"].shape == (40, 2)
    assert (np.diff(r["tica_eigenvalues"]) <= 0).all() and int(r["n_pairs"]) == 35
