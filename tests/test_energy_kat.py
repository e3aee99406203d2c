"""The energy oracle (oracle/energy_oracle.c) and the product's amber99sb-ildn / OBC parameter tables against the
reference's own OpenMM known-answer data: simulation/testdata/implicit-2olx-traj-cpu-arrays.npz, the file
simulation/tests/test_md.py:35-83 checks OpenMM with (40 frames of NNQQ: E_pot and forces; committed as data in
tests/golden/energy_kat_2olx.npz by oracle/gen_golden.py).  The reference's tolerances there: energies atol 1e-3,
forces rtol 0.05 / atol 1e-2.

Two asparagine side-chain torsion series in the tables are FITTED (timewarp_amd/forcefield.py `_ASN_FITTED_TORSIONS`);
everything else is published parm99 / ff99SB / ff94 / OBC data.  `test_everything_but_the_fitted_torsions_is_pinned` shows what
this file pins without them.  r04: the series are fitted on every second frame of ALL the OpenMM data the reference holds
for this peptide (this file and three more trajectories: simulation/testdata/implicit-2olx-traj-arrays.npz,
testdata/output/2olx-traj-arrays.npz, testdata/smallest_molecule/2olx-traj-arrays.npz; tools/pin_energy/refit_asn.py) and
checked on frames the fit never saw: tests/golden/energy_kat_2olx_more.npz, 86 held-out frames of the three other files
(`test_held_out_frames_of_three_more_trajectories`) - the independent evidence r03's review asked for."""
import numpy as np
import pytest
import torch

from tests import helpers as H

ENERGY_ATOL = 1.5e-3    # kJ/mol per frame of |E| ~ 1690 (the reference test's own: 1e-3).  Measured: offset 2.3e-4, spread over
                        # the frames 2.5e-4 (r03: offset 1.2e-3 - the additive constant of the local fit)
FORCE_RMS_TOL = 0.02    # kJ/mol/nm rms over all components (|F| rms is 933; measured 0.008 = the file's float32 noise)


def kat():
    z = np.load(H.GOLDEN + "/energy_kat_2olx.npz")
    return z


def kat_tables(z):
    from timewarp_amd.forcefield import amber99sbildn_obc_tables

    return amber99sbildn_obc_tables(list(z["atom_names"]), list(z["residue_names"]), list(z["residue_ids"]))


def more():
    return np.load(H.GOLDEN + "/energy_kat_2olx_more.npz")


def old_openmm_improper(t, z):
    """Two of the extra files (testdata/output, testdata/smallest_molecule) were written by OpenMM 7.4.1 (their PDB headers),
    which walks an sp2 centre's neighbours in the iteration order of a Python SET of atom indices (by index mod 8 for three
    neighbours) when it places the AMBER impropers; 7.6 - which wrote the simulation/testdata files - and the 7.7 the
    reference pins walk them sorted, the ordering of the tables.  On this peptide the only improper that changes is the
    C-terminal carboxylate, (CA, OXT, C, O) instead of (CA, O, C, OXT).  Each file is compared with the ordering of the OpenMM
    that wrote it (with the other one its carboxylate forces are off by up to 220 kJ/mol/nm).  r04: the set-order rule
    (forcefield._improper, `improper_neighbour_order="pyset"`) replaces the hand-written swap - the protein file below, 691
    atoms with 62 impropers of eight kinds, is what shows that it IS the rule."""
    from timewarp_amd.forcefield import amber99sbildn_obc_tables

    names, rid = list(z["atom_names"]), list(z["residue_ids"])
    told = amber99sbildn_obc_tables(names, list(z["residue_names"]), rid, improper_neighbour_order="pyset")
    idx = {(r, n): i for i, (n, r) in enumerate(zip(names, rid))}
    C, CA, O, OXT = (idx[(4, n)] for n in ("C", "CA", "O", "OXT"))
    changed = [(tuple(a), tuple(b)) for a, b in zip(t.torsion_idx.tolist(), told.torsion_idx.tolist()) if a != b]
    assert changed == [((CA, O, C, OXT), (CA, OXT, C, O))] and np.array_equal(t.torsion_par, told.torsion_par)
    return told


def numerical_forces(tables, x, h=1e-4, atoms=None):
    """central differences of the C oracle in float64-accurate coordinates: x [F,V,3] -> [F,V,3] (rows of `atoms` only)"""
    F, V, _ = x.shape
    out = np.zeros((F, V, 3))
    for a in (range(V) if atoms is None else atoms):
        for c in range(3):
            xp, xm = x.copy(), x.copy()
            xp[:, a, c] += h
            xm[:, a, c] -= h
            ep, _ = H.oracle_energy(tables, xp, dtype=np.float64)
            em, _ = H.oracle_energy(tables, xm, dtype=np.float64)
            out[:, a, c] = -(ep - em) / (2 * h)
    return out


def test_oracle_energy_matches_openmm_known_answers():
    z = kat()
    t = kat_tables(z)
    assert abs(t.atom_par[:, 0].sum()) < 1e-9 and t.n_atoms == 65
    e, terms = H.oracle_energy(t, z["positions"])
    assert np.allclose(e, z["energies"][:, 0], rtol=0, atol=ENERGY_ATOL), np.abs(e - z["energies"][:, 0]).max()
    assert len({round(v, 6) for v in terms[0]}) == 5  # the five force groups all contribute


def test_oracle_forces_match_openmm_known_answers():
    z = kat()
    t = kat_tables(z)
    frames = [0, 7, 19, 39]
    f = numerical_forces(t, z["positions"][frames].astype(np.float64))
    ref = z["forces"][frames].astype(np.float64)
    assert np.sqrt(((f - ref) ** 2).mean()) < FORCE_RMS_TOL
    assert np.allclose(f, ref, rtol=0.05, atol=1e-2)  # per component, the reference's own tolerances (test_md.py:47)


def test_held_out_frames_of_three_more_trajectories():
    """86 frames of three OTHER OpenMM trajectories of the peptide that the reference holds (50 + 35 + 1), none of them used
    in the fit of the asparagine series (the fit took the even frames, these are odd ones): energies to 1.5e-3 kJ/mol with a
    spread of 3e-4, forces (central differences of the C oracle on six of them) to the float32 noise of the files.  The
    trajectories visit all three chi1 rotamers of both asparagines, where r02's local series was off by up to 40 kJ/mol."""
    z, m = kat(), more()
    t = kat_tables(z)
    assert m["positions"].shape == (86, 65, 3) and int(m["old_openmm"].sum()) == 36
    for old in (False, True):
        sel = m["old_openmm"] == old
        tt = old_openmm_improper(t, z) if old else t
        e, _ = H.oracle_energy(tt, m["positions"][sel])
        d = e - m["energies"][sel]
        assert np.abs(d).max() < ENERGY_ATOL and d.std() < 4e-4, (old, np.abs(d).max(), d.std())
        frames = np.where(sel)[0][[0, len(np.where(sel)[0]) // 2, -1]]
        f = numerical_forces(tt, m["positions"][frames].astype(np.float64))
        ref = m["forces"][frames].astype(np.float64)
        assert np.sqrt(((f - ref) ** 2).mean()) < FORCE_RMS_TOL
        assert np.allclose(f, ref, rtol=0.05, atol=1e-2)
    # the ordering matters, i.e. the comparison above is not vacuous: the 7.6 ordering on a 7.4.1 file is far off
    sel = m["old_openmm"]
    e, _ = H.oracle_energy(t, m["positions"][sel])
    assert np.abs(e - m["energies"][sel]).max() > 0.3


def test_everything_but_the_fitted_torsions_is_pinned():
    """Remove the two fitted series and refit them as free linear parameters (8 numbers + 1 constant against
    40 energies): the residual spread must still be at the noise level, i.e. all other terms are right on their own;
    and atoms no fitted torsion touches must already have the right forces."""
    from timewarp_amd import forcefield as ff

    z = kat()
    t = kat_tables(z)
    names, rid = list(z["atom_names"]), list(z["residue_ids"])
    idx = {(r, n): i for i, (n, r) in enumerate(zip(names, rid))}
    fitted_quads = {tuple(idx[(r, n)] for n in q) for r in (1, 2) for q in ff._ASN_FITTED_TORSIONS}
    keep = np.array([tuple(q) not in fitted_quads and tuple(q[::-1]) not in fitted_quads for q in t.torsion_idx])
    assert (~keep).sum() == 2 * sum(len(v) for v in ff._ASN_FITTED_TORSIONS.values())
    import dataclasses

    t0 = dataclasses.replace(t, torsion_idx=t.torsion_idx[keep], torsion_par=t.torsion_par[keep])
    frames = [0, 7, 19, 39]
    f = numerical_forces(t0, z["positions"][frames].astype(np.float64))
    ref = z["forces"][frames].astype(np.float64)
    touched = sorted({a for q in fitted_quads for a in q})
    untouched = [a for a in range(65) if a not in touched]
    assert np.sqrt(((f - ref)[:, untouched] ** 2).mean()) < FORCE_RMS_TOL
    assert np.sqrt(((f - ref)[:, touched] ** 2).mean()) > 10 * FORCE_RMS_TOL  # the fitted terms do matter there


def protein():
    return np.load(H.GOLDEN + "/energy_kat_1hgv.npz")


def protein_tables(z, order="pyset"):
    from timewarp_amd.forcefield import amber99sbildn_obc_tables

    return amber99sbildn_obc_tables(list(z["atom_names"]), list(z["residue_names"]), list(z["residue_ids"]),
                                    improper_neighbour_order=order)


def test_protein_with_18_residue_types_known_answers():
    """The reference's SECOND OpenMM known-answer file (testdata/output/1hgv-traj-arrays.npz: a 46-residue, 691-atom protein;
    NMET ... CGLY with ALA ARG ASN ASP GLN GLU GLY ILE LEU LYS PHE PRO SER THR TRP TYR VAL in between; positions, energies
    and forces of 140 frames, 12 of the odd ones committed as tests/golden/energy_kat_1hgv.npz by tools/pin_energy/pin_1hgv.py).
    The ff94 charges, parm99 / ff99SB parameters, the improper placement and the OBC radii of all these residues were written
    down and met this file at its float32 noise as they stood; the ILDN side-chain series of ILE / LEU / ASP were fitted to the
    EVEN frames (fit_ildn_1hgv.py), the asparagine series come from the other molecule.  Here: ABSOLUTE energies of the
    held-out frames to 6e-3 kJ/mol of -2490 (measured -0.0014 +- 0.0016 in float64; the oracle reads the float32 positions),
    forces on one residue of every type by central differences."""
    z = protein()
    t = protein_tables(z)
    assert t.n_atoms == 691 and abs(t.atom_par[:, 0].sum() - 2.0) < 1e-9   # net charge +2: NMET, 3 LYS, ARG / ASP, GLU, CGLY
    e, _ = H.oracle_energy(t, z["positions"])
    d = e - z["energies"]
    assert np.abs(d).max() < 6e-3 and d.std() < 2.5e-3, (np.abs(d).max(), d.std())
    names, res, rid = list(z["atom_names"]), list(z["residue_names"]), list(z["residue_ids"])
    first = {}
    for r, i in zip(res, rid):
        first.setdefault(("N" if i == rid[0] else "C" if i == rid[-1] else "") + r, i)
    assert len(first) == 19   # 17 residue types inside the chain + the NH3+ methionine + the COO- glycine
    # (central differences step over the 2 nm cutoff when a partner sits within h of it: such atoms are left out - 5 of 156)
    x5, h = z["positions"][5].astype(np.float64), 2e-5
    near_cutoff = lambda a: np.abs(np.linalg.norm(x5 - x5[a], axis=1) - t.cutoff).min() < 3 * h
    atoms = [a for a in range(691) if rid[a] in set(first.values()) and not names[a].startswith("H") and not near_cutoff(a)]
    assert len(atoms) > 145 and {res[a] for a in atoms} == set(res)
    f = numerical_forces(t, x5[None], h=h, atoms=atoms)[:, atoms]
    ref = z["forces"][[5]].astype(np.float64)[:, atoms]
    assert np.sqrt(((f - ref) ** 2).mean()) < FORCE_RMS_TOL, np.sqrt(((f - ref) ** 2).mean())
    assert np.allclose(f, ref, rtol=0.05, atol=1e-2)
    # not vacuous: with the neighbour order of the later OpenMM versions this 7.4.1 file is missed (19 impropers move)
    e76, _ = H.oracle_energy(protein_tables(z, "sorted"), z["positions"])
    assert np.abs(e76 - z["energies"]).max() > 0.1


@pytest.mark.gpu
def test_hip_kernels_on_the_whole_protein_against_openmm():
    """The HIP energy kernel and the analytic force kernel on all 691 atoms (one conformation per wave; the exclusion matrix
    is one bit per pair in LDS since r04, 60 KiB here) against what OpenMM wrote: 12 held-out frames, absolute energies and all
    12 x 691 x 3 force components.  Measured: energies within 3.8e-3 kJ/mol of -2490, forces 0.0016 kJ/mol/nm rms of 890."""
    from timewarp_amd.energy import AmberPotentialEnergyTorch

    z = protein()
    e = AmberPotentialEnergyTorch(protein_tables(z))
    x = torch.from_numpy(z["positions"]).cuda()
    en, f = e.energy_and_forces(x)
    d = en.cpu().numpy().reshape(-1) - z["energies"]
    print("protein, HIP kernels vs OpenMM: E - E_ref", d.round(4), "force rms", float(np.sqrt(((f.cpu().numpy() - z["forces"]) ** 2).mean())))
    assert np.abs(d).max() < 6e-3, d
    assert np.allclose(e(x).cpu().numpy().reshape(-1), en.cpu().numpy().reshape(-1), rtol=0, atol=5e-4)   # energy kernel (returned in the input's fp32) == force kernel's energy
    f, ref = f.cpu().numpy(), z["forces"].astype(np.float64)
    assert np.sqrt(((f - ref) ** 2).mean()) < 0.005
    assert np.allclose(f, ref, rtol=0.05, atol=1e-2)


@pytest.mark.gpu
def test_hip_kernels_on_segments_of_the_protein():
    """The HIP energy / force kernels run the whole 691-atom protein too (the test above; one bit per ordered pair of the exclusion
    matrix in LDS since r05).  This test adds what that one cannot localise: the parameter TABLES of the sixteen residue types the
    peptide files do not hold, segment by segment - five overlapping segments of the chain
    (cut at peptide bonds, 10 residues each, every residue type in at least one), energies and analytic forces against the C
    oracle on the same tables and coordinates."""
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from timewarp_amd.forcefield import amber99sbildn_obc_tables

    z = protein()
    names, res, rid = list(z["atom_names"]), list(z["residue_names"]), list(z["residue_ids"])
    order = list(dict.fromkeys(rid))
    seen = set()
    for start in (0, 9, 18, 27, 36):
        keep_res = set(order[start:start + 10])
        sel = [a for a in range(691) if rid[a] in keep_res]
        assert len(sel) < 240
        seen |= {res[a] for a in sel}
        t = amber99sbildn_obc_tables([names[a] for a in sel], [res[a] for a in sel], [rid[a] for a in sel])
        x = z["positions"][:, sel]
        e_ref, _ = H.oracle_energy(t, x)
        en, f = AmberPotentialEnergyTorch(t).energy_and_forces(torch.from_numpy(x).cuda())
        assert np.allclose(en.cpu().numpy(), e_ref, rtol=0, atol=1e-6 * np.abs(e_ref).max())
        atoms = list(range(0, len(sel), 7))
        fn = numerical_forces(t, x[[3]].astype(np.float64), atoms=atoms)[:, atoms]
        assert np.allclose(f.cpu().numpy()[[3]][:, atoms], fn, rtol=1e-4, atol=2e-2), np.abs(f.cpu().numpy()[[3]][:, atoms] - fn).max()
    assert len(seen) == 18


@pytest.mark.gpu
def test_hip_energy_kernel_small_molecule_build_on_short_segments():
    """Up to 64 atoms the energy kernel runs four waves per conformation with pair-parallel Born-radius sums (r05); the
    segments above and the peptide files are all larger.  Three-residue segments of the protein (every residue type again)
    against the C oracle: the energy kernel's own energy (`energy_and_terms`: amber_energy_kernel<4>) and the one-wave force
    kernel's (`energy_and_forces`: amber_forces_kernel<1>), and that kernel's forces - all 12 frames, every component - against
    the float64 autograd reference of tests/amber_oracle.py at the tolerance of tests/test_amber_kernels_gpu.py."""
    from tests import amber_oracle as ao
    from tests.test_amber_kernels_gpu import DIHEDRAL_ULPS, FORCE_MARGIN, REFERENCE_NOISE_F
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from timewarp_amd.forcefield import amber99sbildn_obc_tables

    z = protein()
    names, res, rid = list(z["atom_names"]), list(z["residue_names"]), list(z["residue_ids"])
    order = list(dict.fromkeys(rid))
    seen, sizes, worst = set(), [], 0.0
    for start in range(0, len(order) - 2, 2):
        keep_res = set(order[start:start + 3])
        sel = [a for a in range(691) if rid[a] in keep_res]
        if len(sel) > 64:
            continue
        sizes.append(len(sel))
        seen |= {res[a] for a in sel}
        t = amber99sbildn_obc_tables([names[a] for a in sel], [res[a] for a in sel], [rid[a] for a in sel])
        x = z["positions"][:, sel]
        e_ref, _ = H.oracle_energy(t, x)
        energy = AmberPotentialEnergyTorch(t)
        en, f = energy.energy_and_forces(torch.from_numpy(x).cuda())
        assert np.allclose(en.cpu().numpy(), e_ref, rtol=0, atol=1e-6 * np.abs(e_ref).max()), (start, len(sel))
        full, _ = energy.energy_and_terms(torch.from_numpy(x).cuda())
        assert np.allclose(full.cpu().numpy(), e_ref, rtol=0, atol=1e-6 * np.abs(e_ref).max()), (start, len(sel), "energy kernel")
        xd = ao.as_kernel_reads(x)
        assert float(ao.switch_margins(t, xd)["min_margin"].min()) > ao.MARGIN
        f_ref = ao.energy_and_forces(t, xd)[1].numpy()
        err = np.abs(f.cpu().numpy() - f_ref).max((1, 2)) / np.abs(f_ref).max((1, 2))
        worst = max(worst, float(err.max()))
        tol = FORCE_MARGIN * REFERENCE_NOISE_F["real"] + DIHEDRAL_ULPS * ao.dihedral_conditioning(t, xd).numpy()
        assert (err <= tol).all(), (start, len(sel), err, tol)
    print(f"three-residue segments: one-wave force kernel vs float64 autograd reference, worst {worst:.2e} of max|F|")
    assert len(seen) >= 16 and min(sizes) < 40 and max(sizes) > 55, (sorted(seen), sizes)


@pytest.mark.gpu
def test_hip_kernels_on_the_held_out_frames():
    """Energy and analytic forces of the HIP kernels on all 86 held-out frames (see above)."""
    from timewarp_amd.energy import AmberPotentialEnergyTorch

    z, m = kat(), more()
    t = kat_tables(z)
    for old in (False, True):
        sel = m["old_openmm"] == old
        e = AmberPotentialEnergyTorch(old_openmm_improper(t, z) if old else t)
        en, f = e.energy_and_forces(torch.from_numpy(m["positions"][sel]).cuda())
        assert np.allclose(en.cpu().numpy(), m["energies"][sel], rtol=0, atol=ENERGY_ATOL)
        f, ref = f.cpu().numpy(), m["forces"][sel].astype(np.float64)
        assert np.sqrt(((f - ref) ** 2).mean()) < 0.005          # measured 0.0017: these files store sharper forces than the 40-frame one
        assert np.allclose(f, ref, rtol=0.05, atol=1e-2)


@pytest.mark.gpu
def test_hip_energy_kernel_matches_openmm_known_answers():
    from timewarp_amd.energy import AmberPotentialEnergyTorch

    z = kat()
    e = AmberPotentialEnergyTorch(kat_tables(z))
    out = e(torch.from_numpy(z["positions"]).cuda()).double().cpu().numpy()[:, 0]
    assert np.allclose(out, z["energies"][:, 0], rtol=0, atol=0.02)  # the callable returns float32 like the bridge
    ref, _ = H.oracle_energy(e.tables, z["positions"])
    full, _ = e.energy_and_terms(torch.from_numpy(z["positions"]).cuda(), want_terms=True)
    assert np.allclose(full.cpu().numpy(), ref, rtol=1e-10, atol=1e-8)
    assert np.allclose(full.cpu().numpy(), z["energies"][:, 0], rtol=0, atol=ENERGY_ATOL)  # float64 path of the kernel
