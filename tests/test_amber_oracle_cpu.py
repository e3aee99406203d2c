"""The float64 autograd reference of the AMBER kernels (tests/amber_oracle.py) checked on its own, without a GPU: against
the C oracle (energies, the five terms, central differences of its energy), the Born-integral branches each synthetic case is
named after, the exactness of the pairs placed on the cutoff, the distance of every case from every switch, and the
reference's own rounding noise - the number the GPU tolerance of tests/test_amber_kernels_gpu.py hangs on."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from tests import amber_oracle as ao
from tests import helpers as H
from tests.test_energy_kat import kat, kat_tables, numerical_forces, protein, protein_tables

# The reference's own rounding noise per family: energy_and_forces on the atoms as given and under a fixed random relabelling
# (all index tables remapped, forces mapped back), max |F_a - F_b| / max |F| of the conformation and |E_a - E_b| / |E|, the worst
# conformation of the worst case of the family.  Measured (forces / energy):
#   covalent 3.22e-16 / 1.33e-13   buried 1.24e-15 / 1.60e-15   skipped 2.47e-15 / 2.62e-15   constant_l 1.14e-15 / 1.99e-15
#   cutoff_exact 4.40e-16 / 7.58e-16   real 3.68e-16 / 1.34e-14
# The constants are these figures rounded up to a power of two with at least a quarter to spare: the order of torch's sums, which
# is what the experiment measures, depends on the host's vector width and thread count.
# test_reference_noise_stays_at_or_below_the_recorded_constants asserts the measurement stays at or below them.
# (The energy figures of `covalent` and `real` come from conformations whose terms cancel: |E| ~ 30 kJ/mol of ~ 1e3 per term.)
REFERENCE_NOISE_F = {"covalent": 2.0 ** -51, "buried": 2.0 ** -49, "skipped": 2.0 ** -48, "constant_l": 2.0 ** -49,
                     "cutoff_exact": 2.0 ** -50, "real": 2.0 ** -50}
REFERENCE_NOISE_E = {"covalent": 2.0 ** -42, "buried": 2.0 ** -48, "skipped": 2.0 ** -48, "constant_l": 2.0 ** -48,
                     "cutoff_exact": 2.0 ** -49, "real": 2.0 ** -45}

ENERGY_TOL = dict(rtol=1e-10, atol=1e-8)     # the project's own numbers between kernel and C oracle (test_energy_kat.py)
TERMS_TOL = dict(rtol=1e-9, atol=1e-8)
FD_TOL = 2e-6                                # central differences, of the largest component (test_md_gpu.py)

COVALENT_V = (1, 2, 3, 4, 22, 63, 64, 65, 66, 127, 128, 129, 192, 193)
SPECIAL_V = (22, 64, 65, 129)
SPECIAL_KINDS = ("buried", "skipped", "constant_l", "cutoff_exact")


def synthetic_cases(kind=None):
    """(V, kind, gb, cutoff) of every synthetic case the GPU tests run"""
    cases = [(V, "covalent", gb, rc) for V in COVALENT_V for gb in (1, 2, 0) for rc in (2.0, 0.6, 0.0)]
    cases += [(V, k, gb, ao.EXACT_CUTOFF if k == "cutoff_exact" else 2.0) for k in SPECIAL_KINDS for V in SPECIAL_V for gb in (1, 2)]
    return [c for c in cases if kind is None or c[1] == kind]


@functools.lru_cache(maxsize=None)
def synthetic(case):
    """(tables, x float32 [5, V, 3], exact [5, V, V]) - built once, shared, read-only"""
    t, x, exact = ao.synthetic_case(*case)
    x.setflags(write=False)
    exact.setflags(write=False)
    return t, x, exact


def segments(z, length, step, most=10 ** 9):
    """(tables, atom selection) of the segments of the protein that test_energy_kat.py cuts: `length` residues from every `step`-th"""
    from timewarp_amd.forcefield import amber99sbildn_obc_tables

    names, res, rid = list(z["atom_names"]), list(z["residue_names"]), list(z["residue_ids"])
    order = list(dict.fromkeys(rid))
    out = []
    for start in (range(0, len(order) - 2, step) if length == 3 else (0, 9, 18, 27, 36)):
        keep = set(order[start:start + length])
        sel = [a for a in range(len(names)) if rid[a] in keep]
        if len(sel) <= most:
            out.append((amber99sbildn_obc_tables([names[a] for a in sel], [res[a] for a in sel], [rid[a] for a in sel]), sel))
    return out


@functools.lru_cache(maxsize=None)
def real_cases():
    """name -> (tables, x float32 [N, V, 3]): alanine dipeptide in the three GBSA modes (six jittered conformations, one of them
    stretched 2.2 times), NNQQ frames 0 / 7 / 19 / 39, frame 5 of the 691-atom protein, frames 0 and 5 of its five ten-residue
    segments and of its three-residue segments up to 64 atoms"""
    from timewarp_amd.forcefield import alanine_dipeptide_amber99sb

    out = {}
    d, _ = H.load("kernel_full_ad")
    x = d["x_coords"] + torch.randn(6, 22, 3, generator=torch.Generator().manual_seed(2)) * 0.01
    x[5] = x[4] * 2.2          # (a jittered one: the file's own conformation has an exactly planar torsion)
    ad = alanine_dipeptide_amber99sb()
    for gb in (1, 2, 0):
        out[f"alanine dipeptide gb={gb}"] = (dataclasses.replace(ad, has_gbsa=gb), x.numpy().astype(np.float32))
    z = kat()
    out["NNQQ"] = (kat_tables(z), z["positions"][[0, 7, 19, 39]].astype(np.float32))
    zp = protein()
    out["protein frame 5"] = (protein_tables(zp), zp["positions"][[5]].astype(np.float32))
    for n, (t, sel) in enumerate(segments(zp, 10, 9)):
        out[f"ten residues #{n}"] = (t, zp["positions"][[0, 5]][:, sel].astype(np.float32))
    for n, (t, sel) in enumerate(segments(zp, 3, 2, most=64)):
        out[f"three residues #{n}"] = (t, zp["positions"][[0, 5]][:, sel].astype(np.float32))
    return out


@functools.lru_cache(maxsize=None)
def reference(key):
    """(E [N], terms [N, 5], F [N, V, 3]) float64 numpy of a synthetic case tuple or a real case name: computed once, shared"""
    t, x = synthetic(key)[:2] if isinstance(key, tuple) else real_cases()[key]
    xd = ao.as_kernel_reads(x)
    e, f = ao.energy_and_forces(t, xd)
    out = e.numpy(), ao.energy_terms(t, xd).numpy(), f.numpy()
    for a in out:
        a.setflags(write=False)
    return out


def assert_matches_c_oracle(t, x, key):
    e_c, terms_c = H.oracle_energy(t, np.asarray(x, dtype=np.float32))
    e, terms, _ = reference(key)
    assert np.allclose(terms, terms_c, **TERMS_TOL), (key, np.abs(terms - terms_c).max(0))
    assert np.allclose(e, e_c, **ENERGY_TOL), (key, np.abs(e - e_c).max())
    assert np.allclose(terms.sum(1), e, rtol=1e-13, atol=1e-9)


def test_reference_matches_the_c_oracle_on_real_molecules():
    for name, (t, x) in real_cases().items():
        assert_matches_c_oracle(t, x, name)


@pytest.mark.parametrize("kind", ao.KINDS)
def test_reference_matches_the_c_oracle_on_every_synthetic_case(kind):
    for case in synthetic_cases(kind):
        t, x, _ = synthetic(case)
        assert_matches_c_oracle(t, x, case)


def test_synthetic_parameters_are_all_distinct():
    """a swapped index cannot cancel: no two atoms and no two terms of a kind share a parameter"""
    for case in [(65, k, 1, 2.0) for k in ao.KINDS]:
        t = synthetic(case)[0]
        for name, cols in (("atom_par", range(5)), ("bond_par", range(2)), ("angle_par", range(2)), ("torsion_par", (1, 2))):
            a = getattr(t, name)
            for c in cols:
                assert len(np.unique(a[:, c])) == len(a), (case, name, c)
        live = t.exc_par[:, 0] != 0.0
        assert live.sum() == 62 and len(np.unique(t.exc_par[live, 0])) == 62 and not t.exc_par[~live][:, [0, 2]].any()
        assert set(t.torsion_par[:, 0]) == {1.0, 2.0, 3.0, 4.0} and (t.torsion_par[:, 1] != 0.0).all()
        assert abs(t.atom_par[:, 0].sum()) > 0.1


FD_CASES = [f"alanine dipeptide gb={gb}" for gb in (1, 2, 0)] + [(22, "buried", 1, 2.0), (22, "skipped", 2, 2.0)]


@pytest.mark.parametrize("key", FD_CASES, ids=str)
def test_autograd_forces_match_central_differences_of_the_c_oracle(key):
    t, x = synthetic(key)[:2] if isinstance(key, tuple) else real_cases()[key]
    _, _, f = reference(key)
    fd = numerical_forces(t, ao.as_kernel_reads(x).numpy(), h=1e-5)
    err = np.abs(f - fd).max() / np.abs(fd).max()
    print(f"{key}: autograd vs central differences {err:.2e} of the largest component")
    assert err < FD_TOL, err


@pytest.mark.parametrize("kind", SPECIAL_KINDS)
def test_named_cases_take_the_branch_they_are_named_after(kind):
    """Counted on the first (least jittered) conformation: at least V/4 ordered pairs in the named Born branch; cutoff_exact: pairs
    on the cutoff in every unstretched conformation, and many beyond it.  Every count a GPU test relies on is above zero."""
    for case in synthetic_cases(kind):
        t, x, _ = synthetic(case)
        V = case[0]
        n = ao.branch_counts(t, ao.as_kernel_reads(x))
        print(case, {k: v.tolist() for k, v in n.items()})
        if kind == "cutoff_exact":
            assert (n["on_cutoff"][:-1] > 0).all() and n["on_cutoff"][-1] == 0
            assert int(n["on_cutoff"][:-1].sum()) >= (V // 5) * 4 // 3          # a third of the rows' pairs, four conformations
            assert (n["beyond_cutoff"] >= V).all()
            assert (n["constant_l"][:-1] > 0).all() and (n["moving_l"] > 0).all()
        else:
            assert int(n[kind][0]) >= V / 4, (case, n[kind])
            assert (n[kind][:-1] > 0).all()
    # the covalent cases: the constant lower limit and the moving one both occur, the cutoff 0.6 leaves most pairs outside
    for case in synthetic_cases("covalent"):
        V, _, gb, rc = case
        if V < 22:
            continue
        t, x, _ = synthetic(case)
        n = ao.branch_counts(t, ao.as_kernel_reads(x))
        assert (n["constant_l"][:-1] > 0).all() and (n["moving_l"] > 0).all()
        if rc == 0.6 and V >= 63:
            assert (2 * n["beyond_cutoff"] > V * (V - 1) // 2).all()


def test_the_exact_pairs_of_cutoff_exact_are_exact():
    """r of the marked pairs, computed in float64 from the float32 coordinates as both kernels do (dx dx + dy dy + dz dz, then the
    root), is exactly 0.5, the float32 below it or the float32 above it - all three occur in every case - and the pairs are
    not excluded, so the nonbonded `r >= rc` and the GB `r > rc` are both decided on the value itself."""
    for case in synthetic_cases("cutoff_exact"):
        t, x, exact = synthetic(case)
        xd = ao.as_kernel_reads(x).numpy()
        excluded = {tuple(sorted(p)) for p in t.exc_idx.tolist()}
        seen = set()
        for c in range(ao.N_CONFORMATIONS):
            for i, j in zip(*np.nonzero(np.tril(exact[c]))):
                d = xd[c, i] - xd[c, j]
                r = float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
                assert r in ao.EXACT_DISTANCES and np.count_nonzero(d) == 1 and tuple(sorted((i, j))) not in excluded
                seen.add((r, int(np.nonzero(d)[0][0])))
        assert not exact[-1].any() and {r for r, _ in seen} == set(ao.EXACT_DISTANCES) and {a for _, a in seen} == {0, 1, 2}
        assert t.cutoff == 0.5 and ao.EXACT_DISTANCES[1] < 0.5 < ao.EXACT_DISTANCES[2]


@pytest.mark.parametrize("kind", ao.KINDS)
def test_every_synthetic_case_keeps_its_distance_from_every_switch(kind):
    """switch_margins > 1e-6 (nm; 1e-6 for the cosines and sines): kernel and reference cannot sit on different sides of a branch.
    The exact pairs of cutoff_exact are left out of |r - rc| only (asserted exact above)."""
    for case in synthetic_cases(kind):
        t, x, exact = synthetic(case)
        m = ao.switch_margins(t, ao.as_kernel_reads(x), exact)
        worst = min(m, key=lambda k: float(m[k].min()))
        assert float(m["min_margin"].min()) > ao.MARGIN, (case, worst, m[worst])


def test_real_molecules_keep_their_distance_from_every_switch():
    for name, (t, x) in real_cases().items():
        m = ao.switch_margins(t, ao.as_kernel_reads(x))
        worst = min(m, key=lambda k: float(m[k].min()))
        assert float(m["min_margin"].min()) > ao.MARGIN, (name, worst, m[worst])


@pytest.mark.parametrize("kind", ("buried", "skipped", "constant_l"))
def test_gb_is_a_visible_share_of_the_forces_of_the_born_cases(kind):
    """max |F_GB| / max |F| per conformation: at least 10 %, so that a wrong Born derivative cannot hide under the other terms"""
    for case in synthetic_cases(kind):
        t, x, _ = synthetic(case)
        f = reference(case)[2]
        f_gb = ao.energy_and_forces(t, ao.as_kernel_reads(x), term=4)[1].numpy()
        share = np.abs(f_gb).max((1, 2)) / np.abs(f).max((1, 2))
        print(case, "share of GB in max|F| per conformation:", share.round(3))
        assert (share >= 0.10).all(), (case, share)


def measured_noise(family):
    keys = list(real_cases()) if family == "real" else synthetic_cases(family)
    worst_f = worst_e = 0.0
    for key in keys:
        t, x = synthetic(key)[:2] if isinstance(key, tuple) else real_cases()[key]
        nf, ne = ao.relabelling_noise(t, ao.as_kernel_reads(x))
        worst_f, worst_e = max(worst_f, nf), max(worst_e, ne)
    return worst_f, worst_e


@pytest.mark.parametrize("family", list(REFERENCE_NOISE_F))
def test_reference_noise_stays_at_or_below_the_recorded_constants(family):
    nf, ne = measured_noise(family)
    print(f"{family}: relabelling noise of the reference: forces {nf:.2e} of max|F|, energy {ne:.2e} of |E| "
          f"(recorded {REFERENCE_NOISE_F[family]:.2e}, {REFERENCE_NOISE_E[family]:.2e})")
    assert 0.0 < nf <= REFERENCE_NOISE_F[family] and ne <= REFERENCE_NOISE_E[family]


def test_relabelling_is_the_same_molecule():
    """the experiment above is not vacuous: the relabelled tables differ, the energies agree to rounding, and the C oracle agrees
    on the relabelled molecule too"""
    t, x, _ = synthetic((22, "buried", 1, 2.0))
    perm = np.random.default_rng(3).permutation(22)
    t2, inv = ao.relabel(t, perm)
    assert not np.array_equal(t2.bond_idx, t.bond_idx) and np.array_equal(perm[t2.bond_idx], t.bond_idx)
    e1, _ = H.oracle_energy(t, x)
    e2, _ = H.oracle_energy(t2, x[:, perm])
    assert np.allclose(e1, e2, rtol=1e-13)
    f1 = ao.energy_and_forces(t, ao.as_kernel_reads(x))[1]
    f2 = ao.energy_and_forces(t2, ao.as_kernel_reads(x[:, perm]))[1][:, inv]
    assert float((f1 - f2).abs().max()) < 1e-9 * float(f1.abs().max()) and float(f1.abs().max()) > 100.0


def test_dihedral_conditioning_is_below_the_noise_on_the_synthetic_chains_and_small_on_the_real_molecules():
    """The first-order cost of taking a dihedral through acos (amber_oracle.dihedral_conditioning): the synthetic helices
    need no allowance for it - eight ulps of cos phi stay below 64 x their relabelling noise; on the real molecules, with their
    planar groups, it is the larger part of the GPU tolerance, which still stays below 1e-11 of max |F|."""
    worst = {}
    for case in synthetic_cases():
        t, x, _ = synthetic(case)
        worst[case[1]] = max(worst.get(case[1], 0.0), float(ao.dihedral_conditioning(t, ao.as_kernel_reads(x)).max()))
    real = {name: float(ao.dihedral_conditioning(t, ao.as_kernel_reads(x)).max()) for name, (t, x) in real_cases().items()}
    print("dihedral conditioning bound (one ulp of cos phi, of max|F|):", {k: f"{v:.1e}" for k, v in worst.items()},
          "real molecules:", {k: f"{v:.1e}" for k, v in real.items()})
    for family, v in worst.items():   # (the lattice of cutoff_exact has flatter torsions: it gets no allowance either and must do without)
        assert family == "cutoff_exact" or 8.0 * v <= 64.0 * REFERENCE_NOISE_F[family], (family, v)
    assert 64.0 * REFERENCE_NOISE_F["real"] + 8.0 * max(real.values()) < 1e-11
    assert max(real.values()) > 64.0 * REFERENCE_NOISE_F["real"]        # (which is why the real family needs the allowance)
