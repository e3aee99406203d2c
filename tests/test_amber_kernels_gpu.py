"""The AMBER energy kernel (csrc/tw_energy.hip, `energy_and_terms`) and force kernel (csrc/tw_md.hip, `energy_and_forces`) held to
the float64 autograd reference of tests/amber_oracle.py: the energy kernel's total and its five terms, the force kernel's energy,
all N x V x 3 force components, the equality of the two kernels' energies, net force and net torque.

Cases (built by amber_oracle.synthetic_case, checked on the CPU by tests/test_amber_oracle_cpu.py): chains of
V = 1, 2, 3, 4, 22, 63 .. 66, 127 .. 129, 192, 193 atoms - no pair, one pair, no torsion; the dispatch between the one- / four-wave
and the sixteen-wave kernels; the 64-lane stride ending exactly, one over, and after three and four rounds - in the three GBSA
modes with cutoff 2.0, 0.6 (most pairs outside) and 0 (none); four kinds that take the Born-integral branches covalent geometry
never does (`buried`, `skipped`, `constant_l`) or sit exactly on the cutoff (`cutoff_exact`); 1 and 257 rows; the largest
molecule the 160 KiB of LDS admit; and the real molecules of test_energy_kat.py.  Five conformations each, one stretched 2.5 times.

Energy tolerance: the project's own between kernel and C oracle (rtol 1e-10 / atol 1e-8; terms rtol 1e-9 / atol 1e-8).
Force tolerance: FORCE_MARGIN x REFERENCE_NOISE_F[family] of max |F_ref| of the conformation - the reference's own relabelling
noise, measured on the CPU, times 64: the kernels sum an atom's V partners in another order than the reference, go through LDS
atomics and use device tanh / log / exp / acos that differ from libm in the last bit.  A ceiling on that, not a fit.  Every
synthetic family meets it.

The real molecules need more, and the reason is shown on the reference (amber_oracle.dihedral_conditioning): the kernels take the
dihedral as acos(cos phi), as OpenMM's algorithm does, and the arc cosine has condition number 1 / |sin phi|.  Peptides are full of
planar groups (omega, the impropers; |sin phi| down to 1e-3), where the rounding of cos phi - DIHEDRAL_ULPS = 8 ulps: the three
products and two sums of each of two cross products and three dot products, a root and a quotient, none cancelling badly at these
angles - reaches the forces two to three digits above the sum-order noise.  The `real` family's tolerance therefore adds
DIHEDRAL_ULPS x that first-order bound, computed per conformation on the reference alone; the measured kernel error stays below ONE
times the bound on every conformation (worst: 3.4e-13 of max |F| where the bound is 1.1e-12), and the tolerance stays below 1e-11
of max |F|.  The synthetic helices (|sin phi| ~ 1) have a bound below the noise; no synthetic family gets an allowance.

MEASURED_KERNEL_ERROR below: the worst max |F - F_ref| / max |F_ref| per family on an MI355X, printed by every test."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import amber_oracle as ao
from tests import test_amber_oracle_cpu as cpu
from tests.test_amber_oracle_cpu import REFERENCE_NOISE_F

pytestmark = pytest.mark.gpu

FORCE_MARGIN = 64.0
DIHEDRAL_ULPS = 8.0
ENERGY_TOL, TERMS_TOL = cpu.ENERGY_TOL, cpu.TERMS_TOL
KERNELS_AGREE = dict(rtol=1e-12, atol=1e-9)      # the two kernels' energies (test_md_gpu.py)
LDS_LIMIT = 160 * 1024

# kernel vs reference, worst max |F - F_ref| / max |F_ref| over the family's conformations, MI355X;
# FORCE_MARGIN x REFERENCE_NOISE_F is 2.8e-14, 1.1e-13, 2.3e-13, 1.1e-13, 5.7e-14 for the synthetic families in this order:
MEASURED_KERNEL_ERROR = {"covalent": 4.19e-15, "buried": 1.49e-15, "skipped": 2.11e-15, "constant_l": 2.07e-15, "cutoff_exact": 9.53e-15,
                         "real": 3.44e-13}   # real: a three-residue segment; 1.2e-13 on the 691-atom protein, 1.7e-14 on NNQQ


@functools.lru_cache(maxsize=None)
def force_tolerance(key, family):
    """[N] relative to max |F_ref| of each conformation"""
    tol = np.full(len(cpu.reference(key)[0]), FORCE_MARGIN * REFERENCE_NOISE_F[family])
    if family == "real":
        t, x = cpu.real_cases()[key]
        tol = tol + DIHEDRAL_ULPS * ao.dihedral_conditioning(t, ao.as_kernel_reads(x)).numpy()
    return tol


@functools.lru_cache(maxsize=None)
def potential(key):
    from timewarp_amd.energy import AmberPotentialEnergyTorch

    return AmberPotentialEnergyTorch(cpu.synthetic(key)[0] if isinstance(key, tuple) else cpu.real_cases()[key][0])


def compare(key, family, rows=None):
    """Both kernels on the case's conformations (tiled to `rows` rows when given) against the shared reference; returns the
    worst force error relative to max |F_ref| of its conformation."""
    x = cpu.synthetic(key)[1] if isinstance(key, tuple) else cpu.real_cases()[key][1]
    e_ref, terms_ref, f_ref = cpu.reference(key)
    tol = force_tolerance(key, family)
    if rows is not None:
        pick = np.arange(rows) % len(x)
        x, e_ref, terms_ref, f_ref, tol = x[pick], e_ref[pick], terms_ref[pick], f_ref[pick], tol[pick]
    xg = torch.from_numpy(np.array(x)).cuda()
    e_k, terms_k = potential(key).energy_and_terms(xg, want_terms=True)
    e_f, f_k = potential(key).energy_and_forces(xg)
    e_k, terms_k, e_f, f_k = (a.cpu().numpy() for a in (e_k, terms_k, e_f, f_k))
    assert np.isfinite(f_k).all() and f_k.shape == f_ref.shape
    assert np.allclose(e_k, e_ref, **ENERGY_TOL), (key, "energy kernel", np.abs(e_k - e_ref).max())
    assert np.allclose(terms_k, terms_ref, **TERMS_TOL), (key, "terms", np.abs(terms_k - terms_ref).max(0))
    assert np.allclose(e_f, e_ref, **ENERGY_TOL), (key, "force kernel's energy", np.abs(e_f - e_ref).max())
    assert np.allclose(e_f, e_k, **KERNELS_AGREE), (key, "the two kernels' energies", np.abs(e_f - e_k).max())
    V = f_ref.shape[1]
    scale = np.abs(f_ref).max((1, 2))
    if V == 1:
        assert not f_k.any() and not f_ref.any()
        return 0.0
    err = np.abs(f_k - f_ref).max((1, 2)) / scale
    # net force and net torque (about the centroid): those of the reference are rounding noise, and so must the kernel's be - a sum of
    # V components, each within the tolerance
    xd = np.asarray(x, dtype=np.float64)
    arm = xd - xd.mean(1, keepdims=True)
    net = np.abs(f_k.sum(1) - f_ref.sum(1)).max(1)
    torque = np.abs(np.cross(arm, f_k).sum(1) - np.cross(arm, f_ref).sum(1)).max(1)
    assert (np.abs(f_ref.sum(1)).max(1) <= V * tol * scale).all(), (key, "net force of the reference")
    assert (net <= V * tol * scale).all(), (key, "net force", (net / scale).max())
    assert (torque <= 2.0 * V * tol * scale * np.abs(arm).max((1, 2))).all(), (key, "net torque", torque.max())
    assert (err <= tol).all(), (key, "forces, of max|F|", err, "tolerance", tol)
    return float(err.max())


def report(family, what, worst):
    print(f"{family}, {what}: kernel vs float64 autograd reference, worst max|F - F_ref| / max|F_ref| = {worst:.2e} "
          f"(tolerance {FORCE_MARGIN * REFERENCE_NOISE_F[family]:.2e} = {FORCE_MARGIN:.0f} x the reference's relabelling noise)")


@pytest.mark.parametrize("V", cpu.COVALENT_V)
def test_covalent_chains_across_the_launch_shapes(V):
    """three GBSA modes x cutoff 2.0 / 0.6 / 0, five conformations each"""
    worst = max(compare(case, "covalent") for case in cpu.synthetic_cases("covalent") if case[0] == V)
    report("covalent", f"V = {V}", worst)


@pytest.mark.parametrize("V", cpu.SPECIAL_V)
@pytest.mark.parametrize("kind", cpu.SPECIAL_KINDS)
def test_born_branches_and_the_exact_cutoff(kind, V):
    """`buried`: off_i < s_j - r with its extra 2 (1 / off_i - l) term; `skipped`: !(off_i < r + s_j); `constant_l`: l = 1 / off_i;
    `cutoff_exact`: pairs at r == rc (nonbonded drops them, GB keeps them) and one float32 to either side - with both OBC modes"""
    worst = max(compare(case, kind) for case in cpu.synthetic_cases(kind) if case[0] == V)
    report(kind, f"V = {V}", worst)


@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("case", [(65, "buried", 1, 2.0), (64, "covalent", 2, 0.6)], ids=str)
def test_row_counts(case, rows):
    report(case[1], f"{case}, {rows} rows", compare(case, case[1], rows=rows))


REAL = ["NNQQ", "protein frame 5"] + [f"alanine dipeptide gb={gb}" for gb in (1, 2, 0)] + [f"ten residues #{n}" for n in range(5)]


@pytest.mark.parametrize("name", REAL + ["three residues"])
def test_real_molecules_all_components(name):
    """NNQQ frames 0 / 7 / 19 / 39, frame 5 of the 691-atom protein, alanine dipeptide, the ten- and three-residue segments of
    test_energy_kat.py: every component against the reference (the OpenMM comparisons of test_energy_kat.py stay as they are)"""
    names = [k for k in cpu.real_cases() if k.startswith(name)]
    assert names and (name != "three residues" or len(names) >= 10)
    report("real", name, max(compare(k, "real") for k in names))


# ---- the LDS ceiling -------------------------------------------------------------------------
def excl_bytes(V):
    return (V * V + 31) // 32 * 4          # one bit per ordered pair, whole 32-bit words


def force_lds_bytes(V):
    """md_lds_bytes(V, with_v = false) of tw_md.hip: x, F [3V] each, born, dEdB, chain [V] each, 16 wave sums, the exclusion bits"""
    return ((9 * V + 16) * 8 + excl_bytes(V) + 15) // 16 * 16


def energy_lds_bytes(V):
    """`shm` of amber_energy (tw_energy.hip) above 64 atoms: x [3V], born [V], 5 sums of 16 waves, the exclusion bits"""
    assert V > 64
    return ((4 * V + 5 * 16) * 8 + excl_bytes(V) + 15) // 16 * 16


def largest_admitted(lds_bytes):
    V = 65
    while lds_bytes(V + 1) <= LDS_LIMIT:
        V += 1
    return V


@functools.lru_cache(maxsize=None)
def ceiling_case(V):
    t, x, _ = ao.synthetic_case(V, "covalent", 1, 2.0, conformations=(0, 4))   # two conformations: one jittered, the stretched one
    return t, x


def test_the_largest_molecule_the_lds_admits():
    """V = 892 for the force kernel and 1021 for the energy kernel (derived from the kernels' own LDS carve, restated above) run and
    agree with the reference; one atom more raises the library's error and launches nothing."""
    from timewarp_amd import _lib
    from timewarp_amd.energy import AmberPotentialEnergyTorch

    v_force, v_energy = largest_admitted(force_lds_bytes), largest_admitted(energy_lds_bytes)
    print(f"largest V under {LDS_LIMIT} bytes of LDS: force kernel {v_force} ({force_lds_bytes(v_force)} bytes), "
          f"energy kernel {v_energy} ({energy_lds_bytes(v_energy)} bytes)")
    assert force_lds_bytes(v_force) <= LDS_LIMIT < force_lds_bytes(v_force + 1)
    assert energy_lds_bytes(v_energy) <= LDS_LIMIT < energy_lds_bytes(v_energy + 1)
    assert 691 < v_force < v_energy
    tol = FORCE_MARGIN * REFERENCE_NOISE_F["covalent"]
    # forces (and both energies) at the force kernel's ceiling
    t, x = ceiling_case(v_force)
    xd = ao.as_kernel_reads(x)
    assert float(ao.switch_margins(t, xd)["min_margin"].min()) > ao.MARGIN
    e_ref, f_ref = (a.numpy() for a in ao.energy_and_forces(t, xd))
    terms_ref = ao.energy_terms(t, xd).numpy()
    p = AmberPotentialEnergyTorch(t)
    xg = torch.from_numpy(x).cuda()
    e_f, f_k = (a.cpu().numpy() for a in p.energy_and_forces(xg))
    e_k, terms_k = (a.cpu().numpy() for a in p.energy_and_terms(xg, want_terms=True))
    assert np.allclose(e_f, e_ref, **ENERGY_TOL) and np.allclose(e_k, e_ref, **ENERGY_TOL) and np.allclose(terms_k, terms_ref, **TERMS_TOL)
    assert np.allclose(e_f, e_k, **KERNELS_AGREE)
    err = np.abs(f_k - f_ref).max((1, 2)) / np.abs(f_ref).max((1, 2))
    report("covalent", f"V = {v_force}, the force kernel's LDS ceiling", float(err.max()))
    assert (err <= tol).all(), err
    # the energy kernel at its own ceiling
    t, x = ceiling_case(v_energy)
    xd = ao.as_kernel_reads(x)
    assert float(ao.switch_margins(t, xd)["min_margin"].min()) > ao.MARGIN
    terms_ref = ao.energy_terms(t, xd).numpy()
    p = AmberPotentialEnergyTorch(t)
    e_k, terms_k = (a.cpu().numpy() for a in p.energy_and_terms(torch.from_numpy(x).cuda(), want_terms=True))
    assert np.allclose(e_k, terms_ref.sum(1), **ENERGY_TOL) and np.allclose(terms_k, terms_ref, **TERMS_TOL)
    # one atom more: refused before any launch - the outputs keep their sentinel
    lib = _lib.load()
    for V, call, what in ((v_force + 1, "tw_amber_energy_forces", "force kernel"), (v_energy + 1, "tw_amber_energy", "energy kernel")):
        t = ao.synthetic_tables(V, "covalent", 1, 2.0)
        xg = torch.zeros(2, V, 3, device="cuda")         # (never read)
        ff = t.to_device(xg.device)
        e = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
        f = torch.full((2, V, 3), -7.0, dtype=torch.float64, device="cuda")
        second = f.data_ptr() if call == "tw_amber_energy_forces" else None
        with pytest.raises(RuntimeError, match=rf"{what}: {V} atoms need \d+ bytes of LDS"):
            _lib.check(getattr(lib, call)(C.byref(ff.struct), xg.data_ptr(), e.data_ptr(), second, 2, _lib.stream_ptr(xg.device)), call)
        torch.cuda.synchronize()
        assert bool((e == -7.0).all()) and bool((f == -7.0).all())
        with pytest.raises(RuntimeError, match="bytes of LDS"):
            (AmberPotentialEnergyTorch(t).energy_and_forces if second else AmberPotentialEnergyTorch(t).energy_and_terms)(xg)
