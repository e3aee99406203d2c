"""Pins tests/glue_oracle.py and proves the inputs of tests/test_glue_kernels_gpu.py and tests/test_mh_chirality_gpu.py, so that the GPU
files cannot pass by leaving things out: the restatements agree with what the project already pins (oracle/mh_oracle.py,
oracle/flow_oracle.py) to 1e-14 relative on the GPU file's shapes; every row of the chirality tables is away from a sign change by
the float32 margin and every case holds both outcomes; and through the CPU oracle the mirrored rows are accepted with the guard
off, carry the penalty and are rejected with it on, and decide which explorers move.  CPU only."""
import numpy as np
import pytest
import torch

from oracle import flow_oracle as fo
from oracle import mh_oracle as mo
from tests import glue_oracle as go

REL = 1e-14


def close(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = np.abs(b).max() if scale is None else scale
    return a.shape == b.shape and (a.size == 0 or float(np.abs(a - b).max()) <= REL * max(float(s), 1e-300))


# ---- restatements against what the project already pins ---------------------------------------------------------------------------

@pytest.mark.parametrize("n_atoms", go.ATOMS)
def test_centre_and_kinetic_restatements_agree_with_the_pinned_oracles(n_atoms):
    for n_rows in go.ROWS:
        for offset in (0.0, 50.0):
            x = go.cloud(n_rows, n_atoms, offset, n_atoms + n_rows).astype(np.float64)
            for kind in go.MASKS:
                m = go.mask(kind, n_rows, n_atoms, n_atoms)
                if m is None:
                    continue
                com, xc, mag = go.centre(x, m)
                ref = fo.centre_of_mass(torch.from_numpy(x), torch.from_numpy(m.astype(bool))).squeeze(1).numpy()
                assert close(com, ref, scale=np.abs(x).max()), (n_rows, offset, kind)
                assert close(xc, x - ref[:, None], scale=np.abs(x).max())
                assert (mag >= np.abs(com) - 1e-12).all()
        v = go.velocities(n_rows, n_atoms, 3 * n_atoms).astype(np.float64)
        masses = go.masses_of(n_atoms, n_atoms).astype(np.float64)
        for kbT in (2.577, 0.5):
            kbT32 = float(np.float32(kbT))
            got, _ = go.kinetic_energy(v, masses, False, kbT)
            assert close(got, mo.compute_kinetic_energy(torch.from_numpy(v), torch.from_numpy(masses), False, kbT32).numpy())
        got, mag = go.kinetic_energy(v, None, True, 0.0)
        assert close(got, mo.compute_kinetic_energy(torch.from_numpy(v), None, True).numpy()) and (mag == got).all()


def test_centre_of_an_all_masked_row_is_nan():
    x = go.cloud(3, 5, 0.0, 1)
    m = np.zeros((3, 5), dtype=np.uint8)
    m[1] = 1
    com, xc, _ = go.centre(x, m)
    assert np.isnan(com[1]).all() and np.isnan(xc[1]).all() and np.isfinite(com[[0, 2]]).all()


@pytest.mark.parametrize("n_atoms", go.CHIRALITY_ATOMS)
def test_chirality_tables_are_off_the_margin_and_hold_both_outcomes(n_atoms):
    for n_rows in go.CHIRALITY_ROWS:
        for n_centres in go.CHIRALITY_CENTRES:
            launches, centres, ref, singles = go.chirality_case(n_rows, n_atoms, n_centres)
            assert centres.shape == (n_centres, 4) and all(x.shape == (n_rows, n_atoms, 3) and x.dtype == np.float32 for x in launches)
            if n_centres == 0:
                assert not any(go.changed(x, centres, ref).any() for x in launches)
                continue
            assert n_centres < 2 or centres.max() == n_atoms - 1          # a centre reads the first atom, one the last
            assert (centres[0] == 0).any() and (n_centres < 2 or (centres[1] == n_atoms - 1).any())
            assert n_centres < 2 or set(ref.tolist()) == {1.0, -1.0}       # reference signs mixed
            outcomes = []
            for x in launches:
                t, mag = go.chirality(x, centres)
                assert (np.abs(t) > go.SIGN_MARGIN * mag).all(), (n_rows, n_centres, float((np.abs(t) / mag).min()))
                # ... against the pinned restatement, on float64 inputs
                x64 = torch.from_numpy(x.astype(np.float64))
                c64 = torch.from_numpy(centres.astype(np.int64))
                assert (np.sign(t) == mo.compute_chirality_sign(x64, c64).numpy()).all()
                rows = np.stack([x.astype(np.float64)[:, centres[:, k]] - x.astype(np.float64)[:, centres[:, 0]] for k in (1, 2, 3)], axis=-2)
                assert close(t, np.linalg.det(rows), scale=float(mag.max()))
                ch = go.changed(x, centres, ref)
                assert (ch == mo.check_symmetry_change(x64, c64, torch.from_numpy(ref)).numpy()).all()
                outcomes.append(ch)
            ch = np.concatenate(outcomes)
            assert ch.any() and not ch.all(), (n_rows, n_centres)
            if n_atoms >= 22:           # "any", not "first" or "last": exactly centre c differs in the row made for it
                for c, r in singles.items():
                    differs = np.sign(go.chirality(launches[0][r:r + 1], centres)[0][0]) != ref
                    assert differs.tolist() == [k == c for k in range(n_centres)]


def test_coplanar_quads_are_exactly_zero():
    x, centres = go.coplanar_table()
    t, mag = go.chirality(x, centres)
    assert (t == 0.0).all() and (mag > 0).any()
    a, b, d = (x[:, centres[:, k]] - x[:, centres[:, 0]] for k in (1, 2, 3))        # float32 arithmetic: the same exact zero
    t32 = (a * np.cross(b, d)).sum(axis=-1)
    assert t32.dtype == np.float32 and (t32 == 0.0).all() and float(np.abs(x).max()) < 64
    assert not go.changed(x, centres, [0.0, 0.0]).any()
    for ref in ([1.0, 0.0], [0.0, -1.0], [1.0, -1.0]):
        assert go.changed(x, centres, ref).all()


# ---- the mirrored-row construction through the CPU oracle --------------------------------------------------------------------------

def test_mirrored_rows_protocol():
    _, coords, _, _, _ = go.alanine()
    a, b = go.chain_noise(), go.chain_noise()
    plain = go.MirroredRows(go.NOISE_SEED, coords, ())
    sc, sv = torch.tensor(np.exp(-2.0)), torch.tensor(1.0)
    zc, zv = a.latents(8, 1, 22, sc, sv)
    pc, pv = plain.latents(8, 1, 22, sc, sv)
    assert torch.equal(zc, b.latents(8, 1, 22, sc, sv)[0]) and torch.equal(zv, pv)
    rows = list(go.MIRRORED)
    others = [r for r in range(8) if r not in rows]
    assert torch.equal(zc[others], pc[others]) and float(pc.abs().max()) < 6 * go.ORDINARY_SCALE
    m = (coords + (zc[rows, 0] - pc[rows, 0]))                                       # x + (m - x)
    assert torch.allclose(m[..., 0] + coords[:, 0], 2 * coords[:, 0].mean().expand(2, 22), atol=1e-6)
    assert torch.equal(m[..., 1:], coords[:, 1:].expand(2, 22, 2))
    assert a.uniform(8).tolist() == [1, 1, 0, 1, 1, 0, 1, 1] and go.chain_noise(accept=False).uniform(8).tolist() == [1.0] * 8
    once = go.MirroredRows(go.NOISE_SEED, coords, rows, first_call_only=True)
    first, second = once.latents(1, 8, 22, sc, sv)[0], once.latents(1, 8, 22, sc, sv)[0]
    assert float(first.abs().max()) > 0.01 > float(second.abs().max())


def test_state_geometry_is_far_from_a_sign_change():
    _, coords, _, _, _ = go.alanine()
    t, mag = go.chirality(coords[None].numpy(), go.CENTRES_TWO)
    assert t[0, 0] > 1e-3 and t[0, 1] < -1e-3 and (np.abs(t) > 1e4 * go.SIGN_MARGIN * mag).all()


@pytest.mark.parametrize("random_velocs", [True, False])
def test_guard_decides_the_chain_in_the_oracle(random_velocs):
    S, (r0, r1) = go.S_PROPOSALS, go.MIRRORED
    _, _, acc_a, st_a = go.oracle_chain(random_velocs, "off", True, r0 + 1)
    _, _, acc_b, st_b = go.oracle_chain(random_velocs, "off", False, S)
    _, _, acc_c, st_c = go.oracle_chain(random_velocs, "one", True, S)
    ordinary = [r for r in range(S) if r not in go.MIRRORED]
    # guard off: the first mirrored row is accepted, its exponent is small, its energy is an ordinary row's
    assert acc_a == 1 and st_a.acceptance_indicator.tolist() == [False] * r0 + [True]
    assert st_a.exponent[r0] < 20 and st_b.exponent[r0] < 20 and st_b.exponent[r1] < 20
    dpot = st_b.energies_pot_delta
    assert dpot[ordinary].min() <= dpot[r0] <= dpot[ordinary].max(), dpot            # within the spread of the ordinary rows
    assert acc_b == 0 and len(st_b.exponent) == S
    # guard on: 2000 on the mirrored rows and on nothing else, nothing accepted
    assert acc_c == 0 and len(st_c.exponent) == S and not st_c.acceptance_indicator.any()
    for r in go.MIRRORED:
        assert abs(float(st_c.energies_pot[r]) - float(st_b.energies_pot[r]) - 2000.0) <= 2.0 ** -13     # float32 spacing below 2048
        assert st_c.exponent[r] > 1900 and st_c.acceptance[r] == 0.0
    for f in ("p_xy", "p_yx", "exponent", "energies_pot", "energies_kin", "energies_pot_delta", "energies_kin_delta", "acceptance"):
        assert np.array_equal(getattr(st_c, f)[ordinary], getattr(st_b, f)[ordinary]), f
        assert np.array_equal(getattr(st_c, f)[:r0], getattr(st_a, f)[:r0]), f          # ... up to the accepted index
    print("exponents off", st_b.exponent[[r0, r1]], "on", st_c.exponent[[r0, r1]], "dpot", dpot)


@pytest.mark.parametrize("guard", ["two", "two_swapped"])
def test_each_table_entry_has_its_own_reference_sign_in_the_oracle(guard):
    S = go.S_PROPOSALS
    _, _, acc, st = go.oracle_chain(False, guard, True, S)
    _, _, _, off = go.oracle_chain(False, "off", False, S)
    assert acc == 0 and not st.acceptance_indicator.any()
    assert (np.abs(st.energies_pot - off.energies_pot - 2000.0) <= 2.0 ** -13).all() and (st.exponent > 1900).all()


def test_guard_decides_which_explorers_move_in_the_oracle():
    e = go.EXPLORE
    P = e["P"]
    _, coords, _, _, _ = go.alanine()
    pos, en = go.oracle_explore(True)
    free, _ = go.oracle_explore(False)
    moved = (pos[:P] != coords[None]).any(-1).any(-1)
    assert moved.tolist() == [r not in go.MIRRORED for r in range(P)]
    assert torch.equal(pos[list(go.MIRRORED)], coords[None].expand(2, 22, 3))
    assert (free[:P] != coords[None]).any(-1).any(-1).all()
    mirrored = free[list(go.MIRRORED)]                    # without centres the explorers become the mirror image
    assert float((mirrored[..., 0] + coords[:, 0] - 2 * coords[:, 0].mean()).abs().max()) < 0.02
    assert pos.shape == (e["steps"] * P, 22, 3) and en.shape == (e["steps"] * P, 1)
