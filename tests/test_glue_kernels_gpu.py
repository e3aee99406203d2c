"""The glue kernels of a Metropolis-Hastings iteration through the C ABI - `tw_centre`, `tw_kinetic_energy`, `tw_chirality_changed`
(csrc/tw_kernels.hip) and the stride edges of `tw_mh_accept` / `tw_mh_accept_chains` - against the float64 restatements of
tests/glue_oracle.py, fed the float32 inputs the kernels read.

Tolerances are derived, not measured, with u = 2^-24 (one float32 rounding):
  tw_centre           |com - com64| <= u sum_kept |x| per component: a float32 sum of n terms in any order carries at most (n - 1) u
                      sum |x|, the count is exact, and the division adds u |com| <= u sum |x| / n.  |xc - xc64| <= that + u |x - com|.
  tw_kinetic_energy   |out - ref| <= (n_atoms + 5) u ref: all terms are non-negative; three roundings in v^2, one for the mass,
                      n - 1 additions, one division.
  tw_chirality_changed  must EQUAL `changed()`: tests/test_glue_oracle_cpu.py asserts that every (row, centre) of the tables is more
                      than 16 u sum |six products| from zero (float32 is within 8 u of it), the exactly coplanar integer quads excepted,
                      whose product is exactly 0 in both precisions.
Outputs are prefilled with poison (NaN, 0xFF) and allocated a few elements longer than needed: what must be written is written,
nothing beyond it changes.  Every test prints its worst error / bound ratio.

Shapes: atoms 1 .. 691 either side of the 64-lane stride; rows 1 / 3 / 257; the chirality kernel's 128 rows per block at 127 / 128 /
129 / 257 rows."""
import numpy as np
import pytest
import torch

from tests import glue_oracle as go

pytestmark = pytest.mark.gpu

U = go.U
PAD = 5


def dev():
    return torch.device("cuda", 0)


def api():
    from timewarp_amd import _lib

    return _lib.load(), _lib.stream_ptr(dev())


def up(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev())


def poison(n, dtype=torch.float32):
    if dtype == torch.uint8:
        return torch.full((n + PAD,), 0xFF, dtype=torch.uint8, device=dev())
    return torch.full((n + PAD,), float("nan"), dtype=dtype, device=dev())


def untouched(buf, n):
    tail = buf[n:].cpu()
    return bool((tail == 0xFF).all()) if buf.dtype == torch.uint8 else bool(torch.isnan(tail).all())


def ptr(t):
    return None if t is None else t.data_ptr()


def worst(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.nanmax(r)) if r.size else 0.0


def same_bits(a, b):
    return bool((np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all())


# ---- tw_centre --------------------------------------------------------------------------------------------------------------------

def run_centre(x, m, want_xc=True, want_com=True):
    lib, s = api()
    n, V = x.shape[0], x.shape[1]
    xd, md = up(x), up(m)
    xc = poison(n * V * 3) if want_xc else None
    com = poison(n * 3) if want_com else None
    assert lib.tw_centre(ptr(xd), ptr(md), ptr(xc), ptr(com), n, V, s) == 0, lib.tw_last_error()
    torch.cuda.synchronize()
    assert (xc is None or untouched(xc, n * V * 3)) and (com is None or untouched(com, n * 3))
    return (None if xc is None else xc[: n * V * 3].cpu().numpy().reshape(n, V, 3),
            None if com is None else com[: n * 3].cpu().numpy().reshape(n, 3))


def check_centre(x, m, xc, com):
    com64, xc64, mag = go.centre(x, m)
    b_com = U * mag
    e_com = np.abs(com.astype(np.float64) - com64)
    assert (e_com <= b_com).all(), ("com", float(e_com.max()), np.argwhere(~(e_com <= b_com))[:4].tolist())
    b_xc = b_com[:, None, :] + U * np.abs(xc64)
    e_xc = np.abs(xc.astype(np.float64) - xc64)
    assert (e_xc <= b_xc).all(), ("xc", float(e_xc.max()), np.argwhere(~(e_xc <= b_xc))[:4].tolist())
    return max(worst(e_com, b_com), worst(e_xc, b_xc))


@pytest.mark.parametrize("n_rows", go.ROWS)
@pytest.mark.parametrize("n_atoms", go.ATOMS)
def test_centre_matches_the_restatement(n_atoms, n_rows):
    ratio = 0.0
    for offset in (0.0, 50.0):
        x = go.cloud(n_rows, n_atoms, offset, n_atoms + n_rows)
        for kind in go.MASKS:
            m = go.mask(kind, n_rows, n_atoms, n_atoms)
            if m is None:
                continue
            xc, com = run_centre(x, m)
            ratio = max(ratio, check_centre(x, m, xc, com))
            if kind == "third":         # each output NULL in turn: the other one is what it was
                only_xc, none = run_centre(x, m, want_com=False)
                none2, only_com = run_centre(x, m, want_xc=False)
                assert none is None and none2 is None and same_bits(only_xc, xc) and same_bits(only_com, com)
    print(f"tw_centre atoms {n_atoms} rows {n_rows}: worst error / bound {ratio:.3f}")


def test_centre_nan_and_all_masked_rows_stay_in_their_row():
    n, V = 5, 129
    x = go.cloud(n, V, 50.0, 9)
    m = go.mask("third", n, V, 9)
    clean_xc, clean_com = run_centre(x, m)
    bad, atom = 2, int(np.flatnonzero(m[2] == 0)[-1])        # a kept atom of the lanes' last pass
    y = x.copy()
    y[bad, atom, 1] = np.nan
    xc, com = run_centre(y, m)
    assert np.isnan(com[bad, 1]) and np.isnan(xc[bad, :, 1]).all()
    keep = np.arange(n) != bad
    assert same_bits(xc[keep], clean_xc[keep]) and same_bits(com[keep], clean_com[keep])
    assert same_bits(xc[bad][:, [0, 2]], clean_xc[bad][:, [0, 2]]) and same_bits(com[bad, [0, 2]], clean_com[bad, [0, 2]])
    # an all-masked row: what the restatement gives, 0 / 0
    mm = m.copy()
    mm[bad] = 1
    xc, com = run_centre(x, mm)
    com64, xc64, _ = go.centre(x, mm)
    assert np.isnan(com64[bad]).all() and np.isnan(com[bad]).all() and np.isnan(xc[bad]).all() and np.isnan(xc64[bad]).all()
    assert same_bits(xc[keep], clean_xc[keep]) and same_bits(com[keep], clean_com[keep])


# ---- tw_kinetic_energy ------------------------------------------------------------------------------------------------------------

def run_kinetic(v, masses, random_velocs, kbT):
    lib, s = api()
    n, V = v.shape[0], v.shape[1]
    vd, md = up(v), up(masses)
    out = poison(n)
    assert lib.tw_kinetic_energy(ptr(vd), ptr(md), int(random_velocs), kbT, ptr(out), n, V, s) == 0, lib.tw_last_error()
    torch.cuda.synchronize()
    assert untouched(out, n)
    return out[:n].cpu().numpy()


@pytest.mark.parametrize("n_rows", go.ROWS)
@pytest.mark.parametrize("n_atoms", go.ATOMS)
def test_kinetic_energy_matches_the_restatement(n_atoms, n_rows):
    v = go.velocities(n_rows, n_atoms, 3 * n_atoms)
    masses = go.masses_of(n_atoms, n_atoms)
    ratio = 0.0
    for random_velocs in (False, True):
        for kbT in (2.577, 0.5):
            got = run_kinetic(v, masses, random_velocs, kbT)
            ref, mag = go.kinetic_energy(v, masses, random_velocs, kbT)
            err, bound = np.abs(got.astype(np.float64) - ref), (n_atoms + 5) * U * mag
            assert (err <= bound).all(), (random_velocs, kbT, float((err / bound).max()))
            ratio = max(ratio, worst(err, bound))
    # masses = NULL is allowed only with random_velocs, and gives the same bits
    assert same_bits(run_kinetic(v, None, True, 0.0), run_kinetic(v, masses, True, 2.577))
    lib, s = api()
    out = poison(n_rows)
    assert lib.tw_kinetic_energy(ptr(up(v)), None, 0, 2.577, ptr(out), n_rows, n_atoms, s) == -1
    assert lib.tw_kinetic_energy(ptr(up(v)), ptr(up(masses)), 0, 0.0, ptr(out), n_rows, n_atoms, s) == -1 and b"kbT" in lib.tw_last_error()
    torch.cuda.synchronize()
    assert untouched(out, 0)
    print(f"tw_kinetic_energy atoms {n_atoms} rows {n_rows}: worst error / bound {ratio:.3f}")


def test_kinetic_energy_nan_stays_in_its_row():
    n, V = 5, 129
    v, masses = go.velocities(n, V, 4), go.masses_of(V, 4)
    for random_velocs in (False, True):
        clean = run_kinetic(v, masses, random_velocs, 2.577)
        w = v.copy()
        w[3, V - 1, 2] = np.nan
        got = run_kinetic(w, masses, random_velocs, 2.577)
        keep = np.arange(n) != 3
        assert np.isnan(got[3]) and same_bits(got[keep], clean[keep])


# ---- tw_chirality_changed ---------------------------------------------------------------------------------------------------------

def run_chirality(x, centres, ref, null_tables=False):
    lib, s = api()
    n, V = x.shape[0], x.shape[1]
    xd = up(x)
    cd = None if null_tables else up(np.asarray(centres, dtype=np.int32).reshape(-1, 4))
    rd = None if null_tables else up(np.asarray(ref, dtype=np.float32))
    n_centres = len(centres)
    if n_centres == 0 and not null_tables:      # (an empty tensor has no address either; a live one stands in)
        cd, rd = torch.zeros(4, dtype=torch.int32, device=dev()), torch.zeros(1, device=dev())
    out = poison(n, torch.uint8)
    assert lib.tw_chirality_changed(ptr(xd), ptr(cd), ptr(rd), n_centres, ptr(out), n, V, s) == 0, lib.tw_last_error()
    torch.cuda.synchronize()
    assert untouched(out, n)
    return out[:n].cpu().numpy()


@pytest.mark.parametrize("n_rows", go.CHIRALITY_ROWS)
@pytest.mark.parametrize("n_atoms", go.CHIRALITY_ATOMS)
def test_chirality_changed_equals_the_restatement(n_atoms, n_rows):
    seen = set()
    for n_centres in go.CHIRALITY_CENTRES:
        launches, centres, ref, singles = go.chirality_case(n_rows, n_atoms, n_centres)
        for x in launches:
            got = run_chirality(x, centres, ref)
            want = go.changed(x, centres, ref)
            assert set(np.unique(got).tolist()) <= {0, 1}
            assert (got.astype(bool) == want).all(), (n_centres, np.flatnonzero(got.astype(bool) != want)[:8].tolist())
            if n_centres:
                seen |= set(want.tolist())
            else:
                assert not got.any() and not run_chirality(x, centres, ref, null_tables=True).any()
        if n_centres and n_rows > 1:
            assert all(got[r] == 1 for r in singles.values())
    assert seen == {True, False}
    print(f"tw_chirality_changed atoms {n_atoms} rows {n_rows}: equal to the restatement (error / bound 0.000)")


def test_chirality_exactly_coplanar_quads():
    x, centres = go.coplanar_table()
    assert not run_chirality(x, centres, [0.0, 0.0]).any()
    for ref in ([1.0, 0.0], [0.0, -1.0], [1.0, -1.0], [-1.0, 1.0]):
        assert run_chirality(x, centres, ref).all(), ref


def test_chirality_rows_give_the_same_bytes_wherever_they_stand():
    (x,), centres, ref, _ = go.chirality_case(257, 65, 5)
    base = run_chirality(x, centres, ref)
    for shift in (1, 127, 131):
        assert (run_chirality(np.roll(x, shift, axis=0), centres, ref) == np.roll(base, shift)).all(), shift
    assert (run_chirality(x[100:140], centres, ref) == base[100:140]).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_glue_calls_refuse_bad_sizes_and_write_nothing():
    lib, s = api()
    x = up(go.cloud(4, 8, 0.0, 1))
    m = up(np.zeros((4, 8), dtype=np.uint8))
    masses = up(go.masses_of(8, 1))
    cen, ref = up(np.array([[0, 1, 2, 3]], dtype=np.int32)), up(np.array([1.0], dtype=np.float32))
    xc, com, ke, ch = poison(96), poison(12), poison(4), poison(4, torch.uint8)
    centre = lambda n, V: lib.tw_centre(ptr(x), ptr(m), ptr(xc), ptr(com), n, V, s)
    kinetic = lambda n, V: lib.tw_kinetic_energy(ptr(x), ptr(masses), 0, 2.577, ptr(ke), n, V, s)
    chir = lambda n, V, C=1: lib.tw_chirality_changed(ptr(x), ptr(cen), ptr(ref), C, ptr(ch), n, V, s)
    for call in (centre, kinetic, chir):
        assert call(-1, 8) == -1 and b"n_rows" in lib.tw_last_error(), lib.tw_last_error()
        assert call(4, 0) == -1 and b"n_atoms" in lib.tw_last_error(), lib.tw_last_error()
        assert call(4, -3) == -1 and b"n_atoms" in lib.tw_last_error()
        assert call(0, 8) == 0                                     # n_rows = 0 launches nothing
    assert chir(4, 8, -1) == -1 and b"n_centres" in lib.tw_last_error()
    torch.cuda.synchronize()
    assert untouched(xc, 0) and untouched(com, 0) and untouched(ke, 0) and untouched(ch, 0)
    assert centre(4, 8) == 0 and kinetic(4, 8) == 0 and chir(4, 8) == 0     # ... and the same arguments with good sizes are taken
    torch.cuda.synchronize()
    assert not torch.isnan(xc[:96]).any() and not torch.isnan(ke[:4]).any() and bool((ch[:4] <= 1).all())


def test_check_symmetry_change_refuses_a_centre_off_the_molecule():
    from timewarp_amd.utils.evaluation_utils import check_symmetry_change

    x = up(go.cloud(3, 22, 0.0, 2))
    ref = torch.ones(1, 1)
    for table in ([[8, 6, 9, 22]], [[-1, 6, 9, 14]], [[8, 6, 9]], [[8.0, 6.0, 9.0, 14.0]]):
        with pytest.raises(ValueError):
            check_symmetry_change(x, torch.tensor(table), ref)
    with pytest.raises(ValueError):
        check_symmetry_change(x, torch.tensor([[8, 6, 9, 14]]), torch.ones(1, 2))
    got = check_symmetry_change(x, torch.tensor([[8, 6, 9, 14], [0, 1, 2, 21]]), torch.tensor([[1.0, -1.0]]))
    assert (got.cpu().numpy() == go.changed(x.cpu().numpy(), [[8, 6, 9, 14], [0, 1, 2, 21]], [1.0, -1.0])).all()


# ---- tw_mh_accept / tw_mh_accept_chains: the 256-lane stride ------------------------------------------------------------------------

def run_accept(energy, u, n_chains, single_call):
    """energy, u [S, C] (p_xy = p_yx = 0).  Returns (exponent, p_acc, accepted [S, C], result [C, 4])."""
    lib, s = api()
    S, Cn = energy.shape
    e, ud, z = up(energy.astype(np.float32)), up(u.astype(np.float32)), torch.zeros(S * Cn, device=dev())
    ex, pa, acc = poison(S * Cn), poison(S * Cn), poison(S * Cn, torch.uint8)
    res = torch.full((Cn * 4 + PAD,), -7, dtype=torch.int32, device=dev())
    if single_call:
        rc = lib.tw_mh_accept(ptr(e), ptr(z), ptr(z), ptr(ud), None, None, None, None, ptr(ex), ptr(pa), ptr(acc), ptr(res), S, 0, s)
    else:
        rc = lib.tw_mh_accept_chains(ptr(e), ptr(z), ptr(z), ptr(ud), None, None, None, None, ptr(ex), ptr(pa), ptr(acc), ptr(res),
                                     S, Cn, 0, s)
    assert rc == 0, lib.tw_last_error()
    torch.cuda.synchronize()
    assert untouched(ex, S * Cn) and untouched(pa, S * Cn) and untouched(acc, S * Cn) and bool((res[Cn * 4:] == -7).all())
    sh = lambda t: t[: S * Cn].cpu().numpy().reshape(S, Cn)
    return sh(ex), sh(pa), sh(acc), res[: Cn * 4].cpu().numpy().reshape(Cn, 4)


@pytest.mark.parametrize("n_chains", [1, 3])
@pytest.mark.parametrize("S", [1, 255, 256, 257, 1000])
def test_accept_stride_edges(S, n_chains):
    rng = np.random.default_rng(S + n_chains)
    calls = [False] + ([True] if n_chains == 1 else [])
    for single_call in calls:
        # random rows against the float64 statement of the same test
        energy = (rng.normal(size=(S, n_chains)) * 3 + 4).astype(np.float32)
        u = rng.random((S, n_chains)).astype(np.float32)
        ex, pa, acc, res = run_accept(energy, u, n_chains, single_call)
        p64 = np.minimum(1.0, np.exp(-energy.astype(np.float64)))
        tol = 6 * U * p64              # the device library's expf is built to OpenCL's full-profile limit, 3 ulp = 6 u relative
        safe = np.abs(u - p64) > tol   # (a draw that close to p_acc is not looked at)
        assert same_bits(ex, energy) and (np.abs(pa - p64) <= tol).all()
        assert (acc.astype(bool) == (u < p64))[safe].all() and set(np.unique(acc).tolist()) <= {0, 1}
        for c in range(n_chains):
            idx = np.flatnonzero(acc[:, c])
            assert res[c].tolist() == ([int(idx[0]), 1, 0, 0] if len(idx) else [S - 1, 0, 0, 0])
        # nothing accepted; only the last row; rows 300 and 256 (the second pass of lane 0) -> first index 256
        patterns = [[], [S - 1], [0]] + ([[300, 256]] if S > 300 else []) + ([[256]] if S > 256 else [])
        for rows in patterns:
            energy = np.full((S, n_chains), 1e4, dtype=np.float32)
            energy[rows, n_chains - 1] = -1.0
            _, _, acc, res = run_accept(energy, np.full((S, n_chains), 0.5), n_chains, single_call)
            for c in range(n_chains):
                hit = rows if c == n_chains - 1 else []
                assert np.flatnonzero(acc[:, c]).tolist() == sorted(hit), (rows, c)
                assert res[c].tolist() == ([min(hit), 1, 0, 0] if hit else [S - 1, 0, 0, 0]), (rows, c)
        # exponent exactly 0: p_acc is exactly 1; u = 1 is rejected (strict <), the float below 1 accepted
        zero = np.zeros((S, n_chains), dtype=np.float32)
        ex, pa, acc, res = run_accept(zero, np.ones((S, n_chains)), n_chains, single_call)
        assert (pa == 1.0).all() and not acc.any() and (res[:, :2] == [S - 1, 0]).all()
        below = np.full((S, n_chains), np.nextafter(np.float32(1), np.float32(0)), dtype=np.float32)
        ex, pa, acc, res = run_accept(zero, below, n_chains, single_call)
        assert acc.all() and (res[:, :2] == [0, 1]).all()
