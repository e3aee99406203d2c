"""csrc/tw_evaluate.hip through the C ABI (`tw_pair_distances`, `tw_column_range`, `tw_column_histogram`, `tw_pair_range`,
`tw_pair_histogram`) and the drivers of timewarp_amd/evaluate.py on the device, against the numpy restatement
tests/evaluate_oracle.py: counts, outside counters, lo and hi EQUAL it; distances within one float32 ulp of the long-double truth
(the fp64 steps contribute about 2^-52 relative, the one rounding to float32 half an ulp).

Shapes sit on each side of every boundary the kernels have: rows 1, 63, 64, 65 (a wave), 777 (ragged, several row blocks) and 5000
(several workgroups merge into one column); columns 1, 2 and TILE - 1 / TILE / TILE + 1 for the bin count in use
(`tw_histogram_column_tile`: 159 at 100 bins, 3 at 4096); col_stride 1 and 3 with a row pitch larger than needed and NaN in every
element the call must not read.  Every raw call runs on over-allocated outputs with guard bands that must come back untouched."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import evaluate_oracle as eo
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

GUARD = 64
POISON_I = -7777777777
POISON_F = -7.25e30
LO, HI = -1.25, 3.5


def dev():
    return torch.device("cuda", 0)


def lib():
    from timewarp_amd import _lib

    return _lib.load()


def stream():
    from timewarp_amd import _lib

    return _lib.stream_ptr(dev())


def tile(bins):
    return int(lib().tw_histogram_column_tile(bins))


def guarded(n, dtype, poison, fill=None):
    t = torch.full((n + 2 * GUARD,), poison, dtype=dtype, device=dev())
    if fill is not None:
        t[GUARD:GUARD + n] = torch.as_tensor(fill, dtype=dtype).reshape(-1).to(dev())
    return t


def clean(t, n, poison):
    return bool((t[:GUARD] == poison).all()) and bool((t[GUARD + n:] == poison).all())


def body(t, n):
    return t[GUARD:GUARD + n].cpu().numpy()


def strided(values, ld=None, col_stride=1):
    """values [T, C] float32 -> (device buffer, ld): column c of row r at r ld + c col_stride, NaN everywhere else."""
    T, C = values.shape
    need = (C - 1) * col_stride + 1 if C else 1
    ld = need if ld is None else ld
    buf = torch.full((max(T, 1), ld), float("nan"), dtype=torch.float32, device=dev())
    if T and C:
        buf[:T, 0:need:col_stride] = torch.as_tensor(values).to(dev())
    return buf, ld


def raw_range(buf, T, C, ld, cs, x_ptr=True):
    lo = guarded(C, torch.float32, POISON_F)
    hi = guarded(C, torch.float32, POISON_F)
    nf = guarded(C, torch.int64, POISON_I)
    st = lib().tw_column_range(buf.data_ptr() if x_ptr else None, T, C, ld, cs, lo[GUARD:].data_ptr(), hi[GUARD:].data_ptr(),
                               nf[GUARD:].data_ptr(), stream())
    torch.cuda.synchronize()
    ok = clean(lo, max(C, 0), POISON_F) and clean(hi, max(C, 0), POISON_F) and clean(nf, max(C, 0), POISON_I)
    return st, body(lo, max(C, 0)), body(hi, max(C, 0)), body(nf, max(C, 0)), ok


def raw_hist(buf, T, C, ld, cs, edges, bins, prefill=None, outside_prefill=None):
    """One tw_column_histogram call.  Returns (status, counts [C, bins], outside [C, 3], clean)."""
    n = max(C, 0) * max(bins, 0)
    counts = guarded(n, torch.int64, POISON_I, fill=np.zeros(n, dtype=np.int64) if prefill is None else prefill)
    outside = guarded(3 * max(C, 0), torch.int64, POISON_I,
                      fill=np.zeros(3 * max(C, 0), dtype=np.int64) if outside_prefill is None else outside_prefill)
    e = None if edges is None else torch.as_tensor(edges, dtype=torch.float64).contiguous().to(dev())
    st = lib().tw_column_histogram(buf.data_ptr(), T, C, ld, cs, None if e is None else e.data_ptr(), bins, counts[GUARD:].data_ptr(),
                                   outside[GUARD:].data_ptr(), stream())
    torch.cuda.synchronize()
    ok = clean(counts, n, POISON_I) and clean(outside, 3 * max(C, 0), POISON_I)
    return st, body(counts, n).reshape(max(C, 0), max(bins, 0)), body(outside, 3 * max(C, 0)).reshape(-1, 3), ok


def raw_pairs(coords, pairs, edges=None, bins=0, what="distances"):
    """tw_pair_distances / tw_pair_range / tw_pair_histogram on coords [T, V, 3], pairs [P, 2] (numpy)."""
    x = torch.as_tensor(np.ascontiguousarray(coords, dtype=np.float32)).to(dev())
    p = torch.as_tensor(np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)).to(dev())
    T, V, P = x.shape[0], x.shape[1], p.shape[0]
    xp, pp = (x.data_ptr() if T else None), (p.data_ptr() if P else None)
    if what == "distances":
        out = guarded(T * P, torch.float32, POISON_F)
        st = lib().tw_pair_distances(xp, pp, P, out[GUARD:].data_ptr(), T, V, stream())
        torch.cuda.synchronize()
        return st, body(out, T * P).reshape(T, P), clean(out, T * P, POISON_F)
    if what == "range":
        lo, hi, nf = guarded(P, torch.float32, POISON_F), guarded(P, torch.float32, POISON_F), guarded(P, torch.int64, POISON_I)
        st = lib().tw_pair_range(xp, pp, P, T, V, lo[GUARD:].data_ptr(), hi[GUARD:].data_ptr(), nf[GUARD:].data_ptr(), stream())
        torch.cuda.synchronize()
        return st, body(lo, P), body(hi, P), body(nf, P), clean(lo, P, POISON_F) and clean(hi, P, POISON_F) and clean(nf, P, POISON_I)
    counts = guarded(P * bins, torch.int64, POISON_I, fill=np.zeros(P * bins, dtype=np.int64))
    outside = guarded(3 * P, torch.int64, POISON_I, fill=np.zeros(3 * P, dtype=np.int64))
    e = torch.as_tensor(edges, dtype=torch.float64).contiguous().to(dev())
    st = lib().tw_pair_histogram(xp, pp, P, T, V, e.data_ptr(), bins, counts[GUARD:].data_ptr(), outside[GUARD:].data_ptr(), stream())
    torch.cuda.synchronize()
    return st, body(counts, P * bins).reshape(P, bins), body(outside, 3 * P).reshape(P, 3), clean(counts, P * bins, POISON_I) and \
        clean(outside, 3 * P, POISON_I)


def dyadic(bins):
    """A range whose np.linspace edges are float32 numbers (-0.5 + k / 64): the planted values sit EXACTLY on them, and their
    float32 neighbours directly on either side.  On (LO, HI) the edges are not float32 numbers and the planted values straddle them."""
    return -0.5, -0.5 + bins / 64.0


def values(T, C, bins, seed, special=True, lo=LO, hi=HI):
    """[T, C] float32: per column the planted-edge set of (lo, hi, bins) as far as T allows, then uniform draws that reach outside;
    with `special`, a NaN and both infinities where there is room."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), size=(T, C)).astype(np.float32)
    for c in range(C):
        planted = eo.planted_values(lo, hi, bins, rng, n_random=0)
        k = min(T, len(planted))
        X[:k, c] = planted[:k]
    if special and T >= 8:
        for c in range(C):
            r = rng.choice(T, size=3, replace=False)
            X[r[0], c], X[r[1], c], X[r[2], c] = np.nan, np.inf, -np.inf
    return X


def check_against_numpy(X, bins, cs=1, pad=0, lo=LO, hi=HI):
    """Range and histogram of X through the C ABI against the restatement; returns the kernel's counts."""
    T, C = X.shape
    buf, ld = strided(X, ld=(C - 1) * cs + 1 + pad, col_stride=cs)
    st, klo, khi, knf, ok = raw_range(buf, T, C, ld, cs)
    assert st == 0 and ok
    rlo, rhi, rnf = eo.column_ranges(X)
    assert (klo == rlo).all() and (khi == rhi).all() and (knf == rnf).all()
    edges = np.stack([np.linspace(lo, hi, bins + 1)] * C)
    st, counts, outside, ok = raw_hist(buf, T, C, ld, cs, edges, bins)
    assert st == 0 and ok
    rc, re_, below, above, nan = eo.histogram_columns(X, bins, lo, hi)
    assert (re_ == edges).all()
    assert (counts == rc).all()
    assert (outside[:, 0] == below).all() and (outside[:, 1] == above).all() and (outside[:, 2] == nan).all()
    assert (counts.sum(axis=1) + outside.sum(axis=1) == T).all()
    return counts


# ---- columns ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 63, 64, 65, 777, 5000])
@pytest.mark.parametrize("C", [1, 2])
def test_rows_on_each_side_of_a_wave_and_of_a_row_block(T, C):
    check_against_numpy(values(T, C, 100, seed=T + C), 100)
    check_against_numpy(values(T, C, 100, seed=T + C + 1), 100, cs=3, pad=5)
    check_against_numpy(values(T, C, 100, seed=T + C + 2), 100, cs=1, pad=3)      # adjacent columns, a row pitch larger than the row


@pytest.mark.parametrize("bins", [100, 4096])
@pytest.mark.parametrize("where", [-1, 0, 1])
@pytest.mark.parametrize("cs,pad", [(1, 0), (1, 5), (3, 7)])
def test_columns_on_each_side_of_the_tile(bins, where, cs, pad):
    C = tile(bins) + where
    assert tile(bins) == min(512, 65536 // (4 * (bins + 3)))
    check_against_numpy(values(777 if bins == 100 else 5000, C, bins, seed=bins + where + cs), bins, cs=cs, pad=pad)


@pytest.mark.parametrize("bins", [1, 2, 100, 127, 4096])
def test_bin_counts(bins):
    counts = check_against_numpy(values(5000, 2, bins, seed=bins), bins)
    assert counts.shape == (2, bins)
    check_against_numpy(values(3 * bins + 11, 1, bins, seed=bins + 1), bins)     # the whole planted set of every edge is in
    lo, hi = dyadic(bins)                                                        # ... and here it is ON every edge
    X = values(3 * bins + 300, 2, bins, seed=bins + 2, special=False, lo=lo, hi=hi)   # (a NaN may not replace a planted value)
    e32 = np.linspace(lo, hi, bins + 1).astype(np.float32)
    assert (e32.astype(np.float64) == np.linspace(lo, hi, bins + 1)).all() and np.isin(e32, X[:, 0]).all()
    check_against_numpy(X, bins, lo=lo, hi=hi)
    check_against_numpy(X, bins, cs=3, pad=2, lo=lo, hi=hi)


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65])
def test_every_row_in_one_bin(C):
    """The worst contention: a whole column, and every lane of every wave, on one counter."""
    T = 5000
    X = np.empty((T, C), dtype=np.float32)
    for c in range(C):
        X[:, c] = np.float32(LO + (HI - LO) * ((7 * c + 3) % 100 + 0.5) / 100)
    counts = check_against_numpy(X, 100)
    assert (counts.max(axis=1) == T).all()
    X[:, 0] = np.float32(HI)                                                      # all of it on the closed last edge
    assert check_against_numpy(X, 100)[0, 99] == T


def test_range_of_special_columns():
    X = values(300, 5, 100, seed=9, special=False)
    X[:, 1] = np.nan                                  # no finite entry: +inf / -inf
    X[:, 2] = np.float32(0.75)                        # constant
    X[::2, 3], X[1::2, 3] = np.float32(-0.0), np.float32(0.0)
    X[5, 4], X[6, 4] = np.inf, -np.inf                # the infinities are not the range
    buf, ld = strided(X)
    st, lo, hi, nf, ok = raw_range(buf, 300, 5, ld, 1)
    assert st == 0 and ok
    rlo, rhi, rnf = eo.column_ranges(X)
    assert (lo == rlo).all() and (hi == rhi).all() and (nf == rnf).all()
    assert lo[1] == np.inf and hi[1] == -np.inf and nf[1] == 300 and lo[2] == hi[2] == np.float32(0.75)
    assert np.signbit(lo[3]) and not np.signbit(hi[3])            # of -0 and +0: lo is -0, hi is +0, whatever the order
    assert np.isfinite(lo[4]) and np.isfinite(hi[4]) and nf[4] == 2


def test_halves_prefill_and_reproducibility():
    bins, T, C = 100, 5000, tile(100) + 1
    X = values(T, C, bins, seed=21)
    edges = np.stack([np.linspace(LO, HI, bins + 1)] * C)
    buf, ld = strided(X)
    st, whole, out_whole, ok = raw_hist(buf, T, C, ld, 1, edges, bins)
    assert st == 0 and ok
    st, again, out_again, ok = raw_hist(buf, T, C, ld, 1, edges, bins)
    assert st == 0 and ok and (again == whole).all() and (out_again == out_whole).all()           # the same call twice: the same bits
    # two calls on two halves accumulate to the whole; counts that were there before stay
    rng = np.random.default_rng(2)
    pre, pre_out = rng.integers(0, 2 ** 40, size=C * bins), rng.integers(0, 2 ** 40, size=3 * C)
    half = 2477
    a, la = strided(X[:half])
    b, lb = strided(X[half:])
    st, c1, o1, ok1 = raw_hist(a, half, C, la, 1, edges, bins, prefill=pre, outside_prefill=pre_out)
    st2, c2, o2, ok2 = raw_hist(b, T - half, C, lb, 1, edges, bins, prefill=c1.reshape(-1), outside_prefill=o1.reshape(-1))
    assert st == 0 and st2 == 0 and ok1 and ok2
    assert (c2 == whole + pre.reshape(C, bins)).all() and (o2 == out_whole + pre_out.reshape(C, 3)).all()


def test_non_uniform_edges():
    rng = np.random.default_rng(4)
    T, C, bins = 3000, 3, 37
    edges = np.sort(rng.uniform(LO, HI, size=(C, bins + 1)), axis=1)
    edges[2] = LO + (HI - LO) * np.linspace(0, 1, bins + 1) ** 3       # far from the uniform estimate: a long walk
    edges = edges.astype(np.float32).astype(np.float64)                # float32 numbers: the values below sit exactly on them
    assert (np.diff(edges, axis=1) > 0).all()
    X = values(T, C, bins, seed=5)
    inf = np.float32(np.inf)
    for c in range(C):
        e32 = edges[c].astype(np.float32)
        X[:3 * (bins + 1), c] = np.concatenate([e32, np.nextafter(e32, -inf), np.nextafter(e32, inf)])
    buf, ld = strided(X)
    st, counts, outside, ok = raw_hist(buf, T, C, ld, 1, edges, bins)
    assert st == 0 and ok
    for c in range(C):
        x = X[:, c].astype(np.float64)
        x = x[~np.isnan(x)]
        assert (counts[c] == np.histogram(x, bins=edges[c])[0]).all()
        assert outside[c, 0] == (x < edges[c, 0]).sum() and outside[c, 1] == (x > edges[c, -1]).sum()


def test_row_offsets_beyond_2_to_the_31():
    """Three rows 2^30 floats apart: the last row starts at element 2^31.  Only the columns are written and read."""
    ld, C, T = 1 << 30, 2, 3
    buf = torch.empty(2 * ld + C, dtype=torch.float32, device=dev())
    X = np.array([[0.5, 1.5], [2.5, -1.0], [3.25, 0.0]], dtype=np.float32)
    for r in range(T):
        buf[r * ld:r * ld + C] = torch.as_tensor(X[r]).to(dev())
    st, lo, hi, nf, ok = raw_range(buf, T, C, ld, 1)
    assert st == 0 and ok and lo.tolist() == [0.5, -1.0] and hi.tolist() == [3.25, 1.5] and nf.tolist() == [0, 0]
    edges = np.stack([np.linspace(LO, HI, 11)] * C)
    st, counts, outside, ok = raw_hist(buf, T, C, ld, 1, edges, 10)
    assert st == 0 and ok and (counts == eo.histogram_columns(X, 10, LO, HI)[0]).all() and outside.sum() == 0


# ---- pairs ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def molecule(n_atoms):
    """(coords [T, V, 3] float32, bonded pairs [n, 2]) - 2: a dimer; 22 / 691: the fixtures' frames tiled with noise."""
    from timewarp_amd import forcefield as ffm

    rng = np.random.default_rng(n_atoms)
    if n_atoms == 2:
        return rng.normal(size=(777, 2, 3)).astype(np.float32), np.array([[0, 1]], dtype=np.int32)
    if n_atoms == 22:
        base = np.load(os.path.join(GOLDEN, "ad_topology.npz"))["coords_nm"][None]
        bonds = ffm.alanine_dipeptide_amber99sb().bond_idx
        T = 777
    else:
        z = np.load(os.path.join(GOLDEN, "energy_kat_1hgv.npz"))
        base = z["positions"]
        bonds = ffm.amber99sbildn_obc_tables(list(z["atom_names"]), list(z["residue_names"]), list(z["residue_ids"])).bond_idx
        T = 130
    x = np.concatenate([base] * (T // len(base) + 1))[:T]
    return (x + rng.normal(scale=0.004, size=x.shape)).astype(np.float32), np.asarray(bonds, dtype=np.int32).reshape(-1, 2)


def pair_cases():
    out = [(2, 1), (22, 1), (22, 21), (691, 1), (691, 21)]
    return out + [(691, "tile-1"), (691, "tile"), (691, "tile+1")]


def pick_pairs(bonds, P, bins=100):
    if isinstance(P, str):
        P = tile(bins) + {"tile-1": -1, "tile": 0, "tile+1": 1}[P]
    assert P <= len(bonds)
    return bonds[:P]


@pytest.mark.parametrize("n_atoms,P", pair_cases())
def test_pair_distances_within_one_ulp_and_fused_equals_columns(n_atoms, P):
    coords, bonds = molecule(n_atoms)
    pairs = pick_pairs(bonds, P)
    st, d, ok = raw_pairs(coords, pairs)
    assert st == 0 and ok
    assert eo.ulp_distance_f32(d, eo.pair_distances_longdouble(coords, pairs)).max() <= 1.0
    # the fused range and histogram are tw_column_* on this very output
    T, n = d.shape
    buf, ld = strided(d)
    st, lo, hi, nf, ok = raw_range(buf, T, n, ld, 1)
    st2, flo, fhi, fnf, ok2 = raw_pairs(coords, pairs, what="range")
    assert st == 0 and st2 == 0 and ok and ok2
    assert (lo == flo).all() and (hi == fhi).all() and (nf == fnf).all() and (lo == eo.column_ranges(d)[0]).all()
    for bins in (100, 127):
        edges = np.stack([np.linspace(l, h, bins + 1) for l, h in zip(lo.astype(np.float64), hi.astype(np.float64))])
        st, counts, outside, ok = raw_hist(buf, T, n, ld, 1, edges, bins)
        st2, fcounts, foutside, ok2 = raw_pairs(coords, pairs, edges, bins, what="histogram")
        assert st == 0 and st2 == 0 and ok and ok2
        assert (counts == fcounts).all() and (outside == foutside).all()
        assert (counts == eo.histogram_columns(d, bins, lo.astype(np.float64), hi.astype(np.float64))[0]).all()
        assert outside.sum() == 0 and (counts.sum(axis=1) == T).all()


def test_repeated_pair_self_pair_and_non_finite_coordinates():
    coords, bonds = molecule(22)
    coords = coords[:65].copy()
    pairs = np.array([[0, 1], [2, 3], [4, 6], [5, 5], [0, 1], [1, 0]], dtype=np.int32)     # a self pair, a repeated and a reversed pair
    coords[7, 2, 2] = np.nan
    coords[9, 6, 0] = np.inf
    st, d, ok = raw_pairs(coords, pairs)
    assert st == 0 and ok
    assert (d[:, 3] == 0).all() and (d[:, 4] == d[:, 0]).all() and (d[:, 5] == d[:, 0]).all()
    bad = ~np.isfinite(d)
    expect = np.zeros_like(bad)
    expect[7, 1], expect[9, 2] = True, True
    assert (bad == expect).all() and np.isnan(d[7, 1])
    assert eo.ulp_distance_f32(d, eo.pair_distances_longdouble(coords, pairs)).max() <= 1.0
    st, lo, hi, nf, ok = raw_pairs(coords, pairs, what="range")
    assert st == 0 and ok and nf.tolist() == [0, 1, 1, 0, 0, 0] and (lo == eo.column_ranges(d)[0]).all()
    edges = np.stack([np.linspace(0.0, 0.3, 11)] * len(pairs))
    st, counts, outside, ok = raw_pairs(coords, pairs, edges, 10, what="histogram")
    assert st == 0 and ok
    rc, _, below, above, nan = eo.histogram_columns(d, 10, 0.0, 0.3)
    assert (counts == rc).all() and (outside[:, 2] == nan).all() and (outside[:, 1] == above).all() and outside[1, 2] == 1 and outside[2, 1] >= 1


# ---- refusals and empty calls -----------------------------------------------------------------------------------------------------------

def last_error():
    return lib().tw_last_error().decode()


def test_refusals_write_nothing():
    X = values(100, 4, 100, seed=1)
    buf, ld = strided(X)
    edges = np.stack([np.linspace(LO, HI, 101)] * 4)
    big_cols = tile(4096) * (1 << 20) + 1
    # (what the call is told where it differs from the buffers, the word tw_last_error must hold, whether tw_column_range shares the refusal)
    cases = [
        (dict(T=-1), "n_rows", True), (dict(C=-1), "n_cols", True), (dict(ld=3), "ld", True), (dict(cs=0), "col_stride", True),
        (dict(cs=2, ld=6), "ld", True), (dict(T=1 << 32), "n_rows", True),
        (dict(cs=(1 << 38) + 1, ld=1 << 62), "col_stride", True),           # (n_cols - 1) col_stride + 1 must not wrap past a small ld
        (dict(cs=1 << 62, ld=4), "col_stride", True),                       # 3 x 2^62 + 1 wraps to a negative number (dict(C=(1 << 24) + 1, ld=1 << 25), "n_cols", True),
        (dict(bins=0), "n_bins", False), (dict(bins=4097), "n_bins", False), (dict(bins=-5), "n_bins", False),
        (dict(C=big_cols, ld=big_cols, bins=4096), "column tiles", False),
    ]
    e = torch.as_tensor(edges).to(dev())
    for override, word, also_range in cases:
        a = dict(T=100, C=4, ld=ld, cs=1, bins=100)
        a.update(override)
        # outputs sized for the honest call: a refused call must not touch them at all
        counts = guarded(400, torch.int64, POISON_I)
        outside = guarded(12, torch.int64, POISON_I)
        st = lib().tw_column_histogram(buf.data_ptr(), a["T"], a["C"], a["ld"], a["cs"], e.data_ptr(), a["bins"],
                                       counts[GUARD:].data_ptr(), outside[GUARD:].data_ptr(), stream())
        torch.cuda.synchronize()
        assert st == -1 and word in last_error(), (override, last_error())
        assert bool((counts == POISON_I).all()) and bool((outside == POISON_I).all()), override
        if not also_range:
            continue
        lo, hi, nf = guarded(4, torch.float32, POISON_F), guarded(4, torch.float32, POISON_F), guarded(4, torch.int64, POISON_I)
        st = lib().tw_column_range(buf.data_ptr(), a["T"], a["C"], a["ld"], a["cs"], lo[GUARD:].data_ptr(), hi[GUARD:].data_ptr(),
                                   nf[GUARD:].data_ptr(), stream())
        torch.cuda.synchronize()
        assert st == -1 and word in last_error(), (override, last_error())
        assert bool((lo == POISON_F).all()) and bool((hi == POISON_F).all()) and bool((nf == POISON_I).all()), override
    # NULL pointers
    counts, outside = guarded(400, torch.int64, POISON_I), guarded(12, torch.int64, POISON_I)
    e = torch.as_tensor(edges).to(dev())
    for args in ((None, e.data_ptr(), counts[GUARD:].data_ptr(), outside[GUARD:].data_ptr()),
                 (buf.data_ptr(), None, counts[GUARD:].data_ptr(), outside[GUARD:].data_ptr()),
                 (buf.data_ptr(), e.data_ptr(), None, outside[GUARD:].data_ptr()),
                 (buf.data_ptr(), e.data_ptr(), counts[GUARD:].data_ptr(), None)):
        st = lib().tw_column_histogram(args[0], 100, 4, ld, 1, args[1], 100, args[2], args[3], stream())
        torch.cuda.synchronize()
        assert st == -1 and "NULL" in last_error()
    assert bool((counts == POISON_I).all()) and bool((outside == POISON_I).all())
    st, _, _, _, ok = raw_range(buf, 100, 4, ld, 1, x_ptr=False)
    assert st == -1 and ok and "NULL" in last_error()
    lo, hi, nf = guarded(4, torch.float32, POISON_F), guarded(4, torch.float32, POISON_F), guarded(4, torch.int64, POISON_I)
    outs = (lo[GUARD:].data_ptr(), hi[GUARD:].data_ptr(), nf[GUARD:].data_ptr())
    for k in range(3):                                   # each output of tw_column_range in turn
        a = [None if i == k else o for i, o in enumerate(outs)]
        st = lib().tw_column_range(buf.data_ptr(), 100, 4, ld, 1, a[0], a[1], a[2], stream())
        torch.cuda.synchronize()
        assert st == -1 and "NULL" in last_error(), k
    assert bool((lo == POISON_F).all()) and bool((hi == POISON_F).all()) and bool((nf == POISON_I).all())
    # the pair calls
    coords, bonds = molecule(22)
    x = torch.as_tensor(coords).to(dev())
    p = torch.as_tensor(bonds).to(dev())
    out = guarded(777 * 21, torch.float32, POISON_F)
    for T, P, V, xp, word in ((-1, 21, 22, x.data_ptr(), "n_rows"), (777, -2, 22, x.data_ptr(), "n_pairs"), (777, 21, 0, x.data_ptr(), "n_atoms"),
                              (777, 21, 22, None, "NULL"), (777, (1 << 24) + 1, 22, x.data_ptr(), "n_pairs")):
        st = lib().tw_pair_distances(xp, p.data_ptr(), P, out[GUARD:].data_ptr(), T, V, stream())
        torch.cuda.synchronize()
        assert st == -1 and word in last_error(), (T, P, V, last_error())
        counts, outside = guarded(2100, torch.int64, POISON_I), guarded(63, torch.int64, POISON_I)
        e21 = torch.as_tensor(np.stack([np.linspace(0, 1, 101)] * 21)).to(dev())
        st = lib().tw_pair_histogram(xp, p.data_ptr(), P, T, V, e21.data_ptr(), 100, counts[GUARD:].data_ptr(), outside[GUARD:].data_ptr(),
                                     stream())
        torch.cuda.synchronize()
        assert st == -1 and word in last_error(), (T, P, V, last_error())
        assert bool((counts == POISON_I).all()) and bool((outside == POISON_I).all())
        lo, hi, nf = guarded(21, torch.float32, POISON_F), guarded(21, torch.float32, POISON_F), guarded(21, torch.int64, POISON_I)
        st = lib().tw_pair_range(xp, p.data_ptr(), P, T, V, lo[GUARD:].data_ptr(), hi[GUARD:].data_ptr(), nf[GUARD:].data_ptr(), stream())
        torch.cuda.synchronize()
        assert st == -1 and word in last_error()
        assert bool((lo == POISON_F).all()) and bool((hi == POISON_F).all()) and bool((nf == POISON_I).all())
    assert bool((out == POISON_F).all())
    # NULL for each pointer of the pair calls in turn
    counts, outside = guarded(2100, torch.int64, POISON_I), guarded(63, torch.int64, POISON_I)
    lo, hi, nf = guarded(21, torch.float32, POISON_F), guarded(21, torch.float32, POISON_F), guarded(21, torch.int64, POISON_I)
    e21 = torch.as_tensor(np.stack([np.linspace(0, 1, 101)] * 21)).to(dev())
    ptrs = [x.data_ptr(), p.data_ptr(), e21.data_ptr(), counts[GUARD:].data_ptr(), outside[GUARD:].data_ptr()]
    for k in range(5):
        a = [None if i == k else v for i, v in enumerate(ptrs)]
        st = lib().tw_pair_histogram(a[0], a[1], 21, 777, 22, a[2], 100, a[3], a[4], stream())
        torch.cuda.synchronize()
        assert st == -1 and "NULL" in last_error(), k
    ptrs = [x.data_ptr(), p.data_ptr(), lo[GUARD:].data_ptr(), hi[GUARD:].data_ptr(), nf[GUARD:].data_ptr()]
    for k in range(5):
        a = [None if i == k else v for i, v in enumerate(ptrs)]
        st = lib().tw_pair_range(a[0], a[1], 21, 777, 22, a[2], a[3], a[4], stream())
        torch.cuda.synchronize()
        assert st == -1 and "NULL" in last_error(), k
    ptrs = [x.data_ptr(), p.data_ptr(), out[GUARD:].data_ptr()]
    for k in range(3):
        a = [None if i == k else v for i, v in enumerate(ptrs)]
        st = lib().tw_pair_distances(a[0], a[1], 21, a[2], 777, 22, stream())
        torch.cuda.synchronize()
        assert st == -1 and "NULL" in last_error(), k
    assert bool((counts == POISON_I).all()) and bool((outside == POISON_I).all()) and bool((out == POISON_F).all())
    assert bool((lo == POISON_F).all()) and bool((hi == POISON_F).all()) and bool((nf == POISON_I).all())
    assert lib().tw_histogram_column_tile(0) == -1 and lib().tw_histogram_column_tile(4097) == -1


def test_empty_calls_launch_nothing_and_write_nothing():
    X = values(10, 3, 100, seed=1)
    buf, ld = strided(X)
    edges = np.stack([np.linspace(LO, HI, 101)] * 3)
    for T, C in ((0, 3), (10, 0), (0, 0)):
        st, lo, hi, nf, ok = raw_range(buf, T, C, ld, 1)
        assert st == 0 and ok and (lo == np.float32(POISON_F)).all() and (nf == POISON_I).all()
        pre = np.arange(C * 100, dtype=np.int64)
        st, counts, outside, ok = raw_hist(buf, T, C, ld, 1, edges[:max(C, 1)], 100, prefill=pre)
        assert st == 0 and ok and (counts.reshape(-1) == pre).all() and outside.sum() == 0
    coords, bonds = molecule(22)
    for c, p in ((coords[:0], bonds), (coords, bonds[:0])):
        st, d, ok = raw_pairs(c, p)
        assert st == 0 and ok and d.size == 0
        st, lo, hi, nf, ok = raw_pairs(c, p, what="range")
        assert st == 0 and ok and (lo == np.float32(POISON_F)).all()
        st, counts, outside, ok = raw_pairs(c, p, np.stack([np.linspace(0, 1, 11)] * max(len(p), 1)), 10, what="histogram")
        assert st == 0 and ok and counts.sum() == 0 and outside.sum() == 0


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------

def same_histograms(a, b):
    return all((getattr(a, f) == getattr(b, f)).all() for f in ("counts", "edges", "below", "above", "nonfinite"))


def test_driver_routes_agree_on_the_device():
    from timewarp_amd import evaluate as ev

    X = torch.as_tensor(values(5000, 5, 100, seed=3, special=False)).to(dev())
    assert same_histograms(ev.column_histograms(X, route="kernel"), ev.column_histograms(X, route="torch"))
    assert same_histograms(ev.column_histograms(X, route="kernel", chunk_rows=1234), ev.column_histograms(X.cpu().numpy(), route="kernel"))
    Y = torch.as_tensor(np.random.default_rng(0).normal(size=(700, 9, 3)).astype(np.float32)).to(dev())
    assert same_histograms(ev.column_histograms(Y[:, :, 0], bins=127, route="kernel"),       # read in place: ld 27, col_stride 3
                           ev.column_histograms(Y[:, :, 0].contiguous(), bins=127, route="torch"))
    assert same_histograms(ev.column_histograms(Y[:, 0, :].T, bins=10, route="kernel"),      # a view the kernel cannot read: copied
                           ev.column_histograms(Y[:, 0, :].T.contiguous(), bins=10, route="torch"))
    bad = X.clone()
    bad[17, 2] = float("nan")
    with pytest.raises(ValueError, match=r"column 2 holds 1 non-finite"):
        ev.column_histograms(bad, route="kernel")
    h = ev.column_histograms(bad, range=(LO, HI), route="kernel")
    assert h.nonfinite.tolist() == [0, 0, 1, 0, 0] and same_histograms(h, ev.column_histograms(bad, range=(LO, HI), route="torch"))
    coords, bonds = molecule(691)
    hists = [ev.pair_histograms(torch.as_tensor(coords).to(dev()), bonds, route=r) for r in ev.PAIR_ROUTES]
    assert same_histograms(hists[0], hists[1]) and same_histograms(hists[0], hists[2])
    bonds_k, (phi, psi) = ev.compute_internal_coordinates(np.load(os.path.join(GOLDEN, "energy_kat_1hgv.npz")), bonds, coords)
    assert bonds_k.shape == (130, len(bonds)) and phi.shape == (130, 45) and psi.shape[0] == 130
    assert eo.ulp_distance_f32(bonds_k, eo.pair_distances_longdouble(coords, bonds)).max() <= 1.0


def integer_fields(arrays):
    return {k: v for k, v in arrays.items() if np.asarray(v).dtype.kind in "iu"}


def test_report_and_command_line_agree_with_the_torch_route(tmp_path):
    from tests.test_evaluate_cpu import cli_files, report_inputs
    from timewarp_amd import evaluate as ev

    model, md, topo, bonds, ll = report_inputs()
    reports = {r: ev.evaluation_report(model, md, topo, bonds, bins=50, log_likelihoods=ll, route=r, chunk_rows=17).arrays()
               for r in ev.PAIR_ROUTES}
    ints = integer_fields(reports["torch"])
    assert {"bonds_model_counts", "delta_x_md_counts", "e_pot_model_below", "ramachandran_model", "likelihood_forward_counts"} <= set(ints)
    for r in ("fused", "kernel"):
        for k, v in ints.items():
            assert np.array_equal(reports[r][k], v), (r, k)
        for k in ("bonds_model_edges", "velocs_md_edges", "bonds_js", "correlation_model"):
            assert np.allclose(reports[r][k], reports["torch"][k], rtol=0, atol=1e-12, equal_nan=True), (r, k)
    mdf, chain, pdb, _, _, _ = cli_files(tmp_path)
    outs = {}
    for r in ("fused", "torch"):
        out = str(tmp_path / f"{r}.npz")
        ev.main(["--md", mdf, "--model-dir", chain, "--protein", "nnqq", "--pdb", pdb, "--bins", "25", "--chunk-frames", "11", "--route", r,
                 "--out", out, "--no-energies"])
        outs[r] = ev.load_report(out)
    for k, v in integer_fields(outs["torch"]).items():
        assert np.array_equal(outs["fused"][k], v), k
    out = ev.main(["--md", mdf, "--model-dir", chain, "--protein", "nnqq", "--pdb", pdb, "--out", str(tmp_path / "default.npz")])
    back = ev.load_report(out)
    assert back["e_pot_model_counts"].sum() == 30 and back["e_pot_md_counts"].sum() == 32 and back["bonds_md_counts"].shape == (64, 100)


def test_conditional_md_samples_are_rows_of_one_step():
    from timewarp_amd import evaluate as ev
    from timewarp_amd import synthetic
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from timewarp_amd.md import LangevinDynamics

    _, coords, masses = synthetic.alanine_dipeptide_state()
    energy = AmberPotentialEnergyTorch.alanine_dipeptide()
    velocs = torch.randn(22, 3, generator=torch.Generator().manual_seed(0)) * 0.3
    S = 6
    x, v = ev.conditional_md_samples(LangevinDynamics(energy, masses, seed=11), coords, velocs, S, step_width=5)
    assert x.shape == (S, 22, 3) and v.shape == (S, 22, 3) and x.is_cuda
    direct = LangevinDynamics(energy, masses, seed=11)
    rx, rv = direct.step(coords.to(dev())[None].expand(S, 22, 3).contiguous(), velocs.to(dev())[None].expand(S, 22, 3).contiguous(),
                         num_steps=5)
    assert torch.equal(x, rx) and torch.equal(v, rv)
    for i in range(S):
        for j in range(i):
            assert not torch.equal(x[i], x[j])
    assert float((x - coords.to(dev())).abs().max()) < 0.1           # five 0.5 fs steps: still the same molecule
    g = torch.Generator(device=dev()).manual_seed(3)
    x2, v2 = ev.conditional_md_samples(LangevinDynamics(energy, masses, seed=11), coords, None, S, step_width=5, random_velocs=True,
                                       generator=g)
    assert not torch.equal(x2, x) and torch.isfinite(x2).all()
