"""`tw_joint_histogram` through the C ABI and its drivers on the device, against the numpy restatement
tests/joint_histogram_oracle.py (np.histogramdd on float64 casts): counts and outside counters EQUAL it, no tolerance anywhere.

Shapes sit on each side of every boundary the kernel has.  Rows: 1, 63, 64, 65 (a wave), 511 .. 513 (a workgroup's row block),
2047 .. 2049 (one trip of the four-row unrolled loop), and one row on each side of the row-share rule (`shares` below restates the
header: a share reads at least as many rows as it has counters - 10 000 at 100 x 100, so the second share appears at 20 000 rows).
Planes: 1 x 1, 1 x 7, 100 x 100, and - placed from `tw_joint_histogram_bands`, not from a constant - the largest plane of one band,
the smallest of two and one with a ragged last band; 4095 x 4 is the largest single band there is (16 380 of 16 381 counters),
4096 x 4 and 4 x 4096 have two.  Pairs: 1, 3; (pair, band) units are the grid's x dimension, 2^24 pairs of at most 86 bands stay
below 2^31, so "one more than a grid dimension's worth" cannot be asked for: the limit that refuses is n_pairs > 2^24, tested with
the refusals.  Every raw call runs on over-allocated outputs whose guard bands must come back untouched."""
import numpy as np
import pytest
import torch

from tests import joint_histogram_oracle as jo
from tests.test_evaluate_gpu import GUARD, POISON_I, body, clean, dev, guarded, last_error, lib, stream, strided

pytestmark = pytest.mark.gpu

LO, HI = -1.25, 3.5
AUTO, PLAIN, VOTE = 0, 1, 2


def bands(bx, by):
    return int(lib().tw_joint_histogram_bands(bx, by))


def band_rows(bx, by):
    return min(bx, (16384 - 3) // by)


def shares(T, P, bx, by):
    """The header's row shares of a (pair, band)."""
    units = P * bands(bx, by)
    return max(1, min(-(-1024 // units), T // (band_rows(bx, by) * by), -(-T // 512)))


def raw_joint(buf, T, C, ld, cs, pairs, ex, ey, bx, by, prefill=None, outside_prefill=None, path=None, P=None):
    """One tw_joint_histogram (path None) or tw_joint_histogram_path call.  Returns (status, counts [P, bx, by], outside [P, 3], clean)."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    P = len(pairs) if P is None else P
    n = max(P, 0) * max(bx, 0) * max(by, 0)
    counts = guarded(n, torch.int64, POISON_I, fill=np.zeros(n, dtype=np.int64) if prefill is None else prefill)
    outside = guarded(3 * max(P, 0), torch.int64, POISON_I,
                      fill=np.zeros(3 * max(P, 0), dtype=np.int64) if outside_prefill is None else outside_prefill)
    pd = torch.as_tensor(pairs).to(dev()) if len(pairs) else torch.zeros(2, dtype=torch.int32, device=dev())
    exd = torch.as_tensor(np.ascontiguousarray(ex, dtype=np.float64)).to(dev())
    eyd = torch.as_tensor(np.ascontiguousarray(ey, dtype=np.float64)).to(dev())
    args = (buf.data_ptr(), T, C, ld, cs, pd.data_ptr(), P, exd.data_ptr(), bx, eyd.data_ptr(), by, counts[GUARD:].data_ptr(),
            outside[GUARD:].data_ptr())
    st = lib().tw_joint_histogram(*args, stream()) if path is None else lib().tw_joint_histogram_path(*args, path, stream())
    torch.cuda.synchronize()
    ok = clean(counts, n, POISON_I) and clean(outside, 3 * max(P, 0), POISON_I)
    return st, body(counts, n).reshape(max(P, 0), max(bx, 0), max(by, 0)), body(outside, 3 * max(P, 0)).reshape(-1, 3), ok


def matrix(T, C, bins, seed, lo=LO, hi=HI, special=True):
    """[T, C] float32: per column the planted-edge set of (lo, hi, bins) as far as T allows and uniform draws that reach outside;
    with `special` a NaN and both infinities per column where there is room."""
    rng = np.random.default_rng(seed)
    X = np.stack([jo.planted(lo, hi, bins, rng, T) for _ in range(C)], axis=1)
    if special and T >= 8:
        for c in range(C):
            r = rng.choice(T, size=3, replace=False)
            X[r[0], c], X[r[1], c], X[r[2], c] = np.nan, np.inf, -np.inf
    return X


def check(X, pairs, bx, by, cs=1, pad=0, lo=LO, hi=HI, path=None):
    T, C = X.shape
    P = len(pairs)
    buf, ld = strided(X, ld=(C - 1) * cs + 1 + pad, col_stride=cs)
    ex, ey = jo.linspace_tables(lo, hi, bx, P), jo.linspace_tables(lo, hi, by, P)
    st, counts, outside, ok = raw_joint(buf, T, C, ld, cs, pairs, ex, ey, bx, by, path=path)
    assert st == 0 and ok, last_error()
    rc, ro = jo.joint_pairs(X, pairs, ex, ey)
    assert (counts == rc).all() and (outside == ro).all()
    assert (counts.sum(axis=(1, 2)) + outside.sum(axis=1) == T).all()
    return counts, outside


PAIRS3 = [[0, 2], [1, 1], [2, 0]]


@pytest.mark.parametrize("T", [1, 63, 64, 65, 511, 512, 513, 777, 2047, 2048, 2049])
@pytest.mark.parametrize("P", [1, 3])
def test_rows_on_each_side_of_a_wave_a_row_block_and_a_trip(T, P):
    X = matrix(T, 3, 100, seed=T + P)
    pairs = PAIRS3[:P]
    for path in (None, PLAIN, VOTE):
        check(X, pairs, 100, 100, path=path)
    check(X, pairs, 100, 100, cs=3, pad=5)              # NaN between the columns and behind them: it must not be read
    check(X, pairs, 7, 5, cs=1, pad=3)


@pytest.mark.parametrize("where", [-1, 0, 1])
def test_rows_on_each_side_of_the_row_share_rule(where):
    T = 20000 + where
    assert shares(19999, 1, 100, 100) == 1 and shares(20000, 1, 100, 100) == 2 and shares(20001, 1, 100, 100) == 2
    X = matrix(T, 2, 100, seed=where + 5)
    check(X, [[0, 1]], 100, 100)
    assert shares(5000, 1, 7, 5) == 10 and shares(5000, 3, 7, 5) == 10    # bounded by the row blocks: ragged last blocks
    check(X[:5000], [[0, 1], [1, 0], [1, 1]], 7, 5)


def one_band_limit(by):
    """(the largest bx with one band, found from tw_joint_histogram_bands)."""
    bx = 1
    while bands(bx + 1, by) == 1:
        bx += 1
    return bx


def plane_cases():
    return [(1, 1), (1, 7), (7, 1), (100, 100), "largest one band", "smallest two bands", "ragged last band", (4095, 4), (4096, 4), (4, 4096)]


@pytest.mark.parametrize("plane", plane_cases(), ids=str)
def test_planes_and_bands(plane):
    by = 127
    full = one_band_limit(by)
    assert bands(full, by) == 1 and bands(full + 1, by) == 2 and full == band_rows(full + 1, by)
    if plane == "largest one band":
        bx, n = full, 1
    elif plane == "smallest two bands":
        bx, n = full + 1, 2
    elif plane == "ragged last band":
        bx, n = 2 * full + 44, 3                          # the last band has 44 of `full` x-rows
    else:
        (bx, by), n = plane, {(4096, 4): 2, (4, 4096): 2}.get(plane, 1)
    assert bands(bx, by) == n == -(-bx // band_rows(bx, by))
    T = 6000
    X = matrix(T, 2, max(bx, by), seed=bx + by)
    check(X, [[0, 1]], bx, by)
    check(X, [[1, 0], [0, 0]], bx, by, cs=3, pad=2, path=PLAIN)
    lo, hi = -0.5, -0.5 + max(bx, by) / 64.0             # edges that ARE float32 numbers: values exactly on them
    X = matrix(3 * max(bx, by) + 300, 2, max(bx, by), seed=bx, lo=lo, hi=hi, special=False)
    e32 = np.linspace(lo, hi, max(bx, by) + 1).astype(np.float32)
    assert (e32.astype(np.float64) == np.linspace(lo, hi, max(bx, by) + 1)).all() and np.isin(e32, X[:, 0]).all()
    check(X, [[0, 1], [1, 0]], bx, by, lo=lo, hi=hi)


def test_band_counts_and_refused_planes():
    assert bands(100, 100) == 1 and bands(1024, 1024) == 69 and bands(4096, 256) == -(-4096 // 63) and bands(256, 4096) == 86
    for bx, by in ((0, 5), (5, 0), (4097, 1), (1, 4097), (1025, 1024), (-1, -1)):
        assert bands(bx, by) == -1
    # many bands: every one reads the rows and counts its own x-rows; the outside counters are added once
    X = matrix(4000, 2, 300, seed=11)
    counts, outside = check(X, [[0, 1], [1, 0]], 300, 1024)
    assert bands(300, 1024) == 20 and outside.min() > 0


@pytest.mark.parametrize("path", [PLAIN, VOTE])
def test_every_row_in_one_bin(path):
    """The worst contention: every lane of every wave on one counter - the count is n_rows."""
    T = 50000
    X = np.empty((T, 2), dtype=np.float32)
    X[:, 0], X[:, 1] = np.float32(LO + (HI - LO) * 37.5 / 100), np.float32(HI)         # y on the closed last edge
    counts, outside = check(X, [[0, 1], [1, 1]], 100, 100, path=path)
    assert counts[0, 37, 99] == T and counts[1, 99, 99] == T and outside.sum() == 0
    X[:, 0] = np.nan
    counts, outside = check(X, [[0, 1]], 100, 100, path=path)
    assert outside[0].tolist() == [0, 0, T]


def test_time_ordered_and_shuffled_rows_count_the_same():
    T = 40000
    X = jo.trajectory(T, seed=3)
    lo, hi = float(X.min()), float(X.max())
    shuffled = X[np.random.default_rng(0).permutation(T)]
    got = [check(x, [[0, 1]], 100, 100, lo=lo, hi=hi, path=path)[0] for x in (X, shuffled) for path in (PLAIN, VOTE, None)]
    assert all((g == got[0]).all() for g in got) and got[0].sum() == T and got[0].max() > 200     # crowded counters


def test_non_finite_values():
    X = matrix(700, 2, 10, seed=5, special=False)
    inside = np.float32(1.0)
    X[:12, 0] = [np.nan, inside, np.nan, np.inf, -np.inf, inside, inside, np.inf, np.nan, np.inf, np.float32(LO - 1), inside]
    X[:12, 1] = [inside, np.nan, np.nan, inside, inside, np.inf, -np.inf, np.inf, np.inf, np.nan, np.float32(HI + 1), np.float32(HI + 1)]
    _, outside = check(X, [[0, 1]], 10, 10)
    _, base = check(X[12:], [[0, 1]], 10, 10)
    assert (outside[0] - base[0]).tolist() == [4, 3, 5]            # NaN in either wins, then x outside, then y outside
    check(X, [[0, 1], [1, 0]], 300, 1024)                          # the same through twenty bands


def test_non_uniform_edges_per_pair():
    rng = np.random.default_rng(7)
    bx, by, P, T = 9, 37, 2, 3000
    ex = np.sort(rng.uniform(LO, HI, size=(P, bx + 1)), axis=1).astype(np.float32).astype(np.float64)
    ey = np.stack([LO + (HI - LO) * np.linspace(0, 1, by + 1) ** 3, np.sort(rng.uniform(LO, HI, size=by + 1))])
    ey = ey.astype(np.float32).astype(np.float64)                  # far from the uniform estimate: a long walk
    assert (np.diff(ex, axis=1) > 0).all() and (np.diff(ey, axis=1) > 0).all()
    X = matrix(T, 2, 10, seed=8)
    inf = np.float32(np.inf)
    for c, e in ((0, ex[0]), (1, ey[0])):
        e32 = e.astype(np.float32)
        X[:3 * len(e32), c] = np.concatenate([e32, np.nextafter(e32, -inf), np.nextafter(e32, inf)])
    pairs = [[0, 1], [1, 1]]
    ex[1] = ey[1][:bx + 1]
    buf, ld = strided(X)
    st, counts, outside, ok = raw_joint(buf, T, 2, ld, 1, pairs, ex, ey, bx, by)
    assert st == 0 and ok
    rc, ro = jo.joint_pairs(X, pairs, ex, ey)
    assert (counts == rc).all() and (outside == ro).all()


def test_halves_prefill_and_reproducibility():
    bx, by, T, P = 300, 127, 30000, 3                              # three bands, two row shares
    assert bands(bx, by) == 3
    X = matrix(T, 3, 300, seed=21)
    ex, ey = jo.linspace_tables(LO, HI, bx, P), jo.linspace_tables(LO, HI, by, P)
    buf, ld = strided(X)
    st, whole, out_whole, ok = raw_joint(buf, T, 3, ld, 1, PAIRS3, ex, ey, bx, by)
    assert st == 0 and ok
    st, again, out_again, ok = raw_joint(buf, T, 3, ld, 1, PAIRS3, ex, ey, bx, by)
    assert st == 0 and ok and (again == whole).all() and (out_again == out_whole).all()        # the same call twice: the same bits
    rng = np.random.default_rng(2)
    pre, pre_out = rng.integers(0, 2 ** 40, size=P * bx * by), rng.integers(0, 2 ** 40, size=3 * P)
    half = 14321
    a, la = strided(X[:half])
    b, lb = strided(X[half:])
    st, c1, o1, ok1 = raw_joint(a, half, 3, la, 1, PAIRS3, ex, ey, bx, by, prefill=pre, outside_prefill=pre_out)
    st2, c2, o2, ok2 = raw_joint(b, T - half, 3, lb, 1, PAIRS3, ex, ey, bx, by, prefill=c1.reshape(-1), outside_prefill=o1.reshape(-1))
    assert st == 0 and st2 == 0 and ok1 and ok2
    assert (c2 == whole + pre.reshape(P, bx, by)).all() and (o2 == out_whole + pre_out.reshape(P, 3)).all()
    assert (whole == jo.joint_pairs(X, PAIRS3, ex, ey)[0]).all()


def test_row_offsets_beyond_2_to_the_31():
    """Three rows 2^30 floats apart: the last row starts at element 2^31.  Only the columns are written and read."""
    ld, C, T = 1 << 30, 2, 3
    buf = torch.empty(2 * ld + C, dtype=torch.float32, device=dev())
    X = np.array([[0.5, 1.5], [2.5, -1.0], [3.25, 0.0]], dtype=np.float32)
    for r in range(T):
        buf[r * ld:r * ld + C] = torch.as_tensor(X[r]).to(dev())
    ex, ey = jo.linspace_tables(LO, HI, 10, 1), jo.linspace_tables(LO, HI, 6, 1)
    st, counts, outside, ok = raw_joint(buf, T, C, ld, 1, [[0, 1]], ex, ey, 10, 6)
    rc, ro = jo.joint_pairs(X, [[0, 1]], ex, ey)
    assert st == 0 and ok and (counts == rc).all() and outside.sum() == 0 and counts.sum() == 3


def test_refusals_and_null_pointers_write_nothing():
    X = matrix(100, 4, 100, seed=1)
    buf, ld = strided(X)
    pairs = np.array([[0, 1], [2, 3]], dtype=np.int32)
    pd = torch.as_tensor(pairs).to(dev())
    e = torch.as_tensor(jo.linspace_tables(LO, HI, 100, 2)).to(dev())
    cases = [
        (dict(T=-1), "n_rows"), (dict(T=1 << 32), "n_rows"), (dict(C=-1), "n_cols"), (dict(C=(1 << 24) + 1, ld=1 << 25), "n_cols"),
        (dict(C=0), "n_cols"), (dict(ld=3), "ld"), (dict(cs=2, ld=6), "ld"), (dict(cs=0), "col_stride"),
        (dict(cs=(1 << 38) + 1, ld=1 << 62), "col_stride"), (dict(cs=1 << 62, ld=4), "col_stride"),
        (dict(P=-1), "n_pairs"), (dict(P=(1 << 24) + 1), "n_pairs"),
        (dict(bx=0), "bins_x"), (dict(bx=4097), "bins_x"), (dict(by=0), "bins_y"), (dict(by=4097), "bins_y"), (dict(by=-3), "bins_y"),
        (dict(bx=1025, by=1024), "2^20"), (dict(bx=4096, by=4096), "2^20"), (dict(path=3), "path"), (dict(path=-1), "path"),
    ]
    for override, word in cases:
        a = dict(T=100, C=4, ld=ld, cs=1, P=2, bx=100, by=100, path=0)
        a.update(override)
        counts, outside = guarded(20000, torch.int64, POISON_I), guarded(6, torch.int64, POISON_I)
        st = lib().tw_joint_histogram_path(buf.data_ptr(), a["T"], a["C"], a["ld"], a["cs"], pd.data_ptr(), a["P"], e.data_ptr(), a["bx"],
                                           e.data_ptr(), a["by"], counts[GUARD:].data_ptr(), outside[GUARD:].data_ptr(), a["path"], stream())
        torch.cuda.synchronize()
        assert st == -1 and "tw_joint_histogram" in last_error() and word in last_error(), (override, last_error())
        assert bool((counts == POISON_I).all()) and bool((outside == POISON_I).all()), override
    counts, outside = guarded(20000, torch.int64, POISON_I), guarded(6, torch.int64, POISON_I)
    ptrs = [buf.data_ptr(), pd.data_ptr(), e.data_ptr(), e.data_ptr(), counts[GUARD:].data_ptr(), outside[GUARD:].data_ptr()]
    for k in range(6):
        p = [None if i == k else v for i, v in enumerate(ptrs)]
        st = lib().tw_joint_histogram(p[0], 100, 4, ld, 1, p[1], 2, p[2], 100, p[3], 100, p[4], p[5], stream())
        torch.cuda.synchronize()
        assert st == -1 and "NULL" in last_error(), k
    assert bool((counts == POISON_I).all()) and bool((outside == POISON_I).all())
    # empty calls: valid, nothing launched, nothing written - pointers are not looked at
    pre = np.arange(2 * 100 * 100, dtype=np.int64)
    ex = jo.linspace_tables(LO, HI, 100, 2)
    for T, P in ((0, 2), (100, 0), (0, 0)):
        st, c, o, ok = raw_joint(buf, T, 4, ld, 1, pairs[:P], ex[:max(P, 1)], ex[:max(P, 1)], 100, 100, prefill=pre[:P * 10000])
        assert st == 0 and ok and (c.reshape(-1) == pre[:P * 10000]).all() and o.sum() == 0


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------

def same_joint(a, b):
    return all((getattr(a, f) == getattr(b, f)).all() for f in ("counts", "outside", "edges_x", "edges_y"))


def test_driver_routes_agree_on_the_device():
    from timewarp_amd import analysis, evaluate as ev

    X = torch.as_tensor(matrix(5000, 5, 100, seed=3, special=False)).to(dev())
    pairs = [[0, 1], [4, 2], [3, 3]]
    k = ev.joint_histograms(X, pairs, route="kernel")
    assert same_joint(k, ev.joint_histograms(X, pairs, route="torch")) and k.outside.sum() == 0 and (k.counts.sum(axis=(1, 2)) == 5000).all()
    assert same_joint(k, ev.joint_histograms(X.cpu().numpy(), pairs, route="kernel", chunk_rows=1234))
    assert same_joint(ev.joint_histograms(X, pairs, bins=(300, 127), route="kernel"), ev.joint_histograms(X, pairs, bins=(300, 127), route="torch"))
    Y = torch.as_tensor(np.random.default_rng(0).normal(size=(700, 9, 3)).astype(np.float32)).to(dev())
    assert same_joint(ev.joint_histograms(Y[:, :, 0], [[0, 8], [3, 4]], bins=(12, 127), route="kernel"),      # in place: ld 27, col_stride 3
                      ev.joint_histograms(Y[:, :, 0].contiguous(), [[0, 8], [3, 4]], bins=(12, 127), route="torch"))
    bad = X.clone()
    bad[17, 2] = float("nan")
    with pytest.raises(ValueError, match=r"column 2 holds 1 non-finite"):
        ev.joint_histograms(bad, pairs, route="kernel")
    h = ev.joint_histograms(bad, pairs, range=((LO, HI), (LO, HI)), route="kernel")
    assert h.outside[1, 2] == 1 and same_joint(h, ev.joint_histograms(bad, pairs, range=((LO, HI), (LO, HI)), route="torch"))
    rng = np.random.default_rng(10)
    phi = rng.uniform(-np.pi, np.pi, size=(3000, 3)).astype(np.float32)
    psi = rng.uniform(-np.pi, np.pi, size=(3000, 2)).astype(np.float32)
    phi[:4, 0] = [np.float32(np.pi), -np.float32(np.pi), 0.0, np.nan]
    rp = [(0, 0), (2, 1), (1, 0)]
    rk = analysis.ramachandran_histograms(torch.as_tensor(phi).to(dev()), torch.as_tensor(psi).to(dev()), rp, bins=50, route="kernel")
    assert same_joint(rk, analysis.ramachandran_histograms(phi, psi, rp, bins=50, route="torch")) and rk.outside.tolist()[0] == [0, 0, 1]
    p = float(np.float32(np.pi))
    assert (rk.counts[1] == jo.joint_counts(phi[:, 2], psi[:, 1], np.linspace(-p, p, 51), np.linspace(-p, p, 51))[0]).all()


def integer_fields(arrays):
    return {k: v for k, v in arrays.items() if np.asarray(v).dtype.kind in "iu"}


def test_tica_report_and_command_line_agree_with_the_torch_route(tmp_path):
    from tests.test_evaluate_cpu import cli_files
    from tests.test_joint_histogram_cpu import chain_inputs
    from timewarp_amd import evaluate as ev, tica_report as tr

    md, model, expl, tors = chain_inputs()
    reports = {r: tr.tica_report(md, model, exploration=expl, torsions=tors, lag=10, dim=3, bins=40, route=r, tica_route="kernel",
                                 chunk_rows=997).arrays() for r in ev.JOINT_ROUTES}
    ints = integer_fields(reports["torch"])
    assert {"md_tic01_counts", "model_tic01_outside", "exploration_projection_counts", "md_ramachandran_counts"} <= set(ints)
    for k, v in ints.items():
        assert np.array_equal(reports["kernel"][k], v), k
    for k in ("md_tic01_edges_x", "model_projection_edges", "md_tic0_series", "md_autocorrelation"):
        assert np.array_equal(reports["kernel"][k], reports["torch"][k]), k
    assert reports["kernel"]["md_tic01_counts"].sum() == len(md)
    # the command line on coordinates: the default route against the same report with torch histograms
    mdf, chain, pdb, z, frames, steps = cli_files(tmp_path)
    out = tr.main(["--md", mdf, "--model-dir", chain, "--protein", "nnqq", "--pdb", pdb, "--lag", "2", "--dim", "2", "--bins", "12",
                   "--out", str(tmp_path / "tica.npz")])
    back = ev.load_report(out)
    direct = tr.tica_report(z["positions"][:len(steps)], frames, topology=pdb, lag=2, dim=2, bins=12, route="torch", tica_route="kernel").arrays()
    assert set(integer_fields(direct)) <= set(back) and back["md_ramachandran_counts"].shape == (2, 12, 12)
    for k, v in integer_fields(direct).items():
        assert np.array_equal(back[k], v), k
