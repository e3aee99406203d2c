"""The analysis kernels (csrc/tw_analysis.hip behind `tw_dihedrals`, `tw_tica_features`, `tw_lagged_moments`) and their drivers in
timewarp_amd/analysis.py against the float64 restatement tests/analysis_oracle.py.

Tolerances are derived, not measured.  Angles, sines and cosines: the kernels work in fp64 and round once, so 2^-22 (one float32
ulp at pi) absolute; an angle within 2^-20 of +-pi is compared modulo 2 pi.  Distances: 2 float32 ulp of the value.  Moments:
products of float32 values are exact in fp64, so an entry differs from the restatement only by summation order, bounded by
N 2^-52 sum |x_i y_j| over the N pairs.

Shapes: alanine dipeptide (22 atoms), the 40 NNQQ frames (65 atoms, 64 rows per block), the 12 frames of 1hgv (691 atoms, 7 rows
per block); rows 1 / 65 / 257; moments F 1 .. 130 (one and two tiles per edge, scalar loads) and 260 (three tiles, vector
loads)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import analysis_oracle as ao
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

ANGLE_TOL = 2.0 ** -22
EPS64 = 2.0 ** -52


def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def molecule(name):
    """(float32 frames [n, V, 3], torsion tables by family, topology tuple)"""
    from timewarp_amd import analysis as an
    from timewarp_amd import forcefield as ffm

    if name == "ad":
        z = np.load(os.path.join(GOLDEN, "ad_topology.npz"))
        rid = {"ACE": 1, "ALA": 2, "NME": 3}
        topo = (list(z["atom_names"]), ffm.AD_RESIDUES, [rid[r] for r in ffm.AD_RESIDUES])
        rng = np.random.default_rng(5)
        frames = (z["coords_nm"][None] + 0.01 * rng.normal(size=(8, 22, 3))).astype(np.float32)
    else:
        z = np.load(os.path.join(GOLDEN, "energy_kat_2olx.npz" if name == "nnqq" else "energy_kat_1hgv.npz"))
        topo = (list(z["atom_names"]), list(z["residue_names"]), list(z["residue_ids"]))
        frames = np.ascontiguousarray(z["positions"], dtype=np.float32)
    return frames, an.torsion_indices(*topo), topo


def rows_of(frames, n_rows):
    return np.ascontiguousarray(frames[np.arange(n_rows) % len(frames)])


def all_quads(tables):
    from timewarp_amd.analysis import FAMILIES

    return np.concatenate([tables[f] for f in FAMILIES], axis=0)


def assert_angles(got, ref):
    d = np.abs(got.astype(np.float64) - ref)
    near_pi = np.abs(np.abs(ref) - np.pi) < 2.0 ** -20
    d = np.where(near_pi, np.minimum(d, np.abs(d - 2 * np.pi)), d)
    print("angle max |delta|", d.max() if d.size else 0.0, "tolerance", ANGLE_TOL)
    assert got.dtype == np.float32 and (d <= ANGLE_TOL).all(), d.max()
    assert (got > -np.pi - 1e-6).all() and (got <= np.float32(np.pi)).all()


# ---- tw_dihedrals -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_quads", [1, 7, "all"])
@pytest.mark.parametrize("n_rows", [1, 65, 257])
@pytest.mark.parametrize("mol", ["ad", "nnqq", "1hgv"])
def test_dihedrals_match_the_restatement(mol, n_rows, n_quads):
    from timewarp_amd import analysis as an

    frames, tables, _ = molecule(mol)
    quads = all_quads(tables)
    if n_quads != "all":
        if len(quads) < n_quads:        # alanine dipeptide has two torsions: fill up with other bonded-looking quads of its atoms
            extra = np.array([[1, 4, 6, 8], [8, 14, 16, 18], [5, 4, 6, 7], [10, 8, 14, 15], [0, 1, 4, 5]], dtype=np.int32)
            quads = np.concatenate([quads, extra], axis=0)
        quads = quads[np.linspace(0, len(quads) - 1, n_quads).astype(int)]
    x = rows_of(frames, n_rows)
    got = an.dihedrals(torch.as_tensor(x).to(dev()), quads).cpu().numpy()
    assert got.shape == (n_rows, len(quads))
    assert_angles(got, ao.dihedrals(x, quads))


def test_dihedrals_collinear_nan_and_neighbours():
    from timewarp_amd import analysis as an

    frames, tables, _ = molecule("nnqq")
    quads = all_quads(tables)
    x = rows_of(frames, 67)
    clean = an.dihedrals(torch.as_tensor(x).to(dev()), quads).cpu().numpy()
    # a collinear quad: four points on a line give atan2(0, 0) = 0
    line = np.zeros((3, 4, 3), dtype=np.float32)
    line[:, :, 0] = np.arange(4, dtype=np.float32) * 0.1
    out = an.dihedrals(torch.as_tensor(line).to(dev()), [[0, 1, 2, 3], [3, 2, 1, 0]]).cpu().numpy()
    assert (out == 0.0).all() and not np.signbit(out).any()
    # NaN in row 64 (the first row of the second block) and row 30: NaN there, the other rows bit for bit what they were
    for bad in (30, 64):
        y = x.copy()
        y[bad] = np.nan
        got = an.dihedrals(torch.as_tensor(y).to(dev()), quads).cpu().numpy()
        assert np.isnan(got[bad]).all()
        keep = np.arange(67) != bad
        assert (got[keep].view(np.uint32) == clean[keep].view(np.uint32)).all()
        # one non-finite atom: only the quads that read it
        y = x.copy()
        y[bad, quads[0, 0]] = np.inf
        got = an.dihedrals(torch.as_tensor(y).to(dev()), quads).cpu().numpy()
        touched = (quads == quads[0, 0]).any(axis=1)
        assert np.isnan(got[bad, touched]).all() and (got[bad, ~touched].view(np.uint32) == clean[bad, ~touched].view(np.uint32)).all()
        assert (got[[bad - 1, bad + 1]].view(np.uint32) == clean[[bad - 1, bad + 1]].view(np.uint32)).all()


def test_dihedrals_empty_calls_launch_nothing():
    from timewarp_amd import _lib
    from timewarp_amd import analysis as an

    frames, tables, _ = molecule("nnqq")
    x = torch.as_tensor(frames).to(dev())
    assert an.dihedrals(x, np.zeros((0, 4), dtype=np.int32)).shape == (40, 0)
    assert an.dihedrals(x[:0], tables["phi"]).shape == (0, 3)
    lib = _lib.load()
    s = _lib.stream_ptr(dev())
    assert lib.tw_dihedrals(None, None, 0, None, 5, 65, s) == 0 and lib.tw_dihedrals(None, None, 3, None, 0, 65, s) == 0
    assert lib.tw_dihedrals(x.data_ptr(), None, 3, None, 5, 65, s) == -1          # NULL where data is needed
    assert lib.tw_dihedrals(x.data_ptr(), x.data_ptr(), 3, x.data_ptr(), 5, 6000, s) == -1   # a row does not fit the LDS
    with pytest.raises(ValueError):
        an.dihedrals(x, [[0, 1, 2, 65]])
    torch.cuda.synchronize()


# ---- tw_tica_features ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_quads", [0, 1, 5])
@pytest.mark.parametrize("n_sel", [0, 1, 2, 3, 11])
def test_features_match_the_restatement(n_sel, n_quads):
    from timewarp_amd import analysis as an

    frames, tables, _ = molecule("nnqq")
    x = rows_of(frames, 65)
    sel = np.array([4, 0, 6, 16, 18, 20, 30, 32, 34, 47, 64], dtype=np.int32)[:n_sel]       # not sorted: the order is the caller's
    fam = [tables["phi"][: min(3, n_quads)], tables["chi1"][: n_quads - min(3, n_quads)]]     # two families: 1+0, 3+2
    fam = [f for f in fam if len(f)]
    quads = np.concatenate(fam, axis=0) if fam else np.zeros((0, 4), dtype=np.int32)
    cols, base = [], 0
    for f in fam:
        cols.append(np.stack([base + np.arange(len(f)), base + len(f) + np.arange(len(f))], axis=1))
        base += 2 * len(f)
    cols = np.concatenate(cols) if cols else np.zeros((0, 2), dtype=np.int32)
    got = an.features_from_tables(torch.as_tensor(x).to(dev()), sel, quads, cols).cpu().numpy()
    ref = ao.features(x, sel, fam)
    n_pairs = n_sel * (n_sel - 1) // 2
    assert got.shape == ref.shape == (65, n_pairs + 2 * n_quads) and got.dtype == np.float32
    if n_pairs:
        i, j = np.triu_indices(n_sel, k=1)
        d64 = np.linalg.norm(x[:, sel[i]].astype(np.float64) - x[:, sel[j]].astype(np.float64), axis=-1)
        assert np.abs(ref[:, :n_pairs] - d64).max() == 0.0 or np.abs(ref[:, :n_pairs] - d64).max() < 1e-15
        err = np.abs(got[:, :n_pairs] - d64)
        ulp = np.spacing(np.abs(d64).astype(np.float32)).astype(np.float64)
        print("distance max error / ulp", (err / ulp).max())
        assert (err <= 2 * ulp).all()
    if n_quads:
        err = np.abs(got[:, n_pairs:] - ref[:, n_pairs:])
        print("sin / cos max |delta|", err.max(), "tolerance", ANGLE_TOL)
        assert (err <= ANGLE_TOL).all()


def test_feature_column_order_family_by_family():
    """`tica_features` puts the families in the order phi, psi, omega, each as sines then cosines; one family at a time gives the
    same columns as the matching slice of the full vector."""
    from timewarp_amd import analysis as an

    frames, tables, topo = molecule("nnqq")
    x = torch.as_tensor(frames).to(dev())
    full = an.tica_features(x, topo).cpu().numpy()
    sel, quads, cols = an.feature_tables(topo)
    n_pairs = len(sel) * (len(sel) - 1) // 2
    assert full.shape == (40, n_pairs + 18)
    at = n_pairs
    for fam in ("phi", "psi", "omega"):
        n = len(tables[fam])
        one = an.features_from_tables(x, np.zeros(0, dtype=np.int32), tables[fam],
                                      np.stack([np.arange(n), n + np.arange(n)], axis=1)).cpu().numpy()
        assert (one.view(np.uint32) == full[:, at:at + 2 * n].view(np.uint32)).all(), fam
        a = ao.dihedrals(frames, tables[fam])
        assert np.abs(one - np.concatenate([np.sin(a), np.cos(a)], axis=1)).max() <= ANGLE_TOL
        at += 2 * n
    # distances only, and nothing at all
    assert (an.tica_features(x, topo, use_dihedrals=False).cpu().numpy().view(np.uint32) == full[:, :n_pairs].view(np.uint32)).all()
    assert an.tica_features(x, topo, use_dihedrals=False, use_distances=False).shape == (40, 0)
    # a collinear quad: sin 0, cos 1
    line = np.zeros((2, 4, 3), dtype=np.float32)
    line[:, :, 1] = np.arange(4, dtype=np.float32)
    sc = an.features_from_tables(torch.as_tensor(line).to(dev()), [], [[0, 1, 2, 3]], [[0, 1]]).cpu().numpy()
    assert (sc == np.array([[0.0, 1.0]] * 2, dtype=np.float32)).all()
    with pytest.raises(ValueError):
        an.features_from_tables(x, [0, 1], tables["phi"], [[0, 1], [2, 3], [4, 4]])     # not a permutation


# ---- tw_lagged_moments --------------------------------------------------------------------------------------------------------------

def raw_moments(X, lag, acc=None):
    """One tw_lagged_moments call on the device tensor X; (acc, count) accumulate when given."""
    from timewarp_amd import analysis as an

    if acc is None:
        acc = an.moments_accumulator(X.shape[-1], X.device)
    an.accumulate_moments(X, lag, *acc)
    return acc


def split_acc(acc, F):
    a = acc.cpu().numpy()
    FF = F * F
    return dict(sum_x=a[:F], sum_y=a[F:2 * F], c_xx=a[2 * F:2 * F + FF].reshape(F, F), c_xy=a[2 * F + FF:2 * F + 2 * FF].reshape(F, F),
                c_yy=a[2 * F + 2 * FF:].reshape(F, F))


def assert_moments(got, ref, what=""):
    n = ref["n_pairs"]
    worst = 0.0
    for key, bound_key in (("sum_x", "abs_x"), ("sum_y", "abs_y"), ("c_xx", "abs_xx"), ("c_xy", "abs_xy"), ("c_yy", "abs_yy")):
        err = np.abs(np.asarray(got[key]) - ref[key])
        bound = n * EPS64 * ref[bound_key]
        ok = err <= bound
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        assert ok.all(), (what, key, float(err.max()), np.argwhere(~ok)[:4].tolist())
    print(what, "worst error / bound", worst)


def make_X(n_chains, T, F, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n_chains, T, F)) + rng.normal(size=F)).astype(np.float32)


@pytest.mark.parametrize("n_chains", [1, 3])
@pytest.mark.parametrize("T,lag", [(200, 1), (200, 7), (200, 199), (2, 1), (8, 7)])
@pytest.mark.parametrize("F", [1, 63, 64, 65, 130])
def test_moments_match_the_restatement(F, T, lag, n_chains):
    X = make_X(n_chains, T, F, F + T + lag)
    acc, count, _ = raw_moments(torch.as_tensor(X).to(dev()), lag)
    ref = ao.lagged_moments(X, lag)
    assert int(count.item()) == ref["n_pairs"] == n_chains * (T - lag)
    assert_moments(split_acc(acc, F), ref, f"F {F} T {T} lag {lag} chains {n_chains}")


def test_moments_vector_path_three_tiles_and_reproducible():
    F, T, lag = 260, 96, 5
    X = make_X(2, T, F, 11)
    Xd = torch.as_tensor(X).to(dev())
    acc, count, _ = raw_moments(Xd, lag)
    assert_moments(split_acc(acc, F), ao.lagged_moments(X, lag), "F 260")
    got = split_acc(acc, F)
    assert (got["c_xx"] == got["c_xx"].T).all() and (got["c_yy"] == got["c_yy"].T).all()       # mirrored, bit for bit
    again, count2, _ = raw_moments(Xd.clone(), lag)
    assert torch.equal(acc.view(torch.int64), again.view(torch.int64)) and int(count2.item()) == int(count.item())
    # the scalar path (F 63) twice as well
    Y = torch.as_tensor(make_X(3, 200, 63, 12)).to(dev())
    a, _, _ = raw_moments(Y, 7)
    b, _, _ = raw_moments(Y, 7)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_moments_never_pair_across_chains():
    """A marker in the last `lag` frames of chain 0 and the first `lag` frames of chain 1: were a pair to cross the boundary, x y^T
    would hold marker x marker; as it is, no pair has the marker on both sides."""
    F, T, lag, big = 5, 40, 7, 1.0e6
    X = make_X(2, T, F, 13) * 0.0 + 1.0
    X[0, T - lag:, 0] = big
    X[1, :lag, 0] = big
    acc, count, _ = raw_moments(torch.as_tensor(X).to(dev()), lag)
    got = split_acc(acc, F)
    assert int(count.item()) == 2 * (T - lag)
    assert got["c_xy"][0, 0] < big * big          # (chain 0's y markers pair with x = 1, chain 1's x markers with y = 1)
    assert got["c_xy"][0, 0] == (T - lag - lag) * 2 * 1.0 + 2 * lag * big
    assert_moments(got, ao.lagged_moments(X, lag), "marker")


def test_moments_in_two_overlapping_halves():
    F, T, lag = 65, 200, 7
    X = make_X(3, T, F, 14)
    Xd = torch.as_tensor(X).to(dev())
    ref = ao.lagged_moments(X, lag)
    acc = raw_moments(Xd[:, : 100 + lag].contiguous(), lag)          # pairs whose first frame is 0 .. 99
    acc = raw_moments(Xd[:, 100:].contiguous(), lag, acc)           # ... 100 .. 192
    assert int(acc[1].item()) == ref["n_pairs"]
    assert_moments(split_acc(acc[0], F), ref, "two halves")


def test_moments_refuse_what_is_not_supported():
    from timewarp_amd import _lib

    lib = _lib.load()
    s = _lib.stream_ptr(dev())
    X = torch.zeros(1, 8, 4, device=dev())
    acc = torch.zeros(2 * 4 + 3 * 16, dtype=torch.float64, device=dev())
    ws = torch.empty(int(lib.tw_lagged_moments_workspace_len(4)), dtype=torch.float64, device=dev())
    call = lambda T, F, lag: lib.tw_lagged_moments(X.data_ptr(), 1, T, F, lag, acc.data_ptr(), None, ws.data_ptr(), s)
    assert call(8, 4, 8) == -1 and b"lag" in lib.tw_last_error()
    assert call(8, 4, 9) == -1 and call(8, 4, 0) == -1
    assert call(8, 1025, 1) == -1 and b"n_features" in lib.tw_last_error()
    assert lib.tw_lagged_moments_workspace_len(1025) == -1 and lib.tw_lagged_moments_workspace_len(0) == -1
    assert lib.tw_lagged_moments_workspace_len(1024) > 0
    assert call(8, 4, 7) == 0          # the largest lag that is supported; NULL pair count is allowed
    torch.cuda.synchronize()
    assert float(acc.abs().sum()) == 0.0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

def test_drivers_agree_on_device_and_numpy_input():
    from timewarp_amd import analysis as an

    frames, tables, topo = molecule("nnqq")
    coords = rows_of(frames, 200).reshape(2, 100, 65, 3)
    coords = coords + np.float32(1e-3) * np.random.default_rng(15).normal(size=coords.shape).astype(np.float32)
    cd = torch.as_tensor(coords).to(dev())
    t_dev, t_np = an.compute_torsions(cd, topo), an.compute_torsions(coords, topo)
    for fam in an.FAMILIES:
        a, b = getattr(t_dev, fam), getattr(t_np, fam)
        assert isinstance(a, torch.Tensor) and a.is_cuda and isinstance(b, np.ndarray)
        assert a.shape == (2, 100, len(tables[fam])) and a.dtype == torch.float32 and b.dtype == np.float32
        assert (a.cpu().numpy().view(np.uint32) == b.view(np.uint32)).all()
        assert (getattr(t_dev, fam + "_indices") == tables[fam]).all()
    assert_angles(t_np.chi2.reshape(200, -1), ao.dihedrals(coords.reshape(200, 65, 3), tables["chi2"]))
    m_dev = an.lagged_moments(cd, 7, topology=topo, route="kernel")
    m_np = an.lagged_moments(coords, 7, topology=topo, route="kernel")
    assert m_dev.n_pairs == m_np.n_pairs == 2 * 93 and isinstance(m_np.c_xy, np.ndarray) and m_dev.c_xy.is_cuda
    for key in ("sum_x", "sum_y", "c_xx", "c_xy", "c_yy"):
        assert (getattr(m_dev, key).cpu().numpy() == getattr(m_np, key)).all(), key


def test_chunked_moments_agree_with_unchunked():
    from timewarp_amd import analysis as an

    frames, _, topo = molecule("nnqq")
    coords = rows_of(frames, 200).reshape(1, 200, 65, 3)
    coords = coords + np.float32(1e-3) * np.random.default_rng(16).normal(size=coords.shape).astype(np.float32)
    cd = torch.as_tensor(coords).to(dev())
    feats = an.tica_features(cd, topo)
    ref = ao.lagged_moments(feats.cpu().numpy(), 7)
    whole = an.lagged_moments(cd, 7, chunk_frames=1 << 20, topology=topo, route="kernel")
    chunked = an.lagged_moments(cd, 7, chunk_frames=64, topology=topo, route="kernel")
    from_features = an.lagged_moments(feats, 7, chunk_frames=64, route="kernel")
    via_torch = an.lagged_moments(feats, 7, chunk_frames=64, route="torch")
    for m, what in ((whole, "whole"), (chunked, "chunks of 64"), (from_features, "features, chunks of 64"), (via_torch, "torch route")):
        assert m.n_pairs == 193, what
        assert_moments({k: getattr(m, k).cpu().numpy() for k in ("sum_x", "sum_y", "c_xx", "c_xy", "c_yy")}, ref, what)
    ev, proj, mean = an.tica_from_moments(whole, 3)
    assert ev.shape == (3,) and proj.shape[0] == feats.shape[-1] and bool((ev[:-1] >= ev[1:]).all()) and float(ev[0]) <= 1.0 + 1e-6
