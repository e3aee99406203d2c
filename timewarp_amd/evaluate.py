"""The evaluation report of the reference's evaluate.py on the device: internal coordinates and the histograms behind its figures.

    python -m timewarp_amd.evaluate --md TRAJ-traj-arrays.npz --model-dir DIR --protein NAME --pdb STATE0.pdb
                                    [--force-field NAME --bins 100 --stride 1 --chunk-frames N --step-width 1 --route R --out FILE]

What stands in for what (the reference computes all of this on the host with mdtraj, matplotlib and OpenMM, which this package does
not use; there are no plots here - the report holds the data behind each figure):

  `pair_distances`                  mdtraj's compute_distances without a unit cell (utils/evaluation_utils.py:752)
  `compute_internal_coordinates`    utils/evaluation_utils.py:749-759: (bonds, (phi, psi))
  `column_histograms`, `Histograms` plt.hist(x, bins=100[, range=...][, density=True]) of every column at once
                                    (plot_marginal_distribution :765-885, plot_energy :1056-1085, evaluate.py:449-484)
  `pair_histograms`                 plot_bonds (:888-996): the bond-length distributions, without the [T, n_bonds] array
  `joint_histograms`, `JointHistograms`  plt.hist2d(x, y, bins=100) of every pair of columns at once (utils/tica_utils.py:49, the
                                    Ramachandran panels): counts, edges and what fell outside; `tw_joint_histogram`
  `trajectory_pairs`                dataloader.py:213-276 (`load_pdb_trace_data`): conditioning / target pairs of an arrays.npz
  `conditional_md_samples`          the MD half of sample_on_single_conditional (utils/evaluation_utils.py:356-413), without OpenMM
  `evaluation_report`               evaluate.py:328-856: bonds, Delta x and velocity marginals, Ramachandran counts, psi transitions
                                    (plot_transitions :1040-1053), energies, the Delta x correlation matrices (evaluate.py:398-399,
                                    :436), likelihood histograms (evaluate.py:449-484)
  the command line                  the "sample on samples" section, evaluate.py:775-855, at chain scale

Hot paths are HIP kernels (csrc/tw_evaluate.hip: `tw_pair_distances`, `tw_column_range`, `tw_column_histogram`, `tw_pair_range`,
`tw_pair_histogram`, `tw_joint_histogram`); the "torch" route restates them with torch ops, runs without a GPU and is the comparison of
profiles/evaluate.txt.  One bin rule holds on every route (include/timewarp_hip.h): float32 values as fp64 against fp64 edges,
e[i] <= x < e[i+1], the last bin closed, values below / above / NaN counted apart - with np.linspace edges exactly np.histogram's
counts.  Nothing here claims equality with mdtraj's or OpenMM's output: neither is available to compare against.
"""
from __future__ import annotations

import argparse
import dataclasses
import os
import warnings
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, analysis

# The routes.  "kernel": tw_column_range + tw_column_histogram (for pairs: on tw_pair_distances' output).  "fused" (pairs only):
# tw_pair_range + tw_pair_histogram, the distances computed on the fly and never stored.  "torch": torch.searchsorted (the batched
# torch.bucketize) on the same fp64 edges + torch.bincount - same semantics, runs without a GPU.  The defaults are the routes that
# measured fastest on the MI355X at the sizes of profiles/evaluate.txt.
COLUMN_ROUTES = ("kernel", "torch")
PAIR_ROUTES = ("fused", "kernel", "torch")
DEFAULT_COLUMN_ROUTE = "kernel"
DEFAULT_PAIR_ROUTE = "fused"
MAX_BINS = 4096
MAX_ROWS_PER_CALL = 1 << 31          # rows of one kernel call here (the library takes fewer than 2^32); longer inputs are chunked
DEFAULT_CHUNK_ROWS = 1 << 22


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------

def _need_gpu(what: str) -> None:
    if not torch.cuda.is_available():
        raise RuntimeError(f"timewarp_amd.evaluate: {what} runs on an MI355X; no GPU is visible and there is no CPU fallback "
                           "(route='torch' is the restatement)")


def _route(route: Optional[str], routes: Tuple[str, ...], default: str) -> str:
    route = default if route is None else route
    if route not in routes:
        raise ValueError(f"route {route!r}: one of {routes}")
    return route


def _place(x, route: str) -> torch.Tensor:
    """A float32 tensor where `route` computes: numpy goes to the device when there is one (always for a kernel route)."""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x, dtype=np.float32))
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    if route != "torch":
        _need_gpu(f"route {route!r}")
    if not x.is_cuda and torch.cuda.is_available():
        x = x.to("cuda")
    return x


def _strided_2d(X: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
    """(tensor, ld, col_stride) of a 2-D float32 view the kernels can read in place; a view they cannot (a transposed one, say) is
    copied."""
    if X.dim() != 2:
        raise ValueError(f"expected a 2-D matrix [rows, columns], got {tuple(X.shape)}")
    T, C = X.shape
    ld, cs = (X.stride(0), X.stride(1)) if T > 0 and C > 0 else (max(C, 1), 1)
    if C == 1 and cs < 1:
        cs = 1
    if T == 1 and ld < (C - 1) * cs + 1:
        ld = (C - 1) * cs + 1
    if cs < 1 or ld < (C - 1) * cs + 1:
        X = X.contiguous()
        ld, cs = max(C, 1), 1
    return X, int(ld), int(cs)


def _pairs_table(pairs, n_atoms: int) -> np.ndarray:
    p = np.asarray(pairs)
    if p.ndim != 2 or p.shape[1] != 2:
        if p.size:
            raise ValueError(f"pairs: expected [n_pairs, 2], got {p.shape}")
        p = p.reshape(0, 2)
    return analysis.check_indices(p, n_atoms, "pairs").reshape(-1, 2)


def _coords_3d(coords, route: str) -> torch.Tensor:
    x = _place(coords, route)
    if x.dim() < 3 or x.shape[-1] != 3:
        raise ValueError(f"coords: expected [..., n_atoms, 3], got {tuple(x.shape)}")
    return x.reshape(-1, x.shape[-2], 3).contiguous()


def _row_chunks(n_rows: int, chunk_rows: Optional[int]):
    step = min(int(chunk_rows or DEFAULT_CHUNK_ROWS), MAX_ROWS_PER_CALL)
    if step < 1:
        raise ValueError("chunk_rows must be positive")
    return [(a, min(a + step, n_rows)) for a in range(0, n_rows, step)]


# ---- distances -----------------------------------------------------------------------------------------------------------------------

def _pair_distances_torch(x: torch.Tensor, pairs: np.ndarray) -> torch.Tensor:
    """`tw_pair_distances`' arithmetic with torch ops: fp64 differences, squares summed in k order, sqrt, one rounding to float32.
    The sum is not fused (torch has no fma), so a value can differ from the kernel's in its last fp64 bit, which changes the float32
    only when it lies within 2^-29 ulp of a rounding boundary."""
    idx = torch.as_tensor(pairs.astype(np.int64), device=x.device)
    t = x[:, idx[:, 0]].double() - x[:, idx[:, 1]].double()
    d2 = t[..., 0] * t[..., 0]
    d2 = d2 + t[..., 1] * t[..., 1]
    d2 = d2 + t[..., 2] * t[..., 2]
    return torch.sqrt(d2).to(torch.float32)


def pair_distances(coords, pairs, route: str = "kernel"):
    """Distances [n_rows, n_pairs] float32 of the atom pairs `pairs` [n_pairs, 2] in every row of coords [..., n_atoms, 3]
    (`tw_pair_distances`: fp64 from the float32 coordinates, one rounding; include/timewarp_hip.h states the order).  A device tensor
    for a tensor, numpy for numpy.  route="torch" is the restatement."""
    route = _route(route, COLUMN_ROUTES, "kernel")
    was_numpy = not isinstance(coords, torch.Tensor)
    x = _coords_3d(coords, route)
    n_rows, n_atoms = int(x.shape[0]), int(x.shape[1])
    p = _pairs_table(pairs, n_atoms)
    if route == "torch":
        out = _pair_distances_torch(x, p)
    else:
        out = torch.empty((n_rows, len(p)), dtype=torch.float32, device=x.device)
        if n_rows and len(p):
            pd = torch.as_tensor(p).to(x.device)
            with torch.cuda.device(x.device):
                _lib.check(_lib.load().tw_pair_distances(x.data_ptr(), pd.data_ptr(), len(p), out.data_ptr(), n_rows, n_atoms,
                                                         _lib.stream_ptr(x.device)), "tw_pair_distances")
    return out.cpu().numpy() if was_numpy else out


def compute_internal_coordinates(topology, adj_list, coords):
    """utils/evaluation_utils.py:749-759 on the device: (bonds [T, n_bonds], (phi [T, n_phi], psi [T, n_psi])) float32 of coords
    [T, V, 3] - the lengths of the bonds `adj_list` [n_bonds, 2] (`pair_distances`) and the backbone torsions
    (`analysis.torsion_indices` + `analysis.dihedrals`).  `topology`: whatever `analysis._topology` accepts (a PDB path, a mapping
    with atom_names / residue_names / residue_ids, or that tuple).  Device tensors for a tensor, numpy for numpy."""
    was_numpy = not isinstance(coords, torch.Tensor)
    x = _coords_3d(coords, "kernel")
    tables = analysis.torsion_indices(*analysis._topology(topology))
    bonds = pair_distances(x, adj_list)
    n_phi = len(tables["phi"])
    ang = analysis.dihedrals(x, np.concatenate([tables["phi"], tables["psi"]], axis=0))
    phi, psi = ang[:, :n_phi].contiguous(), ang[:, n_phi:].contiguous()
    if was_numpy:
        return bonds.cpu().numpy(), (phi.cpu().numpy(), psi.cpu().numpy())
    return bonds, (phi, psi)


# ---- histograms ----------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Histograms:
    """Per-column histograms (numpy): counts int64 [C, B], edges fp64 [C, B + 1], and per column the rows below edges[:, 0], above
    edges[:, -1] and NaN - each row of the input is in exactly one of the four.  Totals are exact while they stay below 2^63."""

    counts: np.ndarray
    edges: np.ndarray
    below: np.ndarray
    above: np.ndarray
    nonfinite: np.ndarray

    def density(self) -> np.ndarray:
        """numpy's density=True per column: counts / (counts.sum() widths), fp64 [C, B] (NaN for a column without counts)."""
        widths = np.diff(self.edges, axis=1)
        total = self.counts.sum(axis=1, keepdims=True).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.counts / total / widths


def linspace_edges(lo, hi, bins: int) -> np.ndarray:
    """edges [C, bins + 1] fp64: np.linspace(lo[c], hi[c], bins + 1) per column, after numpy's rule for an empty range (lo == hi is
    widened to lo - 0.5, hi + 0.5).  A range that is not finite or has lo > hi is refused as numpy refuses it."""
    lo, hi = np.atleast_1d(np.asarray(lo, dtype=np.float64)), np.atleast_1d(np.asarray(hi, dtype=np.float64))
    if lo.shape != hi.shape or lo.ndim != 1:
        raise ValueError("range: one (lo, hi) per column")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        bad = int(np.flatnonzero(~(np.isfinite(lo) & np.isfinite(hi)))[0])
        raise ValueError(f"range of column {bad}: ({lo[bad]}, {hi[bad]}) is not finite")
    if (lo > hi).any():
        bad = int(np.flatnonzero(lo > hi)[0])
        raise ValueError(f"range of column {bad}: max must be larger than min, got ({lo[bad]}, {hi[bad]})")
    same = lo == hi
    lo, hi = np.where(same, lo - 0.5, lo), np.where(same, hi + 0.5, hi)
    # one call for all columns: element for element the operations of the scalar call, unless a column's step underflows to zero
    # (numpy then takes another branch for the whole array) - such columns are done one by one
    with np.errstate(all="ignore"):
        step = (hi - lo) / bins
    if len(lo) and not (step == 0).any():
        return np.ascontiguousarray(np.linspace(lo, hi, bins + 1, axis=-1))
    out = np.empty((len(lo), bins + 1), dtype=np.float64)
    for c in range(len(lo)):
        out[c] = np.linspace(lo[c], hi[c], bins + 1)
    return out


def _check_bins(bins: int) -> int:
    bins = int(bins)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"bins {bins}: 1 .. {MAX_BINS}")
    return bins


def check_edges(edges, n_cols: int, bins: int) -> np.ndarray:
    """A caller's edge table as the contiguous fp64 [n_cols, bins + 1] array the kernels read, after the checks the library cannot
    make (it does not read device arrays on the host): the shape, finite entries, strictly increasing rows - each refused by name."""
    e = np.ascontiguousarray(edges, dtype=np.float64)
    if e.shape != (n_cols, bins + 1):
        raise ValueError(f"edges {e.shape}: expected [n_cols, bins + 1] = {(n_cols, bins + 1)}")
    if not np.isfinite(e).all():
        c = int(np.flatnonzero(~np.isfinite(e).all(axis=1))[0])
        raise ValueError(f"edges of column {c} hold non-finite entries")
    if e.size and not (np.diff(e, axis=1) > 0).all():
        c = int(np.flatnonzero(~(np.diff(e, axis=1) > 0).all(axis=1))[0])
        raise ValueError(f"edges of column {c} are not strictly increasing")
    return e


def _range_torch(X: torch.Tensor):
    finite = torch.isfinite(X)
    inf = torch.tensor(float("inf"), dtype=X.dtype, device=X.device)
    lo = torch.where(finite, X, inf).amin(dim=0) if X.shape[0] else inf.expand(X.shape[1])
    hi = torch.where(finite, X, -inf).amax(dim=0) if X.shape[0] else (-inf).expand(X.shape[1])
    return lo, hi, (~finite).sum(dim=0)


def _histogram_torch(X: torch.Tensor, edges: torch.Tensor, counts: torch.Tensor, outside: torch.Tensor) -> None:
    """The bin rule with torch ops, ADDED into counts [C, B] / outside [C, 3]: a [C, T] int64 index, then one bincount."""
    C, B = counts.shape
    if X.shape[0] == 0 or C == 0:
        return
    x = X.double().T.contiguous()                                        # [C, T]
    e0, eN = edges[:, :1], edges[:, -1:]
    nan = torch.isnan(x)
    below, above = x < e0, x > eN
    inside = ~(nan | below | above)
    idx = torch.searchsorted(edges, torch.where(inside, x, e0), right=True) - 1      # e[i] <= x < e[i+1]
    idx = idx.clamp_(0, B - 1)                                           # x == e[B]: the closed last bin
    flat = (idx + torch.arange(C, device=x.device)[:, None] * B)[inside]
    counts += torch.bincount(flat, minlength=C * B).reshape(C, B)
    outside[:, 0] += below.sum(dim=1)
    outside[:, 1] += above.sum(dim=1)
    outside[:, 2] += nan.sum(dim=1)


class _Columns:
    """The columns of one chunk of rows: a strided float32 matrix, or the distances of `pairs` in coords (route "fused": never
    stored; "kernel" / "torch": materialised for the chunk)."""

    def __init__(self, route: str, X=None, coords=None, pairs: Optional[np.ndarray] = None):
        self.route = route
        if coords is not None:
            self.n_cols = len(pairs)
            self.coords = coords
            self.pairs = pairs
            self.pairs_dev = torch.as_tensor(pairs).to(coords.device) if route != "torch" and len(pairs) else None
            self.X = None
            if route == "torch":
                self.X = _pair_distances_torch(coords, pairs)
            elif route == "kernel":
                self.X = pair_distances(coords, pairs)
            self.device, self.n_rows = coords.device, int(coords.shape[0])
        else:
            self.coords = None
            self.X = X
            self.n_cols, self.device, self.n_rows = int(X.shape[1]), X.device, int(X.shape[0])

    def ranges(self):
        """(lo [C] float32, hi [C] float32, nonfinite [C] int64) tensors over the finite entries of this chunk."""
        C = self.n_cols
        if self.route == "torch":
            return _range_torch(self.X)
        lo = torch.full((C,), float("inf"), dtype=torch.float32, device=self.device)
        hi = torch.full((C,), float("-inf"), dtype=torch.float32, device=self.device)
        nf = torch.zeros(C, dtype=torch.int64, device=self.device)
        if C and self.n_rows:
            lib = _lib.load()
            with torch.cuda.device(self.device):
                if self.X is None:
                    _lib.check(lib.tw_pair_range(self.coords.data_ptr(), self.pairs_dev.data_ptr(), C, self.n_rows,
                                                 int(self.coords.shape[1]), lo.data_ptr(), hi.data_ptr(), nf.data_ptr(),
                                                 _lib.stream_ptr(self.device)), "tw_pair_range")
                else:
                    X, ld, cs = _strided_2d(self.X)
                    _lib.check(lib.tw_column_range(X.data_ptr(), self.n_rows, C, ld, cs, lo.data_ptr(), hi.data_ptr(), nf.data_ptr(),
                                                   _lib.stream_ptr(self.device)), "tw_column_range")
        return lo, hi, nf

    def add_histogram(self, edges: torch.Tensor, counts: torch.Tensor, outside: torch.Tensor) -> None:
        C, B = counts.shape
        if self.route == "torch":
            return _histogram_torch(self.X, edges, counts, outside)
        if not (C and self.n_rows):
            return
        lib = _lib.load()
        with torch.cuda.device(self.device):
            if self.X is None:
                _lib.check(lib.tw_pair_histogram(self.coords.data_ptr(), self.pairs_dev.data_ptr(), C, self.n_rows,
                                                 int(self.coords.shape[1]), edges.data_ptr(), B, counts.data_ptr(), outside.data_ptr(),
                                                 _lib.stream_ptr(self.device)), "tw_pair_histogram")
            else:
                X, ld, cs = _strided_2d(self.X)
                _lib.check(lib.tw_column_histogram(X.data_ptr(), self.n_rows, C, ld, cs, edges.data_ptr(), B, counts.data_ptr(),
                                                   outside.data_ptr(), _lib.stream_ptr(self.device)), "tw_column_histogram")


def _ranges_over(chunks, n_cols: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(lo, hi fp64 [C], nonfinite int64 [C]) over an iterable of `_Columns` (the minimum of the chunks' minima, ...); +inf / -inf
    and 0 when there is no chunk."""
    lo = hi = nf = None
    for ch in chunks:
        l, h, n = ch.ranges()
        lo, hi, nf = (l, h, n) if lo is None else (torch.minimum(lo, l), torch.maximum(hi, h), nf + n)
    if lo is None:
        return np.full(n_cols, np.inf), np.full(n_cols, -np.inf), np.zeros(n_cols, dtype=np.int64)
    return lo.double().cpu().numpy(), hi.double().cpu().numpy(), nf.cpu().numpy().astype(np.int64)


def _auto_range(lo: np.ndarray, hi: np.ndarray, nf: np.ndarray, what: str) -> Tuple[np.ndarray, np.ndarray]:
    """numpy's range=None per column from the read-back ranges: refuses a column with non-finite values (numpy: "autodetected range
    of [nan, nan] is not finite"), an empty column is (0, 1)."""
    if (nf > 0).any():
        c = int(np.flatnonzero(nf > 0)[0])
        raise ValueError(f"{what}: column {c} holds {int(nf[c])} non-finite value(s): the autodetected range is not finite "
                         "(pass range=(lo, hi) to count them apart)")
    empty = lo > hi                       # +inf / -inf: no rows
    return np.where(empty, 0.0, lo), np.where(empty, 1.0, hi)


def _explicit_range(range_, n_cols: int) -> Tuple[np.ndarray, np.ndarray]:
    lo, hi = range_
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return np.broadcast_to(lo, (n_cols,)).copy(), np.broadcast_to(hi, (n_cols,)).copy()


def _histograms_over(make_chunks, n_cols: int, bins: int, range_, device, what: str, edges: Optional[np.ndarray] = None) -> Histograms:
    """Range pass (only for range=None), edges on the host, then the accumulating histogram calls over the same chunks.
    `make_chunks()` yields the `_Columns` of consecutive row chunks, afresh each time it is called."""
    if edges is None:
        if range_ is None:
            lo, hi, nf = _ranges_over(make_chunks(), n_cols)
            lo, hi = _auto_range(lo, hi, nf, what)
        else:
            lo, hi = _explicit_range(range_, n_cols)
        edges = linspace_edges(lo, hi, bins)
    else:
        edges = check_edges(edges, n_cols, bins)
    counts = torch.zeros((n_cols, bins), dtype=torch.int64, device=device)
    outside = torch.zeros((n_cols, 3), dtype=torch.int64, device=device)
    e = torch.as_tensor(edges).to(device)
    for ch in make_chunks():
        ch.add_histogram(e, counts, outside)
    out = outside.cpu().numpy()
    return Histograms(counts.cpu().numpy(), edges, out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy())


def column_histograms(X, bins: int = 100, range=None, route: Optional[str] = None, chunk_rows: Optional[int] = None,
                      edges: Optional[np.ndarray] = None) -> Histograms:
    """`np.histogram(X[:, c].astype(np.float64), bins, range)` of every column c of X [T, C] float32 at once.

    X is a device tensor - any 2-D float32 view whose strides are (ld, col_stride) with col_stride >= 1 and
    ld >= (C - 1) col_stride + 1 is read in place: `coords[:, :, 0]` of a contiguous [T, V, 3] tensor is such a view (ld = 3 V,
    col_stride = 3) - or numpy, which goes to the device `chunk_rows` rows at a time.  range=None is numpy's rule per column: the
    column's own minimum and maximum (`tw_column_range`), widened by +-0.5 when they are equal; a column that holds non-finite values
    raises ValueError naming the column and their number, where numpy raises for an infinite autodetected range.  range=(lo, hi),
    scalars or per-column arrays, is used as given (and widened the same way when lo == hi).  The edges are np.linspace on the host
    from the read-back ranges, a few KB; `edges` [C, bins + 1] replaces them (any finite, strictly increasing table: `check_edges`
    converts it to contiguous fp64 and refuses another shape, non-finite entries and rows that do not increase).  `route`: COLUMN_ROUTES."""
    route = _route(route, COLUMN_ROUTES, DEFAULT_COLUMN_ROUTE)
    bins = _check_bins(bins)
    if len(X.shape) != 2:
        raise ValueError(f"X: expected [rows, columns], got {tuple(X.shape)}")
    T, C = int(X.shape[0]), int(X.shape[1])
    spans = _row_chunks(T, chunk_rows)
    probe = _place(X[:0], route)

    def chunks():
        for a, b in spans:
            yield _Columns(route, X=_place(X[a:b], route))

    return _histograms_over(chunks, C, bins, range, probe.device, "column_histograms", edges)


def pair_histograms(coords, pairs, bins: int = 100, range=None, route: Optional[str] = None, chunk_rows: Optional[int] = None,
                    edges: Optional[np.ndarray] = None) -> Histograms:
    """`column_histograms` of `pair_distances(coords, pairs)` - with route "fused" (`tw_pair_range` + `tw_pair_histogram`) without
    that [T, n_pairs] array: the distances are computed where they are binned, by the function `tw_pair_distances` stores with, so
    the counts are the same on every kernel route.  coords [T, V, 3] float32, a device tensor or numpy (uploaded `chunk_rows` rows
    at a time).  `route`: PAIR_ROUTES."""
    route = _route(route, PAIR_ROUTES, DEFAULT_PAIR_ROUTE)
    bins = _check_bins(bins)
    if len(coords.shape) != 3 or coords.shape[-1] != 3:
        raise ValueError(f"coords: expected [T, n_atoms, 3], got {tuple(coords.shape)}")
    T, V = int(coords.shape[0]), int(coords.shape[1])
    p = _pairs_table(pairs, V)
    spans = _row_chunks(T, chunk_rows)
    probe = _place(coords[:0], route)

    def chunks():
        for a, b in spans:
            yield _Columns(route, coords=_coords_3d(coords[a:b], route), pairs=p)

    return _histograms_over(chunks, len(p), bins, range, probe.device, "pair_histograms", edges)


# ---- joint histograms ----------------------------------------------------------------------------------------------------------------

# "kernel": tw_joint_histogram (ranges from tw_column_range).  "torch": torch.searchsorted on the same two fp64 tables per pair +
# one torch.bincount over the flat (pair, i, j) index - same semantics, runs without a GPU.  The default is the route that measured
# faster on the MI355X at the notebooks' sizes (profiles/joint_histogram.txt).
JOINT_ROUTES = ("kernel", "torch")
DEFAULT_JOINT_ROUTE = "kernel"
MAX_JOINT_PLANE = 1 << 20


@dataclasses.dataclass
class JointHistograms:
    """Joint histograms of P column pairs (numpy): counts int64 [P, bx, by] (first axis x), edges_x fp64 [P, bx + 1], edges_y fp64
    [P, by + 1] and outside int64 [P, 3] - the rows whose x lies outside edges_x (neither coordinate NaN), whose x lies inside and y
    outside edges_y, and with a NaN in either coordinate.  Every row of the input is in exactly one counter of each pair."""

    counts: np.ndarray
    outside: np.ndarray
    edges_x: np.ndarray
    edges_y: np.ndarray

    def density(self) -> np.ndarray:
        """np.histogram2d(..., density=True) per pair, fp64 [P, bx, by], in numpy's order of operations (the counts over the x
        widths, over the y widths, over the total), so the values are numpy's bit for bit; NaN for a pair without counts."""
        h = self.counts.astype(np.float64)
        total = h.sum(axis=(1, 2), keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            h = h / np.diff(self.edges_x, axis=1)[:, :, None]
            h = h / np.diff(self.edges_y, axis=1)[:, None, :]
            return h / total

    def marginal_x(self) -> np.ndarray:
        """int64 [P, bx]: the counts summed over y - the 1-D histogram of x over the rows whose y is inside its table."""
        return self.counts.sum(axis=2)

    def marginal_y(self) -> np.ndarray:
        return self.counts.sum(axis=1)

    def free_energy(self) -> np.ndarray:
        """-log(h / h.max()) per pair (utils/tica_utils.py:59-61 on the plane), fp64 [P, bx, by]; +inf in empty bins, NaN for a
        pair without counts."""
        h = self.counts.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return -np.log(h / h.max(axis=(1, 2), keepdims=True)) if h.size else h


def _check_bins_2d(bins) -> Tuple[int, int]:
    bx, by = (bins, bins) if np.isscalar(bins) else tuple(bins)
    bx, by = _check_bins(bx), _check_bins(by)
    if bx * by > MAX_JOINT_PLANE:
        raise ValueError(f"bins {(bx, by)}: a plane holds at most 2^20 bins")
    return bx, by


def _joint_histogram_torch(X: torch.Tensor, pairs: np.ndarray, ex: torch.Tensor, ey: torch.Tensor, counts: torch.Tensor,
                           outside: torch.Tensor) -> None:
    """`tw_joint_histogram` with torch ops, ADDED into counts [P, bx, by] / outside [P, 3]."""
    P, bx, by = counts.shape
    if X.shape[0] == 0 or P == 0:
        return
    idx = torch.as_tensor(pairs.astype(np.int64), device=X.device)
    x, y = X[:, idx[:, 0]].double().T.contiguous(), X[:, idx[:, 1]].double().T.contiguous()          # [P, T]
    nan = torch.isnan(x) | torch.isnan(y)
    x_out = ~nan & ((x < ex[:, :1]) | (x > ex[:, -1:]))
    y_out = ~nan & ~x_out & ((y < ey[:, :1]) | (y > ey[:, -1:]))
    inside = ~(nan | x_out | y_out)
    ix = (torch.searchsorted(ex, torch.where(inside, x, ex[:, :1]), right=True) - 1).clamp_(0, bx - 1)
    iy = (torch.searchsorted(ey, torch.where(inside, y, ey[:, :1]), right=True) - 1).clamp_(0, by - 1)
    flat = ((torch.arange(P, device=X.device)[:, None] * bx + ix) * by + iy)[inside]
    counts += torch.bincount(flat, minlength=P * bx * by).reshape(P, bx, by)
    outside[:, 0] += x_out.sum(dim=1)
    outside[:, 1] += y_out.sum(dim=1)
    outside[:, 2] += nan.sum(dim=1)


def _joint_histogram_kernel(X: torch.Tensor, pairs_dev: torch.Tensor, ex: torch.Tensor, ey: torch.Tensor, counts: torch.Tensor,
                            outside: torch.Tensor, path: int = _lib.TW_JOINT_PATH_AUTO) -> None:
    P, bx, by = counts.shape
    T, C = int(X.shape[0]), int(X.shape[1])
    if not (T and P):
        return
    X, ld, cs = _strided_2d(X)
    with torch.cuda.device(X.device):
        _lib.check(_lib.load().tw_joint_histogram_path(X.data_ptr(), T, C, ld, cs, pairs_dev.data_ptr(), P, ex.data_ptr(), bx,
                                                       ey.data_ptr(), by, counts.data_ptr(), outside.data_ptr(), path,
                                                       _lib.stream_ptr(X.device)), "tw_joint_histogram")


def joint_histograms(X, pairs, bins=100, range=None, route: Optional[str] = None, chunk_rows: Optional[int] = None,
                     edges=None) -> JointHistograms:
    """`np.histogram2d(X[:, i].astype(np.float64), X[:, j].astype(np.float64), bins, range)[0]` of every pair (i, j) of `pairs`
    [P, 2] at once (`tw_joint_histogram`): the hist2d of the reference's TICA and Ramachandran figures.

    X [T, C] float32 as for `column_histograms` (a strided device view is read in place, numpy goes to the device `chunk_rows`
    rows at a time; the chunks accumulate).  `pairs` is checked here: [P, 2], entries in 0 .. C - 1; a pair may name one column
    twice and pairs may repeat.  `bins`: an int or (bx, by), each 1 .. MAX_BINS, bx by <= 2^20.  range=None is numpy's rule per
    axis and pair: the column's own minimum and maximum (`tw_column_range`, torch on the torch route), an empty range widened by
    +-0.5; a column that some pair names and that holds non-finite values raises ValueError naming it.  range=((x_lo, x_hi),
    (y_lo, y_hi)), scalars or per-pair arrays, is used as given.  edges=(edges_x [P, bx + 1], edges_y [P, by + 1]) replaces the
    np.linspace tables (`check_edges`).  `route`: JOINT_ROUTES."""
    route = _route(route, JOINT_ROUTES, DEFAULT_JOINT_ROUTE)
    bx, by = _check_bins_2d(bins)
    if len(X.shape) != 2:
        raise ValueError(f"X: expected [rows, columns], got {tuple(X.shape)}")
    T, C = int(X.shape[0]), int(X.shape[1])
    p = _pairs_table(pairs, C)
    P = len(p)
    spans = _row_chunks(T, chunk_rows)
    device = _place(X[:0], route).device
    if edges is not None:
        ex, ey = edges
        ex, ey = check_edges(ex, P, bx), check_edges(ey, P, by)
    elif range is not None:
        rx, ry = range
        ex, ey = linspace_edges(*_explicit_range(rx, P), bx), linspace_edges(*_explicit_range(ry, P), by)
    else:
        lo, hi, nf = _ranges_over((_Columns(route, X=_place(X[a:b], route)) for a, b in spans), C)
        named = np.zeros(C, dtype=bool)
        named[p.reshape(-1)] = True
        lo, hi = _auto_range(lo, hi, np.where(named, nf, 0), "joint_histograms")
        ex, ey = linspace_edges(lo[p[:, 0]], hi[p[:, 0]], bx), linspace_edges(lo[p[:, 1]], hi[p[:, 1]], by)
    counts = torch.zeros((P, bx, by), dtype=torch.int64, device=device)
    outside = torch.zeros((P, 3), dtype=torch.int64, device=device)
    exd, eyd = torch.as_tensor(ex).to(device), torch.as_tensor(ey).to(device)
    pd = torch.as_tensor(p).to(device) if route == "kernel" and P else None
    for a, b in spans:
        chunk = _place(X[a:b], route)
        if route == "torch":
            _joint_histogram_torch(chunk, p, exd, eyd, counts, outside)
        else:
            _joint_histogram_kernel(chunk, pd, exd, eyd, counts, outside)
    return JointHistograms(counts.cpu().numpy(), outside.cpu().numpy(), ex, ey)


# ---- the data loader's pairing -------------------------------------------------------------------------------------------------------

class CoordDeltaTooBig(Exception):
    """dataloader.py:196-210: a conditioning / target pair more than 100 nm apart."""

    def __init__(self, name, delta, step1, step2):
        super().__init__(f"{name} trajectory has {delta:g} distance between steps {step1} and {step2}")
        self.name, self.delta, self.step1, self.step2 = name, delta, step1, step2


@dataclasses.dataclass
class TrajectoryPairs:
    """What `trajectory_pairs` returns (numpy): the frames at `step` (features) and at `step + step_width` (targets)."""

    steps: np.ndarray            # int64 [n], the conditioning steps in file order
    coord_features: np.ndarray   # float32 [n, V, 3]
    veloc_features: np.ndarray
    coord_targets: np.ndarray
    veloc_targets: np.ndarray
    spacing: int                 # largest interval of the first 100 steps, times 10 // 9


def trajectory_pairs(traj_npz, step_width: int = 1, equal_data_spacing: bool = False, limit: Optional[int] = None,
                     name: str = "trajectory") -> TrajectoryPairs:
    """The pairing of dataloader.py:213-276 (`load_pdb_trace_data`) on a `*-traj-arrays.npz` (a path, or a mapping with `step`,
    `positions`, `velocities`): for every frame, in file order, the frame `step_width` steps later is looked up BY THE FILE'S `step`
    ARRAY (a later frame with the same step replaces an earlier one, as the reference's dict does); frames without a partner are
    skipped.  spacing = largest interval between the first 100 steps, times 10 // 9 (the logarithmic policy's block length); with
    `equal_data_spacing` only steps that are multiples of it condition; otherwise `spacing <= step_width` gives the reference's
    warning.  A pair more than 100 apart (root of the summed squared displacement) raises `CoordDeltaTooBig`.  `limit` stops after
    that many pairs.

    The reference's `adj_list` comes from mdtraj's topology; here the bonds are the force-field tables' `bond_idx`
    (`forcefield.tables_from_pdb`).  mdtraj's bond ORDER is not reproduced, only the set of bonds."""
    if isinstance(traj_npz, (str, os.PathLike)):
        with np.load(traj_npz) as z:
            data = {k: z[k] for k in ("step", "positions", "velocities")}
    else:
        data = traj_npz
    step = np.asarray(data["step"]).astype(np.int64)
    pos, vel = data["positions"], data["velocities"]
    head = step[:100]
    spacing = int((head[1:] - head[:-1]).max() * 10 // 9)
    if spacing <= step_width and not equal_data_spacing:
        warnings.warn(f"The step_width of {step_width} is larger than or equal to the spacing of {spacing} in the data. This results "
                      "in an unequal spacing between conditioning-target pairs.")
    row_of = {int(s): i for i, s in enumerate(step)}          # the last frame of a step wins
    seen, src, dst = set(), [], []
    for s in step.tolist():
        if s in seen:                                           # the dict holds each step once
            continue
        seen.add(s)
        if equal_data_spacing and s % spacing != 0:
            continue
        j = row_of.get(s + int(step_width))
        if j is None:
            continue
        i = row_of[s]
        delta = float(np.sqrt(np.sum((pos[i] - pos[j]) ** 2)))
        if delta > 100:
            raise CoordDeltaTooBig(name=name, delta=delta, step1=s, step2=s + int(step_width))
        src.append(i)
        dst.append(j)
        if limit is not None and len(src) >= int(limit):
            break
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    f32 = lambda a, i: np.ascontiguousarray(np.asarray(a)[i], dtype=np.float32)
    return TrajectoryPairs(step[src], f32(pos, src), f32(vel, src), f32(pos, dst), f32(vel, dst), spacing)


def conditional_md_samples(dynamics, coords, velocs, num_samples: int, step_width: int, random_velocs: bool = False,
                           generator: Optional[torch.Generator] = None):
    """The MD half of sample_on_single_conditional (utils/evaluation_utils.py:356-413) without OpenMM: `num_samples` replicas of ONE
    state (coords, velocs [V, 3]) go through ONE `dynamics.step(num_steps=step_width)` (`md.LangevinDynamics`; every row of a launch
    has its own noise stream, so the replicas differ).  random_velocs=True starts every replica from its own Maxwell-Boltzmann
    velocities (`simulation.thermal_velocities`, `generator`), the reference's setVelocitiesToTemperature.  Returns (coords,
    velocs) [num_samples, V, 3] float32 on the device.  Not compared with OpenMM."""
    _need_gpu("conditional_md_samples")
    x = torch.as_tensor(coords, dtype=torch.float32)
    dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    V = x.shape[-2]
    x = x.reshape(1, V, 3).to(dev).expand(int(num_samples), V, 3).contiguous()
    if random_velocs:
        from .simulation import thermal_velocities

        v = thermal_velocities(dynamics.masses, dynamics.kbT, x, generator=generator)
    else:
        v = torch.as_tensor(velocs, dtype=torch.float32).reshape(1, V, 3).to(dev).expand(int(num_samples), V, 3).contiguous()
    return dynamics.step(x, v, num_steps=int(step_width))


# ---- the report ----------------------------------------------------------------------------------------------------------------------

def jensen_shannon(counts_a: np.ndarray, counts_b: np.ndarray) -> np.ndarray:
    """The Jensen-Shannon divergence (natural logarithm, 0 .. ln 2) of the two count vectors of every column, fp64 [C]; NaN where
    either has no counts."""
    a, b = np.asarray(counts_a, dtype=np.float64), np.asarray(counts_b, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        p, q = a / a.sum(axis=1, keepdims=True), b / b.sum(axis=1, keepdims=True)
        m = 0.5 * (p + q)
        kl = lambda u: np.where(u > 0, u * np.log(u / m), 0.0).sum(axis=1)
        js = 0.5 * kl(p) + 0.5 * kl(q)
    return np.where(np.isnan(p).any(axis=1) | np.isnan(q).any(axis=1), np.nan, js)


def binned_moments(h: Histograms) -> Tuple[np.ndarray, np.ndarray]:
    """(mean, std) fp64 [C] of the count vectors: of the distribution that puts counts[c, i] at the centre of bin i."""
    centres = 0.5 * (h.edges[:, 1:] + h.edges[:, :-1])
    n = h.counts.sum(axis=1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (h.counts * centres).sum(axis=1) / n
        var = (h.counts * (centres - mean[:, None]) ** 2).sum(axis=1) / n
    return mean, np.sqrt(var)


@dataclasses.dataclass
class SampleSet:
    """One side of the report.  coords [T, V, 3] is required; the rest is optional and switches the figures it feeds on:
    delta_x [T, V, 3] (target minus conditioning coordinates), velocs [T, V, 3], e_pot / e_kin [T] (kJ/mol, however they were
    computed).  numpy or device tensors."""

    coords: object
    delta_x: object = None
    velocs: object = None
    e_pot: object = None
    e_kin: object = None


@dataclasses.dataclass
class HistogramPair:
    """A quantity's histograms for the model and for MD; with shared edges also the binned mean and std of each and the
    Jensen-Shannon divergence between the two count vectors, per column."""

    model: Histograms
    md: Histograms
    mean_model: Optional[np.ndarray] = None
    std_model: Optional[np.ndarray] = None
    mean_md: Optional[np.ndarray] = None
    std_md: Optional[np.ndarray] = None
    js: Optional[np.ndarray] = None


@dataclasses.dataclass
class EvaluationReport:
    """What `evaluation_report` returns; `save` writes it as one npz (`load_report` reads the arrays back)."""

    bins: int
    edges_mode: str
    adj_list: np.ndarray                                   # [n_bonds, 2]
    histograms: Dict[str, HistogramPair]                   # bonds, delta_x, velocs, e_pot, e_kin when their inputs were given
    ramachandran_model: np.ndarray                         # int64 [n_residue_pairs, bins, bins] (first axis phi)
    ramachandran_md: np.ndarray
    psi_transitions_model: np.ndarray                      # float32 [T, n_psi]: (psi - 0.5 + 3) % 6 - 3
    psi_transitions_md: np.ndarray
    correlation_model: Optional[np.ndarray] = None         # fp64 [V, V] of the x components of delta_x
    correlation_md: Optional[np.ndarray] = None
    correlation_difference: Optional[np.ndarray] = None    # |md - model|
    likelihoods: Dict[str, Histograms] = dataclasses.field(default_factory=dict)

    def arrays(self) -> Dict[str, np.ndarray]:
        out = {"bins": np.int64(self.bins), "edges_mode": np.str_(self.edges_mode), "adj_list": self.adj_list,
               "ramachandran_model": self.ramachandran_model, "ramachandran_md": self.ramachandran_md,
               "psi_transitions_model": self.psi_transitions_model, "psi_transitions_md": self.psi_transitions_md}
        for name, pair in self.histograms.items():
            for side in ("model", "md"):
                h = getattr(pair, side)
                for f in ("counts", "edges", "below", "above", "nonfinite"):
                    out[f"{name}_{side}_{f}"] = getattr(h, f)
            for f in ("mean_model", "std_model", "mean_md", "std_md", "js"):
                if getattr(pair, f) is not None:
                    out[f"{name}_{f}"] = getattr(pair, f)
        for f in ("correlation_model", "correlation_md", "correlation_difference"):
            if getattr(self, f) is not None:
                out[f] = getattr(self, f)
        for name, h in self.likelihoods.items():
            for f in ("counts", "edges", "below", "above", "nonfinite"):
                out[f"likelihood_{name}_{f}"] = getattr(h, f)
        return out

    def save(self, path: str) -> str:
        np.savez(path, **self.arrays())
        return path


def load_report(path: str) -> Dict[str, np.ndarray]:
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _correlation(delta_x, route: str, chunk_rows: Optional[int]) -> np.ndarray:
    """np.corrcoef(delta_x[:, :, 0].T) (evaluate.py:398-399) in torch fp64, as numpy computes it - centred first: one walk over the
    chunks for the column means m, a second for S = sum (x - m)(x - m)^T, then S_ij / sqrt(S_ii S_jj).  Nothing cancels however large
    the means are against the spread.  Fewer than two rows have no correlation and are refused; a constant column gives NaN, as
    numpy does."""
    T = int(delta_x.shape[0])
    if T < 2:
        raise ValueError(f"the correlation matrix needs at least two rows of delta_x, got {T}")
    spans = _row_chunks(T, chunk_rows)
    s = None
    for a, b in spans:
        x = _place(delta_x[a:b], "torch")[:, :, 0].double()
        s = x.sum(dim=0) if s is None else s + x.sum(dim=0)
    mean = s / T
    ss = None
    for a, b in spans:
        z = _place(delta_x[a:b], "torch")[:, :, 0].double() - mean
        ss = z.T @ z if ss is None else ss + z.T @ z
    d = torch.sqrt(torch.diagonal(ss))
    return (ss / torch.outer(d, d)).cpu().numpy()


def _paired(name: str, model, md, bins: int, edges_mode: str, route: str, chunk_rows, pairs=None, range_model=None,
            range_md=None) -> HistogramPair:
    """The two histograms of one quantity: `model` / `md` are [T, C] matrices (views are fine) or, with `pairs`, coordinates."""
    def one(x, range_, edges=None):
        if pairs is not None:
            return pair_histograms(x, pairs, bins, range_, route, chunk_rows, edges)
        return column_histograms(x, bins, range_, route if route in COLUMN_ROUTES else "kernel", chunk_rows, edges)

    if edges_mode == "own" or range_model is not None or range_md is not None:
        return HistogramPair(one(model, range_model), one(md, range_md))
    # shared: the union of the two ranges, from a range pass over both
    ranges = []
    for x in (model, md):
        if pairs is not None:
            T = int(x.shape[0])
            chunks = (_Columns(route, coords=_coords_3d(x[a:b], route), pairs=pairs) for a, b in _row_chunks(T, chunk_rows))
        else:
            r = route if route in COLUMN_ROUTES else "kernel"
            chunks = (_Columns(r, X=_place(x[a:b], r)) for a, b in _row_chunks(int(x.shape[0]), chunk_rows))
        n_cols = len(pairs) if pairs is not None else int(x.shape[1])
        lo, hi, nf = _ranges_over(chunks, n_cols)
        ranges.append(_auto_range(lo, hi, nf, f"evaluation_report: {name}"))
    edges = linspace_edges(np.minimum(ranges[0][0], ranges[1][0]), np.maximum(ranges[0][1], ranges[1][1]), bins)
    hm, hd = one(model, None, edges), one(md, None, edges)
    mm, sm = binned_moments(hm)
    md_, sd = binned_moments(hd)
    return HistogramPair(hm, hd, mm, sm, md_, sd, jensen_shannon(hm.counts, hd.counts))


def _column_matrix(x) -> object:
    """[T] -> [T, 1] for the energies and likelihoods."""
    return x.reshape(-1, 1)


def _torsions(coords, tables, chunk_rows, route: str):
    """(phi, psi) float32 numpy [T, n] of coords, chunk by chunk: `analysis.dihedrals`, or the oracle-free torch restatement of
    mdtraj's convention when the report runs without a GPU."""
    n_phi = len(tables["phi"])
    quads = np.concatenate([tables["phi"], tables["psi"]], axis=0)
    parts = []
    for a, b in _row_chunks(int(coords.shape[0]), chunk_rows):
        x = _coords_3d(coords[a:b], route)
        if route == "torch":
            q = torch.as_tensor(quads.astype(np.int64), device=x.device)
            p = x.double()[:, q]                                           # [T, n, 4, 3]
            b1, b2, b3 = p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 1], p[:, :, 3] - p[:, :, 2]
            c1, c2 = torch.linalg.cross(b2, b3), torch.linalg.cross(b1, b2)
            ang = torch.atan2((b1 * c1).sum(-1) * torch.linalg.norm(b2, dim=-1), (c1 * c2).sum(-1)).to(torch.float32)
        else:
            ang = analysis.dihedrals(x, quads)
        parts.append(ang.cpu().numpy())
    ang = np.concatenate(parts, axis=0) if parts else np.zeros((0, len(quads)), dtype=np.float32)
    return ang[:, :n_phi], ang[:, n_phi:]


def _ramachandran(phi: np.ndarray, psi: np.ndarray, residue_pairs, bins: int) -> np.ndarray:
    out = [analysis.ramachandran_histogram(phi[:, i], psi[:, j], bins).cpu().numpy() for i, j in residue_pairs]
    return np.stack(out) if out else np.zeros((0, bins, bins), dtype=np.int64)


def evaluation_report(model: SampleSet, md: SampleSet, topology, adj_list, bins: int = 100, edges: str = "shared",
                      energy_range: Optional[str] = None, log_likelihoods: Optional[Dict[str, object]] = None,
                      route: Optional[str] = None, chunk_rows: Optional[int] = None) -> EvaluationReport:
    """The data behind the figures of evaluate.py:328-856 for a model set against an MD set (`SampleSet`s; numpy inputs are walked
    `chunk_rows` rows at a time: the range pass first, then the accumulating histogram calls).

      histograms["bonds"]    the length of every bond of `adj_list` (plot_bonds), `pair_histograms`
      histograms["delta_x"], ["velocs"]   the x component per atom (plot_marginal_distribution), read in place with col_stride 3
      histograms["e_pot"], ["e_kin"]      plot_energy; energy_range="reference" gives its ranges - the model on (md.min(), 200), MD on
                             its own range - instead of the `edges` rule
      ramachandran_*         counts over [-pi, pi]^2 per residue that has both phi and psi (`analysis.ramachandran_histogram`)
      psi_transitions_*      (psi - 0.5 + 3) % 6 - 3, the series plot_transitions draws
      correlation_*          np.corrcoef of the x components of delta_x and the absolute difference (evaluate.py:398-399, :436)
      likelihoods[name]      a histogram of each array in `log_likelihoods` on its own range (evaluate.py:449-484)

    edges="shared" (the default) bins model and MD on the union of their ranges, so that the two count vectors can be compared, and
    stores per column the binned mean and std of each and their Jensen-Shannon divergence (fp64, on the host).  edges="own"
    reproduces plt.hist's per-array edges.  `route`: PAIR_ROUTES for the bonds; the column histograms take "kernel" unless it is
    "torch", which also computes the torsions with torch ops and so runs without a GPU."""
    if edges not in ("shared", "own"):
        raise ValueError(f"edges {edges!r}: 'shared' or 'own'")
    if energy_range not in (None, "reference"):
        raise ValueError(f"energy_range {energy_range!r}: None or 'reference'")
    route = _route(route, PAIR_ROUTES, DEFAULT_PAIR_ROUTE)
    bins = _check_bins(bins)
    V = int(model.coords.shape[1])
    pairs = _pairs_table(adj_list, V)
    names, res, rid = analysis._topology(topology)
    tables = analysis.torsion_indices(names, res, rid)
    hists: Dict[str, HistogramPair] = {}
    hists["bonds"] = _paired("bonds", model.coords, md.coords, bins, edges, route, chunk_rows, pairs=pairs)
    for key in ("delta_x", "velocs"):
        a, b = getattr(model, key), getattr(md, key)
        if a is not None and b is not None:
            hists[key] = _paired(key, a[:, :, 0], b[:, :, 0], bins, edges, route, chunk_rows)
    for key in ("e_pot", "e_kin"):
        a, b = getattr(model, key), getattr(md, key)
        if a is not None and b is not None:
            a, b = _column_matrix(a), _column_matrix(b)
            if energy_range == "reference":
                md_min = float(torch.as_tensor(b).min()) if isinstance(b, torch.Tensor) else float(np.min(b))
                md_min = float(np.float32(md_min))
                hists[key] = _paired(key, a, b, bins, "own", route, chunk_rows, range_model=(md_min, 200.0))
            else:
                hists[key] = _paired(key, a, b, bins, edges, route, chunk_rows)
    # residues with both angles: phi's second atom (N) and psi's first (N) belong to the same residue
    phi_n = {int(q[1]): i for i, q in enumerate(tables["phi"])}
    residue_pairs = [(phi_n[int(q[0])], j) for j, q in enumerate(tables["psi"]) if int(q[0]) in phi_n]
    tors = {}
    for side, s in (("model", model), ("md", md)):
        phi, psi = _torsions(s.coords, tables, chunk_rows, route)
        tors[side] = (_ramachandran(phi, psi, residue_pairs, bins), ((psi - np.float32(0.5) + np.float32(3)) % np.float32(6)
                                                                      - np.float32(3)).astype(np.float32))
    report = EvaluationReport(bins=bins, edges_mode=edges, adj_list=pairs, histograms=hists, ramachandran_model=tors["model"][0],
                              ramachandran_md=tors["md"][0], psi_transitions_model=tors["model"][1], psi_transitions_md=tors["md"][1])
    if model.delta_x is not None and md.delta_x is not None:
        report.correlation_model = _correlation(model.delta_x, route, chunk_rows)
        report.correlation_md = _correlation(md.delta_x, route, chunk_rows)
        report.correlation_difference = np.abs(report.correlation_md - report.correlation_model)
    for name, values in (log_likelihoods or {}).items():
        report.likelihoods[name] = column_histograms(_column_matrix(values), bins, None,
                                                     route if route in COLUMN_ROUTES else "kernel", chunk_rows)
    return report


# ---- command line --------------------------------------------------------------------------------------------------------------------

def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m timewarp_amd.evaluate",
                                description="Bond, torsion, Delta x and energy histograms of a model chain against an MD run.  Both "
                                            "runs are read whole into host memory; only the device side works in chunks")
    p.add_argument("--md", required=True, help="*-traj-arrays.npz of the MD run (simulation.py's format)")
    p.add_argument("--model-dir", required=True, help="directory of the chain segments sample_trajectory wrote")
    p.add_argument("--protein", required=True, help="the chain's protein name (the segments' file stem)")
    p.add_argument("--pdb", required=True, help="the state0 PDB (topology; its force-field bonds are the adjacency list)")
    p.add_argument("--force-field", default="amber99-implicit", help="a key of forcefield.PRESET_FAMILY: whose bonds and energies")
    p.add_argument("--bins", type=int, default=100)
    p.add_argument("--stride", type=int, default=1, help="thin the chain's segments on reading")
    p.add_argument("--chunk-frames", type=int, default=DEFAULT_CHUNK_ROWS, help="frames uploaded and binned at a time")
    p.add_argument("--step-width", type=int, default=1, help="MD steps between a conditioning frame and its target (Delta x of MD)")
    p.add_argument("--route", default=None, choices=PAIR_ROUTES,
                   help="'torch' runs without a GPU and leaves the energy histograms out: the potential energy is a HIP kernel")
    p.add_argument("--no-energies", action="store_true", help="skip the potential-energy histograms")
    p.add_argument("--out", default=None, help="output file (default <protein>_evaluation.npz in the working directory)")
    return p


def main(argv=None) -> str:
    """The "sample on samples" report (evaluate.py:775-855) at chain scale: the chain `analysis.load_model_chain` reads against the
    MD run, both walked in chunks of --chunk-frames frames.  Delta x: consecutive chain states for the model, `trajectory_pairs`
    with --step-width for MD (skipped, with a note, when the MD file has no such pairs).  --route torch has no energy kernel and
    leaves the energy histograms out, with a note.

    What is chunked is the DEVICE side: the upload, the range pass and the accumulating histogram calls.  Both position arrays, and
    the chain's frame-to-frame differences, are held whole in host memory (numpy), so a run must fit there: 10^7 frames of a 691-atom
    protein (83 GB per array) do not.  Thin with --stride, or call `column_histograms` / `pair_histograms` with `edges=` on pieces
    of a run and add the counts - the kernels accumulate."""
    args = build_parser().parse_args(argv)
    from .simulation import pdb_system

    route = _route(args.route, PAIR_ROUTES, DEFAULT_PAIR_ROUTE)
    positions, _ = analysis.load_model_chain(args.model_dir, args.protein, stride=args.stride)
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    with np.load(args.md) as z:
        md = {k: z[k] for k in z.files}
    md_pos = np.ascontiguousarray(md["positions"], dtype=np.float32)
    if md_pos.ndim != 3 or positions.ndim != 3 or md_pos.shape[1:] != positions.shape[1:]:
        raise SystemExit(f"positions: MD {md_pos.shape} and chain {positions.shape} must both be [T, V, 3] of one molecule")
    energy, _, _, _ = pdb_system(args.pdb, args.force_field)
    adj_list = np.asarray(energy.tables.bond_idx, dtype=np.int32).reshape(-1, 2)
    model_set, md_set = SampleSet(positions), SampleSet(md_pos)
    if len(positions) > 1:
        model_set.delta_x = positions[1:] - positions[:-1]
    if "velocities" in md and "step" in md and len(md["step"]) > 1:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            tp = trajectory_pairs(md, step_width=args.step_width, name=args.protein)
        if len(tp.steps):
            md_set.delta_x = tp.coord_targets - tp.coord_features
    if md_set.delta_x is None or model_set.delta_x is None:
        print(f"no frame pairs {args.step_width} step(s) apart in {args.md}: Delta x histograms and correlations are left out")
        model_set.delta_x = md_set.delta_x = None
    if not args.no_energies and route == "torch":
        print("--route torch: the potential energy is a HIP kernel; the energy histograms are left out")
    if not args.no_energies and route != "torch":
        def potential(x):
            parts = [energy(torch.as_tensor(x[a:b]).to("cuda")).float().cpu().numpy() for a, b in _row_chunks(len(x), args.chunk_frames)]
            return np.concatenate(parts)

        model_set.e_pot, md_set.e_pot = potential(positions), potential(md_pos)
    report = evaluation_report(model_set, md_set, args.pdb, adj_list, bins=args.bins, route=route, chunk_rows=args.chunk_frames)
    out = args.out or f"{args.protein}_evaluation.npz"
    report.save(out)
    js = report.histograms["bonds"].js
    print(f"{out}: {len(positions)} chain frames against {len(md_pos)} MD frames, {len(adj_list)} bonds; "
          f"largest bond-length Jensen-Shannon divergence {np.nanmax(js) if len(js) else float('nan'):.4g}")
    return out


if __name__ == "__main__":
    main()
