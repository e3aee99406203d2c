"""Analysis of trajectories where they are produced, on the device: torsion angles, the TICA feature vector, time-lagged second
moments with the TICA they give, and the effective sample size the paper's speed-up is stated in.

    python -m timewarp_amd.analysis TRAJ-traj-arrays.npz --pdb TRAJ-traj-state0.pdb [--lag 500 --dim 10 --max-lag N]

What stands in for what (the reference does all of this on the host with mdtraj and deeptime, which this package does not use):

  `compute_torsions`, `TorsionAngles`   utils/torsion_utils.py:22-81 (mdtraj's compute_phi ... compute_omega)
  `tica_features`                       utils/tica_utils.py:10-37
  `lagged_moments`, `tica_from_moments` the sums deeptime's covariance estimator takes, and its symmetrised TICA
  `koopman_from_moments`, `frame_weights`   deeptime's KoopmanWeightingEstimator, which utils/tica_utils.py:40-44 fits first
  `run_tica`, `TicaModel`               utils/tica_utils.py:40-46 (`run_tica`): Koopman weights, then TICA on the reweighted
                                        moments; `TicaModel.transform` is deeptime's `transform` (without its kinetic_map scaling)
  `free_energy`                         utils/tica_utils.py:59-63 (`plot_free_energy`, the curve without the plot)
  `autocorrelation`, `effective_sample_size`, `ramachandran_histogram`   the quantities of the paper's evaluation

Hot paths are HIP kernels (csrc/tw_analysis.hip: `tw_dihedrals`, `tw_tica_features`, `tw_lagged_moments`,
`tw_lagged_moments_weighted`, `tw_project`); there is no host fallback for them.  The eigen-solves, the FFT and the histograms are
torch calls on whatever device their input is on (the one non-symmetric eigen-solve, of the Koopman matrix, runs on the host).
Nothing here claims equality with mdtraj's or deeptime's output: neither is available to compare against.
"""
from __future__ import annotations

import argparse
import dataclasses
import os
import warnings
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

FAMILIES = ("phi", "psi", "chi1", "chi2", "chi3", "chi4", "omega")   # the field order of the reference's TorsionAngles

# The routes `lagged_moments` can take.  "kernel": tw_lagged_moments (bounded memory, fixed summation order, bit-reproducible).
# "torch": float64 casts of the lagged slices and torch.matmul.  The default is the one that measured faster on the MI355X
# (profiles/analysis.txt) - for the plain and for the weighted sums alike (6.9 ms against 44 ms weighted).
MOMENTS_ROUTES = ("kernel", "torch")
DEFAULT_MOMENTS_ROUTE = "kernel"

_CHI = {
    "chi1": (("N", "CA", "CB", "CG"), ("N", "CA", "CB", "CG1"), ("N", "CA", "CB", "SG"), ("N", "CA", "CB", "OG"),
             ("N", "CA", "CB", "OG1")),
    "chi2": (("CA", "CB", "CG", "CD"), ("CA", "CB", "CG", "CD1"), ("CA", "CB", "CG1", "CD1"), ("CA", "CB", "CG", "OD1"),
             ("CA", "CB", "CG", "ND1"), ("CA", "CB", "CG", "SD")),
    "chi3": (("CB", "CG", "CD", "NE"), ("CB", "CG", "CD", "CE"), ("CB", "CG", "CD", "OE1"), ("CB", "CG", "SD", "CE")),
    "chi4": (("CG", "CD", "NE", "CZ"), ("CG", "CD", "CE", "NZ")),
}
# (atom name, residue offset) of the backbone quads
_BACKBONE = {
    "phi": (("C", -1), ("N", 0), ("CA", 0), ("C", 0)),
    "psi": (("N", 0), ("CA", 0), ("C", 0), ("N", 1)),
    "omega": (("CA", 0), ("C", 0), ("N", 1), ("CA", 1)),
}

Topology = Union[str, Tuple[Sequence[str], Sequence[str], Sequence[int]], dict]


def _topology(topology: Topology):
    """(atom_names, residue_names, residue_ids) from a PDB path, a mapping with those keys (an `energy_kat_*.npz`) or the tuple."""
    if isinstance(topology, (str, os.PathLike)):
        from .forcefield import read_pdb_topology

        return read_pdb_topology(os.fspath(topology))
    if hasattr(topology, "keys") or hasattr(topology, "files"):
        return topology["atom_names"], topology["residue_names"], topology["residue_ids"]
    names, res, rid = topology
    return names, res, rid


def torsion_indices(atom_names: Sequence[str], residue_names: Sequence[str], residue_ids: Sequence[int]) -> dict:
    """The seven index tables of mdtraj's compute_phi / psi / omega / chi1 .. chi4 as int32 [n, 4], keyed by family, rows ordered
    by residue.  The topology is per atom (name, residue name, residue id), the form `forcefield.tables_from_pdb` and the
    energy_kat fixtures use; one chain, residues in order of first appearance.

    Backbone (i is a residue, i-1 / i+1 its neighbours in the chain; a quad exists when all four atoms do):
        phi   = C(i-1), N, CA, C
        psi   = N, CA, C, N(i+1)
        omega = CA, C, N(i+1), CA(i+1)
    Side chains (within one residue; the first alternative that the residue has):
        chi1 = N-CA-CB-{CG, CG1, SG, OG, OG1}
        chi2 = CA-CB-CG-{CD, CD1, OD1, ND1, SD}, and CA-CB-CG1-CD1 (CG1 is only ever paired with CD1)
        chi3 = CB-CG-CD-NE, CB-CG-CD-CE, CB-CG-CD-OE1, CB-CG-SD-CE
        chi4 = CG-CD-NE-CZ, CG-CD-CE-NZ

    These are mdtraj's documented definitions RESTATED FROM MEMORY.  They are not pinned against mdtraj, which is not available
    here; what is pinned is what the reference's own tests pin (the count of phi angles of 1hgv) and the counts that follow from
    the chemistry of small peptides (tests/test_analysis_cpu.py)."""
    del residue_names  # the atom names decide; kept in the signature because it is the topology's form everywhere else
    rids = list(dict.fromkeys(int(r) for r in residue_ids))
    atoms = [dict() for _ in rids]
    pos = {r: k for k, r in enumerate(rids)}
    for i, (a, r) in enumerate(zip(atom_names, residue_ids)):
        atoms[pos[int(r)]].setdefault(str(a), i)
    out = {f: [] for f in FAMILIES}
    for k in range(len(rids)):
        for fam, spec in _BACKBONE.items():
            if all(0 <= k + off < len(rids) and name in atoms[k + off] for name, off in spec):
                out[fam].append([atoms[k + off][name] for name, off in spec])
        for fam, alternatives in _CHI.items():
            for alt in alternatives:
                if all(name in atoms[k] for name in alt):
                    out[fam].append([atoms[k][name] for name in alt])
                    break
    return {f: np.asarray(out[f], dtype=np.int32).reshape(-1, 4) for f in FAMILIES}


@dataclasses.dataclass
class TorsionAngles:
    """The reference's dataclass (utils/torsion_utils.py:22-41): angles [B, S, n] float32, index tables [n, 4]."""

    phi: np.ndarray
    psi: np.ndarray
    chi1: np.ndarray
    chi2: np.ndarray
    chi3: np.ndarray
    chi4: np.ndarray
    omega: np.ndarray

    phi_indices: np.ndarray
    psi_indices: np.ndarray
    chi1_indices: np.ndarray
    chi2_indices: np.ndarray
    chi3_indices: np.ndarray
    chi4_indices: np.ndarray
    omega_indices: np.ndarray


def check_indices(idx: np.ndarray, n_atoms: int, what: str) -> np.ndarray:
    """int32 copy of an index table after its range check: the library does not read device arrays on the host, so a table is
    checked here before it is uploaded."""
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= n_atoms):
        raise ValueError(f"{what}: entries must be in 0 .. {n_atoms - 1}, got {int(idx.min())} .. {int(idx.max())}")
    return idx.astype(np.int32)


def _device_coords(coords) -> Tuple[torch.Tensor, bool]:
    """(float32 contiguous device tensor, the input was numpy).  numpy input goes to cuda:0 - there is no host path."""
    was_numpy = not isinstance(coords, torch.Tensor)
    if was_numpy:
        if not torch.cuda.is_available():
            raise RuntimeError("timewarp_amd.analysis: the featurisation runs on an MI355X; no GPU is visible and there is no CPU fallback")
        coords = torch.as_tensor(np.ascontiguousarray(coords, dtype=np.float32)).to("cuda")
    return _lib.require_gpu_tensor(coords, torch.float32, "coords"), was_numpy


def dihedrals(coords, quads) -> torch.Tensor:
    """Angles [n_rows, n_quads] float32 (radians, (-pi, pi], IUPAC sign) of coords [n_rows, n_atoms, 3] (`tw_dihedrals`)."""
    x, _ = _device_coords(coords)
    n_rows, n_atoms = x.shape[0], x.shape[1]
    q = check_indices(np.asarray(quads).reshape(-1, 4), n_atoms, "quads")
    out = torch.empty((n_rows, len(q)), dtype=torch.float32, device=x.device)
    if len(q) and n_rows:
        qd = torch.as_tensor(q).to(x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().tw_dihedrals(x.data_ptr(), qd.data_ptr(), len(q), out.data_ptr(), n_rows, n_atoms,
                                                _lib.stream_ptr(x.device)), "tw_dihedrals")
    return out


def compute_torsions(coords, topology: Topology) -> TorsionAngles:
    """utils/torsion_utils.py:44-81 on the device.  coords [B, S, V, 3] (numpy or a device tensor); angles come back [B, S, n]
    float32 - device tensors for a device tensor, numpy for numpy; the index tables are numpy int32 [n, 4] (`torsion_indices`)."""
    if len(coords.shape) != 4:
        raise ValueError("Shape should be [B, S, V, 3]")
    tables = torsion_indices(*_topology(topology))
    x, was_numpy = _device_coords(coords)
    B, S, V = x.shape[0], x.shape[1], x.shape[2]
    sizes = [len(tables[f]) for f in FAMILIES]
    all_quads = np.concatenate([tables[f] for f in FAMILIES], axis=0)
    ang = dihedrals(x.reshape(B * S, V, 3), all_quads)   # one launch for the seven families
    parts = [a.reshape(B, S, -1).contiguous() for a in torch.split(ang, sizes, dim=1)]
    if was_numpy:
        parts = [a.cpu().numpy() for a in parts]
    return TorsionAngles(*parts, *[tables[f] for f in FAMILIES])


def feature_tables(topology: Topology, selection=("C", "N", "S"), use_dihedrals=True, use_distances=True,
                   families=("phi", "psi", "omega")):
    """(atom_sel [n_sel], quads [n_quads, 4], quad_cols [n_quads, 2]) of `tica_features`: the selected atoms (element = first letter
    of the atom name), the quads of `families` one family after the other, and for each quad the columns of its sine and cosine
    within the torsion block: per family the sines of its angles, then the cosines."""
    names, res, rid = _topology(topology)
    sel = np.asarray([i for i, a in enumerate(names) if str(a)[:1] in selection], dtype=np.int32) if use_distances else \
        np.zeros(0, dtype=np.int32)
    quads, cols, base = [], [], 0
    if use_dihedrals:
        tables = torsion_indices(names, res, rid)
        for f in families:
            n = len(tables[f])
            quads.append(tables[f])
            cols.append(np.stack([base + np.arange(n), base + n + np.arange(n)], axis=1))
            base += 2 * n
    quads = np.concatenate(quads, axis=0).astype(np.int32) if quads else np.zeros((0, 4), dtype=np.int32)
    cols = np.concatenate(cols, axis=0).astype(np.int32) if cols else np.zeros((0, 2), dtype=np.int32)
    return sel, quads, cols


def features_from_tables(coords, atom_sel, quads, quad_cols) -> torch.Tensor:
    """`tw_tica_features` on coords [n_rows, n_atoms, 3]: float32 [n_rows, n_sel (n_sel - 1) / 2 + 2 n_quads] on the device."""
    x, _ = _device_coords(coords)
    n_rows, n_atoms = x.shape[0], x.shape[1]
    sel = check_indices(np.asarray(atom_sel).reshape(-1), n_atoms, "atom_sel")
    q = check_indices(np.asarray(quads).reshape(-1, 4), n_atoms, "quads")
    qc = np.ascontiguousarray(np.asarray(quad_cols).reshape(-1, 2), dtype=np.int64)
    if len(qc) != len(q) or sorted(qc.reshape(-1).tolist()) != list(range(2 * len(q))):
        raise ValueError("quad_cols: [n_quads, 2], a permutation of 0 .. 2 n_quads - 1")
    n_pairs = len(sel) * (len(sel) - 1) // 2 if len(sel) > 1 else 0
    F = n_pairs + 2 * len(q)
    out = torch.empty((n_rows, F), dtype=torch.float32, device=x.device)
    if F and n_rows:
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(x.device)
        sd, qd, cd = up(sel), up(q), up(qc)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().tw_tica_features(x.data_ptr(), sd.data_ptr() if len(sel) else None, len(sel),
                                                    qd.data_ptr() if len(q) else None, cd.data_ptr() if len(q) else None, len(q),
                                                    out.data_ptr(), n_rows, n_atoms, F, _lib.stream_ptr(x.device)), "tw_tica_features")
    return out


def tica_features(coords, topology: Topology, selection=("C", "N", "S"), use_dihedrals=True, use_distances=True):
    """utils/tica_utils.py:22-37 on the device: for coords [..., V, 3] the features [..., F] float32 (a device tensor for a device
    tensor, numpy for numpy) - the pair distances of the atoms whose element is in `selection`, in np.triu_indices(n, k=1) order,
    then sin(phi), cos(phi), sin(psi), cos(psi), sin(omega), cos(omega).

    One deliberate difference: the reference calls compute_phi twice (tica_utils.py:26-27), so its "psi" columns are phi again.
    Here they are psi."""
    tables = feature_tables(topology, selection, use_dihedrals, use_distances)
    x, was_numpy = _device_coords(coords)
    out = features_from_tables(x.reshape(-1, x.shape[-2], 3), *tables).reshape(*x.shape[:-2], -1)
    return out.cpu().numpy() if was_numpy else out


@dataclasses.dataclass
class Moments:
    """Sums over the n_pairs pairs x = X[c, t], y = X[c, t + lag] (fp64; tensors, or numpy when the input was numpy).  Weighted
    moments (`lagged_moments(..., weights=...)`) hold sum w x, sum w x x^T, ... and the sum of the weights in `sum_w`; whatever
    divides the sums (`normaliser`) is `sum_w` when it is set and `n_pairs` otherwise."""

    n_pairs: int
    lag: int
    sum_x: torch.Tensor    # [F]
    sum_y: torch.Tensor    # [F]
    c_xx: torch.Tensor     # [F, F]  sum x x^T
    c_xy: torch.Tensor     # [F, F]  sum x y^T
    c_yy: torch.Tensor     # [F, F]  sum y y^T
    sum_w: Optional[float] = None

    @property
    def normaliser(self) -> float:
        return float(self.n_pairs if self.sum_w is None else self.sum_w)


@dataclasses.dataclass
class KoopmanModel:
    """The weight of a frame with features x is (x - mean_0) . u + const (`koopman_from_moments`, `frame_weights`)."""

    u: torch.Tensor          # [F] fp64 (numpy when the moments were numpy)
    const: float
    mean_0: torch.Tensor     # [F] fp64
    eigenvalue: float        # the eigenvalue of the Koopman matrix the weights belong to: 1 up to rounding


def moments_accumulator(n_features: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(acc, pair count, workspace) for `accumulate_moments`: zeroed fp64 [2 F + 3 F^2], zeroed int64 [1], the kernel's scratch."""
    F = int(n_features)
    ws_len = int(_lib.load().tw_lagged_moments_workspace_len(F))
    if ws_len < 0:
        _lib.check(-1, f"tw_lagged_moments_workspace_len (n_features {F}: 1 .. 1024)")
    return (torch.zeros(2 * F + 3 * F * F, dtype=torch.float64, device=device), torch.zeros(1, dtype=torch.int64, device=device),
            torch.empty(ws_len, dtype=torch.float64, device=device))


def accumulate_moments(X: torch.Tensor, lag: int, acc: torch.Tensor, count: torch.Tensor, workspace: torch.Tensor) -> None:
    """One `tw_lagged_moments` call: the pairs of X [n_chains, T, F] (float32, device) are added into acc / count."""
    X = _lib.require_gpu_tensor(X, torch.float32, "X")
    n_chains, T, F = X.shape
    with torch.cuda.device(X.device):
        _lib.check(_lib.load().tw_lagged_moments(X.data_ptr(), n_chains, T, F, int(lag), acc.data_ptr(), count.data_ptr(),
                                                 workspace.data_ptr(), _lib.stream_ptr(X.device)), "tw_lagged_moments")


def accumulate_moments_weighted(X: torch.Tensor, weights: torch.Tensor, lag: int, acc: torch.Tensor, count: torch.Tensor,
                                sum_w: torch.Tensor, workspace: torch.Tensor) -> None:
    """One `tw_lagged_moments_weighted` call: the pairs of X [n_chains, T, F], each times weights [n_chains, T] (fp64, device) at its
    first frame, are added into acc / count, and the pairs' weights into sum_w (fp64 [1], device)."""
    X = _lib.require_gpu_tensor(X, torch.float32, "X")
    weights = _lib.require_gpu_tensor(weights, torch.float64, "weights")
    n_chains, T, F = X.shape
    if tuple(weights.shape) != (n_chains, T):
        raise ValueError(f"weights {tuple(weights.shape)}: expected [n_chains, T] = {(n_chains, T)}")
    with torch.cuda.device(X.device):
        _lib.check(_lib.load().tw_lagged_moments_weighted(X.data_ptr(), weights.data_ptr(), n_chains, T, F, int(lag), acc.data_ptr(),
                                                          count.data_ptr(), sum_w.data_ptr(), workspace.data_ptr(),
                                                          _lib.stream_ptr(X.device)), "tw_lagged_moments_weighted")


def _accumulate_moments_torch(X: torch.Tensor, lag: int, acc: torch.Tensor, count: torch.Tensor,
                              weights: Optional[torch.Tensor] = None, sum_w: Optional[torch.Tensor] = None) -> None:
    """The same sums through float64 casts of the lagged slices and torch.matmul (no fixed summation order)."""
    n_chains, T, F = X.shape
    x = X[:, : T - lag].double().reshape(-1, F)
    y = X[:, lag:].double().reshape(-1, F)
    xa, ya = x, y       # the row operands, weighted when there are weights
    if weights is not None:
        w = weights[:, : T - lag].reshape(-1, 1)
        xa, ya = x * w, y * w
        sum_w += w.sum()
    acc[:F] += xa.sum(0)
    acc[F:2 * F] += ya.sum(0)
    FF = F * F
    acc[2 * F:2 * F + FF] += (xa.T @ x).reshape(-1)
    acc[2 * F + FF:2 * F + 2 * FF] += (xa.T @ y).reshape(-1)
    acc[2 * F + 2 * FF:] += (ya.T @ y).reshape(-1)
    count += x.shape[0]


def project(X, projection, mean=None, offset=None):
    """`tw_project`: offset + (X - mean) @ projection in fp64, every row on its own and in ascending feature order, for X [..., F]
    float32 (numpy or a device tensor), projection [F, k] (1 <= k <= 64), mean [F] and offset [k] (None: zeros).  Returns
    [..., k] fp64 - a device tensor for a device tensor, numpy for numpy."""
    x, was_numpy = _device_coords(X)
    F = int(x.shape[-1])
    up = lambda a: None if a is None else torch.as_tensor(a).to(device=x.device, dtype=torch.float64).contiguous()
    P, m, b = up(projection), up(mean), up(offset)
    if P.dim() != 2 or P.shape[0] != F:
        raise ValueError(f"projection {tuple(P.shape)}: expected [F, k] with F = {F}")
    k = int(P.shape[1])
    if (m is not None and tuple(m.shape) != (F,)) or (b is not None and tuple(b.shape) != (k,)):
        raise ValueError(f"mean [F] = [{F}] and offset [k] = [{k}] expected")
    rows = x.reshape(-1, F)
    out = torch.empty((rows.shape[0], k), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().tw_project(rows.data_ptr(), None if m is None else m.data_ptr(), P.data_ptr(),
                                          None if b is None else b.data_ptr(), out.data_ptr(), rows.shape[0], F, k,
                                          _lib.stream_ptr(x.device)), "tw_project")
    out = out.reshape(*x.shape[:-1], k)
    return out.cpu().numpy() if was_numpy else out


def _chunk_features(data, start: int, stop: int, tables) -> torch.Tensor:
    """Frames start .. stop - 1 of every chain as device features [n_chains, stop - start, F]: uploaded if numpy, featurised if
    `tables` (of `feature_tables`) are given."""
    piece, _ = _device_coords(data[:, start:stop])
    if tables is not None:
        piece = features_from_tables(piece.reshape(-1, piece.shape[-2], 3), *tables).reshape(piece.shape[0], piece.shape[1], -1)
    return piece


def _project_chunked(data, topology, projection, mean, offset, chunk_frames: int, feature_options: dict):
    """`project` over [n_chains, T, F] features or, with `topology`, [n_chains, T, V, 3] coordinates, `chunk_frames` frames at a
    time, so the features of a long trajectory are never held whole.  [n_chains, T, k] fp64."""
    was_numpy = not isinstance(data, torch.Tensor)
    want = 3 if topology is None else 4
    if len(data.shape) != want:
        raise ValueError(f"expected {'features [n_chains, T, F]' if topology is None else 'coords [n_chains, T, V, 3]'}")
    tables = None if topology is None else feature_tables(topology, **feature_options)
    T = int(data.shape[1])
    parts = [project(_chunk_features(data, start, min(start + chunk_frames, T), tables), projection, mean, offset)
             for start in range(0, T, int(chunk_frames))]
    out = torch.cat(parts, dim=1)
    return out.cpu().numpy() if was_numpy else out


def frame_weights(features_or_coords, model: KoopmanModel, topology: Optional[Topology] = None, chunk_frames: int = 16384,
                  **feature_options):
    """The Koopman weight (x - mean_0) . u + const of every frame, fp64 [n_chains, T], through `tw_project` with k = 1.  Input as
    for `lagged_moments`: features [n_chains, T, F], or coordinates [n_chains, T, V, 3] with `topology`."""
    u = torch.as_tensor(model.u, dtype=torch.float64).reshape(-1, 1)
    return _project_chunked(features_or_coords, topology, u, model.mean_0, [float(model.const)], chunk_frames, feature_options)[..., 0]


def lagged_moments(features_or_coords, lag: int, chunk_frames: int = 16384, topology: Optional[Topology] = None,
                   route: Optional[str] = None, weights=None, **feature_options) -> Moments:
    """The time-lagged second moments of a trajectory, walked in chunks of `chunk_frames` frames so that neither the features of a
    long trajectory nor their fp64 casts are ever held whole.

    Without `topology` the input is features [n_chains, T, F]; with it, coordinates [n_chains, T, V, 3], and each chunk is
    featurised (`tica_features` with `feature_options`) just before its moments are taken.  Consecutive chunks overlap by `lag`
    frames: chunk k holds the frames k chunk_frames .. (k + 1) chunk_frames + lag - 1, so it owns exactly the pairs whose first
    frame is in k chunk_frames .. (k + 1) chunk_frames - 1 - no pair is lost and none is counted twice.  numpy input is uploaded
    chunk by chunk and the result comes back as numpy.  `route`: see MOMENTS_ROUTES.

    `weights`: None - the plain sums; a tensor or array [n_chains, T] - the weight of the pair (c, t) is weights[c, t]
    (`tw_lagged_moments_weighted`; the last `lag` weights of a chain pair with nothing); a `KoopmanModel` - the weights of each
    chunk are computed from its features just before they are used (`tw_project`, k = 1), so they are never held whole either.
    Weighted moments carry `sum_w`."""
    route = DEFAULT_MOMENTS_ROUTE if route is None else route
    if route not in MOMENTS_ROUTES:
        raise ValueError(f"route {route!r}: one of {MOMENTS_ROUTES}")
    was_numpy = not isinstance(features_or_coords, torch.Tensor)
    data = features_or_coords
    want = 3 if topology is None else 4
    if len(data.shape) != want:
        raise ValueError(f"expected {'features [n_chains, T, F]' if topology is None else 'coords [n_chains, T, V, 3]'}")
    T, lag, chunk_frames = int(data.shape[1]), int(lag), int(chunk_frames)
    if not 1 <= lag < T:
        raise ValueError(f"lag {lag}: 1 .. T - 1 = {T - 1}")
    if chunk_frames < 1:
        raise ValueError("chunk_frames must be positive")
    tables = None if topology is None else feature_tables(topology, **feature_options)
    if weights is not None:
        return _lagged_moments_weighted(data, lag, chunk_frames, tables, route, weights, was_numpy)
    acc = count = ws = None
    F = 0
    for start in range(0, T - lag, chunk_frames):
        piece = _chunk_features(data, start, min(start + chunk_frames + lag, T), tables)
        if acc is None:
            F = int(piece.shape[-1])
            if route == "kernel":
                acc, count, ws = moments_accumulator(F, piece.device)
            else:
                acc = torch.zeros(2 * F + 3 * F * F, dtype=torch.float64, device=piece.device)
                count = torch.zeros(1, dtype=torch.int64, device=piece.device)
        if route == "kernel":
            accumulate_moments(piece, lag, acc, count, ws)
        else:
            _accumulate_moments_torch(piece, lag, acc, count)
    FF = F * F
    parts = [acc[:F], acc[F:2 * F], acc[2 * F:2 * F + FF].reshape(F, F), acc[2 * F + FF:2 * F + 2 * FF].reshape(F, F),
             acc[2 * F + 2 * FF:].reshape(F, F)]
    if was_numpy:
        parts = [p.cpu().numpy() for p in parts]
    return Moments(int(count.item()), lag, *parts)


def _lagged_moments_weighted(data, lag: int, chunk_frames: int, tables, route: str, weights, was_numpy: bool) -> Moments:
    """`lagged_moments` with weights: the same walk over the same chunks, each with its slice of the weights."""
    T = int(data.shape[1])
    model = weights if isinstance(weights, KoopmanModel) else None
    if model is None and tuple(weights.shape) != (int(data.shape[0]), T):
        raise ValueError(f"weights {tuple(weights.shape)}: expected [n_chains, T] = {(int(data.shape[0]), T)}")
    acc = count = ws = sum_w = None
    F = 0
    for start in range(0, T - lag, chunk_frames):
        stop = min(start + chunk_frames + lag, T)
        piece = _chunk_features(data, start, stop, tables)
        if acc is None:
            F = int(piece.shape[-1])
            acc, count, ws = moments_accumulator(F, piece.device) if route == "kernel" else \
                (torch.zeros(2 * F + 3 * F * F, dtype=torch.float64, device=piece.device),
                 torch.zeros(1, dtype=torch.int64, device=piece.device), None)
            sum_w = torch.zeros(1, dtype=torch.float64, device=piece.device)
            if model is not None:
                ku = torch.as_tensor(model.u, dtype=torch.float64).reshape(-1, 1)
        if model is not None:
            w = project(piece, ku, model.mean_0, [float(model.const)])[..., 0]
        else:
            w = torch.as_tensor(weights[:, start:stop]).to(device=piece.device, dtype=torch.float64).contiguous()
        if route == "kernel":
            accumulate_moments_weighted(piece, w, lag, acc, count, sum_w, ws)
        else:
            _accumulate_moments_torch(piece, lag, acc, count, w, sum_w)
    FF = F * F
    parts = [acc[:F], acc[F:2 * F], acc[2 * F:2 * F + FF].reshape(F, F), acc[2 * F + FF:2 * F + 2 * FF].reshape(F, F),
             acc[2 * F + 2 * FF:].reshape(F, F)]
    if was_numpy:
        parts = [p.cpu().numpy() for p in parts]
    return Moments(int(count.item()), lag, *parts, sum_w=float(sum_w.item()))


def tica_from_moments(moments: Moments, dim: int, eps: float = 1e-6):
    """TICA from the sums, with the symmetrised (reversible) estimator: with N pairs (for weighted moments N = sum w and every sum is
    the weighted one) and the mean m = (sum x + sum y) / 2N,
        C0 = (sum x x^T + sum y y^T) / 2N - m m^T,        Ctau = (sum x y^T + (sum x y^T)^T) / 2N - m m^T.
    C0 is whitened on its eigenvectors whose eigenvalue exceeds eps times the largest (a rank-deficient C0 loses those directions
    and raises nothing); the whitened Ctau is diagonalised.  Both eigen-solves are torch.linalg.eigh in fp64.

    Returns (eigenvalues [k] descending, projection [F, k], mean [F]), k = min(dim, kept directions): the TICs of a feature vector
    f are (f - mean) @ projection.  deeptime's Koopman reweighting, which the reference applies before TICA, is what weighted
    moments carry (`koopman_from_moments`, `run_tica`)."""
    as_t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    n = float(moments.n_pairs) if moments.sum_w is None else float(moments.sum_w)
    sx, sy, cxx, cxy, cyy = (as_t(a) for a in (moments.sum_x, moments.sum_y, moments.c_xx, moments.c_xy, moments.c_yy))
    mean = (sx + sy) / (2.0 * n)
    mm = torch.outer(mean, mean)
    c0 = (cxx + cyy) / (2.0 * n) - mm
    ct = (cxy + cxy.T) / (2.0 * n) - mm
    c0 = 0.5 * (c0 + c0.T)
    lam, u = torch.linalg.eigh(c0)
    keep = lam > eps * lam.max()
    w = u[:, keep] / torch.sqrt(lam[keep])
    m = w.T @ ct @ w
    ev, v = torch.linalg.eigh(0.5 * (m + m.T))
    order = torch.argsort(ev, descending=True)[:dim]
    return ev[order], w @ v[:, order], mean


def koopman_from_moments(moments: Moments, eps: float = 1e-6) -> KoopmanModel:
    """The Koopman reweighting of short off-equilibrium chains, from the plain (not symmetrised) moments.  With N the normaliser,
        mean_0 = sum x / N,  mean_t = sum y / N,  C00 = sum x x^T / N - mean_0 mean_0^T,  C0t = sum x y^T / N - mean_0 mean_t^T,
    R the whitening of C00 on its eigenvectors whose eigenvalue exceeds eps times the largest (a rank-deficient C00 loses those
    directions and raises nothing - the rule of `tica_from_moments`), the Koopman matrix in the whitened basis with a constant
    function appended is
        K = [[R^T C0t R, 0], [(mean_t - mean_0) R, 1]].
    u^ is its LEFT eigenvector whose eigenvalue is nearest 1, scaled so that its last entry is 1; u = R u^[:-1], const = u^[-1],
    and the weight of a frame with features x is (x - mean_0) . u + const: the ratio of the stationary density to the density the
    frames were drawn from, in the span of the features.  Its mean over the x frames is const = 1.

    This is deeptime's KoopmanWeightingEstimator RESTATED FROM MEMORY.  It is not pinned against deeptime, which is not available
    here.  One known difference: deeptime cuts the spectrum of C00 at an absolute epsilon, this at one relative to the largest
    eigenvalue.  C00's eigen-solve is torch.linalg.eigh where the moments are; K is not symmetric, and its eigen-solve
    (torch.linalg.eig, fp64) runs on the host."""
    was_numpy = not isinstance(moments.sum_x, torch.Tensor)
    as_t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    n = moments.normaliser
    sx, sy, cxx, cxy = (as_t(a) for a in (moments.sum_x, moments.sum_y, moments.c_xx, moments.c_xy))
    mean_0, mean_t = sx / n, sy / n
    c00 = cxx / n - torch.outer(mean_0, mean_0)
    c0t = cxy / n - torch.outer(mean_0, mean_t)
    c00 = 0.5 * (c00 + c00.T)
    lam, v = torch.linalg.eigh(c00)
    keep = lam > eps * lam.max()
    R = v[:, keep] / torch.sqrt(lam[keep])
    r = R.shape[1]
    K = torch.zeros((r + 1, r + 1), dtype=torch.float64, device=R.device)
    K[:r, :r] = R.T @ c0t @ R
    K[r, :r] = (mean_t - mean_0) @ R
    K[r, r] = 1.0
    ev, vec = torch.linalg.eig(K.T.cpu())          # columns: the left eigenvectors of K
    i = int(torch.argmin((ev - 1.0).abs()))
    uh = (vec[:, i] / vec[r, i]).real.to(R.device)
    u = R @ uh[:r]
    if was_numpy:
        u, mean_0 = u.cpu().numpy(), mean_0.cpu().numpy()
    return KoopmanModel(u=u, const=float(uh[r]), mean_0=mean_0, eigenvalue=float(ev[i].real))


@dataclasses.dataclass
class TicaModel:
    """What `run_tica` fits: the TICs of a feature vector f are (f - mean) @ projection (`transform`)."""

    eigenvalues: torch.Tensor            # [k] descending (numpy when the input was numpy, as are the next three)
    projection: torch.Tensor             # [F, k]
    mean: torch.Tensor                   # [F]
    timescales: torch.Tensor             # [k]  -lag / ln |eigenvalue|, in frames
    koopman: Optional[KoopmanModel]      # the reweighting the moments were taken with; None for the plain estimator
    lag: int
    topology: Optional[Topology] = None  # set when the model was fitted on coordinates: `transform` then takes coordinates
    feature_options: dict = dataclasses.field(default_factory=dict)

    def transform(self, features_or_coords, chunk_frames: int = 16384):
        """The TICs [..., k] fp64 through `tw_project`: of features [..., F], or - for a model fitted on coordinates - of
        coordinates [..., V, 3], featurised `chunk_frames` frames at a time."""
        data = features_or_coords
        lead = tuple(data.shape[:-1] if self.topology is None else data.shape[:-2])
        flat = data.reshape(1, -1, *data.shape[len(lead):])
        out = _project_chunked(flat, self.topology, self.projection, self.mean, None, chunk_frames, self.feature_options)
        return out.reshape(*lead, out.shape[-1])


def run_tica(features_or_coords, lagtime: int = 500, dim: int = 40, topology: Optional[Topology] = None, koopman: bool = True,
             chunk_frames: int = 16384, **feature_options) -> TicaModel:
    """utils/tica_utils.py:40-46 on the device.  Input as for `lagged_moments`.  koopman=True, the reference's way, walks the
    trajectory twice: plain moments give the Koopman weights (`koopman_from_moments`), moments weighted with them give the TICA
    (`tica_from_moments`) - on many short chains started from one state the plain estimator is biased towards the start
    distribution and its eigenvalues come out too small.  koopman=False is `lagged_moments` + `tica_from_moments` and nothing else.

    The moments stay on the device whatever the input is, so the eigen-solves run there and numpy input gives the bits device
    input gives; the model's arrays come back as numpy for numpy input.  deeptime's kinetic_map scaling is not applied."""
    was_numpy = not isinstance(features_or_coords, torch.Tensor)
    lag = int(lagtime)

    def moments(weights):
        m = lagged_moments(features_or_coords, lag, chunk_frames=chunk_frames, topology=topology, weights=weights, **feature_options)
        if was_numpy:   # back to where they were summed
            for key in ("sum_x", "sum_y", "c_xx", "c_xy", "c_yy"):
                setattr(m, key, torch.as_tensor(getattr(m, key)).to("cuda"))
        return m

    model = koopman_from_moments(moments(None)) if koopman else None
    ev, proj, mean = tica_from_moments(moments(model), dim)
    ts = -float(lag) / torch.log(ev.abs())
    if was_numpy:
        ev, proj, mean, ts = (a.cpu().numpy() for a in (ev, proj, mean, ts))
        if model is not None:
            model = dataclasses.replace(model, u=model.u.cpu().numpy(), mean_0=model.mean_0.cpu().numpy())
    return TicaModel(ev, proj, mean, ts, model, lag, topology, dict(feature_options))


def autocorrelation(series, max_lag: int) -> torch.Tensor:
    """rho [max_lag + 1, n_obs] fp64 of series [n_chains, T, n_obs]: chains centred on the POOLED mean, the biased autocovariance
    gamma_k = (1 / T) sum_t z_t z_{t+k} per chain through torch.fft (zero-padded to at least 2 T, so nothing wraps around),
    averaged over chains, divided by gamma_0.  A constant observable has gamma_0 = 0 and gives NaN."""
    s = torch.as_tensor(series).to(torch.float64)
    if s.dim() != 3:
        raise ValueError("series: [n_chains, T, n_obs]")
    T = s.shape[1]
    if not 0 <= max_lag < T:
        raise ValueError(f"max_lag {max_lag}: 0 .. T - 1 = {T - 1}")
    z = s - s.mean(dim=(0, 1), keepdim=True)
    n = 1 << (2 * T - 1).bit_length()
    f = torch.fft.rfft(z, n=n, dim=1)
    gamma = torch.fft.irfft(f.real ** 2 + f.imag ** 2, n=n, dim=1)[:, : max_lag + 1].mean(dim=0) / T
    return gamma / gamma[:1]


def geyer_tau(rho: torch.Tensor) -> torch.Tensor:
    """1 + 2 sum_{k >= 1} rho_k truncated by Geyer's initial positive sequence, for rho [L, n_obs] with rho[0] = 1: the pairs
    rho_2m + rho_2m+1 (m = 0, 1, ...) are summed while the pair sum stays positive; tau = 2 (sum of those pairs) - 1."""
    rho = torch.as_tensor(rho, dtype=torch.float64)
    L = rho.shape[0] // 2 * 2
    pairs = rho[:L].reshape(L // 2, 2, *rho.shape[1:]).sum(dim=1)
    live = torch.cumprod((pairs > 0).to(torch.float64), dim=0)
    return 2.0 * (pairs * live).sum(dim=0) - 1.0


def effective_sample_size(series, circular: bool = False, max_lag: Optional[int] = None) -> torch.Tensor:
    """ESS [n_obs] fp64 of series [n_chains, T, n_obs]: N / (1 + 2 sum rho_k), N = n_chains T, the sum truncated by Geyer's initial
    positive sequence (`geyer_tau`).  circular=True (angles): the smaller of the ESS of the sine and of the cosine.  A constant
    observable has no autocorrelation: its ESS is NaN, with a warning."""
    s = torch.as_tensor(series)
    if circular:
        return torch.minimum(effective_sample_size(torch.sin(s.double()), False, max_lag),
                             effective_sample_size(torch.cos(s.double()), False, max_lag))
    n_chains, T = s.shape[0], s.shape[1]
    rho = autocorrelation(s, T - 1 if max_lag is None else min(int(max_lag), T - 1))
    ess = (n_chains * T) / geyer_tau(rho)
    constant = torch.isnan(rho[0])
    if bool(constant.any()):
        warnings.warn(f"effective_sample_size: {int(constant.sum())} constant observable(s): ESS is NaN there", RuntimeWarning)
        ess = torch.where(constant, torch.full_like(ess, float("nan")), ess)
    return ess


def ramachandran_histogram(phi, psi, bins: int = 100) -> torch.Tensor:
    """Counts [bins, bins] (int64; first axis phi) of the angle pairs over [-pi, pi]^2: a bin index per sample, then bincount."""
    phi, psi = torch.as_tensor(phi).reshape(-1).double(), torch.as_tensor(psi).reshape(-1).double()
    idx = lambda a: torch.clamp(torch.floor((a + torch.pi) / (2 * torch.pi) * bins).long(), 0, bins - 1)
    return torch.bincount(idx(phi) * bins + idx(psi), minlength=bins * bins).reshape(bins, bins)


def free_energy(hist) -> torch.Tensor:
    """-log(h / h.max()) as in utils/tica_utils.py:59-61 (empty bins give +inf)."""
    h = torch.as_tensor(hist).double()
    return -torch.log(h / h.max())


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m timewarp_amd.analysis", description="Torsions, ESS and TICA of a *-traj-arrays.npz")
    p.add_argument("trajectory", help="*-traj-arrays.npz with `positions` [T, V, 3] (nm), as simulation.py writes it")
    p.add_argument("--pdb", required=True, help="the trajectory's state0 PDB (topology)")
    p.add_argument("--lag", type=int, default=500, help="TICA lag time in frames")
    p.add_argument("--dim", type=int, default=10, help="TICA dimensions kept")
    p.add_argument("--max-lag", type=int, default=None, help="longest lag of the autocorrelation behind the ESS (default T - 1)")
    p.add_argument("--chunk-frames", type=int, default=16384)
    p.add_argument("--koopman", action="store_true",
                   help="Koopman-reweight the frames before TICA, as the reference's run_tica does; adds koopman_u, koopman_const, "
                        "koopman_mean, frame_weights and tica_timescales to the output")
    p.add_argument("--out", default=None, help="output file (default <name>-analysis.npz next to the trajectory)")
    return p


def output_path(trajectory: str) -> str:
    stem = os.path.basename(trajectory)
    for suffix in ("-traj-arrays.npz", ".npz"):
        if stem.endswith(suffix):
            stem = stem[: -len(suffix)]
            break
    return os.path.join(os.path.dirname(trajectory), stem + "-analysis.npz")


def main(argv=None) -> str:
    args = build_parser().parse_args(argv)
    with np.load(args.trajectory) as z:
        positions = np.ascontiguousarray(z["positions"], dtype=np.float32)
    if positions.ndim != 3:
        raise SystemExit(f"positions: expected [T, V, 3], got {positions.shape}")
    T = positions.shape[0]
    if not 1 <= args.lag < T:
        raise SystemExit(f"--lag {args.lag}: the trajectory has {T} frames, so 1 .. {T - 1}")
    coords = torch.as_tensor(positions).to("cuda")[None]            # one chain
    tors = compute_torsions(coords, args.pdb)
    result = {}
    for f in FAMILIES:
        ang = getattr(tors, f)
        result[f] = ang[0].cpu().numpy()
        result[f + "_indices"] = getattr(tors, f + "_indices")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            result["ess_" + f] = (effective_sample_size(ang, circular=True, max_lag=args.max_lag).cpu().numpy() if ang.shape[-1]
                                  else np.zeros(0))
    if args.koopman:
        model = run_tica(coords, lagtime=args.lag, dim=args.dim, topology=args.pdb, koopman=True, chunk_frames=args.chunk_frames)
        ev, proj, mean, km = model.eigenvalues, model.projection, model.mean, model.koopman
        result.update(koopman_u=km.u.cpu().numpy(), koopman_const=np.float64(km.const), koopman_mean=km.mean_0.cpu().numpy(),
                      frame_weights=frame_weights(coords, km, topology=args.pdb, chunk_frames=args.chunk_frames)[0].cpu().numpy(),
                      tica_timescales=model.timescales.cpu().numpy())
        n_pairs = T - args.lag
    else:
        moments = lagged_moments(coords, args.lag, chunk_frames=args.chunk_frames, topology=args.pdb)
        ev, proj, mean = tica_from_moments(moments, args.dim)
        n_pairs = moments.n_pairs
    tics = []
    for start in range(0, T, args.chunk_frames):
        feats = tica_features(coords[0, start:start + args.chunk_frames], args.pdb)
        tics.append(((feats.double() - mean) @ proj[:, :2]).cpu().numpy())
    result.update(tica_eigenvalues=ev.cpu().numpy(), tica_projection=proj.cpu().numpy(), tica_mean=mean.cpu().numpy(),
                  tics=np.concatenate(tics, axis=0), lag=np.int64(args.lag), n_pairs=np.int64(n_pairs))
    out = args.out or output_path(args.trajectory)
    np.savez(out, **result)
    print(f"{out}: {T} frames, " + ", ".join(f"{f} {result[f].shape[-1]}" for f in FAMILIES)
          + f"; TICA lag {args.lag}: eigenvalues {np.array2string(result['tica_eigenvalues'][:4], precision=4)}")
    return out


if __name__ == "__main__":
    main()
