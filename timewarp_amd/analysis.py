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
  `coverage_distance`, `first_zero_ess`, `ess_per_sample`, `speedup_report`, `load_model_chain`, `load_exploration`,
  `acceptance_from_thinned`             notebooks/Paper/speed-up-mcmc.ipynb cells 4, 7, 8 and speed-up-exploration.ipynb cell 4: the
                                        speed-up over MD behind its all-states-found check (command line: `timewarp_amd.speedup`)

Hot paths are HIP kernels (csrc/tw_analysis.hip: `tw_dihedrals`, `tw_tica_features`, `tw_lagged_moments`,
`tw_lagged_moments_weighted`, `tw_project`, `tw_cloud_coverage`); there is no host fallback for them.  The eigen-solves, the FFT and the histograms are
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


def ramachandran_histograms(phi, psi, residue_pairs, bins=100, route: Optional[str] = None, chunk_rows: Optional[int] = None):
    """hist2d(phi[:, i], psi[:, j], bins) of every (i, j) of `residue_pairs` in ONE call: `evaluate.joint_histograms` (an
    `evaluate.JointHistograms`; counts [n_pairs, bins, bins] int64, first axis phi) of phi [T, n_phi] and psi [T, n_psi] float32,
    numpy or tensors.  The edges are np.linspace(-p, p, bins + 1) with p = float32(pi), the largest angle a float32 atan2 returns
    (it lies above the fp64 pi), so every finite angle is inside; NaN angles are counted in `outside[:, 2]`.  The bin rule is the
    one of every histogram of evaluate.py - not `ramachandran_histogram`'s floor of a scaled angle, from which it differs for an
    angle exactly on an edge.  `route`: evaluate.JOINT_ROUTES."""
    from . import evaluate

    as_tensor = lambda a: a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float32))
    phi, psi = as_tensor(phi), as_tensor(psi)
    if phi.dim() != 2 or psi.dim() != 2 or phi.shape[0] != psi.shape[0]:
        raise ValueError(f"phi {tuple(phi.shape)} and psi {tuple(psi.shape)}: expected [T, n_phi] and [T, n_psi] of one trajectory")
    n_phi, n_psi = int(phi.shape[1]), int(psi.shape[1])
    rp = np.asarray(residue_pairs, dtype=np.int64).reshape(-1, 2)
    if rp.size and (rp[:, 0].min() < 0 or rp[:, 0].max() >= n_phi or rp[:, 1].min() < 0 or rp[:, 1].max() >= n_psi):
        raise ValueError(f"residue_pairs: (phi column, psi column) in 0 .. {n_phi - 1} and 0 .. {n_psi - 1}")
    angles = torch.cat([phi.to(torch.float32), psi.to(phi.device).to(torch.float32)], dim=1)
    pairs = np.stack([rp[:, 0], n_phi + rp[:, 1]], axis=1)
    p = float(np.float32(np.pi))
    return evaluate.joint_histograms(angles, pairs, bins=bins, range=((-p, p), (-p, p)), route=route, chunk_rows=chunk_rows)


def free_energy(hist) -> torch.Tensor:
    """-log(h / h.max()) as in utils/tica_utils.py:59-61 (empty bins give +inf)."""
    h = torch.as_tensor(hist).double()
    return -torch.log(h / h.max())


# ---- the speed-up report of notebooks/Paper/speed-up-mcmc.ipynb (cell 8) and speed-up-exploration.ipynb (cell 4) ------------------------

# The routes `coverage_distance` can take.  "kernel": tw_cloud_coverage - one tiled pass with a running minimum, nothing stored per
# pair, bit-reproducible.  "torch": torch.cdist on chunks of both clouds (the direct form, not the matmul one, whose cancellation
# loses small distances) - kept for comparison, and the only route that runs without a GPU.  The default is the one that measured
# faster on the MI355X at the notebook's unthinned sizes (profiles/coverage.txt).
COVERAGE_ROUTES = ("kernel", "torch")
DEFAULT_COVERAGE_ROUTE = "kernel"
COVERAGE_MAX_DIM = 8


def _coverage_kernel(ref: torch.Tensor, cloud: torch.Tensor, n_groups: int, want_min: bool):
    """One `tw_cloud_coverage` call on fp64 device tensors [M, d], [N, d]: (worst [G], arg [G], min d^2 [G, M] or None)."""
    M, d = int(ref.shape[0]), int(ref.shape[1])
    N = int(cloud.shape[0])
    lib = _lib.load()
    need = int(lib.tw_cloud_coverage_workspace_bytes(M, N, d, n_groups))
    if need < 0:
        raise ValueError(f"coverage_distance: tw_cloud_coverage does not support n_ref {M}, n_cloud {N}, dim {d}, n_groups {n_groups} "
                         f"(1 <= dim <= {COVERAGE_MAX_DIM}, n_ref >= 1, n_groups >= 1)")
    dev = ref.device
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    worst = torch.empty(n_groups, dtype=torch.float64, device=dev)
    arg = torch.empty(n_groups, dtype=torch.int64, device=dev)
    min_d2 = torch.empty((n_groups, M), dtype=torch.float64, device=dev) if want_min else None
    with torch.cuda.device(dev):
        _lib.check(lib.tw_cloud_coverage(ref.data_ptr(), cloud.data_ptr() if N else None, M, N, d, n_groups, _lib.ptr(min_d2),
                                         worst.data_ptr(), arg.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr(dev)),
                   "tw_cloud_coverage")
    return worst, arg, min_d2


def _coverage_torch(ref: torch.Tensor, cloud: torch.Tensor, n_groups: int, chunk: int):
    """The same three results through torch.cdist on `chunk` x `chunk` blocks (the minima come back as DISTANCES [G, M]).  The
    direct form of cdist launches one workgroup of 256 threads per pair, and a launch holds fewer than 2^32 threads: chunk < 4096."""
    M = int(ref.shape[0])
    inf = float("inf")
    min_d = torch.full((n_groups, M), inf, dtype=torch.float64, device=ref.device)
    for g in range(n_groups):
        rows = cloud[g::n_groups]
        for a in range(0, M, chunk):
            for b in range(0, int(rows.shape[0]), chunk):
                d = torch.cdist(ref[a:a + chunk], rows[b:b + chunk], compute_mode="donot_use_mm_for_euclid_dist")
                min_d[g, a:a + chunk] = torch.minimum(min_d[g, a:a + chunk], d.min(dim=1).values)
    worst = min_d.max(dim=1).values
    index = torch.arange(M, device=ref.device).expand(n_groups, M)
    arg = torch.where(min_d == worst[:, None], index, M).min(dim=1).values      # the smallest index that attains the maximum
    return worst, arg, min_d


def coverage_distance(ref_tics, cloud_tics, dims: int = 2, n_groups: int = 1, normalise: bool = True, return_min: bool = False,
                      route: Optional[str] = None, chunk: int = 2048):
    """How far the reference cloud is from the sample cloud in the first `dims` TICs: for every group g of the cloud (row j belongs to
    group j % n_groups - explorer i of `exploration.explore` is rows i::P) the largest, over the reference points, of the distance to
    the nearest cloud point of the group.  With n_groups = 1 this is the notebooks'

        distance.cdist(ref / ranges, cloud / ranges).min(axis=1).max()

    ref_tics [M, >= dims], cloud_tics [N, >= dims].  normalise=True divides both by ranges = |ref_tics[:, :dims]|.max(0) in fp64 (the
    notebooks' division); a zero range is refused.  Non-finite TICs are refused before anything is computed.  Returns
    (worst [n_groups] fp64, arg [n_groups] int64 - the smallest reference row that attains it), with return_min=True also the
    distance of every reference point to its nearest cloud point [n_groups, M].  A group without rows gives +inf and arg 0.  Device
    tensors in, device tensors out; numpy in, numpy out.  `route`: see COVERAGE_ROUTES (`chunk` is the torch route's block edge)."""
    route = DEFAULT_COVERAGE_ROUTE if route is None else route
    if route not in COVERAGE_ROUTES:
        raise ValueError(f"route {route!r}: one of {COVERAGE_ROUTES}")
    dims, n_groups = int(dims), int(n_groups)
    if not 1 <= dims <= COVERAGE_MAX_DIM:
        raise ValueError(f"coverage_distance: dims {dims}: 1 .. {COVERAGE_MAX_DIM}")
    if n_groups < 1:
        raise ValueError(f"coverage_distance: n_groups {n_groups}: at least 1")
    if route == "torch" and not 1 <= int(chunk) < 4096:
        raise ValueError(f"coverage_distance: chunk {chunk}: 1 .. 4095 (see `_coverage_torch`)")
    was_numpy = not isinstance(ref_tics, torch.Tensor)
    ref, cloud = torch.as_tensor(ref_tics), torch.as_tensor(cloud_tics)
    for name, t in (("ref_tics", ref), ("cloud_tics", cloud)):
        if t.dim() != 2 or t.shape[1] < dims:
            raise ValueError(f"coverage_distance: {name} {tuple(t.shape)}: expected [rows, >= {dims}]")
    if ref.shape[0] < 1:
        raise ValueError("coverage_distance: ref_tics has no rows")
    if route == "kernel":
        if not torch.cuda.is_available():
            raise RuntimeError("timewarp_amd.analysis: tw_cloud_coverage runs on an MI355X; no GPU is visible and there is no CPU "
                               "fallback (route='torch' is the restatement)")
        dev = ref.device if ref.is_cuda else torch.device("cuda", torch.cuda.current_device())
        ref, cloud = ref.to(dev), cloud.to(dev)
    else:
        cloud = cloud.to(ref.device)
    ref = ref[:, :dims].to(torch.float64)
    cloud = cloud[:, :dims].to(torch.float64)
    for name, t in (("ref_tics", ref), ("cloud_tics", cloud)):
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"coverage_distance: {name} holds non-finite values")
    if normalise:
        ranges = ref.abs().max(dim=0).values
        if bool((ranges == 0).any()):
            raise ValueError(f"coverage_distance: zero range in TIC {int(torch.nonzero(ranges == 0)[0])}: ref_tics is constant there "
                             "and cannot be normalised")
        ref, cloud = ref / ranges, cloud / ranges
    ref, cloud = ref.contiguous(), cloud.contiguous()
    if route == "kernel":
        worst, arg, min_d2 = _coverage_kernel(ref, cloud, n_groups, return_min)
        min_d = torch.sqrt(min_d2) if return_min else None
    else:
        worst, arg, min_d = _coverage_torch(ref, cloud, n_groups, int(chunk))
    out = (worst, arg, min_d) if return_min else (worst, arg)
    return tuple(t.cpu().numpy() for t in out) if was_numpy else out


def first_zero_ess(rho, names: Optional[Sequence[str]] = None) -> torch.Tensor:
    """The notebooks' `ESS(autocorrelations)`: 1 / (-1 + 2 sum_{j < k} |rho_j|), k the first lag with rho_k <= 0 - the effective
    samples PER SAMPLE of a chain whose autocorrelation is rho [L] or [L, n_obs] (fp64 [] or [n_obs]).  An observable whose rho never
    reaches zero within L lags raises ValueError naming it (`names`, else its index); the notebooks' version raises IndexError
    there.  `effective_sample_size` (Geyer's initial positive sequence) is another estimator and is not used by the report."""
    rho = torch.as_tensor(rho, dtype=torch.float64)
    flat = rho.reshape(rho.shape[0], -1)
    crossed = flat <= 0
    never = ~crossed.any(dim=0)
    if bool(never.any()):
        bad = [str(names[i]) if names is not None else f"observable {i}" for i in torch.nonzero(never).reshape(-1).tolist()]
        raise ValueError(f"first_zero_ess: the autocorrelation of {', '.join(bad)} never reaches zero within {rho.shape[0]} lags")
    k = crossed.to(torch.int64).argmax(dim=0)                                        # the first True
    live = torch.arange(flat.shape[0], device=flat.device)[:, None] < k[None, :]
    ess = 1.0 / (-1.0 + 2.0 * (flat.abs() * live).sum(dim=0))
    return ess.reshape(rho.shape[1:])


def ess_per_sample(series, estimator: str = "first-zero", max_lag: Optional[int] = None, names: Optional[Sequence[str]] = None):
    """Effective samples per sample of ONE chain, series [T] or [T, n_obs].  "first-zero": `first_zero_ess` of `autocorrelation` -
    which for one chain is the definition arviz documents for `az.autocorr` (the biased autocovariance (1/T) sum_t z_t z_{t+k} of the
    centred series through an FFT, divided by its lag-0 value); nothing here claims equality with arviz's output, which is not
    available to compare against.  "geyer": `effective_sample_size` / T."""
    s = torch.as_tensor(series)
    squeeze = s.dim() == 1
    s = s.reshape(s.shape[0], -1)[None]
    T = s.shape[1]
    if estimator == "first-zero":
        out = first_zero_ess(autocorrelation(s, T - 1 if max_lag is None else min(int(max_lag), T - 1)), names)
    elif estimator == "geyer":
        out = effective_sample_size(s, max_lag=max_lag) / T
    else:
        raise ValueError(f"estimator {estimator!r}: 'first-zero' or 'geyer'")
    return out[0] if squeeze else out


def load_model_chain(directory: str, protein: str, stride: int = 1, drop_last: bool = False):
    """(positions [n, V, 3], seconds [n_segments]) of the chain `sample_trajectory` wrote to `directory`: the segments
    `sample_trajectory.segment_path(directory, protein, i)`, i = 0, 1, ... while they exist, each thinned by `stride`, concatenated.
    The notebooks read `len(os.listdir(directory)) - 1` segments - one fewer than there are when the directory holds nothing else;
    that is drop_last=True.  The default reads all of them."""
    from .sample_trajectory import segment_path

    if not os.path.isdir(directory):
        raise FileNotFoundError(f"load_model_chain: {directory} is not a directory")
    n = 0
    while os.path.exists(segment_path(directory, protein, n)):
        n += 1
    if drop_last:
        n -= 1
    if n < 1:
        raise FileNotFoundError(f"load_model_chain: no segments {os.path.basename(segment_path(directory, protein, 0))} ... in {directory}"
                                + (" after dropping the last" if drop_last else ""))
    positions, seconds = [], []
    for i in range(n):
        with np.load(segment_path(directory, protein, i)) as z:
            positions.append(z["positions"][::int(stride)])
            seconds.append(float(z["time"]))
    return np.concatenate(positions, axis=0), np.asarray(seconds, dtype=np.float64)


def load_exploration(path: str):
    """(positions [num_steps * P, V, 3], seconds) of the reference's `<protein>_exploration.npz` (keys `positions` and `time`)."""
    with np.load(path) as z:
        return np.asarray(z["positions"]), float(z["time"])


def acceptance_from_thinned(positions, thin: int = 10) -> float:
    """(number of distinct x[:, 0, 0] - 1) / len(x) / thin: the notebooks' estimate of the acceptance rate FROM THE SAVED FRAMES, every
    `thin`-th state of the chain - a frame that differs from the one before it stands for at least one accepted move.  It is not the
    chain's own counter (`MetropolisHastingsChain.result`), which counts every accepted proposal."""
    x = np.asarray(positions)
    return (len(np.unique(x[:, 0, 0])) - 1) / len(x) / int(thin)


@dataclasses.dataclass
class SpeedupReport:
    """What `speedup_report` returns.  Arrays are numpy."""

    coverage: float                  # the (best explorer's) largest distance from an MD point to its nearest model point, normalised TICs
    coverage_arg: int                # the MD frame (after md_stride) that is farthest from every model sample
    covered_fraction: float          # the share of MD points within `threshold` of the cloud
    threshold: float
    all_states_found: bool           # coverage < threshold
    ess_md: np.ndarray               # per sample, TIC 0 and TIC 1
    ess_model: np.ndarray
    speedup_tic0: float              # 0.0 when all_states_found is False
    speedup_tic1: float              # 0.0 for the grouped form, which reports TIC 0 only
    acceptance: Optional[float]      # `acceptance_from_thinned` of a model given as coordinates, else None
    eigenvalues: np.ndarray
    timescales: np.ndarray
    n_groups: int = 1
    best_group: int = 0
    group_coverage: Optional[np.ndarray] = None   # [n_groups]


def _run_tica_torch(features: torch.Tensor, lag: int, dim: int, koopman: bool, chunk_frames: int) -> TicaModel:
    """`run_tica` on features [1, T, F] with the torch moments and a matmul projection: what stands in for the kernels where the
    report runs without a GPU (route="torch")."""
    def moments(weights):
        X = features.to(torch.float32)
        F = X.shape[-1]
        acc = torch.zeros(2 * F + 3 * F * F, dtype=torch.float64, device=X.device)
        count = torch.zeros(1, dtype=torch.int64, device=X.device)
        sum_w = None if weights is None else torch.zeros(1, dtype=torch.float64, device=X.device)
        _accumulate_moments_torch(X, lag, acc, count, weights, sum_w)
        FF = F * F
        return Moments(int(count), lag, acc[:F], acc[F:2 * F], acc[2 * F:2 * F + FF].reshape(F, F),
                       acc[2 * F + FF:2 * F + 2 * FF].reshape(F, F), acc[2 * F + 2 * FF:].reshape(F, F),
                       sum_w=None if weights is None else float(sum_w))

    del chunk_frames  # one piece: this route is for small inputs
    model = weights = None
    if koopman:
        model = koopman_from_moments(moments(None))
        weights = (features.double() - model.mean_0) @ model.u + model.const
    ev, proj, mean = tica_from_moments(moments(weights), dim)
    return TicaModel(ev, proj, mean, -float(lag) / torch.log(ev.abs()), model, lag)


def speedup_report(md, model, *, topology: Optional[Topology] = None, lag: int = 100, dim: int = 40, koopman: bool = True,
                   md_seconds_per_frame: float, model_seconds_per_frame: float, n_groups: int = 1, threshold: Optional[float] = None,
                   md_stride: int = 1, cloud_stride: int = 1, chunk_frames: int = 16384, route: Optional[str] = None) -> SpeedupReport:
    """The speed-up of a sampler over MD, guarded by the check that the sampler found every state MD found: cell 8 of
    notebooks/Paper/speed-up-mcmc.ipynb (n_groups = 1) and cell 4 of speed-up-exploration.ipynb (n_groups = P).

    `md` and `model` are coordinates [T, V, 3] with `topology`, or features [T, F] without (the input rule of `run_tica`); numpy or
    device tensors.  TICA (`run_tica`, `lag`, `dim`, `koopman`) is fitted on `md`, both inputs are projected, and with
    ranges = |tics_md[::md_stride, :2]|.max(0)

        coverage = cdist(tics_md[::md_stride, :2] / ranges, tics_model[::cloud_stride, :2] / ranges).min(axis=1).max()

    through `coverage_distance`.  all_states_found = coverage < threshold; the effective samples per sample of TIC 0 and TIC 1 are
    `ess_per_sample` (the notebooks' first-zero estimator) of the UNTHINNED projections, and

        speedup_tic_k = (ess_model[k] / model_seconds_per_frame) / (ess_md[k] / md_seconds_per_frame),

    0.0 when a state is missing (the notebook's `[acceptance, 0, 0]`).  covered_fraction, the share of MD points within `threshold`
    of the cloud, is a softer reading next to the maximum, which the notebook itself calls conservative.

    n_groups = P: model row j belongs to explorer j % P.  The P coverages come from one call; the best explorer is the one with the
    lowest coverage (the lowest index on ties); ESS and speed-up of TIC 0 are taken on its rows model[best::P], and
    model_seconds_per_frame is the time of one frame of that explorer (the notebook's time / len(tics_model[best::P])).  The
    notebook stops at the first explorer below 0.1; taking the best of all is what it does when none is.  `cloud_stride` thins each
    explorer's rows, not the interleaved array.

    threshold defaults to 0.3 (n_groups = 1) and 0.1 (n_groups > 1), the notebooks' values.  md_stride and cloud_stride default to
    1: every point is compared, which the tiled kernel affords.  The notebooks take every tenth point of both clouds, because cdist
    holds the whole M x N matrix; md_stride=10, cloud_stride=10 reproduces that.  `route`: COVERAGE_ROUTES; "torch" also fits and
    projects with torch ops (features only) and so runs without a GPU."""
    n_groups = int(n_groups)
    if n_groups < 1:
        raise ValueError(f"speedup_report: n_groups {n_groups}: at least 1")
    if not (md_seconds_per_frame > 0 and model_seconds_per_frame > 0):
        raise ValueError("speedup_report: md_seconds_per_frame and model_seconds_per_frame must be positive")
    threshold = (0.3 if n_groups == 1 else 0.1) if threshold is None else float(threshold)
    route = DEFAULT_COVERAGE_ROUTE if route is None else route
    want = 2 if topology is None else 3
    for name, a in (("md", md), ("model", model)):
        if len(a.shape) != want:
            raise ValueError(f"speedup_report: {name}: expected {'features [T, F]' if topology is None else 'coords [T, V, 3]'}")
    if int(model.shape[0]) % n_groups:
        raise ValueError(f"speedup_report: model has {int(model.shape[0])} rows, not a multiple of n_groups {n_groups}")
    if route == "torch":
        if topology is not None:
            raise ValueError("speedup_report: route='torch' takes features; coordinates are featurised by the kernel route only")
        md_f, model_f = torch.as_tensor(md), torch.as_tensor(model)
        tica = _run_tica_torch(md_f[None], int(lag), int(dim), koopman, chunk_frames)
        project_ = lambda x: (x.double() - tica.mean) @ tica.projection
        tics_md, tics_model = project_(md_f), project_(model_f)
    else:
        tica = run_tica(md[None], lagtime=int(lag), dim=int(dim), topology=topology, koopman=koopman, chunk_frames=chunk_frames)
        tics_md = torch.as_tensor(tica.transform(md, chunk_frames=chunk_frames))
        tics_model = torch.as_tensor(tica.transform(model, chunk_frames=chunk_frames))
        if torch.cuda.is_available() and not tics_md.is_cuda:
            tics_md, tics_model = tics_md.to("cuda"), tics_model.to("cuda")
    if tics_md.shape[1] < 2:
        raise ValueError(f"speedup_report: TICA kept {tics_md.shape[1]} dimension(s); the report needs TIC 0 and TIC 1")
    ref = tics_md[::int(md_stride)]
    if n_groups == 1:
        cloud = tics_model[::int(cloud_stride)]
    else:   # thin every explorer's rows and keep the interleaving
        cloud = tics_model.reshape(-1, n_groups, tics_model.shape[1])[::int(cloud_stride)].reshape(-1, tics_model.shape[1])
    worst, arg, min_d = coverage_distance(ref, cloud, dims=2, n_groups=n_groups, normalise=True, return_min=True, route=route,
                                          chunk=2048)
    best = int(torch.where(worst == worst.min(), torch.arange(n_groups, device=worst.device), n_groups).min())
    coverage = float(worst[best])
    found = coverage < threshold
    names = ("TIC 0", "TIC 1")
    ess_md = ess_per_sample(tics_md[:, :2], names=[f"md {n}" for n in names])
    if n_groups == 1:
        ess_model = ess_per_sample(tics_model[:, :2], names=[f"model {n}" for n in names])
    else:
        one = ess_per_sample(tics_model[best::n_groups, :1], names=[f"model explorer {best} TIC 0"])
        ess_model = torch.cat([one, torch.full_like(one, float("nan"))])
    ratio = (ess_model / float(model_seconds_per_frame)) / (ess_md / float(md_seconds_per_frame))
    acceptance = acceptance_from_thinned(model.cpu().numpy() if isinstance(model, torch.Tensor) else model) \
        if topology is not None and n_groups == 1 else None
    host = lambda t: torch.as_tensor(t).detach().cpu().numpy()
    return SpeedupReport(coverage=coverage, coverage_arg=int(arg[best]), covered_fraction=float((min_d[best] < threshold).double().mean()),
                         threshold=threshold, all_states_found=bool(found), ess_md=host(ess_md), ess_model=host(ess_model),
                         speedup_tic0=float(ratio[0]) if found else 0.0,
                         speedup_tic1=float(ratio[1]) if found and n_groups == 1 else 0.0, acceptance=acceptance,
                         eigenvalues=host(tica.eigenvalues), timescales=host(tica.timescales), n_groups=n_groups, best_group=best,
                         group_coverage=host(worst))


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
