"""The data behind the figures of notebooks/Paper/tica-2AA-plots.ipynb and tica-4AA-plots.ipynb, on the device.  No plots.

    python -m timewarp_amd.tica_report --md TRAJ-traj-arrays.npz --model-dir DIR --protein NAME --pdb STATE0.pdb
                                       [--exploration FILE --lag 100 --dim 40 --bins 100 --edges md|own --route R --out FILE]

What stands in for what, per run (MD, the model's chain, the explorers):

  tic01            hist2d(tics[:, 0], tics[:, 1], bins=100) of plot_tic01 / plot_tic01_2 (utils/tica_utils.py:49): the counts, the
                   edges and the outside counters (`evaluate.joint_histograms`, one pair)
  projections      plot_free_energy2 along TIC 0 and TIC 1: np.histogram(tic, bins=100) on the run's own range
                   (`evaluate.column_histograms`), the bin centres and -log(h / h.max()) of the density (`analysis.free_energy`)
  autocorrelation  az.autocorr(tics[:, 0]) up to its first zero, the notebooks' ESS per sample (`analysis.autocorrelation`,
                   `analysis.first_zero_ess`) and, when the time of a frame is given, ESS per second
  tic0_series      tics[::stride, 0] of the scatter plots: every 10th MD frame and every 100th model frame by default
  ramachandran     hist2d(phi_i, psi_i, bins=100) per residue (notebooks/analysis/4AA-sample-trajectory-evaluation.ipynb) through
                   `analysis.ramachandran_histograms`

TICA is `analysis.run_tica` fitted on the MD run; every run is projected with it.  THE TICS ARE ROUNDED ONCE TO FLOAT32 before
anything is binned: the bin rule of this package (include/timewarp_hip.h) is defined on float32 values, and the edges, counts,
projections, autocorrelations and series of the report are all taken from those float32 numbers.  Nothing here claims equality with
deeptime's, arviz's or matplotlib's output: none is available to compare against.
"""
from __future__ import annotations

import argparse
import dataclasses
from typing import Dict, Optional

import numpy as np
import torch

from . import analysis, evaluate

EDGE_MODES = ("md", "own")
RUNS = ("md", "model", "exploration")
DEFAULT_STRIDES = {"md": 10, "model": 100, "exploration": 100}     # spacing and spacing * 10 of tica-2AA-plots.ipynb


@dataclasses.dataclass
class RunReport:
    """One run's share of the report (numpy)."""

    tic01: evaluate.JointHistograms          # one pair: counts [1, bins, bins], x = TIC 0, y = TIC 1
    projections: evaluate.Histograms         # columns TIC 0, TIC 1 on the run's own ranges
    centres: np.ndarray                      # fp64 [2, bins]
    free_energy: np.ndarray                  # fp64 [2, bins]: -log(h / h.max()) of the density, +inf in empty bins
    autocorrelation: np.ndarray              # fp64 [k]: rho_0 .. rho_{k-1} of TIC 0, k the first lag with rho_k <= 0
    ess_per_sample: float
    ess_per_second: Optional[float]          # ess_per_sample / seconds_per_frame when that was given
    tic0_series: np.ndarray                  # float32 [ceil(T / stride)]
    series_stride: int
    ramachandran: Optional[evaluate.JointHistograms]   # one pair per residue with both angles; None without torsions
    n_frames: int


@dataclasses.dataclass
class TicaReport:
    """What `tica_report` returns; `save` writes it as one npz (`evaluate.load_report` reads the arrays back)."""

    bins: int
    edges_mode: str
    lag: int
    eigenvalues: np.ndarray
    timescales: np.ndarray
    residue_pairs: np.ndarray                # int64 [n, 2]: (phi column, psi column) of each Ramachandran plane
    runs: Dict[str, RunReport]

    def arrays(self) -> Dict[str, np.ndarray]:
        out = {"bins": np.int64(self.bins), "edges_mode": np.str_(self.edges_mode), "lag": np.int64(self.lag),
               "eigenvalues": self.eigenvalues, "timescales": self.timescales, "residue_pairs": self.residue_pairs}
        for name, r in self.runs.items():
            out.update({f"{name}_tic01_counts": r.tic01.counts[0], f"{name}_tic01_outside": r.tic01.outside[0],
                        f"{name}_tic01_edges_x": r.tic01.edges_x[0], f"{name}_tic01_edges_y": r.tic01.edges_y[0],
                        f"{name}_projection_counts": r.projections.counts, f"{name}_projection_edges": r.projections.edges,
                        f"{name}_projection_centres": r.centres, f"{name}_free_energy": r.free_energy,
                        f"{name}_autocorrelation": r.autocorrelation, f"{name}_ess_per_sample": np.float64(r.ess_per_sample),
                        f"{name}_tic0_series": r.tic0_series, f"{name}_series_stride": np.int64(r.series_stride),
                        f"{name}_n_frames": np.int64(r.n_frames)})
            if r.ess_per_second is not None:
                out[f"{name}_ess_per_second"] = np.float64(r.ess_per_second)
            if r.ramachandran is not None:
                out[f"{name}_ramachandran_counts"] = r.ramachandran.counts
                out[f"{name}_ramachandran_outside"] = r.ramachandran.outside
                out[f"{name}_ramachandran_edges"] = r.ramachandran.edges_x
        return out

    def save(self, path: str) -> str:
        np.savez(path, **self.arrays())
        return path


def _dihedrals_torch(x: torch.Tensor, quads: np.ndarray) -> torch.Tensor:
    """mdtraj's convention in torch fp64, rounded once to float32 (the restatement `evaluate._torsions` uses on its torch route)."""
    q = torch.as_tensor(quads.astype(np.int64), device=x.device)
    p = x.double()[:, q]
    b1, b2, b3 = p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 1], p[:, :, 3] - p[:, :, 2]
    c1, c2 = torch.linalg.cross(b2, b3), torch.linalg.cross(b1, b2)
    return torch.atan2((b1 * c1).sum(-1) * torch.linalg.norm(b2, dim=-1), (c1 * c2).sum(-1)).to(torch.float32)


def _features_torch(coords, topology) -> torch.Tensor:
    """`analysis.tica_features` with torch ops, in one piece: what the torch route fits on where there is no GPU."""
    sel, quads, cols = analysis.feature_tables(topology)
    x = torch.as_tensor(np.asarray(coords, dtype=np.float32)) if not isinstance(coords, torch.Tensor) else coords.to(torch.float32)
    i, j = np.triu_indices(len(sel), k=1)
    d = evaluate._pair_distances_torch(x, np.stack([sel[i], sel[j]], axis=1))
    block = torch.empty((x.shape[0], 2 * len(quads)), dtype=torch.float32, device=x.device)
    if len(quads):
        ang = _dihedrals_torch(x, quads)
        block[:, torch.as_tensor(cols[:, 0].astype(np.int64))] = torch.sin(ang)
        block[:, torch.as_tensor(cols[:, 1].astype(np.int64))] = torch.cos(ang)
    return torch.cat([d, block], dim=1)


def _one_run(tics32: torch.Tensor, bins: int, route: str, chunk_rows, shared_edges, seconds_per_frame, stride: int,
             name: str) -> RunReport:
    tic01 = evaluate.joint_histograms(tics32, [[0, 1]], bins=bins, route=route, chunk_rows=chunk_rows, edges=shared_edges)
    proj = evaluate.column_histograms(tics32[:, :2], bins=bins, route=route, chunk_rows=chunk_rows)
    centres = 0.5 * (proj.edges[:, 1:] + proj.edges[:, :-1])
    with np.errstate(invalid="ignore", divide="ignore"):
        fe = np.stack([analysis.free_energy(d).numpy() for d in proj.density()])
    tic0 = tics32[:, 0]
    rho = analysis.autocorrelation(tic0.reshape(1, -1, 1), int(tic0.shape[0]) - 1)[:, 0]
    ess = float(analysis.first_zero_ess(rho, names=[f"{name} TIC 0"]))
    k = int((rho <= 0).to(torch.int64).argmax())
    return RunReport(tic01=tic01, projections=proj, centres=centres, free_energy=fe, autocorrelation=rho[:k].cpu().numpy(),
                     ess_per_sample=ess, ess_per_second=None if seconds_per_frame is None else ess / float(seconds_per_frame),
                     tic0_series=tic0[::int(stride)].cpu().numpy(), series_stride=int(stride), ramachandran=None,
                     n_frames=int(tic0.shape[0]))


def tica_report(md, model, *, exploration=None, topology=None, torsions: Optional[Dict[str, tuple]] = None, lag: int = 100,
                dim: int = 40, koopman: bool = True, bins: int = 100, edges: str = "md", route: Optional[str] = None,
                tica_route: Optional[str] = None, seconds_per_frame: Optional[Dict[str, float]] = None,
                strides: Optional[Dict[str, int]] = None, chunk_frames: int = 16384, chunk_rows: Optional[int] = None) -> TicaReport:
    """The module docstring's fields for the MD run `md`, the model's chain `model` and, when given, the explorers' frames
    `exploration`: coordinates [T, V, 3] with `topology`, or features [T, F] without (the input rule of `analysis.run_tica`);
    numpy or device tensors.

    TICA (`lag`, `dim`, `koopman`) is fitted on `md` and projects every run; THE TICS ARE ROUNDED ONCE TO FLOAT32, and everything
    below is computed from those float32 values.  edges="md" (the default) bins TIC 0 x TIC 1 of every run on MD's ranges, so the
    panels compare bin for bin; edges="own" gives each run its own ranges, which is what hist2d does before the notebooks clip the
    axes to MD's limits.  The projections always use the run's own ranges, as plot_free_energy2 does.  The autocorrelation of TIC 0
    is kept up to its first zero; a run whose autocorrelation never reaches zero raises ValueError naming it.
    seconds_per_frame[run] fills in ESS per second; strides[run] thins the TIC 0 series (DEFAULT_STRIDES).

    Ramachandran counts need angles: with `topology` they are computed from the coordinates, one plane per residue that has both
    phi and psi; without, torsions[run] = (phi [T, R], psi [T, R]) pairs them column by column; with neither they are left out.

    `route` (evaluate.JOINT_ROUTES) is the route of every histogram.  `tica_route` ("kernel" or "torch", default: `route`) is where
    the features, the TICA and the angles are computed: "torch" restates them with torch ops in one piece and runs without a
    GPU; the two give TICs that differ in their last bits, so integer fields are comparable between histogram routes only under
    one `tica_route`."""
    if edges not in EDGE_MODES:
        raise ValueError(f"edges {edges!r}: one of {EDGE_MODES}")
    route = evaluate._route(route, evaluate.JOINT_ROUTES, evaluate.DEFAULT_JOINT_ROUTE)
    tica_route = evaluate._route(tica_route, ("kernel", "torch"), route)
    bins = evaluate._check_bins(bins)
    inputs = {"md": md, "model": model}
    if exploration is not None:
        inputs["exploration"] = exploration
    want = 2 if topology is None else 3
    for name, a in inputs.items():
        if len(a.shape) != want:
            raise ValueError(f"tica_report: {name}: expected {'features [T, F]' if topology is None else 'coords [T, V, 3]'}")
    # the TICs of every run, float32
    if tica_route == "torch":
        feats = {k: (_features_torch(a, topology) if topology is not None else torch.as_tensor(a).to(torch.float32))
                 for k, a in inputs.items()}
        tica = analysis._run_tica_torch(feats["md"][None], int(lag), int(dim), koopman, chunk_frames)
        tics = {k: ((f.double() - tica.mean) @ tica.projection) for k, f in feats.items()}
    else:
        evaluate._need_gpu("tica_route 'kernel'")
        tica = analysis.run_tica(md[None], lagtime=int(lag), dim=int(dim), topology=topology, koopman=koopman, chunk_frames=chunk_frames)
        tics = {k: torch.as_tensor(tica.transform(a, chunk_frames=chunk_frames)) for k, a in inputs.items()}
    if tics["md"].shape[1] < 2:
        raise ValueError(f"tica_report: TICA kept {tics['md'].shape[1]} dimension(s); the report needs TIC 0 and TIC 1")
    tics32 = {k: evaluate._place(t.to(torch.float32), route) for k, t in tics.items()}
    seconds, strides = dict(seconds_per_frame or {}), {**DEFAULT_STRIDES, **(strides or {})}
    runs: Dict[str, RunReport] = {}
    shared = None
    for name in inputs:                                     # MD first: its edges are the shared ones
        runs[name] = _one_run(tics32[name], bins, route, chunk_rows, shared, seconds.get(name), strides[name], name)
        if edges == "md" and shared is None:
            shared = (runs["md"].tic01.edges_x, runs["md"].tic01.edges_y)
    # Ramachandran planes
    residue_pairs = np.zeros((0, 2), dtype=np.int64)
    angles = {}
    if topology is not None:
        tables = analysis.torsion_indices(*analysis._topology(topology))
        phi_n = {int(q[1]): i for i, q in enumerate(tables["phi"])}          # as evaluation_report pairs them
        residue_pairs = np.asarray([(phi_n[int(q[0])], j) for j, q in enumerate(tables["psi"]) if int(q[0]) in phi_n],
                                   dtype=np.int64).reshape(-1, 2)
        angles = {k: evaluate._torsions(a, tables, chunk_rows, tica_route) for k, a in inputs.items()}
    elif torsions:
        angles = {k: torsions[k] for k in inputs if k in torsions}
        n = min(min(int(phi.shape[1]), int(psi.shape[1])) for phi, psi in angles.values()) if angles else 0
        residue_pairs = np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.int64)
    for name, (phi, psi) in angles.items():
        runs[name].ramachandran = analysis.ramachandran_histograms(phi, psi, residue_pairs, bins=bins, route=route, chunk_rows=chunk_rows)
    host = lambda t: torch.as_tensor(t).detach().cpu().numpy()
    return TicaReport(bins=bins, edges_mode=edges, lag=int(lag), eigenvalues=host(tica.eigenvalues), timescales=host(tica.timescales),
                      residue_pairs=residue_pairs, runs=runs)


# ---- command line --------------------------------------------------------------------------------------------------------------------

def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m timewarp_amd.tica_report",
                                description="TIC 0 x TIC 1 counts, free-energy projections, TIC 0 autocorrelations and Ramachandran "
                                            "counts of an MD run, a model chain and the explorers.  The runs are read whole into "
                                            "host memory")
    p.add_argument("--md", required=True, help="*-traj-arrays.npz of the MD run (simulation.py's format)")
    p.add_argument("--model-dir", required=True, help="directory of the chain segments sample_trajectory wrote")
    p.add_argument("--protein", required=True, help="the chain's protein name (the segments' file stem)")
    p.add_argument("--pdb", required=True, help="the state0 PDB (topology)")
    p.add_argument("--exploration", default=None, help="<protein>_exploration.npz (keys positions and time)")
    p.add_argument("--lag", type=int, default=100, help="TICA lag time in MD frames")
    p.add_argument("--dim", type=int, default=40)
    p.add_argument("--bins", type=int, default=100)
    p.add_argument("--edges", default="md", choices=EDGE_MODES)
    p.add_argument("--route", default=None, choices=evaluate.JOINT_ROUTES,
                   help="'torch' also fits TICA with torch ops, in one piece, and runs without a GPU")
    p.add_argument("--md-seconds-per-frame", type=float, default=None, help="wall time of one MD frame (fills in MD's ESS per second)")
    p.add_argument("--out", default=None, help="output file (default <protein>_tica_report.npz in the working directory)")
    return p


def main(argv=None) -> str:
    args = build_parser().parse_args(argv)
    with np.load(args.md) as z:
        md = np.ascontiguousarray(z["positions"], dtype=np.float32)
    chain, chain_seconds = analysis.load_model_chain(args.model_dir, args.protein)
    chain = np.ascontiguousarray(chain, dtype=np.float32)
    seconds = {"model": float(chain_seconds.sum()) / len(chain)}
    if args.md_seconds_per_frame is not None:
        seconds["md"] = args.md_seconds_per_frame
    explored = None
    if args.exploration:
        explored, t = analysis.load_exploration(args.exploration)
        explored = np.ascontiguousarray(explored, dtype=np.float32)
        seconds["exploration"] = t / len(explored)
    for name, a in (("MD", md), ("chain", chain), ("exploration", explored)):
        if a is not None and (a.ndim != 3 or a.shape[1:] != md.shape[1:]):
            raise SystemExit(f"positions: {name} {a.shape} and MD {md.shape} must be [T, V, 3] of one molecule")
    if not 1 <= args.lag < len(md):
        raise SystemExit(f"--lag {args.lag}: the MD run has {len(md)} frames, so 1 .. {len(md) - 1}")
    report = tica_report(md, chain, exploration=explored, topology=args.pdb, lag=args.lag, dim=args.dim, bins=args.bins,
                         edges=args.edges, route=args.route, seconds_per_frame=seconds)
    out = args.out or f"{args.protein}_tica_report.npz"
    report.save(out)
    print(f"{out}: " + ", ".join(f"{k} {r.n_frames} frames, TIC 0 ESS per sample {r.ess_per_sample:.4g}" for k, r in report.runs.items())
          + f"; {len(report.residue_pairs)} Ramachandran planes")
    return out


if __name__ == "__main__":
    main()
