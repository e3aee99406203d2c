"""The speed-up of a sampler over MD for one peptide, from the files the two runs leave behind (`analysis.speedup_report`):

    python -m timewarp_amd.speedup --md NAME-traj-arrays.npz --pdb NAME-traj-state0.pdb \\
        (--model-dir DIR --protein NAME | --exploration FILE --explorers P) \\
        --md-seconds-per-step X --md-steps-per-frame K [--lag 100 --dim 40 --threshold T --md-stride 1 --cloud-stride 1 --no-koopman --out F]

--model-dir / --protein: the segments `sample_trajectory` wrote (notebooks/Paper/speed-up-mcmc.ipynb, cell 8).  --exploration /
--explorers: the reference's `<protein>_exploration.npz` with P explorers interleaved (speed-up-exploration.ipynb, cell 4).  The MD
wall time is an argument because `*-traj-arrays.npz` carries none: seconds per integration step times the steps between two saved
frames.  Writes `<name>-speedup.npz` next to the MD trajectory and prints one line.
"""
from __future__ import annotations

import argparse
import dataclasses
import os

import numpy as np

from . import analysis


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m timewarp_amd.speedup", description="Speed-up of a sampler over MD, with the coverage check")
    p.add_argument("--md", required=True, help="*-traj-arrays.npz with `positions` [T, V, 3] (nm), as simulation.py writes it")
    p.add_argument("--pdb", required=True, help="the trajectory's state0 PDB (topology)")
    p.add_argument("--model-dir", default=None, help="directory of <protein>_trajectory_model_<i>.npz segments (sample_trajectory)")
    p.add_argument("--protein", default=None, help="the segments' protein name (with --model-dir)")
    p.add_argument("--exploration", default=None, help="<protein>_exploration.npz with `positions` [steps * P, V, 3] and `time`")
    p.add_argument("--explorers", type=int, default=None, help="P, the number of interleaved explorers (with --exploration)")
    p.add_argument("--md-seconds-per-step", type=float, required=True, help="wall-clock seconds of one MD integration step")
    p.add_argument("--md-steps-per-frame", type=int, required=True, help="integration steps between two saved MD frames")
    p.add_argument("--lag", type=int, default=100, help="TICA lag time in MD frames")
    p.add_argument("--dim", type=int, default=40, help="TICA dimensions kept")
    p.add_argument("--threshold", type=float, default=None, help="coverage below which all states count as found (0.3; 0.1 for explorers)")
    p.add_argument("--md-stride", type=int, default=1, help="compare every n-th MD point (the notebook: 10)")
    p.add_argument("--cloud-stride", type=int, default=1, help="compare every n-th model point (the notebook: 10)")
    p.add_argument("--no-koopman", action="store_true", help="plain TICA, without the Koopman reweighting")
    p.add_argument("--out", default=None, help="output file (default <name>-speedup.npz next to the MD trajectory)")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    """The arguments, after the checks argparse cannot state: exactly one of the two model sources, each with its companion."""
    p = build_parser()
    a = p.parse_args(argv)
    if (a.model_dir is None) == (a.exploration is None):
        p.error("give exactly one of --model-dir (with --protein) and --exploration (with --explorers)")
    if a.model_dir is not None and (a.protein is None or a.explorers is not None):
        p.error("--model-dir goes with --protein, and not with --explorers")
    if a.exploration is not None and (a.explorers is None or a.explorers < 1 or a.protein is not None):
        p.error("--exploration goes with --explorers P >= 1, and not with --protein")
    if not (a.md_seconds_per_step > 0 and a.md_steps_per_frame >= 1):
        p.error("--md-seconds-per-step must be positive and --md-steps-per-frame at least 1")
    return a


def output_path(trajectory: str) -> str:
    stem = os.path.basename(trajectory)
    for suffix in ("-traj-arrays.npz", ".npz"):
        if stem.endswith(suffix):
            stem = stem[: -len(suffix)]
            break
    return os.path.join(os.path.dirname(trajectory), stem + "-speedup.npz")


def main(argv=None) -> str:
    a = parse_args(argv)
    with np.load(a.md) as z:
        md = np.ascontiguousarray(z["positions"], dtype=np.float32)
    if a.model_dir is not None:
        model, seconds = analysis.load_model_chain(a.model_dir, a.protein)
        n_groups, model_seconds_per_frame = 1, float(seconds.sum()) / len(model)
    else:
        model, seconds = analysis.load_exploration(a.exploration)
        n_groups = a.explorers
        if len(model) % n_groups:
            raise SystemExit(f"--explorers {n_groups}: {a.exploration} has {len(model)} frames, not a multiple")
        model_seconds_per_frame = float(seconds) / (len(model) // n_groups)
    model = np.ascontiguousarray(model, dtype=np.float32)
    report = analysis.speedup_report(md, model, topology=a.pdb, lag=a.lag, dim=a.dim, koopman=not a.no_koopman,
                                     md_seconds_per_frame=a.md_seconds_per_step * a.md_steps_per_frame,
                                     model_seconds_per_frame=model_seconds_per_frame, n_groups=n_groups, threshold=a.threshold,
                                     md_stride=a.md_stride, cloud_stride=a.cloud_stride)
    out = a.out or output_path(a.md)
    fields = {k: v for k, v in dataclasses.asdict(report).items() if v is not None}
    np.savez(out, **{k: np.asarray(v) for k, v in fields.items()})
    print(f"{out}: coverage {report.coverage:.4f} ({'all states found' if report.all_states_found else 'STATES MISSING'}, threshold "
          f"{report.threshold:g}, {100 * report.covered_fraction:.1f} % of MD points covered), speed-up TIC 0 {report.speedup_tic0:.4g}"
          + (f", TIC 1 {report.speedup_tic1:.4g}" if n_groups == 1 else f", best explorer {report.best_group} of {n_groups}"))
    return out


if __name__ == "__main__":
    main()
