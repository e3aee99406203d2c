"""Writes tests/golden/spacing_steps.npz: the report steps the REFERENCE's spacing policies (simulation/npzreporter.py:24-193)
give for a handful of parameter sets, for tests/test_md_trajectory_cpu.py to hold timewarp_amd/simulation.py to.

    python tools/gen_spacing_golden.py /path/to/reference [tests/golden/spacing_steps.npz]

The reference's module is imported as it is; its only third-party import, `openmm.unit`, is used by the reporter class alone
and is replaced by an empty stub (no OpenMM is needed for the policies).  A case is walked as OpenMM's Simulation walks a
reporter: from `start`, ask stepsUntilNextReport, advance by the answer, record the step, until `stop` is passed.  The file
holds integer arrays only: per case `<name>__params` (what builds the policy, see CASES) and `<name>__steps`."""
import importlib.util
import os
import sys
import types

import numpy as np

# name -> (policy, constructor arguments, start, stop).  The windowed cases step once through three windows (fixed seeds):
# from before the first window to past the third one's last possible step.
CASES = {
    "regular_7": ("regular", (7,), 0, 50),
    "regular_1000_from_2500": ("regular", (1000,), 2500, 7000),
    "regular_1": ("regular", (1,), 3, 12),
    "log_10000_10": ("logarithmic", (10000, 10), 10000, 31000),
    "log_10_3_from_3": ("logarithmic", (10, 3), 3, 27),
    "log_1000_2_from_0": ("logarithmic", (1000, 2), 0, 2100),
    "log_64_4_from_70": ("logarithmic", (64, 4), 70, 200),
    "windowed_1000_100_10_seed0": ("windowed", (1000, 100, 10, 0), 0, 3100),
    "windowed_500_200_10_seed7": ("windowed", (500, 200, 10, 7), 250, 1749),
    "windowed_64_8_3_seed123": ("windowed", (64, 8, 3, 123), 10, 201),
}


def load_reference_reporter(reference_root):
    openmm = types.ModuleType("openmm")
    openmm.unit = types.ModuleType("openmm.unit")
    sys.modules.setdefault("openmm", openmm)
    sys.modules.setdefault("openmm.unit", openmm.unit)
    spec = importlib.util.spec_from_file_location("reference_npzreporter", os.path.join(reference_root, "simulation", "npzreporter.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def walk(policy, start, stop):
    steps, c = [], start
    while True:
        c += int(policy.stepsUntilNextReport(c))
        if c > stop:
            return np.asarray(steps, dtype=np.int64)
        steps.append(c)


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "spacing_steps.npz")
    ref = load_reference_reporter(sys.argv[1])
    build = {"regular": ref.RegularSpacing, "logarithmic": ref.LogarithmicSpacing,
             "windowed": lambda i, w, s, seed: ref.UniformWindowedSpacing(i, spacing_window=w, subsamples=s, seed=seed)}
    kinds = ["regular", "logarithmic", "windowed"]
    arrays = {}
    for name, (kind, args, start, stop) in CASES.items():
        steps = walk(build[kind](*args), start, stop)
        # params: policy index (regular 0, logarithmic 1, windowed 2), start, stop, then the constructor arguments
        arrays[name + "__params"] = np.asarray([kinds.index(kind), start, stop, *args], dtype=np.int64)
        arrays[name + "__steps"] = steps
        print(f"{name}: {len(steps)} steps, {steps[:6].tolist()} ..")
    np.savez_compressed(out, **arrays)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
