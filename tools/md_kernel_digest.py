#!/usr/bin/env python3
"""One line per case with a sha256 of the raw output bytes of the AMBER energy, force, Langevin, trajectory and minimiser kernels:
two libraries computed the same bits exactly when their outputs are equal line for line.  Run once per library, each in a fresh
process (TW_HIP_LIB names a library other than the in-tree one):

    TW_HIP_LIB=$PWD/timewarp_amd/lib/ab/libtimewarp_hip_parent.so python tools/md_kernel_digest.py > parent.txt
    python tools/md_kernel_digest.py > new.txt && cmp parent.txt new.txt

Cases: every energy / force case of tests/test_amber_kernels_gpu.py (all synthetic families and the real molecules), and the
integrators on alanine dipeptide (one wave), NNQQ (65 atoms: sixteen waves) and a synthetic 66-atom case with cutoff 0.6 and OBC-I,
plus two Langevin steps and one minimiser iteration of the 691-atom protein.  Three rows everywhere.
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import amber_oracle as ao  # noqa: E402
from tests import test_amber_oracle_cpu as cpu  # noqa: E402
from tests.test_langevin_cpu import real_case  # noqa: E402
from timewarp_amd.energy import AmberPotentialEnergyTorch  # noqa: E402
from timewarp_amd.md import LangevinDynamics, minimize_energy  # noqa: E402

ROWS = 3
SCHEMES = ["LangevinMiddleIntegrator", "LangevinIntegrator"]
FRAME_KEYS = ("positions", "velocities", "forces", "energies")


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def rows(x):
    """Three rows of x [N, V, 3], repeating from the start where the case has fewer"""
    return np.ascontiguousarray(x[np.arange(ROWS) % x.shape[0]])


def energy_cases():
    for case in cpu.synthetic_cases():
        t, x, _ = cpu.synthetic(case)
        yield "synthetic V=%d %s gb=%d cutoff=%g" % case, t, x
    for name, (t, x) in cpu.real_cases().items():
        yield name, t, x


def md_cases():
    for mol in ("ad", "nnqq"):
        t, masses, x0, v0 = real_case(mol)
        yield mol, t, masses, rows(x0), rows(v0)
    t, x, _ = ao.synthetic_case(66, "covalent", 2, 0.6)
    masses = (1.0 + 11.0 * (np.arange(66) % 3 == 0)).astype(np.float32)
    v = np.random.default_rng(24).standard_normal((ROWS, 66, 3)) * np.sqrt(2.577 / masses)[None, :, None]   # kT at 310 K, kJ/mol
    yield "synthetic66", t, masses, rows(x), v.astype(np.float32)


def frames_digest(x, v, f, state):
    return digest(x, v, *(getattr(f, k) for k in FRAME_KEYS), *([] if state is None else [state]))


def main():
    for name, t, x in energy_cases():
        p, xg = AmberPotentialEnergyTorch(t), torch.from_numpy(rows(x)).cuda()
        print(f"energy_and_terms  {name}: {digest(*p.energy_and_terms(xg, want_terms=True))}")
        print(f"energy_and_forces {name}: {digest(*p.energy_and_forces(xg))}")
    for mol, t, masses, x0, v0 in md_cases():
        p, m = AmberPotentialEnergyTorch(t), torch.from_numpy(masses)
        x, v = torch.from_numpy(x0).cuda(), torch.from_numpy(v0).cuda()
        for scheme in SCHEMES:
            for friction in (0.0, 0.3):
                make = lambda: LangevinDynamics(p, m, 0.0005, friction, scheme, seed=11)
                tag = f"{mol} {scheme} friction={friction}"
                print(f"step 20           {tag}: {digest(*make().step(x, v, 20, want_energy=True))}")
                for kind in ("stored", "full-step"):
                    md = make()
                    print(f"trajectory        {tag} {kind} one launch: {frames_digest(*md.trajectory(x, v, [0, 5, 12], velocities=kind), None)}")
                    md, cx, cv = make(), x, v
                    state, out = md.new_state(x, v), []
                    for reports in ([0, 5], [5], [2]):   # steps 0, 5 | 10 | 12 of the run
                        cx, cv, f = md.trajectory(cx, cv, reports, state=state, velocities=kind)
                        out.append(frames_digest(cx, cv, f, state))
                    print(f"trajectory        {tag} {kind} launches of 5 with the carry: {' '.join(out)}")
        r = minimize_energy(p, x, max_iterations=3, iterations_per_launch=3)
        fresh = digest(r.coords, r.coords64, r.energy, r.rms_force, r.iterations, r.evaluations, r.status, r.workspace)
        r = minimize_energy(p, x, max_iterations=2, iterations_per_launch=2, workspace=r.workspace)
        print(f"minimize 3 + 2    {mol}: {fresh} {digest(r.coords, r.coords64, r.energy, r.rms_force, r.iterations, r.evaluations, r.status, r.workspace)}")
    t, masses, x0, v0 = real_case("1hgv")
    p, x, v = AmberPotentialEnergyTorch(t), torch.from_numpy(rows(x0)).cuda(), torch.from_numpy(rows(v0)).cuda()
    print(f"step 2            1hgv: {digest(*LangevinDynamics(p, torch.from_numpy(masses), 0.0005, 0.3, SCHEMES[0], seed=11).step(x, v, 2, want_energy=True))}")
    r = minimize_energy(p, x, max_iterations=1, iterations_per_launch=1)
    print(f"minimize 1        1hgv: {digest(r.coords, r.coords64, r.energy, r.rms_force, r.iterations, r.evaluations, r.status, r.workspace)}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
