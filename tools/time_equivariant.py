"""Pass times of the equivariant NVP flow (configs/equivariant_nvp.yaml: emb 32, hidden [256, 256], 4 couplings) on alanine
dipeptide, HIP events around each call:  `python tools/time_equivariant.py [--cpu] [S]`  (S proposals, default 1000).
Prints ms per reverse pass (conditional_sample_with_logp) and per log_likelihood pass over S rows, the median and the minimum
of 7 calls after 2 warm-up calls, and the algorithmic TFLOP/s from the layer shapes.  --cpu adds the plain-torch restatement
(tests/equivariant_flow_oracle.py) on the host for the same two calls.  Under `rocprofv3 --kernel-trace --stats` for the
per-kernel shares (profiles/equivariant_nvp.txt)."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import timewarp_amd as tw  # noqa: E402
from oracle import flow_oracle as fo  # noqa: E402
from timewarp_amd import synthetic  # noqa: E402

S = int(next((a for a in sys.argv[1:] if not a.startswith("--")), "1000"))
m = tw.model_constructor(synthetic.equivariant_nvp_config())
sd = fo.synth_state_dict(m.state_dict(), 0)
m.load_state_dict(sd)
m = m.cuda().eval()
types, coords, _ = synthetic.alanine_dipeptide_state()
V = 22
g = torch.Generator().manual_seed(0)
xv = torch.randn(1, V, 3, generator=g)
mk = torch.zeros(1, V, dtype=torch.bool)
zc, zv = fo.draw_latents(sd, S, (1, V, 3), g)
yc = (coords[None] + zc[:, 0]).contiguous()
yv = zv[:, 0].contiguous()


def pair_flop(E=32, H=256):
    """FLOP per pair of one coupling layer (both modules): the processor's relative MLP and phi, 2 per multiply-add."""
    total = 0
    for P, R, n_rel in ((E + 2, 1, 1), (E + 1, 2, 2)):   # a positions and a velocities coupling
        for out in (E, n_rel):                            # scale module, shift module
            total += 2 * ((2 * P + R) * H + H * H + H * E + E * H + H * H + H * out)
    return total / 2   # mean over the two kinds of coupling


flop = pair_flop() * 4 * V * V * S
dev = dict(at=types[None].cuda(), xc=coords[None].cuda(), xv=xv.cuda(), mk=mk.cuda(), zc=zc.cuda(), zv=zv.cuda(), yc=yc.cuda(),
           yv=yv.cuda())
calls = {
    "reverse pass": lambda: m.conditional_sample_with_logp(
        atom_types=dev["at"], x_coords=dev["xc"], x_velocs=dev["xv"], adj_list=None, edge_batch_idx=None,
        masked_elements=dev["mk"], num_samples=S, z_coords=dev["zc"], z_velocs=dev["zv"]),
    "log_likelihood pass": lambda: m.log_likelihood(
        atom_types=dev["at"].repeat(S, 1), x_coords=dev["xc"].repeat(S, 1, 1), x_velocs=dev["xv"].repeat(S, 1, 1),
        y_coords=dev["yc"], y_velocs=dev["yv"], adj_list=None, edge_batch_idx=None, masked_elements=dev["mk"].repeat(S, 1)),
}
for name, f in calls.items():
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    times = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    med = statistics.median(times)
    print(f"equivariant V={V} S={S} {name}: median {med:.2f} ms, min {min(times):.2f} ms of 7; pair MLPs {flop / 1e12:.3f} TFLOP "
          f"per pass -> {flop / med / 1e9:.1f} TFLOP/s algorithmic", flush=True)

if "--cpu" in sys.argv:
    from tests import equivariant_flow_oracle as eo

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    spec = eo.EquivariantFlowSpec()
    with torch.no_grad():
        t0 = time.perf_counter()
        eo.conditional_sample_with_logp(sd, spec, types[None], coords[None], xv, mk, zc, zv)
        t1 = time.perf_counter()
        eo.log_likelihood(sd, spec, types[None].repeat(S, 1), coords[None].repeat(S, 1, 1), xv.repeat(S, 1, 1), yc, yv,
                          mk.repeat(S, 1))
        t2 = time.perf_counter()
    print(f"CPU restatement, {torch.get_num_threads()} threads, S={S}: reverse pass {1e3 * (t1 - t0):.0f} ms, log_likelihood pass "
          f"{1e3 * (t2 - t1):.0f} ms (one call each)", flush=True)
