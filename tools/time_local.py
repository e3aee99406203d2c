"""Reverse-pass time of the local-attention flow (configs/local_transformer_nvp.yaml: 8 heads of 128, max_radius 0.2 nm) on the
per-op paths, HIP events around each call:  `python tools/time_local.py [--path=2|5] [22x1000 691x16 ...]`.  Alanine dipeptide's
coordinates at 22 atoms, the 691-atom protein's (tests/golden/energy_kat_1hgv.npz, frame 0) otherwise.  Under
`rocprofv3 --kernel-trace --stats` for the per-kernel shares (profiles/local_attention.txt)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import timewarp_amd as tw  # noqa: E402
from oracle import flow_oracle as fo  # noqa: E402
from timewarp_amd import synthetic  # noqa: E402

paths = [int(a.split("=")[1]) for a in sys.argv[1:] if a.startswith("--path=")] or [2, 5]
sizes = [a for a in sys.argv[1:] if not a.startswith("--")] or ["22x1000", "691x16"]
m = tw.model_constructor(synthetic.local_transformer_nvp_config())
m.load_state_dict(fo.synth_state_dict(m.state_dict(), 0))
m = m.cuda().eval()
g = torch.Generator().manual_seed(0)
for spec in sizes:
    V, S = (int(t) for t in spec.split("x"))
    if V == 22:
        types, coords, _ = synthetic.alanine_dipeptide_state()
    else:
        z = np.load(os.path.join(ROOT, "tests", "golden", "energy_kat_1hgv.npz"))
        coords = torch.from_numpy(np.asarray(z["positions"][0][:V], dtype=np.float32))
        types = torch.randint(0, 5, (V,), generator=g)
    at, xc = types[None].cuda(), coords[None].cuda()
    xv = torch.randn(1, V, 3, generator=g).cuda()
    mk = torch.zeros(1, V, dtype=torch.bool).cuda()
    c = xc[0] - xc[0].mean(0)
    kbar = float((torch.cdist(c, c) < 0.2).sum(-1).float().mean())
    f_blk = 6_436_864 + 12_288 * kbar   # FLOP per token per net-block (d_in 25, 8 heads of 128, ff 2048, hidden 256)
    flop = 16 * V * f_blk * S
    for path in paths:
        m.execution_path = path
        f = lambda: m.conditional_sample_with_logp(atom_types=at, x_coords=xc, x_velocs=xv, adj_list=None, edge_batch_idx=None,
                                                   masked_elements=mk, num_samples=S)
        f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 5
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / n
        print(f"local path {path} V={V} S={S}: {ms:.2f} ms per reverse pass, K_mean {kbar:.2f}, {flop / 1e9:.2f} GFLOP per pass, "
              f"{flop / ms / 1e9:.1f} TFLOP/s algorithmic; attention floor {(4 * 8 * 128) * 4 * V * S / 1e6:.2f} MB per launch",
              flush=True)
