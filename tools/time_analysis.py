"""Time of the analysis kernels against the same results through torch ops, in one run on one MI355X (profiles/analysis.txt).

  featurisation   262144 frames of NNQQ (65 atoms; the 40 frames of tests/golden/energy_kat_2olx.npz repeated with seeded noise):
                  `analysis.tica_features` (tw_tica_features, one launch) against gather + cross + atan2 + sin / cos + cdist.
  moments         F = 512, T = 262144, lag = 500, one chain: tw_lagged_moments against X.double() slices and torch.matmul, casts
                  included.
  weighted        the same X with weights normal(1, 1): tw_lagged_moments_weighted against tw_lagged_moments and against the
                  weighted torch route (x w, y w in fp64, then the matmuls).
  projection      the same X as [T, F] rows: tw_project at k = 1 (frame weights) and k = 40 (TICs) against
                  (X.double() - m) @ P, cast included.

Each route is warmed up, then timed `--repeats` times with HIP events on the launch stream, the two routes alternating; the
median, the fastest and the slowest are printed, and how far the two routes' results are apart.

    python tools/time_analysis.py [--out profiles/analysis.txt] [--frames 262144] [--features 512] [--lag 500] [--repeats 7]"""
import argparse, os, platform, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from timewarp_amd import analysis as an

p = argparse.ArgumentParser()
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "analysis.txt"))
p.add_argument("--frames", type=int, default=262144)
p.add_argument("--features", type=int, default=512)
p.add_argument("--lag", type=int, default=500)
p.add_argument("--repeats", type=int, default=7)
args = p.parse_args()
assert torch.cuda.is_available(), "tools/time_analysis.py measures on an MI355X: no GPU is visible"
dev = torch.device("cuda", 0)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(routes, repeats):
    """{name: [ms, ...]}: every route warmed up twice, then `repeats` rounds in which the routes alternate; HIP events on the
    current stream around each call."""
    for fn in routes.values():
        fn(), fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(repeats):
        for k, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


def report(ms):
    for k, v in ms.items():
        say(f"    {k:<28s} median {statistics.median(v):10.3f} ms   fastest {min(v):10.3f}   slowest {max(v):10.3f}   ({len(v)} runs)")


say(f"tools/time_analysis.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).multi_processor_count} CUs), "
    f"host {platform.node()}, torch {torch.__version__}, HIP {torch.version.hip}")
say(f"frames {args.frames}, moments F {args.features}, lag {args.lag}, {args.repeats} timed runs per route after 2 warm-up runs, "
    "HIP events on the launch stream, routes alternating")

# ---- featurisation
z = np.load(os.path.join(ROOT, "tests", "golden", "energy_kat_2olx.npz"))
topo = (list(z["atom_names"]), list(z["residue_names"]), list(z["residue_ids"]))
g = torch.Generator(device=dev).manual_seed(0)
base = torch.as_tensor(np.ascontiguousarray(z["positions"], dtype=np.float32)).to(dev)
coords = base[torch.arange(args.frames, device=dev) % base.shape[0]] + 1e-3 * torch.randn(args.frames, 65, 3, device=dev, generator=g)
sel, quads, cols = an.feature_tables(topo)
sel_t, quads_t = torch.as_tensor(sel).long().to(dev), torch.as_tensor(quads).long().to(dev)
iu = torch.triu_indices(len(sel), len(sel), offset=1, device=dev)
sizes = [3, 3, 3]


def features_torch():
    x = coords[:, sel_t]
    d = torch.cdist(x, x)[:, iu[0], iu[1]]
    p0, p1, p2, p3 = (coords[:, quads_t[:, k]] for k in range(4))
    b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
    c1, c2 = torch.cross(b2, b3, dim=-1), torch.cross(b1, b2, dim=-1)
    ang = torch.atan2((b1 * c1).sum(-1) * b2.norm(dim=-1), (c1 * c2).sum(-1))
    parts = [d]
    for a in torch.split(ang, sizes, dim=1):
        parts += [torch.sin(a), torch.cos(a)]
    return torch.cat(parts, dim=1)


def features_kernel():
    return an.features_from_tables(coords, sel, quads, cols)


F_feat = len(sel) * (len(sel) - 1) // 2 + 2 * len(quads)
say()
say(f"featurisation: {args.frames} frames x 65 atoms -> {F_feat} features ({len(sel)} selected atoms, {len(quads)} torsions); "
    f"{args.frames * 65 * 12 / 1e6:.0f} MB read, {args.frames * F_feat * 4 / 1e6:.0f} MB written")
ms = timed({"tw_tica_features": features_kernel, "torch ops (float32)": features_torch}, args.repeats)
report(ms)
diff = (features_kernel().double() - features_torch().double()).abs().max().item()
say(f"    largest difference between the two: {diff:.3e} (the torch route works in float32)")
k_ms, t_ms = statistics.median(ms["tw_tica_features"]), statistics.median(ms["torch ops (float32)"])
say(f"    kernel / torch = {k_ms / t_ms:.3f};  kernel moves {(args.frames * (65 * 12 + F_feat * 4)) / k_ms / 1e6:.1f} GB/s")
del coords
torch.cuda.empty_cache()

# ---- moments
F, T, lag = args.features, args.frames, args.lag
X = torch.randn(1, T, F, device=dev, generator=g) + torch.randn(F, device=dev, generator=g)
acc_k = an.moments_accumulator(F, dev)
acc_t = (torch.zeros_like(acc_k[0]), torch.zeros_like(acc_k[1]))


def moments_kernel():
    acc_k[0].zero_(), acc_k[1].zero_()
    an.accumulate_moments(X, lag, *acc_k)


def moments_torch():
    acc_t[0].zero_(), acc_t[1].zero_()
    an._accumulate_moments_torch(X, lag, *acc_t)


say()
flop = 2.0 * (T - lag) * F * F
say(f"moments: X [1, {T}, {F}] float32, lag {lag}: {T - lag} pairs; three F x F fp64 products = {3 * flop / 1e9:.1f} GFLOP as torch "
    f"computes them, {(2 * flop + 2.0 * (T - lag) * F * 128) / 1e9:.1f} GFLOP in the kernel (upper tiles only of the two symmetric ones); "
    f"kernel workspace {acc_k[2].numel() * 8 / 1e6:.0f} MB, torch route's fp64 casts {2 * (T - lag) * F * 8 / 1e6:.0f} MB")
ms = timed({"tw_lagged_moments": moments_kernel, "torch double() + matmul": moments_torch}, args.repeats)
report(ms)
moments_kernel(), moments_torch()
rel = ((acc_k[0] - acc_t[0]).abs().max() / acc_t[0].abs().max()).item()
say(f"    largest difference between the two, relative to the largest entry: {rel:.3e}; pair counts {int(acc_k[1])} / {int(acc_t[1])}")
k_ms, t_ms = statistics.median(ms["tw_lagged_moments"]), statistics.median(ms["torch double() + matmul"])
say(f"    kernel / torch = {k_ms / t_ms:.3f};  kernel: {3 * flop / k_ms / 1e9:.2f} TFLOP/s counted as three full products, "
    f"torch: {3 * flop / t_ms / 1e9:.2f} TFLOP/s")
say(f"    analysis.DEFAULT_MOMENTS_ROUTE = {an.DEFAULT_MOMENTS_ROUTE!r}")

# ---- weighted moments
W = 1.0 + torch.randn(1, T, device=dev, generator=g, dtype=torch.float64)
sw_k, sw_t = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)


def weighted_kernel():
    acc_k[0].zero_(), acc_k[1].zero_(), sw_k.zero_()
    an.accumulate_moments_weighted(X, W, lag, acc_k[0], acc_k[1], sw_k, acc_k[2])


def weighted_torch():
    acc_t[0].zero_(), acc_t[1].zero_(), sw_t.zero_()
    an._accumulate_moments_torch(X, lag, *acc_t, W, sw_t)


say()
say(f"weighted moments: the same X, weights [1, {T}] fp64 = 1 + normal ({W.numel() * 8 / 1e6:.1f} MB more to read); the unweighted "
    "kernel is timed again in the same rounds")
ms = timed({"tw_lagged_moments_weighted": weighted_kernel, "tw_lagged_moments": moments_kernel,
            "torch weighted double() + matmul": weighted_torch}, args.repeats)
report(ms)
weighted_kernel(), weighted_torch()
rel = ((acc_k[0] - acc_t[0]).abs().max() / acc_t[0].abs().max()).item()
say(f"    largest difference between the two weighted routes, relative to the largest entry: {rel:.3e}; "
    f"sum w {float(sw_k):.9e} / {float(sw_t):.9e}")
w_ms, k_ms, t_ms = (statistics.median(ms[k]) for k in ("tw_lagged_moments_weighted", "tw_lagged_moments",
                                                        "torch weighted double() + matmul"))
say(f"    weighted / unweighted kernel = {w_ms / k_ms:.3f};  weighted kernel / weighted torch = {w_ms / t_ms:.3f}")

# ---- projection
rows = X[0]
m_p = torch.randn(F, device=dev, generator=g, dtype=torch.float64)
for k in (1, 40):
    P_p = torch.randn(F, k, device=dev, generator=g, dtype=torch.float64)
    b_p = torch.randn(k, device=dev, generator=g, dtype=torch.float64)
    say()
    say(f"projection k = {k}: X [{T}, {F}] float32 -> [{T}, {k}] fp64; {T * F * 4 / 1e6:.0f} MB read, {T * k * 8 / 1e6:.1f} MB written, "
        f"{2.0 * T * F * k / 1e9:.1f} GFLOP; the torch route's fp64 cast is {T * F * 8 / 1e6:.0f} MB")
    ms = timed({"tw_project": lambda: an.project(rows, P_p, m_p, b_p), "torch (X.double() - m) @ P + b": lambda: (rows.double() - m_p) @ P_p + b_p},
               args.repeats)
    report(ms)
    a, b = an.project(rows, P_p, m_p, b_p), (rows.double() - m_p) @ P_p + b_p
    k_ms, t_ms = statistics.median(ms["tw_project"]), statistics.median(ms["torch (X.double() - m) @ P + b"])
    say(f"    largest difference between the two, relative to the largest entry: {((a - b).abs().max() / b.abs().max()).item():.3e}")
    say(f"    kernel / torch = {k_ms / t_ms:.3f};  kernel reads X at {T * F * 4 / k_ms / 1e6:.1f} GB/s")
    del a, b

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
