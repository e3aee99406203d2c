"""Time of `tw_cloud_coverage` against the chunked torch.cdist restatement (`analysis.coverage_distance`, route="kernel" and
route="torch"), in one run on one MI355X (profiles/coverage.txt).  dim = 2 throughout, seeded normal clouds:

  thinned     M = 8192 reference points, N = 196608 cloud points: the sizes the notebooks compare after taking every tenth point;
  unthinned   M = 81920, N = 1966080: every point;
  explorers   the unthinned sizes with n_groups = 100 (the exploration notebook's 100 explorers from one pass).

Each route is warmed up, then timed `--repeats` times with HIP events on the launch stream, the two routes alternating; the median,
the fastest and the slowest are printed, the pair rate, and how far the two routes' results are apart.  The torch route evaluates one
pair per workgroup (the direct form of cdist: the matmul form loses small distances to cancellation), so at the unthinned sizes a
single run of it takes minutes; there it is timed on the first `--torch-rows` reference points against the whole cloud (the work is
linear in the reference rows) and the figure for all rows is an extrapolation, named as one; at any size the rows are cut further
when one run of it exceeds `--torch-seconds`.  The kernels' register, scratch and LDS
use comes from tools/resource_usage.py (`--resources FILE`: a saved copy of its output for csrc/tw_analysis.hip).

    python tools/time_coverage.py [--out profiles/coverage.txt] [--repeats 7] [--torch-rows 1024] [--resources FILE]"""
import argparse, os, platform, statistics, subprocess, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from timewarp_amd import analysis as an

p = argparse.ArgumentParser()
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "coverage.txt"))
p.add_argument("--repeats", type=int, default=7)
p.add_argument("--torch-rows", type=int, default=1024, help="reference rows the torch route is timed on at the unthinned sizes")
p.add_argument("--torch-chunk", type=int, default=2048, help="block edge of the torch route (its cdist launch refuses 4096 x 4096)")
p.add_argument("--torch-seconds", type=float, default=3.0, help="the longest one run of the torch route may take before its rows are cut")
p.add_argument("--resources", default=None)
args = p.parse_args()
assert torch.cuda.is_available(), "tools/time_coverage.py measures on an MI355X: no GPU is visible"
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
        say(f"    {k:<34s} median {statistics.median(v):10.3f} ms   fastest {min(v):10.3f}   slowest {max(v):10.3f}   ({len(v)} runs)")


say(f"tools/time_coverage.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).multi_processor_count} CUs), "
    f"host {platform.node()}, torch {torch.__version__}, HIP {torch.version.hip}")
say(f"dim 2, fp64, {args.repeats} timed runs per route after 2 warm-up runs, HIP events on the launch stream, routes alternating; "
    "both routes include the allocation of their outputs and scratch, the inputs are already normalised (normalise=False)")
g = torch.Generator(device=dev).manual_seed(0)
verdict = None
for name, M, N, G in (("thinned", 8192, 196608, 1), ("unthinned", 81920, 1966080, 1), ("explorers", 81920, 1966080, 100)):
    ref = 1.5 * torch.randn(M, 2, device=dev, generator=g, dtype=torch.float64)
    cloud = torch.randn(N, 2, device=dev, generator=g, dtype=torch.float64)
    rows = M if name == "thinned" else min(M, args.torch_rows)
    kernel = lambda: an.coverage_distance(ref, cloud, n_groups=G, normalise=False, route="kernel")
    kernel_min = lambda: an.coverage_distance(ref, cloud, n_groups=G, normalise=False, return_min=True, route="kernel")
    torch_route = lambda: an.coverage_distance(ref[:rows], cloud, n_groups=G, normalise=False, route="torch", chunk=args.torch_chunk)
    # one run of the torch route on the clock of the host: if it takes longer than --torch-seconds, the rows are cut to fit
    t0 = time.perf_counter()
    torch_route()
    torch.cuda.synchronize()
    probe = time.perf_counter() - t0
    if probe > args.torch_seconds:
        rows = max(64, int(rows * args.torch_seconds / probe) // 64 * 64)
    pairs = float(M) * N        # every reference point meets every cloud point once, whatever the number of groups
    say()
    say(f"{name}: M = {M} reference points, N = {N} cloud points, n_groups = {G}: {pairs:.3e} pairs, {pairs * 16 / 1e12:.2f} TB as a "
        f"cdist matrix; kernel workspace {an._lib.load().tw_cloud_coverage_workspace_bytes(M, N, 2, G) / 1e6:.1f} MB; torch route on "
        f"{rows} of {M} reference rows in {args.torch_chunk} x {args.torch_chunk} blocks")
    try:
        ms = timed({"tw_cloud_coverage": kernel, "tw_cloud_coverage + out_min_d2": kernel_min,
                    f"torch.cdist route ({rows} rows)": torch_route}, args.repeats)
    except torch.cuda.OutOfMemoryError as e:
        say(f"    the torch route did not fit device memory at chunk {args.torch_chunk}: {str(e).splitlines()[0]}")
        ms = timed({"tw_cloud_coverage": kernel, "tw_cloud_coverage + out_min_d2": kernel_min}, args.repeats)
    report(ms)
    k_ms = statistics.median(ms["tw_cloud_coverage"])
    say(f"    kernel: {pairs / k_ms / 1e9:.2f} T pairs/s ({5 * pairs / k_ms / 1e9:.1f} T fp64 VALU lane-operations/s at 5 per pair: two "
        "subtractions, a product, an fma, a minimum)")
    t_key = f"torch.cdist route ({rows} rows)"
    if t_key in ms:
        t_ms = statistics.median(ms[t_key])
        whole = t_ms * M / rows
        say(f"    torch route: {float(rows) * N / t_ms / 1e6:.2f} G pairs/s; for all {M} rows "
            + (f"{whole:.1f} ms (measured)" if rows == M else f"{whole:.0f} ms (EXTRAPOLATED from {rows} rows, not measured)")
            + f";  kernel / torch = {k_ms / whole:.5f}")
        wk, ak = an.coverage_distance(ref[:rows], cloud, n_groups=G, normalise=False, route="kernel")
        wt, at = torch_route()
        say(f"    on those {rows} rows the two routes' coverages differ by at most {((wk - wt).abs() / wt).max().item():.3e} relative; "
            f"arg equal in {int((ak == at).sum())} of {G} groups")
        if name == "unthinned":
            verdict = (k_ms, whole, rows == M)
    del ref, cloud
    torch.cuda.empty_cache()

say()
if verdict is not None:
    k_ms, t_ms, measured = verdict
    say(f"unthinned, one group: kernel {k_ms:.1f} ms, torch route {t_ms:.0f} ms ({'measured' if measured else 'extrapolated'}); "
        f"analysis.DEFAULT_COVERAGE_ROUTE = {an.DEFAULT_COVERAGE_ROUTE!r}")
say()
say("resource use of the coverage kernels (tools/resource_usage.py timewarp_amd/csrc/tw_analysis.hip):")
if args.resources:
    text = open(args.resources).read()
else:
    text = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"),
                           os.path.join(ROOT, "timewarp_amd", "csrc", "tw_analysis.hip")], stdout=subprocess.PIPE, text=True).stdout
for line in text.splitlines():
    if "coverage" in line or "VGPRs" in line:
        say("    " + line)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
