"""Time of the bond-length histograms of the evaluation report (`evaluate.pair_histograms`: the range pass, the edges on the host,
the histogram pass) on its three routes, and of the per-atom marginals (`evaluate.column_histograms` on the x components, read in
place), in one run on one MI355X (profiles/evaluate.txt).  100 bins throughout:

  alanine dipeptide   22 atoms, the 21 bonds of the force-field tables, 2^22 frames (1.1 GB of coordinates);
  protein             691 atoms (the 1hgv fixture's frames tiled with noise), the tables' bonds, 2^15 frames (272 MB).

Every route is warmed up, then the routes alternate over `--rounds` rounds; a timed window is as many back-to-back calls as make it
at least `--window` seconds (the number of calls is grown until the event time of a window reaches it), between two HIP events on the launch stream.  The figure of a route is the bytes it
must move, computed from the shapes below, over its median time, as a share of the HBM rate MI355X_MICROARCH.md measured (6.29 TB/s,
a float4 copy; the 8.0 TB/s of the data sheet is printed beside it).  `bytes_*` state what is counted.  The device part of the fused
and kernel routes is also timed alone (fixed edges, no read-back), and one column of 2^24 rows is binned with every row in ONE bin
and with the rows spread over all bins: what same-counter contention costs.

    python tools/time_evaluate.py [--out profiles/evaluate.txt] [--window 0.5] [--rounds 3] [--resources FILE]"""
import argparse, math, os, platform, statistics, subprocess, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from timewarp_amd import _lib, evaluate as ev, forcefield as ffm

p = argparse.ArgumentParser()
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate.txt"))
p.add_argument("--window", type=float, default=0.5, help="least length of a timed window in seconds")
p.add_argument("--rounds", type=int, default=3)
p.add_argument("--resources", default=None, help="a saved copy of tools/resource_usage.py's output for csrc/tw_evaluate.hip")
args = p.parse_args()
assert torch.cuda.is_available(), "tools/time_evaluate.py measures on an MI355X: no GPU is visible"
dev = torch.device("cuda", 0)
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
BINS = 100
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(routes):
    """{name: [ms per call, one per round]}: every route run twice to warm up, its window sized by device events, then `--rounds`
    rounds in which the routes alternate; HIP events around each window of back-to-back calls.  A window that still comes out
    shorter than --window is a failed measurement: the tool stops."""
    def window(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    calls = {}
    for k, fn in routes.items():
        fn(), fn()
        torch.cuda.synchronize()
        # the number of calls is grown until a window's EVENT time reaches --window (a host clock around one call holds launch and
        # synchronise latency and would size the window too short), then a tenth is added against run-to-run spread
        n = 1
        while True:
            got = window(fn, n)
            if got >= 1e3 * args.window:
                break
            n = max(n + 1, math.ceil(1.25 * n * 1e3 * args.window / max(got, 1e-3)))
        calls[k] = math.ceil(1.1 * n)
    ms = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            got = window(fn, calls[k])
            assert got >= 1e3 * args.window, f"{k}: a window of {calls[k]} calls took {got:.1f} ms, less than --window"
            ms[k].append(got / calls[k])
    return ms, calls


def report(ms, calls, nbytes):
    for k, v in ms.items():
        med = statistics.median(v)
        rate = nbytes[k] / (med * 1e-3)
        say(f"    {k:<30s} median {med:9.3f} ms   fastest {min(v):9.3f}   slowest {max(v):9.3f}   ({len(v)} windows of {calls[k]} calls, {min(v) * calls[k] / 1e3:.2f} s the shortest)   "
            f"{nbytes[k] / 1e9:7.3f} GB -> {rate / 1e12:6.3f} TB/s = {100 * rate / HBM_MEASURED:5.1f} % of 6.29 TB/s "
            f"({100 * rate / HBM_SPEC:4.1f} % of 8.0)")


# the bytes a route must move for T frames of V atoms and P pairs (coordinates float32, 12 V bytes a frame)
def bytes_fused(T, V, P):
    return 2 * T * V * 12                            # the coordinates, once for the ranges and once for the counts


def bytes_kernel(T, V, P):
    return T * V * 12 + T * P * 4 + 2 * T * P * 4    # tw_pair_distances reads the coordinates and writes [T, P]; two passes read it


def bytes_torch(T, V, P):
    # the intermediates it materialises, each written once and read once: the fp64 differences [T, P, 3], the float32 distances
    # (read again by the range pass), their fp64 cast [P, T], the int64 bin index [P, T] and the int64 flat index for bincount
    return T * V * 12 + T * P * (2 * 24 + 3 * 4 + 2 * 8 + 2 * 8 + 2 * 8)


def bytes_columns(T, V):
    return 2 * T * V * 4                             # the x components, twice (the 32-byte sectors they sit in hold y and z as well)


def bytes_columns_torch(T, V):
    return T * V * (3 * 4 + 2 * 8 + 2 * 8 + 2 * 8)   # the finite-masked copy of the range pass, the fp64 cast, the two index arrays


def raw_pair_calls(coords, pairs, edges):
    """The device part of the fused route: tw_pair_range + tw_pair_histogram on preallocated outputs, nothing read back."""
    lib = _lib.load()
    T, V, P = coords.shape[0], coords.shape[1], pairs.shape[0]
    lo = torch.empty(P, dtype=torch.float32, device=dev)
    hi = torch.empty(P, dtype=torch.float32, device=dev)
    nf = torch.empty(P, dtype=torch.int64, device=dev)
    counts = torch.zeros(P, BINS, dtype=torch.int64, device=dev)
    outside = torch.zeros(P, 3, dtype=torch.int64, device=dev)
    s = _lib.stream_ptr(dev)

    def fn():
        _lib.check(lib.tw_pair_range(coords.data_ptr(), pairs.data_ptr(), P, T, V, lo.data_ptr(), hi.data_ptr(), nf.data_ptr(), s), "range")
        _lib.check(lib.tw_pair_histogram(coords.data_ptr(), pairs.data_ptr(), P, T, V, edges.data_ptr(), BINS, counts.data_ptr(),
                                         outside.data_ptr(), s), "histogram")
    return fn


def raw_column_calls(X, edges, n_bins=BINS):
    lib = _lib.load()
    T, C = X.shape
    ld, cs = X.stride(0), X.stride(1)
    lo = torch.empty(C, dtype=torch.float32, device=dev)
    hi = torch.empty(C, dtype=torch.float32, device=dev)
    nf = torch.empty(C, dtype=torch.int64, device=dev)
    counts = torch.zeros(C, n_bins, dtype=torch.int64, device=dev)
    outside = torch.zeros(C, 3, dtype=torch.int64, device=dev)
    s = _lib.stream_ptr(dev)

    def fn():
        _lib.check(lib.tw_column_range(X.data_ptr(), T, C, ld, cs, lo.data_ptr(), hi.data_ptr(), nf.data_ptr(), s), "range")
        _lib.check(lib.tw_column_histogram(X.data_ptr(), T, C, ld, cs, edges.data_ptr(), n_bins, counts.data_ptr(), outside.data_ptr(), s),
                   "histogram")
    return fn


def molecule(name):
    g = torch.Generator(device=dev).manual_seed(0)
    if name == "alanine dipeptide":
        base = torch.as_tensor(np.load(os.path.join(ROOT, "tests", "golden", "ad_topology.npz"))["coords_nm"]).to(dev)[None]
        bonds, T = ffm.alanine_dipeptide_amber99sb().bond_idx, 1 << 22
    else:
        z = np.load(os.path.join(ROOT, "tests", "golden", "energy_kat_1hgv.npz"))
        base = torch.as_tensor(z["positions"]).to(dev)
        bonds = ffm.amber99sbildn_obc_tables(list(z["atom_names"]), list(z["residue_names"]), list(z["residue_ids"])).bond_idx
        T = 1 << 15
    x = base.repeat((T + base.shape[0] - 1) // base.shape[0], 1, 1)[:T].contiguous()
    x += 0.004 * torch.randn(x.shape, device=dev, generator=g)
    return x, np.asarray(bonds, dtype=np.int32).reshape(-1, 2)


say(f"tools/time_evaluate.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).multi_processor_count} CUs), "
    f"host {platform.node()}, torch {torch.__version__}, HIP {torch.version.hip}")
say(f"{BINS} bins; windows of at least {args.window} s of back-to-back calls between HIP events on the launch stream, {args.rounds} per "
    "route, routes alternating, after 2 warm-up calls each; the driver rows include the read-back of the ranges, np.linspace on the host "
    "and the allocation of the outputs; HBM line: 6.29 TB/s measured (float4 copy), 8.0 TB/s data sheet (MI355X_MICROARCH.md)")
fastest = {}
for name in ("alanine dipeptide", "protein"):
    coords, bonds = molecule(name)
    T, V, P = coords.shape[0], coords.shape[1], len(bonds)
    say()
    say(f"{name}: {T} frames x {V} atoms ({T * V * 12 / 1e9:.3f} GB of coordinates), {P} bonds; histogram column tile "
        f"{_lib.load().tw_histogram_column_tile(BINS)}")
    routes = {f"pair_histograms route={r!r}": (lambda r=r: ev.pair_histograms(coords, bonds, bins=BINS, route=r)) for r in ev.PAIR_ROUTES}
    nbytes = dict(zip(routes, (bytes_fused(T, V, P), bytes_kernel(T, V, P), bytes_torch(T, V, P))))
    ref = ev.pair_histograms(coords, bonds, bins=BINS, route="fused")
    pd = torch.as_tensor(bonds).to(dev)
    ed = torch.as_tensor(ref.edges).to(dev)
    routes["tw_pair_range + tw_pair_histogram"] = raw_pair_calls(coords, pd, ed)
    nbytes["tw_pair_range + tw_pair_histogram"] = bytes_fused(T, V, P)
    ms, calls = timed(routes)
    report(ms, calls, nbytes)
    med = {r: statistics.median(ms[f"pair_histograms route={r!r}"]) for r in ev.PAIR_ROUTES}
    fastest[name] = min(med, key=med.get)
    same = all((getattr(ref, f) == getattr(ev.pair_histograms(coords, bonds, bins=BINS, route=r), f)).all()
               for r in ("kernel", "torch") for f in ("counts", "below", "above", "nonfinite"))
    say(f"    fastest driver route: {fastest[name]!r}; the three routes' counts are {'EQUAL' if same else 'NOT equal'}")
    # the marginals of plot_marginal_distribution: the x component of every atom, read in place (ld = 3 V, col_stride = 3)
    X = coords[:, :, 0]
    routes = {f"column_histograms route={r!r}": (lambda r=r: ev.column_histograms(X, bins=BINS, route=r)) for r in ev.COLUMN_ROUTES}
    nbytes = dict(zip(routes, (bytes_columns(T, V), bytes_columns_torch(T, V))))
    href = ev.column_histograms(X, bins=BINS, route="kernel")
    routes["tw_column_range + tw_column_histogram"] = raw_column_calls(X, torch.as_tensor(href.edges).to(dev))
    nbytes["tw_column_range + tw_column_histogram"] = bytes_columns(T, V)
    ms, calls = timed(routes)
    report(ms, calls, nbytes)
    med = {r: statistics.median(ms[f"column_histograms route={r!r}"]) for r in ev.COLUMN_ROUTES}
    fastest[name + " columns"] = min(med, key=med.get)
    same = all((getattr(href, f) == getattr(ev.column_histograms(X, bins=BINS, route="torch"), f)).all()
               for f in ("counts", "below", "above", "nonfinite"))
    say(f"    fastest driver route: {fastest[name + ' columns']!r}; the two routes' counts are {'EQUAL' if same else 'NOT equal'}")
    del coords, X
    torch.cuda.empty_cache()

say()
T = 1 << 24
say(f"same-counter contention: one column of {T} rows ({T * 4 / 1e6:.0f} MB), {BINS} bins on (0, 1); tw_column_range + tw_column_histogram")
g = torch.Generator(device=dev).manual_seed(1)
one_bin = torch.full((T, 1), 0.505, dtype=torch.float32, device=dev)
handful = (0.5 + 0.01 * torch.randn(T, 1, device=dev, generator=g)).clamp_(0, 1)
spread = torch.rand(T, 1, device=dev, generator=g)
edges = torch.as_tensor(np.linspace(0, 1, BINS + 1)[None]).to(dev)
routes = {"every row in one bin": raw_column_calls(one_bin, edges), "a bond length (about 6 bins)": raw_column_calls(handful, edges),
          "uniform over all bins": raw_column_calls(spread, edges)}
ms, calls = timed(routes)
report(ms, calls, {k: 2 * T * 4 for k in routes})

say()
say(f"evaluate.DEFAULT_PAIR_ROUTE = {ev.DEFAULT_PAIR_ROUTE!r}, evaluate.DEFAULT_COLUMN_ROUTE = {ev.DEFAULT_COLUMN_ROUTE!r}; fastest here: "
    + ", ".join(f"{k}: {v!r}" for k, v in fastest.items()))
say()
say("resource use of the kernels (tools/resource_usage.py timewarp_amd/csrc/tw_evaluate.hip):")
if args.resources:
    text = open(args.resources).read()
else:
    text = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"),
                           os.path.join(ROOT, "timewarp_amd", "csrc", "tw_evaluate.hip")], stdout=subprocess.PIPE, text=True).stdout
for line in text.splitlines():
    if "kernel" in line or "VGPRs" in line:
        say("    " + line)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
