"""Time of the joint (2-D) histograms behind the TICA and Ramachandran figures (`evaluate.joint_histograms`: the range pass, the
edges on the host, the histogram pass) on its two routes, in one run on one MI355X (profiles/joint_histogram.txt):

  TIC 0 x TIC 1        2^22 rows of a time-ordered four-well trajectory, [T, 2] float32, one pair, 100 x 100;
  Ramachandran, 4AA    the same length, [T, 6] float32 angles (three phi, three psi), the three residue planes, 100 x 100
                       (`analysis.ramachandran_histograms`: fixed range, no range pass);
  1024 x 1024          the TIC trajectory on a plane of 69 bands: what the bands cost;
  vote against plain   `tw_joint_histogram_path` alone (fixed edges, no read-back) on the time-ordered rows and on the same rows
                       shuffled, and on rows that all fall into one bin, at 100 x 100.

The timing method is tools/time_evaluate.py's: every route is warmed up, then the routes alternate over `--rounds` rounds; a timed
window is as many back-to-back calls as make it at least `--window` seconds by device events (sized with a margin of 1.3 where
time_evaluate.py takes 1.1; a window that still comes out shorter stops the tool).  The figure of a route is the bytes it
must move over its median time, as a share of the HBM rate MI355X_MICROARCH.md measured (6.29 TB/s; profiles/evaluate.txt uses the
same line).

    python tools/time_joint_histogram.py [--out profiles/joint_histogram.txt] [--window 0.5] [--rounds 3] [--tests FILE]"""
import argparse, math, os, platform, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from timewarp_amd import _lib, analysis, evaluate as ev

p = argparse.ArgumentParser()
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_histogram.txt"))
p.add_argument("--window", type=float, default=0.5, help="least length of a timed window in seconds")
p.add_argument("--rounds", type=int, default=3)
p.add_argument("--rows", type=int, default=1 << 22)
p.add_argument("--tests", default=None, help="a saved `pytest --durations` output of tests/test_joint_histogram_gpu.py to append")
args = p.parse_args()
assert torch.cuda.is_available(), "tools/time_joint_histogram.py measures on an MI355X: no GPU is visible"
dev = torch.device("cuda", 0)
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
BINS = 100
T = args.rows
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(routes):
    """tools/time_evaluate.py's `timed`: {name: [ms per call, one per round]} and the calls per window."""
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
        n = 1
        while True:
            got = window(fn, n)
            if got >= 1e3 * args.window:
                break
            n = max(n + 1, math.ceil(1.25 * n * 1e3 * args.window / max(got, 1e-3)))
        calls[k] = math.ceil(1.3 * n)      # a third against run-to-run spread (the drivers allocate and read back: more spread than raw calls)
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
        say(f"    {k:<44s} median {med:9.3f} ms   fastest {min(v):9.3f}   slowest {max(v):9.3f}   ({len(v)} windows of {calls[k]} calls)   "
            f"{nbytes[k] / 1e9:7.3f} GB -> {rate / 1e12:6.3f} TB/s = {100 * rate / HBM_MEASURED:5.1f} % of 6.29 TB/s "
            f"({100 * rate / HBM_SPEC:4.1f} % of 8.0)")
    return {k: statistics.median(v) for k, v in ms.items()}


def trajectory(T, C, seed):
    """[T, C] float32 on the device, time-ordered like MD frames: a chain dwelling in one of four wells for about 500 frames."""
    g = torch.Generator(device=dev).manual_seed(seed)
    jumps = torch.rand(T, device=dev, generator=g) < 0.002
    state = torch.cumsum(jumps.to(torch.int64), 0) % 4
    centres = 4 * torch.rand(4, C, device=dev, generator=g) - 2
    return (centres[state] + 0.05 * torch.randn(T, C, device=dev, generator=g)).to(torch.float32).contiguous()


def raw_calls(X, pairs, ex, ey, bx, by, path):
    """The device part alone: tw_joint_histogram_path on preallocated outputs, nothing read back."""
    lib = _lib.load()
    P = len(pairs)
    pd = torch.as_tensor(np.asarray(pairs, dtype=np.int32)).to(dev)
    counts = torch.zeros(P, bx, by, dtype=torch.int64, device=dev)
    outside = torch.zeros(P, 3, dtype=torch.int64, device=dev)
    exd, eyd = torch.as_tensor(ex).to(dev), torch.as_tensor(ey).to(dev)
    s = _lib.stream_ptr(dev)
    keep = (pd, counts, outside, exd, eyd)

    def fn(_keep=keep):
        _lib.check(lib.tw_joint_histogram_path(X.data_ptr(), X.shape[0], X.shape[1], X.stride(0), X.stride(1), pd.data_ptr(), P,
                                               exd.data_ptr(), bx, eyd.data_ptr(), by, counts.data_ptr(), outside.data_ptr(), path, s),
                   "tw_joint_histogram_path")
    return fn


def same(a, b):
    return all((getattr(a, f) == getattr(b, f)).all() for f in ("counts", "outside"))


say(f"tools/time_joint_histogram.py on {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).multi_processor_count} CUs), "
    f"host {platform.node()}, torch {torch.__version__}, HIP {torch.version.hip}")
say(f"windows of at least {args.window} s of back-to-back calls between HIP events on the launch stream, {args.rounds} per route, routes "
    "alternating, after 2 warm-up calls each; the driver rows include the range pass and the read-back of the ranges where there is "
    "one, np.linspace on the host, the allocation of the outputs and the read-back of the counts; HBM line: 6.29 TB/s measured "
    "(float4 copy), 8.0 TB/s data sheet (MI355X_MICROARCH.md; the line of profiles/evaluate.txt)")
fastest = {}

# ---- TIC 0 x TIC 1 ---------------------------------------------------------------------------------------------------------------------
tics = trajectory(T, 2, seed=0)
say()
say(f"TIC 0 x TIC 1: {T} time-ordered rows x 2 columns ({T * 8 / 1e6:.0f} MB), one pair, {BINS} x {BINS}, "
    f"{_lib.load().tw_joint_histogram_bands(BINS, BINS)} band")
# bytes: the kernel route reads both columns twice (range pass, histogram pass); the torch route also writes and reads its intermediates:
# the finite-masked copy of the range pass, two fp64 casts [P, T], masks, two int64 bin indices and the flat int64 index
bytes_kernel = lambda T, C, P, ranges: (2 if ranges else 1) * T * C * 4
bytes_torch = lambda T, C, P, ranges: (3 if ranges else 1) * T * C * 4 + T * P * (2 * 2 * 8 + 3 * 2 * 8 + 6)
routes = {f"joint_histograms route={r!r}": (lambda r=r: ev.joint_histograms(tics, [[0, 1]], bins=BINS, route=r)) for r in ev.JOINT_ROUTES}
nbytes = dict(zip(routes, (bytes_kernel(T, 2, 1, True), bytes_torch(T, 2, 1, True))))
ref = ev.joint_histograms(tics, [[0, 1]], bins=BINS, route="kernel")
routes["tw_joint_histogram alone"] = raw_calls(tics, [[0, 1]], ref.edges_x, ref.edges_y, BINS, BINS, _lib.TW_JOINT_PATH_AUTO)
nbytes["tw_joint_histogram alone"] = bytes_kernel(T, 2, 1, False)
med = report(*timed(routes), nbytes)
fastest["TIC 0 x TIC 1"] = min(ev.JOINT_ROUTES, key=lambda r: med[f"joint_histograms route={r!r}"])
say(f"    fastest driver route: {fastest['TIC 0 x TIC 1']!r}; the two routes' counts are "
    f"{'EQUAL' if same(ref, ev.joint_histograms(tics, [[0, 1]], bins=BINS, route='torch')) else 'NOT equal'}; "
    f"the fullest bin holds {int(ref.counts.max())} rows")

# ---- Ramachandran, a tetrapeptide ------------------------------------------------------------------------------------------------------
ang = trajectory(T, 6, seed=1).clamp_(-3.1, 3.1)
phi, psi = ang[:, :3], ang[:, 3:]
rp = [(0, 0), (1, 1), (2, 2)]
say()
say(f"Ramachandran counts of a tetrapeptide: {T} time-ordered rows, phi [T, 3] and psi [T, 3] float32 ({T * 24 / 1e6:.0f} MB), three "
    f"(phi, psi) planes of {BINS} x {BINS} in one call (fixed range: no range pass; the driver concatenates phi and psi first)")
routes = {f"ramachandran_histograms route={r!r}": (lambda r=r: analysis.ramachandran_histograms(phi, psi, rp, bins=BINS, route=r))
          for r in ev.JOINT_ROUTES}
routes["_ramachandran (per residue, as before)"] = lambda: ev._ramachandran(phi, psi, rp, BINS)
nbytes = dict(zip(routes, (bytes_kernel(T, 6, 3, False) + 2 * T * 24, bytes_torch(T, 6, 3, False) + 2 * T * 24, bytes_torch(T, 6, 3, False))))
med = report(*timed(routes), nbytes)
fastest["Ramachandran"] = min(ev.JOINT_ROUTES, key=lambda r: med[f"ramachandran_histograms route={r!r}"])
rk = analysis.ramachandran_histograms(phi, psi, rp, bins=BINS, route="kernel")
say(f"    fastest driver route: {fastest['Ramachandran']!r}; the two routes' counts are "
    f"{'EQUAL' if same(rk, analysis.ramachandran_histograms(phi, psi, rp, bins=BINS, route='torch')) else 'NOT equal'}")

# ---- the cost of the bands ---------------------------------------------------------------------------------------------------------------
say()
nb = _lib.load().tw_joint_histogram_bands(1024, 1024)
say(f"a 1024 x 1024 plane of the TIC trajectory: {nb} bands, every band's workgroups read the rows")
routes = {f"joint_histograms bins=1024 route={r!r}": (lambda r=r: ev.joint_histograms(tics, [[0, 1]], bins=1024, route=r)) for r in ev.JOINT_ROUTES}
nbytes = dict(zip(routes, (bytes_kernel(T, 2, 1, True), bytes_torch(T, 2, 1, True))))
big = ev.joint_histograms(tics, [[0, 1]], bins=1024, route="kernel")
routes["tw_joint_histogram alone, 1024 x 1024"] = raw_calls(tics, [[0, 1]], big.edges_x, big.edges_y, 1024, 1024, _lib.TW_JOINT_PATH_AUTO)
nbytes["tw_joint_histogram alone, 1024 x 1024"] = bytes_kernel(T, 2, 1, False)
med = report(*timed(routes), nbytes)
say(f"    (bytes counted once: the {nb} bands re-read the rows from cache); the two routes' counts are "
    f"{'EQUAL' if same(big, ev.joint_histograms(tics, [[0, 1]], bins=1024, route='torch')) else 'NOT equal'}")

# ---- the wave vote -----------------------------------------------------------------------------------------------------------------------
say()
say(f"wave vote against plain LDS atomics: tw_joint_histogram_path alone, {T} rows, {BINS} x {BINS}, the time-ordered TIC rows, the "
    "same rows shuffled, and every row in one bin")
shuffled = tics[torch.randperm(T, device=dev, generator=torch.Generator(device=dev).manual_seed(5))].contiguous()
routes = {}
one_bin = torch.full_like(tics, 0.25)
cases = (("time-ordered", tics), ("shuffled", shuffled), ("every row in one bin", one_bin))
for name, X in cases:
    for pname, path in (("plain", _lib.TW_JOINT_PATH_PLAIN), ("vote", _lib.TW_JOINT_PATH_VOTE)):
        routes[f"{name}, {pname}"] = raw_calls(X, [[0, 1]], ref.edges_x, ref.edges_y, BINS, BINS, path)
med = report(*timed(routes), {k: bytes_kernel(T, 2, 1, False) for k in routes})
for name, _ in cases:
    say(f"    {name}: vote / plain = {med[f'{name}, vote'] / med[f'{name}, plain']:.3f}")

say()
say(f"evaluate.DEFAULT_JOINT_ROUTE = {ev.DEFAULT_JOINT_ROUTE!r}; fastest here: " + ", ".join(f"{k}: {v!r}" for k, v in fastest.items()))
if args.tests:
    say()
    say("tests/test_joint_histogram_gpu.py, `pytest --durations` on the same machine:")
    for line in open(args.tests).read().splitlines():
        if "test_joint_histogram_gpu.py::" in line or " passed" in line or " failed" in line:
            say("    " + line.strip())

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
