"""What the full-step option and checkpointing cost (profiles/md_checkpoint.txt), on alanine dipeptide (22 atoms, one wave per row)
and the reference's 691-atom test protein (1hgv, sixteen waves per row; the systems of tools/time_md_trajectory.py):

  1. per-step time of the recording kernel through the OLD entry point (`LangevinDynamics.trajectory` -> `tw_langevin_trajectory`), a
     frame at every step, this build against another build of the library (`--other-lib`: the parent commit's libtimewarp_hip.so)
     in alternating child processes - one process loads one library.  Without `--other-lib` the build alternates with itself,
     which gives the spread a difference has to be held against;
  2. the same kernel with TW_RECORD_FULL_STEP_VELOCITIES against flags 0, alternating calls in one process;
  3. one segment flush and one checkpoint of `simulate_trajectory` (device -> host copy and the file, into a temporary directory)
     for 256 replicas of alanine dipeptide and 16 of the protein, and what share of wall time a checkpoint interval then costs.

Method as tools/time_md_trajectory.py: one warm-up call, then calls bracketed by HIP events on the launch stream; the host-side
costs of 3 by the wall clock around a synchronised call.  `python tools/time_md_checkpoint.py [--other-lib PATH] [--out FILE]`"""
import argparse, ctypes, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
ROUNDS = 3          # child processes per library in part 1
REPEATS = 5         # timed calls per case


def systems():
    import numpy as np, torch
    from timewarp_amd import synthetic
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from timewarp_amd.forcefield import ELEMENT_MASSES, amber99sbildn_obc_tables

    _, coords, masses = synthetic.alanine_dipeptide_state()
    yield "ad", "alanine dipeptide (22 atoms)", AmberPotentialEnergyTorch.alanine_dipeptide(), masses, coords, 2000, 256
    z = np.load(os.path.join(GOLDEN, "energy_kat_1hgv.npz"))
    names = [str(n) for n in z["atom_names"]]
    tables = amber99sbildn_obc_tables(names, [str(r) for r in z["residue_names"]], [int(i) for i in z["residue_ids"]], improper_neighbour_order="pyset")
    masses = torch.tensor([ELEMENT_MASSES[next(ch for ch in n if ch.isalpha())] for n in names], dtype=torch.float32)
    yield "1hgv", "1hgv (691 atoms)", AmberPotentialEnergyTorch(tables), masses, torch.from_numpy(z["positions"][1].astype(np.float32)), 50, 16


def timed(fn, repeats=REPEATS):
    """ms of `repeats` calls, HIP events on the launch stream, after one warm-up call"""
    import torch

    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def prepared(energy, masses, coords, rows):
    import torch
    from timewarp_amd import simulation as S
    from timewarp_amd.md import LangevinDynamics

    md = LangevinDynamics.for_energy(energy, masses, seed=1)
    x = coords.to("cuda")[None].repeat(rows, 1, 1).contiguous()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    return md, md.new_state(x, S.thermal_velocities(md.masses, md.kbT, x, gen))


def child_old_entry_point():
    """Part 1, one process: us per step through tw_langevin_trajectory, a frame at every step -> one JSON line."""
    import numpy as np
    from timewarp_amd import _lib, build

    if not hasattr(ctypes.CDLL(build.LIB_PATH), "tw_langevin_trajectory_opts"):      # a library from before the option
        _lib.SIGNATURES.pop("tw_langevin_trajectory_opts")
    out = {}
    for key, _, energy, masses, coords, n, rows in systems():
        md, state = prepared(energy, masses, coords, rows)
        ms = timed(lambda: md.trajectory(None, None, np.arange(1, n + 1), num_steps=n, state=state))
        out[key] = [float(np.median(ms)) / n * 1e3, float(min(ms)) / n * 1e3]
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--other-lib", default=None, help="another build of libtimewarp_hip.so to alternate with (the parent commit's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "md_checkpoint.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child_old_entry_point()
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    # ---- 1: the old entry point, this build against the other one, alternating processes
    say("1. tw_langevin_trajectory (the old entry point), a frame at every step, us per step: median (minimum) of 5 launches per process")
    say(f"   alanine dipeptide x 256 rows, 2000 steps per launch; 1hgv x 16 rows, 50 steps per launch; {ROUNDS} processes per library, alternating")
    other = "other build" if args.other_lib else "this build again"
    results = {"this build": [], other: []}
    for i in range(2 * ROUNDS):
        who = "this build" if i % 2 == 0 else other
        env = dict(os.environ)
        if who == "other build":
            env["TW_HIP_LIB"] = os.path.abspath(args.other_lib)
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                             timeout=600)
        if run.returncode != 0:
            raise SystemExit(f"child process failed ({run.returncode}): {run.stderr[-2000:]}")
        got = json.loads(next(l for l in run.stdout.splitlines() if l.startswith("RESULT "))[7:])
        results[who].append(got)
        say(f"   {who:16s} run {i // 2 + 1}:  alanine dipeptide {got['ad'][0]:8.2f} ({got['ad'][1]:8.2f})   1hgv {got['1hgv'][0]:9.1f} ({got['1hgv'][1]:9.1f})")
    for key, label in (("ad", "alanine dipeptide"), ("1hgv", "1hgv")):
        mine, theirs = [r[key][0] for r in results["this build"]], [r[key][0] for r in results[other]]
        spread = max(max(theirs) - min(theirs), max(mine) - min(mine))
        mean = lambda a: sum(a) / len(a)
        say(f"   {label}: this build {mean(mine):.2f}, {other} {mean(theirs):.2f} us per step (means of the medians): difference "
            f"{mean(mine) - mean(theirs):+.2f} us = {100 * (mean(mine) / mean(theirs) - 1):+.2f} %; spread of one library across its runs {spread:.2f} us")

    import numpy as np, torch
    from timewarp_amd import simulation as S

    # ---- 2: full-step flag against flags 0, alternating calls in this process
    say()
    say("2. the same launches with velocities=\"full-step\" (tw_langevin_trajectory_opts, TW_RECORD_FULL_STEP_VELOCITIES) against \"stored\",")
    say("   a frame at every step, alternating calls, 5 each after a warm-up of both: median ms per launch")
    for key, label, energy, masses, coords, n, rows in systems():
        md, state = prepared(energy, masses, coords, rows)
        every = np.arange(1, n + 1)
        ms = {"stored": [], "full-step": []}
        for kind in ms:
            md.trajectory(None, None, every, num_steps=n, state=state, velocities=kind)
        torch.cuda.synchronize()
        for _ in range(REPEATS):
            for kind in ms:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                md.trajectory(None, None, every, num_steps=n, state=state, velocities=kind)
                b.record()
                b.synchronize()
                ms[kind].append(a.elapsed_time(b))
        s, f = float(np.median(ms["stored"])), float(np.median(ms["full-step"]))
        say(f"   {label} x {rows} rows, {n} steps: stored {s:9.3f} ms (min {min(ms['stored']):9.3f}, max {max(ms['stored']):9.3f})   full-step {f:9.3f} ms "
            f"(min {min(ms['full-step']):9.3f}, max {max(ms['full-step']):9.3f})   ratio {f / s:.4f}")

    # ---- 3: one segment flush and one checkpoint
    say()
    say("3. one segment flush (device -> host copy of the buffered frames + the segment file) and one checkpoint (state copy, finite check,")
    say("   checkpoint file), wall clock around a synchronised call, median of 5, files in a temporary directory")
    for key, label, energy, masses, coords, n, rows in systems():
        md, state = prepared(energy, masses, coords, rows)
        T = 100 if key == "ad" else 50
        _, _, frames = md.trajectory(None, None, np.arange(1, T + 1), num_steps=T, state=state)
        fp = S.run_fingerprint(energy, md, state[:, 0].to(torch.float32), None, burn_in=0, sampling=T, seed=1, reports=np.arange(1, T + 1),
                               velocities="stored", redraw_velocities=False, minimize=False, min_tol=2.0)
        start = state[:, 0].to(torch.float32).cpu().numpy()
        with tempfile.TemporaryDirectory() as tmp:
            seg, ck = [], []
            for i in range(REPEATS + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                S.write_segment(S.segment_path(os.path.join(tmp, "t"), i), [frames])
                t1 = time.perf_counter()
                finite = torch.isfinite(state).reshape(rows, -1).all(dim=1).cpu().numpy()
                S.write_checkpoint(S.checkpoint_path(os.path.join(tmp, "t")), fp, steps_done=T, integrator_step=md.steps_done, state=state.cpu().numpy(),
                                   redrawn=True, n_segments=i + 1, start_coords=start)
                t2 = time.perf_counter()
                assert finite.all()
                if i:
                    seg.append(1e3 * (t1 - t0)), ck.append(1e3 * (t2 - t1))
            seg_bytes = os.path.getsize(S.segment_path(os.path.join(tmp, "t"), 0))
            ck_bytes = os.path.getsize(S.checkpoint_path(os.path.join(tmp, "t")))
        s, c = float(np.median(seg)), float(np.median(ck))
        say(f"   {label} x {rows} rows: segment of {T} frames per row ({seg_bytes / 2 ** 20:.1f} MiB) {s:8.1f} ms = {s / T:6.2f} ms per frame of all rows;   "
            f"checkpoint ({ck_bytes / 2 ** 20:.2f} MiB) {c:7.1f} ms")
        say(f"      a checkpoint with a full segment every 300 s: {100 * (s + c) / 300e3:.4f} % of wall time; under 1 % down to one every {(s + c) / 10:.1f} s")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
