"""Build libtimewarp_hip.so for gfx950 with hipcc (in-tree, so the .so travels to the GPU box).

    python -m timewarp_amd.build            # rebuild if any source is newer than the library
"""
import glob
import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
PREBUILT = os.environ.get("TW_HIP_LIB")  # a user's prebuilt library: loaded as is, never rebuilt or overwritten
LIB_PATH = PREBUILT or os.path.join(LIB_DIR, "libtimewarp_hip.so")
STAMP_PATH = os.path.join(LIB_DIR, ".build_stamp")  # sha256 of the sources + flags the in-tree library was built from
SOURCES = ["tw_kernels.hip", "tw_equivariant.hip", "tw_pack.hip", "tw_netblock.hip", "tw_netblock_dense.hip", "tw_netblock_h3.hip", "tw_energy.hip", "tw_md.hip", "tw_mh_step.hip", "tw_analysis.hip", "tw_evaluate.hip", "tw_api.hip"]
# the generated asm statements (tools/h3_asm_manifest.py; committed, so a build needs hipcc only): every include the kernel
# can see, so that an edited statement always reaches the rebuild stamp
HEADERS = [os.path.join(CSRC, "tw_common.h"), os.path.join(CSRC, "tw_amber.h"), os.path.join(CSRC, "tw_nb_f32.h"), os.path.join(HERE, "..", "include", "timewarp_hip.h")] + \
    sorted(glob.glob(os.path.join(CSRC, "*.inc")))


FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
if os.environ.get("TW_EXPERIMENTS") == "1":
    # developer build: the wrong-result timing switches of tw_debug_set_flags (the TW_DEBUG_EXP_* bits) exist only here
    FLAGS.append("-DTW_EXPERIMENTS")


def _source_digest() -> str:
    """Content hash of everything the library is built from (mtimes do not survive a copy of the tree)."""
    h = hashlib.sha256(" ".join(FLAGS).encode())
    for d in sorted([os.path.join(CSRC, s) for s in SOURCES] + HEADERS):
        h.update(os.path.basename(d).encode())
        with open(d, "rb") as f:
            h.update(f.read())
    for src in sorted(EXTRA_FLAGS):
        h.update((src + " ".join(EXTRA_FLAGS[src])).encode())
    return h.hexdigest()


def _stale() -> bool:
    if PREBUILT:
        return False
    if not (os.path.exists(LIB_PATH) and os.path.exists(STAMP_PATH)):
        return True
    with open(STAMP_PATH) as f:
        return f.read().strip() != _source_digest()


def stale() -> bool:
    """The in-tree library is missing or was not built from the sources next to it (by content hash)."""
    return _stale()


# Per-file extra flags (none needed at present; building the split-fp16 kernel without packed-fp32 VALU
# ops, which stall behind the matrix pipe in tools/probe/mfma_valu_overlap.hip, was measured: no gain).
EXTRA_FLAGS = {}


def hipcc_path():
    p = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return p if os.path.exists(p) else None


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP translation unit for gfx950 and link the C-ABI shared library.  A TW_HIP_LIB library is
    the user's: it is returned as is and never rebuilt in place."""
    if PREBUILT:
        if not os.path.exists(PREBUILT):
            raise RuntimeError(f"TW_HIP_LIB={PREBUILT} does not exist")
        return PREBUILT
    if not force and not _stale():
        return LIB_PATH
    hipcc = hipcc_path()
    if hipcc is None:
        raise RuntimeError("hipcc not found: cannot build libtimewarp_hip.so")
    os.makedirs(LIB_DIR, exist_ok=True)
    # one builder at a time (several ranks of a torchrun job may find the library missing together)
    import fcntl

    lock = open(os.path.join(LIB_DIR, ".build.lock"), "w")
    fcntl.flock(lock, fcntl.LOCK_EX)
    try:
        if not force and not _stale():
            return LIB_PATH
        return _build_locked(hipcc, verbose)
    finally:
        fcntl.flock(lock, fcntl.LOCK_UN)
        lock.close()


def _build_locked(hipcc: str, verbose: bool) -> str:
    digest = _source_digest()
    if os.path.exists(STAMP_PATH):
        os.remove(STAMP_PATH)  # no stamp while the objects and the library are being replaced
    def compile_one(src):
        obj = os.path.join(LIB_DIR, src.replace(".hip", ".o"))
        cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        res = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        err = "\n".join(l for l in res.stderr.splitlines() if "is not a recognized feature for this target" not in l)
        if err.strip():
            sys.stderr.write(err + "\n")
        if res.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src} (exit {res.returncode})")
        return obj

    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 1)) as pool:  # one hipcc per translation unit
        objs = list(pool.map(compile_one, SOURCES))
    # link next to the target and rename over it: a process that is not holding the lock (another rank's dlopen)
    # sees the old complete library or the new complete one, never a half-written file
    tmp = LIB_PATH + f".tmp{os.getpid()}"
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    try:
        subprocess.run(cmd, check=True)
        os.replace(tmp, LIB_PATH)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    with open(STAMP_PATH + ".tmp", "w") as f:
        f.write(digest)
    os.replace(STAMP_PATH + ".tmp", STAMP_PATH)
    return LIB_PATH


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
