"""What the tools/gen_h3_*_asm.py generators share word for word: register-range formatting, the MFMA-shadow weaver, the
--out-dir argument, the writers of a statement's two include files, and the loader that runs a generator as a module.
(The stage hand-offs and GEMM stages are NOT here: they differ per statement family in substance.)"""
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def vr(base, n=4):
    return f"v[{base}:{base + n - 1}]"


def ar(base, n=4):
    return f"a[{base}:{base + n - 1}]"


def sr(base, n=2):
    return f"s[{base}:{base + n - 1}]"


def weave(mfmas, valu, misc, valu_per, misc_per, skip=0):
    """Each MFMA (after the first `skip`) is followed by up to `valu_per` VALU ops and `misc_per` other items, spread so
    the queues empty by the last MFMA (leftovers are appended).  An item that is itself a list is atomic."""
    out = []
    valu, misc = list(valu), list(misc)
    n = len(mfmas)

    def emit(item):
        out.extend(item if isinstance(item, list) else [item])

    for i, m in enumerate(mfmas):
        out.append(m)
        if i < skip:
            continue
        left = n - i
        for _ in range(min(valu_per, -(-len(valu) // left)) if valu else 0):
            emit(valu.pop(0))
        for _ in range(min(misc_per, -(-len(misc) // left)) if misc else 0):
            emit(misc.pop(0))
    for item in valu + misc:
        emit(item)
    return out


def out_dir(argv, default="timewarp_amd/csrc"):
    """--out-dir=DIR of a generator's command line (the last one wins)."""
    for a in argv[1:]:
        if a.startswith("--out-dir="):
            default = a.split("=", 1)[1]
    return default


def write_statement(path, header, lines):
    """tw_*_asm.inc: `header` (comment text, may span lines), then one quoted instruction per line."""
    with open(path, "w") as f:
        f.write("\n".join([header] + ['"' + l + '\\n\\t"' for l in lines]) + "\n")


def clobber_regs(n_v, n_a, s_lo, s_hi):
    """v0..v(n_v-1), a0..a(n_a-1), s(s_lo)..s(s_hi-1) and the flags every statement clobbers."""
    return [f"v{i}" for i in range(n_v)] + [f"a{i}" for i in range(n_a)] + [f"s{i}" for i in range(s_lo, s_hi)] + \
        ["vcc", "scc", "memory"]


def write_clobbers(path, header, regs):
    """tw_*_clobbers.inc: `header`, then the quoted names, 12 per line."""
    q = [f'"{r}"' for r in regs]
    with open(path, "w") as f:
        f.write("\n".join([header] + [", ".join(q[i:i + 12]) + ("," if i + 12 < len(q) else "")
                                      for i in range(0, len(q), 12)]) + "\n")


def load_generator(name, argv=None):
    """Run tools/<name>.py as a fresh module object.  The generators read their flags from sys.argv at import: `argv` (flags
    only) stands in for the command line while the module executes; None leaves the caller's own in place."""
    old = sys.argv
    tag = "" if argv is None else "_" + "_".join(a.strip("-").replace("=", "") for a in argv)
    if argv is not None:
        sys.argv = [name] + list(argv)
    try:
        spec = importlib.util.spec_from_file_location(name + tag, os.path.join(HERE, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        sys.argv = old
    return m
