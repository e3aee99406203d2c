#!/usr/bin/env python3
"""One line per (model, flags, path, atoms, rows) with the net-block instantiation the split-fp16 / single-MFMA path selects
(tw_flow_selected_kernel; "-" where the path refuses the case) and the workspace a caller sizes for it (tw_flow_workspace_bytes):
two libraries route alike exactly when their outputs are equal line for line.  No GPU needed.  Run once per library, each in a
fresh process (TW_HIP_LIB names a library other than the in-tree one):

    TW_HIP_LIB=$PWD/timewarp_amd/lib/ab/libtimewarp_hip_parent.so python tools/h3_route_digest.py > parent.txt
    python tools/h3_route_digest.py > new.txt && cmp parent.txt new.txt

Cases: the three synthetic models (kernel attention, dense, dense + 128 position features), the chebyshev shape and the 1-, 12- and
18-head shapes of tests/model_shapes.py; both paths; 1 .. 193 atoms; eight row counts; fifteen debug words (FLAG_SETS).  The last
line counts the cases and the distinct instantiations selected.
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import timewarp_amd as tw  # noqa: E402
from tests import model_shapes as ms  # noqa: E402
from timewarp_amd import _lib, synthetic  # noqa: E402
from timewarp_amd._lib import DebugFlag as F  # noqa: E402

ROWS = (1, 8, 100, 256, 512, 768, 1000, 4096)
ATOMS = range(1, 194)
PATHS = (("h3", _lib.TW_PATH_FUSED_H3), ("h1", _lib.TW_PATH_FUSED_H1))
FLAG_SETS = (
    ("0", 0), ("NEVER_WIDE", F.NEVER_WIDE), ("ALWAYS_WIDE", F.ALWAYS_WIDE), ("ALWAYS_NT4", F.ALWAYS_NT4), ("NEVER_NT4", F.NEVER_NT4),
    ("WIDE_FIVE_GROUP_WINDOWS", F.WIDE_FIVE_GROUP_WINDOWS), ("ALWAYS_WIDE|WIDE_FIVE_GROUP_WINDOWS", F.ALWAYS_WIDE | F.WIDE_FIVE_GROUP_WINDOWS),
    ("ALWAYS_NT4|PER_SECTION", F.ALWAYS_NT4 | F.PER_SECTION), ("NEVER_PAIRED", F.NEVER_PAIRED), ("PER_SECTION", F.PER_SECTION),
    ("COMPILED_CPP", F.COMPILED_CPP), ("SECTION_STAMPS", F.SECTION_STAMPS), ("DUMP_ATTENTION", F.DUMP_ATTENTION),
    ("PER_SECTION|ENC_WITH_DUMPS", F.PER_SECTION | F.ENC_WITH_DUMPS), ("SECTION_STAMPS|ENC_WITH_DUMPS", F.SECTION_STAMPS | F.ENC_WITH_DUMPS),
)


def models():
    rff = synthetic.transformer_nvp_config()
    rff.transformer_nvp_config.rff_position_encoder_config = tw.RFFPositionEncoderConfig(128, 1.0, 1.0)
    yield "kernel", synthetic.kernel_transformer_nvp_config()
    yield "dense", synthetic.transformer_nvp_config()
    yield "dense+rff", rff
    for name in ("k128-h5-cheb", "k128-h1", "k128-h12", "k128-h18"):
        yield name, ms.BY_NAME[name].config()


def main():
    lib = _lib.load()
    cases, picked = 0, set()
    for tag, cfg in models():
        d = tw.model_constructor(cfg).dims.to_desc()
        for fname, flags in FLAG_SETS:
            _lib.check(lib.tw_debug_set_flags(_lib.debug_word(flags)), "tw_debug_set_flags")
            for pname, path in PATHS:
                for V in ATOMS:
                    for rows in ROWS:
                        name = lib.tw_flow_selected_kernel(C.byref(d), V, rows, path).decode()
                        ws = lib.tw_flow_workspace_bytes(C.byref(d), rows, V)
                        print(f"{tag} {fname} {pname} V={V} rows={rows}: {name or '-'} ws={ws}")
                        cases += 1
                        if name:
                            picked.add(name)
    _lib.check(lib.tw_debug_set_flags(0), "tw_debug_set_flags")
    print(f"# {cases} cases, {len(picked)} instantiations selected")


if __name__ == "__main__":
    main()
