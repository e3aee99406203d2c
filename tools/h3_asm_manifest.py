"""The generated asm statements of timewarp_amd/csrc/tw_netblock_h3.hip: one row per generator invocation - the script, its
arguments and the include files it writes.  tools/regen_asm.py runs the rows; tests/test_host_logic.py holds the committed
files to them (and the set of files in csrc to the rows' outputs).  A new statement is one row here, one include site in
the kernel and, if its %[name] operands are a new set, one H3_OPS_* macro there."""
import os
import subprocess
import sys
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "timewarp_amd", "csrc")

Row = namedtuple("Row", "script args outputs")


def _row(script, *args, stem, clobbers=True):
    """`stem`: the run writes tw_<stem>_asm.inc and, unless it shares another row's, tw_<stem>_clobbers.inc."""
    return Row(f"tools/gen_h3_{script}_asm.py", list(args),
               (f"tw_{stem}_asm.inc",) + ((f"tw_{stem}_clobbers.inc",) if clobbers else ()))


ROWS = [
    # split-fp16 statements on 48-token waves: tw_h3_*
    _row("ffn", "--shape=ffn", stem="h3_ffn"),
    _row("ffn", "--shape=in", stem="h3_in"),
    _row("ffn", "--shape=out", stem="h3_out"),
    _row("attn", stem="h3_attn"),
    _row("attn", "--mode=windowed", stem="h3_attnw"),
    _row("attn_wide", stem="h3_attns"),
    _row("dense_attn", stem="h3_attnd"),
    _row("enc", stem="h3_enc"),
    _row("enc", "--mode=windowed", stem="h3_encw", clobbers=False),   # (the clobber list is the row's above)
    # the single-MFMA variant (TW_PATH_FUSED_H1): tw_h1_*
    _row("ffn", "--shape=in", "--h1", stem="h1_in"),
    _row("ffn", "--shape=out", "--h1", stem="h1_out"),
    _row("enc", "--h1", stem="h1_enc"),
    _row("enc", "--mode=windowed", "--h1", stem="h1_encw", clobbers=False),
    _row("ffn", "--shape=ffn", "--h1", stem="h1_ffn"),
    _row("attn_wide", "--h1", stem="h1_attns"),
    # ... on the six-slot ring (one barrier per pair of FFN stages): tw_h1r_*
    _row("ffn", "--shape=in", "--h1", "--ring6", stem="h1r_in"),
    _row("ffn", "--shape=out", "--h1", "--ring6", stem="h1r_out"),
    _row("enc", "--h1", "--ring6", stem="h1r_enc"),
    _row("enc", "--mode=windowed", "--h1", "--ring6", stem="h1r_encw", clobbers=False),
    # wide layout, 65-96 atoms at the 96-slot stride: three-group windows, tw_h?_attns3_*
    _row("attn_wide", "--ng=3", stem="h3_attns3"),
    _row("attn_wide", "--ng=3", "--h1", stem="h1_attns3"),
    # ... 161-192 atoms, one molecule per workgroup: six-group windows, tw_h?_attns6_*
    _row("attn_wide", "--ng=6", stem="h3_attns6"),
    _row("attn_wide", "--ng=6", "--h1", stem="h1_attns6"),
    # 64-token waves (49-64 atoms): tw_h?n4_*
    _row("ffn", "--shape=ffn", "--nt=4", stem="h3n4_ffn"),
    _row("attn", "--nt=4", stem="h3n4_attn"),
    _row("ffn", "--shape=in", "--nt=4", stem="h3n4_in"),
    _row("ffn", "--shape=out", "--nt=4", stem="h3n4_out"),
    _row("ffn", "--shape=ffn", "--nt=4", "--h1", stem="h1n4_ffn"),
    _row("attn", "--nt=4", "--h1", stem="h1n4_attn"),
    _row("ffn", "--shape=in", "--nt=4", "--h1", stem="h1n4_in"),
    _row("ffn", "--shape=out", "--nt=4", "--h1", stem="h1n4_out"),
    # the encoder stack of the 64-token build as one statement, tw_h?n4_enc_*
    _row("enc", "--nt=4", stem="h3n4_enc"),
    _row("enc", "--nt=4", "--h1", stem="h1n4_enc"),
    # ... and of the wide layout (five- / three- / six-group key windows), tw_h?w{,3,6}_enc_*
    _row("enc", "--wide", stem="h3w_enc"),
    _row("enc", "--wide", "--h1", stem="h1w_enc"),
    _row("enc", "--wide", "--ng=3", stem="h3w3_enc"),
    _row("enc", "--wide", "--ng=3", "--h1", stem="h1w3_enc"),
    _row("enc", "--wide", "--ng=6", stem="h3w6_enc"),
    _row("enc", "--wide", "--ng=6", "--h1", stem="h1w6_enc"),
    # ... and of the dense softmax model, tw_h?d_enc_*
    _row("enc", "--dense", stem="h3d_enc"),
    _row("enc", "--dense", "--h1", stem="h1d_enc"),
    # ... and on 64-token waves (49-64 atoms): tw_h3n4d_enc_*
    _row("enc", "--dense", "--nt=4", stem="h3n4d_enc"),
    # ... and of the paired 64-token layout (97-128 atoms), tw_h?n4p_enc_*
    _row("enc", "--nt=4", "--pair", stem="h3n4p_enc"),
    _row("enc", "--nt=4", "--pair", "--h1", stem="h1n4p_enc"),
]


def outputs():
    """Every include file the rows declare, sorted."""
    return sorted(n for r in ROWS for n in r.outputs)


def run(row, out_dir=None, env=None):
    """One generator run from the repository root, into `out_dir` (default: the generator's own, csrc)."""
    subprocess.run([sys.executable, row.script] + row.args + ([f"--out-dir={out_dir}"] if out_dir else []), cwd=ROOT,
                   check=True, env=env, stdout=subprocess.DEVNULL)
