"""The generated asm statements of timewarp_amd/csrc/tw_netblock_h3.hip: one row per statement - its generator, the
generator's options, and the stem of the include files it is written to.  render() turns a row into those files' text;
tools/regen_asm.py writes every row, tests/test_host_logic.py holds the committed files to them (and the set of files in csrc
to the rows' outputs), and the generators' command lines (main() here) name their outputs by the row with their options.  A
new statement is one row here, one include site in the kernel and, if its %[name] operands are a new set, one H3_OPS_* macro
there."""
import os
import sys
from collections import namedtuple

from gen_h3_attn_asm import AttnStatement
from gen_h3_attn_wide_asm import WideAttnStatement
from gen_h3_dense_attn_asm import DenseAttnStatement
from gen_h3_enc_asm import EncStatement
from gen_h3_ffn_asm import FfnStatement
from h3_asm_common import include_files, parse_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "timewarp_amd", "csrc")
GENERATORS = {"ffn": FfnStatement, "attn": AttnStatement, "attn_wide": WideAttnStatement, "dense_attn": DenseAttnStatement,
              "enc": EncStatement}

Row = namedtuple("Row", "script flags options stem clobbers outputs")


def _row(script, *flags, stem, clobbers=True):
    """`flags`: the options as the command line spells them, in the order the files' header lines carry them.  `stem`: the row
    is written to tw_<stem>_asm.inc and, unless it shares another row's, tw_<stem>_clobbers.inc."""
    return Row(script, flags, parse_flags(flags), stem, clobbers,
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
    _row("ffn", "--shape=ffn", "--h1", "--nt=4", stem="h1n4_ffn"),
    _row("attn", "--nt=4", "--h1", stem="h1n4_attn"),
    _row("ffn", "--shape=in", "--h1", "--nt=4", stem="h1n4_in"),
    _row("ffn", "--shape=out", "--h1", "--nt=4", stem="h1n4_out"),
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
    _row("enc", "--nt=4", "--dense", stem="h3n4d_enc"),
    # ... and of the paired 64-token layout (97-128 atoms), tw_h?n4p_enc_*
    _row("enc", "--nt=4", "--pair", stem="h3n4p_enc"),
    _row("enc", "--nt=4", "--pair", "--h1", stem="h1n4p_enc"),
]


def outputs():
    """Every include file the rows declare, sorted."""
    return sorted(n for r in ROWS for n in r.outputs)


def construct(script, flags=(), ffn=(), attn=(), enc=()):
    """The generator `script` for a command line's `flags`; ffn / attn / enc: the flag sets of H3_FFN_EXPERIMENT,
    H3_ATTN_EXPERIMENT and H3_ENC_EXPERIMENT, each handed to the generators that environment variable speaks to."""
    experiments = dict(experiment=ffn) if script == "ffn" else \
        dict(experiment=enc, ffn_experiment=ffn, attn_experiment=attn) if script == "enc" else dict(experiment=attn)
    return GENERATORS[script](**parse_flags(flags), **experiments)


def render(row, **experiments):
    """{file name: text} of a row, in-process."""
    return include_files(construct(row.script, row.flags, **experiments), row.script, row.flags, row.stem, row.clobbers)


def run(row, out_dir=None, env=None):
    """Write a row's files into `out_dir` (default: csrc) and return them.  `env`: a mapping whose H3_FFN_EXPERIMENT /
    H3_ATTN_EXPERIMENT / H3_ENC_EXPERIMENT switches apply (default: none - the process's own environment is not looked at)."""
    experiments = {k: set(filter(None, (env or {}).get(f"H3_{k.upper()}_EXPERIMENT", "").split(","))) for k in ("ffn", "attn", "enc")}
    files = render(row, **experiments)
    for name, text in files.items():
        with open(os.path.join(out_dir or CSRC, name), "w") as f:
            f.write(text)
    return files


def main(script):
    """The command line of tools/gen_h3_<script>_asm.py: [flags] [--out-dir=DIR], experiments from the environment.  The one
    place that reads either; the files are the ones of the manifest row with these options."""
    out_dir, flags = None, []
    for a in sys.argv[1:]:
        if a.startswith("--out-dir="):
            out_dir = a.split("=", 1)[1]   # (relative to the caller's directory; the default is this repository's csrc)
        else:
            flags.append(a)
    options = parse_flags(flags)
    if script == "ffn":
        options.setdefault("shape", "ffn")
    rows = [r for r in ROWS if r.script == script and r.options == options]
    if not rows:
        sys.exit(f"gen_h3_{script}_asm.py {' '.join(flags)}: no row of tools/h3_asm_manifest.py has these options")
    lines = run(rows[0], out_dir, os.environ)[rows[0].outputs[0]].splitlines()
    print(f"{rows[0].stem}: {sum(l.startswith(chr(34)) for l in lines)} instructions, {sum('v_mfma' in l for l in lines)} MFMAs")
