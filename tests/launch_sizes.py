"""The launch sizes at which the per-op paths change route: ONE case table, shared by tests/test_launch_sizes_cpu.py (the
restatement and the references alone) and tests/test_launch_sizes_gpu.py (the HIP kernels against the float32 oracle, and the route
the library reports against the restatement).  TEST INFRASTRUCTURE ONLY.

On TW_PATH_SIMPLE / TW_PATH_SIMPLE_H3 the launch size - rows x atoms, not the atoms alone - picks the route in three places, restated
here (`fold_plan`, `tokens_nt4` / `ffn_form` / `io_form`, `sdpa_plan`; `route` spells them as tw_last_per_op_route does):
- csrc/tw_kernels.hip: per_op_plan - the folded mixing's head_parts by fold_wgs = n_rows * ceil(V / 128): 6 below 128, 2 below 400,
  one workgroup per query tile (GEMM, residual and LayerNorm 1 in its epilogue) from 400 on;
- csrc/tw_netblock_h3.hip: h3_ffn_tokens / h3_io_tokens / h3_tokens_nt4 - the token-list launches by n_tokens = n_rows * V: the hidden
  layer over four workgroups per 192-token tile while ceil(n_tokens / 192) * 2 <= 256, 48-token waves unsplit above, 64-token waves
  where they need fewer rounds' worth of the 256 CUs, 48-token waves again behind that window;
- csrc/tw_kernels.hip: launch_sdpa - sdpa_mfma_kernel's q_tiles_per_wave = n_rows * H * V16 / 4096 clipped to [1, ceil(V16 / 4)] and its
  grid-z chunks.
A routing change in the library is edited here too.

A *case* is a model (the full kernel model, 6 heads; the full dense model, 8 heads of 16), an atom count, a row count and a call form:
"sample" - the reverse pass, ONE conditioning state and n_rows latents - or "loglik" - n_rows rows that each carry their own
conditioning state.  Every case masks tails: the one conditioning row of "sample" always, the rows of "loglik" raggedly, with every
eleventh row full length - at 65 / 129 / 193 / 257 atoms the last 16-query tile (and at 129 / 257 the last 128-query tile) holds ONE
atom, and only a full-length row shows what a kernel does with it.  NAMED_CASES gives each launch size one call form; CASES runs it in the other one as well
(an id takes well under a second on the GPU).  Each case states the regime it is in the table for as python expressions over the
restatement (`facts`, evaluated by the CPU file): the smallest row counts on each side of each threshold.

The rows of a launch are independent given their conditioning state, so the oracle runs on a fixed subset (`checked_rows`): rows 0, 1,
S - 2, S - 1 and row 11 (with row 0 the first full-length rows of "loglik"); for the token-list cases the rows on both sides of the first tile edge, of the last (ragged) tile's start and of the
chip-round edge (workgroup 256), for 192- and for 256-token tiles (the default and the forced alternative); 8 rows drawn from a seed
derived from the case name.  The 128-query tile edge of the fold (129 / 193 atoms) and the chunk edge of sdpa_mfma_kernel lie INSIDE
every row: every checked row crosses them.

The float32 oracle against the float64 oracle on the checked rows (helpers.rel_err, tests/test_launch_sizes_cpu.py holds 2.5e-6, a
quarter of the parity bar), measured on the CPU with 4, 8 and 16 threads: worst 2.0e-6 (kernel-v193-s255-sample, y_coords, 4 threads),
the reverse passes 0.7e-6 .. 2.0e-6, the likelihoods 0.7e-7 .. 3.0e-7; five reverse passes took another draw (RESEED).  The coordinate
spread is tests/model_shapes.py's.
"""
import functools
import zlib
from dataclasses import dataclass
from typing import Tuple

import torch

from oracle import flow_oracle as fo
from tests import helpers as H

SIMPLE, SIMPLE_H3 = 2, 5
H3_CUS = 256          # csrc/tw_netblock_h3.hip: one token-list workgroup per CU, a launch is whole rounds of the chip
FFN_SPLIT = 4         # H3_FFN_SPLIT
D_MODEL, D_FF = 128, 2048


# ---------------------------------------------------------------------------------------------------------------------
# the three decisions, restated
# ---------------------------------------------------------------------------------------------------------------------
def _flag(name):
    from timewarp_amd._lib import DebugFlag

    return int(getattr(DebugFlag, name))


def fold_plan(model, heads, V, n_rows, path, flags=0):
    """per_op_plan: (head_parts, gemm_inside, ln_inside) of the folded mixing; head_parts 0 where no folded mixing runs (the exact-f32
    path, dense attention, up to 64 atoms)."""
    if not (path == SIMPLE_H3 and model == "kernel" and V > 64) or flags & _flag("PER_OP_UNFUSED"):
        return 0, 0, 0
    one_wg = bool(flags & _flag("FOLD_ONE_WG_PER_TILE"))
    wgs = fold_wgs(V, n_rows)
    parts = 1
    if wgs < 400 and not one_wg:
        parts = next((hp for hp in (6 if wgs < 128 else 2, 3, 2) if heads % hp == 0), 1)
    gemm_inside = not flags & _flag("FOLD_GEMM_SEPARATE") and (wgs >= 400 or parts > 1 or one_wg)
    ln_inside = not flags & _flag("FOLD_LN_SEPARATE") and parts == 1
    return parts, int(gemm_inside), int(ln_inside)


def fold_wgs(V, n_rows):
    return n_rows * -(-V // 128)


def tokens_nt4(n_tokens, flags=0):
    """h3_tokens_nt4: 64-token waves (256 tokens per workgroup, 4/3 the time per round) where they need fewer rounds' worth."""
    wg3, wg4 = -(-n_tokens // 192), -(-n_tokens // 256)
    if flags & _flag("TOKENS_NT4"):
        return True
    if flags & _flag("TOKENS_NT3"):
        return False
    return 4 * -(-wg4 // H3_CUS) < 3 * -(-wg3 // H3_CUS)


def ffn_form(n_tokens, path, flags=0):
    """h3_ffn_tokens: "tokens48x4" (four-way split of the hidden layer + a finishing launch), "tokens48x1", "tokens64x1"; "gemms" on the
    exact-f32 path.  (The scratch the split needs, 4 * n_tokens * 128 floats, fits the [n_tokens, 2048] FFN buffer of the full models.)"""
    if path != SIMPLE_H3 or flags & _flag("PER_OP_UNFUSED"):
        return "gemms"
    if tokens_nt4(n_tokens, flags):
        return "tokens64x1"
    split = -(-n_tokens // 192) * 2 <= H3_CUS and FFN_SPLIT * n_tokens * 128 <= n_tokens * D_FF and not flags & _flag("TOKENS_NT3")
    return f"tokens48x{FFN_SPLIT if split else 1}"


def io_form(n_tokens, path, flags=0):
    """h3_io_tokens: the in / out MLPs on the token list (no position features in either full model)."""
    if path != SIMPLE_H3 or flags & (_flag("PER_OP_UNFUSED") | _flag("IO_GEMM_PAIRS")):
        return "gemms"
    return "tokens64" if tokens_nt4(n_tokens, flags) else "tokens48"


def sdpa_plan(model, heads, V, n_rows, flags=0):
    """launch_sdpa: (q_tiles_per_wave, chunks) of sdpa_mfma_kernel; (0, 0) where it does not run."""
    V16 = -(-V // 16)
    if not (model == "dense" and D_MODEL // heads == 16 and V > 64 and V16 * (2 * 1024 + 64) <= 160 * 1024) or flags & _flag("SDPA_SCALAR"):
        return 0, 0
    per_wave = min(max(n_rows * heads * V16 // 4 // 1024, 1), -(-V16 // 4))
    return per_wave, -(-V16 // (4 * per_wave))


def route(case, path, flags=0):
    """The string tw_last_per_op_route returns behind a per-op pass of `case` on `path` under `flags`."""
    hp, gi, li = fold_plan(case.model, case.heads, case.V, case.n_rows, path, flags)
    q, chunks = sdpa_plan(case.model, case.heads, case.V, case.n_rows, flags)
    return (f"head_parts={hp} gemm_inside={gi} ln_inside={li} ffn={ffn_form(case.n_tokens, path, flags)} "
            f"io={io_form(case.n_tokens, path, flags)} q_tiles_per_wave={q} chunks={chunks}")


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    model: str                   # "kernel" (H.full_kernel_sd, 6 heads) | "dense" (H.full_dense_sd, 8 heads of 16)
    V: int
    n_rows: int
    form: str                    # "sample" (one conditioning state, n_rows latents) | "loglik" (n_rows conditioning states)
    about: str                   # "fold" | "tokens" | "sdpa": which decision's threshold the case sits at (its A/B flags, its edge rows)
    regime: str
    facts: Tuple[str, ...]       # python expressions over the restatement on TW_PATH_SIMPLE_H3 (see check_facts) that must hold

    @property
    def name(self):
        return f"{self.model}-v{self.V}-s{self.n_rows}-{self.form}"

    @property
    def heads(self):
        return 6 if self.model == "kernel" else 8

    @property
    def n_tokens(self):
        return self.n_rows * self.V

    @property
    def spec(self):
        return H.FULL_KERNEL_SPEC if self.model == "kernel" else H.FULL_DENSE_SPEC


def _fold(V, n_rows, form, regime, *facts):
    return Case("kernel", V, n_rows, form, "fold", regime, facts)


def _tokens(model, V, n_rows, form, regime, *facts):
    return Case(model, V, n_rows, form, "tokens", regime, facts)


def _sdpa(V, n_rows, form, regime, *facts):
    return Case("dense", V, n_rows, form, "sdpa", regime, facts)


# (`at(n)`: the same expressions' values at n rows - each case is the SMALLEST or LARGEST row count of its regime)
FOLD_CASES = (
    _fold(65, 127, "sample", "heads over 6 workgroups per query tile, the last launch size that does",
          "fold_wgs == 127", "head_parts == 6 and gemm_inside and not ln_inside", "at(n_rows + 1).head_parts == 2"),
    _fold(65, 128, "loglik", "heads over 2 workgroups per query tile, the first launch size",
          "fold_wgs == 128", "head_parts == 2 and gemm_inside and not ln_inside", "at(n_rows - 1).head_parts == 6"),
    _fold(65, 399, "sample", "heads over 2 workgroups per query tile, the last launch size",
          "fold_wgs == 399", "head_parts == 2", "at(n_rows + 1).head_parts == 1"),
    _fold(65, 400, "loglik", "one workgroup walks all heads of its tile: GEMM, residual and LayerNorm 1 in its epilogue",
          "fold_wgs == 400", "head_parts == 1 and gemm_inside and ln_inside", "at(n_rows - 1).head_parts == 2"),
    _fold(129, 199, "loglik", "the 2 / 1 boundary with two query tiles per row (the second one query wide), below",
          "-(-V // 128) == 2 and V % 128 == 1", "fold_wgs == 398", "head_parts == 2", "at(n_rows + 1).head_parts == 1"),
    _fold(129, 200, "sample", "the 2 / 1 boundary with two query tiles per row, above",
          "-(-V // 128) == 2", "fold_wgs == 400", "head_parts == 1 and gemm_inside and ln_inside", "at(n_rows - 1).head_parts == 2"),
    # (three query tiles need 257 atoms: 193 atoms are two tiles, 129 x 199 / 200 above already have those)
    _fold(257, 3, "loglik", "a three-tile row under 6 parts, the third tile one query wide (above every fused layout: the model's default is this path)",
          "V > 192 and -(-V // 128) == 3 and V % 128 == 1", "fold_wgs == 9", "head_parts == 6"),
)


def _token_cases(model, forms):
    return (
        _tokens(model, 65, 378, forms[0], "four-way split of the FFN's hidden layer, the largest launch that takes it",
                "n_tokens == 24570", "wg3 == 128 and wg3 * 2 <= 256", "ffn == 'tokens48x4' and io == 'tokens48'", "at(n_rows + 1).ffn == 'tokens48x1'"),
        _tokens(model, 65, 379, forms[1], "48-token waves unsplit, the smallest launch",
                "wg3 == 129", "ffn == 'tokens48x1' and io == 'tokens48'", "at(n_rows - 1).ffn == 'tokens48x4'", "n_tokens % 192 != 0"),
        _tokens(model, 65, 757, forms[0], "64-token waves by the rule (two rounds of 48-token workgroups against one), the smallest launch",
                "n_tokens == 49205 and 49153 <= n_tokens <= 65536", "wg3 == 257 and wg4 == 193", "ffn == 'tokens64x1' and io == 'tokens64'",
                "at(n_rows - 1).ffn == 'tokens48x1'", "n_tokens % 256 != 0"),
        _tokens(model, 65, 1009, forms[1], "48-token waves again, two rounds of the chip either way, the smallest launch",
                "n_tokens == 65585 and n_tokens > 65536", "wg3 == 342 and wg4 == 257", "ffn == 'tokens48x1' and io == 'tokens48'",
                "at(n_rows - 1).ffn == 'tokens64x1'", "n_tokens % 192 != 0"),
        _tokens(model, 193, 255, forms[0], "the 64-token window at 193 atoms (above every fused layout)",
                "n_tokens == 49215", "wg3 == 257 and wg4 == 193", "ffn == 'tokens64x1' and io == 'tokens64'", "at(n_rows - 1).ffn == 'tokens48x1'"),
    )


TOKEN_CASES = _token_cases("kernel", ("sample", "loglik")) + _token_cases("dense", ("loglik", "sample"))

SDPA_CASES = (
    _sdpa(129, 113, "sample", "one query tile per wave, three chunks, the largest launch",
          "V16 == 9", "n_rows * heads * V16 < 2 * 4096", "q_tiles == 1 and chunks == 3", "at(n_rows + 1).q_tiles == 2"),
    _sdpa(129, 114, "loglik", "two query tiles per wave, two chunks, the last one ragged (one tile of eight)",
          "n_rows * heads * V16 >= 2 * 4096", "q_tiles == 2 and chunks == 2", "V16 % (4 * q_tiles) == 1", "at(n_rows - 1).q_tiles == 1"),
    _sdpa(129, 171, "sample", "three query tiles per wave (the clip's upper end), one chunk: the third trip past the last tile for three waves",
          "n_rows * heads * V16 >= 3 * 4096", "q_tiles == 3 == -(-V16 // 4) and chunks == 1", "at(n_rows - 1).q_tiles == 2"),
    _sdpa(65, 205, "loglik", "two query tiles per wave, one chunk, at five key tiles",
          "V16 == 5", "q_tiles == 2 == -(-V16 // 4) and chunks == 1", "at(n_rows - 1).q_tiles == 1"),
)

NAMED_CASES = FOLD_CASES + TOKEN_CASES + SDPA_CASES


def _other_form(c):
    return Case(c.model, c.V, c.n_rows, "loglik" if c.form == "sample" else "sample", c.about, c.regime + " - the other call form", c.facts)


# An id costs well under a second on the GPU, so every launch size runs in BOTH call forms: the route is the same, but one shared
# conditioning row (scores, masks and centring indexed by row % 1) against one per row is a different index in every kernel of the pass
CASES = NAMED_CASES + tuple(_other_form(c) for c in NAMED_CASES)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


class _Facts:
    """What the restatement says about a case on TW_PATH_SIMPLE_H3, flags 0, as attributes."""

    def __init__(self, case, n_rows=None):
        n_rows = case.n_rows if n_rows is None else n_rows
        c = Case(case.model, case.V, n_rows, case.form, case.about, case.regime, ())
        self.V, self.n_rows, self.heads, self.n_tokens = c.V, n_rows, c.heads, c.n_tokens
        self.V16 = -(-c.V // 16)
        self.fold_wgs = fold_wgs(c.V, n_rows)
        self.head_parts, self.gemm_inside, self.ln_inside = fold_plan(c.model, c.heads, c.V, n_rows, SIMPLE_H3)
        self.wg3, self.wg4 = -(-c.n_tokens // 192), -(-c.n_tokens // 256)
        self.ffn, self.io = ffn_form(c.n_tokens, SIMPLE_H3), io_form(c.n_tokens, SIMPLE_H3)
        self.q_tiles, self.chunks = sdpa_plan(c.model, c.heads, c.V, n_rows)


def check_facts(case):
    """The facts of a case that do NOT hold under the restatement."""
    f = _Facts(case)
    env = dict(vars(f), at=lambda n: _Facts(case, n))
    return [e for e in case.facts if not eval(e, {"__builtins__": {}}, env)]


# ---------------------------------------------------------------------------------------------------------------------
# inputs, checked rows, the oracle's answers
# ---------------------------------------------------------------------------------------------------------------------
def state_dict(model, double=False):
    """The full models' name-seeded weights (shared: do not modify); `double`: the same values as float64."""
    return _state_dict(model, bool(double))


@functools.lru_cache(maxsize=None)
def _state_dict(model, double):
    sd = H.full_kernel_sd() if model == "kernel" else H.full_dense_sd()
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()} if double else sd


# A case whose first draw left the float32 ORACLE itself further than 2.5e-6 from the same oracle in float64 on its checked rows (the CPU
# file's bar) takes the next draw that does not - other inputs, never a wider bar.  case -> draw number; the error of the draws passed
# over in the comment.  The float32 oracle's rounding depends on the host's thread count (the order of its reductions): the figures are
# the worst of 4, 8 and 16 threads, and a draw counts as good at 2.05e-6 or better on all three, half a microunit under the bar.
RESEED = {
    "kernel-v193-s255-sample": 1,   # draw 0: 3.5e-6 (y_coords); draw 1: 2.0e-6
    "kernel-v65-s128-sample": 1,    # draw 0: 3.3e-6 (y_velocs)
    "kernel-v65-s400-sample": 1,    # draw 0: 2.7e-6 (y_velocs)
    "dense-v193-s255-sample": 1,    # draw 0: 2.7e-6 (y_velocs)
    "dense-v129-s113-sample": 2,    # draw 0: 2.3e-6, draw 1: 2.8e-6 (y_coords, 16 threads)
}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The inputs of a case (float32; shared: do not modify).  x_coords ~ N(0, (0.2 + 0.004 V)^2) as tests/model_shapes.py, velocities
    x 0.5.  "sample": one conditioning row with a masked tail of 1 + V % 7 atoms, latents [n_rows, 1, V, 3] at the prior's scales.
    "loglik": n_rows conditioning rows, y = x + 0.02 N, ragged masked tails of (5 row) % 11 atoms - rows 0, 11, 22, ... are full length."""
    V, S = case.V, case.n_rows
    draw = RESEED.get(case.name, 0)
    g = torch.Generator().manual_seed(zlib.crc32((case.name + (f"/{draw}" if draw else "")).encode()))
    B = 1 if case.form == "sample" else S
    d = dict(atom_types=torch.randint(0, 5, (B, V), generator=g),
             x_coords=torch.randn(B, V, 3, generator=g) * (0.2 + 0.004 * V),
             x_velocs=torch.randn(B, V, 3, generator=g) * 0.5)
    mask = torch.zeros(B, V, dtype=torch.bool)
    if case.form == "sample":
        mask[0, V - (1 + V % 7):] = True
        zc, zv = fo.draw_latents(state_dict(case.model), S, (1, V, 3), g)
        d.update(z_coords=zc, z_velocs=zv)
    else:
        for b in range(B):   # (rows 0, 11, 22, ...: full length - at 65 / 129 / 193 / 257 atoms the last query tile is ONE atom wide)
            mask[b, V - (5 * b) % 11:] = (5 * b) % 11 > 0
        d.update(y_coords=d["x_coords"] + torch.randn(B, V, 3, generator=g) * 0.02, y_velocs=torch.randn(B, V, 3, generator=g) * 0.5)
    d["masked"] = mask
    return d


def tile_edge_rows(case):
    """Token-list cases: the rows that hold the tokens on both sides of the first tile edge, of the last tile's start and of the
    chip-round edge (tile 256), for 192- and 256-token tiles."""
    rows = set()
    if case.about != "tokens":
        return rows
    for T in (192, 256):
        tiles = -(-case.n_tokens // T)
        for edge in (T, (tiles - 1) * T, H3_CUS * T):
            if 0 < edge < case.n_tokens:
                rows.update(((edge - 1) // case.V, edge // case.V))
    return rows


@functools.lru_cache(maxsize=None)
def checked_rows(case):
    """The fixed subset of rows held to the oracle (sorted, unique): first two, row 11, last two, the tile-edge rows, 8 seeded draws."""
    S = case.n_rows
    g = torch.Generator().manual_seed(zlib.crc32((case.name + "/rows").encode()))
    drawn = torch.randperm(S, generator=g)[:8].tolist()
    rows = {0, 1, 11, S - 2, S - 1} | tile_edge_rows(case) | set(drawn)   # (0 and 11: the first full-length rows of "loglik")
    return tuple(sorted(r for r in rows if 0 <= r < S))


def _cast(d, double):
    return {k: (v.double() if double and v.is_floating_point() else v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def oracle(case, double=False):
    """The oracle's answer on the checked rows alone (shared: do not modify): "sample" -> (y_coords, y_velocs, logp), "loglik" ->
    (loglik,), each with the checked rows along dim 0."""
    sd, d = state_dict(case.model, double), _cast(inputs(case), double)
    rows = torch.tensor(checked_rows(case))
    if case.form == "sample":
        return tuple(fo.conditional_sample_with_logp(sd, case.spec, d["atom_types"], d["x_coords"], d["x_velocs"], d["masked"],
                                                     d["z_coords"][rows], d["z_velocs"][rows]))
    return (fo.log_likelihood(sd, case.spec, d["atom_types"][rows], d["x_coords"][rows], d["x_velocs"][rows], d["y_coords"][rows],
                              d["y_velocs"][rows], d["masked"][rows]),)


OUTPUTS = {"sample": ("y_coords", "y_velocs", "logp"), "loglik": ("loglik",)}


def unmasked(case, name, t):
    """The part of an output the bar applies to: coordinates and velocities on the unmasked atoms of the (one) conditioning row."""
    return t[:, :, ~inputs(case)["masked"][0]] if name in ("y_coords", "y_velocs") else t


def errors(case, got, want):
    """{output: helpers.rel_err} of two tuples of outputs over the same rows."""
    return {n: H.rel_err(unmasked(case, n, a), unmasked(case, n, b)) for n, a, b in zip(OUTPUTS[case.form], got, want)}
