"""The case table of tests/launch_sizes.py without a GPU: the restatement of the three launch-size decisions and the references
alone.
- every case's facts hold under the restatement (they fail here when a threshold moves);
- both sides of every threshold in the restatement have a case;
- the float32 oracle stays within a QUARTER of the parity bar of the same oracle in float64 on each case's checked rows (a reference
  that is itself 5e-6 off leaves a kernel no room under 1e-5)."""
import ctypes as C
import re

import pytest
import torch

from tests import helpers as H
from tests import launch_sizes as ls
from timewarp_amd import _lib
from timewarp_amd._lib import DebugFlag

REF_TOL = 2.5e-6     # float32 oracle against float64 oracle: a quarter of the project's 1e-5 bar

CASE_PARAMS = [pytest.param(c, id=c.name) for c in ls.CASES]


@pytest.mark.parametrize("case", CASE_PARAMS)
def test_case_facts_hold_under_the_restatement(case):
    assert case.regime and case.facts
    assert ls.check_facts(case) == [], (case.regime, ls.check_facts(case))


def test_restatement_reads_the_thresholds_the_library_states():
    """The constants the restatement repeats, read from the sources: a moved threshold fails here before any GPU run."""
    import os

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "timewarp_amd", "csrc")
    with open(os.path.join(csrc, "tw_kernels.hip")) as f:
        kernels = f.read()
    with open(os.path.join(csrc, "tw_netblock_h3.hip")) as f:
        h3 = f.read()
    assert "p.fold_wgs = n_rows * ((V + 127) / 128);" in kernels
    assert "if (p.fold_wgs < 400 && !one_wg)" in kernels and "for (int hp : {p.fold_wgs < 128 ? 6 : 2, 3, 2})" in kernels
    assert "p.gemm_inside = !(flags & TW_DEBUG_FOLD_GEMM_SEPARATE) && (p.fold_wgs >= 400 || p.head_parts > 1 || one_wg);" in kernels
    assert "int64_t per_wave = n_rows * H * (int64_t)V16 / 4 / 1024;" in kernels
    assert "per_wave = per_wave < 1 ? 1 : per_wave > (V16 + 3) / 4 ? (V16 + 3) / 4 : per_wave;" in kernels
    assert re.search(r"#define H3_FFN_SPLIT 4\b", h3) and ls.FFN_SPLIT == 4
    assert re.search(r"#define H3_CUS 256\b", h3) or re.search(r"constexpr int H3_CUS = 256;", h3)
    assert "return 4 * ((wg4 + H3_CUS - 1) / H3_CUS) < 3 * ((wg3 + H3_CUS - 1) / H3_CUS);" in h3
    assert "wg3 * 2 <= H3_CUS" in h3


def test_both_models_have_the_packed_stream_of_the_token_list_launches():
    """TW_PATH_SIMPLE_H3 runs the token-list launches only with the tw_flow_pack_simple_h3 buffer at hand: both full models have one."""
    lib = _lib.load()
    for make, sd in ((H.tw_kernel_model, H.full_kernel_sd()), (H.tw_dense_model, H.full_dense_sd())):
        desc = make(sd, device="cpu").dims.to_desc()
        assert lib.tw_flow_packed_simple_h3_bytes(C.byref(desc)) > 0
        for V in (65, 129, 193):
            assert lib.tw_flow_path_supported(C.byref(desc), V, ls.SIMPLE) == 1 and lib.tw_flow_path_supported(C.byref(desc), V, ls.SIMPLE_H3) == 1


def test_both_sides_of_every_threshold_have_a_case():
    f = {c.name: ls._Facts(c) for c in ls.CASES}
    fold = [f[c.name] for c in ls.FOLD_CASES]
    # the fold: 127 | 128 and 399 | 400 workgroups, the latter with one and with two query tiles per row; a three-tile row
    assert {(x.fold_wgs, x.head_parts) for x in fold} >= {(127, 6), (128, 2), (399, 2), (400, 1), (398, 2), (9, 6)}
    assert {-(-c.V // 128) for c in ls.FOLD_CASES} == {1, 2, 3}
    assert {c.form for c in ls.FOLD_CASES if f[c.name].head_parts == 1} == {"sample", "loglik"}
    # the token-list launches, both models: the split's last / the unsplit launch's first workgroup count, the 64-token window's
    # first launch and the first one behind it - each with the neighbouring row count on the other side of the threshold
    for model in ("kernel", "dense"):
        tok = [c for c in ls.TOKEN_CASES if c.model == model]
        assert {(f[c.name].wg3, f[c.name].ffn) for c in tok} >= {(128, "tokens48x4"), (129, "tokens48x1"), (257, "tokens64x1"), (342, "tokens48x1")}
        assert {c.form for c in tok} == {"sample", "loglik"} and {c.V for c in tok} == {65, 193}
        for c in tok:
            other = ls._Facts(c, c.n_rows - 1 if c.n_rows != 378 else c.n_rows + 1)
            assert other.ffn != f[c.name].ffn, c.name
    # sdpa_mfma_kernel: q_tiles_per_wave 1 | 2 | 3, one to three chunks, a ragged last chunk
    sd = [f[c.name] for c in ls.SDPA_CASES]
    assert {(x.q_tiles, x.chunks) for x in sd} == {(1, 3), (2, 2), (3, 1), (2, 1)}
    assert any(x.V16 % (4 * x.q_tiles) for x in sd if x.chunks > 1 and x.q_tiles > 1)
    # ... and every case of the dense model runs that kernel, the kernel model's never
    assert all((f[c.name].q_tiles > 0) == (c.model == "dense") for c in ls.CASES)


def test_table_names_every_route_in_the_hooks_spelling():
    """What the GPU file compares with tw_last_per_op_route, case by case: the table as a whole reaches head_parts 6, 2 and 1, the split,
    unsplit 48-token and 64-token launches and q_tiles_per_wave 1, 2 and 3.  Without a per-op pass on this thread the hook returns ""."""
    routes = " | ".join(ls.route(c, ls.SIMPLE_H3) for c in ls.CASES)
    for piece in ("head_parts=6", "head_parts=2", "head_parts=1", "ffn=tokens48x4", "ffn=tokens48x1", "ffn=tokens64x1", "io=tokens48", "io=tokens64",
                  "q_tiles_per_wave=1", "q_tiles_per_wave=2", "q_tiles_per_wave=3"):
        assert piece in routes, piece
    assert ls.route(ls.BY_NAME["kernel-v65-s400-loglik"], ls.SIMPLE_H3) == \
        "head_parts=1 gemm_inside=1 ln_inside=1 ffn=tokens48x1 io=tokens48 q_tiles_per_wave=0 chunks=0"
    assert ls.route(ls.BY_NAME["dense-v129-s114-loglik"], ls.SIMPLE) == \
        "head_parts=0 gemm_inside=0 ln_inside=0 ffn=gemms io=gemms q_tiles_per_wave=2 chunks=2"
    assert isinstance(_lib.load().tw_last_per_op_route(), bytes)


def test_debug_flags_force_what_the_restatement_says():
    """The A/B runs of the GPU file: which flag names the route a launch takes by itself, which the other one."""
    c400, c399 = ls.BY_NAME["kernel-v65-s400-loglik"], ls.BY_NAME["kernel-v65-s399-sample"]
    one, sep = int(DebugFlag.FOLD_ONE_WG_PER_TILE), int(DebugFlag.FOLD_GEMM_SEPARATE)
    assert ls.route(c400, ls.SIMPLE_H3, one) == ls.route(c400, ls.SIMPLE_H3) != ls.route(c400, ls.SIMPLE_H3, sep)
    assert ls.route(c399, ls.SIMPLE_H3, one) != ls.route(c399, ls.SIMPLE_H3)
    assert ls.fold_plan("kernel", 6, 65, 399, ls.SIMPLE_H3, one) == (1, 1, 1) and ls.fold_plan("kernel", 6, 65, 400, ls.SIMPLE_H3, sep) == (1, 0, 1)
    nt3, nt4 = int(DebugFlag.TOKENS_NT3), int(DebugFlag.TOKENS_NT4)
    for model in ("kernel", "dense"):
        inside, below = ls.BY_NAME[f"{model}-v65-s757-" + ("sample" if model == "kernel" else "loglik")], \
            ls.BY_NAME[f"{model}-v65-s379-" + ("loglik" if model == "kernel" else "sample")]
        assert ls.route(inside, ls.SIMPLE_H3, nt4) == ls.route(inside, ls.SIMPLE_H3) != ls.route(inside, ls.SIMPLE_H3, nt3)
        assert ls.route(below, ls.SIMPLE_H3, nt3) == ls.route(below, ls.SIMPLE_H3) != ls.route(below, ls.SIMPLE_H3, nt4)
    # the exact-f32 path takes none of the three token-list / fold routes, whatever the size
    assert all(ls.route(c, ls.SIMPLE).startswith("head_parts=0 gemm_inside=0 ln_inside=0 ffn=gemms io=gemms") for c in ls.CASES)


@pytest.mark.parametrize("case", CASE_PARAMS)
def test_checked_rows_are_the_fixed_set(case):
    rows = ls.checked_rows(case)
    S = case.n_rows
    assert set(rows) >= ({0, 1, 11, S - 2, S - 1} & set(range(S))) | ls.tile_edge_rows(case) and rows == tuple(sorted(set(rows))) and rows == ls.checked_rows(case)
    assert min(S, 8) <= len(rows) <= 5 + 12 + 8 and all(0 <= r < S for r in rows)
    if case.about == "tokens":   # a row on each side of the default route's first edge and of its last tile's start
        T = 256 if ls.tokens_nt4(case.n_tokens) else 192
        last = (-(-case.n_tokens // T) - 1) * T
        assert {(T - 1) // case.V, T // case.V, (last - 1) // case.V, last // case.V} <= set(rows)
    mask = ls.inputs(case)["masked"]
    assert bool(mask.any()) and not bool(mask[:, 0].any())   # every case masks tails
    if case.form == "sample":
        assert mask.shape[0] == 1 and bool(mask[0, -1])
    else:   # ragged, and the full-length rows - the only ones that show the one-atom last tile of 65 / 129 / 193 / 257 atoms - are checked
        full = [b for b in range(S) if not bool(mask[b].any())]
        assert full == list(range(0, S, 11)) and {0, 11} & set(range(S)) <= set(rows)
        assert len({int(m.sum()) for m in mask}) == min(S, 11)


@pytest.mark.parametrize("case", CASE_PARAMS)
def test_float32_oracle_within_a_quarter_of_the_bar_of_float64(case):
    f32, f64 = ls.oracle(case), ls.oracle(case, double=True)
    assert all(v.dtype == torch.float64 for v in f64) and all(v.dtype == torch.float32 for v in f32)
    assert all(v.shape[0] == len(ls.checked_rows(case)) for v in f32)
    errs = ls.errors(case, f32, f64)
    print(f"\nlaunch_sizes oracle | {case.name} | {len(ls.checked_rows(case))} rows | f32 vs f64 {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert max(errs.values()) <= REF_TOL, errs
    # log-densities are held per row on the GPU: none of them may sit near 0, where a relative error says nothing
    logp = f64[-1]
    assert float(logp.abs().min()) > 1.0, float(logp.abs().min())
