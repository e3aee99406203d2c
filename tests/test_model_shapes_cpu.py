"""The case table of tests/model_shapes.py without a GPU: the references alone.  For every (shape, size) case
- the float32 oracle stays within a QUARTER of the parity bar of the same oracle in float64 (a reference that is itself 5e-6 off
  leaves a kernel no room under 1e-5);
- every attention head is visible in the sampled outputs (zeroing its slice of one output projection moves them by 100 x the bar),
  so a kernel that dropped, repeated or mis-strided a head could not pass the GPU file;
- the shape reaches what its `reaches` text claims: the arithmetic facts, and - where the library can be asked without a GPU - the
  predicates and the launch code's own layout choice."""
import ctypes as C

import pytest
import torch

from tests import helpers as H
from tests import model_shapes as ms
from timewarp_amd import _lib
from timewarp_amd._lib import DebugFlag

REF_TOL = 2.5e-6     # float32 oracle against float64 oracle: a quarter of the project's 1e-5 bar
HEAD_MOVES = 1e-3    # what zeroing one head must change: 100 x the bar

CASE_PARAMS = [pytest.param(c, id=ms.case_id(c)) for c in ms.CASES]


def _unmasked(case, key, t):
    keep = ~ms.inputs(*case)["masked"][ms.COND_ROW]
    return t[:, :, keep] if key in ("s_y_coords", "s_y_velocs") else t


@pytest.mark.parametrize("case", CASE_PARAMS)
def test_float32_oracle_within_a_quarter_of_the_bar_of_float64(case):
    f32, f64 = ms.oracle(*case), ms.oracle(*case, double=True)
    assert all(v.dtype == torch.float64 for v in f64.values()) and all(v.dtype == torch.float32 for v in f32.values())
    errs = {k: H.rel_err(_unmasked(case, k, f32[k]), _unmasked(case, k, f64[k])) for k in f32}
    assert max(errs.values()) <= REF_TOL, errs
    # the stage trace the GPU file compares per stage: the same reference, held to the parity bar's quarter where it is well
    # conditioned and to the bar itself everywhere (a LayerNorm output's largest element carries the row's rounding)
    t32, t64 = ms.oracle_trace(*case), ms.oracle_trace(*case, double=True)
    assert [n for n, _ in t32] == [n for n, _ in t64]
    terrs = {n: H.rel_err(a, b) for (n, a), (_, b) in zip(t32, t64)}
    assert max(terrs.values()) < 1e-5, terrs


@pytest.mark.parametrize("case", [c for c in CASE_PARAMS if c.values[0][0].heads])
def test_every_head_moves_the_samples(case):
    shape, V = case
    d, base = ms.inputs(shape, V), ms.oracle(shape, V)
    slices = ms.head_slices(shape)
    assert len(slices) == shape.heads
    moved = []
    for key, cols in slices:
        sd = dict(ms.state_dict(shape))
        w = sd[key].clone()
        assert w.shape[1] == shape.heads * (cols.stop - cols.start)
        w[:, cols] = 0.0
        sd[key] = w
        yc, yv, _ = ms.oracle_sample(shape, sd, d)
        moved.append(max(H.rel_err(_unmasked(case, "s_y_coords", yc), _unmasked(case, "s_y_coords", base["s_y_coords"])),
                         H.rel_err(_unmasked(case, "s_y_velocs", yv), _unmasked(case, "s_y_velocs", base["s_y_velocs"]))))
    assert min(moved) > HEAD_MOVES, moved


@pytest.mark.parametrize("shape", [pytest.param(s, id=s.name) for s in ms.SHAPES])
def test_shape_reaches_what_it_claims(shape):
    assert shape.reaches and shape.facts and shape.sizes
    assert ms.check_facts(shape) == [], (shape.reaches, ms.check_facts(shape))
    lib = _lib.load()
    desc = shape.model().dims.to_desc()
    sup = {V: [lib.tw_flow_path_supported(C.byref(desc), V, p) for p in range(6)] for V in shape.sizes}
    if shape.family == "equivariant":
        assert all(s == [1, 0, 1, 0, 0, 0] for s in sup.values()), sup
    elif shape.d_model != 128 or shape.family == "local":
        # the per-op paths only, and no packed stream: every linear layer is its own (split) GEMM
        assert all(s == [1, 0, 1, 0, 0, 1] for s in sup.values()), sup
        assert lib.tw_flow_packed_simple_h3_bytes(C.byref(desc)) == 0
    elif shape.family == "dense":   # d_model 128 but two heads: the fused dense layouts need eight heads of 16
        assert all(s[ms.FUSED_H3] == 0 and s[ms.FUSED_H1] == 0 and s[ms.SIMPLE] == 1 and s[ms.SIMPLE_H3] == 1 for s in sup.values()), sup
        assert lib.tw_flow_packed_simple_h3_bytes(C.byref(desc)) == 0
    else:
        for V, s in sup.items():
            assert s == [1, int(V <= 64), 1, int(V <= 192), int(V <= 192), 1], (V, s)
        assert lib.tw_flow_packed_simple_h3_bytes(C.byref(desc)) > 0   # the packed stream, the folded projections, the split FFN stages


@pytest.mark.parametrize("case", [c for c in CASE_PARAMS if c.values[0][0].family == "local"])
def test_local_cases_have_the_neighbourhoods_they_claim(case):
    """One query alone with itself (a softmax over a single key), and around it: radius 0.2 nm a few neighbours (all four unmasked
    atoms at 5 atoms, where both radii therefore see the same lists), radius 1.0 nm every other atom up to 22 atoms and most at 70."""
    shape, V = case
    counts = ms.neighbour_counts(shape, V)
    others = len(counts) - 1   # unmasked atoms besides the isolated one
    assert int(counts[ms.ISOLATED_ATOM]) == 1 and int(counts.min()) == 1 and int((counts == 1).sum()) == 1, counts
    rest = counts[1:]
    if V == 5:
        assert bool((rest == others).all()) and others == 3, counts
    elif shape.max_radius < 0.5:
        assert 2 <= int(rest.min()) and int(rest.max()) <= 8 < others, counts   # (measured 2 .. 5 at 22 atoms, 2 .. 8 at 70)
    elif V <= 22:
        assert bool((rest == others).all()), counts
    else:
        assert others // 2 < int(rest.min()) < others and int(rest.max()) <= others, counts   # (measured 40 .. 62 of 62)


def _selected(desc, V, rows, flags, path=ms.FUSED_H3):
    lib = _lib.load()
    with H.debug_flags(flags):
        return lib.tw_flow_selected_kernel(C.byref(desc), V, rows, path).decode()


@pytest.mark.parametrize("shape", [pytest.param(s, id=s.name) for s in ms.A_SHAPES + ms.E_SHAPES])
def test_layout_table_names_what_the_launch_code_selects(shape):
    """LAYOUT_RUNS says which layout each (size, flags) run of the GPU file is there for; the launch code's own branch, run dry
    (tw_flow_selected_kernel), must name it - on the split-fp16 and on the single-MFMA path."""
    desc = shape.model().dims.to_desc()
    # (the narrow layout's instantiation is one for 1, 2 and 3 molecules per 48-token wave - the count is geometry, not a template
    # argument: what puts 16 and 22 atoms in the table is 48 // V)
    assert [48 // V for V in (16, 22, 30, 48)] == [3, 2, 1, 1]
    for V in shape.sizes:
        rows = ms.inputs(shape, V)["x_coords"].shape[0]
        for flags, layout in ms.layout_runs(shape, V):
            for n_rows in (rows, ms.N_SAMPLES):
                for path in (ms.FUSED_H3, ms.FUSED_H1):
                    name = _selected(desc, V, n_rows, flags, path)
                    assert ms.layout_of(name) == layout, (V, flags, n_rows, path, name)


def test_layout_table_covers_every_layout_and_both_sides_of_the_lds_limit():
    seen = {layout for s in ms.A_SHAPES for V in s.sizes for _, layout in ms.layout_runs(s, V)}
    assert seen == {"narrow", "wide", "nt4", "paired", "wide6"}, seen
    by = ms.BY_NAME
    pairs = ((64, by["k128-h9"], by["k128-h10"], "nt4"), (60, by["k128-h11"], by["k128-h12"], "nt4"), (48, by["k128-h17"], by["k128-h18"], "narrow"))
    for V, below, above, layout in pairs:
        assert V in below.sizes and V in above.sizes
        assert layout in [l for _, l in ms.layout_runs(below, V)] and layout not in [l for _, l in ms.layout_runs(above, V)], (V, layout)
        assert ms.sf_lds_bytes(below.heads, V, 1) <= 160 * 1024 < ms.sf_lds_bytes(above.heads, V, 1)


def test_mixed_hidden_widths_are_refused_by_name():
    """(32; 8, 256): the equivariant kernels take hidden layers of ONE width (tw_flow_desc.d_hidden, n_hidden); the constructor says
    so before a descriptor exists."""
    import timewarp_amd as tw

    emb, hidden = ms.D_REFUSED
    cfg = tw.ModelConfig("equivariant_nvp", equivariant_nvp_config=tw.EquivariantNVPConfig(
        atom_embedding_dim=emb, num_coupling_layers=ms.N_COUPLING, latent_mlp_hidden_dims=list(hidden), position_layer_index_mod_2=0))
    with pytest.raises(NotImplementedError, match=r"one width.*latent_mlp_hidden_dims=\[8, 256\]"):
        tw.model_constructor(cfg)


def test_fold_head_parts_restatement():
    assert [ms.head_parts(h) for h in (1, 2, 4, 5, 7, 9, 12)] == [1, 2, 2, 1, 1, 3, 6]
    assert DebugFlag.FOLD_ONE_WG_PER_TILE and DebugFlag.FOLD_GEMM_SEPARATE
