"""Every model shape the path predicates accept, on the MI355X, against the float32 oracle: the case table of
tests/model_shapes.py (head counts 1 - 18 on every layout of the fused kernels and on the folded per-op mixing; the per-op paths at
widths off 128; every local_attend_kernel instance; the corners of the equivariant flow's predicate), one test id per (shape, size).

For every case and every explicit path: `tw_flow_path_supported` == 1 -> the path runs and meets the bar (forward pass, reverse pass
on unmasked atoms, the reverse move's likelihood on the oracle's samples, and the stage trace of one net of the last coupling layer,
so that a miss names its kernel); == 0 -> the library refuses by name and launches nothing.  The model's own default lands on a
supported path and meets the bar.  Bars: 1e-5 (helpers.rel_err) on every parity path; the single-MFMA fast mode at its own 2e-3.
Each run prints `model_shapes | case | path | kernel the library reports | worst error | bar` (pytest -s; profiles/model_shapes.txt)."""
import ctypes as C

import pytest
import torch

from tests import helpers as H
from tests import model_shapes as ms
from timewarp_amd import _lib
from timewarp_amd._lib import DebugFlag

pytestmark = pytest.mark.gpu

TOL = 1e-5
H1_TOL = 2e-3   # TW_PATH_FUSED_H1 is no parity path: its own bar, as tests/test_flow_gpu.py::test_small_feedforward_... holds it
HALF_PATHS = (ms.FUSED_H3, ms.FUSED_H1, ms.SIMPLE_H3)
FOLD_SIZES = (70, 130, 200)   # TW_PATH_SIMPLE_H3 with the packed stream: the folded mixing and its finishing launch


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


def _flow_calls(m, d):
    """The three model calls of an MH iteration on a case's inputs (cuda tensors) -> CPU tensors named like the oracle's."""
    c = slice(ms.COND_ROW, ms.COND_ROW + 1)
    S = ms.N_SAMPLES
    out = {"loglik": m.log_likelihood(atom_types=d["atom_types"], x_coords=d["x_coords"], x_velocs=d["x_velocs"], y_coords=d["y_coords"],
                                      y_velocs=d["y_velocs"], adj_list=None, edge_batch_idx=None, masked_elements=d["masked"]).cpu()}
    yc, yv, lp = m.conditional_sample_with_logp(atom_types=d["atom_types"][c], x_coords=d["x_coords"][c], x_velocs=d["x_velocs"][c],
                                                adj_list=None, edge_batch_idx=None, masked_elements=d["masked"][c], num_samples=S,
                                                z_coords=d["z_coords"], z_velocs=d["z_velocs"])
    out.update(s_y_coords=yc.cpu(), s_y_velocs=yv.cpu(), s_logp=lp.cpu())
    return out


def _reverse_move(m, d, ref):
    """log-likelihood of the reverse move on the ORACLE's samples (isolates this call from the sampling error)."""
    c = slice(ms.COND_ROW, ms.COND_ROW + 1)
    S = ms.N_SAMPLES
    gy, gv = ref["s_y_coords"].squeeze(1).cuda(), ref["s_y_velocs"].squeeze(1).cuda()
    return m.log_likelihood(atom_types=d["atom_types"][c].repeat(S, 1), x_coords=gy, x_velocs=-gv, y_coords=d["x_coords"][c].repeat(S, 1, 1),
                            y_velocs=-d["x_velocs"][c].repeat(S, 1, 1), adj_list=None, edge_batch_idx=None,
                            masked_elements=d["masked"][c].repeat(S, 1)).cpu()


def _errors(case, out, ref):
    keep = ~ms.inputs(*case)["masked"][ms.COND_ROW]
    pick = lambda k, t: t[:, :, keep] if k in ("s_y_coords", "s_y_velocs") else t
    return {k: H.rel_err(pick(k, out[k]), pick(k, ref[k])) for k in out}


def _trace_errors(m, case, path):
    """model.debug_netblock of one net of the last coupling layer against the oracle's stages, unmasked atoms: {stage: error}."""
    shape, V = case
    at, xc, xv, mk, z_other = ms.trace_inputs(shape, V)
    acts, out = m.debug_netblock(ms.TRACE_COUPLING, ms.TRACE_NET, at.cuda(), xc.cuda(), xv.cuda(), mk.cuda(), z_other.cuda(), path)
    keep = ~mk[0]
    stages = ms.oracle_trace(shape, V)
    got = [acts[i].cpu() for i in range(len(stages) - 1)] + [out.cpu()]
    assert len(got) == len(stages)
    return {name: H.rel_err(g[:, keep], want[:, keep]) for g, (name, want) in zip(got, stages)}


def _range_word_clear(m):
    """The equivariant flow runs no half-precision kernel: its range-guard word is never raised (tests/test_equivariant_gpu.py)."""
    assert not m.used_split_fp16 and not m.demoted
    for flag in m._range_flags.values():
        assert int(flag.item()) == 0


def _runs(shape, V, path):
    """[(debug flags, expected layout or None, must differ bit-wise from the first run: True / False / None = not asserted)]."""
    a_shape = shape.family == "kernel" and shape.d_model == 128
    if a_shape and path in (ms.FUSED_H3, ms.FUSED_H1):
        return [(f, layout, i > 0) for i, (f, layout) in enumerate(ms.layout_runs(shape, V))]
    runs = [(0, None, False)]
    if a_shape and path == ms.SIMPLE_H3 and V in FOLD_SIZES:
        # below 128 fold workgroups the heads go over head_parts workgroups per query tile (+ a finishing launch); without a divisor the
        # default IS the per-head launches + separate GEMM, so FOLD_GEMM_SEPARATE changes nothing there; chebyshev_kernel: no folded
        # operands at all (every layer has its own scores), the flags are inert
        parts = ms.head_parts(shape.heads)
        runs.append((int(DebugFlag.FOLD_ONE_WG_PER_TILE), None, not shape.cheb))
        runs.append((int(DebugFlag.FOLD_GEMM_SEPARATE), None, parts > 1 and not shape.cheb))
    if shape in ms.B_SHAPES and (shape.family != "dense" or shape.dh <= 64):   # (dense heads wider than 64: no row-wise kernel, see below)
        if V == 22:
            runs.append((int(DebugFlag.PER_OP_ROWWISE), None, None))
        if shape.family == "dense" and V in (70, 130):
            # head width 16: the default is the matrix-pipe kernel, the flag takes the scalar ones; any other width runs the scalar
            # kernels anyway, and the flag must change nothing
            runs.append((int(DebugFlag.SDPA_SCALAR), None, shape.dh == 16))
    return runs


def _refused(shape, V, path, m_simple, d):
    """tw_flow_path_supported said 0: the explicit path returns the library's error status with a message that names the config,
    and launches nothing - outputs prefilled with NaN stay NaN, the device reports no error."""
    lib = _lib.load()
    dev = d["x_coords"].device
    desc = m_simple._desc(dev)
    raw, _ = m_simple._weights(dev, ms.SIMPLE)
    packed = None
    if shape.family != "equivariant":
        try:   # the path's own pack where one exists for other sizes of this model (e.g. TW_PATH_FUSED above 64 atoms)
            _, packed = m_simple._weights(dev, path)
        except RuntimeError:
            packed = None
    at, mk = d["atom_types"].to(torch.int32).contiguous(), d["masked"].to(torch.uint8).contiguous()
    B = at.shape[0]
    ws = m_simple._ws(dev, B, V)
    out = torch.full((B,), float("nan"), device=dev)
    rc = lib.tw_flow_log_likelihood(C.byref(desc), raw.data_ptr(), _lib.ptr(packed), at.data_ptr(), d["x_coords"].data_ptr(),
                                    d["x_velocs"].data_ptr(), d["y_coords"].data_ptr(), d["y_velocs"].data_ptr(), mk.data_ptr(),
                                    out.data_ptr(), B, V, path, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
    msg = lib.tw_last_error().decode()
    assert rc == -1, (rc, msg)   # TW_ERR_INVALID
    if shape.family == "equivariant":
        assert "equivariant flow" in msg and f"path {path}" in msg, msg
    else:
        assert "unsupported for this config" in msg and f"d_model={shape.d_model}" in msg and f"n_atoms={V}" in msg, msg
    S = ms.N_SAMPLES
    c = slice(ms.COND_ROW, ms.COND_ROW + 1)
    ys = [torch.full((S, 1, V, 3), float("nan"), device=dev), torch.full((S, 1, V, 3), float("nan"), device=dev),
          torch.full((S, 1), float("nan"), device=dev)]
    at1, mk1, xc1, xv1 = at[c].contiguous(), mk[c].contiguous(), d["x_coords"][c].contiguous(), d["x_velocs"][c].contiguous()
    rc = lib.tw_flow_sample_with_logp(C.byref(desc), raw.data_ptr(), _lib.ptr(packed), at1.data_ptr(), xc1.data_ptr(), xv1.data_ptr(),
                                      mk1.data_ptr(), d["z_coords"].data_ptr(), d["z_velocs"].data_ptr(), ys[0].data_ptr(), ys[1].data_ptr(),
                                      ys[2].data_ptr(), S, 1, V, path, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
    assert rc == -1, (rc, lib.tw_last_error().decode())
    torch.cuda.synchronize()   # raises if anything was launched and failed
    assert bool(out.isnan().all()) and all(bool(y.isnan().all()) for y in ys)


def _report(case, label, kernel, errs, bar):
    worst = max(errs, key=errs.get)
    # (a line of its own: under `pytest -q -s` the progress dot of the previous test id has no newline behind it)
    print(f"\nmodel_shapes | {ms.case_id(case)} | {label} | {kernel or '-'} | {errs[worst]:.2e} ({worst}) | {bar:.0e}")


@pytest.mark.parametrize("case", [pytest.param(c, id=ms.case_id(c)) for c in ms.CASES])
def test_case(case):
    shape, V = case
    lib = _lib.load()
    ref, d = ms.oracle(shape, V), _cuda(ms.inputs(shape, V))
    desc0 = shape.model().dims.to_desc()
    supported = {p: lib.tw_flow_path_supported(C.byref(desc0), V, p) for p in ms.EXPLICIT_PATHS}
    assert supported[ms.SIMPLE] == 1   # (every shape of the table has a path)
    ran = []
    for path in ms.EXPLICIT_PATHS:
        if supported[path] != 1:
            continue
        bar = H1_TOL if path == ms.FUSED_H1 else TOL
        first = None
        for i, (flags, layout, differs) in enumerate(_runs(shape, V, path)):
            label = ms.PATH_NAMES[path] + "".join(" " + f.name for f in DebugFlag if int(f) & flags)
            with H.debug_flags(flags):
                m = shape.model(path).cuda()
                if path == ms.SIMPLE_H3 and shape.family != "equivariant":
                    assert (lib.tw_flow_packed_simple_h3_bytes(C.byref(desc0)) > 0) == (shape.family == "kernel" and shape.d_model == 128)
                out = _flow_calls(m, d)
                per_op = path in (ms.SIMPLE, ms.SIMPLE_H3)
                kernel = (lib.tw_last_attention_kernel() if per_op else lib.tw_last_netblock_kernel()).decode()
                if per_op:   # the attention kernel the shape is in the table for is the one that ran (the equivariant flow has none)
                    want = ms.attention_kernel(shape, V, path, flags)
                    assert want is None or kernel == want, (label, kernel, want)
                    kernel = kernel if want else ""
                out["logp_yx"] = _reverse_move(m, d, ref)
                errs = _errors(case, out, ref)
                if i == 0 and path != ms.FUSED_H1:   # (the single-MFMA build has no activation dumps)
                    errs.update({"stage " + k: e for k, e in _trace_errors(m, case, path).items()})
            _report(case, label, kernel, errs, bar)
            if layout is not None:
                assert ms.layout_of(kernel) == layout, (label, kernel, layout)
            assert max(errs.values()) < bar, (label, kernel, errs)
            if path in HALF_PATHS:
                H.assert_not_demoted(m)
            if shape.family == "equivariant":
                _range_word_clear(m)
            flat = torch.cat([out[k].flatten() for k in ("loglik", "s_y_coords", "s_y_velocs", "s_logp")])
            if i == 0:
                first = flat
            elif differs is True:
                assert not torch.equal(flat, first), f"{label}: bit-identical to the run it is an alternative to - the same route ran twice"
            elif differs is False:
                assert torch.equal(flat, first), f"{label}: expected the default route (bit-identical results)"
        ran.append(path)
    assert ms.SIMPLE in ran
    # the model's own default: a supported path, at the bar
    m = shape.model().cuda()
    chosen = m._path_for(V)
    assert chosen in (ms.AUTO,) + ms.EXPLICIT_PATHS and (chosen == ms.AUTO or supported[chosen] == 1), chosen
    out = _flow_calls(m, d)
    out["logp_yx"] = _reverse_move(m, d, ref)
    errs = _errors(case, out, ref)
    _report(case, f"default -> {ms.PATH_NAMES.get(chosen, 'AUTO')}", "", errs, TOL)
    assert max(errs.values()) < TOL, ("default", chosen, errs)
    H.assert_not_demoted(m)
    # ... and what the predicate refuses is refused by the library, by name, before anything is launched
    m_simple = shape.model(ms.SIMPLE).cuda()
    for path in ms.EXPLICIT_PATHS:
        if supported[path] != 1:
            _refused(shape, V, path, m_simple, d)


def test_head_width_80_beyond_the_score_tile_is_refused_by_name():
    """One head of width 80: sdpa_kernel's score tile fits the LDS up to 70 atoms (the table's sizes); at 130 atoms, and wherever
    PER_OP_ROWWISE forces the row-wise kernel, the library refuses - the row-wise kernel serves heads up to 64 wide
    (tests/test_flow_gpu.py::test_per_op_error_between_fork_and_join_leaves_streams_usable pins the contract on the C ABI)."""
    shape = ms.BY_NAME["d80-e16-h1-r0"]
    for path in (ms.SIMPLE, ms.SIMPLE_H3):
        m = shape.model(path).cuda()
        g = torch.Generator().manual_seed(80)
        V = 130
        args = dict(atom_types=torch.randint(0, 5, (2, V), generator=g).cuda(), x_coords=torch.randn(2, V, 3, generator=g).cuda(),
                    x_velocs=torch.randn(2, V, 3, generator=g).cuda(), y_coords=torch.randn(2, V, 3, generator=g).cuda(),
                    y_velocs=torch.randn(2, V, 3, generator=g).cuda(), adj_list=None, edge_batch_idx=None,
                    masked_elements=torch.zeros(2, V, dtype=torch.bool).cuda())
        with pytest.raises(RuntimeError, match="head width 80 > 64 on the row-wise per-op kernel"):
            m.log_likelihood(**args)
        d = _cuda(ms.inputs(shape, 22))
        with H.debug_flags(DebugFlag.PER_OP_ROWWISE):
            with pytest.raises(RuntimeError, match="head width 80 > 64 on the row-wise per-op kernel"):
                _flow_calls(m, d)
        errs = _errors((shape, 22), _flow_calls(m, d), ms.oracle(shape, 22))   # the model still runs, at the bar
        assert max(errs.values()) < TOL, errs
    torch.cuda.synchronize()
