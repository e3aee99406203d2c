"""The per-op paths at every launch size where their route changes, on the MI355X, against the float32 oracle: the case table of
tests/launch_sizes.py, one test id per case.

For each of TW_PATH_SIMPLE, TW_PATH_SIMPLE_H3 and the model's own default path:
- the route the library reports (tw_last_per_op_route) equals the table's restatement of per_op_plan / launch_sdpa / h3_ffn_tokens /
  h3_io_tokens - a case that no longer sits where its facts say fails here, not silently;
- the checked rows (launch_sizes.checked_rows) meet the project's 1e-5 (helpers.rel_err) against the oracle: reverse pass outputs on the
  unmasked atoms and log p, or the log-likelihood;
- EVERY row of the launch: everything on an unmasked atom is finite, and TW_PATH_SIMPLE_H3 agrees with TW_PATH_SIMPLE at 1e-5 over the
  whole launch (helpers.rel_err) and, so that one damaged row is not diluted by the maximum of the tensor, row by row: each row's
  log-density at 1e-5 of itself, each row's coordinates and velocities over that row's own scale at ROW_TOL.
A/B flags on TW_PATH_SIMPLE_H3: where the restatement says a debug flag forces the route the launch takes by itself
(FOLD_ONE_WG_PER_TILE from 400 fold workgroups on, TOKENS_NT4 in the 64-token window) the flagged run equals the default bit for bit;
a flag that changes the route must change the bits, report the route the restatement names, and meet the bar too.
Each run prints `launch_sizes | case | path | route | worst error | bar` (pytest -s; profiles/launch_sizes.txt)."""
import pytest
import torch

from tests import helpers as H
from tests import launch_sizes as ls
from timewarp_amd import _lib
from timewarp_amd._lib import DebugFlag

pytestmark = pytest.mark.gpu

TOL = 1e-5
# Coordinates and velocities of ONE row over that row's own scale, one per-op path against the other: each path is allowed 1e-5 of the
# oracle, so two correct paths may differ by twice that.  (Rows of one launch differ in scale by a factor of ten with these weights;
# measured on an MI355X: worst row 8.3e-6, median row 2.1e-6, and on the worst rows the exact-f32 path is the one further from the
# float64 oracle.  A damaged row would be off by orders of magnitude.)  The log-densities are held per row at the bar itself.
ROW_TOL = 2 * TOL
# The one case exempt from "another route changes the bits": 257 atoms x 3 rows as likelihoods are THREE floats of magnitude 4000, and
# two routes that agree to 1e-7 can round to the same bits there, and did.  That launch size differs bit-wise in its "sample" form
# (kernel-v257-s3-sample, 4600 floats), and the route string is compared in both.
FEW_FLOATS = ("kernel-v257-s3-loglik",)
# A log-density is held per row at 1e-5 of ITSELF: every row of every launch must keep it away from 0 (asserted on the exact-f32 path's
# output over the whole launch; measured: the smallest of any row is 554, profiles/launch_sizes.txt)
MIN_ABS_LOGP = 1.0
PER_OP = (ls.SIMPLE, ls.SIMPLE_H3)
PATH_NAMES = {0: "AUTO", 1: "FUSED", ls.SIMPLE: "SIMPLE", 3: "FUSED_H3", 4: "FUSED_H1", ls.SIMPLE_H3: "SIMPLE_H3"}
# the flags that compete with each decision; which of them equals the default and which must differ is the restatement's answer
AB_FLAGS = {"fold": (DebugFlag.FOLD_ONE_WG_PER_TILE, DebugFlag.FOLD_GEMM_SEPARATE),
            "tokens": (DebugFlag.TOKENS_NT4, DebugFlag.TOKENS_NT3),
            "sdpa": (DebugFlag.SDPA_SCALAR,)}
# ... and the two a launch takes by itself at these sizes: the only same-route runs made (bit for bit)
SAME_ROUTE = (DebugFlag.FOLD_ONE_WG_PER_TILE, DebugFlag.TOKENS_NT4)

_models = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    _models.clear()
    torch.cuda.empty_cache()


def _model(case, path):
    """One product model per (full model, path) for the whole file; `path` None: the constructor's default preference."""
    key = (case.model, path)
    if getattr(_models.get(key), "demoted", False):   # a case that failed on non-finite values must not fail the cases behind it
        del _models[key]
    if key not in _models:
        make = H.tw_kernel_model if case.model == "kernel" else H.tw_dense_model
        _models[key] = make(ls.state_dict(case.model), path=path)
    return _models[key]


def _run(m, case, d):
    """The case's call over the whole launch -> CPU tensors in the order of launch_sizes.OUTPUTS."""
    if case.form == "sample":
        out = m.conditional_sample_with_logp(atom_types=d["atom_types"], x_coords=d["x_coords"], x_velocs=d["x_velocs"], adj_list=None,
                                             edge_batch_idx=None, masked_elements=d["masked"], num_samples=case.n_rows,
                                             z_coords=d["z_coords"].clone(), z_velocs=d["z_velocs"].clone())
        return tuple(t.cpu() for t in out)
    return (m.log_likelihood(atom_types=d["atom_types"], x_coords=d["x_coords"], x_velocs=d["x_velocs"], y_coords=d["y_coords"],
                             y_velocs=d["y_velocs"], adj_list=None, edge_batch_idx=None, masked_elements=d["masked"]).cpu(),)


def _check_rows(case, out, label, route):
    """All rows finite on the unmasked atoms; the checked rows against the oracle at the bar.  Prints the run's line."""
    assert all(t.shape[0] == case.n_rows for t in out), [t.shape for t in out]
    for name, t in zip(ls.OUTPUTS[case.form], out):
        assert bool(torch.isfinite(ls.unmasked(case, name, t)).all()), (label, name, "non-finite on an unmasked atom")
    rows = torch.tensor(ls.checked_rows(case))
    errs = ls.errors(case, tuple(t[rows] for t in out), ls.oracle(case))
    worst = max(errs, key=errs.get)
    # (a line of its own: under `pytest -q -s` the progress dot of the previous test id has no newline behind it)
    print(f"\nlaunch_sizes | {case.name} | {label} | {route or '-'} | {errs[worst]:.2e} ({worst}) | {TOL:.0e}")
    assert max(errs.values()) < TOL, (label, route, errs)


def _per_row_errors(case, got, want):
    """{output: worst row} - every row's max |a - b| over that row's max |b|, no row left out."""
    errs = {}
    for name, a, b in zip(ls.OUTPUTS[case.form], got, want):
        a, b = ls.unmasked(case, name, a).double().reshape(case.n_rows, -1), ls.unmasked(case, name, b).double().reshape(case.n_rows, -1)
        assert a.shape == b.shape and a.shape[0] == case.n_rows
        errs[name] = float(((a - b).abs().amax(1) / b.abs().amax(1).clamp_min(1e-30)).max())
    return errs


def _reported_route(lib):
    return lib.tw_last_per_op_route().decode()


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in ls.CASES])
def test_case(case):
    lib = _lib.load()
    d = {k: v.cuda() for k, v in ls.inputs(case).items()}
    outs = {}
    for path in PER_OP:
        m = _model(case, path)
        outs[path] = _run(m, case, d)
        route = _reported_route(lib)
        assert route == ls.route(case, path), (PATH_NAMES[path], route, ls.route(case, path))
        _check_rows(case, outs[path], PATH_NAMES[path], route)
        H.assert_not_demoted(m)
    # every row: the split-fp16 per-op path against the exact-f32 one
    whole = ls.errors(case, outs[ls.SIMPLE_H3], outs[ls.SIMPLE])
    print(f"launch_sizes | {case.name} | SIMPLE_H3 vs SIMPLE, all {case.n_rows} rows | - | {max(whole.values()):.2e} ({max(whole, key=whole.get)}) | {TOL:.0e}")
    assert max(whole.values()) < TOL, whole
    rows_err = _per_row_errors(case, outs[ls.SIMPLE_H3], outs[ls.SIMPLE])
    smallest = float(outs[ls.SIMPLE][-1].abs().min())   # (the last output is the log-density in both call forms)
    print(f"launch_sizes | {case.name} | SIMPLE, smallest |log-density| of {case.n_rows} rows | - | {smallest:.1f} | > {MIN_ABS_LOGP:.0f}")
    assert smallest > MIN_ABS_LOGP, ("a row's log-density is too near 0 for a bar relative to itself", smallest)
    for name, e in rows_err.items():
        bar = TOL if name in ("logp", "loglik") else ROW_TOL
        print(f"launch_sizes | {case.name} | SIMPLE_H3 vs SIMPLE, worst of {case.n_rows} rows over its own scale | - | {e:.2e} ({name}) | {bar:.0e}")
        assert e < bar, (name, rows_err)
    # the model's own default
    m = _model(case, None)
    chosen = m._path_for(case.V)
    out = _run(m, case, d)
    route = _reported_route(lib) if chosen in PER_OP else ""
    if chosen in PER_OP:
        assert route == ls.route(case, chosen), (chosen, route)
    assert chosen == (ls.SIMPLE_H3 if case.model == "dense" or case.V > 192 else 3), chosen
    _check_rows(case, out, f"default -> {PATH_NAMES[chosen]}", route)
    H.assert_not_demoted(m)
    # A/B flags of the decision the case is about
    m = _model(case, ls.SIMPLE_H3)
    default = torch.cat([t.flatten() for t in outs[ls.SIMPLE_H3]])
    plain = ls.route(case, ls.SIMPLE_H3)
    for flag in AB_FLAGS[case.about]:
        want = ls.route(case, ls.SIMPLE_H3, int(flag))
        if want == plain and flag not in SAME_ROUTE:
            continue
        with H.debug_flags(flag):
            out = _run(m, case, d)
            route = _reported_route(lib)
        assert route == want, (flag.name, route, want)
        _check_rows(case, out, f"SIMPLE_H3 {flag.name}", route)
        flat = torch.cat([t.flatten() for t in out])
        if want == plain:
            assert torch.equal(flat, default), f"{flag.name} names the route this launch takes by itself: expected bit-identical results"
        elif case.name not in FEW_FLOATS:
            assert not torch.equal(flat, default), f"{flag.name}: bit-identical to the default - the same route ran twice"
    H.assert_not_demoted(m)
    torch.cuda.synchronize()   # raises if the device reports an error
