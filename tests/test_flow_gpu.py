"""Parity of the HIP flow (through the C ABI) against the committed reference vectors and the
oracle.  Bar: 1e-5 relative (north-star) on sampled coordinates, velocities and log-densities."""
import hashlib

import pytest
import torch

from oracle import flow_oracle as fo
from tests import helpers as H
from timewarp_amd._lib import DebugFlag

pytestmark = pytest.mark.gpu

TOL = 1e-5
SIMPLE, FUSED, H3 = 2, 1, 3
H3_MAX_ATOMS = 48  # the split-fp16 kernels run 48-token waves: floor(48 / V) molecules each, whatever the f32 kernels pick
H3_WIDE_MAX_ATOMS = 160  # kernel attention only: larger molecules are packed over a workgroup's 192 token slots ("wide")


def test_library_sees_gpu():
    from timewarp_amd import _lib

    assert _lib.load().tw_device_count() >= 1
    assert torch.cuda.is_available()


def test_scores_kernel_vs_oracle():
    import ctypes as C
    from timewarp_amd import _lib

    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    for V in (7, 22, 60):
        B = 5
        x = torch.randn(B, V, 3, generator=g) * 0.4
        mask = torch.zeros(B, V, dtype=torch.bool)
        mask[1, V - 2:] = True
        mask[3, V // 2:] = True
        ls = torch.tensor([0.1, 0.2, 0.5, 0.7, 1.0, 1.2])
        ref = fo.kernel_scores(x, mask, ls)
        out = torch.empty(B, 6, V, V, device="cuda")
        xd, md, ld = x.cuda(), mask.to(torch.uint8).cuda(), ls.cuda()
        _lib.check(lib.tw_kernel_scores(xd.data_ptr(), md.data_ptr(), ld.data_ptr(), 6, B, V, 1, int(V > 25),
                                        out.data_ptr(), None), "tw_kernel_scores")
        assert H.rel_err(out.cpu(), ref) < (4e-6 if V > 25 else 2e-6), V  # V>25: torch.cdist's matmul branch, same rounding sequence (tw_cdist_mm)


def test_tiny_kernel_simple_path():
    d, sd = H.load("kernel_tiny")
    m = H.tw_kernel_model(sd, emb=4, d_model=8, ff=16, hidden=8, n_coupling=2, n_layers=2,
                          lengthscales=(0.1, 0.5, 1.2), path=SIMPLE)
    with torch.no_grad():
        m.coords_prior_log_scale.fill_(-0.3)
        m.velocs_prior_log_scale.fill_(0.2)
    m.load_state_dict(sd)
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)
    H.assert_case_close(H.run_model_case(m, d, "b1_"), d, "b1_", tol=TOL)


def test_tiny_kernel_normalise_flag_is_ignored():
    """normalise_kernel_values=False in the config: the reference still normalises (kernel_attention.py:197-206 never
    forwards the flag); vectors generated from a reference model built that way."""
    d, sd = H.load("kernel_nonorm_tiny")
    m = H.tw_kernel_model(sd, emb=4, d_model=8, ff=16, hidden=8, n_coupling=2, n_layers=2,
                          lengthscales=(0.1, 0.5, 1.2), path=SIMPLE, normalise=False)
    assert m.flow.chain[0].scale_transformer.encoder_layers[0].self_attn.attention.normalise_kernel_values is False
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)
    H.assert_case_close(H.run_model_case(m, d, "b1_"), d, "b1_", tol=TOL)


def test_tiny_learnable_lengthscales():
    """attention_type "learnable_kernel", per-layer log_lengthscales all different: forward and reverse
    passes use the lengthscales of the layer the reference evaluates first (weights.py LENGTHSCALES)."""
    d, sd = H.load("kernel_learnable_tiny")
    m = H.tw_kernel_model(sd, emb=4, d_model=8, ff=16, hidden=8, n_coupling=2, n_layers=2,
                          lengthscales=(0.1, 0.5, 1.2), path=SIMPLE, attention_type="learnable_kernel")
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)
    H.assert_case_close(H.run_model_case(m, d, "b1_"), d, "b1_", tol=TOL)


@pytest.mark.parametrize("path", [FUSED, H3])
def test_full_learnable_lengthscales_fused(path):
    """Full-size model with distinct forward / reverse lengthscales on the fused kernels vs the oracle."""
    spec = fo.FlowSpec(variant="kernel", attention_type="learnable_kernel")
    sd = dict(H.full_kernel_sd())
    g = torch.Generator().manual_seed(5)
    base = torch.log(torch.tensor([0.1, 0.2, 0.5, 0.7, 1.0, 1.2]))
    for c in range(8):
        for net in ("scale_transformer", "shift_transformer"):
            for l in range(3):
                sd[f"flow.chain.{c}.{net}.encoder_layers.{l}.self_attn.attention.log_lengthscales"] = \
                    base + torch.randn(6, generator=g) * 0.3
    m = H.tw_kernel_model(sd, path=path, attention_type="learnable_kernel")
    d, _ = H.load("kernel_full_ad")
    at, xc, xv, mk = d["atom_types"], d["x_coords"], d["x_velocs"], d["masked"]
    zc, zv = d["z_coords"], d["z_velocs"]
    ref = fo.conditional_sample_with_logp(sd, spec, at, xc, xv, mk, zc, zv)
    got = m.conditional_sample_with_logp(atom_types=at.cuda(), x_coords=xc.cuda(), x_velocs=xv.cuda(), adj_list=None,
                                         edge_batch_idx=None, masked_elements=mk.cuda(), num_samples=zc.shape[0],
                                         z_coords=zc.cuda(), z_velocs=zv.cuda())
    for a, b in zip(got, ref):
        assert H.rel_err(a.cpu(), b) < 1e-5
    ll_ref = fo.log_likelihood(sd, spec, at, xc, xv, d["y_coords"], d["y_velocs"], mk)
    ll = m.log_likelihood(atom_types=at.cuda(), x_coords=xc.cuda(), x_velocs=xv.cuda(), y_coords=d["y_coords"].cuda(),
                          y_velocs=d["y_velocs"].cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mk.cuda())
    H.assert_not_demoted(m)
    assert H.rel_err(ll.cpu(), ll_ref) < 1e-5


@pytest.mark.parametrize("name,fz", [("kernel_cheb_tiny", False), ("kernel_cheb_zero_tiny", True)])
def test_tiny_chebyshev_attention(name, fz):
    """attention_type "chebyshev_kernel" on the per-op path (tiny model: the fused kernels need d_model 128)."""
    d, sd = H.load(name)
    m = H.tw_kernel_model(sd, emb=4, d_model=8, ff=16, hidden=8, n_coupling=2, n_layers=2, lengthscales=(0.1, 0.5, 1.2),
                          path=0, attention_type="chebyshev_kernel", cheb_order=6, force_asymptotic_zero=fz)
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)
    H.assert_case_close(H.run_model_case(m, d, "b1_"), d, "b1_", tol=TOL)


@pytest.mark.parametrize("path", [SIMPLE, FUSED, H3])
def test_full_chebyshev_attention_all_paths(path):
    """Full-size chebyshev_kernel model against reference vectors: the fused kernels take one score-fragment set per
    (net, layer) of the coupling layer in flight, because every attention layer owns its coefficients."""
    d, _ = H.load("kernel_cheb_full_ad")
    m = H.tw_kernel_model(H.full_cheb_sd(), path=path, attention_type="chebyshev_kernel", cheb_order=6,
                          force_asymptotic_zero=True)
    # Bar against the reference's vectors: 2e-5 on this one case, on every path.  The reverse-move log-density of ONE of the
    # 64 golden rows (row 34) carries 9.8e-6 of the reference's OWN fp32 rounding noise (its fp32 arithmetic against the
    # same computation in fp64; 90th percentile over the rows 2e-7), and every HIP path lands within 8-11e-6 of the
    # vectors on that row while being within 2e-6 of the fp64 result (tools/cheb_noise_floor.py,
    # profiles/r04_chebyshev_noise_floor.txt; r03 held the split-fp16 kernel to 1e-5 here and sat at 0.81e-5 / 1.01e-5
    # depending on the build - rounding order, not correctness).  The sharper statement follows: against fp64 arithmetic.
    out = H.run_model_case(m, d)
    H.assert_case_close(out, d, tol=2e-5)
    rows = torch.tensor([34, 60, 18, 36, 0, 1, 2, 3])   # the four rows with the largest reference noise, four ordinary ones
    n = len(rows)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in H.full_cheb_sd().items()}
    gy, gv = d["s_y_coords"][rows].squeeze(1).double(), d["s_y_velocs"][rows].squeeze(1).double()
    exact = fo.log_likelihood(sd64, H.FULL_CHEB_SPEC, d["atom_types"].repeat(n, 1), gy, -gv, d["x_coords"].double().repeat(n, 1, 1),
                              -d["x_velocs"].double().repeat(n, 1, 1), d["masked"].repeat(n, 1))
    scale = float(d["logp_yx"].abs().max())
    got = float((out["logp_yx"][rows].double() - exact).abs().max()) / scale
    own = float((d["logp_yx"][rows].double() - exact).abs().max()) / scale
    assert got < 5e-6, (got, own)        # measured 1.7-2.0e-6 on every path
    assert own > 5e-6, own               # the reference's own fp32 result is further from fp64 than the kernels are


def test_chebyshev_scores_kernel_vs_oracle():
    import ctypes as C
    from timewarp_amd import _lib

    lib = _lib.load()
    g = torch.Generator().manual_seed(4)
    B, V, H_, order = 3, 22, 6, 9
    x = torch.randn(B, V, 3, generator=g) * 0.4
    mask = torch.zeros(B, V, dtype=torch.bool)
    mask[1, V - 3:] = True
    ls = torch.tensor([0.1, 0.2, 0.5, 0.7, 1.0, 1.2])
    coeffs = torch.randn(H_, order, generator=g) * 0.3
    for fz in (False, True):
        ref = fo.kernel_scores(x, mask, ls, True, coeffs, fz)
        out = torch.empty(B, H_, V, V, device="cuda")
        xd, md, ld, cd = x.cuda(), mask.to(torch.uint8).cuda(), ls.cuda(), coeffs.cuda()
        _lib.check(lib.tw_kernel_scores_cheb(xd.data_ptr(), md.data_ptr(), ld.data_ptr(), cd.data_ptr(), order, int(fz), H_, B, V,
                                             1, 0, out.data_ptr(), None), "tw_kernel_scores_cheb")
        assert H.rel_err(out.cpu(), ref) < 1e-5


def test_tiny_dense_simple_path():
    d, sd = H.load("dense_tiny")
    m = H.tw_dense_model(sd, emb=4, d_model=8, ff=16, hidden=8, n_coupling=2, n_layers=2, n_head=2, rff_dim=4,
                         path=SIMPLE)
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)
    H.assert_case_close(H.run_model_case(m, d, "b1_"), d, "b1_", tol=TOL)


@pytest.mark.parametrize("path", [SIMPLE, FUSED, H3])
def test_netblock_stages_vs_reference_trace(path):
    """Every stage of one coupling net (first net of the reverse pass) against the reference's
    own intermediate activations."""
    d, _ = H.load("kernel_full_ad")
    sd = H.full_kernel_sd()
    m = H.tw_kernel_model(sd, path=path)
    xc = d["x_coords"] - fo.centre_of_mass(d["x_coords"], d["masked"])
    S = 2
    acts, out = m.debug_netblock(7, 0, d["atom_types"].cuda(), xc.cuda(), d["x_velocs"].cuda(), d["masked"].cuda(),
                                 d["z_coords"][:S, 0].cuda(), path)
    H.assert_not_demoted(m)
    names = ["tr_in_mlp", "tr_enc0", "tr_enc1", "tr_enc2"]
    for i, n in enumerate(names):
        e = H.rel_err(acts[i].cpu(), d[n])
        assert e < TOL, (n, e)
    e = H.rel_err(out.cpu(), d["tr_out_mlp"])
    assert e < TOL, ("out_mlp", e)


@pytest.mark.parametrize("path", [SIMPLE, FUSED, H3])
@pytest.mark.parametrize("name,calibrated", [("kernel_full_ad", False), ("kernel_full_ad_calibrated", True)])
def test_full_kernel_ad_golden(path, name, calibrated):
    d, _ = H.load(name)
    m = H.tw_kernel_model(H.full_kernel_sd(calibrated), path=path)
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)


@pytest.mark.parametrize("path", [SIMPLE, FUSED, H3])
def test_full_kernel_v60_golden(path):
    """60 atoms: 4-tile waves in the fused f32 kernel, three molecules per workgroup in the split-fp16 kernel's wide
    layout, and torch.cdist's matmul branch for the scores."""
    d, _ = H.load("kernel_full_v60")
    m = H.tw_kernel_model(H.full_kernel_sd(), path=path)
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)  # r04: 1e-5 above 25 atoms too (tw_cdist_mm reproduces torch.cdist's rounding sequence)


def test_preferred_split_fp16_path_falls_back_per_call(monkeypatch):
    """TW_EXECUTION_PATH=h3: the split-fp16 fused kernels where a layout exists; above them (r06) the per-op path with split-fp16
    linears (TW_PATH_SIMPLE_H3 = 5) instead of the exact-f32 per-op kernels."""
    from timewarp_amd.modules import flow

    monkeypatch.setenv("TW_EXECUTION_PATH", "h3")
    m = H.tw_kernel_model(H.full_kernel_sd(), path=None)
    assert m.execution_path == flow.PREFER_SPLIT_FP16
    assert m._path_for(22) == H3 and m._path_for(30) == H3 and m._path_for(60) == H3 and m._path_for(161) == H3 and m._path_for(193) == 5
    d, _ = H.load("kernel_full_ad")
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)
    assert m._dev_weights["h3"] is not None and m._dev_weights["f32"] is None  # the 22-atom calls ran on the h3 stream
    d, _ = H.load("kernel_full_v60")
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)  # r04: 1e-5 above 25 atoms too (tw_cdist_mm reproduces torch.cdist's rounding sequence)
    assert m._dev_weights["f32"] is None  # 60 atoms run on the split-fp16 kernel too (wide layout)
    dense = H.tw_dense_model(H.full_dense_sd(), path=None)
    # the dense flow has split-fp16 kernels of its own: 48-token waves, and (r05) 64-token waves for 49-64 atoms
    assert dense._path_for(22) == H3 and dense._path_for(60) == H3 and dense._path_for(64) == H3 and dense._path_for(65) == 5


@pytest.mark.parametrize("path", [SIMPLE, FUSED, 0, H3])
def test_full_dense_ad_golden(path):
    """transformer_nvp (dense softmax attention, BASELINE config 4) on the per-op path, on the fused f32-MFMA dense
    net-block kernel, through TW_PATH_AUTO (which must pick the fused kernel for this configuration) and on the
    split-fp16 dense kernel (q k^T and P.V on the half-precision matrix pipe as well)."""
    d, _ = H.load("dense_full_ad")
    m = H.tw_dense_model(H.full_dense_sd(), path=path)
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)
    if path == 0:
        assert m._dev_weights["f32"] is not None  # the fused kernel's weight stream was built and used


@pytest.mark.parametrize("path", [SIMPLE, FUSED, 0, H3, None])
def test_full_dense_posenc_golden(path):
    """transformer_nvp_posenc.yaml at full size (128 random Fourier features of the conditioning positions appended to
    the in-MLP's input, rff_position_encoder.py:57-62): per-op path, the fused f32 dense kernel (cos / sin in its
    prologue, eleven input tiles), TW_PATH_AUTO, the split-fp16 dense kernel (six input k-steps) and the constructor's
    default, which must land on the latter."""
    d, _ = H.load("dense_posenc_full_ad")
    m = H.tw_dense_model(H.full_dense_posenc_sd(), rff_dim=128, path=path)
    if path is None:
        assert m._path_for(22) == H3
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)
    if path == 0:
        assert m._dev_weights["f32"] is not None
    if path in (H3, None):
        assert m._dev_weights["h3"] is not None and m._dev_weights["f32"] is None


@pytest.mark.parametrize("path", [SIMPLE, FUSED, H3])
def test_full_dense_padded_golden(path):
    """Padded batch (22 / 17 / 20 real atoms) through nn.MultiheadAttention's src_key_padding_mask
    (transformer_block.py:57-68): reference vectors."""
    d, _ = H.load("dense_full_padded")
    m = H.tw_dense_model(H.full_dense_sd(), path=path)
    out = m.log_likelihood(atom_types=d["atom_types"].cuda(), x_coords=d["x_coords"].cuda(), x_velocs=d["x_velocs"].cuda(),
                           y_coords=d["y_coords"].cuda(), y_velocs=d["y_velocs"].cuda(), adj_list=None, edge_batch_idx=None,
                           masked_elements=d["masked"].cuda()).cpu()
    H.assert_not_demoted(m)
    assert H.rel_err(out, d["loglik"]) < TOL


@pytest.mark.parametrize("V,lens", [(22, [22, 20, 22, 17, 22]), (7, [7, 5, 6, 7, 7, 3, 7, 7, 7]), (30, [30, 28, 25]),
                                    (16, [16, 13, 16, 16, 16, 10, 16]), (48, [48, 40, 33]), (60, [60, 44]), (64, [64, 51]),
                                    (49, [49, 49, 31, 49, 49, 49]), (57, [57, 50, 57, 57, 57, 57, 57, 57, 40])])
def test_fused_dense_batched_padding_vs_oracle(V, lens):
    """Ragged batches on the fused dense kernel against the oracle: 3- and 4-tile waves, several molecules per wave,
    padded keys, one molecule filling the whole wave."""
    sd = H.full_dense_sd()
    g = torch.Generator().manual_seed(200 + V)
    B = len(lens)
    at = torch.randint(0, 5, (B, V), generator=g)
    x_c = torch.randn(B, V, 3, generator=g) * 0.3
    x_v = torch.randn(B, V, 3, generator=g) * 0.5
    y_c = x_c + torch.randn(B, V, 3, generator=g) * 0.02
    y_v = torch.randn(B, V, 3, generator=g) * 0.5
    mask = torch.zeros(B, V, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, n:] = True
    ref = fo.log_likelihood(sd, H.FULL_DENSE_SPEC, at, x_c, x_v, y_c, y_v, mask)
    for path in (FUSED, SIMPLE, H3):   # (r05: 49-64 atoms on the split-fp16 path too - 64-token waves, attention block compiled C++)
        m = H.tw_dense_model(sd, path=path)
        out = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                               y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda()).cpu()
        H.assert_not_demoted(m)
        assert H.rel_err(out, ref) < TOL, (path, H.rel_err(out, ref))


@pytest.mark.parametrize("path", [FUSED, H3])
def test_fused_dense_S1000_roundtrip(path):
    """BASELINE config 4 size (1000 proposals): reverse pass then forward pass recover log p; 16 spread rows vs oracle."""
    sd = H.full_dense_sd()
    m = H.tw_dense_model(sd, path=path)
    d, _ = H.load("dense_full_ad")
    S = 1000
    g = torch.Generator().manual_seed(6)
    zc, zv = fo.draw_latents(sd, S, (1, 22, 3), g)
    at, xc, xv, mk = d["atom_types"].cuda(), d["x_coords"].cuda(), d["x_velocs"].cuda(), d["masked"].cuda()
    yc, yv, lp = m.conditional_sample_with_logp(atom_types=at, x_coords=xc, x_velocs=xv, adj_list=None, edge_batch_idx=None,
                                                masked_elements=mk, num_samples=S, z_coords=zc.cuda(), z_velocs=zv.cuda())
    ll = m.log_likelihood(atom_types=at.repeat(S, 1), x_coords=xc.repeat(S, 1, 1), x_velocs=xv.repeat(S, 1, 1),
                          y_coords=yc.squeeze(1), y_velocs=yv.squeeze(1), adj_list=None, edge_batch_idx=None,
                          masked_elements=mk.repeat(S, 1))
    H.assert_not_demoted(m)
    assert H.rel_err(ll.cpu(), lp.squeeze(1).cpu()) < TOL
    rows = torch.tensor([0, 1, 7, 8, 250, 251, 499, 500, 503, 504, 750, 901, 992, 997, 998, 999])
    ryc, ryv, rlp = fo.conditional_sample_with_logp(sd, H.FULL_DENSE_SPEC, d["atom_types"], d["x_coords"], d["x_velocs"],
                                                    d["masked"], zc[rows], zv[rows])
    assert H.rel_err(yc.cpu()[rows], ryc) < TOL and H.rel_err(yv.cpu()[rows], ryv) < TOL and H.rel_err(lp.cpu()[rows], rlp) < TOL


@pytest.mark.parametrize("V,lens", [(22, [22, 20, 22, 17, 22]), (7, [7, 5, 6, 7, 7, 3, 7, 7, 7]), (30, [30, 28, 25]),
                                    (12, [12, 12, 9, 12, 11, 12, 12, 5, 12]), (16, [16, 13, 16, 16, 16, 10, 16]),
                                    (24, [24, 21, 24]), (48, [48, 40, 33]), (17, [17, 17, 12, 17, 15]),
                                    (20, [20, 18, 20]), (21, [21, 21, 21, 9, 21]), (32, [32, 26, 32]), (40, [40, 31]),
                                    (5, [5] * 19 + [3, 4]), (60, [60, 44, 60, 60, 51, 60, 60]), (49, [49, 49, 30, 49]),
                                    (64, [64, 51, 64, 64])])
def test_fused_batched_padding_vs_oracle(V, lens):
    """Ragged batch (different conditioning state per row, padded atoms) on the fused path against
    the oracle: pins the per-row score fragments and the mask handling
    (reference property test: tests/test_batching.py:132-177)."""
    sd = H.full_kernel_sd()
    g = torch.Generator().manual_seed(100 + V)
    B = len(lens)
    at = torch.randint(0, 5, (B, V), generator=g)
    x_c = torch.randn(B, V, 3, generator=g) * 0.3
    x_v = torch.randn(B, V, 3, generator=g) * 0.5
    y_c = x_c + torch.randn(B, V, 3, generator=g) * 0.02
    y_v = torch.randn(B, V, 3, generator=g) * 0.5
    mask = torch.zeros(B, V, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, n:] = True
    ref = fo.log_likelihood(sd, H.FULL_KERNEL_SPEC, at, x_c, x_v, y_c, y_v, mask)
    for path in (FUSED, SIMPLE, H3):
        m = H.tw_kernel_model(sd, path=path)
        out = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                               y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda()).cpu()
        H.assert_not_demoted(m)
        assert H.rel_err(out, ref) < TOL, (path, H.rel_err(out, ref))
        # batched == per item (tests/test_batching.py)
        one = m.log_likelihood(atom_types=at[1:2].cuda(), x_coords=x_c[1:2].cuda(), x_velocs=x_v[1:2].cuda(),
                               y_coords=y_c[1:2].cuda(), y_velocs=y_v[1:2].cuda(), adj_list=None, edge_batch_idx=None,
                               masked_elements=mask[1:2].cuda()).cpu()
        assert abs(float(one[0] - out[1])) < 1e-4 * max(1.0, abs(float(out[1])))


@pytest.mark.parametrize("V,lens", [(22, [22, 20, 22, 17, 22]), (24, [24, 24, 21]), (16, [16, 13, 16, 16, 16, 10, 16]),
                                    (40, [40, 31, 40]), (48, [48, 48])])
def test_encoder_stack_statement_vs_per_section_build(V, lens):
    """The split-fp16 kernel runs its encoder stack as ONE generated asm statement (tools/gen_h3_enc_asm.py: residual folded
    into the accumulator seeds, hand-written LayerNorm / split / transposer) unless DebugFlag.PER_SECTION asks for the
    per-section build (asm GEMM blocks, compiled glue).  Same arithmetic up to summation order and v_rsq_f32: both builds
    on the same ragged batch - windowed (two or more molecules per wave) and full mixing, with and without padding
    tokens - must agree inside the parity bar (measured: log-densities 1e-7, sampled coordinates up to 3e-6 after eight
    coupling layers - profiles/r03_enc_tests.txt), and a repeated run of one build must be bit-identical."""
    sd = H.full_kernel_sd()
    g = torch.Generator().manual_seed(500 + V)
    B = len(lens)
    at = torch.randint(0, 5, (B, V), generator=g)
    x_c = torch.randn(B, V, 3, generator=g) * 0.3
    x_v = torch.randn(B, V, 3, generator=g) * 0.5
    y_c = x_c + torch.randn(B, V, 3, generator=g) * 0.02
    y_v = torch.randn(B, V, 3, generator=g) * 0.5
    mask = torch.zeros(B, V, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, n:] = True
    m = H.tw_kernel_model(sd, path=H3)
    S = 37
    zc, zv = fo.draw_latents(sd, S, (1, V, 3), g)

    def run():
        ll = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                              y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda()).cpu()
        yc, yv, lp = m.conditional_sample_with_logp(
            atom_types=at[:1].cuda(), x_coords=x_c[:1].cuda(), x_velocs=x_v[:1].cuda(), adj_list=None, edge_batch_idx=None,
            masked_elements=mask[:1].cuda(), num_samples=S, z_coords=zc.cuda(), z_velocs=zv.cuda())
        return ll, yc.cpu(), yv.cpu(), lp.cpu()

    stack = run()
    again = run()
    with H.debug_flags(DebugFlag.PER_SECTION):
        sections = run()
    H.assert_not_demoted(m)
    for a, b in zip(stack, again):
        assert torch.equal(a, b)
    errs = {name: H.rel_err(a, b) for name, a, b in zip(("loglik", "y_coords", "y_velocs", "logp"), stack, sections)}
    print("encoder-stack vs per-section build:", errs)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("emb", [16, 24])
def test_other_embedding_widths_take_the_general_input_path(emb):
    """atom_embedding_dim 32 (every config of the reference) has a straight-line input-feature path in the fused kernels'
    prologues; any other width that fits the 64-column input tile goes through the general element-by-element loop.  Both
    fused kernels on 16 and 24 embedding columns against the oracle (the f32 kernel takes up to 39: 48-column input tile)."""
    spec = fo.FlowSpec(variant="kernel", num_transformer_layers=1, num_coupling_layers=2)
    sd = fo.synth_state_dict(fo.make_template(spec, atom_embedding_dim=emb), 0)
    g = torch.Generator().manual_seed(700 + emb)
    V, lens = 22, [22, 18, 22, 22, 21]
    B = len(lens)
    at = torch.randint(0, 5, (B, V), generator=g)
    x_c = torch.randn(B, V, 3, generator=g) * 0.3
    x_v = torch.randn(B, V, 3, generator=g) * 0.5
    y_c = x_c + torch.randn(B, V, 3, generator=g) * 0.02
    y_v = torch.randn(B, V, 3, generator=g) * 0.5
    mask = torch.zeros(B, V, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, n:] = True
    ref = fo.log_likelihood(sd, spec, at, x_c, x_v, y_c, y_v, mask)
    for path in (FUSED, H3):
        m = H.tw_kernel_model(sd, emb=emb, path=path, n_coupling=2, n_layers=1)
        out = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                               y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda()).cpu()
        H.assert_not_demoted(m)
        assert H.rel_err(out, ref) < TOL, (path, H.rel_err(out, ref))


@pytest.mark.parametrize("n_layers", [1, 2, 5])
def test_encoder_stack_statement_layer_counts_vs_oracle(n_layers):
    """The layer loop lives inside the statement (scales, side blocks and, for chebyshev_kernel, score fragments advance
    per layer there): 1, 2 and 5 encoder layers against the oracle."""
    spec = fo.FlowSpec(variant="kernel", num_transformer_layers=n_layers, num_coupling_layers=2)
    sd = fo.synth_state_dict(fo.make_template(spec), 0)
    g = torch.Generator().manual_seed(600 + n_layers)
    V, lens = 22, [22, 19, 22]
    B = len(lens)
    at = torch.randint(0, 5, (B, V), generator=g)
    x_c = torch.randn(B, V, 3, generator=g) * 0.3
    x_v = torch.randn(B, V, 3, generator=g) * 0.5
    y_c = x_c + torch.randn(B, V, 3, generator=g) * 0.02
    y_v = torch.randn(B, V, 3, generator=g) * 0.5
    mask = torch.zeros(B, V, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, n:] = True
    ref = fo.log_likelihood(sd, spec, at, x_c, x_v, y_c, y_v, mask)
    m = H.tw_kernel_model(sd, path=H3, n_coupling=2, n_layers=n_layers)
    out = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                           y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda()).cpu()
    H.assert_not_demoted(m)
    assert H.rel_err(out, ref) < TOL, H.rel_err(out, ref)


@pytest.mark.parametrize("V,lens,paths", [(64, [64, 51], (FUSED, SIMPLE)), (70, [70, 44, 70], (0, SIMPLE, H3)),
                                          (100, [100, 87], (0, H3)), (96, [96, 90, 96], (H3,)), (160, [160, 131], (H3,)),
                                          (81, [81, 70, 81], (H3,)), (88, [88, 88, 61, 88, 88], (SIMPLE, H3)),
                                          (95, [95, 95, 95], (H3,)), (161, [161, 140], (H3,)), (176, [176, 176, 133], (SIMPLE, H3)),
                                          (192, [192, 161, 192], (H3,))])
def test_large_molecules_vs_oracle(V, lens, paths):
    """Maximum sizes: 64 atoms is the largest molecule a fused f32 wave holds (4 tiles); beyond it TW_PATH_AUTO has to fall
    back to the per-op path, while the split-fp16 kernel's wide layout goes on to 160 atoms (two, then one molecule per
    workgroup).  All above 25 atoms, so the scores follow torch.cdist's matmul branch.  81 .. 95 atoms (refused
    until r04) take a slot stride of 96 instead of sitting back to back - molecule 0 on waves 0-1, molecule 1 on waves 2-3,
    padding slots behind each - odd and even row counts, so that the last workgroup holds one molecule and two.  161 .. 192
    atoms (r04): one molecule over the workgroup's 192 slots, every wave mixing against all six key groups."""
    sd = H.full_kernel_sd()
    g = torch.Generator().manual_seed(300 + V)
    B = len(lens)
    at = torch.randint(0, 5, (B, V), generator=g)
    x_c = torch.randn(B, V, 3, generator=g) * 0.6
    x_v = torch.randn(B, V, 3, generator=g) * 0.5
    y_c = x_c + torch.randn(B, V, 3, generator=g) * 0.02
    y_v = torch.randn(B, V, 3, generator=g) * 0.5
    mask = torch.zeros(B, V, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, n:] = True
    ref = fo.log_likelihood(sd, H.FULL_KERNEL_SPEC, at, x_c, x_v, y_c, y_v, mask)
    for path in paths:
        m = H.tw_kernel_model(sd, path=path)
        out = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                               y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda()).cpu()
        H.assert_not_demoted(m)
        assert H.rel_err(out, ref) < TOL, (path, H.rel_err(out, ref))
    if 81 <= V <= 95 or V > 160:
        # the reverse pass as well (its coupling prologue reduces the log-determinant over the strided slots)
        S = 5
        zc, zv = torch.randn(S, 1, V, 3, generator=g), torch.randn(S, 1, V, 3, generator=g)
        mk1 = mask[1:2]
        ryc, ryv, rlp = fo.conditional_sample_with_logp(sd, H.FULL_KERNEL_SPEC, at[1:2], x_c[1:2], x_v[1:2], mk1, zc, zv)
        m = H.tw_kernel_model(sd, path=H3)
        yc, yv, lp = m.conditional_sample_with_logp(atom_types=at[1:2].cuda(), x_coords=x_c[1:2].cuda(), x_velocs=x_v[1:2].cuda(),
                                                    adj_list=None, edge_batch_idx=None, masked_elements=mk1.cuda(),
                                                    num_samples=S, z_coords=zc.cuda(), z_velocs=zv.cuda())
        H.assert_not_demoted(m)
        assert H.rel_err(yc.cpu(), ryc) < TOL and H.rel_err(yv.cpu(), ryv) < TOL and H.rel_err(lp.cpu(), rlp) < TOL
    if V > 64:
        with pytest.raises(RuntimeError, match="unsupported"):
            H.tw_kernel_model(sd, path=FUSED).log_likelihood(
                atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(), y_velocs=y_v.cuda(),
                adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda())


@pytest.mark.parametrize("V,lens", [(25, [25, 25, 20, 25, 25, 25, 25, 11, 25]), (30, [30, 28, 30, 30, 25, 30, 30, 30]),
                                    (32, [32, 32, 17, 32, 32, 32, 32]), (38, [38, 38, 38, 30, 38, 38]), (48, [48, 40, 48, 48, 48])])
def test_wide_layout_on_25_to_48_atoms_vs_oracle(V, lens):
    """r04: the wide layout (floor(192 / V) molecules back to back over a workgroup's four waves) also takes molecules of
    25 - 48 atoms, for which a 48-token wave holds only one.  Forced here (DebugFlag.ALWAYS_WIDE) on ragged batches of more
    than one workgroup, against the oracle and against the narrow layout (NEVER_WIDE) - the launch code picks between the
    two by rounds of the chip (next test)."""
    sd = H.full_kernel_sd()
    g = torch.Generator().manual_seed(700 + V)
    B = len(lens)
    at = torch.randint(0, 5, (B, V), generator=g)
    x_c = torch.randn(B, V, 3, generator=g) * 0.4
    x_v = torch.randn(B, V, 3, generator=g) * 0.5
    y_c = x_c + torch.randn(B, V, 3, generator=g) * 0.02
    y_v = torch.randn(B, V, 3, generator=g) * 0.5
    mask = torch.zeros(B, V, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, n:] = True
    ref = fo.log_likelihood(sd, H.FULL_KERNEL_SPEC, at, x_c, x_v, y_c, y_v, mask)
    args = dict(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(), y_velocs=y_v.cuda(),
                adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda())
    outs = {}
    for flag in (DebugFlag.ALWAYS_WIDE, DebugFlag.NEVER_WIDE):
        with H.debug_flags(flag):
            m = H.tw_kernel_model(sd, path=H3)
            outs[flag] = m.log_likelihood(**args).cpu()
            H.assert_not_demoted(m)
    tol = TOL
    assert H.rel_err(outs[DebugFlag.ALWAYS_WIDE], ref) < tol, H.rel_err(outs[DebugFlag.ALWAYS_WIDE], ref)
    assert H.rel_err(outs[DebugFlag.NEVER_WIDE], ref) < tol


def test_layout_choice_by_rounds_of_the_chip():
    """Which layout a launch takes between 25 and 48 atoms follows from its row count (h3_wide_choice): 768 proposals of a
    30-atom molecule are one round of workgroups wide (2 x 128) against two narrow (2 x 192); 1000 proposals are two rounds
    either way and stay narrow.  Both must give the oracle's numbers; that the choice is really made shows in the workspace
    the library asks for and in the two results differing in the last bits."""
    sd = H.full_kernel_sd()
    V = 30
    g = torch.Generator().manual_seed(31)
    at = torch.randint(0, 5, (1, V), generator=g)
    x_c = torch.randn(1, V, 3, generator=g) * 0.4
    x_v = torch.randn(1, V, 3, generator=g) * 0.5
    mk = torch.zeros(1, V, dtype=torch.bool)
    for S in (768, 1000):
        zc, zv = fo.draw_latents(sd, S, (1, V, 3), g)
        res = {}
        for flag in (0, DebugFlag.NEVER_WIDE, DebugFlag.ALWAYS_WIDE):
            with H.debug_flags(flag):
                m = H.tw_kernel_model(sd, path=H3)
                yc, yv, lp = m.conditional_sample_with_logp(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(),
                                                            adj_list=None, edge_batch_idx=None, masked_elements=mk.cuda(),
                                                            num_samples=S, z_coords=zc.cuda(), z_velocs=zv.cuda())
                res[flag] = (yc.cpu(), lp.cpu())
                H.assert_not_demoted(m)
        chosen = DebugFlag.ALWAYS_WIDE if S == 768 else DebugFlag.NEVER_WIDE
        other = DebugFlag.NEVER_WIDE if S == 768 else DebugFlag.ALWAYS_WIDE
        assert torch.equal(res[0][0], res[chosen][0]) and torch.equal(res[0][1], res[chosen][1]), S
        assert not torch.equal(res[0][1], res[other][1]), S
        rows = torch.tensor([0, 1, 5, 6, S // 2, S - 7, S - 1])
        ryc, _, rlp = fo.conditional_sample_with_logp(sd, H.FULL_KERNEL_SPEC, at, x_c, x_v, mk, zc[rows], zv[rows])
        for flag in (DebugFlag.NEVER_WIDE, DebugFlag.ALWAYS_WIDE):
            assert H.rel_err(res[flag][0][rows], ryc) < TOL and H.rel_err(res[flag][1][rows], rlp) < TOL, (S, flag)


# (flags as plain ints: they name the test ids)
@pytest.mark.parametrize("V,lens,layout", [(30, [30, 28, 25, 30, 30, 30, 30], int(DebugFlag.ALWAYS_WIDE)),
                                           (60, [60, 44, 60, 60], int(DebugFlag.NEVER_NT4)),
                                           (70, [70, 44, 70], 0), (100, [100, 87, 100], 0), (160, [160, 131], 0), (180, [180, 171], 0)])
def test_wide_layout_transposed_tile_through_matrix_pipe(V, lens, layout):
    """r04: the wide layout's shared transposed tile is written through the matrix pipe (K = 16 MFMAs against the identity, 48
    eight-byte stores per lane and layer) instead of with 192 two-byte stores (DebugFlag.WIDE_XT_BYTE_STORES keeps r03's form: the
    section profile had 46 k cycles per layer there).  The transposition is exact, so both builds must agree bit for bit -
    on the split-fp16 kernel and on the fast path, whichever statement (three- or five-group windows) the size takes."""
    sd = H.full_kernel_sd()
    g = torch.Generator().manual_seed(1700 + V)
    B = len(lens)
    at = torch.randint(0, 5, (B, V), generator=g)
    x_c = torch.randn(B, V, 3, generator=g) * 0.5
    x_v = torch.randn(B, V, 3, generator=g) * 0.5
    y_c = x_c + torch.randn(B, V, 3, generator=g) * 0.02
    y_v = torch.randn(B, V, 3, generator=g) * 0.5
    mask = torch.zeros(B, V, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, n:] = True
    ref = fo.log_likelihood(sd, H.FULL_KERNEL_SPEC, at, x_c, x_v, y_c, y_v, mask)
    args = dict(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(), y_velocs=y_v.cuda(),
                adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda())
    outs = {}
    for path in (H3, 4):
        for flag in (0, DebugFlag.WIDE_XT_BYTE_STORES):
            with H.debug_flags(layout | flag):
                m = H.tw_kernel_model(sd, path=path)
                outs[path, flag] = m.log_likelihood(**args).cpu()
                H.assert_not_demoted(m)
    assert H.rel_err(outs[H3, 0], ref) < TOL, H.rel_err(outs[H3, 0], ref)
    assert torch.equal(outs[H3, 0], outs[H3, DebugFlag.WIDE_XT_BYTE_STORES]) and torch.equal(outs[4, 0], outs[4, DebugFlag.WIDE_XT_BYTE_STORES])


@pytest.mark.parametrize("V,lens", [(65, [65, 65, 50, 65, 65]), (70, [70, 44, 70]), (80, [80, 80, 80, 66]), (88, [88, 61, 88]),
                                    (96, [96, 90, 96, 96])])
def test_wide_layout_three_group_windows_vs_five(V, lens):
    """r04: molecules of 65 .. 96 atoms sit at a slot stride of 96 in the wide layout (two per workgroup either way) - each on
    its own pair of waves, so a wave's keys are its molecule's three K = 32 groups: tw_h3_attns3_asm.inc (54 mixing MFMAs per
    head and k-step, 18 fragment loads per head) instead of the five-group statement (90 / 30; DebugFlag.WIDE_FIVE_GROUP_WINDOWS,
    molecules back to back where that fits).  Both against the oracle on ragged batches of odd and even row counts, on the
    split-fp16 kernel; the fast mode's two statements against each other at its own error."""
    sd = H.full_kernel_sd()
    g = torch.Generator().manual_seed(1200 + V)
    B = len(lens)
    at = torch.randint(0, 5, (B, V), generator=g)
    x_c = torch.randn(B, V, 3, generator=g) * 0.55
    x_v = torch.randn(B, V, 3, generator=g) * 0.5
    y_c = x_c + torch.randn(B, V, 3, generator=g) * 0.02
    y_v = torch.randn(B, V, 3, generator=g) * 0.5
    mask = torch.zeros(B, V, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, n:] = True
    ref = fo.log_likelihood(sd, H.FULL_KERNEL_SPEC, at, x_c, x_v, y_c, y_v, mask)
    args = dict(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(), y_velocs=y_v.cuda(),
                adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda())
    outs = {}
    for path in (H3, 4):
        for flag in (0, DebugFlag.WIDE_FIVE_GROUP_WINDOWS):
            with H.debug_flags(flag):
                m = H.tw_kernel_model(sd, path=path)
                outs[path, flag] = m.log_likelihood(**args).cpu()
                H.assert_not_demoted(m)
    assert H.rel_err(outs[H3, 0], ref) < TOL, H.rel_err(outs[H3, 0], ref)
    assert H.rel_err(outs[H3, DebugFlag.WIDE_FIVE_GROUP_WINDOWS], ref) < TOL
    assert H.rel_err(outs[H3, 0], outs[H3, DebugFlag.WIDE_FIVE_GROUP_WINDOWS]) < 2e-6
    assert 0 < H.rel_err(outs[4, 0], ref) < 3e-3 and H.rel_err(outs[4, 0], outs[4, DebugFlag.WIDE_FIVE_GROUP_WINDOWS]) < 3e-3
    # the reverse pass of one conditioning state (shared score fragments), five proposals
    S = 5
    zc, zv = torch.randn(S, 1, V, 3, generator=g), torch.randn(S, 1, V, 3, generator=g)
    ryc, ryv, rlp = fo.conditional_sample_with_logp(sd, H.FULL_KERNEL_SPEC, at[2:3], x_c[2:3], x_v[2:3], mask[2:3], zc, zv)
    m = H.tw_kernel_model(sd, path=H3)
    yc, yv, lp = m.conditional_sample_with_logp(atom_types=at[2:3].cuda(), x_coords=x_c[2:3].cuda(), x_velocs=x_v[2:3].cuda(),
                                                adj_list=None, edge_batch_idx=None, masked_elements=mask[2:3].cuda(),
                                                num_samples=S, z_coords=zc.cuda(), z_velocs=zv.cuda())
    H.assert_not_demoted(m)
    assert H.rel_err(yc.cpu(), ryc) < TOL and H.rel_err(yv.cpu(), ryv) < TOL and H.rel_err(lp.cpu(), rlp) < TOL


@pytest.mark.parametrize("V,lens", [(49, [49, 49, 40, 49, 49, 49, 49, 31, 49]), (52, [52, 52, 52, 45, 52]),
                                    (60, [60, 60, 60, 60, 51, 60, 60, 60, 60, 60, 42]), (64, [64, 64, 50, 64, 64, 64])])
def test_64_token_waves_on_49_to_64_atoms_vs_oracle(V, lens):
    """r04: 64-token waves - ONE molecule of 49-64 atoms per wave (NT = 4, keys = two K = 32 groups, a three-slot weight ring
    beside four 32 KiB wave blocks; the FFN as generated asm, tools/gen_h3_ffn_asm.py --nt=4, the rest compiled C++) - the geometry that runs BASELINE config 3 (60 atoms x 512 proposals) in one round of
    the chip.  Forced here (DebugFlag.ALWAYS_NT4) on ragged batches of more than one workgroup, against the oracle and
    against the wide layout (NEVER_NT4); the launch code picks between the two (next test)."""
    sd = H.full_kernel_sd()
    g = torch.Generator().manual_seed(900 + V)
    B = len(lens)
    at = torch.randint(0, 5, (B, V), generator=g)
    x_c = torch.randn(B, V, 3, generator=g) * 0.5
    x_v = torch.randn(B, V, 3, generator=g) * 0.5
    y_c = x_c + torch.randn(B, V, 3, generator=g) * 0.02
    y_v = torch.randn(B, V, 3, generator=g) * 0.5
    mask = torch.zeros(B, V, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, n:] = True
    ref = fo.log_likelihood(sd, H.FULL_KERNEL_SPEC, at, x_c, x_v, y_c, y_v, mask)
    args = dict(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(), y_velocs=y_v.cuda(),
                adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda())
    outs = {}
    for flag in (DebugFlag.ALWAYS_NT4, DebugFlag.NEVER_NT4):
        with H.debug_flags(flag):
            m = H.tw_kernel_model(sd, path=H3)
            outs[flag] = m.log_likelihood(**args).cpu()
            H.assert_not_demoted(m)
    assert H.rel_err(outs[DebugFlag.ALWAYS_NT4], ref) < TOL, H.rel_err(outs[DebugFlag.ALWAYS_NT4], ref)
    assert H.rel_err(outs[DebugFlag.NEVER_NT4], ref) < TOL
    assert not torch.equal(outs[DebugFlag.ALWAYS_NT4], outs[DebugFlag.NEVER_NT4])   # two different kernels did run
    # the all-C++ statement of the 64-token kernel (COMPILED_CPP) against the build with the generated FFN
    with H.debug_flags(DebugFlag.ALWAYS_NT4 | DebugFlag.COMPILED_CPP):
        m = H.tw_kernel_model(sd, path=H3)
        cpp = m.log_likelihood(**args).cpu()
    assert H.rel_err(cpp, ref) < TOL and H.rel_err(cpp, outs[DebugFlag.ALWAYS_NT4]) < 2e-6


def test_64_token_layout_choice_and_config_3_size():
    """BASELINE config 3's size, 60 atoms x 512 proposals: 128 workgroups per net in 64-token waves = one round of the chip,
    171 in the wide layout = 1.34 - the launch code takes the 64-token build there (h3_nt4_choice) and the wide layout at 768
    proposals (two rounds either way, the wide workgroup is cheaper).  Sample rows of both launches against the oracle; that
    the choice is really made shows in the results being bit-identical to the forced layout."""
    sd = H.full_kernel_sd()
    V = 60
    g = torch.Generator().manual_seed(61)
    at = torch.randint(0, 5, (1, V), generator=g)
    x_c = torch.randn(1, V, 3, generator=g) * 0.5
    x_v = torch.randn(1, V, 3, generator=g) * 0.5
    mk = torch.zeros(1, V, dtype=torch.bool)
    for S, chosen, other in ((512, DebugFlag.ALWAYS_NT4, DebugFlag.NEVER_NT4), (768, DebugFlag.NEVER_NT4, DebugFlag.ALWAYS_NT4)):
        zc, zv = fo.draw_latents(sd, S, (1, V, 3), g)
        res = {}
        for flag in (0, DebugFlag.ALWAYS_NT4, DebugFlag.NEVER_NT4):
            with H.debug_flags(flag):
                m = H.tw_kernel_model(sd, path=H3)
                yc, yv, lp = m.conditional_sample_with_logp(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(),
                                                            adj_list=None, edge_batch_idx=None, masked_elements=mk.cuda(),
                                                            num_samples=S, z_coords=zc.cuda(), z_velocs=zv.cuda())
                res[flag] = (yc.cpu(), yv.cpu(), lp.cpu())
                H.assert_not_demoted(m)
        assert all(torch.equal(a, b) for a, b in zip(res[0], res[chosen])), S
        assert not torch.equal(res[0][2], res[other][2]), S
        rows = torch.tensor([0, 1, 3, 4, 7, S // 2, S // 2 + 1, S - 5, S - 1])
        ryc, ryv, rlp = fo.conditional_sample_with_logp(sd, H.FULL_KERNEL_SPEC, at, x_c, x_v, mk, zc[rows], zv[rows])
        for flag in (DebugFlag.ALWAYS_NT4, DebugFlag.NEVER_NT4):
            assert H.rel_err(res[flag][0][rows], ryc) < TOL and H.rel_err(res[flag][1][rows], ryv) < TOL and \
                H.rel_err(res[flag][2][rows], rlp) < TOL, (S, flag)


@pytest.mark.parametrize("variant", ["kernel", "dense"])
def test_per_op_split_path_size_sweep_vs_exact_f32(variant):
    """TW_PATH_SIMPLE_H3 against the exact-f32 per-op kernels (themselves held to the oracle elsewhere) over the sizes where its
    launch forms change: token counts around the 48- / 64-token FFN launches and their four-way split, one to three query tiles of
    the mixing launch with the heads over 1 / 2 / 3 / 6 workgroups, padded key blocks (atoms not a multiple of 16 / 32), one row and
    odd row counts, masked tails; both passes, both nets side by side on two streams.  Conditional samples: 3 (n_atoms) coordinates
    per row, so every token is looked at.  Both paths are also held to the oracle at every size (reverse pass and the likelihood of
    the way back): the two share the scores, centring, input and coupling kernels, so their agreement alone is a self-comparison.
    Measured on an MI355X: worst 6.2e-6 (22 atoms x 7 rows, exact-f32 path, y_coords), the split path 3.6e-6.  The reference's own
    share, measured once on the CPU (16 threads) as the float32 oracle against the float64 oracle on these inputs and its own
    samples: y_coords up to 3.0e-6 (300 x 33; 2.6e-6 at 22 x 7), y_velocs 3.1e-6 (129 x 2), log p 2.1e-7, the likelihood of the way
    back 1.6e-6 - about half of the worst figures above is the float32 reference, and it leaves a kernel 7e-6 under the bar."""
    sd = H.full_kernel_sd() if variant == "kernel" else H.full_dense_sd()
    make = H.tw_kernel_model if variant == "kernel" else H.tw_dense_model
    spec = H.FULL_KERNEL_SPEC if variant == "kernel" else H.FULL_DENSE_SPEC
    m5, m2 = make(sd, path=5), make(sd, path=SIMPLE)
    g = torch.Generator().manual_seed(123)
    for V, S in ((1, 1), (5, 1), (22, 7), (64, 9), (65, 1), (65, 7), (97, 3), (129, 2), (193, 5), (200, 64), (257, 1), (257, 6), (300, 33), (385, 2), (691, 3)):
        at = torch.randint(0, 5, (1, V), generator=g).cuda()
        xc = (torch.randn(1, V, 3, generator=g) * (0.8 if V < 300 else 1.5)).cuda()
        xv = (torch.randn(1, V, 3, generator=g) * 0.5).cuda()
        mk = torch.zeros(1, V, dtype=torch.bool)
        if V > 5:
            mk[0, V - (V % 5):] = True
        mk = mk.cuda()
        zc = (torch.randn(S, 1, V, 3, generator=g) * 0.05).cuda()
        zv = (torch.randn(S, 1, V, 3, generator=g) * 0.5).cuda()
        out = [m.conditional_sample_with_logp(atom_types=at, x_coords=xc, x_velocs=xv, adj_list=None, edge_batch_idx=None, masked_elements=mk,
                                              num_samples=S, z_coords=zc.clone(), z_velocs=zv.clone()) for m in (m5, m2)]
        keep = ~mk[0]
        for a, b in zip(out[0][:2], out[1][:2]):
            assert H.rel_err(a[:, :, keep].cpu(), b[:, :, keep].cpu()) < TOL, (variant, V, S, H.rel_err(a[:, :, keep].cpu(), b[:, :, keep].cpu()))
        assert H.rel_err(out[0][2].cpu(), out[1][2].cpu()) < TOL, (variant, V, S)
        # ... and back: every row conditioned on its own state
        yc, yv = out[1][0].squeeze(1), out[1][1].squeeze(1)
        ll = [m.log_likelihood(atom_types=at.repeat(S, 1), x_coords=yc, x_velocs=yv, y_coords=xc.repeat(S, 1, 1), y_velocs=xv.repeat(S, 1, 1),
                               adj_list=None, edge_batch_idx=None, masked_elements=mk.repeat(S, 1)) for m in (m5, m2)]
        assert H.rel_err(ll[0].cpu(), ll[1].cpu()) < TOL, (variant, V, S, H.rel_err(ll[0].cpu(), ll[1].cpu()))
        # both paths against the oracle as well (the two share the scores, centring, input and coupling kernels: agreeing with each
        # other says nothing about those): the reverse pass on the unmasked atoms, and the likelihood of the way back
        keep_c = keep.cpu()
        ref = fo.conditional_sample_with_logp(sd, spec, at.cpu(), xc.cpu(), xv.cpu(), mk.cpu(), zc.cpu(), zv.cpu())
        ref_ll = fo.log_likelihood(sd, spec, at.cpu().repeat(S, 1), yc.cpu(), yv.cpu(), xc.cpu().repeat(S, 1, 1), xv.cpu().repeat(S, 1, 1),
                                   mk.cpu().repeat(S, 1))
        for name, o, l in (("SIMPLE_H3", out[0], ll[0]), ("SIMPLE", out[1], ll[1])):
            errs = {"y_coords": H.rel_err(o[0].cpu()[:, :, keep_c], ref[0][:, :, keep_c]), "y_velocs": H.rel_err(o[1].cpu()[:, :, keep_c], ref[1][:, :, keep_c]),
                    "logp": H.rel_err(o[2].cpu(), ref[2]), "loglik back": H.rel_err(l.cpu(), ref_ll)}
            print(f"\nsize sweep vs oracle | {variant} | {V} atoms x {S} rows | {name} | " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
            assert max(errs.values()) < TOL, (variant, V, S, name, errs)
    H.assert_not_demoted(m5)


@pytest.mark.parametrize("path", [0, 5, -1], ids=["exact-f32", "split-fp16-linears", "model-default"])
def test_per_op_path_large_molecules(path):
    """r06: `path` 5 = TW_PATH_SIMPLE_H3 (the per-op path with its linear layers as split-fp16 MFMA GEMMs) and -1 = what a model
    built without an explicit path takes at these sizes (the same) are held to the same bar as the exact-f32 per-op kernels.
    Above every fused layout (192 atoms) the flow runs on the per-op path.  r04 stopped at ~200 atoms there (one V x V score
    tile per molecule in the LDS) and refused anything larger; r05: the scores are computed row-wise and the mixing is a tiled
    f32-MFMA GEMM from 129 atoms on, so the reference's own 691-atom test protein size goes through - against the oracle at the
    bar, ragged (masked tails), forward and reverse.  The row-wise scores kernel must equal the tile kernel to one float ulp (150
    atoms fit both; r06: a wave per row, so the double sum of a row is added in another order).  The dense softmax variant's
    attention has a row-wise form too."""
    import ctypes as C

    from timewarp_amd import _lib

    lib = _lib.load()
    sd = H.full_kernel_sd()
    g = torch.Generator().manual_seed(77)
    m = H.tw_kernel_model(sd, path=path)
    assert path != -1 or m._path_for(256) == _lib.TW_PATH_SIMPLE_H3 == 5
    for V in ((256, 691) if path == -1 else (150, 256, 691)):   # (150 atoms: the model default is a fused layout)
        at = torch.randint(0, 5, (2, V), generator=g)
        x_c = torch.randn(2, V, 3, generator=g) * (0.8 if V < 300 else 1.5)
        x_v = torch.randn(2, V, 3, generator=g) * 0.5
        y_c = x_c + torch.randn(2, V, 3, generator=g) * 0.02
        y_v = torch.randn(2, V, 3, generator=g) * 0.5
        mask = torch.zeros(2, V, dtype=torch.bool)
        mask[1, V - 9:] = True
        out = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                               y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda())
        ref = fo.log_likelihood(sd, H.FULL_KERNEL_SPEC, at, x_c, x_v, y_c, y_v, mask)
        assert H.rel_err(out.cpu(), ref) < TOL, (V, H.rel_err(out.cpu(), ref))
        if V == 256:
            S = 3
            zc, zv = fo.draw_latents(sd, S, (1, V, 3), g)
            rs = fo.conditional_sample_with_logp(sd, H.FULL_KERNEL_SPEC, at[1:], x_c[1:], x_v[1:], mask[1:], zc, zv)
            got = m.conditional_sample_with_logp(atom_types=at[1:].cuda(), x_coords=x_c[1:].cuda(), x_velocs=x_v[1:].cuda(), adj_list=None,
                                                 edge_batch_idx=None, masked_elements=mask[1:].cuda(), num_samples=S,
                                                 z_coords=zc.cuda(), z_velocs=zv.cuda())
            keep = ~mask[1]
            assert H.rel_err(got[0].cpu()[:, :, keep], rs[0][:, :, keep]) < TOL and H.rel_err(got[1].cpu()[:, :, keep], rs[1][:, :, keep]) < TOL
            assert H.rel_err(got[2].cpu(), rs[2]) < TOL
    H.assert_not_demoted(m)
    if path == 5:
        # the FFN of this path is one launch of the fused kernels' chunk loop on the flat token list (the split-fp16 stream is at
        # hand for this model); PER_OP_UNFUSED: two GEMMs + add_ln instead - both at the bar
        # Route distinctness: a flag that silently took the default route would still pass at the bar, so each A/B output must also differ
        # from the output it is an alternative to.  All of these already hold at the commit before the route plan (691 atoms x 2 rows):
        # PER_OP_UNFUSED, FOLD_ONE_WG_PER_TILE, FOLD_GEMM_SEPARATE, IO_GEMM_PAIRS against the default, FOLD_LN_SEPARATE against
        # FOLD_ONE_WG_PER_TILE alone.
        with H.debug_flags(DebugFlag.PER_OP_UNFUSED):
            out2 = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                                    y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda())
        assert H.rel_err(out2.cpu(), ref) < TOL
        assert not torch.equal(out2, out)
        # FOLD_ONE_WG_PER_TILE: the folded GEMM inside ONE mixing workgroup per query tile also for this small launch (default below 400
        # workgroups: the heads over several workgroups per tile + a finishing launch; FOLD_GEMM_SEPARATE would take the per-head launches)
        with H.debug_flags(DebugFlag.FOLD_ONE_WG_PER_TILE):
            out3 = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                                    y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda())
        assert H.rel_err(out3.cpu(), ref) < TOL
        assert not torch.equal(out3, out)
        # ... and with residual + LayerNorm 1 as the add_ln launch behind it (FOLD_LN_SEPARATE) instead of in its epilogue
        with H.debug_flags(DebugFlag.FOLD_ONE_WG_PER_TILE | DebugFlag.FOLD_LN_SEPARATE):
            out4 = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                                    y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda())
        assert H.rel_err(out4.cpu(), ref) < TOL
        assert not torch.equal(out4, out3)
        # FOLD_GEMM_SEPARATE: per-head mixing launches + the folded GEMM + add_ln
        with H.debug_flags(DebugFlag.FOLD_GEMM_SEPARATE):
            out4b = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                                     y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda())
        assert H.rel_err(out4b.cpu(), ref) < TOL
        assert not torch.equal(out4b, out)
        # IO_GEMM_PAIRS: the in / out MLPs as two GEMMs each instead of one launch of the fused kernels' statements on the token list
        with H.debug_flags(DebugFlag.IO_GEMM_PAIRS):
            out5 = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                                    y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda())
        assert H.rel_err(out5.cpu(), ref) < TOL
        assert not torch.equal(out5, out)
        # the FFN launch on 48-token waves (TOKENS_NT3) and on 64-token waves (TOKENS_NT4; the default picks whichever needs fewer rounds'
        # worth of the chip): the same arithmetic per token.  This launch is small (691 atoms x 2 rows = 8 workgroups), so the default
        # also spreads the hidden layer over four workgroups per token tile (partial sums + a finishing launch; TOKENS_NT3: never)
        ffn = {}
        for bit in (DebugFlag.TOKENS_NT3, DebugFlag.TOKENS_NT4):
            with H.debug_flags(bit):
                ffn[bit] = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                                            y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda())
            assert H.rel_err(ffn[bit].cpu(), ref) < TOL, bit
        assert H.rel_err(ffn[DebugFlag.TOKENS_NT3].cpu(), out.cpu()) < 2e-6 and H.rel_err(ffn[DebugFlag.TOKENS_NT4].cpu(), out.cpu()) < 2e-6
        # the dense softmax variant above its fused layouts (65+ atoms): q / k / v and output projections, in / out MLPs on the
        # split-fp16 GEMMs, the FFN through the fused launches, the softmax attention itself in fp32
        dsd = H.full_dense_sd()
        md5 = H.tw_dense_model(dsd, path=5)
        gg = torch.Generator().manual_seed(5)
        V = 256
        at = torch.randint(0, 5, (2, V), generator=gg)
        xx = torch.randn(2, V, 3, generator=gg)
        yy = xx + torch.randn(2, V, 3, generator=gg) * 0.02
        vv = torch.randn(2, V, 3, generator=gg) * 0.5
        mk = torch.zeros(2, V, dtype=torch.bool)
        mk[1, V - 7:] = True
        outd = md5.log_likelihood(atom_types=at.cuda(), x_coords=xx.cuda(), x_velocs=vv.cuda(), y_coords=yy.cuda(), y_velocs=vv.cuda(),
                                  adj_list=None, edge_batch_idx=None, masked_elements=mk.cuda()).cpu()
        refd = fo.log_likelihood(dsd, H.FULL_DENSE_SPEC, at, xx, vv, yy, vv, mk)
        assert H.rel_err(outd, refd) < TOL, H.rel_err(outd, refd)
        with H.debug_flags(DebugFlag.IO_GEMM_PAIRS):
            outd2 = md5.log_likelihood(atom_types=at.cuda(), x_coords=xx.cuda(), x_velocs=vv.cuda(), y_coords=yy.cuda(), y_velocs=vv.cuda(),
                                       adj_list=None, edge_batch_idx=None, masked_elements=mk.cuda()).cpu()
        assert H.rel_err(outd2, refd) < TOL, H.rel_err(outd2, refd)
        # the softmax attention above 64 atoms runs on the fp32 matrix pipe (sdpa_mfma_kernel); SDPA_SCALAR: the scalar kernels - same bar,
        # on the exact-f32 per-op path too
        for pth in (5, SIMPLE):
            mdp = md5 if pth == 5 else H.tw_dense_model(dsd, path=SIMPLE)
            res = {}
            for flag in (0, DebugFlag.SDPA_SCALAR):
                with H.debug_flags(flag):
                    res[flag] = mdp.log_likelihood(atom_types=at.cuda(), x_coords=xx.cuda(), x_velocs=vv.cuda(), y_coords=yy.cuda(),
                                                   y_velocs=vv.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mk.cuda()).cpu()
                assert H.rel_err(res[flag], refd) < TOL, (pth, flag, H.rel_err(res[flag], refd))
        H.assert_not_demoted(md5)
    if path != 0:
        return
    # the two scores kernels on the same 150 atoms (PER_OP_ROWWISE forces the row-wise one), both cdist branches, Gaussian and Chebyshev:
    # the same values - the arithmetic of tw_cdist_mm / basis_value must not depend on the kernel it is inlined into
    V = 150
    x = torch.randn(1, V, 3, generator=g) * 0.8
    ls = torch.tensor([0.1, 0.2, 0.5, 0.7, 1.0, 1.2])
    coeffs = torch.randn(6, 7, generator=g) * 0.3
    xd, md, ld, cd = x.cuda(), torch.zeros(1, V, dtype=torch.uint8).cuda(), ls.cuda(), coeffs.cuda()
    for use_mm in (1, 0):
        outs = []
        for flags in (0, DebugFlag.PER_OP_ROWWISE):
            with H.debug_flags(flags):
                a, b = torch.empty(1, 6, V, V, device="cuda"), torch.empty(1, 6, V, V, device="cuda")
                _lib.check(lib.tw_kernel_scores(xd.data_ptr(), md.data_ptr(), ld.data_ptr(), 6, 1, V, 1, use_mm, a.data_ptr(), None), "tw_kernel_scores")
                _lib.check(lib.tw_kernel_scores_cheb(xd.data_ptr(), md.data_ptr(), ld.data_ptr(), cd.data_ptr(), 7, 1, 6, 1, V, 1, use_mm,
                                                     b.data_ptr(), None), "tw_kernel_scores_cheb")
                outs.append((a, b))
        # (the row sums are the same exact sums rounded once, added in another order in double: equal floats up to a rounding tie)
        for k in (0, 1):
            a, b = outs[0][k], outs[1][k]
            assert bool(((a - b).abs() <= 1.2e-7 * a.abs()).all()) and float((a != b).float().mean()) < 1e-3, (use_mm, k)
    # ... and the whole flow with the tiled kernels forced at a size the tile kernels take too
    at = torch.randint(0, 5, (3, 100), generator=g)
    xx = torch.randn(3, 100, 3, generator=g) * 0.7
    yy = xx + torch.randn(3, 100, 3, generator=g) * 0.02
    vv = torch.randn(3, 100, 3, generator=g) * 0.5
    mk = torch.zeros(3, 100, dtype=torch.bool)
    mk[2, 91:] = True
    ref = fo.log_likelihood(sd, H.FULL_KERNEL_SPEC, at, xx, vv, yy, vv, mk)
    for flags in (0, DebugFlag.PER_OP_ROWWISE):
        with H.debug_flags(flags):
            out = H.tw_kernel_model(sd, path=SIMPLE).log_likelihood(atom_types=at.cuda(), x_coords=xx.cuda(), x_velocs=vv.cuda(), y_coords=yy.cuda(),
                                                                     y_velocs=vv.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mk.cuda())
            assert H.rel_err(out.cpu(), ref) < TOL, (flags, H.rel_err(out.cpu(), ref))
    # dense softmax variant (r05: row-wise attention without a V x V tile in the LDS): 256 atoms against the oracle, and the
    # row-wise kernel bit-identical to the tile kernel where both run (PER_OP_ROWWISE forces it)
    dsd = H.full_dense_sd()
    md_ = H.tw_dense_model(dsd, path=0)
    for V, flags in ((256, 0), (40, 0), (40, DebugFlag.PER_OP_ROWWISE)):
        gg = torch.Generator().manual_seed(5)
        at = torch.randint(0, 5, (2, V), generator=gg)
        xx = torch.randn(2, V, 3, generator=gg)
        yy = xx + torch.randn(2, V, 3, generator=gg) * 0.02
        vv = torch.randn(2, V, 3, generator=gg) * 0.5
        mk = torch.zeros(2, V, dtype=torch.bool)
        mk[1, V - 7:] = True
        with H.debug_flags(flags):
            out = md_.log_likelihood(atom_types=at.cuda(), x_coords=xx.cuda(), x_velocs=vv.cuda(), y_coords=yy.cuda(), y_velocs=vv.cuda(),
                                     adj_list=None, edge_batch_idx=None, masked_elements=mk.cuda()).cpu()
        if V == 256:
            ref = fo.log_likelihood(dsd, H.FULL_DENSE_SPEC, at, xx, vv, yy, vv, mk)
            assert H.rel_err(out, ref) < TOL, H.rel_err(out, ref)
        elif flags == 0:
            tile = out
        else:
            assert torch.equal(out, tile)


def test_per_op_error_between_fork_and_join_leaves_streams_usable():
    """An error return of the per-op path after its two-stream fork brings the side stream back first: the refused call must
    not leave the second net of a coupling layer running on the side stream into the caller's workspace.  A dense model with one
    head of width 80 runs on sdpa_kernel at 40 atoms (44 800 B of LDS); at 120 atoms the score tile needs 172 800 B > 160 KiB, the
    row-wise kernel serves heads up to 64 wide, and the library refuses with TW_ERR_INVALID - a host-side argument check in the
    first net of the first coupling layer, behind the fork; nothing on the device faults.  A second 40-atom pass on the same
    workspace and stream then equals the first bit for bit, and the device reports no error.
    This pins the contract; it does not reproduce the leak: the commit before the scoped fork passes it too, because this refusal
    happens to come before anything is queued on the side stream."""
    import ctypes as C

    from timewarp_amd import _lib
    from timewarp_amd.weights import DENSE, FlowDims

    lib = _lib.load()
    desc = FlowDims(variant=DENSE, n_coupling=1, n_layers=1, d_model=80, d_ff=32, d_hidden=32, d_emb=32, n_heads=1).to_desc()
    g = torch.Generator().manual_seed(11)
    raw = (torch.randn(lib.tw_flow_raw_floats(C.byref(desc)), generator=g) * 0.1).cuda()
    ws = torch.empty(lib.tw_flow_workspace_bytes(C.byref(desc), 1, 120), dtype=torch.uint8, device="cuda")   # serves 40 atoms too
    assert 0 < lib.tw_flow_workspace_bytes(C.byref(desc), 1, 40) <= ws.numel()
    stream = _lib.stream_ptr(ws.device)

    def inputs(V):
        return (torch.randint(0, 5, (1, V), generator=g).to(torch.int32).cuda(), torch.randn(1, V, 3, generator=g).cuda(),
                (torch.randn(1, V, 3, generator=g) * 0.5).cuda(), torch.zeros(1, V, dtype=torch.uint8).cuda(),
                (torch.randn(1, V, 3, generator=g) * 0.05).cuda(), (torch.randn(1, V, 3, generator=g) * 0.5).cuda())

    def flow_pass(V, at, xc, xv, mk, zc, zv):
        zc, zv, dlp = zc.clone(), zv.clone(), torch.zeros(1, device="cuda")
        rc = lib.tw_flow_pass(C.byref(desc), raw.data_ptr(), None, at.data_ptr(), xc.data_ptr(), xv.data_ptr(), mk.data_ptr(), 1,
                              zc.data_ptr(), zv.data_ptr(), dlp.data_ptr(), 1, V, 0, SIMPLE, ws.data_ptr(), ws.numel(), stream)
        return rc, torch.cat([zc.flatten(), zv.flatten(), dlp])

    small, large = inputs(40), inputs(120)
    rc, first = flow_pass(40, *small)
    assert rc == 0 and torch.isfinite(first).all(), lib.tw_last_error()
    rc, _ = flow_pass(120, *large)
    assert rc == -1 and lib.tw_last_error().decode() == "dense attention: head width 80 > 64 on the row-wise per-op kernel"   # TW_ERR_INVALID
    rc, second = flow_pass(40, *small)
    assert rc == 0 and torch.equal(first, second)
    torch.cuda.synchronize()   # raises if a launch on either stream failed


@pytest.mark.parametrize("path", [SIMPLE, FUSED, H3])
def test_empty_batch_and_zero_samples(path):
    """Empty inputs: B = 0 rows / num_samples = 0 return empty tensors of the right shapes without launching anything."""
    m = H.tw_kernel_model(H.full_kernel_sd(), path=path)
    z = lambda *s: torch.zeros(*s, device="cuda")
    ll = m.log_likelihood(atom_types=torch.zeros(0, 22, dtype=torch.int64, device="cuda"), x_coords=z(0, 22, 3), x_velocs=z(0, 22, 3),
                          y_coords=z(0, 22, 3), y_velocs=z(0, 22, 3), adj_list=None, edge_batch_idx=None,
                          masked_elements=torch.zeros(0, 22, dtype=torch.bool, device="cuda"))
    assert tuple(ll.shape) == (0,)
    d, _ = H.load("kernel_full_ad")
    yc, yv, lp = m.conditional_sample_with_logp(
        atom_types=d["atom_types"].cuda(), x_coords=d["x_coords"].cuda(), x_velocs=d["x_velocs"].cuda(), adj_list=None,
        edge_batch_idx=None, masked_elements=d["masked"].cuda(), num_samples=0)
    assert tuple(yc.shape) == (0, 1, 22, 3) and tuple(yv.shape) == (0, 1, 22, 3) and tuple(lp.shape) == (0, 1)


def _overflowing_sd():
    """Weights that push activations past the fp16 range: in_mlp output ~1e6-1e7, representable in fp32, not in fp16."""
    sd = {k: v.clone() for k, v in H.full_kernel_sd().items()}
    for k in sd:
        if k.endswith("in_mlp._layers.2.weight"):
            sd[k] *= 1.0e7
    return sd


def test_split_fp16_overflow_demotes_to_f32():
    """A checkpoint whose activations leave the fp16 range: the split-fp16 path neither returns NaN log-densities nor
    raises - the call notices (tw_flow_nonfinite), the model moves to the exact-f32 kernels with one warning and the
    call is redone there, so its result IS the f32 kernel's.  Inside `deferred_range_check()` (what the MH loops use)
    nothing synchronises and `check_finite` is the raising form of the same flag."""
    from timewarp_amd import _lib

    sd = _overflowing_sd()
    d, _ = H.load("kernel_full_ad")
    args = dict(atom_types=d["atom_types"].cuda(), x_coords=d["x_coords"].cuda(), x_velocs=d["x_velocs"].cuda(),
                y_coords=d["y_coords"].cuda(), y_velocs=d["y_velocs"].cuda(), adj_list=None, edge_batch_idx=None,
                masked_elements=d["masked"].cuda())
    m32 = H.tw_kernel_model(sd, path=FUSED)
    ref = m32.log_likelihood(**args)
    assert torch.isfinite(ref).all()
    m32.check_finite()
    m = H.tw_kernel_model(sd, path=H3)
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        out = m.log_likelihood(**args)
    assert m.demoted and m.execution_path == _lib.TW_PATH_AUTO and torch.equal(out, ref)
    S = 8
    sargs = dict(atom_types=args["atom_types"], x_coords=args["x_coords"], x_velocs=args["x_velocs"], adj_list=None,
                 edge_batch_idx=None, masked_elements=args["masked_elements"], num_samples=S,
                 z_coords=d["z_coords"][:S].cuda(), z_velocs=d["z_velocs"][:S].cuda())
    m = H.tw_kernel_model(sd, path=None)  # the constructor's default: split-fp16 where it applies
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        got = m.conditional_sample_with_logp(**sargs)
    for a, b in zip(got, m32.conditional_sample_with_logp(**sargs)):
        assert torch.equal(a, b)
    # deferred: the caller looks at the flag itself
    m = H.tw_kernel_model(sd, path=H3)
    with m.deferred_range_check():
        m.log_likelihood(**args)
    assert not m.demoted
    with pytest.raises(RuntimeError, match="fp16 range"):
        m.check_finite()
    m.check_finite()  # the flag was reset by the failing check
    good = H.tw_kernel_model(H.full_kernel_sd(), path=H3)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        good.log_likelihood(**args)
    assert not good.demoted
    good.check_finite()


def test_range_guard_is_per_model_not_per_device():
    """ABI 7 (tw_flow_desc.range_flag): two models on one device, only one of which overflows, both inside
    `deferred_range_check()` so that nobody looks at a flag between the calls.  With the per-device word of ABI 6 whoever
    asked first saw - and cleared - the other model's overflow: the good model was demoted and the bad one sampled on."""
    import ctypes as C
    import warnings

    from timewarp_amd import _lib

    d, _ = H.load("kernel_full_ad")
    args = dict(atom_types=d["atom_types"].cuda(), x_coords=d["x_coords"].cuda(), x_velocs=d["x_velocs"].cuda(),
                y_coords=d["y_coords"].cuda(), y_velocs=d["y_velocs"].cuda(), adj_list=None, edge_batch_idx=None,
                masked_elements=d["masked"].cuda())
    bad = H.tw_kernel_model(_overflowing_sd(), path=H3)
    good = H.tw_kernel_model(H.full_kernel_sd(), path=H3)
    with bad.deferred_range_check(), good.deferred_range_check():
        bad.log_likelihood(**args)
        good.log_likelihood(**args)
    # the good model asks first
    assert not good.split_fp16_overflowed(torch.device("cuda", 0))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        good.check_finite()
        good.log_likelihood(**args)
    assert not good.demoted
    assert bad.split_fp16_overflowed(torch.device("cuda", 0))          # ... and the bad one still finds its own overflow
    assert not bad.split_fp16_overflowed(torch.device("cuda", 0))      # read and cleared
    # the per-device word (descriptors without a flag: raw C-ABI callers) saw none of it
    flag = C.c_int32(7)
    _lib.check(_lib.load().tw_flow_nonfinite(1, C.byref(flag)), "tw_flow_nonfinite")
    assert flag.value == 0
    # ... and still works for them: the same call through a descriptor with range_flag = NULL
    desc = bad.dims.to_desc()
    assert not desc.range_flag
    raw, packed = bad._weights(torch.device("cuda", 0), H3)
    B, V = args["x_coords"].shape[:2]
    ws = bad._ws(torch.device("cuda", 0), B, V)
    out = torch.empty(B, dtype=torch.float32, device="cuda")
    at, mk, xc, xv, yc, yv = bad._prep(args["atom_types"], args["masked_elements"], args["x_coords"], args["x_velocs"],
                                       args["y_coords"], args["y_velocs"])
    _lib.check(_lib.load().tw_flow_log_likelihood(C.byref(desc), raw.data_ptr(), _lib.ptr(packed), at.data_ptr(), xc.data_ptr(),
                                                  xv.data_ptr(), yc.data_ptr(), yv.data_ptr(), mk.data_ptr(), out.data_ptr(), B, V, H3,
                                                  ws.data_ptr(), ws.numel(), _lib.stream_ptr(torch.device("cuda", 0))),
               "tw_flow_log_likelihood")
    torch.cuda.synchronize()
    _lib.check(_lib.load().tw_flow_nonfinite(1, C.byref(flag)), "tw_flow_nonfinite")
    assert flag.value == 1
    assert not bad.split_fp16_overflowed(torch.device("cuda", 0))      # the model's own word was not involved


@pytest.mark.parametrize("path", [FUSED, H3])
def test_full_size_S1000_rows_vs_oracle(path):
    """BASELINE size (S = 1000 proposals, 22 atoms, 125 workgroups per coupling net) on both fused kernels - the
    split-fp16 one is bench.py's default.  (1) 48 rows spread over the launch - all 8 rows of the first, the middle and
    the last workgroup of each net, 24 random ones in between - against the oracle: proposals, velocities, log p(y|x),
    and the reverse-move density log p(x~|y~) of those same rows (per-row conditioning, forward pass).  (2) all 1000
    rows: the size-independent round trip - pushing (y, v) back through the density direction recovers log p."""
    sd = H.full_kernel_sd()
    m = H.tw_kernel_model(sd, path=path)
    d, _ = H.load("kernel_full_ad")
    S = 1000
    g = torch.Generator().manual_seed(5)
    zc, zv = fo.draw_latents(sd, S, (1, 22, 3), g)
    at, xc, xv, mk = d["atom_types"].cuda(), d["x_coords"].cuda(), d["x_velocs"].cuda(), d["masked"].cuda()
    yc, yv, lp = m.conditional_sample_with_logp(atom_types=at, x_coords=xc, x_velocs=xv, adj_list=None,
                                                edge_batch_idx=None, masked_elements=mk, num_samples=S,
                                                z_coords=zc.cuda(), z_velocs=zv.cuda())
    ll = m.log_likelihood(atom_types=at.repeat(S, 1), x_coords=xc.repeat(S, 1, 1), x_velocs=xv.repeat(S, 1, 1),
                          y_coords=yc.squeeze(1), y_velocs=yv.squeeze(1), adj_list=None, edge_batch_idx=None,
                          masked_elements=mk.repeat(S, 1))
    assert torch.isfinite(lp).all() and torch.isfinite(ll).all()
    H.assert_not_demoted(m)
    assert H.rel_err(ll.cpu(), lp.squeeze(1).cpu()) < TOL
    # reverse-move density of every row (velocities negated, evaluation_utils.py:648-657)
    p_yx = m.log_likelihood(atom_types=at.repeat(S, 1), x_coords=yc.squeeze(1), x_velocs=-yv.squeeze(1),
                            y_coords=xc.repeat(S, 1, 1), y_velocs=-xv.repeat(S, 1, 1), adj_list=None,
                            edge_batch_idx=None, masked_elements=mk.repeat(S, 1)).cpu()
    rows = list(range(0, 8)) + list(range(496, 504)) + list(range(992, 1000))
    rest = [r for r in torch.randperm(S, generator=g).tolist() if r not in rows][:24]
    rows = torch.tensor(sorted(rows + rest))
    assert len(rows) == 48
    ryc, ryv, rlp = fo.conditional_sample_with_logp(sd, H.FULL_KERNEL_SPEC, d["atom_types"], d["x_coords"],
                                                    d["x_velocs"], d["masked"], zc[rows], zv[rows])
    assert H.rel_err(yc.cpu()[rows], ryc) < TOL and H.rel_err(yv.cpu()[rows], ryv) < TOL
    assert H.rel_err(lp.cpu()[rows], rlp) < TOL and H.elem_rel_err(lp.cpu()[rows], rlp) < TOL
    n = len(rows)
    r_yx = fo.log_likelihood(sd, H.FULL_KERNEL_SPEC, d["atom_types"].repeat(n, 1), ryc.squeeze(1), -ryv.squeeze(1),
                             d["x_coords"].repeat(n, 1, 1), -d["x_velocs"].repeat(n, 1, 1), d["masked"].repeat(n, 1))
    assert H.rel_err(p_yx[rows], r_yx) < TOL and H.elem_rel_err(p_yx[rows], r_yx) < TOL


@pytest.mark.parametrize("path", [FUSED, H3])
def test_full_size_v60_S512_rows_vs_oracle(path):
    """BASELINE config 3 at full size: 60 atoms, 512 proposals on the fused f32 kernel (64-token waves, 1024 waves = one
    round of the chip) and on the split-fp16 kernel's wide layout (three molecules per workgroup, 171 workgroups per net).  40 rows spread over the launch - the 4 rows of the first, a middle and the last workgroup of each
    net, 28 random ones - against the oracle: proposals, velocities, log p(y|x) and the reverse-move density; and all 512
    rows through the size-independent round trip.  1e-5 since r04 (r03: 2e-5; the scores now follow torch.cdist's rounding
    sequence, tw_cdist_mm)."""
    tol = TOL
    sd = H.full_kernel_sd()
    m = H.tw_kernel_model(sd, path=path)
    d, _ = H.load("kernel_full_v60")
    V = d["x_coords"].shape[1]
    assert V == 60
    S = 512
    g = torch.Generator().manual_seed(11)
    zc, zv = fo.draw_latents(sd, S, (1, V, 3), g)
    at, xc, xv, mk = d["atom_types"].cuda(), d["x_coords"].cuda(), d["x_velocs"].cuda(), d["masked"].cuda()
    yc, yv, lp = m.conditional_sample_with_logp(atom_types=at, x_coords=xc, x_velocs=xv, adj_list=None,
                                                edge_batch_idx=None, masked_elements=mk, num_samples=S,
                                                z_coords=zc.cuda(), z_velocs=zv.cuda())
    ll = m.log_likelihood(atom_types=at.repeat(S, 1), x_coords=xc.repeat(S, 1, 1), x_velocs=xv.repeat(S, 1, 1),
                          y_coords=yc.squeeze(1), y_velocs=yv.squeeze(1), adj_list=None, edge_batch_idx=None,
                          masked_elements=mk.repeat(S, 1))
    assert torch.isfinite(lp).all() and torch.isfinite(ll).all()
    assert H.rel_err(ll.cpu(), lp.squeeze(1).cpu()) < tol
    p_yx = m.log_likelihood(atom_types=at.repeat(S, 1), x_coords=yc.squeeze(1), x_velocs=-yv.squeeze(1),
                            y_coords=xc.repeat(S, 1, 1), y_velocs=-xv.repeat(S, 1, 1), adj_list=None,
                            edge_batch_idx=None, masked_elements=mk.repeat(S, 1)).cpu()
    rows = list(range(0, 4)) + list(range(256, 260)) + list(range(508, 512))
    rest = [r for r in torch.randperm(S, generator=g).tolist() if r not in rows][:28]
    rows = torch.tensor(sorted(rows + rest))
    assert len(rows) == 40
    ryc, ryv, rlp = fo.conditional_sample_with_logp(sd, H.FULL_KERNEL_SPEC, d["atom_types"], d["x_coords"],
                                                    d["x_velocs"], d["masked"], zc[rows], zv[rows])
    assert H.rel_err(yc.cpu()[rows], ryc) < tol and H.rel_err(yv.cpu()[rows], ryv) < tol
    assert H.rel_err(lp.cpu()[rows], rlp) < tol and H.elem_rel_err(lp.cpu()[rows], rlp) < tol
    n = len(rows)
    # The reverse-move density as a FUNCTION: the oracle evaluated at the kernel's own proposals, element-wise at the bar.
    g_yx = fo.log_likelihood(sd, H.FULL_KERNEL_SPEC, d["atom_types"].repeat(n, 1), yc.cpu()[rows].squeeze(1), -yv.cpu()[rows].squeeze(1),
                             d["x_coords"].repeat(n, 1, 1), -d["x_velocs"].repeat(n, 1, 1), d["masked"].repeat(n, 1))
    assert H.rel_err(p_yx[rows], g_yx) < tol and H.elem_rel_err(p_yx[rows], g_yx) < tol, H.elem_rel_err(p_yx[rows], g_yx)
    # ... and as a CHAIN (kernel's proposals -> kernel's density against oracle's proposals -> oracle's density): relative to
    # the tensor's scale at the bar; element-wise this is two evaluations at inputs that differ by the proposals' own
    # 2-3e-6, and this un-calibrated 60-atom model turns a 1e-6 perturbation of y into 1.9e-5 of log p(x|y) in fp64
    # arithmetic (tools/v60_conditioning.py, profiles/r05_v60_conditioning.txt: condition number ~19; the fp32 oracle's own
    # chain is 2.9e-6 from the fp64 one) - so element-wise the chain is held to 2e-5 (r05: the encoder-stack statement of the
    # 64-token build measured 1.02e-5, its per-section build passed at 1e-5; r04's 1e-5 here had no margin over that noise).
    r_yx = fo.log_likelihood(sd, H.FULL_KERNEL_SPEC, d["atom_types"].repeat(n, 1), ryc.squeeze(1), -ryv.squeeze(1),
                             d["x_coords"].repeat(n, 1, 1), -d["x_velocs"].repeat(n, 1, 1), d["masked"].repeat(n, 1))
    assert H.rel_err(p_yx[rows], r_yx) < tol and H.elem_rel_err(p_yx[rows], r_yx) < 2e-5, H.elem_rel_err(p_yx[rows], r_yx)
    if path == H3:
        # the 2e-5 above must not hide a divergence of the PRODUCT build (encoder-stack statement) from its own
        # per-section build (DebugFlag.PER_SECTION): same latents -> same proposals, same inputs -> same density
        with H.debug_flags(DebugFlag.PER_SECTION):
            yc2, yv2, lp2 = m.conditional_sample_with_logp(atom_types=at, x_coords=xc, x_velocs=xv, adj_list=None,
                                                            edge_batch_idx=None, masked_elements=mk, num_samples=S,
                                                            z_coords=zc.cuda(), z_velocs=zv.cuda())
            p_yx2 = m.log_likelihood(atom_types=at.repeat(S, 1), x_coords=yc.squeeze(1), x_velocs=-yv.squeeze(1),
                                     y_coords=xc.repeat(S, 1, 1), y_velocs=-xv.repeat(S, 1, 1), adj_list=None,
                                     edge_batch_idx=None, masked_elements=mk.repeat(S, 1)).cpu()
        # (measured r06: proposals 3.9e-6 of the tensor's scale apart - each build is 2-3e-6 from the oracle with its own
        # rounding sequence, e.g. the residual folded into the accumulators' start values; the density at the SAME inputs,
        # element-wise, stays inside the 1e-5 bar that the 2e-5 above relaxes for the chained comparison)
        assert H.rel_err(yc2.cpu(), yc.cpu()) < 6e-6 and H.rel_err(lp2.cpu(), lp.cpu()) < 6e-6, (H.rel_err(yc2.cpu(), yc.cpu()), H.rel_err(lp2.cpu(), lp.cpu()))
        assert H.elem_rel_err(p_yx2, p_yx) < 1e-5, H.elem_rel_err(p_yx2, p_yx)


@pytest.mark.parametrize("n_coupling,pos_mod2", [(2, 0), (2, 1), (4, 1), (6, 0)])
def test_other_layer_counts_and_velocity_first_flows(n_coupling, pos_mod2):
    """Coupling-layer counts (even, as the constructor demands) and `position_layer_index_mod_2` other than the shipped 8 / 0: the split-fp16 flow pass
    applies layer i's coupling update in layer i + 1's launch and ping-pongs both variables between the caller's buffers
    and workspace copies - where the results end up depends on the parity of both numbers.  Full-width nets (the fused
    kernels need d_model 128), one encoder layer each; all three paths against the oracle, both directions."""
    spec = fo.FlowSpec(variant="kernel", num_coupling_layers=n_coupling, num_transformer_layers=1,
                       position_layer_index_mod_2=pos_mod2)
    sd = fo.synth_state_dict(fo.make_template(spec), 3)
    d, _ = H.load("kernel_full_ad")
    at, xc, xv, mk = d["atom_types"], d["x_coords"], d["x_velocs"], d["masked"]
    zc, zv = d["z_coords"][:9], d["z_velocs"][:9]
    ref = fo.conditional_sample_with_logp(sd, spec, at, xc, xv, mk, zc, zv)
    ll_ref = fo.log_likelihood(sd, spec, at.repeat(9, 1), ref[0].squeeze(1), ref[1].squeeze(1), xc.repeat(9, 1, 1),
                               xv.repeat(9, 1, 1), mk.repeat(9, 1))
    for path in (SIMPLE, FUSED, H3):
        m = H.tw_kernel_model(sd, n_coupling=n_coupling, n_layers=1, path=path, pos_mod2=pos_mod2)
        got = m.conditional_sample_with_logp(atom_types=at.cuda(), x_coords=xc.cuda(), x_velocs=xv.cuda(), adj_list=None,
                                             edge_batch_idx=None, masked_elements=mk.cuda(), num_samples=9,
                                             z_coords=zc.cuda(), z_velocs=zv.cuda())
        for a, b in zip(got, ref):
            assert H.rel_err(a.cpu(), b) < TOL, (path, H.rel_err(a.cpu(), b))
        ll = m.log_likelihood(atom_types=at.repeat(9, 1).cuda(), x_coords=ref[0].squeeze(1).cuda(), x_velocs=ref[1].squeeze(1).cuda(),
                              y_coords=xc.repeat(9, 1, 1).cuda(), y_velocs=xv.repeat(9, 1, 1).cuda(), adj_list=None,
                              edge_batch_idx=None, masked_elements=mk.repeat(9, 1).cuda())
        assert H.rel_err(ll.cpu(), ll_ref) < TOL, (path, H.rel_err(ll.cpu(), ll_ref))
        H.assert_not_demoted(m)


def test_fused_equals_simple_large_batch():
    sd = H.full_kernel_sd()
    d, _ = H.load("kernel_full_ad")
    S = 131  # odd: partial last wave block AND a workgroup with idle waves
    g = torch.Generator().manual_seed(9)
    zc, zv = fo.draw_latents(sd, S, (1, 22, 3), g)
    outs = []
    for path in (FUSED, SIMPLE, H3):
        m = H.tw_kernel_model(sd, path=path)
        outs.append(m.conditional_sample_with_logp(
            atom_types=d["atom_types"].cuda(), x_coords=d["x_coords"].cuda(), x_velocs=d["x_velocs"].cuda(),
            adj_list=None, edge_batch_idx=None, masked_elements=d["masked"].cuda(), num_samples=S,
            z_coords=zc.cuda(), z_velocs=zv.cuda()))
        H.assert_not_demoted(m)
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert H.rel_err(a.cpu(), b.cpu()) < TOL


def test_no_cpu_fallback():
    m = H.tw_kernel_model(H.full_kernel_sd(), device="cpu")
    d, _ = H.load("kernel_full_ad")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.log_likelihood(atom_types=d["atom_types"], x_coords=d["x_coords"], x_velocs=d["x_velocs"],
                         y_coords=d["y_coords"], y_velocs=d["y_velocs"], adj_list=None, edge_batch_idx=None,
                         masked_elements=d["masked"])


@pytest.mark.parametrize("ff,hidden", [(32, 32), (64, 64), (96, 32), (512, 128)])
def test_small_feedforward_and_hidden_widths_vs_oracle(ff, hidden):
    """The chunked MLP sections run a software pipeline over 32-unit chunks (A(0) | A(c+1) B(c) ... | B(n-1)); the reference's
    configs have 64 (FFN) and 8 (in / out MLP) of them.  One, two and three chunks are the edge cases of that pipeline's
    prologue and epilogue: every fused path that claims the shape (`tw_flow_path_supported`) against the oracle, the parity
    paths at 1e-5, the fast mode at its own bar."""
    import ctypes as C
    from timewarp_amd import _lib

    spec = fo.FlowSpec(variant="kernel", num_transformer_layers=2, num_coupling_layers=2)
    sd = fo.synth_state_dict(fo.make_template(spec, dim_feedforward=ff, mlp_hidden=(hidden,)), 0)
    g = torch.Generator().manual_seed(ff + hidden)
    V, lens = 22, [22, 20, 22, 17, 22]
    B = len(lens)
    at = torch.randint(0, 5, (B, V), generator=g)
    x_c = torch.randn(B, V, 3, generator=g) * 0.3
    x_v = torch.randn(B, V, 3, generator=g) * 0.5
    y_c = x_c + torch.randn(B, V, 3, generator=g) * 0.02
    y_v = torch.randn(B, V, 3, generator=g) * 0.5
    mask = torch.zeros(B, V, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, n:] = True
    ref = fo.log_likelihood(sd, spec, at, x_c, x_v, y_c, y_v, mask)
    lib = _lib.load()
    ran = []
    for path, bar in ((FUSED, TOL), (H3, TOL), (4, 2e-3)):
        m = H.tw_kernel_model(sd, ff=ff, hidden=hidden, path=path, n_coupling=2, n_layers=2)
        desc = m.dims.to_desc()
        if lib.tw_flow_path_supported(C.byref(desc), V, path) != 1:
            continue
        out = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                               y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda()).cpu()
        H.assert_not_demoted(m)
        assert H.rel_err(out, ref) < bar, (path, H.rel_err(out, ref))
        ran.append(path)
    assert H3 in ran and 4 in ran, ran


def test_random_shapes_split_fp16_against_the_per_op_path():
    """Twenty-four seeded random shapes - atoms 1..192, 1..40 conformations, ragged padding, types at random - through the
    split-fp16 kernel (48-token waves, windowed and wide layouts as the launch code picks them) and through the per-op path
    (one plain kernel per reference op, any shape): log-likelihoods at 1e-5, and the fast mode within its bar of both.  Not an
    oracle test (the per-op path is held to the oracle elsewhere): a net for layout bugs at sizes no fixture happens to have."""
    import ctypes as C

    import numpy as np
    from timewarp_amd import _lib

    sd = H.full_kernel_sd()
    lib = _lib.load()
    models = {p: H.tw_kernel_model(sd, path=p) for p in (SIMPLE, H3, 4)}
    desc = models[H3].dims.to_desc()
    rng = np.random.default_rng(2024)
    done = 0
    sizes = []
    while done < 24:
        V = int(rng.integers(1, 193))
        if lib.tw_flow_path_supported(C.byref(desc), V, H3) != 1:
            continue
        B = int(rng.integers(1, 41 if V <= 64 else 9))
        g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
        at = torch.randint(0, 5, (B, V), generator=g)
        x_c = torch.randn(B, V, 3, generator=g) * (0.2 + 0.004 * V)
        x_v = torch.randn(B, V, 3, generator=g) * 0.5
        y_c = x_c + torch.randn(B, V, 3, generator=g) * 0.02
        y_v = torch.randn(B, V, 3, generator=g) * 0.5
        mask = torch.zeros(B, V, dtype=torch.bool)
        for b in range(B):
            n = int(rng.integers(max(1, V - 12), V + 1))
            mask[b, n:] = True
        mask[0] = False   # one full-length row
        out = {}
        for p, m in models.items():
            out[p] = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(),
                                      y_velocs=y_v.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda()).cpu()
            H.assert_not_demoted(m)
        assert torch.isfinite(out[SIMPLE]).all()
        e3, e1 = H.rel_err(out[H3], out[SIMPLE]), H.rel_err(out[4], out[SIMPLE])
        assert e3 < TOL, (V, B, e3)
        assert e1 < 1e-3, (V, B, e1)
        sizes.append((V, B))
        done += 1
    assert min(v for v, _ in sizes) <= 24 and max(v for v, _ in sizes) >= 161, sizes
    assert any(81 <= v <= 95 for v, _ in sizes) or any(65 <= v <= 96 for v, _ in sizes), sizes


def test_64_token_waves_chebyshev_kernel_and_reverse_pass():
    """The 64-token build with what the plain forward test does not touch: the chebyshev_kernel model (one score-fragment set
    per (net, layer): the fragment stride of four query tiles x 4 KiB enters the variant arithmetic) and the reverse pass
    (sampling) - 52 atoms, ragged, forced layout, against the oracle."""
    sd = H.full_cheb_sd()
    V, lens = 52, [52, 47, 52, 52, 52, 39]
    g = torch.Generator().manual_seed(4052)
    B = len(lens)
    at = torch.randint(0, 5, (B, V), generator=g)
    x_c = torch.randn(B, V, 3, generator=g) * 0.5
    x_v = torch.randn(B, V, 3, generator=g) * 0.5
    y_c = x_c + torch.randn(B, V, 3, generator=g) * 0.02
    y_v = torch.randn(B, V, 3, generator=g) * 0.5
    mask = torch.zeros(B, V, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, n:] = True
    ref = fo.log_likelihood(sd, H.FULL_CHEB_SPEC, at, x_c, x_v, y_c, y_v, mask)
    zc, zv = fo.draw_latents(sd, 1, (B, V, 3), g)
    ryc, ryv, rlp = fo.conditional_sample_with_logp(sd, H.FULL_CHEB_SPEC, at, x_c, x_v, mask, zc, zv)
    with H.debug_flags(DebugFlag.ALWAYS_NT4):
        m = H.tw_kernel_model(sd, path=H3, attention_type="chebyshev_kernel", cheb_order=6, force_asymptotic_zero=True)
        out = m.log_likelihood(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), y_coords=y_c.cuda(), y_velocs=y_v.cuda(),
                               adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda()).cpu()
        yc, yv, lp = m.conditional_sample_with_logp(atom_types=at.cuda(), x_coords=x_c.cuda(), x_velocs=x_v.cuda(), adj_list=None,
                                                    edge_batch_idx=None, masked_elements=mask.cuda(), num_samples=1,
                                                    z_coords=zc.cuda(), z_velocs=zv.cuda())
        H.assert_not_demoted(m)
    keep = ~mask
    assert H.rel_err(out, ref) < 2e-5, H.rel_err(out, ref)
    assert H.rel_err(lp.cpu(), rlp) < 2e-5
    # The sampled coordinates of this un-calibrated model on random 0.5 nm inputs are ill-conditioned in fp32: the oracle's own
    # fp32 run is 9.2e-5 from the same computation in fp64, and EVERY path (64-token, wide, f32 MFMA, per-op) sits 6e-5 from
    # fp64 and 9.2e-5 from the fp32 oracle.  So the bar is the noise floor itself: no further from fp64 than the fp32 oracle is.
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    eyc, eyv, _ = fo.conditional_sample_with_logp(sd64, H.FULL_CHEB_SPEC, at, x_c.double(), x_v.double(), mask, zc.double(), zv.double())
    floor_c = H.rel_err(ryc[0][keep], eyc[0][keep].float())
    floor_v = H.rel_err(ryv[0][keep], eyv[0][keep].float())
    assert H.rel_err(yc.cpu()[0][keep], eyc[0][keep].float()) < max(1.2 * floor_c, TOL), floor_c
    assert H.rel_err(yv.cpu()[0][keep], eyv[0][keep].float()) < max(1.2 * floor_v, TOL), floor_v


def test_mfma_stream_probe_entry_point():
    """tw_probe_mfma_clock (bench.py's roofline.power_bound): a bare v_mfma_f32_16x16x32_f16 stream costs ~16.8 cycles per
    instruction whatever the load; the clock it reports for one workgroup / the whole chip is a plausible gfx950 clock and the
    whole chip does not run faster than one CU."""
    import ctypes as C
    from timewarp_amd import _lib

    lib = _lib.load()
    torch.zeros(1, device="cuda")
    res = {}
    for wgs in (1, 256):
        cyc, ms = C.c_int64(0), C.c_double(0.0)
        assert lib.tw_probe_mfma_clock(wgs, 2048, C.byref(cyc), C.byref(ms), None) == 0
        per = cyc.value / (36.0 * 2048)
        ghz = cyc.value / (ms.value * 1e6)
        assert 16.0 <= per <= 18.0, per
        assert 1.0 < ghz < 2.7, ghz
        res[wgs] = ghz
    assert res[256] <= res[1] * 1.05, res
    assert lib.tw_probe_mfma_clock(0, 10, C.byref(cyc), C.byref(ms), None) != 0


def pack_stream_digests():
    """sha256 of every weight stream of a set of models, each packed once into a buffer pre-filled with 0xA5 (so bytes no
    packer writes hash the same every time).  The last 256 bytes of each split-fp16 / single-MFMA region are zeroed before
    hashing (the library built before the single-launch packer kept its scale search there); returns the digests and, per
    stream, whether those bytes came out of the packer zero."""
    import ctypes as C
    from timewarp_amd import _lib
    from timewarp_amd.weights import pack_raw

    lib = _lib.load()
    spec = fo.FlowSpec(variant="kernel", num_transformer_layers=1, num_coupling_layers=2)
    zero_sd = dict(H.full_kernel_sd())
    for k in ("flow.chain.0.scale_transformer.encoder_layers.1.linear2.weight",  # a plain matrix's scale search: m == 0
              "flow.chain.1.shift_transformer.encoder_layers.2.self_attn.values_proj.weight"):  # ... and a folded layer's
        zero_sd[k] = torch.zeros_like(zero_sd[k])
    all4 = ("f32", "h3", "h1", "simple_h3")
    models = [
        ("kernel", lambda: H.tw_kernel_model(H.full_kernel_sd(), path=None, device="cpu"), all4),
        ("cheb", lambda: H.tw_kernel_model(H.full_cheb_sd(), path=None, device="cpu", attention_type="chebyshev_kernel",
                                           cheb_order=6, force_asymptotic_zero=True), ("h3",)),
        ("dense", lambda: H.tw_dense_model(H.full_dense_sd(), path=None, device="cpu"), all4),
        ("dense_posenc", lambda: H.tw_dense_model(H.full_dense_posenc_sd(), rff_dim=128, path=None, device="cpu"),
         ("f32", "h3", "h1")),
        ("kernel_emb16", lambda: H.tw_kernel_model(fo.synth_state_dict(fo.make_template(spec, atom_embedding_dim=16), 0),
                                                   emb=16, n_coupling=2, n_layers=1, path=None, device="cpu"), all4),
        ("kernel_zero", lambda: H.tw_kernel_model(zero_sd, path=None, device="cpu"), ("f32", "h3", "h1")),
    ]
    entry = {"f32": ("tw_flow_packed_floats", "tw_flow_pack", 4), "h3": ("tw_flow_packed_h3_bytes", "tw_flow_pack_h3", 1),
             "h1": ("tw_flow_packed_h1_bytes", "tw_flow_pack_h1", 1),
             "simple_h3": ("tw_flow_packed_simple_h3_bytes", "tw_flow_pack_simple_h3", 1)}
    digests, tail_zero = {}, {}
    for name, make, streams in models:
        m = make()
        desc = m.dims.to_desc()
        raw = pack_raw(m.state_dict(), m.dims).cuda()
        for st in streams:
            size_fn, pack_fn, unit = entry[st]
            n = getattr(lib, size_fn)(C.byref(desc)) * unit
            assert n > 0, (name, st)
            buf = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
            _lib.check(getattr(lib, pack_fn)(C.byref(desc), raw.data_ptr(), buf.data_ptr(), None), pack_fn)
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            if st != "f32":
                end = (lib.tw_flow_packed_h1_bytes if st == "h1" else lib.tw_flow_packed_h3_bytes)(C.byref(desc))
                tail_zero[name, st] = not host[end - 256:end].any()
                host[end - 256:end] = 0
            digests[name, st] = hashlib.sha256(host.tobytes()).hexdigest()[:32]
    return digests, tail_zero


# recorded from the library as it was before the streams were built from one op table (one launch per tile)
PACK_DIGESTS = {
    ("kernel", "f32"): "b1658a492a98024ae3d29574d6b20be7",
    ("kernel", "h3"): "9f540fab049181f0f8224db565c49397",
    ("kernel", "h1"): "8239e36cfa0c006fcae3d5171ada8449",
    ("kernel", "simple_h3"): "6833fd919fd13000fe6815857afbfcd3",
    ("cheb", "h3"): "9f540fab049181f0f8224db565c49397",
    ("dense", "f32"): "5b174c141db8a137d804e7582788d86c",
    ("dense", "h3"): "9b542a2f373553ad7e184a14469c0871",
    ("dense", "h1"): "3cb759ee3a21a38141c60636122e860a",
    ("dense", "simple_h3"): "8517cdb905be171b769c94b61a4ee0cf",
    ("dense_posenc", "f32"): "393dbbebfeda29ef689a09c87750a0b4",
    ("dense_posenc", "h3"): "f643e0cdbe6aa9fa4b4032be61e1d814",
    ("dense_posenc", "h1"): "876e1fde96f117210e1e244f52e170ef",
    ("kernel_emb16", "f32"): "509697d328c2ed90fcb9a4b08cd6b6b1",
    ("kernel_emb16", "h3"): "8192e4241521d1e36fd3aed7f6291c7a",
    ("kernel_emb16", "h1"): "e17dccee401324a4333b4d23208956de",
    ("kernel_emb16", "simple_h3"): "f488a789942c08b8f63d0396a6c6a2fd",
    ("kernel_zero", "f32"): "31193bd23b30bcf30bad12ee714b70b1",
    ("kernel_zero", "h3"): "f3dfed101a5d444bb30c126206b0b07c",
    ("kernel_zero", "h1"): "dd9aa05d333e462358dc7481e3dad0cc",
}


def test_pack_streams_are_byte_identical():
    """Every weight stream (f32, split-fp16, single-MFMA, the per-op path's split-fp16 + folded Wc) of the kernel, chebyshev,
    dense and position-feature models, a narrower embedding and a model with all-zero matrices is byte for byte what the
    per-tile packer wrote; the split-fp16 streams' last 256 bytes are left zero (no scratch in the caller's buffer)."""
    digests, tail_zero = pack_stream_digests()
    assert digests == PACK_DIGESTS
    assert all(tail_zero.values()), tail_zero
