"""Local self-attention (attention_type "local") without a GPU: the CPU restatement against the reference's own vectors
(tests/golden/local_*.npz, tools/gen_local_golden.py), the product model's state dict, raw layout, path table and
descriptor checks, and the drop-in seam."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import flow_oracle as fo
from tests import helpers as H
from tests import local_flow_oracle as lo
from tests.test_integration_reference import REF as _REF, _import_reference

TINY_SPEC = lo.LocalFlowSpec(num_coupling_layers=2, num_transformer_layers=2, n_head=2, max_radius=0.8)
FULL_CASES = [("local_full_ad", 0.2), ("local_full_ad_r005", 0.05), ("local_full_ad_r100", 1.0)]
TOL = 2e-6


def _local_model(sd=None, **kw):
    import timewarp_amd as tw
    from timewarp_amd import synthetic

    cfg = synthetic.local_transformer_nvp_config()
    enc = cfg.custom_transformer_nvp_config.encoder_layer_config
    for k, v in kw.items():
        setattr(enc, k, v)
    m = tw.model_constructor(cfg)
    if sd is not None:
        m.load_state_dict(sd)
    return m


def _check_case(d, sd, spec, prefix=""):
    g = lambda k: d[prefix + k]
    ll = lo.log_likelihood(sd, spec, g("atom_types"), g("x_coords"), g("x_velocs"), g("y_coords"), g("y_velocs"), g("masked"))
    assert H.rel_err(ll, g("loglik")) < TOL, ("loglik", H.rel_err(ll, g("loglik")))
    if prefix + "z_coords" not in d:
        return
    yc, yv, lp = lo.conditional_sample_with_logp(sd, spec, g("atom_types"), g("x_coords"), g("x_velocs"), g("masked"),
                                                 g("z_coords"), g("z_velocs"))
    keep = ~g("masked")[0]
    for name, got in (("s_y_coords", yc), ("s_y_velocs", yv)):
        e = H.rel_err(got[:, :, keep], g(name)[:, :, keep])
        assert e < TOL, (name, e)
    assert H.rel_err(lp, g("s_logp")) < TOL, ("s_logp", H.rel_err(lp, g("s_logp")))
    S = g("z_coords").shape[0]
    gy, gv = g("s_y_coords").squeeze(1), g("s_y_velocs").squeeze(1)
    lyx = lo.log_likelihood(sd, spec, g("atom_types").repeat(S, 1), gy, -gv, g("x_coords").repeat(S, 1, 1),
                            -g("x_velocs").repeat(S, 1, 1), g("masked").repeat(S, 1))
    assert H.rel_err(lyx, g("logp_yx")) < TOL, ("logp_yx", H.rel_err(lyx, g("logp_yx")))


def test_tiny_golden_is_not_degenerate():
    d, _ = H.load("local_tiny")
    for k, m in (("counts", d["masked"]), ("b1_counts", d["b1_masked"])):
        c, real = d[k], ~m
        assert int(c[~real].max()) == 0 and int(c[real].min()) >= 1   # masked atoms have no neighbours, real ones themselves
        assert int(c[real].max()) > 1
    c, real = d["counts"], ~d["masked"]
    assert int(c[real].min()) == 1                                       # an isolated atom: only itself
    sizes = real.sum(-1)
    assert any(int(c[b].max()) == int(sizes[b]) for b in range(c.shape[0]))   # an atom whose radius covers its molecule


def test_restatement_matches_tiny_golden():
    d, sd = H.load("local_tiny")
    _check_case(d, sd, TINY_SPEC)
    _check_case(d, sd, TINY_SPEC, "b1_")


@pytest.mark.parametrize("name,radius", FULL_CASES)
def test_restatement_matches_full_ad_goldens(name, radius):
    d, _ = H.load(name)
    sd = fo.synth_state_dict(_local_model(max_radius=radius).state_dict(), 0)
    spec = lo.LocalFlowSpec(max_radius=radius)
    _check_case(d, sd, spec)
    c = d["counts"]
    expect = {0.2: (2, 5), 0.05: (1, 1), 1.0: (22, 22)}[radius]
    assert (int(c.min()), int(c.max())) == expect


def test_restatement_layer_trace():
    d, _ = H.load("local_full_ad")
    sd = fo.synth_state_dict(_local_model().state_dict(), 0)
    spec = lo.LocalFlowSpec()
    xc = d["x_coords"] - fo.centre_of_mass(d["x_coords"], d["masked"])
    S = 2
    feats = torch.nn.functional.embedding(d["atom_types"], sd["flow.atom_embedder.weight"]).repeat(S, 1, 1)
    # chain[7] transforms velocities: the other input is the coordinate latent
    u = torch.cat([feats, xc.repeat(S, 1, 1), d["x_velocs"].repeat(S, 1, 1), d["z_coords"][:S, 0]], -1)
    trace = []
    lo.local_netblock(sd, "flow.chain.7.scale_transformer", u, spec, xc.repeat(S, 1, 1), d["masked"].repeat(S, 1), trace)
    for (name, got), key in zip(trace, ["tr_in_mlp", "tr_enc0", "tr_enc1", "tr_enc2", "tr_out_mlp"]):
        assert H.rel_err(got, d[key]) < TOL, (key, H.rel_err(got, d[key]))


def test_full_radius_is_unrestricted_softmax():
    """At 1.0 nm every alanine-dipeptide atom sees all 22: local attention is plain softmax attention there."""
    g = torch.Generator().manual_seed(3)
    h = torch.randn(2, 22, 8, generator=g)
    d, _ = H.load("local_full_ad_r100")
    pos = (d["x_coords"] - fo.centre_of_mass(d["x_coords"], d["masked"])).repeat(2, 1, 1)
    sd = {"a.qkv_proj.weight": torch.randn(3 * 2 * 8, 8, generator=g), "a.output_proj.weight": torch.randn(8, 16, generator=g)}
    got = lo.local_self_attention(sd, "a", h, pos, torch.zeros(2, 22, dtype=torch.bool), 2, 1.0)
    qkv = (h @ sd["a.qkv_proj.weight"].T).reshape(2, 22, 2, 24)
    q, k, v = qkv[..., :8], qkv[..., 8:16], qkv[..., 16:]
    att = torch.softmax(torch.einsum("bqhf,bkhf->bhqk", q, k) / 8 ** 0.5, -1)
    want = torch.einsum("bhqk,bkhf->bqhf", att, v).reshape(2, 22, 16) @ sd["a.output_proj.weight"].T
    assert H.rel_err(got, want) < 1e-6


def test_state_dict_matches_reference_keys_and_shapes():
    _, tiny_sd = H.load("local_tiny")
    import timewarp_amd as tw

    cfg = tw.ModelConfig("custom_attention_transformer_nvp", custom_transformer_nvp_config=tw.CustomAttentionTransformerNVPConfig(
        4, [8], 2, 2, tw.CustomAttentionEncoderLayerConfig(d_model=8, dim_feedforward=16, dropout=0.0, num_heads=2,
                                                           attention_type="local", max_radius=0.8)))
    tiny = tw.model_constructor(cfg)
    got = {k: tuple(v.shape) for k, v in tiny.state_dict().items()}
    assert got == {k: tuple(v.shape) for k, v in tiny_sd.items()}
    tiny.load_state_dict({"module." + k: v for k, v in tiny_sd.items()})   # DeepSpeed-style prefix accepted
    assert torch.equal(tiny.state_dict()["flow.chain.1.shift_transformer.encoder_layers.1.self_attn.qkv_proj.weight"],
                       tiny_sd["flow.chain.1.shift_transformer.encoder_layers.1.self_attn.qkv_proj.weight"])
    full = _local_model().state_dict()
    z = np.load(os.path.join(H.GOLDEN, "local_full_ad.npz"))
    ref = {str(k): tuple(int(s) for s in shp[: max(1, (shp > 0).sum())]) if shp.any() else () for k, shp in zip(z["sd_keys"], z["sd_shapes"])}
    assert {k: tuple(v.shape) for k, v in full.items()} == ref
    assert len(full) == 611 and sum(v.numel() for v in full.values()) == 51_634_306


def test_raw_layout_agrees_with_library():
    from timewarp_amd import _lib, weights

    lib = _lib.load()
    for m in (_local_model(), _local_model(num_heads=3, max_radius=0.5)):
        desc = m.dims.to_desc()
        assert m.dims.variant == weights.LOCAL
        assert lib.tw_flow_raw_floats(C.byref(desc)) == weights.raw_numel(m.dims)
        raw = weights.pack_raw(m.state_dict(), m.dims)
        assert raw.numel() == weights.raw_numel(m.dims)
        keys = [k for k, _ in weights.raw_entries(m.dims)]
        assert weights.LENGTHSCALES not in keys
        assert "flow.chain.0.scale_transformer.encoder_layers.0.self_attn.qkv_proj.weight" in keys


def test_paths_and_packs():
    from timewarp_amd import _lib
    from timewarp_amd.modules.flow import PREFER_SPLIT_FP16

    lib = _lib.load()
    m = _local_model()
    desc = m.dims.to_desc()
    for V in (1, 22, 48, 64, 192, 691):
        got = [lib.tw_flow_path_supported(C.byref(desc), V, p) for p in range(6)]
        assert got == [1, 0, 1, 0, 0, 1], (V, got)
    for fn in ("tw_flow_packed_floats", "tw_flow_packed_h3_bytes", "tw_flow_packed_simple_h3_bytes", "tw_flow_packed_h1_bytes"):
        assert getattr(lib, fn)(C.byref(desc)) == 0, fn
    for fn in ("tw_flow_pack", "tw_flow_pack_h3", "tw_flow_pack_simple_h3", "tw_flow_pack_h1"):
        assert getattr(lib, fn)(C.byref(desc), None, None, None) == -1, fn   # TW_ERR_INVALID
    m.execution_path = PREFER_SPLIT_FP16
    assert m._path_for(22) == _lib.TW_PATH_SIMPLE_H3 and m._path_for(691) == _lib.TW_PATH_SIMPLE_H3
    # the neighbour structure at its worst case is part of the scratch the flow entry points ask for
    small = lib.tw_flow_workspace_bytes(C.byref(desc), 16, 691)
    assert small >= 2 * 16 * 691 * 691 * 4


def test_execution_path_defaults(monkeypatch):
    from timewarp_amd import _lib
    from timewarp_amd.modules.flow import PREFER_SPLIT_FP16

    monkeypatch.delenv("TW_EXECUTION_PATH", raising=False)
    m = _local_model()
    assert m.execution_path == PREFER_SPLIT_FP16 and m._path_for(22) == _lib.TW_PATH_SIMPLE_H3
    for name in ("f32", "auto"):
        monkeypatch.setenv("TW_EXECUTION_PATH", name)
        m = _local_model()
        assert m._path_for(22) == _lib.TW_PATH_SIMPLE and m._path_for(691) == _lib.TW_PATH_SIMPLE   # no fused layout exists


@pytest.mark.parametrize("bad", [0.0, -0.2, float("nan"), float("inf")])
def test_descriptor_rejects_bad_radius(bad):
    from timewarp_amd import _lib

    lib = _lib.load()
    desc = _local_model().dims.to_desc()
    desc.max_radius = bad
    assert lib.tw_flow_raw_floats(C.byref(desc)) == -1
    assert b"max_radius" in lib.tw_last_error()
    assert lib.tw_flow_workspace_bytes(C.byref(desc), 4, 22) == -1
    with pytest.raises((ValueError, AssertionError)):
        _local_model(max_radius=bad if bad == bad else None)


def test_descriptor_rejects_chebyshev_and_rff_fields():
    from timewarp_amd import _lib

    lib = _lib.load()
    for field in ("cheb_order", "d_rff"):
        desc = _local_model().dims.to_desc()
        setattr(desc, field, 2)
        assert lib.tw_flow_raw_floats(C.byref(desc)) == -1, field


def test_constructor_rules():
    with pytest.raises(NotImplementedError):
        _local_model(dropout=0.1)
    with pytest.raises(AssertionError):
        _local_model(max_radius=None)
    import timewarp_amd as tw
    from timewarp_amd import synthetic

    cfg = synthetic.local_transformer_nvp_config()
    cfg.custom_transformer_nvp_config.encoder_layer_config.attention_type = "no_such_attention"
    with pytest.raises(NotImplementedError):
        tw.model_constructor(cfg)


@pytest.mark.skipif(not os.path.isdir(_REF), reason="reference checkout not present")
def test_install_routes_local_config_to_this_package():

    _import_reference()
    import timewarp.model_constructor as ref_mc
    from timewarp.model_configs import CustomAttentionTransformerNVPConfig, ModelConfig
    from timewarp.modules.layers.custom_attention_encoder import CustomAttentionEncoderLayerConfig

    import timewarp_amd.integration as twi
    from timewarp_amd.modules.flow import ConditionalFlowDensityModel

    twi.install(replace_energy=False, replace_mh_loop=False)
    enc = CustomAttentionEncoderLayerConfig(d_model=128, dim_feedforward=2048, dropout=0.0, num_heads=8,
                                            attention_type="local", max_radius=0.2)
    cfg = ModelConfig(model_type="custom_attention_transformer_nvp",
                      custom_transformer_nvp_config=CustomAttentionTransformerNVPConfig(
                          atom_embedding_dim=16, latent_mlp_hidden_dims=[256], num_coupling_layers=8,
                          num_transformer_layers=3, encoder_layer_config=enc))
    model = ref_mc.model_constructor(cfg)
    assert isinstance(model, ConditionalFlowDensityModel)
    assert model.dims.max_radius == pytest.approx(0.2) and model.dims.n_heads == 8
    assert len(model.state_dict()) == 611
