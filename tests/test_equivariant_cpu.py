"""The E(3)-equivariant NVP flow (model_type "equivariant_nvp") without a GPU: the CPU restatement
(tests/equivariant_flow_oracle.py) against the reference's own vectors (tests/golden/equivariant_*.npz,
tools/gen_equivariant_golden.py), the product model's state dict, raw layout, path table and descriptor checks, the
drop-in seam, and the reference's rotation / translation property on the restatement."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import flow_oracle as fo
from tests import equivariant_flow_oracle as eo
from tests import helpers as H
from tests.test_integration_reference import REF as _REF, _import_reference

TOL = 2e-6   # the bar tests/test_local_attention_cpu.py sets for a restatement against the reference's vectors
TINY = [("equivariant_tiny", [8, 8], 0), ("equivariant_tiny_h1", [8], 0), ("equivariant_tiny_pm1", [8, 8], 1)]


def _model(emb=32, hidden=(256, 256), n_coupling=4, pos_mod=0, sd=None):
    import timewarp_amd as tw

    cfg = tw.ModelConfig("equivariant_nvp", equivariant_nvp_config=tw.EquivariantNVPConfig(
        atom_embedding_dim=emb, num_coupling_layers=n_coupling, latent_mlp_hidden_dims=list(hidden),
        position_layer_index_mod_2=pos_mod))
    m = tw.model_constructor(cfg)
    if sd is not None:
        m.load_state_dict(sd)
    return m


def _check_case(d, sd, spec, prefix=""):
    g = lambda k: d[prefix + k]
    ll = eo.log_likelihood(sd, spec, g("atom_types"), g("x_coords"), g("x_velocs"), g("y_coords"), g("y_velocs"), g("masked"))
    assert H.rel_err(ll, g("loglik")) < TOL, ("loglik", H.rel_err(ll, g("loglik")))
    if prefix + "z_coords" not in d:
        return
    yc, yv, lp = eo.conditional_sample_with_logp(sd, spec, g("atom_types"), g("x_coords"), g("x_velocs"), g("masked"),
                                                 g("z_coords"), g("z_velocs"))
    keep = ~g("masked")[0]
    for name, got in (("s_y_coords", yc), ("s_y_velocs", yv)):
        e = H.rel_err(got[:, :, keep], g(name)[:, :, keep])
        assert e < TOL, (name, e)
    assert H.rel_err(lp, g("s_logp")) < TOL, ("s_logp", H.rel_err(lp, g("s_logp")))
    S = g("z_coords").shape[0]
    gy, gv = g("s_y_coords").squeeze(1), g("s_y_velocs").squeeze(1)
    lyx = eo.log_likelihood(sd, spec, g("atom_types").repeat(S, 1), gy, -gv, g("x_coords").repeat(S, 1, 1),
                            -g("x_velocs").repeat(S, 1, 1), g("masked").repeat(S, 1))
    assert H.rel_err(lyx, g("logp_yx")) < TOL, ("logp_yx", H.rel_err(lyx, g("logp_yx")))


def _check_trace(d, sd, spec):
    """The modules of chain[0] and chain[1] on the inputs the reference's modules saw in its log_likelihood call."""
    n = d["tr0_z_other"].shape[0]
    feats = torch.nn.functional.embedding(d["atom_types"][:n], sd["flow.atom_embedder.weight"])
    for c in (0, 1):
        positions = c % 2 == spec.position_layer_index_mod_2
        args = (positions, feats, d[f"tr{c}_z_other"], d[f"tr{c}_x_coords"], d["x_velocs"][:n], d["masked"][:n])
        keep = ~d["masked"][:n]
        ls = eo.scale_module(sd, f"flow.chain.{c}.scale_module", *args)
        sh = eo.shift_module(sd, f"flow.chain.{c}.shift_module", *args)
        assert H.rel_err(ls[keep], d[f"tr{c}_log_scale"][keep]) < TOL, (c, "log_scale")
        assert H.rel_err(sh[keep], d[f"tr{c}_shift"][keep]) < TOL, (c, "shift")


@pytest.mark.parametrize("name,hidden,pos_mod", TINY)
def test_restatement_matches_tiny_goldens(name, hidden, pos_mod):
    d, sd = H.load(name)
    spec = eo.EquivariantFlowSpec(num_coupling_layers=2, position_layer_index_mod_2=pos_mod)
    _check_case(d, sd, spec)
    _check_case(d, sd, spec, "b1_")
    _check_trace(d, sd, spec)
    # the nets act: scales away from 1 and shifts away from 0 on the unmasked atoms
    keep = ~d["masked"]
    assert float(d["tr0_log_scale"][keep].abs().max()) > 1e-3 and float(d["tr1_shift"][keep].abs().max()) > 1e-4


def test_restatement_matches_full_ad_golden():
    d, _ = H.load("equivariant_full_ad")
    sd = fo.synth_state_dict(_model().state_dict(), 0)
    spec = eo.EquivariantFlowSpec()
    _check_case(d, sd, spec)
    _check_trace(d, sd, spec)


@pytest.mark.parametrize("name,hidden,pos_mod", TINY)
def test_state_dict_matches_reference_tiny(name, hidden, pos_mod):
    _, ref_sd = H.load(name)
    m = _model(emb=4, hidden=hidden, n_coupling=2, pos_mod=pos_mod)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in ref_sd.items()}
    m.load_state_dict({"module." + k: v for k, v in ref_sd.items()})   # DeepSpeed-style prefix accepted
    key = "flow.chain.1.scale_module.feature_processor._relative_features_mlp._layers.0.weight"
    assert torch.equal(m.state_dict()[key], ref_sd[key])
    m.load_state_dict(ref_sd)


def test_state_dict_matches_reference_yaml_size():
    full = _model().state_dict()
    z = np.load(os.path.join(H.GOLDEN, "equivariant_full_ad.npz"))
    ref = {str(k): tuple(int(s) for s in shp[: max(1, (shp > 0).sum())]) if shp.any() else () for k, shp in zip(z["sd_keys"], z["sd_shapes"])}
    assert {k: tuple(v.shape) for k, v in full.items()} == ref
    assert list(full.keys()) == [str(k) for k in z["sd_keys"]]
    assert len(full) == 219 and sum(v.numel() for v in full.values()) == 3_017_650 == int(z["n_parameters"])


def test_config_round_trip_from_yaml_mapping():
    import timewarp_amd as tw
    from timewarp_amd import synthetic

    mapping = {"model_type": "equivariant_nvp",
               "equivariant_nvp_config": {"atom_embedding_dim": 32, "num_coupling_layers": 4, "latent_mlp_hidden_dims": [256, 256]}}
    cfg = tw.model_config_from_dict(mapping)
    assert isinstance(cfg.equivariant_nvp_config, tw.EquivariantNVPConfig)
    assert cfg == synthetic.equivariant_nvp_config()
    assert cfg.equivariant_nvp_config.position_layer_index_mod_2 == 0
    assert cfg.equivariant_nvp_config.conditional_flow_density.use_displacement_as_target
    m = tw.model_constructor(cfg)
    assert m.dims.n_hidden == 2 and m.dims.d_hidden == 256 and m.dims.d_emb == 32 and m.dims.n_coupling == 4
    with pytest.raises(KeyError):
        tw.model_config_from_dict({"model_type": "equivariant_nvp", "equivariant_nvp_config": {"atom_embedding_dim": 32,
                                   "num_coupling_layers": 4, "latent_mlp_hidden_dims": [256], "no_such_key": 1}})


def test_constructor_rules():
    import timewarp_amd as tw

    with pytest.raises(AssertionError):
        _model(n_coupling=3)
    with pytest.raises(AssertionError):
        _model(pos_mod=2)
    with pytest.raises(NotImplementedError, match="sub-config is missing"):
        tw.model_constructor(tw.ModelConfig("equivariant_nvp"))
    with pytest.raises(AssertionError):
        tw.model_constructor(tw.ModelConfig("equivariant_nvp", equivariant_nvp_config=tw.EquivariantNVPConfig(32, 4, None)))
    with pytest.raises(NotImplementedError):
        _model(hidden=(256, 128))
    with pytest.raises(NotImplementedError):
        _model(hidden=(12,))


def test_raw_layout_agrees_with_library():
    from timewarp_amd import _lib, weights

    lib = _lib.load()
    for m in (_model(), _model(emb=4, hidden=(8, 8), n_coupling=2), _model(emb=4, hidden=(8,), n_coupling=2, pos_mod=1),
              _model(emb=5, hidden=(24, 24, 24), n_coupling=6)):
        desc = m.dims.to_desc()
        assert m.dims.variant == weights.EQUIVARIANT == 3
        assert lib.tw_flow_raw_floats(C.byref(desc)) == weights.raw_numel(m.dims), lib.tw_last_error()
        raw = weights.pack_raw(m.state_dict(), m.dims)
        assert raw.numel() == weights.raw_numel(m.dims)
        entries = weights.raw_entries(m.dims)
        assert {k for k, _ in entries if k != weights.PAD} == set(m.state_dict().keys())
        pos = 0
        for k, shape in entries:   # every tensor with an axis starts at a multiple of 4 floats
            if k != weights.PAD and len(shape) > 0:
                assert pos % 4 == 0, k
            pos += int(np.prod(shape)) if len(shape) else 1


def test_descriptor_checks():
    from timewarp_amd import _lib

    lib = _lib.load()
    good = _model().dims.to_desc()
    assert lib.tw_flow_raw_floats(C.byref(good)) > 3_017_650 - 1
    assert lib.tw_flow_workspace_bytes(C.byref(good), 64, 22) > 0
    for field in ("n_layers", "d_model", "d_ff", "n_heads", "d_rff", "cheb_order"):   # stray attention fields
        desc = _model().dims.to_desc()
        setattr(desc, field, 2)
        assert lib.tw_flow_raw_floats(C.byref(desc)) == -1, field
        assert b"equivariant" in lib.tw_last_error()
    for field, bad in (("n_hidden", 0), ("n_hidden", 4), ("d_hidden", 12), ("d_hidden", 264), ("d_emb", 65), ("d_emb", 0),
                       ("pos_mod2", 2), ("n_coupling", 0)):
        desc = _model().dims.to_desc()
        setattr(desc, field, bad)
        assert lib.tw_flow_raw_floats(C.byref(desc)) == -1, (field, bad)
        assert lib.tw_flow_workspace_bytes(C.byref(desc), 4, 22) == -1


def test_paths_and_packs():
    from timewarp_amd import _lib

    lib = _lib.load()
    desc = _model().dims.to_desc()
    for V in (1, 22, 48, 64, 192, 691):
        got = [lib.tw_flow_path_supported(C.byref(desc), V, p) for p in range(6)]
        assert got == [1, 0, 1, 0, 0, 0], (V, got)   # AUTO and SIMPLE only
    for fn in ("tw_flow_packed_floats", "tw_flow_packed_h3_bytes", "tw_flow_packed_simple_h3_bytes", "tw_flow_packed_h1_bytes"):
        assert getattr(lib, fn)(C.byref(desc)) == 0, fn
    for fn in ("tw_flow_pack", "tw_flow_pack_h3", "tw_flow_pack_simple_h3", "tw_flow_pack_h1"):
        assert getattr(lib, fn)(C.byref(desc), None, None, None) == -1, fn   # TW_ERR_INVALID
        assert b"unsupported" in lib.tw_last_error(), fn


def test_execution_path_names(monkeypatch):
    from timewarp_amd import _lib

    for name in (None, "auto", "f32", "simple", "h3"):
        if name is None:
            monkeypatch.delenv("TW_EXECUTION_PATH", raising=False)
        else:
            monkeypatch.setenv("TW_EXECUTION_PATH", name)
        m = _model()
        assert m._path_for(22) == _lib.TW_PATH_SIMPLE and m._path_for(691) == _lib.TW_PATH_SIMPLE, name
        assert not m.used_split_fp16
    for name in ("h1", "simple_h3"):
        monkeypatch.setenv("TW_EXECUTION_PATH", name)
        with pytest.raises(RuntimeError, match="half-precision"):
            _model()._path_for(22)


def _rotation(g):
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.float()


@pytest.mark.parametrize("name,pos_mod", [("equivariant_tiny", 0), ("equivariant_tiny_pm1", 1)])
def test_log_likelihood_invariant_under_rotation_and_translation(name, pos_mod):
    """The reference's tests/test_distributional_equivariance.py on the restatement: one random rotation and one translation of
    (x, y), velocities rotated only, at its rtol = atol = 1e-4."""
    d, sd = H.load(name)
    spec = eo.EquivariantFlowSpec(num_coupling_layers=2, position_layer_index_mod_2=pos_mod)
    g = torch.Generator().manual_seed(5)
    rot, shift = _rotation(g), torch.randn(3, generator=g)
    base = eo.log_likelihood(sd, spec, d["atom_types"], d["x_coords"], d["x_velocs"], d["y_coords"], d["y_velocs"], d["masked"])
    moved = eo.log_likelihood(sd, spec, d["atom_types"], d["x_coords"] @ rot.T + shift, d["x_velocs"] @ rot.T,
                              d["y_coords"] @ rot.T + shift, d["y_velocs"] @ rot.T, d["masked"])
    assert torch.allclose(moved, base, rtol=1e-4, atol=1e-4), (moved, base)


@pytest.mark.skipif(not os.path.isdir(_REF), reason="reference checkout not present")
def test_install_routes_equivariant_config_to_this_package():
    _import_reference()
    import timewarp.model_constructor as ref_mc
    from timewarp.model_configs import EquivariantNVPConfig, ModelConfig

    import timewarp_amd.integration as twi
    from timewarp_amd.modules.flow import ConditionalFlowDensityModel

    twi.install(replace_energy=False, replace_mh_loop=False)
    cfg = ModelConfig(model_type="equivariant_nvp", equivariant_nvp_config=EquivariantNVPConfig(
        atom_embedding_dim=32, num_coupling_layers=4, latent_mlp_hidden_dims=[256, 256]))
    model = ref_mc.model_constructor(cfg)
    assert isinstance(model, ConditionalFlowDensityModel)
    assert model.dims.variant == 3 and model.dims.n_hidden == 2
    assert len(model.state_dict()) == 219
