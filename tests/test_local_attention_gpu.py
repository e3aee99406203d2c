"""Local self-attention (attention_type "local") on the MI355X: the per-op paths (TW_PATH_SIMPLE, TW_PATH_SIMPLE_H3 and the
constructor's default) against the reference's own vectors (tests/golden/local_*.npz), against the CPU restatement
(tests/local_flow_oracle.py) over molecule sizes 1 .. 691, through whole MH iterations, and for run-to-run determinism."""
import numpy as np
import pytest
import torch

from oracle import flow_oracle as fo
from oracle import mh_oracle as mo
from tests import helpers as H
from tests import local_flow_oracle as lo

pytestmark = pytest.mark.gpu

SIMPLE, SIMPLE_H3 = 2, 5
PATHS = [SIMPLE, SIMPLE_H3, None]   # None: the constructor's default (split-fp16 preference -> TW_PATH_SIMPLE_H3)
TOL = 1e-5
FULL_CASES = [("local_full_ad", 0.2), ("local_full_ad_r005", 0.05), ("local_full_ad_r100", 1.0)]


def tw_local_model(sd, emb=16, d_model=128, ff=2048, hidden=256, n_coupling=8, n_layers=3, num_heads=8, max_radius=0.2,
                   path=SIMPLE):
    import timewarp_amd as tw

    enc = tw.CustomAttentionEncoderLayerConfig(d_model=d_model, dim_feedforward=ff, dropout=0.0, num_heads=num_heads,
                                               attention_type="local", max_radius=max_radius)
    cfg = tw.ModelConfig("custom_attention_transformer_nvp", custom_transformer_nvp_config=tw.CustomAttentionTransformerNVPConfig(
        emb, [hidden], n_coupling, n_layers, enc))
    m = tw.model_constructor(cfg)
    if sd is None:
        sd = fo.synth_state_dict(m.state_dict(), 0)
    m.load_state_dict(sd)
    if path is not None:
        m.execution_path = path
    return m.cuda().eval(), sd


def tiny_model(sd, path):
    return tw_local_model(sd, emb=4, d_model=8, ff=16, hidden=8, n_coupling=2, n_layers=2, num_heads=2, max_radius=0.8,
                          path=path)[0]


@pytest.mark.parametrize("path", PATHS)
def test_tiny_golden(path):
    d, sd = H.load("local_tiny")
    m = tiny_model(sd, path)
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)
    H.assert_case_close(H.run_model_case(m, d, "b1_"), d, "b1_", tol=TOL)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,radius", FULL_CASES)
def test_full_ad_goldens(name, radius, path):
    d, _ = H.load(name)
    m, _ = tw_local_model(None, max_radius=radius, path=path)
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)


@pytest.mark.parametrize("path", [SIMPLE, SIMPLE_H3])
def test_netblock_stages_vs_reference_trace(path):
    """Every stage of the first net of the reverse pass (chain[7].scale_transformer) against the reference's activations."""
    d, _ = H.load("local_full_ad")
    m, _ = tw_local_model(None, path=path)
    xc = d["x_coords"] - fo.centre_of_mass(d["x_coords"], d["masked"])
    acts, out = m.debug_netblock(7, 0, d["atom_types"].cuda(), xc.cuda(), d["x_velocs"].cuda(), d["masked"].cuda(),
                                 d["z_coords"][:2, 0].cuda(), path)
    H.assert_not_demoted(m)
    for i, n in enumerate(["tr_in_mlp", "tr_enc0", "tr_enc1", "tr_enc2"]):
        e = H.rel_err(acts[i].cpu(), d[n])
        assert e < TOL, (n, e)
    assert H.rel_err(out.cpu(), d["tr_out_mlp"]) < TOL


def _molecule(V):
    """Realistic atom densities: alanine dipeptide's coordinates up to 22 atoms, the 691-atom protein's (frame 0) above."""
    from timewarp_amd import synthetic

    if V <= 22:
        types, coords, _ = synthetic.alanine_dipeptide_state()
        return types[:V], coords[:V]
    z = np.load(f"{H.GOLDEN}/energy_kat_1hgv.npz")
    pos = torch.from_numpy(np.asarray(z["positions"], dtype=np.float32))
    pos = pos[0] if pos.dim() == 3 else pos
    vocab = {"C": 0, "H": 1, "N": 2, "O": 3, "S": 4}
    types = torch.tensor([vocab.get(str(n).strip()[0], 0) for n in z["atom_names"]], dtype=torch.int64)
    return types[:V], pos[:V]


@pytest.mark.parametrize("path", [SIMPLE, SIMPLE_H3])
@pytest.mark.parametrize("V", [1, 5, 22, 65, 129, 257, 691])
def test_size_sweep_vs_restatement(V, path):
    """Both passes against the CPU restatement: the forward pass (log_likelihood) over 3 rows of different conditioning
    states, the reverse pass (sampling) of 3 samples; a masked tail of ~10 % of the atoms from 5 atoms on."""
    torch.manual_seed(V)
    types, coords = _molecule(V)
    m, sd = tw_local_model(None, path=path)
    spec = lo.LocalFlowSpec()
    n_masked = V // 10 if V >= 5 else 0
    mask = torch.zeros(1, V, dtype=torch.bool)
    if n_masked:
        mask[0, V - n_masked:] = True
    g = torch.Generator().manual_seed(V)
    B = 3
    at = types[None].repeat(B, 1)
    xc = coords[None] + 0.01 * torch.randn(B, V, 3, generator=g)
    xv = torch.randn(B, V, 3, generator=g)
    yc = xc + 0.01 * torch.randn(B, V, 3, generator=g)
    yv = torch.randn(B, V, 3, generator=g)
    mk = mask.repeat(B, 1)
    ref = lo.log_likelihood(sd, spec, at, xc, xv, yc, yv, mk)
    got = m.log_likelihood(atom_types=at.cuda(), x_coords=xc.cuda(), x_velocs=xv.cuda(), y_coords=yc.cuda(),
                           y_velocs=yv.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mk.cuda()).cpu()
    assert H.rel_err(got, ref) < TOL, ("loglik", H.rel_err(got, ref))
    zc, zv = fo.draw_latents(sd, 3, (1, V, 3), g)
    ryc, ryv, rlp = lo.conditional_sample_with_logp(sd, spec, at[:1], xc[:1], xv[:1], mask, zc, zv)
    gyc, gyv, glp = m.conditional_sample_with_logp(atom_types=at[:1].cuda(), x_coords=xc[:1].cuda(), x_velocs=xv[:1].cuda(),
                                                   adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda(), num_samples=3,
                                                   z_coords=zc.cuda(), z_velocs=zv.cuda())
    keep = ~mask[0]
    assert H.rel_err(gyc.cpu()[:, :, keep], ryc[:, :, keep]) < TOL
    assert H.rel_err(gyv.cpu()[:, :, keep], ryv[:, :, keep]) < TOL
    assert H.rel_err(glp.cpu(), rlp) < TOL
    H.assert_not_demoted(m)


def _mh_sd(random_velocs):
    """The YAML config's name-seeded weights with the last out_mlp layers scaled by 1e-4 (shifts ~1e-4 nm: proposals the
    stiff bonded terms still accept), prior log-scales as in tests/helpers.py::mh_state_dict."""
    _, sd = tw_local_model(None)
    sd = dict(sd)
    for k in sd:
        if ".out_mlp._layers.2." in k:
            sd[k] = sd[k] * 1e-4
    sd["coords_prior_log_scale"] = torch.tensor(-7.0)
    sd["velocs_prior_log_scale"] = torch.tensor(0.0 if random_velocs else -3.0)
    return sd


@pytest.mark.parametrize("path", [SIMPLE, SIMPLE_H3])
@pytest.mark.parametrize("random_velocs,seed", [(False, 3), (True, 4)])
def test_full_size_mh_iterations_vs_oracle(path, random_velocs, seed):
    """Whole MH iterations (sample_with_model: tw_mh_iteration) with the local model, AMBER energy kernel, alanine dipeptide,
    64 proposals per iteration, against oracle/mh_oracle.sample_with_model with the restatement installed, on shared
    host-drawn noise."""
    from timewarp_amd import synthetic
    from timewarp_amd.dataloader import single_state_batch
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from timewarp_amd.utils.evaluation_utils import sample_with_model

    S, N = 64, 130
    sd = _mh_sd(random_velocs)
    types, coords, masses = synthetic.alanine_dipeptide_state()
    v0 = torch.randn(1, 22, 3, generator=torch.Generator().manual_seed(9)) * 0.05
    kw = dict(accept=True, num_proposal_steps=S)
    if random_velocs:
        kw.update(random_velocs=True, resample_velocs=True)
    energy = AmberPotentialEnergyTorch.alanine_dipeptide()
    with lo.installed():
        ref = mo.sample_with_model(types[None], coords[None], v0, torch.zeros(1, 22, dtype=torch.bool),
                                   mo.OracleModel(sd, lo.LocalFlowSpec()), H.OracleAmberEnergy(energy.tables), masses, N,
                                   H.HostNoise(seed), **kw)
    model, _ = tw_local_model(sd, path=path)
    got = sample_with_model(single_state_batch("ad", types, coords, v0[0]), model, torch.device("cuda"), energy, masses, N,
                            disable_tqdm=True, noise=H.HostNoise(seed, "cuda"), **kw)
    H.assert_not_demoted(model)
    (rc, rv, racc, rs), (gc, gv, gacc, gs) = ref, got
    assert racc >= 1
    assert gc.shape == rc.shape and gacc == racc
    assert np.array_equal(gs.acceptance_indicator.astype(bool), rs.acceptance_indicator.astype(bool))
    assert H.rel_err(gc, rc) < TOL and H.rel_err(gv, rv) < TOL
    assert H.elem_rel_err(gs.p_xy, rs.p_xy) < TOL and H.elem_rel_err(gs.p_yx, rs.p_yx) < TOL
    scale = float(np.abs(rs.p_xy).max() + np.abs(rs.energies_pot).max() + np.abs(rs.energies_kin).max())
    assert np.abs(gs.exponent - rs.exponent).max() < TOL * scale


def test_lockstep_chains_equal_single_chains():
    """tw_mh_iteration_chains with the local model: three chains in lock-step, each bit-identical to the single-chain route
    driven by the same noise."""
    from timewarp_amd import synthetic
    from timewarp_amd.dataloader import single_state_batch
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from timewarp_amd.utils.evaluation_utils import DeviceNoise, sample_with_model
    from timewarp_amd.utils.multichain import sample_with_model_chains

    sd = _mh_sd(True)
    model, _ = tw_local_model(sd, path=SIMPLE_H3)
    types, coords, masses = synthetic.alanine_dipeptide_state()
    energy = AmberPotentialEnergyTorch.alanine_dipeptide()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1)
    starts = [coords + 0.002 * torch.randn(coords.shape, generator=g) for _ in range(3)]
    kw = dict(random_velocs=True, resample_velocs=True)
    N, S = 40, 16
    singles = [sample_with_model(single_state_batch("ad", types, xc), model, dev, energy, masses, N, accept=True,
                                 num_proposal_steps=S, disable_tqdm=True, noise=DeviceNoise(dev, seed=60 + c), **kw)
               for c, xc in enumerate(starts)]
    multi = sample_with_model_chains([single_state_batch("ad", types, xc) for xc in starts], model, dev, energy, masses, N, S,
                                     noises=[DeviceNoise(dev, seed=60 + c) for c in range(3)], sync_every=2, **kw)
    H.assert_not_demoted(model)
    assert sum(a[2] for a in singles) > 0
    for a, b in zip(singles, multi):
        assert a[0].shape == b[0].shape and a[2] == b[2]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[3].p_xy, b[3].p_xy) and np.array_equal(a[3].exponent, b[3].exponent)


@pytest.mark.parametrize("path", [SIMPLE, SIMPLE_H3])
def test_deterministic(path):
    """Two identical calls give bit-identical results (no atomics anywhere on the local-attention route)."""
    d, _ = H.load("local_full_ad")
    m, _ = tw_local_model(None, path=path)
    a = H.run_model_case(m, d)
    b = H.run_model_case(m, d)
    for k in a:
        assert torch.equal(a[k], b[k]), k
