"""The E(3)-equivariant NVP flow (model_type "equivariant_nvp") on the MI355X, through the C ABI (TW_PATH_SIMPLE, the only
path that serves it): against the reference's own vectors (tests/golden/equivariant_*.npz), against the CPU restatement
(tests/equivariant_flow_oracle.py) over molecule sizes 1 .. 691, forward / reverse consistency, run-to-run determinism,
rotation / translation invariance, whole MH iterations and lock-step chains.

Tolerances: TOL = 1e-5 (helpers.rel_err, unmasked atoms) is the standing bar of tests/test_flow_gpu.py; the invariance check
uses the reference test's own rtol = atol = 1e-4 (tests/test_distributional_equivariance.py)."""
import numpy as np
import pytest
import torch

from oracle import flow_oracle as fo
from oracle import mh_oracle as mo
from tests import equivariant_flow_oracle as eo
from tests import helpers as H

pytestmark = pytest.mark.gpu

SIMPLE = 2
TOL = 1e-5
TINY = [("equivariant_tiny", [8, 8], 0), ("equivariant_tiny_h1", [8], 0), ("equivariant_tiny_pm1", [8, 8], 1)]


def tw_eq_model(sd, emb=32, hidden=(256, 256), n_coupling=4, pos_mod=0, path=SIMPLE):
    import timewarp_amd as tw

    cfg = tw.ModelConfig("equivariant_nvp", equivariant_nvp_config=tw.EquivariantNVPConfig(
        atom_embedding_dim=emb, num_coupling_layers=n_coupling, latent_mlp_hidden_dims=list(hidden),
        position_layer_index_mod_2=pos_mod))
    m = tw.model_constructor(cfg)
    if sd is None:
        sd = fo.synth_state_dict(m.state_dict(), 0)
    m.load_state_dict(sd)
    if path is not None:
        m.execution_path = path
    return m.cuda().eval(), sd


def _range_word_clear(m):
    """The fp16 range-guard word of the model is never raised: this variant runs no half-precision kernel."""
    assert not m.used_split_fp16 and not m.demoted
    for flag in m._range_flags.values():
        assert int(flag.item()) == 0


def _check_trace(m, d, pos_mod):
    n = d["tr0_z_other"].shape[0]
    keep = ~d["masked"][:n]
    for c in (0, 1):
        for net, key in ((0, "log_scale"), (1, "shift")):
            _, out = m.debug_netblock(c, net, d["atom_types"][:n].cuda(), d[f"tr{c}_x_coords"].cuda(), d["x_velocs"][:n].cuda(),
                                      d["masked"][:n].cuda(), d[f"tr{c}_z_other"].cuda(), SIMPLE)
            want = d[f"tr{c}_{key}"]
            want = want.repeat(1, 1, 3) if net == 0 else want
            e = H.rel_err(out.cpu()[keep], want[keep])
            assert e < TOL, (c, key, e)


@pytest.mark.parametrize("path", [SIMPLE, None])   # None: the constructor's default preference, which resolves to SIMPLE
@pytest.mark.parametrize("name,hidden,pos_mod", TINY)
def test_tiny_goldens(name, hidden, pos_mod, path):
    d, sd = H.load(name)
    m, _ = tw_eq_model(sd, emb=4, hidden=hidden, n_coupling=2, pos_mod=pos_mod, path=path)
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)
    H.assert_case_close(H.run_model_case(m, d, "b1_"), d, "b1_", tol=TOL)
    _check_trace(m, d, pos_mod)
    _range_word_clear(m)


def test_full_ad_golden():
    d, _ = H.load("equivariant_full_ad")
    m, _ = tw_eq_model(None)
    H.assert_case_close(H.run_model_case(m, d), d, tol=TOL)
    _check_trace(m, d, 0)
    _range_word_clear(m)


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


def _sweep_case(V, B, padded, seed):
    types, coords = _molecule(V)
    mask = torch.zeros(1, V, dtype=torch.bool)
    if padded and V >= 2:
        mask[0, V - max(1, V // 10):] = True
    g = torch.Generator().manual_seed(seed)
    at = types[None].repeat(B, 1)
    xc = coords[None] + 0.01 * torch.randn(B, V, 3, generator=g)
    xv = torch.randn(B, V, 3, generator=g)
    yc = xc + 0.01 * torch.randn(B, V, 3, generator=g)
    yv = torch.randn(B, V, 3, generator=g)
    return at, xc, xv, yc, yv, mask, g


def _sweep(V, B, S, padded):
    m, sd = tw_eq_model(None)
    spec = eo.EquivariantFlowSpec()
    at, xc, xv, yc, yv, mask, g = _sweep_case(V, B, padded, 1000 * V + B)
    mk = mask.repeat(B, 1)
    ref = eo.log_likelihood(sd, spec, at, xc, xv, yc, yv, mk)
    got = m.log_likelihood(atom_types=at.cuda(), x_coords=xc.cuda(), x_velocs=xv.cuda(), y_coords=yc.cuda(),
                           y_velocs=yv.cuda(), adj_list=None, edge_batch_idx=None, masked_elements=mk.cuda()).cpu()
    assert H.rel_err(got, ref) < TOL, ("loglik", H.rel_err(got, ref))
    zc, zv = fo.draw_latents(sd, S, (1, V, 3), g)
    ryc, ryv, rlp = eo.conditional_sample_with_logp(sd, spec, at[:1], xc[:1], xv[:1], mask, zc, zv)
    gyc, gyv, glp = m.conditional_sample_with_logp(atom_types=at[:1].cuda(), x_coords=xc[:1].cuda(), x_velocs=xv[:1].cuda(),
                                                   adj_list=None, edge_batch_idx=None, masked_elements=mask.cuda(), num_samples=S,
                                                   z_coords=zc.cuda(), z_velocs=zv.cuda())
    keep = ~mask[0]
    assert H.rel_err(gyc.cpu()[:, :, keep], ryc[:, :, keep]) < TOL
    assert H.rel_err(gyv.cpu()[:, :, keep], ryv[:, :, keep]) < TOL
    assert H.rel_err(glp.cpu(), rlp) < TOL
    _range_word_clear(m)


SWEEP = [(1, 3, 2), (2, 1, 3), (5, 3, 5), (22, 2, 7), (33, 3, 2), (64, 2, 3), (65, 3, 2), (192, 1, 2), (257, 2, 1)]


@pytest.mark.parametrize("V,B,S,padded", [c + (False,) for c in SWEEP] + [c + (True,) for c in SWEEP if c[0] > 1])
def test_size_sweep_vs_restatement(V, B, S, padded):
    """Both passes against the CPU restatement at yaml size with name-seeded weights: tile edges of the pair kernel (32 pairs
    per tile, 16 query atoms per workgroup) and its key loop, with and without a masked tail."""
    _sweep(V, B, S, padded)


def test_691_atoms():
    _sweep(691, 4, 1, True)


def test_forward_reverse_consistency():
    """log_likelihood of the model's own samples equals the log-density sampling returned."""
    d, _ = H.load("equivariant_full_ad")
    m, _ = tw_eq_model(None)
    S = 16
    yc, yv, lp = m.conditional_sample_with_logp(
        atom_types=d["atom_types"].cuda(), x_coords=d["x_coords"].cuda(), x_velocs=d["x_velocs"].cuda(), adj_list=None,
        edge_batch_idx=None, masked_elements=d["masked"].cuda(), num_samples=S, z_coords=d["z_coords"][:S].cuda(),
        z_velocs=d["z_velocs"][:S].cuda())
    ll = m.log_likelihood(atom_types=d["atom_types"].cuda().repeat(S, 1), x_coords=d["x_coords"].cuda().repeat(S, 1, 1),
                          x_velocs=d["x_velocs"].cuda().repeat(S, 1, 1), y_coords=yc[:, 0], y_velocs=yv[:, 0], adj_list=None,
                          edge_batch_idx=None, masked_elements=d["masked"].cuda().repeat(S, 1))
    assert H.rel_err(ll.cpu(), lp[:, 0].cpu()) < TOL, H.rel_err(ll.cpu(), lp[:, 0].cpu())


def test_deterministic():
    """Two identical calls give bit-identical results (no atomics in the reductions)."""
    d, _ = H.load("equivariant_full_ad")
    m, _ = tw_eq_model(None)
    a = H.run_model_case(m, d)
    b = H.run_model_case(m, d)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _rotation(g):
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.float()


def test_log_likelihood_invariant_under_rotation_and_translation():
    at, xc, xv, yc, yv, mask, g = _sweep_case(22, 4, True, 77)
    m, _ = tw_eq_model(None)
    mk = mask.repeat(4, 1)
    rot, shift = _rotation(g), torch.randn(3, generator=g)
    run = lambda a, b, c, e: m.log_likelihood(atom_types=at.cuda(), x_coords=a.cuda(), x_velocs=b.cuda(), y_coords=c.cuda(),
                                              y_velocs=e.cuda(), adj_list=None, edge_batch_idx=None,
                                              masked_elements=mk.cuda()).cpu()
    base = run(xc, xv, yc, yv)
    moved = run(xc @ rot.T + shift, xv @ rot.T, yc @ rot.T + shift, yv @ rot.T)
    assert torch.allclose(moved, base, rtol=1e-4, atol=1e-4), (moved, base)


def _mh_sd(random_velocs):
    """The yaml config's name-seeded weights with the last layers of the shift coefficients and of the scale's gamma scaled by
    1e-3 (proposals the stiff bonded terms still accept), prior log-scales as in tests/helpers.py::mh_state_dict."""
    _, sd = tw_eq_model(None)
    sd = dict(sd)
    for k in sd:
        if "._layers.4." in k and ("_shift_with_" in k or "._scale_mlp." in k):
            sd[k] = sd[k] * 1e-3
    sd["coords_prior_log_scale"] = torch.tensor(-7.0)
    sd["velocs_prior_log_scale"] = torch.tensor(0.0 if random_velocs else -3.0)
    return sd


@pytest.mark.parametrize("random_velocs,seed", [(False, 3), (True, 4)])
def test_mh_iterations_vs_oracle(random_velocs, seed):
    """Five whole MH iterations (sample_with_model: tw_mh_iteration) on alanine dipeptide, 64 proposals each, against
    oracle/mh_oracle.sample_with_model with the restatement installed, on shared host-drawn noise."""
    from timewarp_amd import synthetic
    from timewarp_amd.dataloader import single_state_batch
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from timewarp_amd.utils.evaluation_utils import sample_with_model

    S, N = 64, 5 * 64
    sd = _mh_sd(random_velocs)
    types, coords, masses = synthetic.alanine_dipeptide_state()
    v0 = torch.randn(1, 22, 3, generator=torch.Generator().manual_seed(9)) * 0.05
    kw = dict(accept=True, num_proposal_steps=S)
    if random_velocs:
        kw.update(random_velocs=True, resample_velocs=True)
    energy = AmberPotentialEnergyTorch.alanine_dipeptide()
    with eo.installed():
        ref = mo.sample_with_model(types[None], coords[None], v0, torch.zeros(1, 22, dtype=torch.bool),
                                   mo.OracleModel(sd, eo.EquivariantFlowSpec()), H.OracleAmberEnergy(energy.tables), masses, N,
                                   H.HostNoise(seed), **kw)
    model, _ = tw_eq_model(sd)
    got = sample_with_model(single_state_batch("ad", types, coords, v0[0]), model, torch.device("cuda"), energy, masses, N,
                            disable_tqdm=True, noise=H.HostNoise(seed, "cuda"), **kw)
    H.assert_not_demoted(model)
    (rc, rv, racc, rs), (gc, gv, gacc, gs) = ref, got
    assert gc.shape == rc.shape and gacc == racc
    assert np.array_equal(gs.acceptance_indicator.astype(bool), rs.acceptance_indicator.astype(bool))
    assert H.rel_err(gc, rc) < TOL and H.rel_err(gv, rv) < TOL
    assert H.elem_rel_err(gs.p_xy, rs.p_xy) < TOL and H.elem_rel_err(gs.p_yx, rs.p_yx) < TOL
    scale = float(np.abs(rs.p_xy).max() + np.abs(rs.energies_pot).max() + np.abs(rs.energies_kin).max())
    assert np.abs(gs.exponent - rs.exponent).max() < TOL * scale
    _range_word_clear(model)


def test_lockstep_chains_equal_single_chains():
    """tw_mh_iteration_chains with the equivariant model: four chains in lock-step, each bit-identical to the single-chain
    route driven by the same noise."""
    from timewarp_amd import synthetic
    from timewarp_amd.dataloader import single_state_batch
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from timewarp_amd.utils.evaluation_utils import DeviceNoise, sample_with_model
    from timewarp_amd.utils.multichain import sample_with_model_chains

    sd = _mh_sd(True)
    model, _ = tw_eq_model(sd)
    types, coords, masses = synthetic.alanine_dipeptide_state()
    energy = AmberPotentialEnergyTorch.alanine_dipeptide()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1)
    starts = [coords + 0.002 * torch.randn(coords.shape, generator=g) for _ in range(4)]
    kw = dict(random_velocs=True, resample_velocs=True)
    N, S = 40, 16
    singles = [sample_with_model(single_state_batch("ad", types, xc), model, dev, energy, masses, N, accept=True,
                                 num_proposal_steps=S, disable_tqdm=True, noise=DeviceNoise(dev, seed=60 + c), **kw)
               for c, xc in enumerate(starts)]
    multi = sample_with_model_chains([single_state_batch("ad", types, xc) for xc in starts], model, dev, energy, masses, N, S,
                                     noises=[DeviceNoise(dev, seed=60 + c) for c in range(4)], sync_every=2, **kw)
    H.assert_not_demoted(model)
    for a, b in zip(singles, multi):
        assert a[0].shape == b[0].shape and a[2] == b[2]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[3].p_xy, b[3].p_xy) and np.array_equal(a[3].exponent, b[3].exponent)
    _range_word_clear(model)
