"""Reference vectors of the E(3)-equivariant NVP flow (model_type "equivariant_nvp") from the REFERENCE's own model.

    python tools/gen_equivariant_golden.py        # needs the reference checkout the oracle generator imports

Follows tools/gen_local_golden.py: it imports, and does not change, the helpers of oracle/gen_golden.py (the reference import
recipe, the alanine-dipeptide topology, the padded batch, run_case) and builds the reference's model through its
equivariant_nvp_constructor.  Writes to tests/golden/:

  equivariant_tiny.npz       emb 4, latent_mlp_hidden_dims [8, 8], 2 couplings, reference-initialised weights stored in full
                             (sd::*); the padded 3-molecule batch and the B = 1 sampling case with padding (b1_*).
  equivariant_tiny_h1.npz    the same with ONE hidden layer ([8]).
  equivariant_tiny_pm1.npz   the same as the first with position_layer_index_mod_2 = 1.
  equivariant_full_ad.npz    configs/equivariant_nvp.yaml (emb 32, [256, 256], 4 couplings) with the name-seeded weights of
                             oracle.flow_oracle.synth_state_dict (the tests regenerate them from the same key set: `sd_keys`,
                             `sd_shapes`); alanine dipeptide, S = 64.
Each holds log_likelihood, sample + logp, logp_yx and the per-module trace of the first two coupling layers (one that
transforms positions, one that transforms velocities) in the forward pass of the log_likelihood call: tr{c}_z_other (the
modules' z_untransformed input), tr{c}_log_scale [B, V, 1], tr{c}_shift [B, V, 3]; tr{c}_x_coords is the centred
conditioning state the modules saw.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as gg  # noqa: E402  (imports the reference; see oracle/gen_golden.py)
from oracle import flow_oracle as fo  # noqa: E402
from timewarp.model_configs import EquivariantNVPConfig  # noqa: E402
from timewarp.model_constructor import equivariant_nvp_constructor  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def equivariant_model(emb, hidden, n_coupling, pos_mod=0):
    cfg = EquivariantNVPConfig(atom_embedding_dim=emb, num_coupling_layers=n_coupling, latent_mlp_hidden_dims=list(hidden),
                               position_layer_index_mod_2=pos_mod)
    return equivariant_nvp_constructor(cfg).eval()


def traced_loglik(model, at, x_c, x_v, mask, y_c, y_v, rows=2):
    """The log_likelihood call again with hooks on the modules of chain[0] and chain[1]."""
    trace = {}

    def saver(c, name):
        def hook(m, args, kwargs, out):  # must return None: a returned value would replace the module output
            trace[f"tr{c}_{name}"] = out[:rows].detach().numpy().copy()
            trace[f"tr{c}_z_other"] = kwargs["z_untransformed"][:rows].detach().numpy().copy()
            trace[f"tr{c}_x_coords"] = kwargs["x_coords"][:rows].detach().numpy().copy()
        return hook

    hooks = []
    for c in (0, 1):
        hooks.append(model.flow.chain[c].scale_module.register_forward_hook(saver(c, "log_scale"), with_kwargs=True))
        hooks.append(model.flow.chain[c].shift_module.register_forward_hook(saver(c, "shift"), with_kwargs=True))
    with torch.no_grad():
        model.log_likelihood(atom_types=at, x_coords=x_c, x_velocs=x_v, y_coords=y_c, y_velocs=y_v,
                             adj_list=torch.zeros((0, 2), dtype=torch.int64),
                             edge_batch_idx=torch.zeros((0,), dtype=torch.int64), masked_elements=mask)
    for h in hooks:
        h.remove()
    return trace


def gen_tiny(name, hidden, pos_mod, seed):
    torch.manual_seed(seed)
    m = equivariant_model(emb=4, hidden=hidden, n_coupling=2, pos_mod=pos_mod)
    with torch.no_grad():
        m.coords_prior_log_scale.fill_(-0.3)
        m.velocs_prior_log_scale.fill_(0.2)
    g = torch.Generator().manual_seed(7)
    at, x_c, x_v, mask, y_c, y_v = gg.padded_batch(g, 3, 7, [7, 5, 6])
    d = gg.base_inputs(at, x_c, x_v, mask, y_c, y_v)
    d.update(gg.run_case(m, at, x_c, x_v, mask, y_c, y_v, 0, 0))
    d.update(traced_loglik(m, at, x_c, x_v, mask, y_c, y_v, rows=3))
    d.update(gg.np_sd(m.state_dict()))
    at1, x1, v1, m1, yc1, yv1 = gg.padded_batch(g, 1, 7, [5])
    r = gg.run_case(m, at1, x1, v1, m1, yc1, yv1, 4, 99)
    d.update({"b1_" + k: v for k, v in gg.base_inputs(at1, x1, v1, m1, yc1, yv1).items()})
    d.update({"b1_" + k: v for k, v in r.items()})
    d["pos_mod"] = np.int64(pos_mod)
    for k in ("loglik", "b1_s_y_coords", "b1_s_logp", "b1_logp_yx"):
        assert np.isfinite(d[k]).all(), (name, k)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
    print(name, "loglik", d["loglik"], "b1_s_logp", d["b1_s_logp"][:, 0])


def gen_full(ad_x, ad_t):
    full = equivariant_model(emb=32, hidden=[256, 256], n_coupling=4)
    sd = fo.synth_state_dict(full.state_dict(), base_seed=0)
    full.load_state_dict(sd)
    n_param = sum(p.numel() for p in full.parameters())
    g = torch.Generator().manual_seed(11)
    x_c = ad_x[None].clone()
    x_v = torch.randn(1, 22, 3, generator=g) * 0.5
    mask = torch.zeros(1, 22, dtype=torch.bool)
    y_c = x_c + torch.randn(1, 22, 3, generator=g) * 0.01
    y_v = torch.randn(1, 22, 3, generator=g) * 0.5
    at = ad_t[None]
    S = gg.S_FULL
    d = gg.base_inputs(at, x_c, x_v, mask, y_c, y_v)
    d.update(gg.run_case(full, at, x_c, x_v, mask, y_c, y_v, S, 2024))
    d.update(traced_loglik(full, at, x_c, x_v, mask, y_c, y_v, rows=1))
    keys = list(sd.keys())
    d["sd_keys"] = np.array(keys)
    d["sd_shapes"] = np.array([list(sd[k].shape) + [0] * (2 - sd[k].dim()) for k in keys], dtype=np.int64)
    d["n_parameters"] = np.int64(n_param)
    for k in ("loglik", "s_y_coords", "s_logp", "logp_yx"):
        assert np.isfinite(d[k]).all(), k
    np.savez_compressed(os.path.join(OUT, "equivariant_full_ad.npz"), **d)
    print("equivariant_full_ad", len(keys), "entries", n_param, "parameters; loglik", d["loglik"], "s_logp[:3]", d["s_logp"][:3, 0],
          "max |log_scale|", [float(np.abs(d[f"tr{c}_log_scale"]).max()) for c in (0, 1)],
          "max |shift|", [float(np.abs(d[f"tr{c}_shift"]).max()) for c in (0, 1)])


def main():
    torch.set_num_threads(8)
    ad_x, ad_t = gg.ad_topology()
    gen_tiny("equivariant_tiny", [8, 8], 0, 1234)
    gen_tiny("equivariant_tiny_h1", [8], 0, 1235)
    gen_tiny("equivariant_tiny_pm1", [8, 8], 1, 1236)
    gen_full(ad_x, ad_t)


if __name__ == "__main__":
    main()
