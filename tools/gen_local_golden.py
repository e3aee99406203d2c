"""Reference vectors of the local-attention flow (attention_type "local") from the REFERENCE's own model.

    python tools/gen_local_golden.py        # needs the reference checkout the oracle generator imports

Follows tools/pin_energy: it imports, and does not change, the helpers of oracle/gen_golden.py (the reference import recipe,
the alanine-dipeptide topology, the padded batch, run_case) and builds the reference's LocalSelfAttention model through its
custom_transformer_nvp_constructor.  Writes to tests/golden/:

  local_tiny.npz      emb 4, d_model 8, ff 16, hidden [8], 2 couplings x 2 layers, 2 heads, max_radius 0.8 nm (in-radius
                      counts 1 .. molecule size on these coordinates: `counts`, `b1_counts`), reference-initialised weights
                      stored in full (sd::*); the padded 3-molecule batch and the B = 1 sampling case with padding (b1_*).
  local_full_ad.npz   configs/local_transformer_nvp.yaml (emb 16, d_model 128, ff 2048, 8 heads, 0.2 nm) with the name-seeded
                      weights of oracle.flow_oracle.synth_state_dict (the tests regenerate them from the same key set:
                      `sd_keys`, `sd_shapes`); alanine dipeptide, S = 64: log_likelihood, sample + logp, logp_yx, and the
                      layer trace of chain[7].scale_transformer (the first net of the reverse pass).  The plain recipe keeps
                      every coupling in range (finite, O(1) outputs), so no calibration is applied.
  local_full_ad_r005.npz, local_full_ad_r100.npz
                      the same weights and inputs at 0.05 nm (every atom its own only neighbour) and 1.0 nm (every atom sees
                      all 22: alanine dipeptide's largest separation is 0.885 nm - unrestricted softmax attention).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as gg  # noqa: E402  (imports the reference; see oracle/gen_golden.py)
from oracle import flow_oracle as fo  # noqa: E402
from timewarp.model_configs import CustomAttentionTransformerNVPConfig  # noqa: E402
from timewarp.model_constructor import custom_transformer_nvp_constructor  # noqa: E402
from timewarp.modules.layers.custom_attention_encoder import CustomAttentionEncoderLayerConfig  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TINY_RADIUS = 0.8


def local_model(emb, d_model, ff, mlp_hidden, n_coupling, n_layers, num_heads, max_radius):
    enc = CustomAttentionEncoderLayerConfig(d_model=d_model, dim_feedforward=ff, dropout=0.0, num_heads=num_heads,
                                            attention_type="local", max_radius=max_radius)
    cfg = CustomAttentionTransformerNVPConfig(atom_embedding_dim=emb, latent_mlp_hidden_dims=list(mlp_hidden),
                                              num_coupling_layers=n_coupling, num_transformer_layers=n_layers,
                                              encoder_layer_config=enc)
    return custom_transformer_nvp_constructor(cfg).eval()


def in_radius_counts(x_c, mask, r):
    """Per (row, query) in-radius counts on the centred conditioning coordinates the flow sees (local_self_attention.py:66-79)."""
    xc = x_c - fo.centre_of_mass(x_c, mask)
    dist = torch.cdist(xc, xc, compute_mode="donot_use_mm_for_euclid_dist")
    dist = dist.masked_fill(mask[:, None, :] | mask[:, :, None], float("inf"))
    return (dist < r).sum(-1).to(torch.int32).numpy()


def gen_tiny():
    torch.manual_seed(1234)
    m = local_model(emb=4, d_model=8, ff=16, mlp_hidden=[8], n_coupling=2, n_layers=2, num_heads=2, max_radius=TINY_RADIUS)
    with torch.no_grad():
        m.coords_prior_log_scale.fill_(-0.3)
        m.velocs_prior_log_scale.fill_(0.2)
    g = torch.Generator().manual_seed(7)
    at, x_c, x_v, mask, y_c, y_v = gg.padded_batch(g, 3, 7, [7, 5, 6])
    d = gg.base_inputs(at, x_c, x_v, mask, y_c, y_v)
    d.update(gg.run_case(m, at, x_c, x_v, mask, y_c, y_v, 0, 0))
    d.update(gg.np_sd(m.state_dict()))
    d["counts"] = in_radius_counts(x_c, mask, TINY_RADIUS)
    d["max_radius"] = np.float32(TINY_RADIUS)
    at1, x1, v1, m1, yc1, yv1 = gg.padded_batch(g, 1, 7, [5])
    r = gg.run_case(m, at1, x1, v1, m1, yc1, yv1, 4, 99)
    d.update({"b1_" + k: v for k, v in gg.base_inputs(at1, x1, v1, m1, yc1, yv1).items()})
    d.update({"b1_" + k: v for k, v in r.items()})
    d["b1_counts"] = in_radius_counts(x1, m1, TINY_RADIUS)
    np.savez_compressed(os.path.join(OUT, "local_tiny.npz"), **d)
    print("local_tiny", d["counts"].tolist(), d["b1_counts"].tolist())


def gen_full(ad_x, ad_t):
    for tag, radius in (("local_full_ad", 0.2), ("local_full_ad_r005", 0.05), ("local_full_ad_r100", 1.0)):
        full = local_model(emb=16, d_model=128, ff=2048, mlp_hidden=[256], n_coupling=8, n_layers=3, num_heads=8,
                           max_radius=radius)
        sd = fo.synth_state_dict(full.state_dict(), base_seed=0)
        full.load_state_dict(sd)
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
        d["counts"] = in_radius_counts(x_c, mask, radius)
        d["max_radius"] = np.float32(radius)
        if tag == "local_full_ad":
            keys = list(sd.keys())
            d["sd_keys"] = np.array(keys)
            d["sd_shapes"] = np.array([list(sd[k].shape) + [0] * (2 - sd[k].dim()) for k in keys], dtype=np.int64)
            trace = {}

            def saver(key):
                def hook(m, i, o):  # must return None: a returned value would replace the module output
                    trace.setdefault(key, o[:2].detach().numpy().copy())
                return hook

            net = full.flow.chain[7].scale_transformer
            hooks = [net.in_mlp.register_forward_hook(saver("tr_in_mlp"))]
            for l in range(3):
                hooks.append(net.encoder_layers[l].register_forward_hook(saver(f"tr_enc{l}")))
            hooks.append(net.out_mlp.register_forward_hook(saver("tr_out_mlp")))
            torch.manual_seed(2024)
            with torch.no_grad():
                full.conditional_sample_with_logp(
                    atom_types=at, x_coords=x_c, x_velocs=x_v, adj_list=torch.zeros((0, 2), dtype=torch.int64),
                    edge_batch_idx=torch.zeros((0,), dtype=torch.int64), masked_elements=mask, num_samples=S)
            for h in hooks:
                h.remove()
            d.update(trace)
        for k in ("loglik", "s_y_coords", "s_logp", "logp_yx"):
            assert np.isfinite(d[k]).all(), (tag, k)
        np.savez_compressed(os.path.join(OUT, tag + ".npz"), **d)
        c = d["counts"]
        print(tag, "counts min/mean/max", c.min(), float(c.mean()), c.max(), "loglik", d["loglik"], "s_logp[:3]", d["s_logp"][:3, 0])


def main():
    torch.set_num_threads(8)
    ad_x, ad_t = gg.ad_topology()
    gen_tiny()
    gen_full(ad_x, ad_t)


if __name__ == "__main__":
    main()
