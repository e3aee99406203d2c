"""CPU restatement of the reference's local self-attention flow (attention_type "local").  TEST INFRASTRUCTURE ONLY.

The reference's LocalSelfAttention (modules/layers/local_self_attention.py:14-117) in plain PyTorch (CPU, fp32), plugged
into oracle/flow_oracle.py without changing it: `installed()` substitutes `fo.scale_and_shift` for specs whose variant is
"local" and hands every other spec to the original.  `fo.flow_pass` computes kernel scores only for the "kernel" variant, so
with the substitution in place `fo.log_likelihood`, `fo.conditional_sample_with_logp` and `oracle.mh_oracle.OracleModel`
serve the local model unchanged.  Pinned against the reference by tests/test_local_attention_cpu.py on the vectors
tools/gen_local_golden.py wrote.  File:line citations are relative to the reference root.
"""
from __future__ import annotations

import contextlib
import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import flow_oracle as fo

Tensor = torch.Tensor


@dataclass
class LocalFlowSpec(fo.FlowSpec):
    """custom_attention_transformer_nvp with attention_type "local" (custom_attention_encoder.py:140-153)."""

    variant: str = "local"
    attention_type: str = "local"
    n_head: int = 8           # num_heads of the encoder-layer config (no lengthscales decide it here)
    max_radius: float = 0.2   # nm


def in_radius(positions: Tensor, masked: Tensor, max_radius: float) -> Tensor:
    """local_self_attention.py:64-79: [B, V, V] True where key m lies strictly within max_radius of query q; torch.cdist's
    direct form; a masked atom is nobody's neighbour, not even its own (its distances are +inf)."""
    dist = torch.cdist(positions, positions, compute_mode="donot_use_mm_for_euclid_dist")
    dist = dist.masked_fill(torch.logical_or(masked[:, None, :], masked[:, :, None]), math.inf)
    return dist < max_radius


def local_self_attention(sd: Dict[str, Tensor], prefix: str, h: Tensor, positions: Tensor, masked: Tensor,
                         n_head: int, max_radius: float) -> Tensor:
    """local_self_attention.py:43-117, op for op.  qkv = h W^T reshaped to [B, V, H, 3 d] and split q, k, v (:53-59, key /
    query / value width d = d_model); the K = max in-radius count nearest keys by topk (:81-90) gathered (get_closest,
    :120-137); scores (k q).sum(-1) / sqrt(d) with -inf beyond the radius (:95-100); softmax over the K; masked_fill(0),
    which zeroes the NaN rows of queries without neighbours (:103-108); weighted sum; bias-free output projection (:110-117)."""
    b, v, d = h.shape
    qkv = F.linear(h, sd[f"{prefix}.qkv_proj.weight"]).reshape(b, v, n_head, 3 * d)
    q, k, val = torch.split(qkv, [d, d, d], dim=-1)
    dist = torch.cdist(positions, positions, compute_mode="donot_use_mm_for_euclid_dist")
    dist = dist.masked_fill(torch.logical_or(masked[:, None, :], masked[:, :, None]), math.inf)
    max_neighbors = int((dist < max_radius).sum(dim=-1).max())
    top_d, idx = torch.topk(dist, k=max_neighbors, dim=-1, largest=False)
    far = top_d > max_radius
    gather = lambda m: torch.gather(m[:, None].expand(-1, v, -1, -1, -1), -3,
                                    idx[:, :, :, None, None].expand(-1, -1, -1, n_head, d))
    scores = (gather(k) * q[:, :, None]).sum(-1) / math.sqrt(d)  # [B, V, K, H]
    scores = scores.masked_fill(far[..., None], -math.inf)
    weights = torch.softmax(scores, dim=-2).masked_fill(far[..., None], 0.0)
    out = (weights[..., None] * gather(val)).sum(dim=-3).reshape(b, v, n_head * d)
    return F.linear(out, sd[f"{prefix}.output_proj.weight"])


def local_netblock(sd: Dict[str, Tensor], prefix: str, u: Tensor, spec: LocalFlowSpec, positions: Tensor, masked: Tensor,
                   trace: Optional[list] = None) -> Tensor:
    """custom_transformer_block.py:46-82 with local encoder layers: in_mlp -> L x (attention, post-norm residual, ReLU FFN;
    custom_attention_encoder.py:82-114) -> out_mlp."""
    h = fo.mlp(sd, f"{prefix}.in_mlp", u)
    if trace is not None:
        trace.append(("in_mlp", h))
    for l in range(spec.num_transformer_layers):
        p = f"{prefix}.encoder_layers.{l}"
        a = local_self_attention(sd, f"{p}.self_attn", h, positions, masked, spec.n_head, spec.max_radius)
        h = fo.encoder_layer_tail(sd, p, h, a, spec.layer_norm_eps)
        if trace is not None:
            trace.append((f"enc{l}", h))
    out = fo.mlp(sd, f"{prefix}.out_mlp", h)
    if trace is not None:
        trace.append(("out_mlp", out))
    return out


def local_scale_and_shift(sd, spec: LocalFlowSpec, c: int, z_coords: Tensor, z_velocs: Tensor, x_features: Tensor,
                          x_coords: Tensor, x_velocs: Tensor, masked: Tensor, scores=None):
    """custom_transformer_nvp.py:44-93: both nets take the (centred) conditioning coordinates as positions."""
    positions = c % 2 == spec.position_layer_index_mod_2
    z_other = z_velocs if positions else z_coords
    u = torch.cat([x_features, x_coords, x_velocs, z_other], dim=-1)
    pre = f"flow.chain.{c}"
    s = local_netblock(sd, f"{pre}.scale_transformer", u, spec, x_coords, masked)
    t = local_netblock(sd, f"{pre}.shift_transformer", u, spec, x_coords, masked)
    return torch.exp(s), t


@contextlib.contextmanager
def installed():
    """Within the block, oracle.flow_oracle evaluates LocalFlowSpec models with the restatement above."""
    original = fo.scale_and_shift

    def scale_and_shift(sd, spec, *args, **kwargs):
        if getattr(spec, "variant", None) == "local":
            return local_scale_and_shift(sd, spec, *args, **kwargs)
        return original(sd, spec, *args, **kwargs)

    fo.scale_and_shift = scale_and_shift
    try:
        yield
    finally:
        fo.scale_and_shift = original


def log_likelihood(sd, spec: LocalFlowSpec, *args) -> Tensor:
    with installed():
        return fo.log_likelihood(sd, spec, *args)


def conditional_sample_with_logp(sd, spec: LocalFlowSpec, *args):
    with installed():
        return fo.conditional_sample_with_logp(sd, spec, *args)
