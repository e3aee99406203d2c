"""CPU restatement of the reference's E(3)-equivariant NVP flow (model_type "equivariant_nvp").  TEST INFRASTRUCTURE ONLY.

The coupling nets of modules/dense_equivariant_nvp.py, modules/layers/dense_equivariant_coupling_layer.py,
equivariant_features_basis.py and feature_processor.py in plain PyTorch (CPU, fp32), plugged into oracle/flow_oracle.py
without changing it: `installed()` substitutes `fo.scale_and_shift` for specs whose variant is "equivariant" and hands every
other spec to the original, so `fo.log_likelihood`, `fo.conditional_sample_with_logp` and `oracle.mh_oracle.OracleModel`
serve the equivariant model unchanged.  Pinned against the reference by tests/test_equivariant_cpu.py on the vectors
tools/gen_equivariant_golden.py wrote.  File:line citations are relative to the reference root.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from oracle import flow_oracle as fo

Tensor = torch.Tensor


@dataclass
class EquivariantFlowSpec(fo.FlowSpec):
    """equivariant_nvp (model_configs.py:40-48): no transformer; the MLP depth is read off the state dict."""

    variant: str = "equivariant"
    attention_type: str = "none"
    num_coupling_layers: int = 4
    num_transformer_layers: int = 0


def features_and_basis(positions: bool, x_features: Tensor, z_untransformed: Tensor, x_coords: Tensor, x_velocs: Tensor):
    """equivariant_features_basis.py:41-108 (ConditionalEquivariantCoordBasis: the coupling transforms velocities) and
    :111-172 (ConditionalEquivariantVelocityBasis: it transforms positions)."""
    x_rel = x_coords.unsqueeze(-2) - x_coords.unsqueeze(-3)                      # [B, V, V, 3], [b, i, j] = x_i - x_j
    x_rel_norm = torch.linalg.norm(x_rel, ord=2, dim=-1, keepdim=True)
    xv_norm = torch.linalg.norm(x_velocs, ord=2, dim=-1, keepdim=True)
    if positions:
        zv_norm = torch.linalg.norm(z_untransformed, ord=2, dim=-1, keepdim=True)
        relative_features = x_rel_norm
        pointwise_features = torch.cat((x_features, zv_norm, xv_norm), dim=-1)
        relative_basis = x_rel[:, :, :, None, :]
        pointwise_basis = torch.stack((z_untransformed, x_velocs), dim=-2)
    else:
        z_rel = z_untransformed.unsqueeze(-2) - z_untransformed.unsqueeze(-3)
        z_rel_norm = torch.linalg.norm(z_rel, ord=2, dim=-1, keepdim=True)
        relative_features = torch.cat((z_rel_norm, x_rel_norm), dim=-1)
        pointwise_features = torch.cat((x_features, xv_norm), dim=-1)
        relative_basis = torch.stack((z_rel, x_rel), dim=-2)
        pointwise_basis = x_velocs[:, :, None, :]
    return relative_features, pointwise_features, relative_basis, pointwise_basis


def feature_processor(sd: Dict[str, Tensor], prefix: str, relative_features: Tensor, pointwise_features: Tensor, masked: Tensor):
    """feature_processor.py:37-80."""
    v = pointwise_features.shape[-2]
    pi = pointwise_features.unsqueeze(-2).expand(-1, -1, v, -1)
    pj = pointwise_features.unsqueeze(-3).expand(-1, v, -1, -1)
    rel = fo.mlp(sd, f"{prefix}._relative_features_mlp", torch.cat((pi, pj, relative_features), dim=-1))
    rel = rel * ~masked[:, None, :, None]
    num_atoms = (~masked).sum(dim=-1)
    avg = rel.sum(-2) / num_atoms[:, None, None]
    pw = fo.mlp(sd, f"{prefix}._pointwise_features_mlp", torch.cat((pointwise_features, avg), dim=-1))
    return rel, pw


def shift_module(sd: Dict[str, Tensor], prefix: str, positions: bool, x_features, z_untransformed, x_coords, x_velocs, masked):
    """DenseEquivariantShiftModule.forward + _calc_shift (dense_equivariant_coupling_layer.py:97-194), the basis-axis
    broadcast of `pointwise_shift + relative_shift` included."""
    rf, pf, rb, pb = features_and_basis(positions, x_features, z_untransformed, x_coords, x_velocs)
    rf, pf = feature_processor(sd, f"{prefix}.feature_processor", rf, pf, masked)
    num_atoms = (~masked).sum(dim=-1)
    pointwise_shift = pb * fo.mlp(sd, f"{prefix}._shift_with_pointwise_mlp", pf)[..., None]
    relative_shift = rb * fo.mlp(sd, f"{prefix}._shift_with_relative_mlp", rf)[..., None]
    relative_shift = relative_shift * ~masked[:, None, :, None, None]
    relative_shift = relative_shift.sum(-3) / num_atoms[:, None, None, None]
    all_shifts = pointwise_shift + relative_shift
    return all_shifts.sum(dim=-2) / num_atoms[:, None, None]


def scale_module(sd: Dict[str, Tensor], prefix: str, positions: bool, x_features, z_untransformed, x_coords, x_velocs, masked):
    """DenseInvariantScaleModule.forward + _calc_scale (dense_equivariant_coupling_layer.py:324-400): log-scale [B, V, 1]."""
    rf, pf, _, _ = features_and_basis(positions, x_features, z_untransformed, x_coords, x_velocs)
    rf, pf = feature_processor(sd, f"{prefix}.feature_processor", rf, pf, masked)
    num_atoms = (~masked).sum(dim=-1)
    rel = fo.mlp(sd, f"{prefix}._scale_with_relative_mlp", rf) * ~masked[:, None, :, None]
    return fo.mlp(sd, f"{prefix}._scale_mlp",
                  fo.mlp(sd, f"{prefix}._scale_with_pointwise_mlp", pf) + rel.sum(-2) / num_atoms[:, None, None])


def equivariant_scale_and_shift(sd, spec, c: int, z_coords: Tensor, z_velocs: Tensor, x_features: Tensor, x_coords: Tensor,
                                x_velocs: Tensor, masked: Tensor, scores=None, trace: Optional[dict] = None):
    """dense_equivariant_nvp.py:23-68: scale = exp(log_scale) repeated over xyz."""
    positions = c % 2 == spec.position_layer_index_mod_2
    z_other = z_velocs if positions else z_coords
    pre = f"flow.chain.{c}"
    log_scale = scale_module(sd, f"{pre}.scale_module", positions, x_features, z_other, x_coords, x_velocs, masked)
    shift = shift_module(sd, f"{pre}.shift_module", positions, x_features, z_other, x_coords, x_velocs, masked)
    if trace is not None:
        trace[c] = (log_scale, shift)
    return torch.exp(log_scale).repeat(1, 1, 3), shift


@contextlib.contextmanager
def installed():
    """Within the block, oracle.flow_oracle evaluates EquivariantFlowSpec models with the restatement above."""
    original = fo.scale_and_shift

    def scale_and_shift(sd, spec, *args, **kwargs):
        if getattr(spec, "variant", None) == "equivariant":
            return equivariant_scale_and_shift(sd, spec, *args, **kwargs)
        return original(sd, spec, *args, **kwargs)

    fo.scale_and_shift = scale_and_shift
    try:
        yield
    finally:
        fo.scale_and_shift = original


def log_likelihood(sd, spec: EquivariantFlowSpec, *args) -> Tensor:
    with installed():
        return fo.log_likelihood(sd, spec, *args)


def conditional_sample_with_logp(sd, spec: EquivariantFlowSpec, *args):
    with installed():
        return fo.conditional_sample_with_logp(sd, spec, *args)
