"""`model_constructor(config) -> nn.Module`: the drop-in seam (reference model_constructor.py:51-76).

`config` may be this package's ModelConfig, the reference's own ModelConfig dataclass or an
OmegaConf node with the same fields (they are read by attribute).  Supported model types: the
transformer NVP flows on the sampling hot path, the E(3)-equivariant NVP flow and the Euler-Maruyama plumbing baseline; any other
`model_type` raises NotImplementedError exactly like the reference's final branch."""
from __future__ import annotations

import math
import os
from typing import Optional

import torch.nn as nn

from . import _lib
from .model_configs import duck_get as g
from .modules import layers as L
from .modules.baselines import EulerMaruyamaGaussian
from .modules.flow import PREFER_SINGLE_FP16, PREFER_SPLIT_FP16, ConditionalFlowDensityModel
from .weights import DENSE, EQUIVARIANT, KERNEL, LOCAL, FlowDims

ELEMENT_VOCAB = ("C", "H", "N", "O", "S")  # dataloader.py:24-25


def model_constructor(config) -> nn.Module:
    model_type = g(config, "model_type")
    if model_type == "custom_attention_transformer_nvp":
        sub = g(config, "custom_transformer_nvp_config")
        assert sub is not None
        return custom_transformer_nvp_constructor(sub)
    if model_type == "transformer_nvp":
        sub = g(config, "transformer_nvp_config")
        assert sub is not None
        return transformer_nvp_constructor(sub)
    if model_type == "equivariant_nvp":
        sub = g(config, "equivariant_nvp_config")
        if sub is None:
            raise NotImplementedError("equivariant_nvp: the equivariant_nvp_config sub-config is missing")
        return equivariant_nvp_constructor(sub)
    if model_type == "euler_maruyama_gaussian":
        return EulerMaruyamaGaussian()
    raise NotImplementedError(f"{model_type} is not a recognised model.")


_PATH_NAMES = {"auto": _lib.TW_PATH_AUTO, "f32": _lib.TW_PATH_FUSED, "simple": _lib.TW_PATH_SIMPLE, "simple_h3": _lib.TW_PATH_SIMPLE_H3,
               "h3": PREFER_SPLIT_FP16, "split_fp16": PREFER_SPLIT_FP16,
               # opt-in fast mode: one fp16 MFMA per product (~1e-4 relative deviation from the reference; not a parity path)
               "h1": PREFER_SINGLE_FP16, "fast": PREFER_SINGLE_FP16}


def default_execution_path() -> int:
    """Execution path of models built without an explicit one: the environment variable TW_EXECUTION_PATH
    (h3 | auto | f32 | simple), so that unmodified reference scripts can choose the kernel family.  Unset means "h3":
    the split-fp16 MFMA kernel - the one bench.py measures - wherever it applies, decided per call, and the exact-fp32
    kernels (the C ABI's TW_PATH_AUTO) for every other molecule size / attention type.  It holds the same 1e-5 parity
    tests as the fp32 kernels; its operands are fp16, so activations beyond +-65504 are reported (tw_flow_nonfinite,
    model.check_finite()) with a pointer to TW_EXECUTION_PATH=f32 rather than sampled through."""
    name = os.environ.get("TW_EXECUTION_PATH", "h3").strip().lower()
    if name not in _PATH_NAMES:
        raise ValueError(f"TW_EXECUTION_PATH={name!r}: expected one of {sorted(_PATH_NAMES)}")
    return _PATH_NAMES[name]


def _density_flags(cfg):
    cfd = g(cfg, "conditional_flow_density")
    return (
        bool(g(cfd, "scale_requires_grad", True)),
        bool(g(cfd, "ignore_conditional_velocity", False)),
        bool(g(cfd, "use_displacement_as_target", True)),
    )


def _single_hidden(cfg) -> int:
    hidden = list(g(cfg, "latent_mlp_hidden_dims"))
    if len(hidden) != 1:
        raise NotImplementedError("the HIP path supports exactly one hidden layer in in_mlp/out_mlp "
                                  f"(every reference config uses [256]); got {hidden}")
    return int(hidden[0])


def custom_transformer_nvp_constructor(config, execution_path: Optional[int] = None) -> ConditionalFlowDensityModel:
    """custom_transformer_nvp_constructor (model_constructor.py:153-197): kernel attention (Gaussian, learnable-lengthscale or
    Chebyshev basis) or local attention."""
    n_coupling = int(g(config, "num_coupling_layers"))
    assert n_coupling % 2 == 0, "Real NVP should have an even number of coupling layers"
    pos_mod = int(g(config, "position_layer_index_mod_2", 0))
    assert pos_mod in (0, 1), "positions_layer_index can only be 0 or 1"
    enc = g(config, "encoder_layer_config")
    attention_type = g(enc, "attention_type")
    if attention_type == "local":
        return _local_transformer_nvp(config, n_coupling, pos_mod, enc, execution_path)
    if attention_type not in ("kernel", "learnable_kernel", "chebyshev_kernel"):
        raise NotImplementedError(
            f"attention_type '{attention_type}' is outside the HIP hot path ('kernel', 'learnable_kernel', 'chebyshev_kernel', 'local')")
    cheb_order, cheb_zero = 0, False
    if attention_type == "chebyshev_kernel":
        cheb_order = int(g(enc, "cheb_order"))
        assert cheb_order >= 1
        assert g(enc, "force_asymptotic_zero") is not None
        cheb_zero = bool(g(enc, "force_asymptotic_zero"))
    att_cls = {"kernel": L.KernelAttention, "learnable_kernel": L.LearnableLengthscaleKernelAttention}.get(attention_type)
    lengthscales = list(g(enc, "lengthscales"))
    assert len(lengthscales) > 0
    normalise = g(enc, "normalise_kernel_values")
    assert normalise is not None
    d_model, d_ff = int(g(enc, "d_model")), int(g(enc, "dim_feedforward"))
    if float(g(enc, "dropout", 0.0)) != 0.0:
        raise NotImplementedError("dropout must be 0 for sampling (stochastic likelihood otherwise)")
    emb = int(g(config, "atom_embedding_dim"))
    hidden = _single_hidden(config)
    n_layers = int(g(config, "num_transformer_layers"))
    H = len(lengthscales)  # the number of heads is the number of lengthscales (custom_attention_encoder.py:165-168)

    def encoder_layer():
        if attention_type == "chebyshev_kernel":
            att = L.LearnableChebyshevKernelAttention(
                value_dim=d_model, output_dim=d_model, lengthscales=lengthscales, cheb_order=cheb_order,
                normalise_kernel_values=bool(normalise), force_asymptotic_zero=cheb_zero)
        else:
            att = att_cls(value_dim=d_model, output_dim=d_model, lengthscales=lengthscales,
                          normalise_kernel_values=bool(normalise))
        sa = L.KernelSelfAttention(input_dim=d_model, num_heads=H, value_dim=d_model, attention=att)
        return L.CustomTransformerEncoderLayer(d_model=d_model, self_attention=sa, dim_feedforward=d_ff)

    def block():
        return L.CustomAttentionTransformerBlock(emb + 9, 3, [hidden], [encoder_layer() for _ in range(n_layers)])

    chain = [
        L.CouplingLayer("positions" if i % 2 == pos_mod else "velocities", block(), block())
        for i in range(n_coupling)
    ]
    flow = L.ConditionalSequentialFlow(chain, nn.Embedding(len(ELEMENT_VOCAB), emb))
    srg, icv, disp = _density_flags(config)
    # normalise = True whatever the config says: KernelAttention.forward (kernel_attention.py:197-206, inherited by the
    # learnable-lengthscale and Chebyshev classes) never hands `normalise_kernel_values` to
    # compute_kernel_attention_scores, whose default is True (:75) - reference models always L1-normalise.  The flag
    # stays on the attention modules as an attribute, as in the reference (golden kernel_nonorm_tiny.npz).
    dims = FlowDims(KERNEL, n_coupling, n_layers, d_model, d_ff, hidden, emb, H, 0, len(ELEMENT_VOCAB), pos_mod,
                    disp, icv, True, 1e-5, learnable_lengthscales=attention_type == "learnable_kernel", cheb_order=cheb_order, cheb_force_zero=cheb_zero)
    path = default_execution_path() if execution_path is None else execution_path
    return ConditionalFlowDensityModel(flow, dims, scale_requires_grad=srg, execution_path=path)


def _local_transformer_nvp(config, n_coupling: int, pos_mod: int, enc, execution_path: Optional[int]) -> ConditionalFlowDensityModel:
    """attention_type 'local' (custom_attention_encoder.py:140-153): LocalSelfAttention with num_heads heads of
    key / query / value width d_model each, softmax over the atoms within max_radius (nm) of the query's conditioning
    position.  The per-op kernels serve it at every molecule size (TW_PATH_SIMPLE, TW_PATH_SIMPLE_H3): the default
    split-fp16 preference resolves to TW_PATH_SIMPLE_H3, auto / f32 to TW_PATH_SIMPLE."""
    max_radius = g(enc, "max_radius")
    assert max_radius is not None
    max_radius = float(max_radius)
    if not (math.isfinite(max_radius) and max_radius > 0.0):
        raise ValueError(f"local attention: max_radius must be finite and positive, got {max_radius}")
    H = int(g(enc, "num_heads"))
    assert H > 0
    d_model, d_ff = int(g(enc, "d_model")), int(g(enc, "dim_feedforward"))
    if float(g(enc, "dropout", 0.0)) != 0.0:
        raise NotImplementedError("dropout must be 0 for sampling (stochastic likelihood otherwise)")
    emb = int(g(config, "atom_embedding_dim"))
    hidden = _single_hidden(config)
    n_layers = int(g(config, "num_transformer_layers"))

    def encoder_layer():
        sa = L.LocalSelfAttention(input_dim=d_model, output_dim=d_model, num_heads=H, value_dim=d_model,
                                  key_query_dim=d_model, max_radius=max_radius)
        return L.CustomTransformerEncoderLayer(d_model=d_model, self_attention=sa, dim_feedforward=d_ff)

    def block():
        return L.CustomAttentionTransformerBlock(emb + 9, 3, [hidden], [encoder_layer() for _ in range(n_layers)])

    chain = [
        L.CouplingLayer("positions" if i % 2 == pos_mod else "velocities", block(), block())
        for i in range(n_coupling)
    ]
    flow = L.ConditionalSequentialFlow(chain, nn.Embedding(len(ELEMENT_VOCAB), emb))
    srg, icv, disp = _density_flags(config)
    dims = FlowDims(LOCAL, n_coupling, n_layers, d_model, d_ff, hidden, emb, H, 0, len(ELEMENT_VOCAB), pos_mod, disp, icv,
                    True, 1e-5, max_radius=max_radius)
    path = default_execution_path() if execution_path is None else execution_path
    return ConditionalFlowDensityModel(flow, dims, scale_requires_grad=srg, execution_path=path)


def equivariant_nvp_constructor(config, execution_path: Optional[int] = None) -> ConditionalFlowDensityModel:
    """equivariant_nvp_constructor (model_constructor.py:103-150): coupling layers of a dense E(3)-equivariant shift module
    and an invariant scale module, each with its own FeatureProcessor; the atom embedding width is also the width of the
    processed features.  Runs on the exact-f32 per-op kernels (TW_PATH_SIMPLE) at every molecule size."""
    n_coupling = int(g(config, "num_coupling_layers"))
    assert n_coupling % 2 == 0, "Real NVP should have an even number of coupling layers"
    hidden = g(config, "latent_mlp_hidden_dims")
    assert hidden is not None
    hidden = [int(h) for h in hidden]
    pos_mod = int(g(config, "position_layer_index_mod_2", 0))
    assert pos_mod in (0, 1), "positions_layer_index can only be 0 or 1"
    emb = int(g(config, "atom_embedding_dim"))
    if not (1 <= len(hidden) <= 3 and len(set(hidden)) == 1 and hidden[0] % 8 == 0 and hidden[0] <= 256 and 1 <= emb <= 64):
        raise NotImplementedError("the HIP equivariant flow supports 1 to 3 hidden layers of one width (a multiple of 8, at most "
                                  f"256) and an embedding of at most 64; got latent_mlp_hidden_dims={hidden}, "
                                  f"atom_embedding_dim={emb}")
    chain = []
    for i in range(n_coupling):
        tv = "positions" if i % 2 == pos_mod else "velocities"
        chain.append(L.EquivariantCouplingLayer(tv, L.DenseEquivariantShiftModule(tv, emb, hidden),
                                                L.DenseInvariantScaleModule(tv, emb, hidden)))
    flow = L.ConditionalSequentialFlow(chain, nn.Embedding(len(ELEMENT_VOCAB), emb))
    srg, icv, disp = _density_flags(config)
    dims = FlowDims(EQUIVARIANT, n_coupling, 0, 0, 0, hidden[0], emb, 0, 0, len(ELEMENT_VOCAB), pos_mod, disp, icv, True, 1e-5,
                    n_hidden=len(hidden))
    path = default_execution_path() if execution_path is None else execution_path
    return ConditionalFlowDensityModel(flow, dims, scale_requires_grad=srg, execution_path=path)


def transformer_nvp_constructor(config, execution_path: Optional[int] = None) -> ConditionalFlowDensityModel:
    """transformer_nvp_constructor (model_constructor.py:200-238): dense softmax attention."""
    n_coupling = int(g(config, "num_coupling_layers"))
    assert n_coupling % 2 == 0, "Real NVP should have an even number of coupling layers"
    pos_mod = int(g(config, "position_layer_index_mod_2", 0))
    assert pos_mod in (0, 1), "positions_layer_index can only be 0 or 1"
    tc = g(config, "transformer_config")
    n_head, d_ff = int(g(tc, "n_head", 8)), int(g(tc, "dim_feedforward", 2048))
    dropout = float(g(tc, "dropout", 0.0))
    if dropout != 0.0:
        raise NotImplementedError("dropout must be 0 for sampling (stochastic likelihood otherwise)")
    rff = g(config, "rff_position_encoder_config")
    enc_dim = int(g(rff, "encoding_dim", 0)) if rff is not None else 0
    scale_mean = float(g(rff, "scale_mean", 1.0)) if rff is not None else 1.0
    scale_std = float(g(rff, "scale_stddev", 1.0)) if rff is not None else 1.0
    emb = int(g(config, "atom_embedding_dim"))
    d_model = int(g(config, "transformer_hidden_dim"))
    hidden = _single_hidden(config)
    n_layers = int(g(config, "num_transformer_layers"))

    def block():
        return L.TransformerBlock(emb + 9 + enc_dim, 3, d_model, [hidden], n_layers, n_head, d_ff, dropout)

    chain = [
        L.CouplingLayer("positions" if i % 2 == pos_mod else "velocities", block(), block(),
                        position_encoder=L.RFFPositionEncoder(3, enc_dim, scale_mean, scale_std))
        for i in range(n_coupling)
    ]
    flow = L.ConditionalSequentialFlow(chain, nn.Embedding(len(ELEMENT_VOCAB), emb))
    srg, icv, disp = _density_flags(config)
    dims = FlowDims(DENSE, n_coupling, n_layers, d_model, d_ff, hidden, emb, n_head, enc_dim, len(ELEMENT_VOCAB),
                    pos_mod, disp, icv, True, 1e-5)
    path = default_execution_path() if execution_path is None else execution_path
    return ConditionalFlowDensityModel(flow, dims, scale_requires_grad=srg, execution_path=path)
