/*
 * timewarp_hip.h -- C ABI of libtimewarp_hip.so: the MI355X (gfx950) implementation of
 * Timewarp's conditional-flow sampling hot path.
 *
 * The reference (microsoft/timewarp) is pure Python/PyTorch: it has no FFI of its own, so the
 * "binding" a maintainer adds is a ctypes stub (INTEGRATION.md shows it).  Each entry point below
 * names the reference function (file:line under the reference root) whose torch-op chain it
 * replaces.  Conventions:
 *
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it says "host";
 *   - all float tensors are contiguous fp32, index tensors int32, masks uint8 (1 = masked);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); nothing synchronises the host;
 *   - return value: 0 on success, a negative tw_status otherwise; tw_last_error() gives the
 *     message of the last failure on the calling thread.  No entry point allocates or frees
 *     caller memory; workspaces are caller-provided (tw_flow_workspace_bytes);
 *   - thread-safety: the compute entry points are re-entrant across streams.  Process-wide state: the per-thread error
 *     string; the debug / measurement word of tw_debug_set_flags (one atomic int, read once per launch: set it while no
 *     other thread launches); the profile hooks (tw_profile_begin / tw_profile_end, not thread-safe); the sticky
 *     per-device non-finite flag of tw_flow_nonfinite (used by descriptors whose range_flag is NULL; since ABI 7 a
 *     descriptor can carry its caller's own word instead); tw_mh_iteration keeps one helper stream and two events per device
 *     and calling thread, created on first use.
 */
#ifndef TIMEWARP_HIP_H
#define TIMEWARP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TW_ABI_VERSION 8

typedef enum {
  TW_OK = 0,
  TW_ERR_INVALID = -1,   /* bad argument / unsupported shape */
  TW_ERR_HIP = -2,       /* a HIP runtime call failed */
  TW_ERR_WORKSPACE = -3, /* workspace too small */
  TW_ERR_NO_DEVICE = -4  /* no gfx950 device visible */
} tw_status;

/* Hyper-parameters of one flow (model_configs.py:51-76, custom_attention_encoder.py:126-137,
 * transformer_block.py:11-15).  kernel variant: n_heads = len(lengthscales), value_dim = d_model.  local variant: n_heads from
 * the config, key / query / value width d_model per head (custom_attention_encoder.py:140-153). */
typedef struct {
  int32_t variant;      /* 0 = kernel (custom_attention_transformer_nvp), 1 = dense (transformer_nvp), 2 = local
                           (custom_attention_transformer_nvp with attention_type "local": softmax attention over the keys within
                           max_radius of the query's conditioning position, local_self_attention.py:14-117; TW_PATH_SIMPLE and
                           TW_PATH_SIMPLE_H3 only - no fused layout, no packed stream), 3 = equivariant (equivariant_nvp: the
                           dense E(3)-equivariant coupling nets of dense_equivariant_coupling_layer.py; TW_PATH_SIMPLE only, which
                           TW_PATH_AUTO resolves to - the fused paths, every pack and TW_PATH_SIMPLE_H3 refuse it.  It reads
                           n_coupling, d_emb (atom_embedding_dim <= 64, also the width of the processed features), d_hidden
                           (width of every hidden layer: a multiple of 8, <= 256), n_hidden, n_elements, pos_mod2, displacement,
                           ignore_cond_velocity and range_flag; n_layers, d_model, d_ff, n_heads, d_rff and cheb_order MUST be 0;
                           normalise, ln_eps, cheb_force_zero and max_radius are ignored) */
  int32_t n_coupling;   /* 8 */
  int32_t n_layers;     /* 3 encoder layers per net */
  int32_t d_model;      /* 128 */
  int32_t d_ff;         /* 2048 */
  int32_t d_hidden;     /* 256: the single hidden layer of in_mlp / out_mlp */
  int32_t d_emb;        /* 32 */
  int32_t n_heads;      /* 6 (kernel) / 8 (dense) */
  int32_t d_rff;        /* dense only: RFF encoding dims (0 in transformer_nvp.yaml) */
  int32_t n_elements;   /* 5 = len(ELEMENT_VOCAB) */
  int32_t pos_mod2;     /* position_layer_index_mod_2 */
  int32_t displacement; /* use_displacement_as_target */
  int32_t ignore_cond_velocity;
  int32_t normalise;    /* normalise_kernel_values */
  float ln_eps;         /* 1e-5 */
  int32_t cheb_order;   /* kernel variant: 0 = Gaussian basis exp(-s^2) (attention_type "kernel"/"learnable_kernel");
                           > 0 = attention_type "chebyshev_kernel": rational Chebyshev expansion of that order of s^2
                           with per-layer coefficients (kernel_attention.py:12-66, 255-339); all execution paths (the
                           fused kernels take one score-fragment set per (net, layer) of the coupling layer in flight) */
  int32_t cheb_force_zero; /* force_asymptotic_zero: subtract each head's mean coefficient */
  int32_t* range_flag;  /* ABI 7 - split-fp16 range guard, per model / per call: DEVICE pointer to a caller-owned int32
                           (zeroed by the caller) that the flow kernels OR to 1 when a coupling net returns a non-finite
                           scale or shift; every entry point that takes this descriptor reports there.  NULL: the
                           per-device word of tw_flow_nonfinite (two models on one device then share one flag). */
  float max_radius;     /* local variant only (read only when variant == 2; finite, > 0): nm; key m is a neighbour of query q
                           iff neither is masked and |x_q - x_m| < max_radius in fp32 (torch.cdist's direct form) */
  int32_t n_hidden;     /* equivariant variant only (read only when variant == 3): hidden layers per MLP, 1 .. 3 - the length of
                           latent_mlp_hidden_dims, whose entries all equal d_hidden (equivariant_nvp.yaml: [256, 256]) */
} tw_flow_desc;

const char* tw_last_error(void);
int tw_abi_version(void);
/* Number of gfx950 devices visible (0 on a CPU-only box; never fails). */
int tw_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * Weights.  The host packs the reference state_dict (SURVEY.md section 8b names) into ONE flat fp32
 * device buffer in the canonical order documented in DESIGN.md ("raw layout"):
 *   embedding[n_elements,d_emb], lengthscales[2,n_heads] (kernel only; row 0 is used by forward passes, row 1 by
 *   reverse passes - equal unless the lengthscales are learnable, see timewarp_amd/weights.py), prior log-scales[2],
 *   then for c in coupling layers, net in (scale, shift):  [dense: rff vectors[3,d_rff/2] once per c]
 *     in_mlp.0.{w[d_hidden,d_in],b}, in_mlp.2.{w[d_model,d_hidden],b},
 *     per layer: kernel: values_proj.w[H*d_model,d_model], out_projection.w[d_model,H*d_model],
 *                        [cheb_coeffs[H,cheb_order] when cheb_order > 0]
 *                dense : in_proj.{w[3d,d],b[3d]}, out_proj.{w[d,d],b[d]}
 *                local : qkv_proj.w[3*H*d_model,d_model] (per head h: rows of q, then k, then v), output_proj.w[d_model,H*d_model]
 *                linear1.{w,b}, linear2.{w,b}, norm1.{w,b}, norm2.{w,b}
 *     out_mlp.0.{w[d_hidden,d_model],b}, out_mlp.2.{w[3,d_hidden],b}
 * equivariant variant: embedding[n_elements,d_emb], prior log-scales[2], then for c in coupling layers, module in (scale_module,
 *   shift_module) the MLPs feature_processor._relative_features_mlp (2P+R -> E), feature_processor._pointwise_features_mlp
 *   (P+E -> E), _{scale,shift}_with_pointwise_mlp (E -> E | n_pw), _{scale,shift}_with_relative_mlp (E -> E | n_rel) and, scale
 *   only, _scale_mlp (E -> 1); an MLP is n_hidden + 1 layers {w[out,in], b[out]} with d_hidden-wide hidden layers.  E = d_emb;
 *   a coupling that transforms positions (c % 2 == pos_mod2) has P = E + 2, R = 1, n_pw = 2, n_rel = 1, one that transforms
 *   velocities P = E + 1, R = 2, n_pw = 1, n_rel = 2.  Every tensor of this variant with at least one axis (each w, each b, the
 *   embedding) starts at a multiple of 4 floats (zero padding in front of it), so that weight rows can be read 16 bytes at a time.
 * tw_flow_raw_floats returns the total so the host can check its packing.
 * ------------------------------------------------------------------------------------------- */
int64_t tw_flow_raw_floats(const tw_flow_desc* desc);
/* The pack entry points below (tw_flow_pack, _h3, _simple_h3, _h1) return after `stream` has completed: they synchronise it
 * (packing is one-time set-up, not something to capture into a graph). */
/* Size (floats) of the MFMA-fragment-ordered weight stream used by the fused kernel path
 * (kernel variant only; 0 for dense). */
int64_t tw_flow_packed_floats(const tw_flow_desc* desc);
/* Builds the fused-path weight stream from the raw buffer on the device (folds
 * W_o[:,h] @ W_v[h] per head in fp64, re-tiles every matrix into 16x16 MFMA A-fragments). */
int tw_flow_pack(const tw_flow_desc* desc, const float* raw, float* packed, void* stream);

/* The split-fp16 weight stream of TW_PATH_FUSED_H3: size in BYTES (0 if unsupported) and builder
 * (per-matrix power-of-two scaling, fp16 hi/lo tile pairs in LDS-DMA stage order). */
int64_t tw_flow_packed_h3_bytes(const tw_flow_desc* desc);
int tw_flow_pack_h3(const tw_flow_desc* desc, const float* raw, void* packed_h3, void* stream);
/* ABI 8 - the pack of TW_PATH_SIMPLE_H3 (0 bytes where the model has no split-fp16 stream: that path then takes packed = NULL):
 * the tw_flow_pack_h3 stream (its FFN stages feed the path's fused FFN launches), then - kernel attention - the per-head folded
 * value / output projections Wc[coupling][net][layer][d_model][n_heads d_model] (fp32, folded in fp64) and their split-fp16 copies
 * per head in MFMA-operand order, which let the mixing run on the layer input with the ONE remaining GEMM inside the same launch; then
 * the FFN stages of every (coupling, net, layer) once more as four self-contained streams of a quarter of the hidden layer each (small
 * launches spread an FFN over four workgroups per token tile). */
int64_t tw_flow_packed_simple_h3_bytes(const tw_flow_desc* desc);
int tw_flow_pack_simple_h3(const tw_flow_desc* desc, const float* raw, void* packed, void* stream);
/* The same for TW_PATH_FUSED_H1 (fp16 hi tiles only: 8 tiles per 9 KiB stage, half as many stages). */
int64_t tw_flow_packed_h1_bytes(const tw_flow_desc* desc);
int tw_flow_pack_h1(const tw_flow_desc* desc, const float* raw, void* packed_h1, void* stream);

/* Bytes of scratch the flow entry points need for n_rows conformations of n_atoms atoms.  (The per-op paths run the two nets of a
 * coupling layer side by side - the second on a library-owned side stream that waits for and is waited for by `stream` through
 * events, so the caller sees ordinary stream order - and size the scratch for two sets of activations.) */
int64_t tw_flow_workspace_bytes(const tw_flow_desc* desc, int64_t n_rows, int32_t n_atoms);

/* Execution path selector for the flow entry points. */
#define TW_PATH_AUTO 0   /* fused MFMA path where supported, else simple */
#define TW_PATH_FUSED 1  /* fused f32-MFMA net-block kernel (kernel variant, n_atoms <= 64) */
#define TW_PATH_SIMPLE 2 /* one plain HIP kernel per reference op (all variants) */
#define TW_PATH_FUSED_H3 3 /* fused split-fp16 kernel: every fp32 product as 3 half-precision MFMAs with fp32
                              accumulation (2^-22 operand representation); needs |activations| < 65504.  Kernel
                              attention: n_atoms <= 48 in 48-token waves holding floor(48 / n_atoms) molecules, and
                              25 .. 192 atoms in the "wide" layout - floor(192 / n_atoms) molecules packed over a workgroup's
                              four waves (81 .. 95 atoms: two, at a slot stride of 96) - chosen per launch where both exist (fewer rounds of
                              the chip); dense softmax attention: n_atoms <= 48.  tw_flow_path_supported answers per size.
                              `packed` must then point at the tw_flow_pack_h3 stream.  Never chosen by
                              TW_PATH_AUTO. */
#define TW_PATH_FUSED_H1 4 /* "fast" mode, NOT a parity path: the same fused kernel with ONE half-precision MFMA per
                              product (fp16 operands, 11 significand bits, fp32 accumulation) and half the weight stream.
                              Kernel attention, every molecule size TW_PATH_FUSED_H3 takes (48-token waves and the wide
                              layout); the dense softmax model up to 48 atoms too (its in / FFN / out
                              sections - 88 % of the work - run single-MFMA, the softmax attention block stays in
                              split form; with position features the in-MLP as well).  Results deviate from the reference's fp32 arithmetic by
                              ~1e-4 relative (measured per case in tests/test_flow_h1_gpu.py); proposal and reverse-move
                              densities of an MH iteration are evaluated by the same arithmetic.  `packed` must point at
                              the tw_flow_pack_h1 stream.  Only ever chosen by name. */
#define TW_PATH_SIMPLE_H3 5 /* ABI 8: TW_PATH_SIMPLE with its linear layers (in / out MLPs, value and output projections, q / k / v,
                              FFN) as split-fp16 MFMA GEMMs - the arithmetic of TW_PATH_FUSED_H3 (3 half-precision MFMAs per fp32
                              product, fp32 accumulation), one kernel per reference op, ANY molecule size and both model variants:
                              what serves the sizes no fused layout takes (kernel attention above 192 atoms, dense above 64) at 2-4x
                              the rate of the exact-f32 per-op kernels.  Scores, softmax, LayerNorm stay fp32.  Needs
                              |activations| < 65504 and |weights| < 256 (else non-finite outputs -> range flag).  `packed`: NULL, or
                              the tw_flow_pack_simple_h3 buffer where that exists (d_model 128) - the FFN of every encoder layer
                              and the in / out MLPs then run as ONE launch each of the fused kernels' statements on the flat token
                              list (hidden layer on chip) instead of two GEMMs through HBM, and kernel attention mixes the layer
                              input itself with the one folded 768 -> 128 GEMM inside the mixing launch. */

/* 1 if `path` can run this configuration on molecules of n_atoms atoms (TW_PATH_AUTO / TW_PATH_SIMPLE / TW_PATH_SIMPLE_H3: always), else 0.
 * What a caller asks before it requests TW_PATH_FUSED / TW_PATH_FUSED_H3 by name (those fail with TW_ERR_INVALID on an
 * unsupported shape instead of falling back). */
int tw_flow_path_supported(const tw_flow_desc* desc, int32_t n_atoms, int32_t path);

/* ConditionalSequentialFlow.forward (modules/model_wrappers/flow.py:51-103) over
 * NVPCouplingLayer.forward (modules/layers/nvp.py:22-183) with
 * CustomAttentionTransformerCouplingLayer._get_scale_and_shift (modules/custom_transformer_nvp.py:44-93)
 * or TransformerCouplingLayer (modules/transformer_nvp.py:58-97).
 *   x_coords/x_velocs/atom_types/masked: [n_cond, n_atoms, ...] conditioning rows; row n of z uses
 *   conditioning row n % n_cond (the reference's .repeat(S,1,1) tiling, flow.py:284-296).
 *   z_coords/z_velocs [n_rows,n_atoms,3] and delta_logp [n_rows] are updated in place.
 *   x_coords must already be centred (flow.py:156-157 / 261-262).  `packed` may be NULL for
 *   TW_PATH_SIMPLE. */
int tw_flow_pass(const tw_flow_desc* desc, const float* raw, const float* packed,
                 const int32_t* atom_types, const float* x_coords, const float* x_velocs,
                 const uint8_t* masked, int64_t n_cond, float* z_coords, float* z_velocs,
                 float* delta_logp, int64_t n_rows, int32_t n_atoms, int32_t reverse, int32_t path,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* ConditionalFlowDensityModel.log_likelihood (modules/model_wrappers/flow.py:131-215).
 * All inputs [n_rows,n_atoms,(3)]; out_logp [n_rows]. */
int tw_flow_log_likelihood(const tw_flow_desc* desc, const float* raw, const float* packed,
                           const int32_t* atom_types, const float* x_coords, const float* x_velocs,
                           const float* y_coords, const float* y_velocs, const uint8_t* masked,
                           float* out_logp, int64_t n_rows, int32_t n_atoms, int32_t path,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* ConditionalFlowDensityModel.conditional_sample_with_logp (flow.py:242-336) with the latent
 * noise passed in: z_* [n_samples,n_cond,n_atoms,3] ALREADY multiplied by exp(prior log-scale)
 * (the reference draws Normal(0,scale).rsample((S,)), coords first, flow.py:274-275).
 * Outputs y_* [n_samples,n_cond,n_atoms,3], out_logp [n_samples,n_cond].  The reference's mask
 * broadcast (flow.py:326) only works for n_cond == 1 or n_samples == 1; same restriction here. */
int tw_flow_sample_with_logp(const tw_flow_desc* desc, const float* raw, const float* packed,
                             const int32_t* atom_types, const float* x_coords,
                             const float* x_velocs, const uint8_t* masked, const float* z_coords,
                             const float* z_velocs, float* y_coords, float* y_velocs,
                             float* out_logp, int64_t n_samples, int64_t n_cond, int32_t n_atoms,
                             int32_t path, void* workspace, int64_t workspace_bytes, void* stream);

/* Extension: the same without the reference's n_cond == 1 || n_samples == 1 restriction (flow.py:326 broadcasts a
 * [B,V,1] mask into [S*B,V,3]); rows are ordered sample-major, row = sample * n_cond + cond, as the reference's
 * reshape would produce.  Used to evaluate several chains' proposals in one launch. */
int tw_flow_sample_with_logp_multi(const tw_flow_desc* desc, const float* raw, const float* packed,
                                   const int32_t* atom_types, const float* x_coords,
                                   const float* x_velocs, const uint8_t* masked,
                                   const float* z_coords, const float* z_velocs, float* y_coords,
                                   float* y_velocs, float* out_logp, int64_t n_samples, int64_t n_cond,
                                   int32_t n_atoms, int32_t path, void* workspace,
                                   int64_t workspace_bytes, void* stream);

/* compute_kernel_attention_scores (modules/layers/kernel_attention.py:69-121):
 * out [n_cond, n_heads, n_atoms, n_atoms].  use_mm != 0 selects torch.cdist's matmul
 * formulation (the reference gets it for n_atoms > 25). */
int tw_kernel_scores(const float* x_coords, const uint8_t* masked, const float* lengthscales,
                     int32_t n_heads, int64_t n_cond, int32_t n_atoms, int32_t normalise,
                     int32_t use_mm, float* out, void* stream);

/* Same with the learnable rational-Chebyshev basis (chebyshev_basis_function / chebyshev_expansion,
 * kernel_attention.py:12-66):  score = sum_c coeff[h,c] R_c(s^2),  R_0 = 1, R_1 = (x-1)/(x+1),
 * R_{n+1} = 2 R_1 R_n - R_{n-1};  cheb_coeffs [n_heads, cheb_order];  force_zero subtracts each head's mean
 * coefficient (force_asymptotic_zero). */
int tw_kernel_scores_cheb(const float* x_coords, const uint8_t* masked, const float* lengthscales,
                          const float* cheb_coeffs, int32_t cheb_order, int32_t force_zero, int32_t n_heads,
                          int64_t n_cond, int32_t n_atoms, int32_t normalise, int32_t use_mm, float* out,
                          void* stream);

/* get_centre_of_mass (utils/molecule_utils.py:15-29): out_centred = x - masked mean,
 * out_com [n_rows,3] (either output may be NULL).  An all-masked row is 0 / 0 = NaN, as in the reference.
 * n_rows == 0 launches nothing; n_rows < 0 and n_atoms <= 0 are refused by name (-1, nothing queued or written). */
int tw_centre(const float* x_coords, const uint8_t* masked, float* out_centred, float* out_com,
              int64_t n_rows, int32_t n_atoms, void* stream);

/* compute_kinetic_energy (utils/evaluation_utils.py:416-436):
 * random_velocs ? 0.5*sum v^2 : 0.5*sum m v^2 / kbT.  masses [n_atoms] (may be NULL when random_velocs); out [n_rows].
 * n_rows == 0 launches nothing; n_rows < 0 and n_atoms <= 0 are refused by name. */
int tw_kinetic_energy(const float* velocs, const float* masses, int32_t random_velocs, float kbT,
                      float* out, int64_t n_rows, int32_t n_atoms, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Potential energy: replaces OpenmmPotentialEnergyTorch.forward
 * (utils/openmm/openmm_bridge.py:281-294 -> bgflow -> OpenMM Context.getState(getEnergy)) for a
 * System built by simulation/md.py:128-187 (HarmonicBond, HarmonicAngle, PeriodicTorsion,
 * Nonbonded CutoffNonPeriodic with reaction field, GBSAOBC).  Parameter tables are what
 * system.getForces() exposes (INTEGRATION.md has the extractor).  Units nm / kJ/mol / e.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_atoms;
  int32_t n_bonds;      /* bond_idx [n_bonds,2] int32,  bond_par [n_bonds,2] = (r0, k)          */
  int32_t n_angles;     /* angle_idx [n_angles,3],      angle_par [n_angles,2] = (theta0, k)    */
  int32_t n_torsions;   /* torsion_idx [n_torsions,4],  torsion_par [n_torsions,3] = (n, phase, k) */
  int32_t n_exceptions; /* exc_idx [n_exceptions,2],    exc_par [n_exceptions,3] = (qq, sigma, eps); 1-2/1-3 have zeros */
  int32_t has_gbsa;     /* 0: no implicit solvent; 1: GBSA-OBC II (GBSAOBCForce, amber99_obc.xml); 2: GBSA-OBC I (obc1.xml) */
  double cutoff;        /* nonbondedCutoff (nm); <= 0 means NoCutoff */
  double rf_dielectric; /* reaction-field dielectric (78.3 default; OpenMM uses 1.0 when GBSA is present) */
  double solute_dielectric, solvent_dielectric; /* GBSA: 1.0 / 78.5 */
  double surface_area_energy;                   /* GBSA ACE term coefficient, 2.25936 kJ/mol/nm^2 */
  const int32_t* bond_idx;    const double* bond_par;
  const int32_t* angle_idx;   const double* angle_par;
  const int32_t* torsion_idx; const double* torsion_par;
  const int32_t* exc_idx;     const double* exc_par;
  const double* atom_par;     /* [n_atoms,5] = (charge, sigma, epsilon, gb_radius, gb_scale) */
} tw_forcefield;

/* coords [n_rows,n_atoms,3] fp32 (nm) -> out_energy [n_rows] fp64 kJ/mol (fp64 like the bridge's
 * numpy round trip, openmm_bridge.py:206-221).  All tw_forcefield pointers are device pointers.
 * out_terms, if not NULL, receives [n_rows,5] = bond, angle, torsion, nonbonded, gbsa
 * (the decomposition of simulation/md.py:288-413).  One conformation per workgroup (four waves up to 64 atoms, sixteen above; the
 * force / Langevin kernels one / sixteen), coordinates and the pair-exclusion bit matrix in LDS: molecules up to ~1000 atoms (TW_ERR_INVALID beyond what 160 KiB hold; the force / Langevin entry points
 * below ~850 / ~800). */
int tw_amber_energy(const tw_forcefield* ff, const float* coords, double* out_energy,
                    double* out_terms, int64_t n_rows, void* stream);

/* Forces of the same potential (kJ/mol/nm, fp64): out_forces [n_rows,n_atoms,3] = -dE/dx, analytic for all five terms
 * (the Born-radius chain rule of GBSA-OBC included); out_energy [n_rows] may be NULL.  What OpenMM's
 * Context.getState(getForces=True) returns for the Systems of simulation/md.py:128-187; pinned against the forces of the
 * reference's own known-answer file (simulation/testdata/implicit-2olx-traj-cpu-arrays.npz, simulation/tests/test_md.py:35-47). */
int tw_amber_energy_forces(const tw_forcefield* ff, const float* coords, double* out_energy, double* out_forces,
                           int64_t n_rows, void* stream);

/* `n_steps` integration steps of every conformation on the device - what `openmm_step` (utils/evaluation_utils.py:439-466)
 * does through the caller's openmm.app.Simulation, for the two integrators simulation/md.py:213-231 builds:
 *   scheme 0  LangevinMiddleIntegrator (v += dt F/m; x += dt/2 v; v <- a v + sqrt(1 - a^2) sqrt(kT/m) N(0,1); x += dt/2 v)
 *   scheme 1  LangevinIntegrator       (v <- a v + (1 - a)/friction F/m + sqrt(kT (1 - a^2)/m) N(0,1); x += dt v),  a = exp(-friction dt)
 * coords (nm) / velocs (nm/ps) [n_rows,n_atoms,3] are updated in place; masses [n_atoms] in dalton; kbT in kJ/mol;
 * friction 0 = plain leapfrog.  The Gaussian noise is counter-based on (seed, conformation, first_step + step as 64 bits, component 3 atom + axis): a
 * trajectory is reproducible for a seed but NOT the trajectory OpenMM would produce (its generator is its own).
 * out_energy [n_rows] (may be NULL): potential energy at the positions of the last force evaluation - those BEFORE the last update,
 * not the returned ones. */
int tw_langevin_steps(const tw_forcefield* ff, const float* masses, float* coords, float* velocs, int32_t n_steps,
                      double timestep_ps, double friction_per_ps, double kbT, int32_t scheme, uint64_t seed, int64_t first_step,
                      double* out_energy, int64_t n_rows, void* stream);

/* tw_langevin_steps that records a trajectory - the device-side stand-in for simulation/simulate_trajectory.py with the NPZReporter
 * of simulation/npzreporter.py:196-293 (positions, velocities, forces and [E_pot, E_kin] per reported step).  Additive: the ABI version
 * stays 8.  Integrators, units and the noise stream are those of tw_langevin_steps: without state64 and for the same arguments, coords
 * and velocs come back bit for bit as tw_langevin_steps returns them.
 *   report_steps [n_frames] int32 (device): strictly increasing, 0 <= r <= n_steps, counted from the start of THIS call (r = 0 is the
 *     input state).  The caller guarantees order and range: the library does not read a device array on the host, and the kernel
 *     walks the list with one running index (an entry out of order is never reached; nothing is written out of bounds).
 *   Frame k of row n holds the state after report_steps[k] steps: out_positions / out_velocities [n_rows,n_frames,n_atoms,3] - x and v
 *     as float32 casts of the fp64 state (what tw_langevin_steps would return there); out_forces (same shape, float32, kJ/mol/nm) -
 *     the forces AT those positions; out_energies [n_rows,n_frames,2] fp64 kJ/mol = E_pot at those positions, E_kin = 1/2 sum m v^2
 *     of those velocities.  A row's trajectory is contiguous.  Frames are a function of (seed, row, first_step) bit for bit: they do
 *     not depend on which other steps are reported.
 *   Velocities, scheme 0: the recorded velocities are the integrator's own stored ones, which for LangevinMiddleIntegrator live at the
 *     half step - the ones tw_langevin_steps returns - and E_kin is computed from them.  OpenMM's getState shifts velocities to the
 *     full step before it reports them (and its kinetic energy likewise); nothing here claims equality with those.
 *   state64 (may be NULL) [n_rows,2,n_atoms,3] fp64 = (x, v) per row: when given, the initial state is read from it INSTEAD of coords /
 *     velocs, and the final fp64 state is written back; coords / velocs still receive the float32 casts.  With it a run split over
 *     several calls (first_step advanced by the caller) is bit for bit the run of one call; without it the state is rounded to float32
 *     between calls.
 *   n_frames == 0 (report_steps and the four frame buffers may then be NULL): plain stepping with the fp64 carry.
 *   n_steps == 0 with report_steps = {0}: records the input state (one force evaluation).
 * Cost: one force evaluation per step, plus one if n_steps itself is reported.  LDS limit as tw_langevin_steps (~800 atoms). */
int tw_langevin_trajectory(const tw_forcefield* ff, const float* masses, float* coords, float* velocs, double* state64 /* may be NULL */,
                           int32_t n_steps, double timestep_ps, double friction_per_ps, double kbT, int32_t scheme,
                           uint64_t seed, int64_t first_step, const int32_t* report_steps, int32_t n_frames,
                           float* out_positions, float* out_velocities, float* out_forces, double* out_energies,
                           int64_t n_rows, void* stream);

/* tw_langevin_trajectory with options for what a frame records.  Additive: the ABI version stays 8.  The arguments are those of
 * tw_langevin_trajectory plus `record_flags`, a set of TW_RECORD_* bits; an unknown bit is refused (TW_ERR_ARG) before anything is
 * launched and nothing is written.  record_flags == 0 IS tw_langevin_trajectory, bit for bit: both are one kernel template.
 *   TW_RECORD_FULL_STEP_VELOCITIES: out_velocities of every frame holds, for component i of atom i / 3,
 *       v_full[i] = v[i] + (dt/2) F[i] / (double)masses[i / 3]
 *     computed in fp64 from the fp64 velocity of the state and the force of that frame's own force evaluation (the one out_forces
 *     holds), rounded to float32 once at the store; and out_energies[..., 1] = 1/2 sum m v_full^2 in fp64 with the reduction order
 *     of tw_langevin_trajectory (per-thread partial sums, wave butterflies, the waves' sums in wave order; no atomics).
 *     out_positions, out_forces and E_pot are those of record_flags == 0, and so are state64, coords, velocs and the integration
 *     itself: the carried velocity stays the stored one, and a trajectory's positions do not depend on the flag.
 *     Scheme 0 (LangevinMiddleIntegrator): the stored velocity lives half a step behind the positions and this half kick moves it
 *     to the full step - the shift OpenMM's getState applies before it reports velocities and kinetic energy.  OpenMM is not a
 *     dependency here and nothing was compared with it.
 *     Scheme 1 (LangevinIntegrator): the same formula is applied; nothing is claimed about what OpenMM reports for it. */
#define TW_RECORD_FULL_STEP_VELOCITIES (1 << 0)
int tw_langevin_trajectory_opts(const tw_forcefield* ff, const float* masses, float* coords, float* velocs, double* state64 /* may be NULL */,
                                int32_t n_steps, double timestep_ps, double friction_per_ps, double kbT, int32_t scheme,
                                uint64_t seed, int64_t first_step, const int32_t* report_steps, int32_t n_frames,
                                float* out_positions, float* out_velocities, float* out_forces, double* out_energies,
                                int64_t n_rows, int32_t record_flags, void* stream);

/* Langevin dynamics with holonomic constraints on the bonds to hydrogen - OpenMM's `constraints=HBonds`, the switch the reference's
 * simulation/md.py:182 leaves at None.  Additive: the ABI version stays 8.  Opt-in: constrained dynamics samples another ensemble
 * (X-H lengths fixed) than the one the flow was trained on.
 *
 * The constraint set (tw_constraints): disjoint clusters (c; h_1 .. h_k), 1 <= k <= 3 - a heavy atom c and its hydrogens.
 *   atoms [n_clusters,4] int32 = (c, h_1, h_2, h_3), unused slots -1 and after the used ones; lengths [n_clusters,3] fp64 = the
 *   constrained distances d_a (nm).  No atom is in two clusters.  The caller guarantees all this (timewarp_amd/forcefield.py
 *   HBondConstraints.check()): the library does not read a device array on the host.  tolerance (> 0, finite) is relative to the
 *   SQUARED length; max_sweeps (1 .. TW_CONSTRAINT_MAX_SWEEPS) bounds the one loop whose length depends on data.
 *
 * Algorithm (restated in float64 numpy by tests/constraint_oracle.py from this text).  One lane solves one cluster; all arithmetic is
 * fp64 in the order written; w = 1 / (double)mass; r_a = xref_c - xref_{h_a} are the reference vectors, from positions `xref` that
 * satisfy the constraints.
 *   Position projection P(x; xref) (SHAKE, Gauss-Seidel).  sweeps = 0.  At most max_sweeps times:  sweeps += 1;  for a = 1 .. k in
 *     order:  s = x_c - x_{h_a};  delta = d_a^2 - s.s;  if |delta| > tolerance d_a^2:  g = delta / (2 (r_a.s) (w_c + w_{h_a}));
 *     x_c += g w_c r_a;  x_{h_a} -= g w_{h_a} r_a.  The loop ends after the first sweep that changed nothing (that sweep is counted).
 *     residual = max_a |d_a^2 - s.s| / d_a^2 of the final positions, evaluated once more after the loop.
 *   Velocity projection Q(v; r) (direct).  A_ab = (r_a.r_b) w_c + [a = b] (r_a.r_a) w_{h_a};  b_a = (v_c - v_{h_a}).r_a;  A lambda = b
 *     by Gaussian elimination without pivoting in index order (A is symmetric positive definite), back substitution from a = k;
 *     v_c -= lambda_a w_c r_a for a = 1 .. k in order;  v_{h_a} += lambda_a w_{h_a} r_a.  Afterwards (v_c - v_{h_a}).r_a = 0.
 *   Scheme 0 (LangevinMiddleIntegrator), one step from the forces F(x):
 *     1. v += dt F / m                                                     (every component, the line of tw_langevin_steps)
 *     2. Q(v; r from x)                                                    (clusters)
 *     3. xref = x;  x += dt/2 v;  v <- a v + sqrt(1 - a^2) sqrt(kT/m) N;  x += dt/2 v     (every component; call the result x_u)
 *     4. P(x; xref)                                                        (clusters)
 *     5. v += (x - x_u) / dt for the atoms of the clusters                 (the displacement as computed, x - x_u, divided by dt)
 *   Scheme 1 (LangevinIntegrator): xref = x;  v <- a v + (1 - a)/friction F/m + sqrt(kT (1 - a^2)/m) N;  x += dt v  (= x_u);  then 4
 *     and 5.
 *   Atoms in no cluster see exactly the arithmetic of tw_langevin_steps, the noise key (seed, row, first_step + step, component) is
 *   unchanged, and with n_clusters == 0 the call IS tw_langevin_trajectory_opts(record_flags = 0) bit for bit - frames, coords, velocs,
 *   state64.  No atomics and no cross-lane arithmetic in the constraint phases: a row stays a function of (seed, row, first_step),
 *   independent of the other rows and of how the steps are cut into calls (with state64).
 *   The harmonic terms of the constrained bonds stay in the force field: at fixed length their energy is ~ k (tolerance d)^2 and the
 *   projections remove their force along the bond.  Recorded velocities are the stored ones (scheme 0: half step).
 *
 * tw_langevin_trajectory_constrained: the arguments of tw_langevin_trajectory_opts up to record_flags, then
 *   cons          the constraint set (not NULL; n_clusters may be 0)
 *   out_residual  [n_rows] fp64, may be NULL: the largest `residual` any cluster of the row reported in any step of this call
 *                 (0 with no step or no cluster).  A value above `tolerance` says max_sweeps did not suffice somewhere.
 *   out_sweeps    [n_rows] int32, may be NULL: the largest `sweeps` likewise.
 *   The input state must satisfy the constraints (tw_apply_constraints makes it so).  record_flags: an unknown bit is refused, and so
 *   is TW_RECORD_FULL_STEP_VELOCITIES - a constrained full-step velocity would need a projection of its own and is not built.
 *   Everything is validated before anything is queued; a refusal writes nothing.  LDS: one more array of 3 n_atoms doubles (xref)
 *   than tw_langevin_trajectory; a molecule that no longer fits 160 KiB is refused (TW_ERR_INVALID) naming the constrained kernel.
 *
 * tw_apply_constraints: one workgroup per row, no forces.  x <- P(x; xref = the input x);  then, when velocities are given,
 *   Q(v; r from the projected x).  state64 != NULL: x and v are the fp64 [n_rows,2,n_atoms,3] state, projected in place (both halves;
 *   coords / velocs are then ignored and may be NULL).  Otherwise coords float32 [n_rows,n_atoms,3] are read, projected in fp64 and
 *   the cluster atoms written back as float32 casts; velocs (may be NULL) likewise.  Atoms in no cluster are not touched.
 *   out_residual [n_rows] fp64 (may be NULL): the largest fp64 `residual` of the row, before any rounding to float32. */
#define TW_CONSTRAINT_MAX_SWEEPS 64
typedef struct {
  int32_t n_clusters, max_sweeps;
  double tolerance;
  const int32_t* atoms;    /* device [n_clusters,4] */
  const double* lengths;   /* device [n_clusters,3] */
} tw_constraints;
int tw_langevin_trajectory_constrained(const tw_forcefield* ff, const float* masses, float* coords, float* velocs,
                                       double* state64 /* may be NULL */, int32_t n_steps, double timestep_ps, double friction_per_ps,
                                       double kbT, int32_t scheme, uint64_t seed, int64_t first_step, const int32_t* report_steps,
                                       int32_t n_frames, float* out_positions, float* out_velocities, float* out_forces,
                                       double* out_energies, int64_t n_rows, int32_t record_flags, const tw_constraints* cons,
                                       double* out_residual /* [n_rows], may be NULL */, int32_t* out_sweeps /* [n_rows], may be NULL */,
                                       void* stream);
int tw_apply_constraints(const tw_constraints* cons, const float* masses, int32_t n_atoms, float* coords, float* velocs /* may be NULL */,
                         double* state64 /* may be NULL */, double* out_residual /* may be NULL */, int64_t n_rows, void* stream);

/* Local energy minimisation of every conformation on the device - what simulation/simulate_trajectory.py:186-191 does through OpenMM's
 * `simulation.minimizeEnergy(tolerance=--min-tol)` before anything moves.  Additive: the ABI version stays 8.  One workgroup per row on
 * the force kernels of tw_amber_energy_forces, all arithmetic in fp64, LDS limit as tw_langevin_steps (~800 atoms).
 *
 * What is claimed: the STOPPING RULE of OpenMM's LocalEnergyMinimizer - the root mean square of all 3 n_atoms force components at or
 * below `tolerance` (kJ/mol/nm).  OpenMM is not a dependency here and its L-BFGS iterates are NOT reproduced: the minimum reached is a
 * local minimum near the start, not necessarily the one OpenMM would stop in.
 *
 * Algorithm (restated in float64 numpy by tests/minimize_oracle.py from this text).  x: accepted coordinates, E = E(x), g = -F(x),
 * N = 3 n_atoms, m = `history`; a ring of at most m pairs (s_k, y_k) with rho_k = 1 / (s_k . y_k); c1 = 1e-4.
 *   start (fresh = 1): x = coords as fp64, one force evaluation gives E and g.  evaluations = 1, iterations = 0, empty ring.
 *     status = 3 if E or g.g is not finite;  else 0 if sqrt(g.g / N) <= tolerance;  else 1.
 *   continue (fresh = 0): the state is the workspace's.  A row of status 1 is checked against `tolerance` again (-> 0), no evaluation.
 *   Then at most n_iterations times, while status == 1:
 *     1. direction d.  Empty ring: d = -g.  Otherwise the two-loop recursion: q = g; for the pairs from newest to oldest
 *        a_k = rho_k (s_k . q), q -= a_k y_k;  q *= gamma, gamma = (s . y) / (y . y) of the newest pair;  for the pairs from oldest to
 *        newest b = rho_k (y_k . q), q += (a_k - b) s_k;  d = -q.  If then g.d >= 0 (or is not a number): the ring is emptied, d = -g.
 *     2. first trial step.  D = max_i |d_i|.  t = 1 with a ring, t = min(1, max_displacement / D) without;  then
 *        t = min(t, max_displacement / D): no coordinate moves by more than max_displacement (nm) in one trial.
 *     3. line search, at most 21 trials (t, t/2, ..., t / 2^20).  A trial is ONE force evaluation at x + t d, which gives E' and g'
 *        (evaluations += 1).  It is accepted if E' and g'.g' are finite and E' <= E + c1 t (g.d);  otherwise t <- t / 2.
 *     4. accepted: s = (x + t d) - x, y = g' - g, both as computed in fp64.  If s.y > 1e-10 (y.y) the pair enters the ring (the oldest is
 *        overwritten once m are held), otherwise it is skipped.  x <- x + t d, g <- g', E <- E', iterations += 1;
 *        status = 0 if sqrt(g.g / N) <= tolerance.
 *     5. 21 rejections: with a non-empty ring the ring is emptied and the iteration is repeated from 1 as steepest descent (the same
 *        iteration: it is not counted twice);  with an empty ring status = 2.
 *   Every loop has a bound known at launch - at most n_iterations x 2 x 21 force evaluations per row - and nothing waits on data.
 *   Reductions (g.g, g.d, s.y, y.y, the two-loop's dots, D): per-thread partial sums over i = thread, thread + threads, ... in that
 *   order, butterflies within a wave, then the waves' sums added in wave order.  No atomics: a row's result is a function of its
 *   input bit for bit - it does not depend on the other rows, nor on how the iterations are cut into calls.
 *
 * status (sticky: rows of status 0, 2, 3 do no force evaluation in later calls on the same workspace):
 *   0 converged   1 this call's n_iterations are used up - continue with fresh = 0   2 stalled (the line search failed as steepest
 *   descent)   3 energy or forces not finite at the input state; coords come back unchanged
 *
 * coords [n_rows,n_atoms,3] float32 (nm): read when fresh = 1; always written with the float32 cast of the accepted x (a row that
 *   did not move gets its input back bit for bit).
 * workspace [n_rows, tw_minimize_workspace_len(n_atoms, history)] fp64, owned by the caller, initialised here when fresh = 1.  Per
 *   row: [E, ring head, ring count, iterations, evaluations, status, 0, 0], x [N], g [N], s [m,N], y [m,N], rho [m], the two-loop's
 *   a_k [m].  Every entry is an fp64 VALUE - counters and status are small integers held exactly - nothing is a reinterpreted bit
 *   pattern.  `history` (0 .. TW_MINIMIZE_MAX_HISTORY; 0 is steepest descent) must be the same in every call on a workspace.
 * out_energy / out_rms [n_rows] fp64: E(x) kJ/mol and sqrt(g.g / N) kJ/mol/nm of the accepted x;  out_iterations / out_evaluations /
 *   out_status [n_rows] int32: totals since fresh = 1.  Each may be NULL.
 * n_iterations = 0 with fresh = 1 evaluates the input state only. */
#define TW_MINIMIZE_MAX_HISTORY 64
int64_t tw_minimize_workspace_len(int32_t n_atoms, int32_t history);   /* in doubles per row; -1 for arguments out of range */
int tw_minimize(const tw_forcefield* ff, float* coords /* in: start when `fresh`; out: float32 cast of the accepted x */,
                double* workspace, int32_t fresh /* 1: initialise the workspace from coords; 0: continue from it */,
                int32_t history, int32_t n_iterations, double tolerance, double max_displacement,
                double* out_energy, double* out_rms, int32_t* out_iterations, int32_t* out_evaluations, int32_t* out_status,
                int64_t n_rows, void* stream);

/* ---- Trajectory analysis (timewarp_amd/analysis.py).  Additive: the ABI version stays 8. ----
 *
 * Torsion angles of every row - what mdtraj's compute_dihedrals does for utils/torsion_utils.py:44-81.
 *   coords [n_rows,n_atoms,3] float32;  quads [n_quads,4] int32, each entry in 0 .. n_atoms - 1 (the caller guarantees the range: the
 *   library does not read a device array on the host);  out [n_rows,n_quads] float32, radians in (-pi, pi].
 *   Convention (mdtraj's): b1 = x1 - x0, b2 = x2 - x1, b3 = x3 - x2, c1 = b2 x b3, c2 = b1 x b2, angle = atan2((b1.c1) |b2|, c1.c2) -
 *   the IUPAC sign.  The arithmetic is fp64 from the float32 coordinates, rounded once at the store.  A collinear quad gives
 *   atan2(0, 0) = 0;  a non-finite coordinate gives NaN in the angles that read it and nowhere else.
 *   One workgroup per block of up to 64 rows (fewer for large molecules: a block's coordinates are staged in 64 KiB of LDS, so
 *   n_atoms <= 5461).  n_quads == 0 or n_rows == 0: a valid call that launches nothing. */
int tw_dihedrals(const float* coords, const int32_t* quads, int32_t n_quads, float* out, int64_t n_rows, int32_t n_atoms, void* stream);

/* The TICA feature vector of every row - utils/tica_utils.py:10-37 (`distances` and `tica_features`).
 *   out [n_rows,n_features] float32, n_features = n_sel (n_sel - 1) / 2 + 2 n_quads (anything else is TW_ERR_INVALID):
 *     columns 0 .. n_pairs - 1: |x[atom_sel[i]] - x[atom_sel[j]]| for the pairs i < j in np.triu_indices(n_sel, k=1) order;
 *     columns n_pairs + quad_cols[q,0] and n_pairs + quad_cols[q,1]: sin and cos of the angle of quad q (tw_dihedrals' convention;
 *     the collinear quad gives 0 and 1).  quad_cols [n_quads,2] int32 is a permutation of 0 .. 2 n_quads - 1 chosen by the caller
 *     (analysis.tica_features: per torsion family its sines, then its cosines); atom_sel [n_sel] int32 in 0 .. n_atoms - 1.  The caller
 *     guarantees those ranges.  fp64 arithmetic, one rounding at the store.
 *   n_features == 0 (n_sel <= 1 and n_quads == 0) or n_rows == 0: a valid call that launches nothing; atom_sel may be NULL when
 *   n_sel <= 1, quads / quad_cols when n_quads == 0. */
int tw_tica_features(const float* coords, const int32_t* atom_sel, int32_t n_sel, const int32_t* quads, const int32_t* quad_cols,
                     int32_t n_quads, float* out, int64_t n_rows, int32_t n_atoms, int32_t n_features, void* stream);

/* Time-lagged second moments - the sums deeptime's covariance estimator takes inside utils/tica_utils.py:40-46 (`run_tica`).
 *   X [n_chains,n_frames,n_features] float32.  Over all pairs x = X[c,t], y = X[c,t+lag], 0 <= t < n_frames - lag (a pair never
 *   crosses a chain) the call ADDS into acc, fp64 of 2 F + 3 F^2 entries (F = n_features):
 *     [ sum x (F) | sum y (F) | sum x x^T (F,F) | sum x y^T (F,F) | sum y y^T (F,F) ]   (row-major, x indexes the row of x y^T)
 *   and adds the pair count n_chains (n_frames - lag) to *n_pairs_out (device int64, may be NULL).  The caller zeroes both before the
 *   first call; several calls (chunks of a long trajectory, overlapping by `lag` frames) accumulate.
 *   A product of two float32 values is exact in fp64, so the only error is the order of summation, and that order is fixed: the pair
 *   axis is cut into equal contiguous ranges (their number a function of F and the pair count alone), each range is summed in pair
 *   order on the fp64 MFMA, the ranges' partials are added in range order.  No floating-point atomics: the same call on the same
 *   input gives the same bits.  Only the tiles on and above the diagonal of the two symmetric matrices are computed; the rest is
 *   mirrored (the same products in the same order).
 *   Supported: 1 <= F <= TW_MOMENTS_MAX_FEATURES, 1 <= lag < n_frames, n_chains x n_frames < 2^31; else TW_ERR_INVALID.  n_chains == 0
 *   launches nothing.
 *   workspace: tw_lagged_moments_workspace_len(F) doubles (-1 for F out of range), caller-owned, contents irrelevant before and
 *   after;  calls that share it must be ordered on one stream. */
#define TW_MOMENTS_MAX_FEATURES 1024
int64_t tw_lagged_moments_workspace_len(int32_t n_features);
int tw_lagged_moments(const float* X, int64_t n_chains, int64_t n_frames, int32_t n_features, int64_t lag, double* acc,
                      int64_t* n_pairs_out, double* workspace, void* stream);

/* The same sums with a weight per pair - what deeptime's covariance estimator takes once a KoopmanWeightingEstimator has been fitted
 * (utils/tica_utils.py:40-46).  weights [n_chains,n_frames] fp64: the weight of the pair (c, t) is weights[c,t]; the last `lag`
 * entries of a chain are never read.  The call ADDS into acc, in tw_lagged_moments' layout,
 *     [ sum w x | sum w y | sum w x x^T | sum w x y^T | sum w y y^T ],
 * adds sum w into *sum_w_out (device fp64, may be NULL) and the pair count into *n_pairs_out as before.
 *   The weight multiplies ONE operand as it is staged: a term is rnd((double)a w) b with a the row operand (x of x x^T and x y^T, y of
 *   y y^T; the sums of w x and w y add rnd((double)x w)) - one rounding more per term than the unweighted call, whose products are
 *   exact.  Negative and zero weights are legal.  With every weight exactly 1.0 the result equals tw_lagged_moments' on the same input
 *   bit for bit: x 1.0 is exact and the plan, the split of the pair axis and the order of summation are the same.  sum w is taken in a
 *   fixed order as well (contiguous ranges of the pair axis, a tree inside a range and over the ranges); nothing is atomic, a call is
 *   bit-reproducible.
 *   The two symmetric matrices are NOT bitwise symmetric here: inside a diagonal tile entry (i, j) sums rnd(w x_i) x_j and entry (j, i)
 *   sums rnd(w x_j) x_i; the tiles below the diagonal mirror those above.  The caller symmetrises (analysis.tica_from_moments does).
 *   Same support, same workspace (tw_lagged_moments_workspace_len) and same refusals as tw_lagged_moments; NULL weights is refused. */
int tw_lagged_moments_weighted(const float* X, const double* weights, int64_t n_chains, int64_t n_frames, int32_t n_features, int64_t lag,
                               double* acc, int64_t* n_pairs_out, double* sum_w_out, double* workspace, void* stream);

/* An affine map of every row in fp64 - the frame weights of a Koopman model (k = 1) and the TICs of a TICA model:
 *     out[n,j] = offset[j] + sum_f (X[n,f] - mean[f]) P[f,j]
 *   X [n_rows,n_features] float32;  mean [n_features], P [n_features,k] (row-major), offset [k] fp64;  out [n_rows,k] fp64.  mean and
 *   offset may be NULL, meaning zeros.  1 <= n_features <= TW_MOMENTS_MAX_FEATURES and 1 <= k <= 64, else TW_ERR_INVALID;
 *   n_rows == 0 launches nothing.
 *   fp64 throughout: the accumulator starts at offset[j] and takes fma(rnd(X[n,f] - mean[f]), P[f,j], .) for f = 0, 1, ... in that
 *   order, so a row's result is a function of that row alone - not of n_rows, of the row's position or of how rows are blocked.
 *   One workgroup per 64 rows; P is staged through LDS in slices of 64 features (it can be 512 KiB whole).  X is read once. */
int tw_project(const float* X, const double* mean, const double* P, const double* offset, double* out, int64_t n_rows, int32_t n_features,
               int32_t k, void* stream);

/* How far a reference cloud is from a sample cloud - the coverage check of the speed-up notebooks
 * (notebooks/Paper/speed-up-mcmc.ipynb cell 8, speed-up-exploration.ipynb cell 4:
 * `distance.cdist(ref, cloud).min(axis=1).max()`), in one pass that keeps a running minimum and stores nothing per pair.
 *   ref [n_ref,dim], cloud [n_cloud,dim] fp64, row-major.  Cloud row j belongs to group j % n_groups (the layout
 *   exploration.explore returns: explorer i in rows i::P); n_groups = 1 is the one-cloud expression above.
 *     out_min_d2[g,a] = min over the rows j of group g of d2(a, j),  d2(a, j) = sum_k (ref[a,k] - cloud[j,k])^2   (fp64 [n_groups,n_ref];
 *                       may be NULL: nothing is stored then and the other two outputs are the same)
 *     out_worst[g]    = sqrt(max_a out_min_d2[g,a])                                                               (fp64 [n_groups])
 *     out_arg[g]      = the smallest a that attains that maximum                                                  (int64 [n_groups])
 *   d2 is summed over k ASCENDING in fp64: t = rnd(ref[a,k] - cloud[j,k]); d2 = rnd(t_0 t_0), then d2 = fma(t_k, t_k, d2) for
 *   k = 1 .. dim - 1 (one rounding per step).  min, max and the comparison of indices are exact, so neither the tiling nor the split
 *   of the cloud axis over workgroups (a function of the shapes alone) changes a bit, and a call is bit-reproducible; nothing is
 *   atomic.  A group without rows (n_cloud < n_groups, or n_cloud == 0) gives +inf in out_min_d2 and out_worst and 0 in out_arg.
 *   The inputs are finite (the caller checks: the library does not read a device array on the host); a non-finite coordinate
 *   gives unspecified values, written inside the stated extents only.
 *   1 <= dim <= TW_COVERAGE_MAX_DIM, n_ref >= 1, n_cloud >= 0, n_groups >= 1, else TW_ERR_INVALID with the argument named in
 *   tw_last_error; also refused: n_ref > 2^31, n_groups > 2^22, more than 2^22 workgroups (ceil(n_ref / 512) n_groups times the
 *   splits of the cloud axis, at most 64).  A refused call launches nothing and writes nothing.
 *   workspace: tw_cloud_coverage_workspace_bytes(...) bytes (-1 for arguments the call refuses), 8-byte aligned, caller-owned,
 *   contents irrelevant before and after; a smaller workspace_bytes is TW_ERR_WORKSPACE.  Everything is enqueued on `stream`; the
 *   host does not wait. */
#define TW_COVERAGE_MAX_DIM 8
int64_t tw_cloud_coverage_workspace_bytes(int64_t n_ref, int64_t n_cloud, int32_t dim, int32_t n_groups);
int tw_cloud_coverage(const double* ref, const double* cloud, int64_t n_ref, int64_t n_cloud, int32_t dim, int32_t n_groups,
                      double* out_min_d2, double* out_worst, int64_t* out_arg, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The evaluation report (timewarp_amd/evaluate.py, csrc/tw_evaluate.hip).  Additive: the ABI version stays 8. ----
 *
 * Distances of atom pairs in every row - mdtraj's compute_distances without a unit cell, which utils/evaluation_utils.py:752 calls
 * on the bonds.
 *   coords [n_rows,n_atoms,3] float32;  pairs [n_pairs,2] int32, each entry in 0 .. n_atoms - 1 (the caller guarantees the range:
 *   the library does not read a device array on the host);  out [n_rows,n_pairs] float32.
 *   fp64 from the float32 coordinates (the conversion is exact) in this order, for the pair (i, j):
 *     t_k = rnd(x[i,k] - x[j,k]), k = 0, 1, 2;  d2 = rnd(t_0 t_0);  d2 = fma(t_1, t_1, d2);  d2 = fma(t_2, t_2, d2);  d = sqrt(d2),
 *   then ONE rounding of d to float32.  That is one device function; tw_pair_range and tw_pair_histogram call the same function, so
 *   they see the very float32 this call stores.  i == j gives 0 (of finite coordinates); a repeated pair is a repeated column.  A NaN
 *   coordinate gives NaN and an infinite one +inf or NaN (inf - inf) in the distances that read it, and nothing anywhere else.
 *   n_pairs <= TW_EVAL_MAX_COLS; one workgroup per block of max(1, 2048 / n_pairs) rows, at most 2^31 - 1 blocks; else TW_ERR_INVALID.
 *   n_pairs == 0 or n_rows == 0: a valid call that launches nothing. */
#define TW_EVAL_MAX_COLS (1 << 24)
int tw_pair_distances(const float* coords, const int32_t* pairs, int32_t n_pairs, float* out, int64_t n_rows, int32_t n_atoms,
                      void* stream);

/* The bin rule of every histogram below.  edges [n_cols,n_bins+1] fp64, strictly increasing per column (the caller guarantees it);
 * write e = edges[c].  A float32 value x of column c is converted to fp64 (exact) and
 *     e[i] <= x < e[i+1]           ->  counts[c,i]            (0 <= i < n_bins)
 *     x == e[n_bins]               ->  counts[c,n_bins-1]     (the last bin is closed)
 *     x < e[0]   (-inf included)   ->  outside[c,0]
 *     x > e[n_bins] (+inf included)->  outside[c,1]
 *     x is NaN                     ->  outside[c,2]
 * and nowhere else: every row adds exactly 1 to exactly one of these counters of its column.  With e = np.linspace(lo, hi, n_bins + 1)
 * the counts equal np.histogram(x.astype(np.float64), bins=n_bins, range=(lo, hi))[0].  The bin is found by a uniform estimate from
 * e[0] and e[n_bins] followed by a walk against the table; the table alone defines the result, for non-uniform edges as well.
 *
 * Per-column minimum and maximum over the FINITE entries, and the number of non-finite ones.
 *   Column c of row r is X[r ld + c col_stride] (float32; ld and col_stride in elements): the x components of a contiguous [T,V,3]
 *   tensor are the columns of ld = 3 V, col_stride = 3, without a copy.  Nothing between the columns (padding, the other components) is
 *   read.  out_lo, out_hi [n_cols] float32; out_nonfinite [n_cols] int64 (NaN and +-inf).  All three are OVERWRITTEN.
 *   min and max are taken as integer atomics on an order-preserving image of the float (-0 below +0), so they are exact, independent of
 *   how the rows are split over workgroups, and a call is bit-reproducible; of -0 and +0 in one column lo is -0 and hi is +0.  A column
 *   without a finite entry gives lo = +inf, hi = -inf.  Between the call's three launches out_lo and out_hi hold intermediate bits; they
 *   are floats once the stream has passed the call.
 *   Refused (TW_ERR_INVALID, the argument named in tw_last_error, nothing launched, nothing written): a negative size, n_rows >= 2^32,
 *   n_cols > TW_EVAL_MAX_COLS, col_stride < 1 or > 2^38, ld < (n_cols - 1) col_stride + 1, a NULL pointer.  n_rows == 0 or n_cols == 0: a
 *   valid call that launches nothing and leaves the outputs as they are.  Everything is enqueued on `stream`; the host does not wait. */
int tw_column_range(const float* X, int64_t n_rows, int32_t n_cols, int64_t ld, int64_t col_stride, float* out_lo, float* out_hi,
                    int64_t* out_nonfinite, void* stream);

/* Per-column histograms by the bin rule above.  The call ADDS into counts [n_cols,n_bins] int64 and outside [n_cols,3] int64: the
 * caller zeroes them before the first call, and chunks of a long run accumulate.
 *   A workgroup of 512 threads owns a tile of tw_histogram_column_tile(n_bins) = min(512, 65536 / (4 (n_bins + 3))) consecutive columns
 *   (159 at 100 bins, 3 at 4096; the last tile may be narrower) and a bounded share of the rows (at most 1024 workgroups per launch
 *   over the tiles, each walking every k-th block of rows in a persistent loop).  It counts in LDS in u32 - a call takes fewer than
 *   2^32 rows, so no counter wraps - and then adds every non-zero counter to the caller's array with one 64-bit INTEGER atomic.  Integer
 *   sums do not depend on order: the same call on the same input gives the same bits, and two calls on two halves give what one call on
 *   the whole gives.  There are no floating-point atomics.  Where a tile is narrower than a wave, lanes of a wave that hit the same
 *   counter are counted by a wave vote and added once (a bond length sends every row to a handful of bins).
 *   1 <= n_bins <= TW_HIST_MAX_BINS; at most 2^20 column tiles; otherwise the refusals of tw_column_range, and the same empty calls. */
#define TW_HIST_MAX_BINS 4096
int32_t tw_histogram_column_tile(int32_t n_bins);   /* -1 for n_bins out of range */
int tw_column_histogram(const float* X, int64_t n_rows, int32_t n_cols, int64_t ld, int64_t col_stride, const double* edges,
                        int32_t n_bins, int64_t* counts, int64_t* outside, void* stream);

/* The same two calls with column p of row r = the distance of pair p in row r, computed on the fly by tw_pair_distances' function from
 * coords [n_rows,n_atoms,3] (gathered from global memory: a thread keeps its pair's two indices in registers and reads six floats per
 * row); no [n_rows,n_pairs] array exists.  The results equal tw_column_range / tw_column_histogram on tw_pair_distances' output bit for
 * bit.  Same kernels (a column-source template parameter), same tiles, same refusals with n_pairs for n_cols; n_atoms >= 1. */
int tw_pair_range(const float* coords, const int32_t* pairs, int32_t n_pairs, int64_t n_rows, int32_t n_atoms, float* out_lo,
                  float* out_hi, int64_t* out_nonfinite, void* stream);
int tw_pair_histogram(const float* coords, const int32_t* pairs, int32_t n_pairs, int64_t n_rows, int32_t n_atoms, const double* edges,
                      int32_t n_bins, int64_t* counts, int64_t* outside, void* stream);

/* Joint (2-D) histograms of pairs of columns by the same bin rule - np.histogram2d of every pair at once (the hist2d of the
 * reference's TICA and Ramachandran figures).  Additive: the ABI version stays 8.
 *   X, n_rows, n_cols, ld, col_stride: the strided matrix of tw_column_histogram, addressed the same way; nothing between the columns
 *   is read.  pairs [n_pairs,2] int32: (x column, y column), each entry in 0 .. n_cols - 1 (the caller guarantees the range, as for
 *   tw_pair_distances; n_cols only bounds ld).  A pair may name one column twice, and pairs may repeat.
 *   edges_x [n_pairs,bins_x+1], edges_y [n_pairs,bins_y+1] fp64, one table per pair and axis, strictly increasing.
 *   counts [n_pairs,bins_x,bins_y] int64 and outside [n_pairs,3] int64 are ADDED into.  Each coordinate of a row is binned by the rule
 *   above against its own table, and the row adds exactly 1 to exactly one counter of its pair:
 *     either coordinate NaN                         -> outside[p,2]
 *     neither NaN, x outside its table (inf too)    -> outside[p,0]
 *     x inside, y outside its table                 -> outside[p,1]
 *     both inside, bins i and j                     -> counts[p,i,j]
 *   so counts[p].sum() + outside[p].sum() grows by n_rows per call.  With np.linspace edges counts[p] equals
 *   np.histogram2d(x.astype(float64), y.astype(float64), bins=(bins_x, bins_y), range=...)[0].
 *   A workgroup of 512 threads owns one pair, one BAND of the pair's bin plane and a share of the rows; lanes are consecutive rows.  A
 *   band is a run of min(bins_x, (16384 - 3) / bins_y) whole x-rows of the plane: its u32 counters and the three outside counters fit
 *   the 64 KB of LDS a launch gets without opting in (100 x 100 is one band, 1024 x 1024 is 69 of 15 x-rows, the last of 4).
 *   tw_joint_histogram_bands gives their number.  Every band's workgroups read the rows and count what falls into the band; the
 *   outside counters belong to band 0.  A (pair, band) gets min(ceil(1024 / (n_pairs bands)), n_rows / (band counters),
 *   ceil(n_rows / 512)) row shares, at least 1: the workgroup budget of the column kernels, and a share reads at least as many rows as
 *   its merge walks counters; share k reads the row blocks k, k + shares, ... of 512 rows.  The merge adds every non-zero counter with
 *   one 64-bit INTEGER atomic, so a call is bit-reproducible and two calls on two halves give what one call on the whole gives; there
 *   are no floating-point atomics and no workspace.  Rows are counted with one LDS atomic each: tw_column_histogram's wave vote was
 *   carried over and measured (profiles/joint_histogram.txt) - it costs a tenth on a time-ordered trajectory, on shuffled rows and
 *   with every row in one bin alike; it is reachable as TW_JOINT_PATH_VOTE and is not what tw_joint_histogram runs.
 *   Refused (TW_ERR_INVALID, the argument named, nothing launched or written): what tw_column_histogram refuses of n_rows, n_cols, ld
 *   (for n_cols columns) and col_stride; n_pairs < 0 or > TW_EVAL_MAX_COLS; bins_x or bins_y outside 1 .. TW_HIST_MAX_BINS;
 *   bins_x bins_y > 2^20; n_cols == 0 with rows and pairs to count; a NULL pointer.  n_rows == 0 or n_pairs == 0: a valid call that
 *   launches nothing.  The (pair, band) units are the grid's x dimension: 2^24 pairs of at most 86 bands stay below 2^31.
 * tw_joint_histogram_path is the same call with the counting path named: TW_JOINT_PATH_AUTO (what tw_joint_histogram takes: plain),
 * TW_JOINT_PATH_PLAIN (one LDS atomic per row) or TW_JOINT_PATH_VOTE (lanes of a wave that hit one counter are counted by a wave vote
 * and added once; the vote is left as soon as a round retires fewer than 4 lanes).  Every path gives the same counts. */
#define TW_JOINT_PATH_AUTO 0
#define TW_JOINT_PATH_PLAIN 1
#define TW_JOINT_PATH_VOTE 2
int32_t tw_joint_histogram_bands(int32_t bins_x, int32_t bins_y);   /* -1 when the plane is refused */
int tw_joint_histogram(const float* X, int64_t n_rows, int32_t n_cols, int64_t ld, int64_t col_stride, const int32_t* pairs,
                       int32_t n_pairs, const double* edges_x, int32_t bins_x, const double* edges_y, int32_t bins_y, int64_t* counts,
                       int64_t* outside, void* stream);
int tw_joint_histogram_path(const float* X, int64_t n_rows, int32_t n_cols, int64_t ld, int64_t col_stride, const int32_t* pairs,
                            int32_t n_pairs, const double* edges_x, int32_t bins_x, const double* edges_y, int32_t bins_y,
                            int64_t* counts, int64_t* outside, int32_t path, void* stream);

/* The accept step of sample_with_model (utils/evaluation_utils.py:659-713) for one chain:
 *   exp_ = e_pot_y/kbT(scaled by caller) ...: exponent[s] = energy[s] + p_xy[s] - p_yx[s];
 *   p_acc = min(1, e^-exponent); accepted[s] = u[s] < p_acc; k = first accepted index (or S-1);
 *   if any accepted: x <- y[k].  result (device, int32[4]) = {k_unclipped, any_accepted, 0, 0}.
 * energy = (e_pot_y - e_pot_x) + (e_kin_y - e_kin_x) is formed by the caller.
 * x_coords/x_velocs [n_atoms,3] are the chain state, updated in place; pass both NULL to only
 * score the proposals (the host then applies the reference's `k = min(k, N - i)` clipping,
 * evaluation_utils.py:680, before it moves the chain). */
int tw_mh_accept(const float* energy, const float* p_xy, const float* p_yx, const float* u,
                 const float* y_coords, const float* y_velocs, float* x_coords, float* x_velocs,
                 float* out_exponent, float* out_p_acc, uint8_t* out_accepted, int32_t* result,
                 int64_t n_proposals, int32_t n_atoms, void* stream);

/* Extension (no reference counterpart): n_chains independent chains evaluated in one flow
 * call of n_chains conditioning states x n_proposals samples.  Every per-proposal array is in the row order of that
 * call, index = proposal * n_chains + chain; x_coords / x_velocs [n_chains, n_atoms, 3]; result int32 [n_chains, 4].
 * Per chain exactly the semantics of tw_mh_accept. */
int tw_mh_accept_chains(const float* energy, const float* p_xy, const float* p_yx, const float* u,
                        const float* y_coords, const float* y_velocs, float* x_coords, float* x_velocs,
                        float* out_exponent, float* out_p_acc, uint8_t* out_accepted, int32_t* result,
                        int64_t n_proposals, int64_t n_chains, int32_t n_atoms, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One whole iteration of the loop body of sample_with_model (utils/evaluation_utils.py:609-713) in one call, for the
 * case the reference's scripts run: B = 1 conditioning state, S parallel proposals, accept = True.  Equivalent to
 *   tw_flow_sample_with_logp (proposals y, log p(y|x))  ->  tw_amber_energy (y and x)  ->  tw_kinetic_energy (y and x)
 *   ->  tw_chirality_changed  ->  tw_flow_log_likelihood (reverse move, velocities negated unless random_velocs)
 *   ->  tw_mh_accept
 * with the elementwise steps in between done on the device; the glue is four small launches instead of ~70.
 *   zy_coords / zy_velocs [n_proposals + 1, n_atoms, 3]: IN the latent noise of the S proposals, already multiplied by
 *     exp(prior log-scale) (rows 0..S-1; flow.py:274-275, coords drawn first); OUT the proposals y_coords / y_velocs in
 *     those rows.  Row S of zy_coords is scratch (the current state rides along in the energy launch).
 *   x_coords / x_velocs [n_atoms, 3]: the current state (x_velocs already resampled if the caller resamples);
 *   new_coords / new_velocs [n_atoms, 3]: y[k] if a proposal was accepted, else the current state.
 *   u [S]: the uniform draws of the accept test.
 *   out_stats [8, S]: p_acc, log p(y|x), log p(x~|y~), exponent, E_pot(y)/kT (+2000 on a chirality change), E_kin(y),
 *     E_pot(y)/kT - E_pot(x)/kT, E_kin(y) - E_kin(x)  (the ChainStats columns, evaluation_utils.py:721-728);
 *   out_accepted [S]; result int32[4] = {first accepted index or S-1, any accepted, 0, 0}  (as tw_mh_accept).
 * The caller applies the reference's clip k = min(k, N - i) (:680) when it emits the chain states. */
typedef struct {
  int32_t random_velocs;       /* compute_kinetic_energy form and the sign of the reverse move's velocities */
  int32_t n_centres;           /* chirality guard (utils/chirality.py): 0 = off */
  const int32_t* centres;      /* [n_centres, 4] */
  const float* reference_signs;/* [n_centres] */
  const float* masses;         /* [n_atoms]; may be NULL when random_velocs */
  float kbT;                   /* kJ/mol */
} tw_mh_options;

int64_t tw_mh_iteration_workspace_bytes(const tw_flow_desc* desc, int64_t n_proposals, int32_t n_atoms);
int tw_mh_iteration(const tw_flow_desc* desc, const float* raw, const void* packed, int32_t path,
                    const tw_forcefield* ff, const tw_mh_options* opt, const int32_t* atom_types,
                    const uint8_t* masked, int32_t n_atoms, const float* x_coords, const float* x_velocs,
                    float* zy_coords, float* zy_velocs, const float* u, float* new_coords, float* new_velocs,
                    float* out_stats, uint8_t* out_accepted, int32_t* result, int64_t n_proposals,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* ABI 8 - extension (the reference runs ONE chain per process, utils/evaluation_utils.py:517): the same
 * iteration for n_chains independent chains of one molecule in lock-step - ONE flow reverse pass over n_proposals x n_chains
 * rows, ONE energy launch (proposals + the n_chains current states), ONE forward pass, one accept workgroup per chain.  Row
 * order of every per-proposal array: index = proposal * n_chains + chain (the reference's [S, B] reshape, flow.py:284-296).
 * Per chain the arithmetic is that of tw_mh_iteration on that chain alone.
 *   atom_types / masked [n_chains, n_atoms]; x_coords / x_velocs [n_chains, n_atoms, 3]: the current states;
 *   cur_velocs [n_chains, n_atoms, 3] OUT: the velocities the iteration ran with (x_velocs, or the resampled ones);
 *   zy_coords [(n_proposals + 1) * n_chains, n_atoms, 3], zy_velocs [n_proposals * n_chains, n_atoms, 3]: latents IN (scaled,
 *     as for tw_mh_iteration) / proposals OUT; the last n_chains rows of zy_coords are scratch;
 *   u [n_proposals, n_chains]: accept uniforms; new_coords / new_velocs [n_chains, n_atoms, 3];
 *   out_stats [8, n_proposals, n_chains], out_accepted [n_proposals, n_chains], result int32 [n_chains, 4].
 * draws == NULL: the caller drew the latents, the (resampled) x_velocs and u - the route the oracle / trace tests take.
 * draws != NULL: they are drawn inside the first glue kernel by a counter-based generator - Philox4x32-10 with
 *   key = (seed & 0xffffffff, seed >> 32), counter = (element >> 2, kind | (iteration >> 32) << 4, iteration & 0xffffffff,
 *   first_chain + chain); kind 0 coordinate latents, 1 velocity latents (element = proposal * 3 n_atoms + component), 2
 *   resampled current velocities (element = component), 3 uniforms (element = proposal); word element & 3 of the block; normals
 *   by Box-Muller on the word pairs (0,1), (2,3): u1 = w * 2^-32 + 2^-33, u2 = (w >> 8) * 2^-24, cos for even elements, sin for
 *   odd; latents multiplied by exp(prior log-scale); uniforms (w >> 8) * 2^-24.  zy_* and u are then pure outputs, and a
 *   chain's draws depend on (seed, first_chain + chain, iteration) only - not on n_chains, not on what ran before.
 *   tw_mh_draw_chains writes exactly those draws (any of the four output pointers may be NULL) for tests and replays. */
typedef struct {
  uint64_t seed;
  int64_t iteration;        /* >= 0; the caller counts iterations */
  int32_t first_chain;      /* global id of chain 0 of this call (rank * chains_per_rank) */
  int32_t resample_velocs;  /* draw fresh N(0,1) current velocities (the reference's --resample-velocities; needs random_velocs) */
} tw_mh_draws;

int64_t tw_mh_iteration_chains_workspace_bytes(const tw_flow_desc* desc, int64_t n_proposals, int64_t n_chains, int32_t n_atoms);
int tw_mh_iteration_chains(const tw_flow_desc* desc, const float* raw, const void* packed, int32_t path,
                           const tw_forcefield* ff, const tw_mh_options* opt, const tw_mh_draws* draws,
                           const int32_t* atom_types, const uint8_t* masked, int32_t n_atoms, const float* x_coords,
                           const float* x_velocs, float* cur_velocs, float* zy_coords, float* zy_velocs, float* u,
                           float* new_coords, float* new_velocs, float* out_stats, uint8_t* out_accepted, int32_t* result,
                           int64_t n_proposals, int64_t n_chains, void* workspace, int64_t workspace_bytes, void* stream);
int tw_mh_draw_chains(const tw_flow_desc* desc, const float* raw, const tw_mh_draws* draws, float* z_coords, float* z_velocs,
                      float* u, float* velocs, int64_t n_proposals, int64_t n_chains, int32_t n_atoms, void* stream);

/* check_symmetry_change (utils/chirality.py:40-80): sign of the triple product at each
 * chirality centre vs reference_signs; out_changed [n_rows] uint8.  centres [n_centres,4] int32, every entry in
 * 0 .. n_atoms - 1 (the caller's to check: the table is on the device; the Python loops do, on the host).  n_centres == 0:
 * all rows unchanged, both tables may be NULL.  n_rows == 0 launches nothing; n_rows < 0, n_atoms <= 0 and n_centres < 0
 * are refused by name. */
int tw_chirality_changed(const float* coords, const int32_t* centres, const float* reference_signs,
                         int32_t n_centres, uint8_t* out_changed, int64_t n_rows, int32_t n_atoms,
                         void* stream);

/* Measurement hooks (bench.py roofline leg): between tw_profile_begin() and tw_profile_end() every
 * launch of the dominant kernel (the fused net-block kernel) is bracketed by hipEvents recorded on
 * the launch stream.  tw_profile_end synchronises those events and returns (host pointers) the
 * summed kernel time in milliseconds and the number of launches (of the bracketed ones: with TW_PROFILE_STRIDE=n in the
 * environment at tw_profile_begin only every n-th launch is bracketed - two event records cost a few microseconds of
 * stream time per launch).  Not thread-safe. */
int tw_profile_begin(void);
int tw_profile_end(double* total_ms, int64_t* launches);

/* Measurement hook (bench.py roofline.power_bound): a bare stream of v_mfma_f32_16x16x32_f16 - 36 * iters instructions per
 * wave, one wave per SIMD, `workgroups` workgroups of four waves (256 fills the chip), random fp16 operands of magnitude ~1 -
 * i.e. what the matrix pipes of THIS device sustain when nothing else happens (tools/probe/mfma_stream_probe.hip as an entry
 * point).  Returns (host pointers) the shader clocks one wave spent in the stream and the launch's duration from HIP events:
 * clock = cycles / ms, sustained rate = workgroups * 4 * 36 * iters * 16384 FLOP / ms.  Synchronous; launches on `stream`. */
int tw_probe_mfma_clock(int32_t workgroups, int32_t iters, int64_t* cycles, double* ms, void* stream);

/* Measurement hook (bench.py roofline.kernel, ABI 7): the template instantiation of the fused net-block kernel the calling
 * thread launched last, spelled as rocprofv3 prints it ("tw::netblock_h3_kernel<3, true, false, false, false, true, false,
 * false>": NT, ASM, DENSE, WIDE, RFF, ENC, H1, NG6) - which layout and build a flow call took is decided per launch (molecule
 * size, row count, tw_debug_set_flags).  A static string ("" before the first launch); never NULL. */
const char* tw_last_netblock_kernel(void);

/* Test hook (additive, ABI still 8): the attention kernel of the per-op paths (TW_PATH_SIMPLE / TW_PATH_SIMPLE_H3) the calling thread
 * launched last, spelled as rocprofv3 prints it - "tw::attend_kernel", "tw::attend_mfma_kernel", "tw::attend_h3_kernel",
 * "tw::attend_h3p_kernel", "tw::attend_fold_h3_kernel<2, 2>" (kernel attention), "tw::sdpa_kernel", "tw::sdpa_rows_kernel<16 | 64>",
 * "tw::sdpa_mfma_kernel" (dense softmax attention), "tw::local_attend_kernel<1 | 2 | 4 | 8>" (local attention).  Which one serves a model
 * is decided per launch from its widths, the molecule size and tw_debug_set_flags; a parity test of one of them asks here that it is the
 * one that ran.  A static string ("" before the first launch); never NULL. */
const char* tw_last_attention_kernel(void);

/* Test hook (additive, ABI still 8): the route the calling thread's last flow pass on the per-op paths took, as the plan and the
 * launchers decided it from the launch size (rows x atoms), the model and tw_debug_set_flags:
 *   "head_parts=<n> gemm_inside=<0|1> ln_inside=<0|1> ffn=<form> io=<form> q_tiles_per_wave=<n> chunks=<n>"
 * head_parts: workgroups per 128-query tile of the folded mixing (6, 3, 2 or 1; 0: no folded mixing), gemm_inside / ln_inside: the
 * folded GEMM / the residual and LayerNorm 1 inside that launch; ffn: "tokens48x4" (48-token waves, the hidden layer over four
 * workgroups per token tile), "tokens48x1", "tokens64x1" or "gemms" (plain GEMM launches); io (in / out MLPs): "tokens48", "tokens64"
 * or "gemms"; q_tiles_per_wave and chunks (grid z) of sdpa_mfma_kernel, 0 where it did not run.  tests/launch_sizes.py restates the
 * decisions and the GPU suite compares.  A string in thread-local static storage, rewritten by the next call on the thread ("" before
 * the first per-op pass); never NULL. */
const char* tw_last_per_op_route(void);

/* ABI 8: the instantiation a flow pass over n_rows x n_atoms on `path` (TW_PATH_FUSED_H3 / TW_PATH_FUSED_H1) WOULD launch under
 * the debug flags in force - the launch code's own branch run dry, nothing is launched and no GPU is needed.  "" when the path
 * does not serve the shape.  tests/test_host_logic.py enumerates 1 .. 192 atoms through it and holds every kernel it names to
 * ScratchSize 0 (one stated exception). */
const char* tw_flow_selected_kernel(const tw_flow_desc* desc, int32_t n_atoms, int64_t n_rows, int32_t path);

/* Safety net for TW_PATH_FUSED_H3 (no counterpart in the reference): *out_flag = 1 if, since the last reset, any
 * coupling net on the current device returned a non-finite scale or shift.  The split-fp16 kernel holds its operands in
 * fp16 (|value| < 65504); a checkpoint whose activations leave that range produces inf/NaN there, which the exact-f32
 * paths would not.  Synchronous (a device-to-host copy of one int): call it where the caller synchronises anyway.
 * `reset` != 0 clears the flag. */
int tw_flow_nonfinite(int32_t reset, int32_t* out_flag);

/* Debug / measurement switches of the split-fp16 kernel: tw_debug_set_flags takes an OR of the TW_DEBUG_* bits below (the
 * Python mirror is timewarp_amd._lib.DebugFlag).  0 restores normal operation.  Process-wide (see the thread-safety note at
 * the top).  The five TW_DEBUG_EXP_* bits are timing experiments that make results WRONG: the product library refuses them
 * (TW_ERR_INVALID) and compiles their branches out; they exist in a -DTW_EXPERIMENTS build only
 * (TW_EXPERIMENTS=1 python -m timewarp_amd.build).  Bits 8 and 9 are unassigned. */
/* timing experiments on the compiled-C++ sections only (results WRONG): no weight LDS-DMA after the prologue / no
 * workgroup barriers */
#define TW_DEBUG_EXP_NO_WEIGHT_DMA (1 << 0)
#define TW_DEBUG_EXP_NO_BARRIERS (1 << 1)
/* tw_debug_netblock dumps the attention output (before the first LayerNorm) instead of the layer output */
#define TW_DEBUG_DUMP_ATTENTION (1 << 2)
/* run the compiled-C++ variant of the kernel (attention / FFN / in / out sections as C++ instead of the generated asm
 * blocks); same results, slower - the A/B reference for the asm */
#define TW_DEBUG_COMPILED_CPP (1 << 3)
/* tw_debug_netblock: wave 0 of workgroup 0 writes s_memtime stamps of the section boundaries into the dump buffer instead
 * of activations (tools/profile_h3_sections.py) */
#define TW_DEBUG_SECTION_STAMPS (1 << 4)
/* split-fp16 flow pass: every affine coupling update as its own launch instead of in the next net-block launch's prologue
 * (A/B switch; same results up to the summation order of the log-determinant) */
#define TW_DEBUG_SEPARATE_COUPLING (1 << 5)
/* fused dense kernel, timing experiments (results WRONG): no softmax section / also no LDS round trip of q, k, v - what
 * the attention block costs beyond its MFMAs (0.8 of 11.4 ms per 1000-proposal pass) */
#define TW_DEBUG_EXP_DENSE_NO_SOFTMAX (1 << 6)
#define TW_DEBUG_EXP_DENSE_NO_QKV_LDS (1 << 7)
/* split-fp16 kernel: do not zero the padding tokens of a wave between sections (A/B switch; results equal) */
#define TW_DEBUG_KEEP_PADDING (1 << 10)
/* split-fp16 dense kernel, compiled-C++ attention: no scores / softmax / P.V (timing experiment, results WRONG) */
#define TW_DEBUG_EXP_DENSE_NO_ATTENTION (1 << 11)
/* split-fp16 kernel-attention kernel, <= 48 atoms: run the per-section build (attention / FFN asm blocks with compiled
 * glue between them) instead of the encoder-stack statement (tools/gen_h3_enc_asm.py); same results up to the last bits.
 * Activation dumps (tw_debug_netblock), TW_DEBUG_DUMP_ATTENTION and TW_DEBUG_SECTION_STAMPS take that build anyway. */
#define TW_DEBUG_PER_SECTION (1 << 12)
/* ... the encoder-stack build even with a dump buffer (profiling: only stamps outside the stack) */
#define TW_DEBUG_ENC_WITH_DUMPS (1 << 13)
/* molecules of 25 .. 48 atoms: never the wide layout / the wide layout wherever it exists (the launch code otherwise picks
 * the layout that needs fewer rounds of the chip; same results up to the last bits; A/B switch and tests) */
#define TW_DEBUG_NEVER_WIDE (1 << 14)
#define TW_DEBUG_ALWAYS_WIDE (1 << 15)
/* molecules of 49 .. 64 atoms: always 64-token waves (one molecule per wave) / never - the wide layout instead (the launch
 * code otherwise picks by rounds of the chip x cost per workgroup) */
#define TW_DEBUG_ALWAYS_NT4 (1 << 16)
#define TW_DEBUG_NEVER_NT4 (1 << 17)
/* wide layout, 65 .. 96 atoms: five-group key windows (molecules back to back where that fits) instead of the 96-slot
 * stride with three-group windows; same results up to the last bits (A/B switch and tests) */
#define TW_DEBUG_WIDE_FIVE_GROUP_WINDOWS (1 << 18)
/* wide layout: the transposed tile written with two-byte stores (r03's form) instead of through the matrix pipe;
 * bit-identical results (A/B switch and tests) */
#define TW_DEBUG_WIDE_XT_BYTE_STORES (1 << 19)
/* molecules of 97 .. 128 atoms: never the paired layout (one molecule per pair of 64-token waves, two per workgroup; r05) -
 * the wide layout's 48-token waves instead, one molecule per workgroup; same results up to the last bits (A/B switch and
 * tests).  The paired layout exists as the encoder-stack build only: TW_DEBUG_DUMP_ATTENTION / TW_DEBUG_SECTION_STAMPS /
 * TW_DEBUG_PER_SECTION (without TW_DEBUG_ENC_WITH_DUMPS) and tw_debug_netblock take the 48-token wide layout as well */
#define TW_DEBUG_NEVER_PAIRED (1 << 20)
/* per-op path: the row-wise scores kernel and the tiled MFMA mixing kernel (what molecules above 160 / 64 atoms take) at
 * every size; the same scores up to the order of a row sum's double additions, the mixing in another summation order
 * (A/B switch and tests) */
#define TW_DEBUG_PER_OP_ROWWISE (1 << 21)
/* tw_mh_iteration: the energy kernel on the caller's stream / on the side stream, whatever the launch size (default: side
 * stream only while the flow's launches leave compute units idle) */
#define TW_DEBUG_ENERGY_MAIN_STREAM (1 << 22)
#define TW_DEBUG_ENERGY_SIDE_STREAM (1 << 23)
/* TW_PATH_SIMPLE_H3: the FFN as two linear launches + add_ln, the attention unfolded, even when the path's pack is at hand
 * (default then: one launch of the fused kernels' chunk loop on the flat token list; folded attention); A/B switch and
 * tests */
#define TW_DEBUG_PER_OP_UNFUSED (1 << 24)
/* TW_PATH_SIMPLE_H3, folded attention (A/B switches and tests): the 768 -> 128 GEMM as its own launch behind the mixing
 * kernel instead of inside it (attend_fold_h3_kernel) / inside it with one workgroup per query tile whatever the launch
 * size (default below 400 workgroups: the heads over 6 / 2 workgroups per tile + a finishing launch) / residual +
 * LayerNorm 1 as the add_ln launch behind that kernel instead of in its epilogue */
#define TW_DEBUG_FOLD_GEMM_SEPARATE (1 << 25)
#define TW_DEBUG_FOLD_ONE_WG_PER_TILE (1 << 26)
#define TW_DEBUG_FOLD_LN_SEPARATE (1 << 27)
/* TW_PATH_SIMPLE_H3: the in-MLP and the out-MLP as two linear launches each instead of one launch of the fused kernels'
 * statements on the flat token list (h3_io_tokens_kernel) */
#define TW_DEBUG_IO_GEMM_PAIRS (1 << 28)
/* TW_PATH_SIMPLE_H3: the FFN / MLP token launches on 48-token / on 64-token waves whatever the launch size (default:
 * whichever needs fewer rounds' worth of the chip); same arithmetic per token.  TW_DEBUG_TOKENS_NT3 also turns off what
 * the per-op paths do for launches that do not fill the chip: the FFN's hidden layer over four workgroups per token tile,
 * and the second net of a coupling layer on a side stream (both nets then run on the caller's stream) */
#define TW_DEBUG_TOKENS_NT3 (1 << 29)
#define TW_DEBUG_TOKENS_NT4 (1 << 30)
/* per-op paths, dense softmax variant: the scalar attention kernels above 64 atoms instead of sdpa_mfma_kernel (fp32
 * matrix pipe); A/B switches and tests.  Bit 31: INT_MIN as the int tw_debug_set_flags takes. */
#define TW_DEBUG_SDPA_SCALAR (-0x7fffffff - 1)
int tw_debug_set_flags(int flags);

/* Debug/inspection: run ONE net-block of the fused path and dump the activation after every
 * stage (in_mlp, each encoder layer, out_mlp) as [n_rows,n_atoms,d] row-major floats.
 * dump must hold (n_layers+1)*n_rows*n_atoms*d_model + n_rows*n_atoms*3 floats.  Tests only. */
int tw_debug_netblock(const tw_flow_desc* desc, const float* raw, const float* packed,
                      int32_t coupling, int32_t net, const int32_t* atom_types,
                      const float* x_coords, const float* x_velocs, const uint8_t* masked,
                      int64_t n_cond, const float* z_other, int64_t n_rows, int32_t n_atoms,
                      int32_t path, float* dump, void* workspace, int64_t workspace_bytes,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TIMEWARP_HIP_H */
