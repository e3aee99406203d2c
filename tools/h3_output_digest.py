#!/usr/bin/env python3
"""One line per case with a sha256 of the raw output bytes of the split-fp16 / single-MFMA net-block path: two libraries computed
the same bits exactly when their outputs are equal line for line.  Run once per library, each in a fresh process (TW_HIP_LIB
names a library other than the in-tree one):

    TW_HIP_LIB=$PWD/timewarp_amd/lib/ab/libtimewarp_hip_parent.so python tools/h3_output_digest.py > parent.txt
    python tools/h3_output_digest.py > new.txt && cmp parent.txt new.txt

Cases (CASES): one per selectable family of instantiations, 7 rows each - the last block is ragged for every molecules-per-block
count - as forward pass, reverse pass with one conditioning state (shared score fragments) and reverse pass with one per row;
both paths.  Then tw_debug_netblock at three sizes and ten tw_mh_iteration calls of 16 proposals on alanine dipeptide.  A case the
library refuses prints the refusal.  Every line also names the instantiation that ran (tw_last_netblock_kernel).
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import timewarp_amd as tw  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import model_shapes as ms  # noqa: E402
from timewarp_amd import _lib, synthetic  # noqa: E402
from timewarp_amd._lib import DebugFlag as F  # noqa: E402

ROWS = 7
H3, H1 = _lib.TW_PATH_FUSED_H3, _lib.TW_PATH_FUSED_H1
BOTH = (("h3", H3), ("h1", H1))
SPLIT = (("h3", H3),)
CASES = (   # model, atoms, debug word, its name, paths
    ("kernel", 16, 0, "0", BOTH), ("kernel", 22, 0, "0", BOTH), ("kernel", 22, F.COMPILED_CPP, "COMPILED_CPP", BOTH),
    ("kernel", 30, 0, "0", BOTH), ("kernel", 30, F.ALWAYS_WIDE, "ALWAYS_WIDE", BOTH),
    ("kernel", 48, 0, "0", BOTH), ("kernel", 49, 0, "0", BOTH),
    ("kernel", 60, F.ALWAYS_NT4, "ALWAYS_NT4", BOTH), ("kernel", 60, F.ALWAYS_NT4 | F.PER_SECTION, "ALWAYS_NT4|PER_SECTION", BOTH),
    ("kernel", 60, F.ALWAYS_NT4 | F.COMPILED_CPP, "ALWAYS_NT4|COMPILED_CPP", SPLIT),
    ("kernel", 80, 0, "0", BOTH), ("kernel", 80, F.WIDE_FIVE_GROUP_WINDOWS, "WIDE_FIVE_GROUP_WINDOWS", BOTH),
    ("kernel", 110, 0, "0", BOTH), ("kernel", 110, F.NEVER_PAIRED, "NEVER_PAIRED", BOTH),
    ("kernel", 150, 0, "0", BOTH), ("kernel", 161, 0, "0", BOTH), ("kernel", 161, F.PER_SECTION, "PER_SECTION", BOTH),
    ("cheb", 22, 0, "0", BOTH), ("cheb", 80, 0, "0", BOTH),
    ("dense", 22, 0, "0", BOTH), ("dense", 60, 0, "0", BOTH), ("dense+rff", 22, 0, "0", BOTH),
)
DEBUG_NETBLOCK_SIZES = (22, 60, 110)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t).tobytes())
    return h.hexdigest()


def model(tag):
    if tag == "cheb":
        return ms.BY_NAME["k128-h5-cheb"].model().cuda()
    cfg = synthetic.kernel_transformer_nvp_config() if tag == "kernel" else synthetic.transformer_nvp_config()
    if tag == "dense+rff":
        cfg.transformer_nvp_config.rff_position_encoder_config = tw.RFFPositionEncoderConfig(128, 1.0, 1.0)
    m = tw.model_constructor(cfg)
    m.load_state_dict(dict(synthetic.synth_state_dict(m.state_dict(), 0)))
    return m.cuda().eval()


def inputs(V, n_cond):
    g = torch.Generator().manual_seed(1000 * V + n_cond)
    at = torch.randint(0, 5, (n_cond, V), generator=g, dtype=torch.int32).cuda()
    xc = (torch.randn(n_cond, V, 3, generator=g) * 0.35).cuda()
    xv = (torch.randn(n_cond, V, 3, generator=g) * 0.5).cuda()
    return g, at, xc, xv, torch.zeros(n_cond, V, dtype=torch.bool).cuda()


def attempt(label, fn):
    lib = _lib.load()
    try:
        out = digest(*fn())
    except RuntimeError as e:
        out = "refused: " + str(e).splitlines()[0]
    print(f"{label}: {out}  [{lib.tw_last_netblock_kernel().decode()}]", flush=True)


def flow_cases(models):
    for tag, V, flags, fname, paths in CASES:
        m = models[tag]
        for pname, path in paths:
            m.execution_path = path
            label = f"{tag} V={V} flags={fname} {pname}"
            # (no demotion to the exact-f32 kernels on a range overflow: whatever the path computes is what is compared)
            with H.debug_flags(flags), m.deferred_range_check():
                g, at, xc, xv, mk = inputs(V, ROWS)
                yc, yv = (torch.randn(ROWS, V, 3, generator=g) * 0.1).cuda() + xc, (torch.randn(ROWS, V, 3, generator=g) * 0.5).cuda()
                attempt(label + " forward", lambda: (m.log_likelihood(at, xc, xv, yc, yv, None, None, mk),))
                for n_cond, what in ((1, "reverse n_cond=1"), (ROWS, "reverse n_cond=n_rows")):
                    g, at, xc, xv, mk = inputs(V, n_cond)
                    S = ROWS // n_cond
                    zc, zv = (torch.randn(S, n_cond, V, 3, generator=g) * 0.05).cuda(), (torch.randn(S, n_cond, V, 3, generator=g) * 0.5).cuda()
                    attempt(f"{label} {what}", lambda: m.conditional_sample_with_logp(at, xc, xv, None, None, mk, S, z_coords=zc, z_velocs=zv))


def debug_netblock_cases(m):
    for V in DEBUG_NETBLOCK_SIZES:
        for pname, path in BOTH:
            g, at, xc, xv, mk = inputs(V, 1)
            zo = (torch.randn(ROWS, V, 3, generator=g) * 0.05).cuda()
            attempt(f"tw_debug_netblock kernel V={V} {pname}", lambda: m.debug_netblock(1, 1, at, xc - xc.mean(1, keepdim=True), xv, mk, zo, path))


def mh_case():
    from timewarp_amd.dataloader import single_state_batch
    from timewarp_amd.energy import AmberPotentialEnergyTorch
    from timewarp_amd.utils.evaluation_utils import MetropolisHastingsChain

    m = tw.model_constructor(synthetic.kernel_transformer_nvp_config())
    sd = dict(synthetic.synth_state_dict(m.state_dict(), 0))
    for k in sd:   # proposals near the state, as smoke(): shifts ~1e-4 nm stay acceptable against the stiff bonded terms
        if ".out_mlp._layers.2." in k:
            sd[k] = sd[k] * 1e-4
    sd["coords_prior_log_scale"], sd["velocs_prior_log_scale"] = torch.tensor(-7.0), torch.tensor(0.0)
    m.load_state_dict(sd)
    m.execution_path = H3
    m = m.cuda().eval()
    types, coords, masses = synthetic.alanine_dipeptide_state()
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    chain = MetropolisHastingsChain(single_state_batch("alanine-dipeptide", types, coords), m, torch.device("cuda", 0),
                                    AmberPotentialEnergyTorch.alanine_dipeptide(), masses, accept=True, random_velocs=True,
                                    resample_velocs=True, num_proposal_steps=16)
    with torch.no_grad():
        emitted = sum(chain.step() for _ in range(10))
    c, v, accepted, stats = chain.result()
    h = hashlib.sha256(np.ascontiguousarray(stats.exponent).tobytes()).hexdigest()
    print(f"tw_mh_iteration x 10, 16 proposals, alanine dipeptide: {digest(c, v)} {h} emitted={emitted} accepted={accepted}", flush=True)


def main():
    torch.manual_seed(0)   # the position encoder's Gaussian vectors are buffers drawn at construction
    models ={tag: model(tag) for tag in ("kernel", "cheb", "dense", "dense+rff")}
    flow_cases(models)
    debug_netblock_cases(models["kernel"])
    mh_case()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
