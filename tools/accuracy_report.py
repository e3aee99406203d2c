"""Actual relative errors of every execution path against the reference vectors (GPU)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import helpers as H  # noqa: E402

from timewarp_amd._lib import DebugFlag  # noqa: E402

for name, cal in (("kernel_full_ad", False), ("kernel_cheb_full_ad", False)):
    d, _ = H.load(name)
    for path, label, flags in ((2, "simple", 0), (1, "fused-f32", 0), (3, "fused-h3", 0),
                               (3, "fused-h3 per-section build (PER_SECTION)", DebugFlag.PER_SECTION)):
        with H.debug_flags(flags):
            if "cheb" in name:
                m = H.tw_kernel_model(H.full_cheb_sd(), path=path, attention_type="chebyshev_kernel", cheb_order=6, force_asymptotic_zero=True)
            else:
                m = H.tw_kernel_model(H.full_kernel_sd(cal), path=path)
            out = H.run_model_case(m, d)
        keep = ~d["masked"][0]
        errs = {k: H.rel_err(out[k][:, :, keep] if out[k].dim() == 4 else out[k], d[k][:, :, keep] if d[k].dim() == 4 else d[k])
                for k in ("loglik", "s_y_coords", "s_y_velocs", "s_logp", "logp_yx")}
        print(name, label, {k: f"{v:.2e}" for k, v in errs.items()}, flush=True)
