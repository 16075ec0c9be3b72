"""Mixed-precision reference fixtures of the two constructor variants with their own bf16 kernels:
attention_weights="spatial_channel" and pool_by_max=True.

Same format as ``python -m oracle.make_golden --bf16-only``: the reference's training step under CPU bf16 autocast
(oracle.make_golden._train_case(..., autocast=True)), plus the ``fp32_*`` keys of the SAME case in fp32, so the tests
can state their tolerances relative to the reference's own bf16 deviation. Needs the reference (oracle.refimport).
Run from the repository root:

    TORCHDYNAMO_DISABLE=1 python tools/make_bf16_variant_golden.py [NAME ...]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import refimport  # noqa: E402
from oracle.make_golden import OUT, _train_case  # noqa: E402

# name -> ((hidden, B, H, W, with_mask), constructor keywords). The h32 b4 case is the decoder at its real width
# (128 channels at 100 / 50 / 25 px).
CASES = {
    "h8_b2_28_sca": ((8, 2, 28, 28, True), {"attention_weights": "spatial_channel"}),
    "h8_b2_28_poolmax": ((8, 2, 28, 28, True), {"pool_by_max": True}),
    "h32_b4_100_sca": ((32, 4, 100, 100, True), {"attention_weights": "spatial_channel"}),
}
FP32_KEYS = ("distance", "edge", "crop", "loss", "dloss", "eloss", "closs", "grad_norms")


def main(names):
    assert refimport.available(), "the reference is required to generate fixtures"
    torch.set_float32_matmul_precision("highest")
    torch.set_num_threads(8)
    ns = refimport.import_reference()
    os.makedirs(OUT, exist_ok=True)
    for name in names:
        args, kw = CASES[name]
        a = _train_case(ns, *args, autocast=True, **kw)
        f = _train_case(ns, *args, autocast=False, **kw)
        for k in FP32_KEYS:
            a["fp32_" + k] = f[k]
        path = os.path.join(OUT, f"train_bf16_{name}.npz")
        np.savez_compressed(path, **a)
        dmax = max(float(np.abs(a[k] - f[k]).max()) for k in ("distance", "edge", "crop"))
        print(os.path.basename(path), os.path.getsize(path) // 1024, "KiB", "loss", float(a["loss"]), "fp32",
              float(f["loss"]), "map dev max", dmax)


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES))
