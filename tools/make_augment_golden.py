#!/usr/bin/env python
"""Writes tests/golden/augment_perlin.npz: outputs of the reference's own generate_perlin_noise_3d
(cultionet/augment/augmenter_utils.py) for (T, H, W) = (3, 20, 20) and res = (1, r, r), r = 2, 5, 10, with the gradient
angle tables it drew, which tests/test_augment_ref.py feeds to the restatement in tests/augment_ref.py.

    python tools/make_augment_golden.py /path/to/reference/src

The reference module is executed from where it lies. Its package __init__ files are skipped (empty stand-in packages),
`tsaug` -- which it imports and the Perlin generator does not use -- and `cultionet.data` are stand-in modules. The
angle tables are recorded from the two torch.rand calls the generator makes.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

SHAPE = (3, 20, 20)
RES = (2, 5, 10)
SEEDS = (11, 12, 13)


def load_reference(src):
    for name, path in (("cultionet", "cultionet"), ("cultionet.augment", "cultionet/augment")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(src, path)]
        sys.modules[name] = pkg
    tsaug = types.ModuleType("tsaug")
    tsaug.AddNoise = tsaug.Drift = tsaug.TimeWarp = object
    sys.modules["tsaug"] = tsaug
    data = types.ModuleType("cultionet.data")
    data.Data = object
    sys.modules["cultionet.data"] = data
    return importlib.import_module("cultionet.augment.augmenter_utils")


def main():
    ref = load_reference(sys.argv[1])
    out = {"shape": np.array(SHAPE), "res": np.array(RES), "seeds": np.array(SEEDS)}
    rand = torch.rand
    for r, seed in zip(RES, SEEDS):
        drawn = []
        torch.rand = lambda *a, **k: (drawn.append(rand(*a, **k)), drawn[-1])[1]
        try:
            noise = ref.generate_perlin_noise_3d(shape=SHAPE, res=(1, r, r), tileable=(False, False, False),
                                                 out_range=(-0.03, 0.03), rng=np.random.default_rng(seed))
        finally:
            torch.rand = rand
        assert len(drawn) == 2 and tuple(drawn[0].shape) == (2, r + 1, r + 1)
        out[f"theta_r{r}"] = (2 * np.pi * drawn[0]).numpy()  # float32, as the generator holds them
        out[f"phi_r{r}"] = (2 * np.pi * drawn[1]).numpy()
        out[f"noise_r{r}"] = noise.numpy()
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "augment_perlin.npz")
    np.savez_compressed(dst, **out)
    print(dst, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
