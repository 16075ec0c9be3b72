"""CPU tests of tests/augment_ref.py, the float64 restatement the GPU tests of the device augmentation stage are held to
(tests/test_augment_gpu.py), and of the host side of cultionet_amd.augment (plans and their draws):

* flips and rotations equal torch.flip / torch.rot90 exactly;
* cropresize equals F.interpolate of the crop (bilinear within 1e-6, nearest exactly), also at the non-exact scale 12 / 50;
* gaussian equals F.conv2d over a reflect-padded plane with the three taps, within 1e-6;
* perlin equals the reference's own generate_perlin_noise_3d, recorded in tests/golden/augment_perlin.npz by
  tools/make_augment_golden.py, within 1e-6;
* the Box-Muller noise has the mean and variance of a standard normal, within 4 standard errors;
* DeviceAugmenter.draw augments the requested fraction, uses every enabled op, is reproducible from its seed, and refuses
  what the device stage does not cover."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as R


def _sample(C, T, H, W, seed):
    g = np.random.default_rng(seed)
    x = g.uniform(1e-9, 1.0, (C, T, H, W))
    bd = g.uniform(0.0, 1.0, (H, W))
    y = g.integers(-1, 4, (H, W))
    return x, bd, y


@pytest.mark.parametrize("H,W", [(20, 20), (13, 13), (10, 28)])
def test_flips_and_rotations_equal_torch(H, W):
    x, bd, y = _sample(2, 3, H, W, 1)
    tx, ty = torch.from_numpy(x), torch.from_numpy(y)
    want = {"fliplr": lambda a: torch.flip(a, (-1,)), "flipud": lambda a: torch.flip(a, (-2,)),
            "rot180": lambda a: torch.rot90(a, 2, (-2, -1))}
    if H == W:
        want["rot90"] = lambda a: torch.rot90(a, 1, (-2, -1))
        want["rot270"] = lambda a: torch.rot90(a, 3, (-2, -1))
    for op, fn in want.items():
        xa, ba, ya = R.augment_sample(x, bd, y, {"op": op})
        assert torch.equal(torch.from_numpy(np.ascontiguousarray(xa)), fn(tx)), op
        assert torch.equal(torch.from_numpy(np.ascontiguousarray(ya)), fn(ty)), op
        assert torch.equal(torch.from_numpy(np.ascontiguousarray(ba)), fn(torch.from_numpy(bd))), op
    if H != W:
        with pytest.raises(AssertionError):
            R.permute(x, "rot90")


@pytest.mark.parametrize("H,W,div,top,left", [(50, 50, 4, 7, 31), (20, 28, 2, 10, 3)])
def test_cropresize_equals_interpolate(H, W, div, top, left):
    x, bd, y = _sample(2, 3, H, W, 2)
    xa, ba, ya = R.augment_sample(x, bd, y, {"op": "cropresize", "div": div, "top": top, "left": left})
    h, w = H // div, W // div
    cx = torch.from_numpy(x[..., top:top + h, left:left + w]).float()
    wx = F.interpolate(cx, size=(H, W), mode="bilinear", align_corners=False)
    assert np.abs(xa - wx.double().numpy()).max() <= 1e-6
    cb = torch.from_numpy(bd[top:top + h, left:left + w]).float()[None, None]
    wb = F.interpolate(cb, size=(H, W), mode="bilinear", align_corners=False)[0, 0]
    assert np.abs(ba - wb.double().numpy()).max() <= 1e-6
    cy = torch.from_numpy(y[top:top + h, left:left + w]).float()[None, None]
    wy = F.interpolate(cy, size=(H, W), mode="nearest")[0, 0].long()
    assert torch.equal(torch.from_numpy(np.ascontiguousarray(ya)), wy)
    assert ya.min() == -1  # labels keep every value


def test_nearest_source_is_torchs():
    """The nearest source index, min(floor(d * s), h - 1) with s = (float) h / H and the product in float32, is torch's
    at every plane size up to 128 and both crop divisors -- 50 -> 12 (s = 0.24f, h * div != H) among them. (At these
    sizes the float32 product happens to pick the same pixels as exact integer arithmetic; the definition is kept in
    float32 because that is what torch evaluates.)"""
    for H in range(2, 129):
        for div in (2, 4):
            h = H // div
            if h < 1:
                continue
            want = F.interpolate(torch.arange(float(h))[None, None], size=H, mode="nearest")[0, 0].long().numpy()
            assert np.array_equal(R.nearest_coords(H, h), want), (H, div)


@pytest.mark.parametrize("H,W,sigma", [(20, 20, 0.2), (13, 13, 0.37), (10, 28, 0.5)])
def test_gaussian_equals_conv2d(H, W, sigma):
    x, bd, y = _sample(2, 3, H, W, 3)
    xa, ba, ya = R.augment_sample(x, bd, y, {"op": "gaussian", "sigma": sigma})
    k = torch.from_numpy(R.gaussian_taps(sigma))
    assert abs(float(k.sum()) - 1) < 1e-12 and abs(float(k[0] / k[1]) - np.exp(-0.5 / sigma ** 2)) < 1e-12
    p = F.pad(torch.from_numpy(x).reshape(1, -1, H, W), (1, 1, 1, 1), mode="reflect").reshape(-1, 1, H + 2, W + 2)
    want = F.conv2d(p, torch.outer(k, k)[None, None]).reshape(x.shape)
    assert np.abs(xa - want.numpy()).max() <= 1e-6
    assert ba is bd and ya is y  # x only


def test_perlin_equals_the_reference_generator(golden_dir):
    g = np.load(os.path.join(golden_dir, "augment_perlin.npz"))
    T, H, W = (int(v) for v in g["shape"])
    assert (T, H, W) == (3, 20, 20) and [int(r) for r in g["res"]] == [2, 5, 10]
    for r in (2, 5, 10):
        got = R.perlin_field(T, H, W, r, g[f"theta_r{r}"], g[f"phi_r{r}"])
        want = g[f"noise_r{r}"].astype(np.float64)
        assert want.shape == (T, H, W) and np.abs(want).max() > 1e-3
        assert np.abs(got - want).max() <= 1e-6, r
        assert np.abs(got).max() <= 0.06
    x, bd, y = _sample(2, T, H, W, 4)
    xa, ba, ya = R.augment_sample(x, bd, y, {"op": "perlin", "r": 5, "theta": g["theta_r5"], "phi": g["phi_r5"]})
    assert np.abs((xa - x) - g["noise_r5"][None]).max() <= 1e-6  # broadcast over channels


def test_noise_statistics():
    N = 100_000
    n = R.normal_noise(0x1234_5678_9ABC_DEF0, N)
    assert np.isfinite(n).all() and np.abs(n).max() <= np.sqrt(2 * 24 * np.log(2)) + 1e-12
    assert abs(n.mean()) < 4 / np.sqrt(N)
    assert abs(n.var() - 1) < 4 * np.sqrt(2 / N)
    assert not np.array_equal(n[:100], R.normal_noise(7, 100))


def test_pipeline_of_none_is_the_plain_prologue():
    g = np.random.default_rng(5)
    xr = g.integers(-20, 11000, (2, 2, 3, 6, 7))
    br = g.integers(0, 10001, (2, 6, 7))
    y = g.integers(-1, 4, (2, 6, 7))
    mean, std = np.array([0.3, 0.2]), np.array([0.2, 0.1])
    x, bd, yo = R.pipeline(xr, br, y, [{"op": "none"}] * 2, mean, std)
    want = (np.clip(xr / 10000.0, 1e-9, 1) - mean.reshape(1, 2, 1, 1, 1)) / std.reshape(1, 2, 1, 1, 1)
    # raw * 1e-4 against raw / 10000: float64 roundoff of values up to 1 / std = 10
    assert np.abs(x - want).max() <= 1e-13 and np.array_equal(yo, y) and yo.dtype == np.int64
    assert np.abs(bd - np.clip(br / 10000.0, 1e-9, 1)).max() <= 1e-15


# ---- host side of cultionet_amd.augment ----------------------------------------------------------------------------

def test_draw_fraction_ops_and_parameters():
    from cultionet_amd.augment import DEVICE_AUGMENTATIONS, DeviceAugmenter

    aug = DeviceAugmenter(augment_prob=0.5, seed=42)
    N, H, W = 20_000, 20, 20
    plan = aug.draw(N, 3, H, W)
    ops = [plan.op(b) for b in range(N)]
    frac = sum(o != "none" for o in ops) / N
    assert abs(frac - 0.5) <= 4 * np.sqrt(0.25 / N) + 1e-12, frac  # 4 standard errors = 0.0141
    assert set(ops) == set(DEVICE_AUGMENTATIONS) | {"none"}
    for b, e in enumerate(R.entries_of(plan)):
        assert e["op"] == ops[b]
        if e["op"] == "gaussian":
            assert 0.2 <= e["sigma"] <= 0.5
        elif e["op"] == "cropresize":
            assert e["div"] in (2, 4)
            assert 0 <= e["top"] <= H - H // e["div"] and 0 <= e["left"] <= W - W // e["div"]
        elif e["op"] == "perlin":
            assert e["r"] in (2, 5, 10) and e["theta"].shape == (2, e["r"] + 1, e["r"] + 1)
            assert 0 <= e["theta"].min() and e["phi"].max() <= np.float32(2 * np.pi)
        elif e["op"] == "saltpepper":
            assert e["seed"] == plan.seed(b)
    seeds = [plan.seed(b) for b in range(N) if ops[b] == "saltpepper"]
    assert len(set(seeds)) == len(seeds)
    assert {int(plan.table[b, 1]) for b in range(N) if ops[b] == "cropresize"} == {2, 4}
    assert {int(plan.table[b, 4]) for b in range(N) if ops[b] == "perlin"} == {2, 5, 10}


def test_draw_is_reproducible_and_respects_prob():
    from cultionet_amd.augment import DeviceAugmenter

    a, b = DeviceAugmenter(seed=7), DeviceAugmenter(seed=7)
    for _ in range(3):
        pa, pb = a.draw(64, 3, 20, 20), b.draw(64, 3, 20, 20)
        assert np.array_equal(pa.table, pb.table) and np.array_equal(pa.perlin, pb.perlin)
    assert not np.array_equal(pa.table, DeviceAugmenter(seed=8).draw(64, 3, 20, 20).table)
    assert not DeviceAugmenter(augment_prob=0.0).draw(256, 3, 20, 20).table.any()
    assert (DeviceAugmenter(augment_prob=1.0).draw(256, 3, 20, 20).table[:, 0] != 0).all()


def test_draw_follows_the_shape():
    from cultionet_amd.augment import DeviceAugmenter

    # 13 x 13: neither 2, 5 nor 10 divides it, so perlin leaves the candidates; 10 x 28: only r = 2 does
    plan = DeviceAugmenter(augment_prob=1.0).draw(2000, 3, 13, 13)
    ops = {plan.op(b) for b in range(2000)}
    assert "perlin" not in ops and "rot90" in ops and "cropresize" in ops
    names = ("fliplr", "flipud", "rot180", "gaussian", "saltpepper", "cropresize", "perlin")
    plan = DeviceAugmenter(augment_prob=1.0, augmentations=names).draw(2000, 3, 10, 28)
    assert {int(plan.table[b, 4]) for b in range(2000) if plan.op(b) == "perlin"} == {2}
    with pytest.raises(ValueError):
        DeviceAugmenter().draw(4, 3, 10, 28)  # rot90 / rot270 enabled on a non-square chip
    with pytest.raises(ValueError):
        DeviceAugmenter(augmentations=("fliplr", "rot270")).draw(4, 3, 10, 28)


def test_unknown_and_host_side_names():
    from cultionet_amd.augment import HOST_AUGMENTATIONS, DeviceAugmenter

    with pytest.raises(KeyError):
        DeviceAugmenter(augmentations=("fliplr", "shear"))
    for name in HOST_AUGMENTATIONS:
        with pytest.raises(NotImplementedError, match="host"):
            DeviceAugmenter(augmentations=("fliplr", name))
    assert set(HOST_AUGMENTATIONS) == {"tswarp", "tsnoise", "tsdrift", "tspeaks", "roll"}
