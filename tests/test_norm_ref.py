"""A float64 restatement of BatchNorm (+ SiLU + residual) and of LayerNorm over the channel axis of NCHW, forward and
backward, written as explicit formulas. tests/test_norm_gpu.py holds the HIP kernels to it; the test here holds it to
torch (F.batch_norm / F.layer_norm and autograd, all in float64) so the reference itself is known to be right.

BatchNorm tensors are viewed as [B, C, L] (L = H*W, or T*H*W for BatchNorm3d); LayerNorm normalises the C values of
one pixel of a [B, C, L] tensor.
"""
import pytest
import torch
import torch.nn.functional as F


def _silu(z):
    return z / (1.0 + torch.exp(-z))


def _silu_grad(z):
    s = 1.0 / (1.0 + torch.exp(-z))
    return s * (1.0 + z * (1.0 - s))


def bn_fwd64(x, gamma, beta, running_mean, running_var, *, training, momentum, eps, act, res=None):
    """x [B, C, L] float64. Returns a dict: y, mean, var (biased), rstd, xhat, z (pre-activation) and, when running
    statistics are given and training, the updated running_mean / running_var (unbiased variance; a batch of one value
    per channel keeps its biased variance 0, as the kernels' count > 1 guard does -- torch refuses that case)."""
    x = x.double()
    n = x.shape[0] * x.shape[2]
    if training:
        mean = x.sum(dim=(0, 2)) / n
        var = ((x - mean[None, :, None]) ** 2).sum(dim=(0, 2)) / n
    else:
        mean, var = running_mean.double(), running_var.double()
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean[None, :, None]) * rstd[None, :, None]
    z = gamma.double()[None, :, None] * xhat + beta.double()[None, :, None]
    y = _silu(z) if act else z
    if res is not None:
        y = y + res.double()
    out = dict(y=y, mean=mean, var=var, rstd=rstd, xhat=xhat, z=z)
    if training and running_mean is not None:
        unbiased = var * n / (n - 1) if n > 1 else var
        out["running_mean"] = (1.0 - momentum) * running_mean.double() + momentum * mean
        out["running_var"] = (1.0 - momentum) * running_var.double() + momentum * unbiased
    return out


def bn_bwd64(fwd, gamma, dy, *, training, act):
    """Gradients of y = act(gamma * xhat + beta) (+ res) from bn_fwd64's dict: dx, dgamma, dbeta and dz (dy through the
    activation). training: batch statistics depend on x; eval: frozen statistics, dx = gamma * rstd * dz."""
    dy = dy.double()
    dz = dy * _silu_grad(fwd["z"]) if act else dy
    xhat = fwd["xhat"]
    n = dy.shape[0] * dy.shape[2]
    dbeta = dz.sum(dim=(0, 2))
    dgamma = (dz * xhat).sum(dim=(0, 2))
    scale = (gamma.double() * fwd["rstd"])[None, :, None]
    if training:
        dx = scale * (dz - (dbeta / n)[None, :, None] - xhat * (dgamma / n)[None, :, None])
    else:
        dx = scale * dz
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, dz=dz)


def ln_fwd64(x, w, b, *, eps, res=None):
    """LayerNorm over C of x [B, C, L] float64: per pixel mean / biased variance over the C values."""
    x = x.double()
    C = x.shape[1]
    mean = x.sum(dim=1, keepdim=True) / C
    var = ((x - mean) ** 2).sum(dim=1, keepdim=True) / C
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    y = xhat * w.double()[None, :, None] + b.double()[None, :, None]
    if res is not None:
        y = y + res.double()
    return dict(y=y, mean=mean, var=var, rstd=rstd, xhat=xhat)


def ln_bwd64(fwd, w, dy):
    dy = dy.double()
    C = dy.shape[1]
    xhat = fwd["xhat"]
    g = dy * w.double()[None, :, None]
    dx = fwd["rstd"] * (g - g.sum(dim=1, keepdim=True) / C - xhat * (g * xhat).sum(dim=1, keepdim=True) / C)
    return dict(dx=dx, dw=(dy * xhat).sum(dim=(0, 2)), db=dy.sum(dim=(0, 2)))


def _rel_err(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("res", [False, True])
def test_batchnorm_restatement_matches_torch(training, act, res):
    g = torch.Generator().manual_seed(3)
    B, C, L, eps, momentum = 3, 5, 17, 1e-3, 0.3
    x = torch.randn(B, C, L, generator=g, dtype=torch.float64) * 2 + 0.7
    x[:, 1] += 50.0  # a channel far from zero
    gamma = 1 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    beta = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    rm = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    rv = 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    r = torch.randn(B, C, L, generator=g, dtype=torch.float64) if res else None
    dy = torch.randn(B, C, L, generator=g, dtype=torch.float64)

    fwd = bn_fwd64(x, gamma, beta, rm, rv, training=training, momentum=momentum, eps=eps, act=act, res=r)
    bwd = bn_bwd64(fwd, gamma, dy, training=training, act=act)

    xt, gt, bt = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    trm, trv = rm.clone(), rv.clone()
    z = F.batch_norm(xt, trm, trv, gt, bt, training, momentum, eps)
    yt = F.silu(z) if act else z
    if res:
        yt = yt + r
    yt.backward(dy)
    tol = 1e-12
    assert _rel_err(fwd["y"], yt.detach()) < tol
    assert _rel_err(bwd["dx"], xt.grad) < tol
    assert _rel_err(bwd["dgamma"], gt.grad) < tol
    assert _rel_err(bwd["dbeta"], bt.grad) < tol
    if training:
        assert _rel_err(fwd["running_mean"], trm) < tol
        assert _rel_err(fwd["running_var"], trv) < tol
    # the 4-D (BatchNorm2d) form is the same computation on the [B, C, H*W] view
    z4 = F.batch_norm(x.reshape(B, C, L, 1), rm.clone(), rv.clone(), gamma, beta, training, momentum, eps)
    assert _rel_err(fwd["z"], z4.reshape(B, C, L)) < tol


def test_batchnorm_restatement_count_one_keeps_the_biased_variance():
    x = torch.tensor([[[2.5], [-1.0]]], dtype=torch.float64)
    fwd = bn_fwd64(x, torch.ones(2), torch.zeros(2), torch.zeros(2), torch.ones(2), training=True, momentum=0.1,
                   eps=1e-5, act=0)
    assert torch.equal(fwd["var"], torch.zeros(2, dtype=torch.float64))
    assert torch.allclose(fwd["running_var"], torch.full((2,), 0.9, dtype=torch.float64), rtol=0, atol=1e-15)
    assert torch.equal(fwd["y"], torch.zeros(1, 2, 1, dtype=torch.float64))


@pytest.mark.parametrize("res", [False, True])
def test_layernorm_restatement_matches_torch(res):
    g = torch.Generator().manual_seed(4)
    B, C, L, eps = 2, 33, 19, 1e-4
    x = torch.randn(B, C, L, generator=g, dtype=torch.float64) * 3 - 1.0
    x[:, :, 3] += 200.0  # one pixel far from zero
    w = 1 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    b = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    r = torch.randn(B, C, L, generator=g, dtype=torch.float64) if res else None
    dy = torch.randn(B, C, L, generator=g, dtype=torch.float64)
    fwd = ln_fwd64(x, w, b, eps=eps, res=r)
    bwd = ln_bwd64(fwd, w, dy)

    xt, wt, bt = (t.clone().requires_grad_(True) for t in (x, w, b))
    yt = F.layer_norm(xt.permute(0, 2, 1), (C,), wt, bt, eps).permute(0, 2, 1)
    if res:
        yt = yt + r
    yt.backward(dy)
    tol = 1e-12
    assert _rel_err(fwd["y"], yt.detach()) < tol
    assert _rel_err(bwd["dx"], xt.grad) < tol
    assert _rel_err(bwd["dw"], wt.grad) < tol
    assert _rel_err(bwd["db"], bt.grad) < tol
