"""float64 restatement of the optimizers and clip modes of the native step (torch 2.10 single-tensor semantics,
maximize=False, no amsgrad / nesterov / dampening), on plain tensors. tests/test_optim_ref.py pins it to torch.optim on
the CPU; the GPU tests compare the HIP kernels with it.

State per tensor: ``m`` (exp_avg; SGD's momentum buffer) and ``v`` (exp_avg_sq; unused by SGD), zero before the first
step. ``beta1`` is the first-moment coefficient of the step (OneCycleLR cycles it: betas[0], or SGD's momentum)."""
import math

KINDS = {"AdamW": 0, "Adam": 0, "SGD": 1, "RAdam": 2}  # CN_OPT_* of csrc/cn_optim.hip
CLIP_NONE, CLIP_NORM, CLIP_VALUE = 0, 1, 2             # CN_CLIP_*

# the reference's constructor arguments (models/lightning.py:611-655) besides lr / weight_decay / eps
BETA2 = {"Adam": 0.999, "AdamW": 0.98, "RAdam": 0.99, "SGD": 0.0}
TAKES_WD = {"Adam": False, "AdamW": True, "RAdam": True, "SGD": True}


def torch_optimizer(name, params, lr, weight_decay, eps):
    """The torch optimizer the reference constructs for --optimizer ``name``."""
    import torch

    if name == "Adam":
        return torch.optim.Adam(params, lr=lr, eps=eps)
    if name == "AdamW":
        return torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay, eps=eps, betas=(0.9, 0.98))
    if name == "RAdam":
        return torch.optim.RAdam(params, lr=lr, weight_decay=weight_decay, eps=eps, betas=(0.9, 0.99),
                                 decoupled_weight_decay=True)
    if name == "SGD":
        return torch.optim.SGD(params, lr=lr, weight_decay=weight_decay, momentum=0.9)
    raise NameError(name)


def clip_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_: the factor every gradient is multiplied by."""
    return min(1.0, max_norm / (norm + 1e-6))


def clip_value(g, clip):
    """torch.nn.utils.clip_grad_value_."""
    return g.clamp(-clip, clip)


def radam_rect(step, b2):
    """RAdam's variance rectification at ``step`` (None while rho_t <= 5: the un-rectified branch)."""
    rho_inf = 2.0 / (1.0 - b2) - 1.0
    rho_t = rho_inf - 2.0 * step * b2 ** step / (1.0 - b2 ** step)
    if rho_t <= 5.0:
        return None
    return math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))


def step(name, p, g, m, v, lr, beta1, eps, wd, t, b2=None):
    """One update of ``name`` at step count ``t`` (1-based) on the (already scaled and clipped) gradient ``g``.
    Returns (p, m, v)."""
    b2 = BETA2[name] if b2 is None else b2
    if not TAKES_WD[name]:
        wd = 0.0
    if name == "SGD":
        g = g + wd * p
        m = beta1 * m + g
        return p - lr * m, m, v
    p = p * (1.0 - lr * wd)
    m = beta1 * m + (1.0 - beta1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - b2 ** t
    if name in ("Adam", "AdamW"):
        return p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps), m, v
    rect = radam_rect(t, b2)
    if rect is None:
        return p - lr * m / bc1, m, v
    return p - lr * (m / bc1) * rect * math.sqrt(bc2) / (v.sqrt() + eps), m, v


def clipped(g, scale, mode, clip, norm_of=None):
    """The gradient the update sees: ``g * scale``, then norm-clipped (the norm over ``norm_of(g * scale)``, default the
    whole tensor) or value-clipped."""
    g = g * scale
    if mode == CLIP_NORM:
        sel = g if norm_of is None else norm_of(g)
        return g * clip_coef(float(sel.norm()), clip)
    if mode == CLIP_VALUE:
        return clip_value(g, clip)
    return g
