"""Float64 reference of the weighted head (lf_head_focal_fwd_f32 / lf_head_focal_bwd_f32, include/leafhip.h).

Per sample, z = logits, p = softmax(z), y = the (label-smoothed or mixed) target, cw = the class weights or None,
gamma = 0 or 1 <= gamma <= 8:

    s    = sum_j cw_j y_j                                    (1 without cw)
    m_j  = (1 - p_j)^gamma                                   (1 at gamma = 0, also at p_j = 1)
    loss = s sum_j -y_j m_j log(clip(p_j, 1e-7, 1 - 1e-7))   (m_j takes the unclipped p_j)
    l_j  = log(max(p_j, FLT_MIN))
    u_j  = y_j (gamma (1 - p_j)^(gamma-1) p_j l_j - m_j)     (-y_j at gamma = 0)
    dz_k = s (u_k - p_k sum_j u_j) inv_n                     (the unclipped rule)

u_j is p_j d(loss / s)/dp_j: d/dp of -y (1 - p)^gamma log p is y (gamma (1 - p)^(gamma-1) log p - (1 - p)^gamma / p);
the softmax Jacobian dp_j/dz_k = p_j ([j == k] - p_k) turns sum_j (u_j / p_j) dp_j/dz_k into u_k - p_k sum_j u_j.
"""
import numpy as np
import torch

D = torch.float64
FLT_MIN = float(np.finfo(np.float32).tiny)     # 1.17549435e-38, the smallest normal float


def sample_weights(y, cw):
    y = y.to(D)
    return torch.ones(y.shape[0], dtype=D) if cw is None else (y * cw.to(D)).sum(-1)


def modulating(p, gamma):
    """(1 - p)^gamma, exactly 1 at gamma = 0 (torch's 0^0 is 1 as well)."""
    return torch.ones_like(p) if gamma == 0 else (1 - p).clamp_min(0.0) ** gamma


def loss_from_probs(p, y, cw, gamma):
    p, y = p.to(D), y.to(D)
    return sample_weights(y, cw) * -(y * modulating(p, gamma) * torch.log(p.clamp(1e-7, 1 - 1e-7))).sum(-1)


def u_from_probs(p, y, gamma):
    p, y = p.to(D), y.to(D)
    if gamma == 0:
        return -y
    q = (1 - p).clamp_min(0.0)
    return y * (gamma * q ** (gamma - 1) * p * torch.log(p.clamp_min(FLT_MIN)) - q ** gamma)


def dz_from_probs(p, y, cw, gamma, inv_n=1.0):
    """dlogits of the backward entry for given probabilities (the entry is handed fp32 ones)."""
    p = p.to(D)
    u = u_from_probs(p, y, gamma)
    return sample_weights(y, cw)[:, None] * (u - p * u.sum(-1, keepdim=True)) * inv_n


def focal(z, y, cw, gamma, inv_n=1.0):
    """All of the above for float64 [n, c] tensors z, y and cw [c] or None.  Returns a dict of float64 tensors: p, s,
    m, loss (per sample), u and dz."""
    z, y = z.to(D), y.to(D)
    p = torch.softmax(z, -1)
    return {"p": p, "s": sample_weights(y, cw), "m": modulating(p, gamma), "loss": loss_from_probs(p, y, cw, gamma),
            "u": u_from_probs(p, y, gamma), "dz": dz_from_probs(p, y, cw, gamma, inv_n)}


def mean_loss(z, y, cw, gamma, inv_n):
    """sum_n loss_n * inv_n: the scalar whose gradient with respect to z is `dz` (where no probability is clipped)."""
    return loss_from_probs(torch.softmax(z.to(D), -1), y, cw, gamma).sum() * inv_n
