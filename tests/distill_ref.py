"""Float64 reference of the distillation head (lf_head_distill_fwd_f32 / lf_head_distill_bwd_f32, include/leafhip.h).

Per sample, z = student logits, y = the (label-smoothed) target, tp = the teacher's probabilities, T > 0,
0 <= alpha <= 1:

    p    = softmax(z)                        p_T = softmax(z / T)
    lt_j = log(max(tp_j, FLT_MIN))           q_T = softmax(lt / T)
    hard = -sum_j y_j log(clip(p_j, 1e-7, 1 - 1e-7))
    kd   = T^2 sum_j q_T,j (log q_T,j - log p_T,j)         both logs as log-softmax
    loss = (1 - alpha) hard + alpha kd
    dz   = [(1 - alpha)(p - y) + alpha T (p_T - q_T)] * inv_n     (the unclipped rule for the hard term)
"""
import numpy as np
import torch

D = torch.float64
FLT_MIN = float(np.finfo(np.float32).tiny)     # 1.17549435e-38, the smallest normal float


def teacher_logs(tp):
    return torch.log(tp.to(D).clamp_min(FLT_MIN))


def distill(z, y, tp, temperature, alpha, inv_n=1.0):
    """All of the above for float64 [n, c] tensors z, y, tp.  Returns a dict of float64 tensors: p, p_t, q_t, log_p_t,
    log_q_t, soft (= p_t - q_t), hard, kd, loss (per sample) and dz."""
    z, y = z.to(D), y.to(D)
    t = float(temperature)
    p = torch.softmax(z, -1)
    log_p_t = torch.log_softmax(z / t, -1)
    log_q_t = torch.log_softmax(teacher_logs(tp) / t, -1)
    p_t, q_t = log_p_t.exp(), log_q_t.exp()
    hard = -(y * torch.log(p.clamp(1e-7, 1 - 1e-7))).sum(-1)
    kd = t * t * (q_t * (log_q_t - log_p_t)).sum(-1)
    soft = p_t - q_t
    return {"p": p, "p_t": p_t, "q_t": q_t, "log_p_t": log_p_t, "log_q_t": log_q_t, "soft": soft, "hard": hard,
            "kd": kd, "loss": (1 - alpha) * hard + alpha * kd,
            "dz": ((1 - alpha) * (p - y) + alpha * t * soft) * inv_n}


def mean_loss(z, y, tp, temperature, alpha, inv_n):
    """sum_n loss_n * inv_n: the scalar whose gradient with respect to z is `dz`."""
    return distill(z, y, tp, temperature, alpha)["loss"].sum() * inv_n
