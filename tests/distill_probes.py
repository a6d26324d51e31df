"""Float64 twin and input builders for the fused distillation loss
(ops/hip/distill_loss.hip: distill_loss_fwd). Nothing here needs a GPU.
Validated against torch autograd by tests/test_distill_loop.py, used by
tests/test_gpu_distill.py.
"""
from __future__ import annotations

import numpy as np
import torch

KINDS = ("kl_divergence", "mean_squared_error")
KIND_ID = {"kl_divergence": 0, "mean_squared_error": 1}
CLAMP = 1e-12
MS = (1, 63, 64, 65, 257)
GUARD_ROWS = 256


def _softmax64(z: np.ndarray) -> np.ndarray:
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def distill_twin(teacher_logits, student_logits, temperature, kind):
    """(loss, d loss / d student_logits [M, 5]) of
    losses.DistillationLoss in float64, as closed-form expressions.

    t = softmax(teacher / T), s = softmax(student / T), loss = mean over the
    M positions of per(t, s), and through the softmax Jacobian
    d loss / d student_j = s_j (g_j - sum_k g_k s_k) / (T M), g = d per / d s.

    KL:  per = sum_k t_k (log max(t_k, c) - log max(s_k, c)), c = 1e-12;
         g_k = -t_k / s_k where s_k >= c (torch's clamp_min passes the
         gradient at equality) and 0 below, so
         s_j (g_j - sum_k g_k s_k) = s_j A - [s_j >= c] t_j with
         A = sum_{k: s_k >= c} t_k = 1 - sum_{k: s_k < c} t_k.
    MSE: per = mean_k (t_k - s_k)^2, g_k = -2 (t_k - s_k) / 5.
    """
    tl = np.asarray(teacher_logits, dtype=np.float64).reshape(-1, 5)
    sl = np.asarray(student_logits, dtype=np.float64).reshape(-1, 5)
    m = tl.shape[0]
    t = _softmax64(tl / temperature)
    s = _softmax64(sl / temperature)
    if kind == "mean_squared_error":
        d = t - s
        per = (d * d).mean(-1)
        g = -2.0 * d / 5.0
        dz = s * (g - (g * s).sum(-1, keepdims=True))
    else:
        passes = s >= CLAMP
        per = (t * (np.log(np.maximum(t, CLAMP))
                    - np.log(np.maximum(s, CLAMP)))).sum(-1)
        a = 1.0 - (t * ~passes).sum(-1, keepdims=True)
        dz = s * a - np.where(passes, t, 0.0)
    return per.mean(), dz / (temperature * m)


def torch_loss_and_grad(teacher_logits, student_logits, temperature, kind,
                        dtype):
    """(loss, grad) of losses.DistillationLoss under torch autograd on CPU,
    computed in dtype, returned as float64 numpy."""
    from deepconsensus_amd.models import losses as losses_lib

    t = torch.as_tensor(np.asarray(teacher_logits)).to(dtype)
    s = torch.as_tensor(np.asarray(student_logits)).to(dtype)
    s.requires_grad_(True)
    loss = losses_lib.DistillationLoss(temperature, kind)(t, s)
    loss.backward()
    return (loss.detach().double().numpy(),
            s.grad.detach().double().numpy())


def clamp_rows() -> np.ndarray:
    """Student rows whose softmax falls below 1e-12 on one to four classes:
    logit gaps of 40 and 200 (exp(-40) = 4e-18; exp(-200) is 0 in fp32)."""
    rows = []
    for gap in (40.0, 200.0):
        for n_low in (1, 2, 4):
            for shift in (0.0, 3.0):
                row = np.full(5, shift)
                row[5 - n_low:] -= gap
                rows.append(row)
                rows.append(row[::-1].copy())
    return np.array(rows, dtype=np.float32)


def random_logits(m: int, seed: int):
    """(teacher, student) fp32 [m, 5] in [-8, 8]; the first rows of the
    student (as many as fit) are clamp_rows()."""
    rng = np.random.default_rng(seed)
    teacher = rng.uniform(-8, 8, size=(m, 5)).astype(np.float32)
    student = rng.uniform(-8, 8, size=(m, 5)).astype(np.float32)
    cr = clamp_rows()[:m]
    student[: len(cr)] = cr
    return teacher, student
