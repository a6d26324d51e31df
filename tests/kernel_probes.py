"""Input builders and float64 references for the exact-answer kernel probes.

Every builder here picks inputs for which the right answer is known exactly
(or to one bf16 rounding), so that a wrong kernel shows as a bitwise mismatch
at a named row and column instead of a small error under a global bound.
All references run on the CPU in float64; nothing here needs a GPU.
Validated by tests/test_kernel_probes.py, used by tests/test_gpu_kernel_exact.py.
"""
from __future__ import annotations

import math

import numpy as np
import torch

BF16 = torch.bfloat16

# ---------------------------------------------------------------------------
# Banded attention: read the probabilities out through a one-hot V
# ---------------------------------------------------------------------------

# |out - P64| <= ATTN_RTOL * P64 + ATTN_ATOL. One or two round-to-nearest bf16
# roundings cost 2^-9 relative each; the fp32 dot and exp errors are orders
# smaller (< 2^-12 even at |logit| = 150).
ATTN_RTOL = 2.0 ** -8
ATTN_ATOL = 1e-6


def band_mask(L: int, win: int) -> torch.Tensor:
    i = torch.arange(L)
    return (i[:, None] - i[None, :]).abs() <= win


def band_counts(L: int, win: int) -> torch.Tensor:
    """n_i = number of in-band keys of row i (win+1 at the ends of a long
    sequence, 2*win+1 in the middle, never more than L)."""
    return band_mask(L, win).sum(-1)


def make_qk(B, L, H, D, seed, logit_peak=None, win=None):
    """q, k [B, L, H, D] bf16, distinct for every (b, h) item.

    With logit_peak set, q and k are rescaled so that the largest in-band
    |logit| (scale D^-0.5) is about logit_peak."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, L, H, D, generator=g)
    k = torch.randn(B, L, H, D, generator=g)
    if logit_peak is not None:
        s = logits64(q.to(BF16), k.to(BF16))
        peak = s[..., band_mask(L, win)].abs().max().item()
        f = math.sqrt(logit_peak / peak)
        q, k = q * f, k * f
    return q.to(BF16), k.to(BF16)


def onehot_v(B, L, H, D) -> torch.Tensor:
    """V[b, j, h, :] one-hot at dimension j mod D."""
    v = torch.zeros(B, L, H, D, dtype=BF16)
    j = torch.arange(L)
    v[:, j, :, j % D] = 1.0
    return v


def pack_qkv(q, k, v) -> torch.Tensor:
    """[B, L, H, D] x 3 -> packed [B, L, 3*H*D] (q | k | v, head-major)."""
    B, L, H, D = q.shape
    return torch.cat(
        [t.reshape(B, L, H * D) for t in (q, k, v)], dim=-1
    ).contiguous()


def logits64(q, k) -> torch.Tensor:
    """[B, H, L, L] float64 scaled logits from the bf16-rounded q, k."""
    D = q.shape[-1]
    qd = q.double().permute(0, 2, 1, 3)
    kd = k.double().permute(0, 2, 1, 3)
    return torch.matmul(qd, kd.transpose(-1, -2)) * (D ** -0.5)


def p64(q, k, win) -> torch.Tensor:
    """Banded softmax [B, H, L, L] in float64; out-of-band exactly 0."""
    L = q.shape[1]
    s = logits64(q, k).masked_fill(~band_mask(L, win), -math.inf)
    return torch.softmax(s, dim=-1)


def p32_bf16(q, k, win) -> torch.Tensor:
    """The same softmax in float32 torch, rounded to bf16 (CPU stand-in for
    what a correct kernel computes)."""
    L, D = q.shape[1], q.shape[-1]
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * torch.tensor(
        D ** -0.5, dtype=torch.float32)
    s = s.masked_fill(~band_mask(L, win), -math.inf)
    return torch.softmax(s, dim=-1).to(BF16)


def probe_expected(P: torch.Tensor, D: int):
    """What the one-hot V makes of P [B, H, L, L] (exactly 0 off the band).

    Returns expect [B, L, H, D] with P[i, j] at dim j mod D; every in-band
    key of a row lands on a dim of its own when D >= band width."""
    B, H, L, _ = P.shape
    idx = (torch.arange(L) % D).view(1, 1, 1, L).expand(B, H, L, L)
    exp = torch.zeros(B, H, L, D, dtype=P.dtype)
    exp.scatter_add_(-1, idx, P)
    return exp.permute(0, 2, 1, 3).contiguous()


def probe_hit_mask(L: int, D: int, win: int) -> torch.Tensor:
    """[L, D] bool: element (i, d) receives an in-band key of row i."""
    assert D >= min(2 * win + 1, L), "one-hot V needs D >= band width"
    hit = torch.zeros(L, D, dtype=torch.bool)
    i, j = band_mask(L, win).nonzero(as_tuple=True)
    hit[i, j % D] = True
    return hit


def band_slots(P: torch.Tensor, win: int) -> torch.Tensor:
    """P [B, H, L, L] -> band layout [B*H, L, 2*win+1]; slot w holds key
    i - win + w, slots with key < 0 or >= L are 0."""
    B, H, L, _ = P.shape
    W = 2 * win + 1
    out = torch.zeros(B * H, L, W, dtype=P.dtype)
    Pf = P.reshape(B * H, L, L)
    i = torch.arange(L)
    for w in range(W):
        j = i - win + w
        ok = (j >= 0) & (j < L)
        out[:, i[ok], w] = Pf[:, i[ok], j[ok]]
    return out


def slot_valid(L: int, win: int) -> torch.Tensor:
    """[L, 2*win+1] bool: slot's key index lies in [0, L)."""
    j = torch.arange(L)[:, None] - win + torch.arange(2 * win + 1)[None, :]
    return (j >= 0) & (j < L)


def attn_within_bound(got: torch.Tensor, ref64: torch.Tensor) -> torch.Tensor:
    """Elementwise |got - ref| <= 2^-8 ref + 1e-6 (non-finite got fails)."""
    g = got.double()
    return torch.isfinite(g) & (
        (g - ref64).abs() <= ATTN_RTOL * ref64.abs() + ATTN_ATOL
    )


def first_bad(ok: torch.Tensor):
    """Index tuple of the first False of `ok`, or None."""
    bad = (~ok).nonzero()
    return None if bad.numel() == 0 else tuple(int(t) for t in bad[0])


# (L, win, H) for the MFMA kernels: every (L, win) pair, with H rotated so
# that every (L, H) and every (win, H) pair appears as well.
MFMA_LS = (32, 33, 63, 64, 65, 96, 97, 100, 104)
MFMA_WINS = (1, 2, 6, 11, 12)
MFMA_HS = (1, 2, 3)
MFMA_CASES = [
    (L, win, MFMA_HS[(a + b) % 3])
    for a, L in enumerate(MFMA_LS)
    for b, win in enumerate(MFMA_WINS)
]


# ---- backward ------------------------------------------------------------

def attn_bwd_inputs(B, H, T, D, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (
        torch.randn(B, H, T, D, generator=g).to(BF16) for _ in range(4)
    )
    return q, k, v, do


def _banded_ctx(q, k, v, win, cast_p):
    """model.py SelfAttention chain on [B, H, T, D] tensors of any dtype."""
    T, D = q.shape[-2], q.shape[-1]
    logits = torch.matmul(q * D ** -0.5, k.transpose(-1, -2))
    logits = logits.masked_fill(~band_mask(T, win), -1e9)
    if cast_p:
        w = torch.softmax(logits.float(), dim=-1).to(q.dtype)
    else:
        w = torch.softmax(logits, dim=-1)
    return torch.matmul(w, v)


def attn_bwd_ref64(q, k, v, do, win):
    """float64 autograd dq, dk, dv of the banded softmax attention."""
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    _banded_ctx(qd, kd, vd, win, cast_p=False).backward(do.double())
    return qd.grad, kd.grad, vd.grad


def attn_bwd_torch_bf16(q, k, v, do, win):
    """The bf16 torch autograd chain the training path falls back to."""
    qb, kb, vb = (t.clone().requires_grad_() for t in (q, k, v))
    _banded_ctx(qb, kb, vb, win, cast_p=True).backward(do)
    return qb.grad, kb.grad, vb.grad


def row_groups(T: int, win: int):
    """Row slices: first win+1 rows, middle, last win+1 rows."""
    return (slice(0, win + 1), slice(win + 1, T - 1 - win),
            slice(T - 1 - win, T))


def group_rel_err(got, ref64, T, win):
    """Relative Frobenius error over each row group; tensors [B, H, T, D]."""
    out = []
    for sl in row_groups(T, win):
        num = (got.double()[..., sl, :] - ref64[..., sl, :]).norm()
        out.append((num / ref64[..., sl, :].norm()).item())
    return tuple(out)


BWD_CASES = [(32, 1), (32, 12), (100, 1), (100, 12)]  # (T, win); B=2, H=2
BWD_B, BWD_H, BWD_D = 2, 2, 140

# Relative Frobenius error of the bf16 torch autograd chain (CPU) against
# float64 autograd on attn_bwd_inputs(2, 2, T, 140, seed=700+T+win), per
# (T, win) -> {grad: (rows [0,win], middle, rows [T-1-win,T-1])}. Measured
# by test_kernel_probes.py::test_bwd_baseline_table_is_current. The kernels
# are allowed BWD_MARGIN x these figures: they round P and dP to bf16 once
# more than torch does. On an MI355X the three backward kernels measured
# 2.1e-3 .. 3.4e-3 in every group, i.e. below the torch chain itself.
BWD_MARGIN = 2.0
BWD_TORCH_BF16_ERR = {
    (32, 1): {"dq": (4.136e-3, 3.663e-3, 3.410e-3),
              "dk": (4.264e-3, 3.666e-3, 3.442e-3),
              "dv": (2.341e-3, 2.607e-3, 2.888e-3)},
    (32, 12): {"dq": (3.874e-3, 4.373e-3, 3.704e-3),
               "dk": (3.622e-3, 3.636e-3, 4.256e-3),
               "dv": (3.497e-3, 3.899e-3, 3.565e-3)},
    (100, 1): {"dq": (3.590e-3, 3.628e-3, 3.371e-3),
               "dk": (3.816e-3, 3.665e-3, 3.400e-3),
               "dv": (2.306e-3, 2.685e-3, 2.946e-3)},
    (100, 12): {"dq": (4.310e-3, 4.030e-3, 4.041e-3),
                "dk": (3.885e-3, 4.094e-3, 4.077e-3),
                "dv": (3.409e-3, 3.592e-3, 3.294e-3)},
}


# ---------------------------------------------------------------------------
# Exact-arithmetic GEMM probes
# ---------------------------------------------------------------------------

def grid_tensor(shape, step, kmax, seed):
    """Independent draws from {k*step : |k| <= kmax} as float64."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-kmax, kmax + 1, shape, generator=g)
    return k.double() * step


def linear_probe(M, N, Npad, seed, bias=False):
    """fused_linear inputs: x on k/8 (|k| <= 16), dense W in {-1,0,1} zero
    padded to [Npad, 296], optional fp32 bias on the same grid. Every partial
    sum is a multiple of 1/8 below 2^10, exact in fp32 in any order."""
    x = grid_tensor((M, 280), 1 / 8, 16, seed)
    g = torch.Generator().manual_seed(seed + 1)
    w = torch.randint(-1, 2, (N, 280), generator=g).double()
    w_img = torch.zeros(Npad, 296, dtype=torch.float64)
    w_img[:N, :280] = w
    b = grid_tensor((N,), 1 / 8, 16, seed + 2) if bias else None
    return x, w, w_img, b


def linear_ref(x, w, b=None, relu=False, resid=None, alpha=0.0,
               dtype=torch.float64, perm=None):
    """bf16 result of fused_linear in `dtype` arithmetic. The kernel stages
    act(xW^T + b) through bf16 before the residual, so that rounding is part
    of the operation: out = bf16(resid + alpha * bf16(act(...)))."""
    xd, wd = x.to(dtype), w.to(dtype)
    if perm is not None:
        xd, wd = xd[:, perm], wd[:, perm]
    y = xd @ wd.t()
    if b is not None:
        y = y + b.to(dtype)
    if relu:
        y = torch.relu(y)
    y = y.to(BF16)
    if resid is not None:
        y = (resid.to(dtype) + alpha * y.to(dtype)).to(BF16)
    return y


def ffn_probe(M, seed):
    """fused_ffn* inputs. x on k/4 (|k| <= 8); W1 has at most 4 nonzeros in
    {-1, 1} per hidden unit and b1 in {0, +-0.25}, so a hidden pre-activation
    is a multiple of 1/4 of magnitude <= 8.25: 6 significant bits, and its
    bf16 rounding is the identity. W2 dense in {-1,0,1}, b2 on the grid."""
    x = grid_tensor((M, 280), 1 / 4, 8, seed)
    g = torch.Generator().manual_seed(seed + 1)
    w1 = torch.zeros(2048, 280, dtype=torch.float64)
    cols = torch.randint(0, 280, (2048, 4), generator=g)
    sign = torch.randint(0, 2, (2048, 4), generator=g).double() * 2 - 1
    # Colliding columns overwrite: "at most" 4 nonzeros, each still +-1.
    w1.scatter_(1, cols, sign)
    b1 = torch.randint(-1, 2, (2048,), generator=g).double() * 0.25
    w2 = torch.randint(-1, 2, (280, 2048), generator=g).double()
    b2 = grid_tensor((280,), 1 / 4, 8, seed + 2)
    return x, w1, b1, w2, b2


def ffn_ref(x, w1, b1, w2, b2, alpha, dtype=torch.float64, perm1=None,
            perm2=None):
    """bf16(x + alpha * (bf16(relu(x W1^T + b1)) W2^T + b2)) in `dtype`."""
    xd, w1d = x.to(dtype), w1.to(dtype)
    if perm1 is not None:
        h = xd[:, perm1] @ w1d[:, perm1].t()
    else:
        h = xd @ w1d.t()
    h = torch.relu(h + b1.to(dtype)).to(BF16).to(dtype)
    w2d = w2.to(dtype)
    if perm2 is not None:
        h, w2d = h[:, perm2], w2d[:, perm2]
    y = h @ w2d.t() + b2.to(dtype)
    return (xd + alpha * y).to(BF16)


def ffn_images(w1, b1, w2, b2):
    """Host weight layouts as models/runner.py builds them (CPU tensors):
    w1_pad [2048,288] + b1 fp32 (v1); w1_v2 [2048,296] with b1 folded into
    column 287 (v2/v3/v5); w2_pad [320,2048]; b2 fp32 [320]."""
    w1_pad = torch.zeros(2048, 288)
    w1_pad[:, :280] = w1.float()
    w1_v2 = torch.zeros(2048, 296)
    w1_v2[:, :280] = w1.float()
    w1_v2[:, 287] = b1.float()
    w2_pad = torch.zeros(320, 2048)
    w2_pad[:280] = w2.float()
    b2_pad = torch.zeros(320)
    b2_pad[:280] = b2.float()
    return dict(w1_pad=w1_pad.to(BF16), b1=b1.float(), w1_v2=w1_v2.to(BF16),
                w2_pad=w2_pad.to(BF16), b2=b2_pad)


def first_mismatch(got: torch.Tensor, ref: torch.Tensor):
    """(count, (row, col) of the first bitwise difference) of two bf16
    matrices, or (0, None)."""
    ne = got.view(torch.int16) != ref.view(torch.int16)
    n = int(ne.sum())
    if n == 0:
        return 0, None
    r, c = ne.nonzero()[0].tolist()
    return n, (r, c)


# ---------------------------------------------------------------------------
# fused_ln_head_qv
# ---------------------------------------------------------------------------

LN_EPS = 1e-6
LN_CS = (0.0, 5.0, 20.0, 100.0, 300.0)
LN_RATIOS = (1.0, 1e-1, 1e-2, 1e-3, 1e-4)
LN_HS = (64, 65, 280, 512)
LN_REPS = 4


def ln_rows(H, seed):
    """Rows c + s*N(0,1) for every (c, s/|c|) pair (s itself at c = 0),
    LN_REPS draws each, then one exactly constant row per c. fp32 [R, H].
    Returns (x, labels) with labels[r] = (c, s)."""
    g = torch.Generator().manual_seed(seed)
    rows, labels = [], []
    for c in LN_CS:
        for ratio in LN_RATIOS:
            s = ratio * (abs(c) if c != 0 else 1.0)
            for _ in range(LN_REPS):
                rows.append(c + s * torch.randn(H, generator=g))
                labels.append((c, s))
    for c in LN_CS + (5.3,):
        rows.append(torch.full((H,), c))
        labels.append((c, 0.0))
    return torch.stack(rows).float(), labels


def ln_params_random(H, seed):
    g = torch.Generator().manual_seed(seed)
    gamma = 1.0 + 0.3 * torch.randn(H, generator=g)
    beta = 0.3 * torch.randn(H, generator=g)
    w_head = torch.randn(5, H, generator=g) * H ** -0.5
    b_head = 0.5 * torch.randn(5, generator=g)
    return gamma, beta, w_head, b_head


def ln_params_model():
    """The final LayerNorm and head of the flagship model (H = 280), as
    models/runner.py hands them to the kernel."""
    from deepconsensus_amd.models import config as cfg
    from deepconsensus_amd.models.model import get_model

    params = cfg.get_config("transformer_learn_values+custom")
    cfg.modify_params(params, is_training=False)
    torch.manual_seed(0)
    model = get_model(params)
    return (model.output_norm.weight.detach().float(),
            model.output_norm.bias.detach().float(),
            model.fc1.weight.detach().float().contiguous(),
            model.fc1.bias.detach().float())


def ln_param_sets(H):
    """[(name, (gamma, beta, w_head, b_head))] to run at width H."""
    sets = [("random", ln_params_random(H, 900 + H))]
    if H == 280:
        sets.append(("model", ln_params_model()))
    return sets


def ln_inputs(H):
    """[(dtype name, x as the kernel receives it)] at width H."""
    x, _ = ln_rows(H, 800 + H)
    return [("fp32", x), ("bf16", x.to(BF16))]


def ln_head_ref(x, gamma, beta, w_head, b_head, dtype=torch.float64):
    """LayerNorm(eps 1e-6) -> Dense(5) -> softmax on x as given."""
    xd = x.to(dtype)
    n = torch.nn.functional.layer_norm(
        xd, (xd.shape[-1],), gamma.to(dtype), beta.to(dtype), LN_EPS)
    logits = n @ w_head.to(dtype).t() + b_head.to(dtype)
    return torch.softmax(logits, dim=-1)


# Largest |probs - ref64| of float32 torch layer_norm + float32 head + softmax
# (CPU) over ln_rows at every H in LN_HS, fp32 and bf16-rounded inputs, the
# model's head and ln_params_random. Measured by
# test_kernel_probes.py::test_ln_float32_baseline_is_current. The kernel is
# allowed LN_MARGIN x this (different reduction order, __expf), and never
# less than the suite's existing atol 2e-4 + rtol 1e-3.
# 6.21e-4 is reached at H=65 on the fp32 row 300 + 0.03*N(0,1); the bf16 input
# path alone measures 1.26e-4.
# The two-pass kernel measured 4.25e-4 (fp32 rows) and 1.96e-5 (bf16 rows) on
# an MI355X against the resulting bound of 2.48e-3.
LN_F32_BASELINE_MAX_ERR = 6.21e-4
LN_MARGIN = 4.0
LN_ATOL, LN_RTOL = 2e-4, 1e-3


def ln_bound(ref64: torch.Tensor) -> torch.Tensor:
    floor = LN_ATOL + LN_RTOL * ref64.abs()
    return torch.clamp_min(floor, LN_MARGIN * LN_F32_BASELINE_MAX_ERR)


# ---- exact QV logic --------------------------------------------------------

QV_CALIBS = (
    (-1.0, 1.0, 0.0),
    (0.0, 1.197654, -0.99781),
    (20.0, 1.197654, -0.99781),
    # Not a production setting: the only one here whose line goes negative
    # inside the reachable range (raw q >= 0.97), so it alone hits the floor.
    (0.0, 1.0, -2.6),
)
QV_MAX_QUALS = (93.0, 40.0)
QV_EXACT_BELOW = 45.0      # fp32 cancellation in 1 - pmax moves q < 0.01 here
QV_HALF_GUARD = 0.05
QV_MAX_EXCLUDED = 0.15


def qv_sweep_a() -> np.ndarray:
    """float32 head biases a. With w_head = 0 and b_head = a at one class,
    1 - pmax = 4 / (e^a + 4) for every row. Raw qualities run 0.97 (a = 0,
    the lowest reachable: pmax >= 0.2) to 60 in steps of 0.3, then values
    where 4 e^-a < 2^-25 so that 1 - pmax is exactly 0 in fp32."""
    qt = 1.0 + 0.3 * np.arange(197)          # 1.0 .. 59.8
    ep = 10.0 ** (-qt / 10.0)
    a = np.log(4.0 * (1.0 / ep - 1.0))
    a = np.concatenate([[0.0], a, [20.0, 25.0, 40.0, 80.0]])
    return a.astype(np.float32)


def qv_saturated(a: np.ndarray) -> np.ndarray:
    """1 - pmax is exactly 0 in fp32: denom = 1 + 4 e^-a rounds to 1."""
    return 4.0 * np.exp(-a.astype(np.float64)) < 2.0 ** -25


def qv_ref(a: np.ndarray, calib, max_qual):
    """float64 probs_to_calls on the exact 1 - pmax. Returns (q64 before
    rounding, expected integer quality, exact-comparison mask)."""
    thr, w, b = calib
    ep = 4.0 / (np.exp(a.astype(np.float64)) + 4.0)
    q = -10.0 * np.log10(np.maximum(ep, 1e-300))
    # Once fp32 cannot tell pmax from 1 the quality is the cap, as in
    # probs_to_calls (clamp of 1 - pmax, then the cap).
    q = np.where(qv_saturated(a), 1e9, q)
    q = np.where((thr == 0) | (q > thr), q * w + b, q)
    q = np.minimum(q, max_qual)
    expect = np.maximum(np.rint(q), 0.0)      # rint = round half to even
    off_half = np.abs(q - np.floor(q) - 0.5) > QV_HALF_GUARD
    exact = (q < QV_EXACT_BELOW) & off_half & ~qv_saturated(a)
    return q, expect, exact


def qv_excluded_fraction(a, calib, max_qual) -> float:
    """Share of the sweep points below QV_EXACT_BELOW that the half-integer
    guard takes out of the exact comparison."""
    q, _, exact = qv_ref(a, calib, max_qual)
    zone = (q < QV_EXACT_BELOW) & ~qv_saturated(a)
    return float((zone & ~exact).sum()) / float(zone.sum())
