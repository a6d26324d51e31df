"""Exact-answer probes for the serving kernels (and the attention training
kernels that share their code).

Inputs come from tests/kernel_probes.py and are chosen so that the right
answer is known exactly or to one bf16 rounding: attention probabilities are
read out through a one-hot V, the GEMM kernels run on a coarse binary grid
where every partial sum is exact in fp32, and the QV logic is driven through
the head bias alone. A wrong kernel then shows as a bitwise mismatch at a
named row and column. References are float64 on the CPU; the premises are
proven without a GPU in tests/test_kernel_probes.py.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_probes as kp  # noqa: E402

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ext():
    from deepconsensus_amd import ops

    return ops.get_ext(required=True)


def _bits(t):
    return t.contiguous().view(torch.int16)


# ===========================================================================
# 1. Attention
# ===========================================================================

@functools.lru_cache(maxsize=None)
def _attn_case(kind, B, L, H, D, win):
    """(q, k, P64) on the CPU for one probe kind; built once per shape."""
    seed = 1000 + 7 * L + 3 * win + H + D
    if kind == "uniform":
        _, k = kp.make_qk(B, L, H, D, seed)
        q = torch.zeros_like(k)
    elif kind == "random":
        q, k = kp.make_qk(B, L, H, D, seed)
    else:
        q, k = kp.make_qk(B, L, H, D, seed, logit_peak=150.0, win=win)
    return q, k, kp.p64(q, k, win)


def _fwd_packed(fn):
    """fn(qkv_cuda) -> [B, L, H*D]; returns out [B, L, H, D] on the CPU."""
    def run(q, k, v):
        B, L, H, D = q.shape
        return fn(kp.pack_qkv(q, k, v).cuda()).cpu().view(B, L, H, D)
    return run


def _fwd_bhtd(fn):
    """fn(q, k, v as [B,H,T,D] cuda) -> [B,H,T,D]; out [B, L, H, D] CPU."""
    def run(q, k, v):
        a = [t.permute(0, 2, 1, 3).contiguous().cuda() for t in (q, k, v)]
        return fn(*a).cpu().permute(0, 2, 1, 3).contiguous()
    return run


def _check_probe(run, kind, B, L, H, D, win, tag):
    q, k, P = _attn_case(kind, B, L, H, D, win)
    out = run(q, k, kp.onehot_v(B, L, H, D))
    hit = kp.probe_hit_mask(L, D, win)[None, :, None, :].expand(B, L, H, D)
    nz = (_bits(out) != 0) & ~hit
    assert not nz.any(), (
        f"{tag} {kind}: nonzero off-band element at (b,i,h,d)="
        f"{kp.first_bad(~nz)}")
    if kind == "uniform":
        n = kp.band_counts(L, win).double()
        exp = (hit.double() / n[None, :, None, None]).to(BF16)
        ne = _bits(out) != _bits(exp)
        where = kp.first_bad(~ne)
        assert not ne.any(), (
            f"{tag} uniform: (b,i,h,d)={where} got {out[where].item()} want "
            f"bf16(1/{int(n[where[1]])})")
    else:
        assert torch.isfinite(out.float()).all(), f"{tag} {kind}: non-finite"
        exp = kp.probe_expected(P, D)
        ok = kp.attn_within_bound(out, exp)
        where = kp.first_bad(ok)
        assert ok.all(), (
            f"{tag} {kind}: (b,i,h,d)={where} got {out[where].item()} "
            f"want {exp[where].item()}")


KINDS = ("uniform", "random", "large")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L,win,H", kp.MFMA_CASES)
def test_banded_attn_mfma_probe(ext, L, win, H, kind):
    D = 140
    run = _fwd_packed(lambda qkv: ext.banded_attn_mfma(qkv, H, win, D ** -0.5))
    _check_probe(run, kind, 2, L, H, D, win, f"mfma L={L} win={win} H={H}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L,win,H", kp.MFMA_CASES)
def test_banded_attn_mfma_train_fwd_probe(ext, L, win, H, kind):
    """Same probes on `out`, and the returned band P against P64."""
    D, B = 140, 2
    saved = {}

    def fn(qkv):
        out, p = ext.banded_attn_mfma_train_fwd(
            qkv, H, win, D ** -0.5, qkv.new_empty(0), 0.0)
        saved["p"] = p.cpu()
        return out

    tag = f"mfma_train L={L} win={win} H={H}"
    _check_probe(_fwd_packed(fn), kind, B, L, H, D, win, tag)
    p = saved["p"]
    assert p.shape == (B * H, L, 2 * win + 1)
    _check_band_p(p, _attn_case(kind, B, L, H, D, win)[2], win, tag)


def _check_band_p(p, P, win, tag):
    L = P.shape[-1]
    ref = kp.band_slots(P, win)
    invalid = ~kp.slot_valid(L, win)
    assert (_bits(p)[:, invalid] == 0).all(), f"{tag}: P slot past the ends"
    ok = kp.attn_within_bound(p, ref)
    where = kp.first_bad(ok)
    assert ok.all(), (
        f"{tag}: p(item,row,slot)={where} got {p[where].item()} want "
        f"{ref[where].item()}")


def _dropout_expected(p, mask, win, B, H, D, p_drop):
    """bf16(float(p) * keep_inv) where kept, 0 where dropped, laid out as the
    one-hot V reads it: [B, L, H, D]."""
    L, W = p.shape[1], p.shape[2]
    keep_inv = torch.tensor(1.0 / (1.0 - p_drop)).float()
    val = torch.where(mask, p.float() * keep_inv, torch.zeros(())).to(BF16)
    val = val.view(B, H, L, W)
    exp = torch.zeros(B, L, H, D, dtype=BF16)
    i = torch.arange(L)
    for w in range(W):
        j = i - win + w
        ok = (j >= 0) & (j < L)
        exp[:, i[ok], :, j[ok] % D] = val[:, :, i[ok], w].permute(2, 0, 1)
    return exp


@pytest.mark.parametrize("L,win,H", [(32, 1, 2), (65, 6, 3), (100, 12, 2),
                                     (104, 11, 1)])
def test_banded_attn_mfma_train_fwd_dropout_probe(ext, L, win, H):
    D, B, p_drop = 140, 2, 0.25
    q, k, P = _attn_case("random", B, L, H, D, win)
    qkv = kp.pack_qkv(q, k, kp.onehot_v(B, L, H, D)).cuda()
    g = torch.Generator().manual_seed(L + win)
    mask = torch.rand(B * H, L, 2 * win + 1, generator=g) >= p_drop
    out, p = ext.banded_attn_mfma_train_fwd(
        qkv, H, win, D ** -0.5, mask.cuda(), p_drop)
    _, p0 = ext.banded_attn_mfma_train_fwd(
        qkv, H, win, D ** -0.5, qkv.new_empty(0), 0.0)
    assert torch.equal(_bits(p), _bits(p0)), "dropout changed the saved P"
    out, p = out.cpu().view(B, L, H, D), p.cpu()
    exp = _dropout_expected(p, mask, win, B, H, D, p_drop)
    ne = _bits(out) != _bits(exp)
    where = kp.first_bad(~ne)
    assert not ne.any(), (
        f"(b,i,h,d)={where} got {out[where].item()} want {exp[where].item()}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,win", [(32, 1), (32, 12), (100, 1), (100, 12)])
def test_banded_attn_train_fwd_probe(ext, T, win, kind):
    D, B, H = 140, 2, 2
    saved = {}

    def fn(q, k, v):
        out, p = ext.banded_attn_train_fwd(q, k, v, q.new_empty(0), win, 0.0)
        saved["p"] = p.cpu()
        return out

    tag = f"train_fwd T={T} win={win}"
    _check_probe(_fwd_bhtd(fn), kind, B, T, H, D, win, tag)
    p = saved["p"].view(B * H, T, 2 * win + 1)
    _check_band_p(p, _attn_case(kind, B, T, H, D, win)[2], win, tag)


@pytest.mark.parametrize("T,win", [(32, 12), (100, 12)])
def test_banded_attn_train_fwd_dropout_probe(ext, T, win):
    D, B, H, p_drop = 140, 2, 2, 0.25
    q, k, _ = _attn_case("random", B, T, H, D, win)
    v = kp.onehot_v(B, T, H, D)
    a = [t.permute(0, 2, 1, 3).contiguous().cuda() for t in (q, k, v)]
    g = torch.Generator().manual_seed(T + win)
    mask = torch.rand(B, H, T, 2 * win + 1, generator=g) >= p_drop
    out, p = ext.banded_attn_train_fwd(*a, mask.cuda(), win, p_drop)
    out = out.cpu().permute(0, 2, 1, 3).contiguous()
    p = p.cpu().view(B * H, T, -1)
    exp = _dropout_expected(p, mask.view(B * H, T, -1), win, B, H, D, p_drop)
    ne = _bits(out) != _bits(exp)
    where = kp.first_bad(~ne)
    assert not ne.any(), (
        f"(b,i,h,d)={where} got {out[where].item()} want {exp[where].item()}")


GENERIC_CASES = [(100, 4, 70, 12), (120, 2, 140, 12), (128, 2, 160, 15),
                 (1, 2, 140, 12), (13, 1, 32, 12)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L,H,D,win", GENERIC_CASES)
def test_banded_attn_generic_probe(ext, L, H, D, win, kind):
    run = _fwd_packed(lambda qkv: ext.banded_attn(qkv, H, win))
    _check_probe(run, kind, 2, L, H, D, win,
                 f"generic L={L} H={H} D={D} win={win}")


@pytest.mark.parametrize("L,H,D,win", [(129, 1, 140, 12), (100, 1, 161, 12),
                                       (100, 2, 140, 16)])
def test_banded_attn_generic_rejects_past_limits(ext, L, H, D, win):
    qkv = torch.zeros(1, L, 3 * H * D, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError):
        ext.banded_attn(qkv, H, win)


@pytest.mark.parametrize("L,win", [(31, 12), (105, 12), (100, 13), (100, 0)])
def test_banded_attn_mfma_rejects_past_limits(ext, L, win):
    qkv = torch.zeros(1, L, 3 * 2 * 140, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError):
        ext.banded_attn_mfma(qkv, 2, win, 140 ** -0.5)
    with pytest.raises(RuntimeError):
        ext.banded_attn_mfma_train_fwd(qkv, 2, win, 140 ** -0.5,
                                       qkv.new_empty(0), 0.0)


@pytest.mark.parametrize("train", [False, True])
def test_banded_attn_mfma_several_items_per_block(ext, train):
    """B*H = 1040 items on the 512-block persistent grid: every block walks
    two or three items, each with its own q, k, each against P64. First
    reference check of the item loop and the cross-item K/V prefetch."""
    B, H, L, D, win = 520, 2, 32, 140, 6
    q, k, P = _attn_case("random", B, L, H, D, win)
    qkv = kp.pack_qkv(q, k, kp.onehot_v(B, L, H, D)).cuda()
    if train:
        out, p = ext.banded_attn_mfma_train_fwd(
            qkv, H, win, D ** -0.5, qkv.new_empty(0), 0.0)
        _check_band_p(p.cpu(), P, win, "persistent train")
    else:
        out = ext.banded_attn_mfma(qkv, H, win, D ** -0.5)
    out = out.cpu().view(B, L, H, D)
    hit = kp.probe_hit_mask(L, D, win)[None, :, None, :].expand(B, L, H, D)
    assert not ((_bits(out) != 0) & ~hit).any()
    exp = kp.probe_expected(P, D)
    ok = kp.attn_within_bound(out, exp)
    where = kp.first_bad(ok)
    assert ok.all(), (
        f"(b,i,h,d)={where} item {where[0] * H + where[2]}: got "
        f"{out[where].item()} want {exp[where].item()}; "
        f"{int((~ok).sum())} elements off")


# ---- backward ----------------------------------------------------------------

def _assert_bwd(name, grads, ref, T, win):
    rec = kp.BWD_TORCH_BF16_ERR[(T, win)]
    for gname, g, r in zip(("dq", "dk", "dv"), grads, ref):
        err = kp.group_rel_err(g, r, T, win)
        bound = [kp.BWD_MARGIN * c for c in rec[gname]]
        print(f"{name} T={T} win={win} {gname}: rel err (first rows, middle, "
              f"last rows) = " + ", ".join(f"{e:.3e}" for e in err)
              + " bound " + ", ".join(f"{b:.3e}" for b in bound))
        for grp, e, b in zip(("first rows", "middle", "last rows"), err,
                             bound):
            assert e <= b, f"{name} {gname} {grp}: {e:.3e} > {b:.3e}"


@functools.lru_cache(maxsize=None)
def _bwd_case(T, win):
    q, k, v, do = kp.attn_bwd_inputs(kp.BWD_B, kp.BWD_H, T, kp.BWD_D,
                                     700 + T + win)
    return q, k, v, do, kp.attn_bwd_ref64(q, k, v, do, win)


@pytest.mark.parametrize("T,win", kp.BWD_CASES)
def test_banded_attn_train_bwd_row_groups(ext, T, win):
    q, k, v, do, ref = _bwd_case(T, win)
    qc, kc, vc, dc = (t.cuda() for t in (q, k, v, do))
    empty = qc.new_empty(0)
    _, p = ext.banded_attn_train_fwd(qc, kc, vc, empty, win, 0.0)
    grads = ext.banded_attn_train_bwd(qc, kc, vc, p, empty, dc, win, 0.0)
    _assert_bwd("train_bwd", [g.cpu() for g in grads], ref, T, win)


@pytest.mark.parametrize("kernel", ["banded_attn_bwd_mfma",
                                    "banded_attn_train_bwd2"])
@pytest.mark.parametrize("T,win", kp.BWD_CASES)
def test_banded_attn_packed_bwd_row_groups(ext, T, win, kernel):
    B, H, D = kp.BWD_B, kp.BWD_H, kp.BWD_D
    q, k, v, do, ref = _bwd_case(T, win)
    to_bthd = lambda t: t.permute(0, 2, 1, 3).contiguous()  # noqa: E731
    qkv = kp.pack_qkv(to_bthd(q), to_bthd(k), to_bthd(v)).cuda()
    dout = to_bthd(do).reshape(B, T, H * D).cuda()
    empty = qkv.new_empty(0)
    _, p = ext.banded_attn_mfma_train_fwd(qkv, H, win, D ** -0.5, empty, 0.0)
    dqkv = getattr(ext, kernel)(qkv, p, empty, dout, H, win, 0.0).cpu()
    grads = dqkv.view(B, T, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    _assert_bwd(kernel, grads, ref, T, win)


# ===========================================================================
# 2. Projection and FFN: exact-arithmetic GEMM probes
# ===========================================================================

def _assert_bitwise(got, ref, tag):
    n, where = kp.first_mismatch(got, ref)
    assert n == 0, (
        f"{tag}: {n} elements differ, first at (row, col)={where}: got "
        f"{got[where].item()} want {ref[where].item()}")


LIN_NS = [(840, 896), (280, 320), (64, 64), (8, 64)]
LIN_MS = [1, 31, 32, 33, 127, 128, 129, 257]
HUGE = 3e38


def _with_tail(t):
    """t as the first rows of a buffer whose next 128 rows hold 3e38."""
    big = torch.cat([t, torch.full((128, t.shape[1]), HUGE, dtype=t.dtype,
                                   device=t.device)])
    return big[: t.shape[0]]


@pytest.mark.parametrize("N,Npad", LIN_NS)
@pytest.mark.parametrize("M", LIN_MS)
def test_fused_linear_exact(ext, M, N, Npad):
    x64, w64, w_img64, b64 = kp.linear_probe(M, N, Npad, 3000 + M + N,
                                             bias=True)
    x = x64.to(BF16).cuda()
    w_img = w_img64.to(BF16).cuda()
    w_dirty = w_img.clone()
    w_dirty[N:] = 1e4                     # padded weight rows must not leak
    bias = b64.float().cuda()
    empty = x.new_empty(0)
    variants = [("plain", dict(), (empty, empty, N, False, 0.0)),
                ("bias+relu", dict(b=b64, relu=True),
                 (bias, empty, N, True, 0.0))]
    resid = None
    if N == 280:
        r64 = kp.grid_tensor((M, 280), 1 / 8, 16, 4000 + M)
        resid = r64.to(BF16).cuda()
        for alpha in (0.5, 1.0, -2.0):
            variants.append((f"resid alpha={alpha}",
                             dict(resid=r64, alpha=alpha),
                             (empty, resid, N, False, alpha)))
    for name, ref_kw, args in variants:
        tag = f"fused_linear M={M} N={N} {name}"
        ref = kp.linear_ref(x64, w64, **ref_kw)
        out = ext.fused_linear(x, w_img, *args).cpu()
        assert out.shape == (M, N)
        _assert_bitwise(out, ref, tag)
        # Rows past M (x and resid) and weight rows past N are never read
        # into a result.
        t_args = list(args)
        if args[1].numel() > 0:
            t_args[1] = _with_tail(resid)
        out_t = ext.fused_linear(_with_tail(x), w_dirty, *t_args).cpu()
        _assert_bitwise(out_t, ref, tag + " (3e38 tail, 1e4 pad rows)")


def test_fused_linear_wrapper_checks(ext):
    x = torch.zeros(4, 280, dtype=BF16, device="cuda")
    w = torch.zeros(64, 296, dtype=BF16, device="cuda")
    empty = x.new_empty(0)
    assert ext.fused_linear(x, w, empty, empty, 8, False, 0.0).shape == (4, 8)
    for n_out in (12, 7, 63):
        with pytest.raises(RuntimeError, match="multiple of 8"):
            ext.fused_linear(x, w, empty, empty, n_out, False, 0.0)
    with pytest.raises(RuntimeError):
        ext.fused_linear(x, w.float(), empty, empty, 8, False, 0.0)
    with pytest.raises(RuntimeError):
        ext.fused_linear(x, w.cpu(), empty, empty, 8, False, 0.0)
    w_t = torch.zeros(296, 64, dtype=BF16, device="cuda").t()
    assert w_t.shape == (64, 296) and not w_t.is_contiguous()
    with pytest.raises(RuntimeError):
        ext.fused_linear(x, w_t, empty, empty, 8, False, 0.0)


FFN_MS = [1, 129, 255, 256, 257, 513]


@pytest.fixture(scope="module")
def ffn_weights():
    _, w1, b1, w2, b2 = kp.ffn_probe(1, 50)
    img = {k: v.cuda() for k, v in kp.ffn_images(w1, b1, w2, b2).items()}
    return (w1, b1, w2, b2), img


def _ffn_call(ext, kernel, x, img, alpha):
    if kernel == "fused_ffn":
        return ext.fused_ffn(x, img["w1_pad"], img["b1"], img["w2_pad"],
                             img["b2"], alpha)
    if kernel.startswith("fused_ffn_v5"):
        mb = int(kernel.split(":")[1])
        return ext.fused_ffn_v5(x, img["w1_v2"], img["w2_pad"], img["b2"],
                                alpha, mb)
    return getattr(ext, kernel)(x, img["w1_v2"], img["w2_pad"], img["b2"],
                                alpha)


@pytest.mark.parametrize("kernel", ["fused_ffn", "fused_ffn_v2",
                                    "fused_ffn_v3", "fused_ffn_v5:0",
                                    "fused_ffn_v5:1", "fused_ffn_v5:3"])
@pytest.mark.parametrize("M", FFN_MS)
def test_fused_ffn_exact(ext, ffn_weights, M, kernel):
    (w1, b1, w2, b2), img = ffn_weights
    x64 = kp.grid_tensor((M, 280), 1 / 4, 8, 60 + M)
    x = x64.to(BF16).cuda()
    for alpha in (0.5, 1.0):
        ref = kp.ffn_ref(x64, w1, b1, w2, b2, alpha)
        out = _ffn_call(ext, kernel, x, img, alpha).cpu()
        assert out.shape == (M, 280)
        _assert_bitwise(out, ref, f"{kernel} M={M} alpha={alpha}")


# ===========================================================================
# 3. fused_ln_head_qv
# ===========================================================================

def _ln_call(ext, x, params, calib=(-1.0, 1.0, 0.0), max_qual=93.0):
    g, b, w, bh = (t.float().cuda() for t in params)
    return ext.fused_ln_head_qv(x.cuda(), g, b, w, bh, *calib, max_qual, True)


@pytest.mark.parametrize("H", kp.LN_HS)
def test_ln_head_conditioning(ext, H):
    """Near-constant rows c + s*N(0,1), s/|c| down to 1e-4, and constant rows:
    finite probs within 4x the float32 torch layer_norm error (measured:
    6.21e-4, kernel_probes.LN_F32_BASELINE_MAX_ERR) and never tighter than
    atol 2e-4 + rtol 1e-3. The one-pass variance this kernel used to have
    fails here on the fp32 rows with c >= 20 and s/|c| <= 1e-3 (NaN probs)."""
    _, labels = kp.ln_rows(H, 800 + H)
    for pname, params in kp.ln_param_sets(H):
        for dname, x in kp.ln_inputs(H):
            tag = f"H={H} {pname} {dname}"
            ref = kp.ln_head_ref(x, *params)
            bases, quals, probs = (t.cpu() for t in _ln_call(ext, x, params))
            fin = torch.isfinite(probs).all(-1)
            assert fin.all(), (
                f"{tag}: non-finite probs on rows (c, s) "
                f"{[labels[i] for i in (~fin).nonzero().flatten().tolist()]}")
            err = (probs.double() - ref).abs()
            print(f"{tag}: max |probs - ref64| = {err.max().item():.3e}")
            ok = err <= kp.ln_bound(ref)
            where = kp.first_bad(ok)
            assert ok.all(), (
                f"{tag}: row {where[0]} (c, s)={labels[where[0]]} class "
                f"{where[1]}: got {probs[where].item()} want "
                f"{ref[where].item()}")
            # The call follows the reference wherever the reference is clear.
            top2 = ref.topk(2, dim=-1).values
            clear = (top2[:, 0] - top2[:, 1]) > 2 * kp.ln_bound(ref).max()
            assert torch.equal(bases[clear].long(), ref.argmax(-1)[clear])


@pytest.mark.parametrize("N", [1, 3, 5, 8197])
@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_ln_head_persistent_loop(ext, N, dtype):
    """N = 8197 > 2048 blocks x 4 waves (and no multiple of 4): positions
    handled on a wave's second trip match the float64 reference too."""
    H = 280
    g = torch.Generator().manual_seed(N)
    x = (2.0 * torch.randn(N, H, generator=g)).to(dtype)
    params = kp.ln_params_random(H, 31)
    ref = kp.ln_head_ref(x, *params)
    bases, quals, probs = (t.cpu() for t in _ln_call(ext, x, params))
    assert probs.shape == (N, 5) and bases.shape == (N,)
    err = (probs.double() - ref).abs()
    ok = err <= kp.LN_ATOL + kp.LN_RTOL * ref
    where = kp.first_bad(ok)
    assert ok.all(), (
        f"row {where[0]} class {where[1]}: got {probs[where].item()} want "
        f"{ref[where].item()}")
    top2 = ref.topk(2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3
    assert torch.equal(bases[clear].long(), ref.argmax(-1)[clear])
    # Qualities follow from the kernel's own probs (float64 logic) to +-1,
    # on every row including the last partial block.
    pmax = probs.double().max(-1).values
    q = (-10 * torch.log10((1 - pmax).clamp_min(1e-12))).clamp(max=93.0)
    assert ((quals.double() - torch.round(q)).abs() <= 1).all()


@pytest.mark.parametrize("max_qual", kp.QV_MAX_QUALS)
@pytest.mark.parametrize("calib", kp.QV_CALIBS)
def test_ln_head_qv_exact(ext, calib, max_qual):
    """w_head = 0, b_head = a at one class: 1 - pmax = 4/(e^a + 4) on every
    row whatever x holds, so the integer quality is known in float64."""
    H, N = 280, 5
    a = kp.qv_sweep_a()
    q64, expect, exact = kp.qv_ref(a, calib, max_qual)
    sat = kp.qv_saturated(a)
    g = torch.Generator().manual_seed(17)
    x = (3.0 * torch.randn(N, H, generator=g) + 1.0).cuda()
    gamma, beta, _, _ = (t.cuda() for t in kp.ln_params_random(H, 5))
    w_head = torch.zeros(5, H, device="cuda")
    a_dev = torch.from_numpy(a).cuda()
    for cls in range(5):
        bh = torch.zeros(len(a), 5, device="cuda")
        bh[:, cls] = a_dev
        outs = [ext.fused_ln_head_qv(x, gamma, beta, w_head, bh[i], *calib,
                                     max_qual, False) for i in range(len(a))]
        bases = torch.stack([o[0] for o in outs]).cpu().numpy()
        quals = torch.stack([o[1] for o in outs]).cpu().numpy().astype(float)
        # a = 0 is a five-way tie: the first maximum wins, as in torch.max.
        want_base = np.where(a > 0, cls, 0)[:, None]
        assert (bases == want_base).all(), f"class {cls}: wrong base"
        assert (quals == quals[:, :1]).all(), "quality depends on x"
        got = quals[:, 0]
        bad = exact & (got != expect)
        assert not bad.any(), (
            f"class {cls} calib {calib} cap {max_qual}: a={a[bad][0]} "
            f"q64={q64[bad][0]:.4f} got {got[bad][0]} want {expect[bad][0]}")
        assert (np.abs(got - expect)[~exact & ~sat] <= 1).all()
        assert (got[sat] == max_qual).all()
        assert got.min() >= 0 and got.max() <= max_qual


@pytest.mark.parametrize("c", [0.0, 1.5, -3.0])
def test_ln_head_all_equal_bias_calls_base_zero(ext, c):
    H = 280
    x = torch.randn(5, H, generator=torch.Generator().manual_seed(2)).cuda()
    gamma, beta, _, _ = (t.cuda() for t in kp.ln_params_random(H, 5))
    bases, quals, probs = ext.fused_ln_head_qv(
        x, gamma, beta, torch.zeros(5, H, device="cuda"),
        torch.full((5,), c, device="cuda"), -1.0, 1.0, 0.0, 93.0, True)
    assert (bases == 0).all()
    assert ((probs - 0.2).abs() < 1e-6).all()
    assert (quals == 1).all()          # -10 log10(0.8) = 0.97
