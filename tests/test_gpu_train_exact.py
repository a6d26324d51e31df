"""Exact-answer probes for the training kernels: ffn_train_fwd/dgrad,
resid_drop_fwd/bwd, embed_grad and alignment_dp_fwd/bwd.

Inputs and references come from tests/train_probes.py. The dropout masks are
predicted by numpy twins of the kernels' integer hashes, not read back from
the kernel; on the grid-valued inputs every partial sum is exact in fp32, so
results compare bitwise. A wrong kernel shows as a mismatch at a named row
and column. The premises are proven without a GPU in
tests/test_train_probes.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_probes as kp  # noqa: E402
import train_probes as tp  # noqa: E402

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ext():
    from deepconsensus_amd import ops

    return ops.get_ext(required=True)


def _assert_bitwise(got, ref, tag):
    assert got.shape == ref.shape, f"{tag}: shape {tuple(got.shape)}"
    n, where = kp.first_mismatch(got, ref)
    assert n == 0, (
        f"{tag}: {n} elements differ, first at (row, col)={where}: got "
        f"{got[where].item()} want {ref[where].item()}")


def _assert_within(got, ref64, bound, tag):
    ok = torch.isfinite(got.double()) & ((got.double() - ref64).abs() <= bound)
    where = kp.first_bad(ok)
    assert ok.all(), (
        f"{tag}: (row, col)={where} got {got[where].item()} want "
        f"{ref64[where].item()} bound {bound[where].item():.3e}")


# ===========================================================================
# 2. ffn_train_fwd
# ===========================================================================

@pytest.fixture(scope="module")
def ffn_weights():
    _, w1, b1, w2, b2 = kp.ffn_probe(1, tp.FFN_WEIGHT_SEED)
    img = {k: v.cuda() for k, v in kp.ffn_images(w1, b1, w2, b2).items()}
    s_img, d_img = (t.cuda() for t in tp.dgrad_images(w1, w2))
    return (w1, b1, w2, b2), img, (s_img, d_img)


@pytest.mark.parametrize("M", tp.FFN_MS)
def test_ffn_train_fwd_exact(ext, ffn_weights, M):
    """hd and y bitwise for p in {0, 0.5, 0.75} with the mask the numpy twin
    predicts from (seed, global row, hidden index); p = 0.1 keeps hd bitwise
    and y under 2^-8 |ref| + 2^-12 sum|hd w|. x ends in 256 NaN rows."""
    (w1, b1, w2, b2), img, _ = ffn_weights
    x64 = kp.grid_tensor((M, 280), 1 / 4, 8, 160 + M)
    x = tp.with_nan_tail(x64.to(BF16).cuda())
    for pi, p in enumerate(tp.FFN_PS_EXACT + (tp.FFN_P_GENERAL,)):
        seed = tp.SEEDS[(tp.FFN_MS.index(M) + pi) % len(tp.SEEDS)]
        tag = f"ffn_train_fwd M={M} p={p} seed={seed}"
        hd_ref, y64, terms, keep = tp.ffn_fwd_ref(x64, w1, b1, w2, b2, p,
                                                  seed)
        y, hd = ext.ffn_train_fwd(x, img["w1_v2"], img["w2_pad"], img["b2"],
                                  p, seed)
        y, hd = y.cpu(), hd.cpu()
        _assert_bitwise(hd, hd_ref, tag + " hd")
        if p in tp.FFN_PS_EXACT:
            _assert_bitwise(y, y64.to(BF16), tag + " y")
        else:
            _assert_within(y, y64, tp.y_bound(y64, terms), tag + " y")
        if M == 513 and p > 0:
            # Global row index: the second tile's mask is its own.
            assert not torch.equal(keep[256:512], keep[:256])
            live = hd_ref[256:512].float() > 0
            got = hd[256:512].float() > 0
            assert torch.equal(got, live & keep[256:512]), (
                tag + ": rows 256..511 do not follow the twin's mask")


# ===========================================================================
# 3. ffn_train_dgrad
# ===========================================================================

@pytest.mark.parametrize("M", tp.FFN_MS)
def test_ffn_train_dgrad_exact(ext, ffn_weights, M):
    """dh_pre and dx bitwise for p in {0, 0.5, 0.75} on an hd the test
    supplies (positives, +0, -0.0, negatives; the rule is hd > 0); p = 0.1
    keeps dh_pre bitwise and bounds dx. dy and hd end in 256 NaN rows."""
    (w1, _, w2, _), _, (s_img, d_img) = ffn_weights
    dy64 = kp.grid_tensor((M, 280), 1 / 4, 8, 260 + M)
    hd = tp.dgrad_hd(M)
    dy_d = tp.with_nan_tail(dy64.to(BF16).cuda())
    hd_d = tp.with_nan_tail(hd.cuda())
    for p in tp.FFN_PS_EXACT + (tp.FFN_P_GENERAL,):
        tag = f"ffn_train_dgrad M={M} p={p}"
        dh_ref, dx64, terms = tp.ffn_dgrad_ref(dy64, hd, w1, w2, p)
        dx, dh = ext.ffn_train_dgrad(dy_d, hd_d, s_img, d_img, p)
        dx, dh = dx.cpu(), dh.cpu()
        _assert_bitwise(dh, dh_ref, tag + " dh_pre")
        if p in tp.FFN_PS_EXACT:
            _assert_bitwise(dx, dx64.to(BF16), tag + " dx")
        else:
            _assert_within(dx, dx64, tp.y_bound(dx64, terms), tag + " dx")


@pytest.mark.parametrize("M", [1, 33, 257])
def test_ffn_train_dgrad_ones_equals_nomask(ext, ffn_weights, M):
    _, _, (s_img, d_img) = ffn_weights
    dy = kp.grid_tensor((M, 280), 1 / 4, 8, 360 + M).to(BF16).cuda()
    ones = torch.ones(M, 2048, dtype=BF16, device="cuda")
    dx, dh = ext.ffn_train_dgrad(dy, ones, s_img, d_img, 0.0)
    dx2, dh2 = ext.ffn_train_dgrad_nomask(dy, ones, s_img, d_img, 0.0)
    _assert_bitwise(dh.cpu(), dh2.cpu(), f"dgrad vs nomask M={M} dh_pre")
    _assert_bitwise(dx.cpu(), dx2.cpu(), f"dgrad vs nomask M={M} dx")


def test_ffn_train_fused_end_to_end(ext):
    """_FFNTrainFused at M = 257, p = 0.5: y and dx bitwise, the weight and
    bias gradients against the float64 chain built from the twin's mask."""
    from deepconsensus_amd.models.model import _FFNTrainFused

    M, p, seed = 257, 0.5, tp.SEEDS[3]
    x64, w1, b1, w2, b2, dy64 = tp.ffn_e2e_probe(M, 400)
    ref = tp.ffn_e2e_ref(x64, w1, b1, w2, b2, dy64, p, seed)
    x = x64.to(BF16).cuda().requires_grad_()
    params = [t.float().cuda().requires_grad_() for t in (w1, b1, w2, b2)]
    y = _FFNTrainFused.apply(x, *params, p, seed)
    y.backward(dy64.to(BF16).cuda())
    _assert_bitwise(y.detach().cpu(), ref["y"].to(BF16), "FFNTrainFused y")
    _assert_bitwise(x.grad.cpu(), ref["dx"].to(BF16), "FFNTrainFused dx")
    for name, t in zip(("dw1", "db1", "dw2", "db2"), params):
        r = ref[name]
        torch.testing.assert_close(
            t.grad.cpu().double(), r, rtol=2.0 ** -7,
            atol=2.0 ** -7 * r.abs().max().item(),
            msg=lambda m, n=name: f"FFNTrainFused {n}: {m}")


# ===========================================================================
# 4. resid_drop_fwd / resid_drop_bwd
# ===========================================================================

def _rd_first_bad(ne):
    i = int(ne.reshape(-1).nonzero()[0])
    return f"element {i} (granule {i // 8}, lane {i % 8})"


def _rd_bitwise(got, ref64, tag):
    ref = ref64.to(BF16)
    ne = got.reshape(-1).view(torch.int16) != ref.view(torch.int16)
    assert not ne.any(), (
        f"{tag}: {int(ne.sum())} differ, first at {_rd_first_bad(ne)}: got "
        f"{got.reshape(-1)[ne][0].item()} want {ref[ne][0].item()}")


def _rd_run_exact(ext, numel, alpha, p, seed, tag, kmax_yd=16, shape=None):
    x, y, dout = tp.rd_inputs(numel, 500 + numel % 1000, kmax_yd)
    out64, dy64, terms = tp.rd_ref(x, y, dout, alpha, p, seed)
    assert float(terms.abs().sum()) < tp.RD_DALPHA_CAP
    dev = [t.to(BF16).cuda() for t in (x, y, dout)]
    if shape is not None:
        dev = [t.view(shape) for t in dev]
    xd, yd, dd = dev
    out = ext.resid_drop_fwd(xd, yd, alpha, p, seed)
    dy, part = ext.resid_drop_bwd(dd, yd, alpha, p, seed)
    assert out.shape == xd.shape and dy.shape == dd.shape
    _rd_bitwise(out.cpu(), out64, f"resid_drop_fwd {tag}")
    _rd_bitwise(dy.cpu(), dy64, f"resid_drop_bwd {tag} dy")
    assert part.shape == (tp.rd_part_len(numel),), (
        f"resid_drop_bwd {tag}: part shape {tuple(part.shape)}")
    got, want = float(part.sum()), float(terms.sum())
    assert got == want, f"resid_drop_bwd {tag}: dalpha {got} want {want}"


@pytest.mark.parametrize("numel", tp.RD_NUMELS)
@pytest.mark.parametrize("p", tp.RD_PS_EXACT)
def test_resid_drop_exact(ext, numel, p):
    for ai, alpha in enumerate(tp.RD_ALPHAS_EXACT):
        for seed in tp.SEEDS:
            _rd_run_exact(ext, numel, alpha, p, seed,
                          f"numel={numel} alpha={alpha} p={p} seed={seed}")


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_resid_drop_grid_stride(ext, p):
    """n8 = 4096*256 + 257 granules: 257 threads take a second trip."""
    numel = 8 * tp.RD_N8_STRIDE
    _rd_run_exact(ext, numel, 0.375, p, tp.SEEDS[3],
                  f"grid-stride numel={numel} p={p}", kmax_yd=1)


@pytest.mark.parametrize("p", [0.5, 0.75])
def test_resid_drop_3d_and_noncontiguous(ext, p):
    B, L = 3, 7
    numel = B * L * 280
    _rd_run_exact(ext, numel, -1.5, p, tp.SEEDS[2], f"3-D [{B},{L},280]",
                  shape=(B, L, 280))
    # A transposed view: the wrapper's contiguous() copy defines the element
    # order, so the answer is that of the materialised tensor.
    x, y, dout = tp.rd_inputs(numel, 77)
    seed = tp.SEEDS[4]
    as_t = lambda t: t.view(280, B * L).t()  # noqa: E731  [B*L, 280] strided
    out64, dy64, terms = tp.rd_ref(
        *(as_t(t).contiguous().view(-1) for t in (x, y, dout)), 0.375, p,
        seed)
    xd, yd, dd = (as_t(t.to(BF16).cuda()) for t in (x, y, dout))
    assert not xd.is_contiguous()
    out = ext.resid_drop_fwd(xd, yd, 0.375, p, seed)
    dy, part = ext.resid_drop_bwd(dd, yd, 0.375, p, seed)
    _rd_bitwise(out.cpu().contiguous(), out64, "resid_drop_fwd strided")
    _rd_bitwise(dy.cpu().contiguous(), dy64, "resid_drop_bwd strided dy")
    assert float(part.sum()) == float(terms.sum())


@pytest.mark.parametrize("numel", tp.RD_NUMELS)
@pytest.mark.parametrize("p", tp.RD_PS_GENERAL)
def test_resid_drop_general(ext, numel, p):
    alpha = tp.RD_ALPHA_GENERAL
    for seed in tp.SEEDS:
        tag = f"numel={numel} alpha={alpha} p={p} seed={seed}"
        x, y, dout = tp.rd_general_inputs(numel, 600 + numel % 1000)
        out64, dy64, terms = tp.rd_ref(x, y, dout, alpha, p, seed)
        xd, yd, dd = (t.to(BF16).cuda() for t in (x, y, dout))
        out = ext.resid_drop_fwd(xd, yd, alpha, p, seed).cpu()
        dy, part = ext.resid_drop_bwd(dd, yd, alpha, p, seed)
        for name, got, ref in (("fwd out", out, out64),
                               ("bwd dy", dy.cpu(), dy64)):
            ok = (got.double() - ref).abs() <= tp.rd_bound(ref)
            where = kp.first_bad(ok)
            assert ok.all(), (
                f"resid_drop {name} {tag}: element {where} got "
                f"{got[where].item()} want {ref[where].item()}")
        # Dropped positions are exact zeros / exact x, not merely small.
        keep = torch.from_numpy(tp.rd_keep(seed, numel, p))
        assert (dy.cpu()[~keep].view(torch.int16) == 0).all(), tag
        assert torch.equal(out[~keep], x.to(BF16)[~keep]), tag
        ref = float(terms.sum())
        mag = float(terms.abs().sum())
        got = float(part.double().sum())
        rel = max(2.0 ** -20 * mag / abs(ref), 1e-5)
        print(f"resid_drop_bwd {tag}: dalpha {got} ref {ref} "
              f"rel err {abs(got - ref) / abs(ref):.3e} bound {rel:.3e}")
        assert abs(got - ref) <= rel * abs(ref), (
            f"resid_drop_bwd {tag}: dalpha {got} want {ref}")


def test_resid_drop_rejects_ragged(ext):
    x = torch.zeros(12, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.resid_drop_fwd(x, x, 0.5, 0.0, 0)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.resid_drop_bwd(x, x, 0.5, 0.0, 0)


# ===========================================================================
# 5. embed_grad
# ===========================================================================

def _eg_call(ext, meta, rows, grad_out, scales, tables):
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")  # noqa
    ext.embed_grad(rows.cuda(), grad_out.float().cuda(), i32(meta.row_shift),
                   i32(meta.row_vocab), i32(meta.row_tbase),
                   i32(meta.row_width), i32(meta.row_col),
                   torch.tensor(scales, dtype=torch.float32, device="cuda"),
                   tables)


def _eg_where(meta, i):
    t = max(k for k in range(len(meta.table_vocab))
            if sorted(set(meta.row_tbase))[k] <= i)
    off = i - sorted(set(meta.row_tbase))[t]
    w = meta.table_width[t]
    return f"table {t} (id, col)=({off // w}, {off % w})"


@pytest.mark.parametrize("B,L", tp.EG_POSITIONS)
def test_embed_grad_exact(ext, B, L):
    """k/8-grid grad_out, power-of-two row scales, grid prefill: the result
    equals the float64 index_add_ exactly in any atomic order."""
    meta = tp.EmbedMetaProbe()
    rows = tp.eg_rows(B, L, 900 + B * L % 1000)
    go = kp.grid_tensor((B, L, meta.C), 1 / 8, 16, 901 + B * L % 1000)
    prefill = kp.grid_tensor((meta.tbl_elems,), 1 / 8, 16, 902)
    ref, mag = tp.eg_ref(rows, go, meta.scale_exact, prefill, meta.tbl_elems)
    assert float(mag.max()) < tp.EG_EXACT_CAP
    tables = prefill.float().cuda()
    _eg_call(ext, meta, rows, go, meta.scale_exact, tables)
    got = tables.cpu().double()
    ne = got != ref
    if ne.any():
        i = int(ne.nonzero()[0])
        raise AssertionError(
            f"embed_grad B*L={B * L}: {int(ne.sum())} cells differ, first "
            f"{_eg_where(meta, i)}: got {got[i].item()} want {ref[i].item()} "
            f"(prefill {prefill[i].item()})")


@pytest.mark.parametrize("B,L", tp.EG_POSITIONS)
def test_embed_grad_real_scale(ext, B, L):
    meta = tp.EmbedMetaProbe()
    rows = tp.eg_rows(B, L, 910 + B * L % 1000)
    g = torch.Generator().manual_seed(911)
    go = torch.randn(B, L, meta.C, generator=g).float().double()
    prefill = torch.randn(meta.tbl_elems, generator=g).float().double()
    ref, mag = tp.eg_ref(rows, go, meta.scale_real, prefill, meta.tbl_elems)
    tables = prefill.float().cuda()
    _eg_call(ext, meta, rows, go, meta.scale_real, tables)
    got = tables.cpu().double()
    ok = (got - ref).abs() <= 2.0 ** -20 * mag
    if not ok.all():
        i = int((~ok).nonzero()[0])
        raise AssertionError(
            f"embed_grad real-scale B*L={B * L}: {_eg_where(meta, i)}: got "
            f"{got[i].item()} want {ref[i].item()} bound "
            f"{2.0 ** -20 * mag[i].item():.3e}")


def test_embed_grad_table_limit(ext):
    """12288 table elements fit the LDS accumulator; 12289 raise. The
    elements past the tables the metadata names stay untouched."""
    meta = tp.EmbedMetaProbe()
    rows = tp.eg_rows(1, 257, 920)
    go = kp.grid_tensor((1, 257, meta.C), 1 / 8, 16, 921)
    prefill = kp.grid_tensor((tp.EG_MAX_TBL,), 1 / 8, 16, 922)
    ref, _ = tp.eg_ref(rows, go, meta.scale_exact,
                       prefill[: meta.tbl_elems], meta.tbl_elems)
    tables = prefill.float().cuda()
    _eg_call(ext, meta, rows, go, meta.scale_exact, tables)
    got = tables.cpu().double()
    assert torch.equal(got[: meta.tbl_elems], ref), "embed_grad at 12288"
    assert torch.equal(got[meta.tbl_elems:], prefill[meta.tbl_elems:])
    big = torch.zeros(tp.EG_MAX_TBL + 1, device="cuda")
    with pytest.raises(RuntimeError, match="too large"):
        _eg_call(ext, meta, rows, go, meta.scale_exact, big)


# ===========================================================================
# 6. alignment_dp_fwd / alignment_dp_bwd
# ===========================================================================

def _dp_run(ext, subs, ins, seq_lens, del_cost, reg, width, grad_out):
    B, m, n = subs.shape
    r = 0.0 if reg is None else reg
    w = 0 if width is None else width
    sl = seq_lens.cuda()
    loss, weights = ext.alignment_dp_fwd(subs.cuda(), ins.cuda(), sl,
                                         del_cost, r, w)
    gs, gi = ext.alignment_dp_bwd(grad_out.float().cuda(), weights, sl, m, n,
                                  w)
    return loss.cpu(), gs.cpu(), gi.cpu()


def _dp_first_cell(ok):
    where = kp.first_bad(ok)
    return f"example {where[0]} cell {tuple(x + 1 for x in where[1:])}"


DP_MEASURED = {}


@pytest.mark.parametrize("m,n", tp.DP_SHAPES)
def test_alignment_dp_against_direct_dp(ext, m, n):
    """Loss and both gradients of every (width, reg) combo against the
    cell-by-cell float64 DP. Soft min: within 4x the float32 CPU path's own
    error (train_probes.DP_F32_BASELINE), never tighter than the suite's
    present tolerances. Hard min on these continuous costs: the loss only
    (gradients at near-ties are checked by the gap-guarded test below).

    seq_len 0 with width 1 or n = 1 (k_end <= 1) is checked here against the
    direct DP, V[0][1] = ins[0] with its gradient on ins[0]; the CPU
    wavefront path returns 1e9 there, so that comparison leaves it out."""
    for ci, c in enumerate(tp.dp_shape_cases(m, n)):
        width, reg, kind = c["width"], c["reg"], c["kind"]
        tag = (f"alignment_dp m={m} n={n} width={width} reg={reg} "
               f"del={c['del_cost']} {kind}")
        loss, gs, gi = _dp_run(ext, c["subs"], c["ins"], c["seq_lens"],
                               c["del_cost"], reg, width, c["grad_out"])
        rl, rs, ri = c["ref"]
        unreach = tp.dp_unreachable(c["seq_lens"], n, width)
        assert (loss[unreach] == 1e9).all() and (rl[unreach] == 1e9).all(), (
            f"{tag}: unreachable end cell must give 1e9")
        assert (gs[unreach] == 0).all() and (gi[unreach] == 0).all(), tag
        assert (rs[unreach] == 0).all() and (ri[unreach] == 0).all(), tag
        div = tp.dp_divergent(c["seq_lens"], n, width)
        for b in div.nonzero().flatten().tolist():
            assert loss[b] == c["ins"][b, 0], f"{tag}: k_end<=1 example {b}"
            assert gi[b, 0] == c["grad_out"][b] and (gi[b, 1:] == 0).all()
            assert (gs[b] == 0).all()
        assert torch.isfinite(loss).all() and torch.isfinite(gs).all()
        if reg is None:
            allow = (1.0, None, None)
        else:
            allow = tp.dp_allowed(reg, kind)
        errs = (tp.dp_err_norm(loss, rl, tp.DP_LOSS_TOL),
                tp.dp_err_norm(gs, rs, tp.DP_GRAD_TOL),
                tp.dp_err_norm(gi, ri, tp.DP_GRAD_TOL))
        print(f"{tag}: err_norm loss {errs[0]:.3e} grad_subs {errs[1]:.3e} "
              f"grad_ins {errs[2]:.3e} allowed {allow}")
        if reg is not None:
            key = (reg, kind)
            DP_MEASURED[key] = tuple(
                max(a, b) for a, b in zip(DP_MEASURED.get(key, (0, 0, 0)),
                                          errs))
        a, r = tp.DP_LOSS_TOL
        ok = (loss.double() - rl).abs() <= allow[0] * (a + r * rl.abs())
        assert ok.all(), (
            f"{tag}: loss of example {kp.first_bad(ok)[0]} got "
            f"{loss[kp.first_bad(ok)].item()} want "
            f"{rl[kp.first_bad(ok)].item()}")
        if reg is None:
            continue
        a, r = tp.DP_GRAD_TOL
        for name, got, ref, al in (("grad_subs", gs, rs, allow[1]),
                                   ("grad_ins", gi, ri, allow[2])):
            ok = (got.double() - ref).abs() <= al * (a + r * ref.abs())
            assert ok.all(), (
                f"{tag}: {name} {_dp_first_cell(ok)} got "
                f"{got[kp.first_bad(ok)].item()} want "
                f"{ref[kp.first_bad(ok)].item()}")


def test_alignment_dp_measured_summary():
    """Prints the kernel's largest err_norm per (reg, kind) over the shapes
    run above (the figures recorded in train_probes.DP_KERNEL_MEASURED)."""
    for key in sorted(DP_MEASURED, key=str):
        print(f"DP kernel measured {key}: "
              + ", ".join(f"{e:.3e}" for e in DP_MEASURED[key]))


@pytest.mark.parametrize("m,n", tp.DP_SHAPES)
@pytest.mark.parametrize("width", [None, 1, 4])
def test_alignment_dp_hard_grid_loss_exact(ext, m, n, width):
    """Hard min on k/8-grid costs: every V is exact in fp32, so the loss
    equals the float64 DP."""
    for del_cost in tp.DP_DEL_COSTS:
        seq_lens = tp.dp_seq_lens(m, 40 + m + n)
        subs, ins = tp.dp_grid_costs(m, n, 41 + m + n)
        want, _, _, _ = tp.dp_hard_path(subs, ins, seq_lens, del_cost, width)
        loss, _, _ = _dp_run(ext, subs, ins, seq_lens, del_cost, None, width,
                             torch.ones(tp.DP_B))
        ne = loss.double().numpy() != want
        assert not ne.any(), (
            f"alignment_dp hard m={m} n={n} width={width} del={del_cost}: "
            f"example {int(ne.nonzero()[0][0])} (seq_len "
            f"{int(seq_lens[int(ne.nonzero()[0][0])])}) got "
            f"{loss[ne][0].item()} want {want[ne][0]}")


@pytest.mark.parametrize("m,n,width,del_cost,kind,seed",
                         tp.DP_HARD_GRAD_CASES)
def test_alignment_dp_hard_gradients(ext, m, n, width, del_cost, kind, seed):
    """Where the float64 optimal path is unique by >= 1e-3 at every cell,
    the gradients are the 0/1 path indicators and insertion counts times
    grad_out, exactly."""
    seq_lens = tp.dp_seq_lens(m, seed)
    subs, ins = tp.dp_costs(m, n, kind, seed, seq_lens)
    want, path, nins, gap = tp.dp_hard_path(subs, ins, seq_lens, del_cost,
                                            width)
    assert gap >= tp.DP_HARD_GAP, gap
    go = tp.dp_grad_out(seed + 1)
    loss, gs, gi = _dp_run(ext, subs, ins, seq_lens, del_cost, None, width,
                           go)
    tag = f"alignment_dp hard grads m={m} n={n} width={width}"
    torch.testing.assert_close(loss.double(), torch.from_numpy(want),
                               atol=1e-3, rtol=1e-4)
    want_s = torch.from_numpy(path) * go.double()[:, None, None]
    want_i = torch.from_numpy(nins) * go.double()[:, None]
    ok = gs.double() == want_s
    assert ok.all(), f"{tag}: grad_subs {_dp_first_cell(ok)}"
    ok = gi.double() == want_i
    assert ok.all(), f"{tag}: grad_ins {_dp_first_cell(ok)}"


def test_alignment_dp_rejects_long_label(ext):
    subs = torch.zeros(1, 159, 5, device="cuda")
    ins = torch.zeros(1, 5, device="cuda")
    sl = torch.ones(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="window too long"):
        ext.alignment_dp_fwd(subs, ins, sl, 1.0, 0.1, 0)
    ext.alignment_dp_fwd(subs[:, :158], ins, sl, 1.0, 0.1, 0)
