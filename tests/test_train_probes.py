"""CPU validation of tests/train_probes.py: the premises the GPU probes in
test_gpu_train_exact.py rest on, shown without a GPU.

 * the hash twins are deterministic, keep the right share and depend on the
   seed;
 * every exact-grid builder stays exact: float32 arithmetic in a permuted
   order equals the float64 reference bitwise, and the caps that make atomic
   or tree sums order-independent hold on the reference alone;
 * the direct float64 DP agrees with AlignmentLoss.alignment and with the
   hand-computed loss cases;
 * the recorded float32 DP baseline is what the CPU path gives today, and the
   hard-min gradient cases have a unique optimal path.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_probes as kp  # noqa: E402
import train_probes as tp  # noqa: E402


# ---- 1. hash twins -----------------------------------------------------------

def test_seed_truncation():
    assert [int(tp.seed32(s)) for s in tp.SEEDS] == [
        0, 1, 2 ** 31 - 2, 5, 2 ** 32 - 1]


@pytest.mark.parametrize("seed", tp.SEEDS)
def test_twins_deterministic_and_seeded(seed):
    N = 1 << 20
    a, b = tp.rd_rand01(seed, np.arange(N)), tp.rd_rand01(seed, np.arange(N))
    assert a.dtype == np.float32 and np.array_equal(a, b)
    assert a.min() >= 0.0 and a.max() < 1.0
    # (z >> 8) * 2^-24 is exact: every value is a multiple of 2^-24.
    assert np.array_equal(a.astype(np.float64) * 2 ** 24 % 1, np.zeros(N))
    f = tp.rand01(seed, np.arange(512)[:, None], np.arange(2048)[None, :])
    assert np.array_equal(
        f, tp.rand01(seed, np.arange(512)[:, None], np.arange(2048)[None, :]))
    for p in (0.1, 0.5, 0.75):
        sd = 4 * math.sqrt(p * (1 - p) / N)
        for r in (a, f):
            share = tp.keep_of(r, p).mean()
            assert abs(share - (1 - p)) <= sd, (seed, p, share)
        assert (tp.rd_keep(seed, N, p) != tp.rd_keep(seed + 1, N, p)).any()
        assert (tp.ffn_keep(seed, 64, p) != tp.ffn_keep(seed + 1, 64, p)).any()
    assert tp.keep_of(a, 0.0).all()


def test_ffn_mask_is_a_function_of_row_and_hidden():
    k = tp.ffn_keep(5, 513, 0.5)
    assert (k[256:512] != k[:256]).any()          # not keyed by the tile row
    assert (k[0] != k[1]).any()                   # not of the hidden idx only
    assert (k[:, 0] != k[:, 1]).any()
    # Scalar evaluation of the same formula at one point.
    z = (5 + 300 * 0x9E3779B9 + 77 * 0x85EBCA6B) & 0xFFFFFFFF
    z ^= z >> 16
    z = z * 0x7FEB352D & 0xFFFFFFFF
    z ^= z >> 15
    z = z * 0x846CA68B & 0xFFFFFFFF
    z ^= z >> 16
    assert float(tp.rand01(5, 300, 77)[0]) == (z >> 8) / 2 ** 24


def test_inv_keep_dyadic():
    assert [float(tp.inv_keep32(p)) for p in (0.0, 0.5, 0.75)] == [1, 2, 4]
    assert float(tp.inv_keep32(0.1)) != 1 / 0.9   # float32 value, not float64


# ---- 2./3. ffn_train ---------------------------------------------------------

@pytest.mark.parametrize("p", tp.FFN_PS_EXACT)
def test_ffn_fwd_probe_exact_in_any_order(p):
    M = 33
    x, w1, b1, w2, b2 = kp.ffn_probe(M, tp.FFN_WEIGHT_SEED)
    hd, y64, terms, keep = tp.ffn_fwd_ref(x, w1, b1, w2, b2, p, 7)
    assert float(terms.max()) < 2 ** 17
    assert torch.equal(y64 * 4, (y64 * 4).round())
    perm = torch.randperm(2048, generator=torch.Generator().manual_seed(1))
    y32 = hd.float()[:, perm] @ w2.float()[:, perm].t() + b2.float()
    assert torch.equal(y32.double(), y64)
    # Dropped and relu-dead units are +0, never -0.
    assert (hd.view(torch.int16)[hd.float() == 0] == 0).all()
    assert ((hd.float() > 0) <= keep).all()
    assert 0.2 < (hd.float() > 0).float().mean() / (1 - p) < 0.6


def test_ffn_fwd_general_p_is_one_rounding():
    x, w1, b1, w2, b2 = kp.ffn_probe(5, tp.FFN_WEIGHT_SEED)
    hd, y64, terms, keep = tp.ffn_fwd_ref(x, w1, b1, w2, b2, 0.1, 3)
    h = torch.relu(x @ w1.t() + b1)
    want = (h.float() * torch.tensor(float(tp.inv_keep32(0.1)))).to(kp.BF16)
    assert torch.equal(hd[keep], want[keep])
    assert (tp.y_bound(y64, terms) > 0).all()


def test_dgrad_probe_exact_and_rows_distinct():
    M = 513
    hd = tp.dgrad_hd(M)
    assert len({bytes(r.view(torch.int16).numpy()) for r in hd}) == M
    bits = hd.view(torch.int16)
    assert (bits == 0).any() and (bits == -32768).any()       # +0 and -0.0
    assert (hd.float() > 0).any() and (hd.float() < 0).any()
    _, w1, _, w2, _ = kp.ffn_probe(1, tp.FFN_WEIGHT_SEED)
    s_img, d_img = tp.dgrad_images(w1, w2)
    assert s_img.shape == (2048, 296) and d_img.shape == (320, 2048)
    dy = kp.grid_tensor((33, 280), 1 / 4, 8, 9)
    for p in tp.FFN_PS_EXACT:
        dh, dx64, terms = tp.ffn_dgrad_ref(dy, hd[:33], w1, w2, p)
        assert float((dy @ w1.t()).abs().max()) <= 8
        assert float(terms.max()) < 2 ** 17
        perm = torch.randperm(2048, generator=torch.Generator().manual_seed(2))
        dx32 = dh.float()[:, perm] @ w2.float()[:, perm].t()
        assert torch.equal(dx32.double(), dx64)
        assert (dh.view(torch.int16)[hd[:33].float() <= 0] == 0).all()


def test_ffn_e2e_probe_exact():
    x, w1, b1, w2, b2, dy = tp.ffn_e2e_probe(257, 400)
    ref = tp.ffn_e2e_ref(x, w1, b1, w2, b2, dy, 0.5, tp.SEEDS[3])
    dhd = dy @ w2
    assert torch.equal(dhd.to(kp.BF16).double(), dhd)
    for k in ("y", "dx"):
        assert torch.equal(ref[k].float().double(), ref[k])
        assert float(ref[k].abs().max()) < 2 ** 17
    assert all(float(ref[k].abs().max()) > 0 for k in ref)


# ---- 4. resid_drop -----------------------------------------------------------

@pytest.mark.parametrize("numel,kmax",
                         [(n, 16) for n in tp.RD_NUMELS]
                         + [(8 * tp.RD_N8_STRIDE, 1)])
def test_resid_drop_inputs_stay_exact(numel, kmax):
    x, y, dout = tp.rd_inputs(numel, 500 + numel % 1000, kmax)
    for alpha in tp.RD_ALPHAS_EXACT:
        assert float(np.float32(alpha)) == alpha
        for p in tp.RD_PS_EXACT:
            out, dy, terms = tp.rd_ref(x, y, dout, alpha, p, tp.SEEDS[3])
            assert float(terms.abs().sum()) < tp.RD_DALPHA_CAP
            assert torch.equal(terms * 64, (terms * 64).round())
            # float32 with separate roundings equals float64: every product
            # and the sum are exact, so FMA contraction cannot matter.
            a32 = torch.tensor(alpha, dtype=torch.float32)
            ik = torch.tensor(float(tp.inv_keep32(p)) if p else 1.0)
            keep = torch.from_numpy(tp.rd_keep(tp.SEEDS[3], numel, p))
            o32 = x.float() + a32 * (keep.float() * y.float() * ik)
            d32 = a32 * dout.float() * ik * keep.float()
            assert torch.equal(o32.double(), out)
            assert torch.equal(d32.double(), dy)
            assert (dy.to(kp.BF16).view(torch.int16)[~keep] == 0).all()
            if numel > 10 ** 6:
                break
    assert tp.rd_part_len(numel) == min(4096, -(-(numel // 8) // 256))


def test_resid_drop_part_lengths():
    assert [tp.rd_part_len(n) for n in tp.RD_NUMELS] == [1, 1, 8, 4]
    assert tp.rd_part_len(8 * tp.RD_N8_STRIDE) == 4096


# ---- 5. embed_grad -----------------------------------------------------------

def test_embed_meta_probe_layout():
    meta = tp.EmbedMetaProbe()
    assert meta.R == 5 and meta.C == 30
    assert meta.row_tbase[0] == meta.row_tbase[1]             # aliased table
    assert meta.row_vocab[0] != meta.row_vocab[1]
    assert sorted(set(meta.row_width)) == [2, 4, 8]
    assert meta.row_shift.count(1) == 1
    assert meta.tbl_elems == sum(
        v * w for v, w in zip(meta.table_vocab, meta.table_width))
    assert meta.tbl_elems <= tp.EG_MAX_TBL
    for r in range(meta.R):                # a row's clamp stays in its table
        assert meta.row_vocab[r] <= meta.table_vocab[meta.row_table[r]]
    assert all(s >= 1 and math.log2(s) % 1 == 0 for s in meta.scale_exact)


@pytest.mark.parametrize("B,L", tp.EG_POSITIONS)
def test_embed_grad_reference_exact_and_covers_edges(B, L):
    meta = tp.EmbedMetaProbe()
    rows = tp.eg_rows(B, L, 900 + B * L % 1000)
    go = kp.grid_tensor((B, L, meta.C), 1 / 8, 16, 901 + B * L % 1000)
    prefill = kp.grid_tensor((meta.tbl_elems,), 1 / 8, 16, 902)
    ref, mag = tp.eg_ref(rows, go, meta.scale_exact, prefill, meta.tbl_elems)
    assert float(mag.max()) < tp.EG_EXACT_CAP
    assert torch.equal(ref * 8, (ref * 8).round())
    assert torch.equal(ref.float().double(), ref)
    # Row 0 of every table (id 0) receives nothing: the prefill survives.
    for base, w in zip(sorted(set(meta.row_tbase)), meta.table_width):
        assert torch.equal(ref[base:base + w], prefill[base:base + w])
    if B * L >= 32:
        ids = rows.long()
        for r in range(meta.R):
            sh = ids[:, r] + meta.row_shift[r]
            assert (sh == 0).any() and (sh < 0).any()
            assert (sh >= meta.row_vocab[r]).any()
        assert (ref != prefill).any()


# ---- 6. alignment DP ----------------------------------------------------------

def test_dp_ref_matches_hand_computed_cases():
    from test_losses import ALIGNMENT_LOSS_CASES, convert_seqs
    from deepconsensus_amd.models import losses as L

    for name, seqs, del_cost, reg, width, expected in ALIGNMENT_LOSS_CASES:
        y_true, y_pred = convert_seqs(seqs)
        oh, seq_lens = L.AlignmentLoss.preprocess_y_true(y_true)
        pred = L.AlignmentLoss.preprocess_y_pred(y_pred)
        subs = L.xentropy_subs_cost_fn(oh, pred)
        ins = L.xentropy_ins_cost_fn(pred)
        loss, _, _ = tp.dp_ref64(subs, ins, seq_lens, del_cost, reg, width)
        assert abs(float(loss.mean()) - expected) < 0.01, (name, loss)


@pytest.mark.parametrize("m,n", [s for s in tp.DP_SHAPES if s[0] <= 12])
def test_dp_ref_matches_cpu_path_float64(m, n):
    """The direct DP against AlignmentLoss.alignment run in float64, loss and
    both gradients at 1e-5, on every combo; k_end <= 1 examples left out
    (the wavefront path returns 1e9 there, the direct DP V[0][1])."""
    for c in tp.dp_shape_cases(m, n):
        got = tp.dp_cpu_path(c["subs"], c["ins"], c["seq_lens"],
                             c["del_cost"], c["reg"], c["width"],
                             c["grad_out"], dtype=torch.float64)
        keep = ~tp.dp_divergent(c["seq_lens"], n, c["width"])
        for g, r in zip(got, c["ref"]):
            torch.testing.assert_close(g[keep], r[keep], atol=1e-5, rtol=1e-5)
        div = ~keep
        assert (got[0][div] == 1e9).all()
        assert torch.equal(c["ref"][0][div], c["ins"][div, 0].double())
        un = tp.dp_unreachable(c["seq_lens"], n, c["width"])
        assert (c["ref"][0][un] == 1e9).all()
        assert (c["ref"][1][un] == 0).all() and (c["ref"][2][un] == 0).all()


def test_dp_cases_cover_the_edges():
    for m, n in tp.DP_SHAPES:
        combos = tp.dp_combos(m, n)
        assert {(c[0], c[1]) for c in combos} == {
            (w, r) for w in tp.dp_widths(m, n) for r in tp.DP_REGS}
        for reg in tp.DP_REGS:
            mine = [c for c in combos if c[1] == reg]
            assert {c[3] for c in mine} == set(tp.DP_KINDS)
            assert {c[2] for c in mine} == set(tp.DP_DEL_COSTS)
        sl = tp.dp_seq_lens(m, 3).tolist()
        assert sl[:3] == [0, 1, m]
    un = [tp.dp_unreachable(tp.dp_seq_lens(m, 0), n, 1).any()
          for m, n in tp.DP_SHAPES]
    assert any(un)
    subs, ins = tp.dp_costs(12, 7, "onehot", 1)
    assert float(subs.min()) < 2e-3 and float(subs.max()) > 16
    assert 1e-3 < float(ins.min()) and float(ins.max()) > 16


def test_dp_grid_costs_exact_in_float32():
    m, n = 158, 158
    subs, ins = tp.dp_grid_costs(m, n, 41 + m + n)
    assert torch.equal(subs * 8, (subs * 8).round())
    # Largest conceivable V: (m + n) steps of cost <= 10 on the 1/8 grid.
    assert (m + n) * 10 * 8 < 2 ** 24


@pytest.mark.parametrize("m,n,width,del_cost,kind,seed",
                         tp.DP_HARD_GRAD_CASES)
def test_dp_hard_gradient_cases_have_unique_paths(m, n, width, del_cost,
                                                  kind, seed):
    seq_lens = tp.dp_seq_lens(m, seed)
    subs, ins = tp.dp_costs(m, n, kind, seed, seq_lens)
    loss, path, nins, gap = tp.dp_hard_path(subs, ins, seq_lens, del_cost,
                                            width)
    assert gap >= tp.DP_HARD_GAP, gap
    if m * n <= 129 * 40:
        rl, rs, ri = tp.dp_ref64(subs, ins, seq_lens, del_cost, None, width)
        np.testing.assert_allclose(rl.numpy(), loss, rtol=1e-12)
        assert np.array_equal(rs.numpy(), path)
        assert np.array_equal(ri.numpy(), nins)


def measure_dp_baseline():
    """err_norm of the float32 CPU wavefront path against dp_ref64, per
    (reg, kind) -> (loss, grad_subs, grad_ins)."""
    out = {}
    for m, n in tp.DP_SHAPES:
        for c in tp.dp_shape_cases(m, n):
            if c["reg"] is None:
                continue
            got = tp.dp_cpu_path(c["subs"], c["ins"], c["seq_lens"],
                                 c["del_cost"], c["reg"], c["width"],
                                 c["grad_out"])
            keep = ~tp.dp_divergent(c["seq_lens"], n, c["width"])
            errs = [tp.dp_err_norm(g[keep], r[keep], tol) for g, r, tol in
                    zip(got, c["ref"], (tp.DP_LOSS_TOL, tp.DP_GRAD_TOL,
                                        tp.DP_GRAD_TOL))]
            key = (c["reg"], c["kind"])
            out[key] = tuple(max(a, b) for a, b in
                             zip(out.get(key, (0.0, 0.0, 0.0)), errs))
    return out


def test_dp_baseline_table_is_current():
    """The recorded float32-CPU-path-vs-float64 figures are what the CPU
    path gives today."""
    got = measure_dp_baseline()
    assert set(got) == set(tp.DP_F32_BASELINE)
    for key in sorted(got, key=str):
        print(f"DP baseline {key}: "
              + ", ".join(f"{e:.3e}" for e in got[key]))
        for e, c in zip(got[key], tp.DP_F32_BASELINE[key]):
            assert 0.5 * c <= e <= 2.0 * c, (key, got[key],
                                             tp.DP_F32_BASELINE[key])
