"""GPU tests: fused_condense at the ccs_bq and 32-pass widths (568/872/880).

Bound used throughout: |out - ref| <= 2**-8 * |ref| + 1e-3 against an fp64
reference built from the bf16-rounded operands (+ the fp32 pos table).
bf16 keeps 8 significant bits, so the output round is at most 2**-9
relative; 2**-8 leaves a factor of two. The absolute term covers fp32
accumulation over at most 880 products of this scale (|x| ~ 0.5,
|w| ~ 0.05: partial sums stay below ~4, fp32 ulp there is 4.8e-7).
"""
import numpy as np
import pytest
import torch

from deepconsensus_amd import ops as dc_ops
from deepconsensus_amd.models import config as cfg
from deepconsensus_amd.models.model import get_model
from deepconsensus_amd.models.runner import (
    InferenceRunner,
    build_condense_image,
)

pytestmark = pytest.mark.gpu

N_OUT = 280  # last 64-column chunk has 24 live columns
NEW_WIDTHS = (568, 872, 880)


@pytest.fixture(scope="module")
def ext():
    return dc_ops.get_ext(required=True)


def _operands(k, m, seed, n=N_OUT):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(m, k, generator=g) * 0.5).to(torch.bfloat16)
    w = torch.randn(n, k, generator=g) * 0.05
    return x, w


def _reference(x_bf, w, pos, seq_len):
    """fp64 from the bf16-rounded operands (CPU tensors)."""
    ref = x_bf.double() @ w.to(torch.bfloat16).double().t()
    if pos is not None:
        idx = torch.arange(x_bf.shape[0]) % seq_len
        ref = ref + pos.double()[idx]
    return ref


def _assert_within_bound(out, ref, what=""):
    err = (out.double().cpu() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-3
    worst = (err - bound).max().item()
    print(f"{what} max err {err.max().item():.3e} "
          f"max(err - bound) {worst:.3e}")
    assert bool((err <= bound).all()), (what, err.max().item(), worst)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("m,seq_len", [(1, 1), (31, 7), (257, 100), (300, 77)])
@pytest.mark.parametrize("k", NEW_WIDTHS)
def test_wide_matches_fp64_reference(ext, k, m, seq_len):
    """Single partial wave / partial 32-row group / one row past a 256 (and
    128) tile / position index wrapping out of step with the tile."""
    x, w = _operands(k, m, seed=1000 * k + m)
    g = torch.Generator().manual_seed(7 * k + m)
    pos = torch.randn(seq_len, N_OUT, generator=g) * 0.3
    img = build_condense_image(w).cuda()
    xd = x.cuda()
    out = ext.fused_condense(xd, img, pos.cuda(), N_OUT, seq_len)
    assert out.shape == (m, N_OUT) and out.dtype == torch.bfloat16
    _assert_within_bound(out, _reference(x, w, pos, seq_len),
                         f"K={k} M={m} L={seq_len} pos")
    empty = torch.empty(0, device="cuda", dtype=torch.float32)
    out2 = ext.fused_condense(xd, img, empty, N_OUT, seq_len)
    _assert_within_bound(out2, _reference(x, w, None, seq_len),
                         f"K={k} M={m} L={seq_len} nopos")


@pytest.mark.parametrize("k_lo,k_hi", [(560, 568), (872, 880)])
def test_zero_extension_is_bitwise_identity(ext, k_lo, k_hi):
    """x extended by 8 zero columns (weight by 8 arbitrary non-zero ones)
    gives the same bits: the extra half granule only adds +0 products to
    the odd accumulator chain."""
    m, seq_len = 300, 77
    x_lo, w_lo = _operands(k_lo, m, seed=k_lo)
    g = torch.Generator().manual_seed(k_hi)
    w_ext = torch.randn(N_OUT, 8, generator=g) * 0.05 + 0.5
    assert bool((w_ext.to(torch.bfloat16) != 0).all())
    x_hi = torch.cat([x_lo, torch.zeros(m, 8, dtype=torch.bfloat16)], 1)
    w_hi = torch.cat([w_lo, w_ext], 1)
    pos = (torch.randn(seq_len, N_OUT, generator=g) * 0.3).cuda()
    out_lo = ext.fused_condense(
        x_lo.cuda(), build_condense_image(w_lo).cuda(), pos, N_OUT, seq_len)
    out_hi = ext.fused_condense(
        x_hi.cuda(), build_condense_image(w_hi).cuda(), pos, N_OUT, seq_len)
    assert torch.equal(_bits(out_lo), _bits(out_hi))
    _assert_within_bound(out_hi, _reference(x_hi, w_hi, pos.cpu(), seq_len),
                         f"K={k_hi} zero-ext")


@pytest.mark.parametrize("k", [568, 872])
def test_half_granule_poison(ext, k):
    """The out-of-row half of the last granule is never loaded.

    x is the first M*K elements of a NaN-filled buffer. Row r = 7 sits in
    the first wave and row r + 1 starts with 8 NaNs; row M - 1 = 32 is the
    second wave's only row and is followed by the buffer's NaN tail. Every
    read stays inside the one live allocation. A kernel that loads elements
    K .. K+7 and trusts the zero weight columns turns rows 7 and 32 into
    NaN (0 x NaN)."""
    m, seq_len, r = 33, 11, 7
    x, w = _operands(k, m, seed=31 * k)
    x[r + 1, :8] = float("nan")
    buf = torch.full((m * k + 4096,), float("nan"), dtype=torch.bfloat16,
                     device="cuda")
    xd = buf[: m * k].view(m, k)
    xd.copy_(x)
    assert bool(torch.isnan(buf[m * k:]).all())
    g = torch.Generator().manual_seed(k)
    pos = torch.randn(seq_len, N_OUT, generator=g) * 0.3
    out = ext.fused_condense(
        xd, build_condense_image(w).cuda(), pos.cuda(), N_OUT, seq_len
    ).cpu()
    assert bool(torch.isnan(out[r + 1]).all())
    finite_rows = [i for i in range(m) if i != r + 1]
    assert bool(torch.isfinite(out[r].float()).all())
    assert bool(torch.isfinite(out[m - 1].float()).all())
    assert bool(torch.isfinite(out[finite_rows].float()).all())
    x_ref = x.clone()
    x_ref[r + 1] = 0
    ref = _reference(x_ref, w, pos, seq_len)
    _assert_within_bound(out[finite_rows], ref[finite_rows],
                         f"K={k} poison")


@pytest.mark.parametrize("k", NEW_WIDTHS)
def test_wide_is_deterministic(ext, k):
    m, seq_len = 300, 77
    x, w = _operands(k, m, seed=5 * k)
    g = torch.Generator().manual_seed(k + 1)
    pos = (torch.randn(seq_len, N_OUT, generator=g) * 0.3).cuda()
    xd, img = x.cuda(), build_condense_image(w).cuda()
    a = ext.fused_condense(xd, img, pos, N_OUT, seq_len)
    b = ext.fused_condense(xd, img, pos, N_OUT, seq_len)
    assert torch.equal(_bits(a), _bits(b))


def test_other_widths_still_raise(ext):
    for k in (552, 576):
        x = torch.zeros(4, k, dtype=torch.bfloat16, device="cuda")
        img = torch.zeros(320, 584, dtype=torch.bfloat16, device="cuda")
        empty = torch.empty(0, device="cuda", dtype=torch.float32)
        with pytest.raises(RuntimeError):
            ext.fused_condense(x, img, empty, N_OUT, 1)
    # A supported width with the wrong image stride raises too (568 input
    # must not be paired with the 560 image).
    x = torch.zeros(4, 568, dtype=torch.bfloat16, device="cuda")
    img = torch.zeros(320, 568, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        ext.fused_condense(x, img, empty, N_OUT, 1)


def _make_rows(params, batch, seed):
    rng = np.random.default_rng(seed)
    R, L, mp = params.total_rows, params.max_length, params.max_passes
    rows = np.zeros((batch, R, L), dtype=np.float32)
    rows[:, 0:mp] = rng.integers(0, 5, size=(batch, mp, L))
    rows[:, mp:2 * mp] = rng.integers(0, 256, size=(batch, mp, L))
    rows[:, 2 * mp:3 * mp] = rng.integers(0, 256, size=(batch, mp, L))
    rows[:, 3 * mp:4 * mp] = rng.integers(0, 3, size=(batch, mp, L))
    rows[:, 4 * mp] = rng.integers(0, 5, size=(batch, L))
    if params.use_ccs_bq:
        rows[:, 4 * mp + 1] = rng.integers(-1, 94, size=(batch, L))
    rows[:, -4:] = rng.integers(0, 501, size=(batch, 4, 1))
    return torch.from_numpy(rows)


def _runner_pair(monkeypatch, use_ccs_bq, max_passes, seed):
    """(params, runner with the variable unset, runner with =wide)."""
    params = cfg.get_config("transformer_learn_values+custom")
    params.use_ccs_bq = use_ccs_bq
    params.max_passes = max_passes
    cfg.modify_params(params, is_training=False)
    torch.manual_seed(seed)
    model = get_model(params)
    monkeypatch.delenv("DC_FUSED_CONDENSE", raising=False)
    plain = InferenceRunner(params, model, device="cuda:0")
    monkeypatch.setenv("DC_FUSED_CONDENSE", "wide")
    wide = InferenceRunner(params, model, device="cuda:0")
    assert plain.native and wide.native
    return params, plain, wide


def _assert_runners_agree(plain, wide, rows):
    b1, q1 = wide.forward_windows(rows)
    b2, q2 = plain.forward_windows(rows)
    agree = (b1 == b2).float().mean().item()
    dqv = (q1.float() - q2.float()).abs().mean().item()
    print(f"base agreement {agree:.5f} mean |dQV| {dqv:.4f}")
    assert agree > 0.99
    assert dqv < 1.0
    return b1, q1


def test_runner_wide_bq_model(monkeypatch):
    """DC_FUSED_CONDENSE=wide on a ccs_bq model (86 rows, K = 568)."""
    params, plain, wide = _runner_pair(monkeypatch, True, 20, seed=13)
    assert params.total_rows == 86
    # Default did not move: the bq layout stays on the library fallback.
    assert plain.cond_img is None
    assert wide.cond_img is not None
    assert tuple(wide.cond_img.shape) == (320, 584)
    rows = _make_rows(params, 16, seed=4)
    b_e, q_e = _assert_runners_agree(plain, wide, rows)
    b_e, q_e = b_e.cpu(), q_e.cpu()
    b_g, q_g = wide.forward_windows_graphed(rows.pin_memory())
    assert getattr(wide, "_graph", None) is not None, "capture fell back"
    assert torch.equal(b_g.cpu(), b_e)
    assert torch.equal(q_g.cpu(), q_e)


def test_runner_wide_max_passes_32(monkeypatch):
    """DC_FUSED_CONDENSE=wide at max_passes=32 without bq (133 rows,
    K = 872, the 4-wave instantiation)."""
    params, plain, wide = _runner_pair(monkeypatch, False, 32, seed=17)
    assert params.total_rows == 133
    assert plain.cond_img is None
    assert wide.cond_img is not None
    assert tuple(wide.cond_img.shape) == (320, 888)
    _assert_runners_agree(plain, wide, _make_rows(params, 8, seed=6))
