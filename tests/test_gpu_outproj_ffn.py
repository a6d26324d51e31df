"""fused_outproj_ffn vs fused_ffn_v5(fused_linear(out-projection)), bitwise.

The fused kernel multiplies the same (a, Wout) pairs in the same k-step
order as fused_linear (in the swapped MFMA orientation), rounds the
accumulator to bf16 and applies the ReZero residual with the same
arithmetic, then runs v5's chunk loop and epilogue unchanged. Every case
therefore requires torch.equal with the two-kernel pair.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

ALPHA_ATTN = 0.37
ALPHA_FFN = 0.7


@pytest.fixture(scope="module")
def ext():
    from deepconsensus_amd import ops

    return ops.get_ext(required=True)


@pytest.fixture(scope="module")
def weights():
    """Production-shaped out-projection and FFN weights, host layouts."""
    g = torch.Generator().manual_seed(43)
    wout = torch.zeros(320, 296)
    wout[:280, :280] = torch.randn(280, 280, generator=g) * 0.08
    w1 = torch.zeros(2048, 296)
    w1[:, :280] = torch.randn(2048, 280, generator=g) * 0.05
    w1[:, 287] = torch.randn(2048, generator=g) * 0.1  # folded b1
    w2 = torch.zeros(320, 2048)
    w2[:280] = torch.randn(280, 2048, generator=g) * 0.05
    b2 = torch.zeros(320)
    b2[:280] = torch.randn(280, generator=g) * 0.1
    bf = torch.bfloat16
    return (wout.to(bf).cuda(), w1.to(bf).cuda(), w2.to(bf).cuda(), b2.cuda())


def _inputs(M, seed):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(M, 280, generator=g) * 0.5).to(torch.bfloat16).cuda()
    resid = (torch.randn(M, 280, generator=g) * 0.5).to(torch.bfloat16).cuda()
    return a, resid


def _pair(ext, a, resid, weights):
    wout, w1, w2, b2 = weights
    empty = a.new_empty(0)
    flat = ext.fused_linear(a, wout, empty, resid, 280, False, ALPHA_ATTN)
    return flat, ext.fused_ffn_v5(flat, w1, w2, b2, ALPHA_FFN, 0)


def _fused(ext, a, resid, weights, max_blocks):
    wout, w1, w2, b2 = weights
    return ext.fused_outproj_ffn(a, resid, wout, ALPHA_ATTN, w1, w2, b2,
                                 ALPHA_FFN, max_blocks)


def _assert_bitwise(out, ref, what):
    assert out.shape == ref.shape
    ne = out.view(torch.int16) != ref.view(torch.int16)
    if ne.any():
        r, c = (int(v) for v in ne.nonzero()[0])
        raise AssertionError(
            f"{what}: {int(ne.sum())} elements differ, first at row {r} "
            f"col {c}: got {float(out[r, c])}, want {float(ref[r, c])}"
        )


# (M, max_blocks): 0 = default grid (one block per tile here). The
# max_blocks cases put several tiles on one block, which exercises the
# cross-tile Wout/FFN rotation and the epilogue-slice reuse: 1 -> one block
# walks 6 tiles; 2 -> 3 + 3; 4 -> 2, 2, 1, 1; 1024 rows over 3 blocks ->
# one block gets two tiles. 1297 = 5 * 256 + 17 leaves the last tile ragged.
CASES = [
    (1, 0), (31, 0), (33, 0), (255, 0), (256, 0), (257, 0), (513, 0),
    (1297, 1), (1297, 2), (1297, 4),
    (1024, 3),
]


@pytest.mark.parametrize("M,max_blocks", CASES)
def test_fused_bitwise_equals_pair(ext, weights, M, max_blocks):
    a, resid = _inputs(M, 2000 + M)
    flat, ref = _pair(ext, a, resid, weights)
    out = _fused(ext, a, resid, weights, max_blocks)
    torch.cuda.synchronize()
    assert torch.isfinite(ref.float()).all()
    # Neither residual may dominate: both GEMM terms change most elements.
    assert (flat != resid).float().mean().item() > 0.5
    assert (ref != flat).float().mean().item() > 0.5
    _assert_bitwise(out, ref, f"M={M} max_blocks={max_blocks}")


def test_fused_deterministic_across_runs(ext, weights):
    """A rotation race would show up as run-to-run differences."""
    a, resid = _inputs(1297, 78)
    _, ref = _pair(ext, a, resid, weights)
    outs = [_fused(ext, a, resid, weights, 2) for _ in range(5)]
    torch.cuda.synchronize()
    for i, out in enumerate(outs):
        _assert_bitwise(out, outs[0], f"run {i} vs run 0")
    _assert_bitwise(outs[0], ref, "run 0 vs pair")


def test_resid_at_end_of_exact_allocation(ext, weights):
    """resid is the last M rows of an exactly-sized allocation and M is no
    multiple of 32: the result must not depend on what lies beyond row M or
    column 280 (the kernel never reads there)."""
    M, lead = 77, 19
    a, resid = _inputs(M, 79)
    backing = torch.empty((lead + M) * 280, dtype=torch.bfloat16,
                          device="cuda")
    backing[: lead * 280] = 7.0
    tail = backing[lead * 280:].view(M, 280)
    tail.copy_(resid)
    assert tail.is_contiguous() and tail.data_ptr() != backing.data_ptr()
    _, ref = _pair(ext, a, resid, weights)
    out = _fused(ext, a, tail, weights, 0)
    torch.cuda.synchronize()
    _assert_bitwise(out, ref, "resid at end of allocation")


def test_runner_fused_matches_pair(monkeypatch):
    """forward_windows on 8 windows: DC_FUSED_OUTPROJ=1 and =0 give the same
    bases and quals."""
    import numpy as np

    from deepconsensus_amd.models import config as cfg
    from deepconsensus_amd.models.model import get_model
    from deepconsensus_amd.models.runner import InferenceRunner

    params = cfg.get_config("transformer_learn_values+custom")
    cfg.modify_params(params, is_training=False)
    torch.manual_seed(7)
    model = get_model(params)
    rng = np.random.default_rng(3)
    B, R, L, mp = 8, params.total_rows, params.max_length, params.max_passes
    rows = np.zeros((B, R, L), dtype=np.float32)
    rows[:, 0:mp] = rng.integers(0, 5, size=(B, mp, L))
    rows[:, mp:2 * mp] = rng.integers(0, 256, size=(B, mp, L))
    rows[:, 2 * mp:3 * mp] = rng.integers(0, 256, size=(B, mp, L))
    rows[:, 3 * mp:4 * mp] = rng.integers(0, 3, size=(B, mp, L))
    rows[:, 4 * mp] = rng.integers(0, 5, size=(B, L))
    rows[:, -4:] = rng.integers(0, 501, size=(B, 4, 1))
    rows = torch.from_numpy(rows)

    outs = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("DC_FUSED_OUTPROJ", flag)
        runner = InferenceRunner(params, model, device="cuda:0")
        assert runner.native and runner.ffn_fused_ok and runner.ffn_v5
        assert runner.fused_outproj == (flag == "1")
        bases, quals = runner.forward_windows(rows)
        torch.cuda.synchronize()
        outs[flag] = (bases.cpu(), quals.cpu())
    assert torch.equal(outs["1"][0], outs["0"][0])
    assert torch.equal(outs["1"][1], outs["0"][1])
