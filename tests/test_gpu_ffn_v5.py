"""fused_ffn_v5 (persistent-grid FFN) vs fused_ffn_v3, bitwise.

v5 runs v3's chunk loop unchanged — same MFMA order per output, same
`resid + alpha * (oacc + bias)` rounding — so every case requires
torch.equal with v3. Both kernels allocate `out` as exactly [M, 280], and
v3 never touches rows at or beyond M; equality with v3 on all M rows plus
the partial-tile shapes below is the rows-beyond-M check.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ALPHA = 0.7


@pytest.fixture(scope="module")
def ext():
    from deepconsensus_amd import ops

    return ops.get_ext(required=True)


@pytest.fixture(scope="module")
def weights():
    """Production-shaped FFN weights in the kernels' host layouts."""
    g = torch.Generator().manual_seed(41)
    w1 = torch.zeros(2048, 296)
    w1[:, :280] = torch.randn(2048, 280, generator=g) * 0.05
    w1[:, 287] = torch.randn(2048, generator=g) * 0.1  # folded b1
    w2 = torch.zeros(320, 2048)
    w2[:280] = torch.randn(280, 2048, generator=g) * 0.05
    b2 = torch.zeros(320)
    b2[:280] = torch.randn(280, generator=g) * 0.1
    return (w1.to(torch.bfloat16).cuda(), w2.to(torch.bfloat16).cuda(),
            b2.cuda())


def _x(M, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, 280, generator=g) * 0.5).to(torch.bfloat16).cuda()


# (M, max_blocks): 0 = default grid (one block per tile here, all M are
# far below one tile per CU). The max_blocks cases force several tiles
# per block: 1 -> one block walks 6 tiles; 2 -> 3 + 3; 4 -> 2,2,1,1
# (uneven); 256*4 over 3 blocks -> one block gets two tiles.
CASES = [
    (1, 0), (31, 0), (33, 0), (255, 0), (256, 0), (257, 0), (513, 0),
    (256 * 5 + 17, 1), (256 * 5 + 17, 2), (256 * 5 + 17, 4),
    (256 * 4, 3),
]


@pytest.mark.parametrize("M,max_blocks", CASES)
def test_v5_bitwise_equals_v3(ext, weights, M, max_blocks):
    w1, w2, b2 = weights
    x = _x(M, 1000 + M)
    ref = ext.fused_ffn_v3(x, w1, w2, b2, ALPHA)
    out = ext.fused_ffn_v5(x, w1, w2, b2, ALPHA, max_blocks)
    torch.cuda.synchronize()
    assert out.shape == ref.shape
    assert torch.isfinite(ref.float()).all()
    # The residual must not dominate: the FFN term changes most elements.
    assert (ref != x).float().mean().item() > 0.5
    ne = out.view(torch.int16) != ref.view(torch.int16)
    assert not ne.any(), (
        f"M={M} max_blocks={max_blocks}: {int(ne.sum())} elements differ, "
        f"first bad row {int(ne.any(dim=1).nonzero()[0])}"
    )


def test_ablate_mode0_bitwise_equals_v3(ext, weights):
    """ffn_ablate mode 0 is v3's sequencing of the shared tile core."""
    w1, w2, b2 = weights
    x = _x(257, 1257)
    ref = ext.fused_ffn_v3(x, w1, w2, b2, ALPHA)
    out = ext.ffn_ablate(x, w1, w2, b2, ALPHA, 0)
    torch.cuda.synchronize()
    assert out.shape == ref.shape
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))


def test_v5_deterministic_across_runs(ext, weights):
    """Races in this kernel family showed up as schedule-dependent NaNs."""
    w1, w2, b2 = weights
    M = 256 * 5 + 17
    x = _x(M, 77)
    first = ext.fused_ffn_v5(x, w1, w2, b2, ALPHA, 2)
    for _ in range(4):
        again = ext.fused_ffn_v5(x, w1, w2, b2, ALPHA, 2)
        assert torch.equal(again.view(torch.int16), first.view(torch.int16))


def test_runner_v5_matches_v3(monkeypatch):
    """forward_windows on 8 windows: DC_FFN_V5=1 and =0 give the same
    bases and quals."""
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
        monkeypatch.setenv("DC_FFN_V5", flag)
        runner = InferenceRunner(params, model, device="cuda:0")
        assert runner.native and runner.ffn_fused_ok
        assert runner.ffn_v5 == (flag == "1")
        bases, quals = runner.forward_windows(rows)
        torch.cuda.synchronize()
        outs[flag] = (bases.cpu(), quals.cpu())
    assert torch.equal(outs["1"][0], outs["0"][0])
    assert torch.equal(outs["1"][1], outs["0"][1])
