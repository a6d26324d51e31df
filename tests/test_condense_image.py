"""CPU tests: fused_condense weight image + DC_FUSED_CONDENSE resolution."""
import pytest
import torch

from deepconsensus_amd.models import runner as runner_mod

WIDTHS = (560, 568, 872, 880)
STRIDES = {560: 568, 568: 584, 872: 888, 880: 888}


def test_condense_image_stride_supported_widths():
    for k in WIDTHS:
        assert runner_mod.condense_image_stride(k) == STRIDES[k]


@pytest.mark.parametrize("k", [552, 576, 1000])
def test_condense_image_stride_unsupported_is_none(k):
    assert runner_mod.condense_image_stride(k) is None


def test_condense_image_stride_covers_last_granule():
    """WS >= 16*ceil(K/16): the B-side read of the last granule's upper
    half stays inside the row, and 64 rows are whole KiB units."""
    for k in WIDTHS:
        ws = runner_mod.condense_image_stride(k)
        assert ws >= 16 * -(-k // 16)
        assert (64 * ws * 2) % 1024 == 0
        assert (ws * 2) % 16 == 0


@pytest.mark.parametrize("k", WIDTHS)
def test_build_condense_image(k):
    g = torch.Generator().manual_seed(100 + k)
    w = torch.randn(280, k, generator=g) * 0.05
    # No exact zeros in the live block, so "zero elsewhere" is meaningful.
    w = torch.where(w == 0, torch.full_like(w, 0.01), w)
    img = runner_mod.build_condense_image(w)
    ws = STRIDES[k]
    assert img.shape == (320, ws)
    assert img.dtype == torch.bfloat16
    assert img.is_contiguous()
    assert torch.equal(img[:280, :k], w.to(torch.bfloat16))
    assert not img[:280, k:].any()
    assert not img[280:].any()
    assert int((img != 0).sum()) == 280 * k


def test_build_condense_image_rejects_unsupported_width():
    with pytest.raises(ValueError):
        runner_mod.build_condense_image(torch.zeros(280, 576))


def test_fused_condense_env_resolution():
    en = runner_mod.fused_condense_enabled
    # unset or "1": today's behaviour, fused at 560 only.
    for value in (None, "1"):
        assert en(560, value) is True
        for k in (568, 872, 880, 552, 576, 1000):
            assert en(k, value) is False
    # "0": never fused.
    for k in WIDTHS + (552,):
        assert en(k, "0") is False
    # "wide": fused at every supported width, nowhere else.
    for k in WIDTHS:
        assert en(k, "wide") is True
    for k in (552, 576, 1000):
        assert en(k, "wide") is False
