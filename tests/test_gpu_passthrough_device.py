"""GPU tests for the device CCS passthrough: the passthrough_fill kernel
against its numpy twin (bit-exact, guarded and unaligned output rows), the
runner path against host-mode passthrough, and `run` with passthrough_mode
device against host on the same runner."""
import dataclasses

import numpy as np
import pytest
import torch

from deepconsensus_amd.preprocess import featurize_device as fd

from test_io_and_pipeline import make_test_bams
from test_passthrough_device import DEVICE, _plan_zmw

pytestmark = pytest.mark.gpu

_GUARD = 64
_WIDTHS = (1, 100, 333)  # W of the three ZMWs
_WG_BYTES = 1024  # output bytes of one workgroup: 256 lanes x 4


@pytest.fixture(scope="module")
def ext():
    from deepconsensus_amd import ops

    return ops.get_ext(required=True)


@pytest.fixture(scope="module")
def planes():
    """ccs, ccs_q, zmw_tab, qual_lut of three packed ZMWs, W = 1, 100, 333,
    with zmw_tab as wide as pack_batch makes it."""
    rng = np.random.default_rng(5)
    total = sum(_WIDTHS)
    zmw_tab = np.zeros((3, fd.TAB_FIXED + 20 + 4), np.int64)
    zmw_tab[:, fd.TAB_CCS_OFF] = np.cumsum(_WIDTHS) - _WIDTHS
    zmw_tab[:, fd.TAB_W] = _WIDTHS
    lut = rng.integers(0, 94, 256).astype(np.uint8)
    lut[0] = 7  # the padding quality is its own value
    return (rng.integers(1, 5, total).astype(np.uint8),
            rng.integers(0, 256, total).astype(np.uint8), zmw_tab, lut)


def _table(P, L):
    """P valid entries cycling over the ZMWs, over w in {1, 3, 99, 100}
    (as far as the ZMW and L allow), overflow widths 101 and 137, odd
    starts and windows ending exactly at W; a zmw_index -1 entry in the
    middle and, for larger tables, every 13th."""
    tab = np.zeros((P, 5), np.int64)
    for i in range(P):
        zi = i % 3
        W = _WIDTHS[zi]
        overflow = zi == 2 and i % 4 == 1
        if overflow:
            width = (101, 137)[(i // 4) % 2]
            w = min(W, width - (i // 8) % 2 * 30)  # full, or clipped at W
        else:
            width = L
            w = min((1, 3, 99, 100)[(i // 3) % 4], L, W)
        start = (1, W - w, min(7, W - w))[(i // 12) % 3]
        tab[i] = (zi, min(start, W - w), w, width, 0)
    if P >= 3:
        tab[P // 2, 0] = -1
        tab[12::13, 0] = -1
    tab[:, fd.PT_DST] = np.cumsum(tab[:, fd.PT_WIDTH]) - tab[:, fd.PT_WIDTH]
    # Every live entry is one pack_batch would accept.
    live = tab[tab[:, 0] >= 0].copy()
    live[:, fd.PT_DST] = (
        np.cumsum(live[:, fd.PT_WIDTH]) - live[:, fd.PT_WIDTH])
    fd.validate_passthrough_table(live, _WIDTHS)
    return tab.astype(np.int32)


def _rows(base, n):
    """A [2, base + n + _GUARD] stitch buffer of 0xA5 bytes behind _GUARD
    leading bytes, on the host; the passthrough region is [base, base + n)
    of both rows and row 1 starts wherever row 0 ends."""
    row = base + n + _GUARD
    return np.full(_GUARD + 2 * row, 0xA5, np.uint8), row


def _fill_both(ext, planes, tab, base):
    """(device result, twin result) as whole flat buffers, guards
    included."""
    ccs, ccs_q, zmw_tab, lut = planes
    n = int(tab[:, fd.PT_WIDTH].sum()) if len(tab) else 0
    flat, row = _rows(base, n)
    want = flat.copy()
    acc = want[_GUARD:].reshape(2, row)
    fd.passthrough_fill_numpy(ccs, ccs_q, zmw_tab, tab, lut,
                              acc[0, base : base + n],
                              acc[1, base : base + n])
    dev_flat = torch.from_numpy(flat).cuda()
    dev_acc = dev_flat[_GUARD:].view(2, row)
    dev = [torch.from_numpy(a).cuda() for a in (ccs, ccs_q, zmw_tab, tab)]
    args = (*dev, torch.from_numpy(lut).cuda(),
            dev_acc[0, base : base + n], dev_acc[1, base : base + n])
    ext.passthrough_fill_into(*args)
    torch.cuda.synchronize()
    return dev_flat, want, args, n


# P around one and two workgroups' worth of output bytes, at both L.
_P = {100: (0, 1, 2, 9, 10, 11, 20, 21, 40),
      7: (0, 1, 5, 60, 64, 68, 124, 130, 300)}


@pytest.mark.parametrize("base", [0, 100, 7])
@pytest.mark.parametrize("L", [100, 7])
def test_kernel_matches_numpy_twin(ext, planes, L, base):
    sizes = []
    for P in _P[L]:
        tab = _table(P, L)
        got, want, _, n = _fill_both(ext, planes, tab, base)
        got = got.cpu().numpy()
        row = base + n + _GUARD
        # Guards: before row 0, between the regions, after row 1.
        assert (got[:_GUARD + base] == 0xA5).all(), P
        assert (got[_GUARD + base + n : _GUARD + row + base] == 0xA5).all()
        assert (got[_GUARD + row + base + n :] == 0xA5).all(), P
        assert np.array_equal(got, want), P
        if P:
            region = got[_GUARD + base : _GUARD + base + n]
            assert region.any() and not (region == 0xA5).all()
        sizes.append(n)
    assert min(s for s in sizes if s) < _WG_BYTES
    assert any(_WG_BYTES - 100 <= s <= _WG_BYTES + 100 for s in sizes)
    assert any(s > 2 * _WG_BYTES for s in sizes)


def test_table_covers_the_listed_shapes():
    tab = _table(40, 100)
    live = tab[tab[:, 0] >= 0]
    assert {1, 3, 99, 100} <= set(live[:, fd.PT_W].tolist())
    assert {100, 101, 137} == set(tab[:, fd.PT_WIDTH].tolist())
    assert (tab[:, 0] == -1).sum() >= 2 and {0, 1, 2} <= set(live[:, 0])
    assert (live[:, fd.PT_START] % 2 == 1).any()
    assert (live[:, fd.PT_W] < live[:, fd.PT_WIDTH]).any()
    ends = live[:, fd.PT_START] + live[:, fd.PT_W]
    assert (ends == np.array(_WIDTHS)[live[:, 0]]).any()
    assert set(_table(300, 7)[:, fd.PT_WIDTH].tolist()) == {7, 101, 137}


def test_kernel_is_deterministic(ext, planes):
    tab = _table(21, 100)
    flat, want, args, _ = _fill_both(ext, planes, tab, 7)
    first = flat.clone()
    flat.fill_(0xA5)  # the output views in args alias it
    ext.passthrough_fill_into(*args)
    torch.cuda.synchronize()
    assert torch.equal(first, flat)
    assert np.array_equal(first.cpu().numpy(), want)


def test_kernel_rejects_bad_arguments(ext, planes):
    tab = _table(5, 100)
    _, _, args, n = _fill_both(ext, planes, tab, 0)
    ccs, ccs_q, zmw_tab, pt_tab, lut, bases, quals = args
    with pytest.raises(RuntimeError, match="ccs"):
        ext.passthrough_fill_into(ccs.int(), ccs_q, zmw_tab, pt_tab, lut,
                                  bases, quals)
    with pytest.raises(RuntimeError, match="zmw_tab"):
        ext.passthrough_fill_into(ccs, ccs_q, zmw_tab.int(), pt_tab, lut,
                                  bases, quals)
    with pytest.raises(RuntimeError, match="pt_tab"):
        ext.passthrough_fill_into(ccs, ccs_q, zmw_tab,
                                  pt_tab[:, :4].contiguous(), lut, bases,
                                  quals)
    with pytest.raises(RuntimeError, match="pt_tab"):
        ext.passthrough_fill_into(ccs, ccs_q, zmw_tab, pt_tab.long(), lut,
                                  bases, quals)
    with pytest.raises(RuntimeError, match="qual_lut"):
        ext.passthrough_fill_into(ccs, ccs_q, zmw_tab, pt_tab, lut[:255],
                                  bases, quals)
    with pytest.raises(RuntimeError, match="equal length"):
        ext.passthrough_fill_into(ccs, ccs_q, zmw_tab, pt_tab, lut, bases,
                                  quals[:-1])
    with pytest.raises(RuntimeError, match="device"):
        ext.passthrough_fill_into(ccs.cpu(), ccs_q, zmw_tab, pt_tab, lut,
                                  bases, quals)


@pytest.fixture(scope="module")
def runner():
    from deepconsensus_amd.models import config as cfg
    from deepconsensus_amd.models.model import get_model
    from deepconsensus_amd.models.runner import InferenceRunner

    params = cfg.get_config("transformer_learn_values+custom")
    cfg.modify_params(params, is_training=False)
    torch.manual_seed(11)
    r = InferenceRunner(params, get_model(params), device="cuda")
    assert r.native
    return r


def _same_stitched(a, b):
    assert (a.n_model, a.n_skipped) == (b.n_model, b.n_skipped)
    assert a.plan.read_names == b.plan.read_names
    assert np.array_equal(a.plan.read_empty, b.plan.read_empty)
    for name in ("seq_out", "qual_out", "out_off"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_runner_path_matches_host_passthrough(runner, monkeypatch):
    """A mixed batch (table passthrough, object passthrough of a fallback
    ZMW, model windows; 9 model windows at batch_size 5) and a batch of
    passthrough windows only equal the host-mode result."""
    from deepconsensus_amd.inference import quick_inference as qi

    monkeypatch.delenv("DC_SERVE_GRAPH", raising=False)
    options = qi.InferenceOptions(
        batch_size=5, min_quality=0, skip_windows_above=30, **DEVICE)
    spec = [
        ("m0/50/ccs", dict(seed=1, skip_windows=(0, 2))),
        ("m0/9/ccs", dict(seed=2, skip_windows=(0, 1, 2))),
        ("m0/30/ccs", dict(seed=3, skip_windows=(1,), irregular=True)),
        ("m0/40/ccs", dict(seed=5)),
        ("m0/20/ccs", dict(seed=6, skip_windows=(1,))),
    ]
    zmws = {
        mode: [_plan_zmw(monkeypatch, name, mode, **kw) for name, kw in spec]
        for mode in ("host", "device")
    }
    assert [fd.n_table_passthrough(z) for z in zmws["device"]] == [
        2, 3, 0, 0, 1]
    assert sum(len(z.skipped) for z in zmws["device"]) == 1
    want = qi.run_model_and_stitch_on_zmws(zmws["host"], runner, options)
    got = qi.run_model_and_stitch_on_zmws(zmws["device"], runner, options)
    assert got.n_model == 8 and got.n_skipped == 7
    assert got.plan.n_table_bytes == 600 and want.plan.n_table_bytes == 0
    assert len(got.seq_out) > 600
    _same_stitched(got, want)

    only = {
        mode: [zmws[mode][1],
               _plan_zmw(monkeypatch, "m0/8/ccs", mode, seed=7,
                         skip_windows=(0, 1, 2))]
        for mode in ("host", "device")
    }
    want = qi.run_model_and_stitch_on_zmws(only["host"], runner, options)
    got = qi.run_model_and_stitch_on_zmws(only["device"], runner, options)
    assert got.n_model == 0 and got.n_skipped == 6
    assert got.plan.n_table_bytes == 600 and len(got.seq_out) > 0
    _same_stitched(got, want)


def test_run_device_passthrough_matches_host_on_gpu(tmp_path, monkeypatch):
    from deepconsensus_amd.inference import quick_inference as qi

    sub, ccs = make_test_bams(tmp_path, n_zmws=4, length=350, seed=3)
    tables = []
    real = qi.run_model_and_stitch_on_zmws

    def spy(zmws, runner, options):
        out = real(zmws, runner, options)
        tables.append((out.plan.n_table_bytes, out.n_model))
        return out

    monkeypatch.setattr(qi, "run_model_and_stitch_on_zmws", spy)
    outs, counters = {}, {}
    for mode in ("host", "device"):
        torch.manual_seed(7)
        out = tmp_path / f"out_{mode}.fastq"
        options = qi.InferenceOptions(
            batch_size=4, batch_zmws=3, cpus=0, min_quality=0,
            skip_windows_above=27, passthrough_mode=mode, **DEVICE,
        )
        counters[mode] = dataclasses.asdict(qi.run(
            subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
            output=str(out), options=options, device="cuda",
        ))
        outs[mode] = out.read_bytes()
    host, device = tables[: len(tables) // 2], tables[len(tables) // 2 :]
    assert all(t == 0 for t, _ in host) and sum(t for t, _ in device) > 0
    assert sum(m for _, m in device) == sum(m for _, m in host) > 0
    assert counters["host"]["success"] == 4
    assert counters["host"] == counters["device"]
    assert outs["host"] and outs["host"] == outs["device"]
