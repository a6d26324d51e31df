"""GPU tests for device-side subread spacing: the subread_space kernel
against its numpy twin (byte-exact, guarded outputs), the spaced planes
through the graphed runner against host spacing, and `run` with
spacing_mode device against host on the same runner."""
import collections
import dataclasses
import types

import numpy as np
import pytest
import torch

from deepconsensus_amd.preprocess import featurize_device as fd
from deepconsensus_amd.preprocess import spacing_device as spd
from deepconsensus_amd.preprocess.windows import DcConfig

from test_io_and_pipeline import make_test_bams
from test_spacing_device import (
    D, I, M, N, _preprocess, make_ccs, make_read, random_zmw,
)

pytestmark = pytest.mark.gpu

_GUARD = 64
_MAX_PASSES = 3
N_WINDOWS = 19


@pytest.fixture(scope="module")
def ext():
    from deepconsensus_amd import ops

    return ops.get_ext(required=True)


def _unspaced(reads, ccs, want_q, keep_subreads=True):
    config = DcConfig(_MAX_PASSES, 25, True)
    counter = collections.Counter()
    u = spd.build_unspaced(reads, ccs, config, None, counter)
    assert u is not None, counter
    u.win_start = np.zeros(1, np.int32)
    u.win_w = np.ones(1, np.int32)
    u.want_q = want_q
    if not keep_subreads:
        u = u.without_subreads()
    return types.SimpleNamespace(rows=None, planes=u)


@pytest.fixture(scope="module")
def packed(ext):
    """Three ZMWs: Lc = 1 with one read; Lc = 37 without kept subreads;
    Lc = 2 * T + 3 with max_passes reads (and a dropped one), one of them
    with an insertion run across the first tile boundary, one indented and
    ending early. The first ZMW's odd W makes every later offset odd."""
    T = int(ext.subread_space_tile())
    rng = np.random.default_rng(77)
    Lc = 2 * T + 3
    straddle = [M] * (T - 5) + [I] * 11 + [M, D] * 20
    straddle += [M] * (Lc - (T - 5) - 40) + [I, I]
    long_reads = [
        make_read(straddle, rng),
        make_read([N] * 7 + [I] * 3 + [M] * (T + 90) + [I] * 4, rng),
        random_zmw(5, Lc=Lc, n_reads=1)[0][0],
        make_read([M] * T + [I] * 20 + [M] * (Lc - T), rng),  # dropped
    ]
    zmws = [
        _unspaced([make_read([I, I, M, I, I], rng)], make_ccs(1, rng),
                  True),
        _unspaced(random_zmw(6, Lc=37, n_reads=2)[0], make_ccs(37, rng),
                  True, keep_subreads=False),
        _unspaced(long_reads, make_ccs(Lc, rng), False),
    ]
    batch = fd.pack_batch(zmws)
    widths = batch.zmw_tab[:, fd.TAB_W]
    assert widths[0] % 2 == 1 and batch.zmw_tab[1, fd.TAB_SUB_OFF] % 2 == 1
    assert batch.zmw_tab[:, fd.TAB_N_SUB].tolist() == [1, 0, _MAX_PASSES]
    # The dropped read holds the longest run of slot T.
    assert zmws[2].planes.ins_max[T] == 20
    assert batch.ccs_q.size and batch.ccs_bq.size
    return batch, T


def _guarded(a, lead=0):
    """Device copy of ``a`` (zeros) with _GUARD bytes of 0xA5 on both
    sides, ``lead`` more bytes in front to make the pointer odd."""
    g = (_GUARD + lead) // a.itemsize
    full = np.empty(len(a) + 2 * g, a.dtype)
    full.view(np.uint8)[:] = 0xA5
    full[g : g + len(a)] = 0
    big = torch.from_numpy(full).cuda()
    return big, big[g : g + len(a)], g


def _launch(ext, batch, lead=1):
    sp = batch.spacing
    outs = {
        "sub": _guarded(batch.sub, lead), "ccs": _guarded(batch.ccs, lead),
        "ccs_q": _guarded(batch.ccs_q, lead),
        "ccs_bq": _guarded(batch.ccs_bq),
        "col_ref": _guarded(np.zeros(len(sp.ins_max), np.int32)),
    }
    ext.subread_space_into(
        torch.from_numpy(sp.src.copy()).cuda(),
        torch.from_numpy(sp.ins_max.view(np.int16).copy()).cuda(),
        torch.from_numpy(sp.sp_tab.copy()).cuda(),
        torch.from_numpy(sp.read_tab.copy()).cuda(),
        torch.from_numpy(batch.zmw_tab.copy()).cuda(),
        outs["col_ref"][1], outs["sub"][1], outs["ccs"][1],
        outs["ccs_q"][1], outs["ccs_bq"][1], True,
    )
    torch.cuda.synchronize()
    got = {}
    for name, (big, view, g) in outs.items():
        raw = big.cpu().numpy()
        edge = raw[:g].view(np.uint8), raw[len(raw) - g:].view(np.uint8)
        assert (edge[0] == 0xA5).all() and (edge[1] == 0xA5).all(), name
        got[name] = view.cpu().numpy()
    return got


def test_kernel_matches_numpy_twin(ext, packed):
    batch, T = packed
    assert not batch.sub.any() and not batch.ccs.any()  # not yet spaced
    want = dataclasses.replace(
        batch, sub=batch.sub.copy(), ccs=batch.ccs.copy(),
        ccs_q=batch.ccs_q.copy(), ccs_bq=batch.ccs_bq.copy())
    spd.space_batch_numpy(want)
    assert want.sub.any() and want.ccs.any() and want.ccs_q.any()
    assert (want.ccs_bq == -1).any()
    # want_q off on the last ZMW: its ccs_q slice stays zero.
    off, W = (int(batch.zmw_tab[2, c]) for c in (fd.TAB_CCS_OFF, fd.TAB_W))
    assert not want.ccs_q[off : off + W].any()
    got = _launch(ext, batch)
    for name in ("sub", "ccs", "ccs_q", "ccs_bq"):
        assert got[name].dtype == getattr(want, name).dtype
        np.testing.assert_array_equal(got[name], getattr(want, name),
                                      err_msg=name)
    # Same batch, run again: bitwise-equal output.
    again = _launch(ext, batch)
    for name in got:
        assert np.array_equal(got[name], again[name]), name


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


def test_runner_path_matches_host_spacing(runner, monkeypatch):
    """Three unspaced ZMWs and one that falls back to host spacing, 19
    windows at batch_size 5: four graph replays, the last a short tail;
    then with a threshold that sends 11 of them through the device
    passthrough. The model input and the stitched output equal host
    spacing's."""
    from deepconsensus_amd.inference import quick_inference as qi

    for knob in ("DC_SERVE_GRAPH", "DC_SPACING_MODE", "DC_FEATURIZE_MODE",
                 "DC_STITCH_MODE", "DC_PASSTHROUGH_MODE"):
        monkeypatch.delenv(knob, raising=False)
    config = DcConfig(20, 100, False)
    cases = [random_zmw(70 + i, Lc=Lc, n_reads=n) for i, (Lc, n) in
             enumerate([(230, 4), (180, 22), (170, 3), (200, 1)])]
    rng = np.random.default_rng(2)
    cases[2][0][0] = make_read([M] * 172, rng)  # past the CCS: fallback
    outs = {}
    for passthrough, skip in (("host", 0), ("device", 12)):
        options = qi.InferenceOptions(
            batch_size=5, min_quality=0, skip_windows_above=skip,
            featurize_mode="device", stitch_mode="device",
            passthrough_mode=passthrough)
        zmws = {
            mode: [_preprocess(z, config, options, mode, f"m0/{k}/ccs")
                   for k, z in enumerate(cases)]
            for mode in ("host", "device")
        }
        assert [getattr(z.planes, "unspaced", False)
                for z in zmws["device"]] == [True, True, False, True]
        rows = {}
        for mode in ("host", "device"):
            chunks = qi._ModelChunks(zmws[mode], runner, options)
            assert chunks.use_graph
            assert (chunks.batch.spacing is not None) == (mode == "device")
            rows[mode] = [
                chunks.chunk(i)[0].cpu().numpy()
                for i in range(0, chunks.n_model, 5)]
        if not skip:
            assert chunks.n_model == N_WINDOWS
        assert len(rows["host"]) == len(rows["device"]) > 0
        for a, b in zip(rows["device"], rows["host"]):
            assert a.any() and np.array_equal(a, b)
        want = qi.run_model_and_stitch_on_zmws(zmws["host"], runner, options)
        got = qi.run_model_and_stitch_on_zmws(zmws["device"], runner,
                                              options)
        assert got.n_model == want.n_model
        assert got.n_skipped == want.n_skipped
        assert np.array_equal(got.seq_out, want.seq_out)
        assert np.array_equal(got.qual_out, want.qual_out)
        assert np.array_equal(got.out_off, want.out_off)
        outs[passthrough] = got
    assert outs["device"].n_skipped > 0 and outs["device"].n_model > 0


@pytest.mark.parametrize("modes", [
    dict(stitch_mode="serial"),
    dict(stitch_mode="device", passthrough_mode="device"),
], ids=["serial", "stitch+passthrough"])
def test_run_device_spacing_matches_host_on_gpu(tmp_path, modes,
                                                monkeypatch):
    from deepconsensus_amd.inference import quick_inference as qi

    for knob in ("DC_SPACING_MODE", "DC_FEATURIZE_MODE", "DC_STITCH_MODE",
                 "DC_PASSTHROUGH_MODE"):
        monkeypatch.delenv(knob, raising=False)
    sub, ccs = make_test_bams(tmp_path, n_zmws=4, length=300)
    seen = collections.Counter()
    real = fd.pack_batch

    def spy(zmws, **kw):
        seen.update("unspaced" if getattr(z.planes, "unspaced", False)
                    else "planes" for z in zmws if z.planes is not None)
        return real(zmws, **kw)

    monkeypatch.setattr(fd, "pack_batch", spy)
    outs, counters, kinds = {}, {}, {}
    for mode in ("host", "device"):
        seen.clear()
        torch.manual_seed(7)
        out = tmp_path / f"out_{mode}.fastq"
        options = qi.InferenceOptions(
            batch_size=4, batch_zmws=2, cpus=0, min_quality=0,
            skip_windows_above=27, featurize_mode="device",
            spacing_mode=mode, **modes,
        )
        counters[mode] = dataclasses.asdict(qi.run(
            subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
            output=str(out), options=options, device="cuda",
        ))
        outs[mode] = out.read_bytes()
        kinds[mode] = dict(seen)
    assert kinds["device"].get("planes", 0) == 0
    assert kinds["device"]["unspaced"] == kinds["host"]["planes"] > 0
    assert kinds["host"].get("unspaced", 0) == 0
    assert counters["host"]["success"] == 4
    assert counters["host"] == counters["device"]
    assert outs["host"] and outs["host"] == outs["device"]
