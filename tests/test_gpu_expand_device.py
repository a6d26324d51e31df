"""GPU tests for device-side alignment expansion: the cigar_expand kernel
against its numpy twin (byte-exact, guarded and pre-filled src), its output
through subread_space_into against the host-expanded planes, the graphed
runner path and `run` with expand_mode device against host on the same
runner. Only validated tables reach the GPU."""
import collections
import copy
import dataclasses

import numpy as np
import pytest
import torch

from deepconsensus_amd.preprocess import expand_device as xd
from deepconsensus_amd.preprocess import featurize_device as fd
from deepconsensus_amd.preprocess import feeder as pre_feeder
from deepconsensus_amd.preprocess import spacing_device as spd
from deepconsensus_amd.preprocess.windows import DcConfig

from test_expand_device import (
    D, I, M, S, X, _packed, _zmw, ccs_record, make_jobs, n_ref, record,
)
from test_io_and_pipeline import make_test_bams

pytestmark = pytest.mark.gpu

_GUARD = 64
_FILL = 0x5A
KNOBS = ("DC_SERVE_GRAPH", "DC_EXPAND_MODE", "DC_SPACING_MODE",
         "DC_FEATURIZE_MODE", "DC_STITCH_MODE", "DC_PASSTHROUGH_MODE")


@pytest.fixture(scope="module")
def ext():
    from deepconsensus_amd import ops

    return ops.get_ext(required=True)


@pytest.fixture(scope="module")
def packed(ext, tmp_path_factory):
    """Two ZMWs. The first read has l_seq = 1, so the operands of the later
    reads start at odd and even offsets of ``raw``; the second ZMW runs
    under ins_trim 2."""
    T = int(ext.cigar_expand_tile())
    stage = int(ext.cigar_expand_stage())
    assert T % 2 == 0 and 2 * stage <= T
    rng = np.random.default_rng(31)
    first = [
        record([(M, 1)], rng),
        record([(M, 2 * T + 3)], rng),  # one op, three tiles
        record([(M, T), (X, 5)], rng),  # an op boundary at element T
        record([(M, T - 2), (I, 5), (M, 4)], rng),  # an op across T
        record([(M, 2 * T - 3), (D, 7), (M, 3)], rng),  # D run across 2T
        record([(M, 10)], rng, pos=T + 5),
        record([(S, 3), (M, T + 1), (I, 2), (S, 3)], rng, reverse=True),
        # 2T op rows over two tiles: more than one LDS stage per tile.
        record([(M, 1), (I, 1)] * T, rng),
    ]
    assert len(first[6].seq) % 2 == 1
    second = [
        record([(M, 5), (I, 6), (M, T)], rng),  # dropped mid-read
        record([(S, 2), (I, 3), (M, 4), (I, 2), (M, 3)], rng, reverse=True),
    ]
    config = DcConfig(20, 25, True)
    zmws, hosts = [], []
    for k, (reads, ins_trim) in enumerate(((first, 0), (second, 2))):
        Lc = max(n_ref(r) for r in reads) + 2
        tmp = tmp_path_factory.mktemp(f"zmw{k}")
        (job,) = make_jobs(tmp, [(reads, ccs_record(Lc, rng))], ins_trim)
        raw = xd.build_raw(copy.deepcopy(job), config, None, ins_trim)
        assert raw is not None and raw.n_sub == len(reads)
        zmws.append(_zmw(raw))
        host = job.materialize(collections.Counter())
        hosts.append(_zmw(spd.build_unspaced(host[:-1], host[-1], config)))
    # Two trimmed insertions and a soft clip.
    assert (zmws[1].planes.ops[:, xd.OP_KIND] == xd.DROP).sum() == 3
    batch = fd.pack_batch(zmws)
    xr = batch.spacing.expand.xr_tab
    assert xr[1, xd.XR_SEQ] % 2 == 1 and (xr[:, xd.XR_TAG] % 2 == 1).any()
    assert xr[7, xd.XR_NOPS] > 2 * stage
    return batch, _packed(hosts)


def _guarded(n, fill, lead=1):
    """Device uint8 [n] filled with ``fill`` between _GUARD bytes of 0xA5,
    ``lead`` more in front to make the pointer odd."""
    g = _GUARD + lead
    full = np.full(n + 2 * g, 0xA5, np.uint8)
    full[g : g + n] = fill
    big = torch.from_numpy(full).cuda()
    return big, big[g : g + n], g


def _expand_on_device(ext, batch):
    sp = batch.spacing
    ex = sp.expand
    # The validator passed in pack_batch; once more on what is sent.
    xd.validate_expand_tables(ex.op_tab, ex.xr_tab, len(ex.raw), sp.n_src,
                              sp.n_src_host, sp.read_tab)
    big, src, g = _guarded(sp.n_src, _FILL)
    src[: sp.n_src_host].copy_(
        torch.from_numpy(sp.src[: sp.n_src_host].copy()))
    ext.cigar_expand_into(
        torch.from_numpy(ex.raw.copy()).cuda(),
        torch.from_numpy(ex.op_tab.copy()).cuda(),
        torch.from_numpy(ex.xr_tab.copy()).cuda(),
        src, torch.from_numpy(xd.NT16_LUT.copy()),
    )
    torch.cuda.synchronize()
    raw = big.cpu().numpy()
    assert (raw[:g] == 0xA5).all() and (raw[len(raw) - g:] == 0xA5).all()
    return src


def test_kernel_matches_numpy_twin(ext, packed):
    batch, _ = packed
    sp = batch.spacing
    assert not sp.src[sp.n_src_host:].any()  # not yet expanded
    want = sp.src.copy()
    xd.expand_reads_numpy(sp.expand.raw, sp.expand.op_tab,
                          sp.expand.xr_tab, want)
    assert (want[sp.n_src_host:] & spd.INS_FLAG).any()
    got = _expand_on_device(ext, batch).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    again = _expand_on_device(ext, batch).cpu().numpy()
    assert np.array_equal(got, again)


def test_expanded_reads_through_subread_space(ext, packed):
    """cigar_expand_into, then subread_space_into on its output: the planes
    of the host-expanded, host-spaced ZMWs."""
    batch, want = packed
    sp = batch.spacing
    src = _expand_on_device(ext, batch)
    outs = {name: torch.zeros(len(getattr(batch, name)),
                              dtype=getattr(torch, getattr(
                                  batch, name).dtype.name), device="cuda")
            for name in ("sub", "ccs", "ccs_q", "ccs_bq")}
    ext.subread_space_into(
        src, torch.from_numpy(sp.ins_max.view(np.int16).copy()).cuda(),
        torch.from_numpy(sp.sp_tab.copy()).cuda(),
        torch.from_numpy(sp.read_tab.copy()).cuda(),
        torch.from_numpy(batch.zmw_tab.copy()).cuda(),
        torch.zeros(len(sp.ins_max), dtype=torch.int32, device="cuda"),
        outs["sub"], outs["ccs"], outs["ccs_q"], outs["ccs_bq"], True,
    )
    torch.cuda.synchronize()
    assert want.sub.any()
    for name, t in outs.items():
        np.testing.assert_array_equal(t.cpu().numpy(), getattr(want, name),
                                      err_msg=name)


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


def test_runner_path_matches_host_expansion(runner, tmp_path, monkeypatch):
    """Four ZMWs from the feeder, one of which falls back (an inner clip),
    at batch_size 5 through the graph; then with a threshold that sends
    windows through the device passthrough. The model input and the
    stitched output equal host expansion's."""
    from deepconsensus_amd.dcio import bam as bam_lib
    from deepconsensus_amd.inference import quick_inference as qi

    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    sub, ccs = make_test_bams(tmp_path, n_zmws=4, length=230, seed=13)
    config = DcConfig(20, 100, False)
    feeder, _ = pre_feeder.create_proc_feeder(
        subreads_to_ccs=sub, ccs_bam=ccs, dc_config=config, ins_trim=0,
        defer_expansion=True)
    jobs = list(feeder())
    # ZMW 2: its first record gets a soft clip between two matches.
    job = jobs[2][0]
    rec = bam_lib.decode_record(job.read_set[0], job.header)
    rec.cigartuples = [(M, 100), (S, 10), (M, 120)]
    (clipped,) = make_jobs(tmp_path, [([rec], ccs_record(1, np.random
                                                         .default_rng(0)))])
    job.read_set[0] = clipped.read_set[0]
    outs = {}
    for passthrough, skip in (("host", 0), ("device", 27)):
        zmws = {}
        for mode in ("host", "device"):
            options = qi.InferenceOptions(
                batch_size=5, min_quality=0, skip_windows_above=skip,
                featurize_mode="device", stitch_mode="device",
                passthrough_mode=passthrough, spacing_mode="device",
                expand_mode=mode)
            zmws[mode] = [
                qi.preprocess_one_zmw((zmw, copy.deepcopy(j), dcc, ww,
                                       options))
                for j, zmw, dcc, _, ww in jobs]
        assert [getattr(z.planes, "raw_records", False)
                for z in zmws["device"]] == [True, True, False, True]
        assert zmws["device"][2].counter[
            xd.fallback_counter("inner_clip")] == 1
        rows = {}
        for mode in ("host", "device"):
            chunks = qi._ModelChunks(zmws[mode], runner, options)
            assert chunks.use_graph
            assert (chunks.batch.spacing.expand is not None) == (
                mode == "device")
            rows[mode] = [
                chunks.chunk(i)[0].cpu().numpy()
                for i in range(0, chunks.n_model, 5)]
        assert len(rows["host"]) == len(rows["device"]) > 1
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
def test_run_device_expand_matches_host_on_gpu(tmp_path, modes,
                                               monkeypatch):
    from deepconsensus_amd.inference import quick_inference as qi

    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    sub, ccs = make_test_bams(tmp_path, n_zmws=4, length=300)
    seen = collections.Counter()
    real = fd.pack_batch

    def spy(zmws, **kw):
        seen.update("raw" if getattr(z.planes, "raw_records", False)
                    else "other" for z in zmws if z.planes is not None)
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
            spacing_mode="device", expand_mode=mode, **modes,
        )
        counters[mode] = dataclasses.asdict(qi.run(
            subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
            output=str(out), options=options, device="cuda",
        ))
        outs[mode] = out.read_bytes()
        kinds[mode] = dict(seen)
    assert kinds["host"] == {"other": 4}
    assert kinds["device"] == {"raw": 4}
    assert counters["host"]["success"] == 4
    assert counters["host"] == counters["device"]
    assert outs["host"] and outs["host"] == outs["device"]
