"""Device CCS passthrough, host side: the worker's passthrough table +
pack_batch + the kernel's numpy twin against the host mode's
DCModelOutput, the quality LUT against the host arithmetic, build_plan
with table and object passthrough windows, the host validator, mode
resolution, and `run` on CPU with passthrough_mode device against host."""
import collections
import csv
import dataclasses
import glob
import json
import os

import numpy as np
import pytest
import torch

from deepconsensus_amd.calibration import calibration as calibration_lib
from deepconsensus_amd.inference import quick_inference as qi
from deepconsensus_amd.postprocess import stitch_device as sd
from deepconsensus_amd.preprocess import featurize_device as fd
from deepconsensus_amd.preprocess import feeder as pre_feeder
from deepconsensus_amd.preprocess.windows import DcConfig, DcExample
from deepconsensus_amd.utils import constants

from test_io_and_pipeline import make_test_bams
from test_preprocess import _make_zmw, _make_zmw_with_insertions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_CASES = 120
# As tests/test_featurize_device.py: between the quartiles of human_1m's
# first ZMWs, so both window classes get a good share.
HUMAN_1M_SKIP = 15
DEVICE = dict(featurize_mode="device", stitch_mode="device")
_ASCII_TO_ID = {c: i for i, c in enumerate(constants.SEQ_VOCAB)}


def _smart_widths(rng, length, max_length):
    widths, left = [], length
    while left:
        w = min(left, int(rng.integers(1, int(1.5 * max_length) + 1)))
        widths.append(w)
        left -= w
    return np.array(widths)


def _case(seed):
    """(build, options): build() returns a fresh spaced DcExample.

    Axes: fixed / smart windows (widths below L and overflow), a ragged
    last window, use_ccs_bq, two layouts, and skip thresholds that skip
    no window (0: overflow only), some (18..20) or every window (1)."""
    rng = np.random.default_rng(5000 + seed)
    max_passes, max_length = [(20, 100), (3, 25)][seed % 2]
    use_ccs_bq = bool(rng.integers(0, 2))
    length = int(rng.choice([130, 250, 257]))
    smart = rng.random() < 0.5
    widths = _smart_widths(rng, length, max_length) if smart else None
    threshold = int(rng.choice([0, 1, 18, 19, 20, 45]))
    config = DcConfig(max_passes, max_length, use_ccs_bq)

    def build():
        ex = _make_zmw_with_insertions(length=length, seed=seed)
        return DcExample(ex.name, ex.reads, config, window_widths=widths)

    options = qi.InferenceOptions(
        max_length=max_length, max_passes=max_passes,
        use_ccs_bq=use_ccs_bq, skip_windows_above=threshold,
        example_height=fd.tensor_height(max_passes, use_ccs_bq), **DEVICE,
    )
    return build, options


def _preprocess(monkeypatch, ex, options, mode):
    """preprocess_one_zmw on an already spaced DcExample."""
    monkeypatch.setattr(
        pre_feeder, "subreads_to_dc_example",
        lambda subreads, **kw: subreads,
    )
    monkeypatch.delenv("DC_PASSTHROUGH_MODE", raising=False)
    options = dataclasses.replace(options, passthrough_mode=mode)
    return qi.preprocess_one_zmw(
        (ex.name, ex, ex.config, ex.window_widths, options)
    )


def _expand(zmws, options):
    """pack_batch + LUT + twin: (batch, ids, qvs) of the passthrough
    region."""
    batch = fd.pack_batch(zmws)
    ids = np.full(batch.n_pt_bytes, 0xEE, np.uint8)
    qvs = np.full(batch.n_pt_bytes, 0xEE, np.uint8)
    fd.passthrough_fill_numpy(
        batch.ccs, batch.ccs_q, batch.zmw_tab, batch.pt_tab,
        qi.passthrough_quality_lut(options), ids, qvs)
    return batch, ids, qvs


def _decode(output):
    """(ids, QVs) of a DCModelOutput over its full padded width."""
    ids = np.array([_ASCII_TO_ID[c] for c in output.sequence], np.uint8)
    qvs = np.frombuffer(
        output.quality_string.encode("ascii"), np.uint8) - np.uint8(33)
    return ids, qvs


def _assert_table_equals_objects(dev, host, options, seed=None):
    """dev's passthrough table expands to host's skipped objects."""
    p = dev.planes
    assert dev.skipped == [] and p is not None and p.ccs_q is not None
    assert p.ccs_q.dtype == np.uint8 and p.ccs_q.shape == p.ccs.shape
    assert p.pt_start.dtype == p.pt_w.dtype == p.pt_width.dtype == np.int32
    assert p.pt_pos.dtype == np.int64
    assert len(p.pt_start) == len(host.skipped), seed
    batch, ids, qvs = _expand([dev], options)
    assert batch.pt_tab.dtype == np.int32
    assert batch.n_pt_bytes == sum(len(sk.sequence) for sk in host.skipped)
    for k, sk in enumerate(host.skipped):
        _, start, w, width, dst = (int(v) for v in batch.pt_tab[k])
        assert width == len(sk.sequence) == len(sk.quality_string), seed
        assert int(p.pt_pos[k]) == sk.window_pos, seed
        want_ids, want_qvs = _decode(sk)
        assert np.array_equal(ids[dst : dst + width], want_ids), (seed, k)
        assert np.array_equal(qvs[dst : dst + width], want_qvs), (seed, k)
        assert (sk.molecule_name, sk.ec, sk.np_num_passes, sk.rq, sk.rg) == (
            dev.name, dev.ec, dev.np_num_passes, dev.rq, dev.rg)


@pytest.mark.parametrize("block", range(6))
def test_property_table_expands_to_host_passthrough(monkeypatch, block):
    """20 seeded ZMWs per block: the device-mode worker's table + pack_batch
    + LUT + twin equals, window by window, the ids and QVs of the host
    mode's DCModelOutput over the full padded width; model windows,
    counters and scalars are those of the host mode."""
    for seed in range(block * 20, (block + 1) * 20):
        build, options = _case(seed)
        host = _preprocess(monkeypatch, build(), options, "host")
        dev = _preprocess(monkeypatch, build(), options, "device")
        np.testing.assert_array_equal(dev.window_pos, host.window_pos)
        assert dev.counter == host.counter, seed
        assert (dev.n_model, dev.n_skipped, dev.n_examples) == (
            host.n_model, host.n_skipped, host.n_examples), seed
        assert host.n_skipped == len(host.skipped)
        if not host.skipped:
            # Nothing skipped: exactly the featurize-mode output.
            assert dev.planes.ccs_q is None
            assert fd.n_table_passthrough(dev) == 0
            continue
        _assert_table_equals_objects(dev, host, options, seed)
        if host.n_model:
            assert np.array_equal(dev.planes.sub, host.planes.sub)
            assert np.array_equal(dev.planes.win_start,
                                  host.planes.win_start)
        else:
            assert host.planes is None
            assert dev.planes.sub.shape == (3, 0, dev.planes.width)


def test_property_cases_cover_every_window_kind(monkeypatch):
    """The generator reaches: a table window skipped by quality, an
    overflow one, one narrower than its padded width, ZMWs with none, some
    and all windows skipped, both layouts and both use_ccs_bq values."""
    seen = collections.Counter()
    for seed in range(N_CASES):
        build, options = _case(seed)
        dev = _preprocess(monkeypatch, build(), options, "device")
        n_pt, c = fd.n_table_passthrough(dev), dev.counter
        seen["overflow"] += c["n_examples_overflow"] > 0
        seen["quality_skip"] += n_pt > c["n_examples_overflow"]
        if n_pt:
            p = dev.planes
            seen["padded"] += bool((p.pt_w < p.pt_width).any())
            seen["wide"] += bool((p.pt_width > options.max_length).any())
            seen["odd_start"] += bool((p.pt_start % 4 != 0).any())
        seen["none_skipped"] += n_pt == 0
        seen["some_skipped"] += n_pt > 0 and dev.n_model > 0
        seen["all_skipped"] += n_pt > 0 and dev.n_model == 0
        seen[f"L_{options.max_length}"] += 1
        seen[f"bq_{options.use_ccs_bq}"] += 1
    for key in ("overflow", "quality_skip", "padded", "wide", "odd_start",
                "none_skipped", "some_skipped", "all_skipped", "L_100",
                "L_25", "bq_True", "bq_False"):
        assert seen[key] > 0, (key, seen)


def _irregular(seed):
    """A ZMW off the fast path: one subread three columns short."""
    ex = _make_zmw_with_insertions(length=250, seed=seed)
    ex.reads[0] = ex.reads[0][: ex.width - 3]
    return ex


def test_zmws_that_keep_host_objects(monkeypatch):
    """Off the fast path, or with qualities outside the uint8 code, a ZMW
    keeps `skipped` objects equal to the host mode's; host mode itself
    never fills a table."""
    options = qi.InferenceOptions(skip_windows_above=1, **DEVICE)

    def fractional():
        ex = _make_zmw_with_insertions(length=250, seed=2)
        q = ex.ccs.base_quality_scores.astype(np.float64)
        q[q >= 0] += 0.5
        ex.ccs.base_quality_scores = q
        return ex

    def too_large():
        ex = _make_zmw_with_insertions(length=250, seed=2)
        q = ex.ccs.base_quality_scores.astype(np.int64)
        q[3] = 255
        ex.ccs.base_quality_scores = q
        return ex

    for build in (lambda: _irregular(2), fractional, too_large):
        host = _preprocess(monkeypatch, build(), options, "host")
        dev = _preprocess(monkeypatch, build(), options, "device")
        assert len(host.skipped) == 3 and dev.skipped == host.skipped
        assert fd.n_table_passthrough(dev) == 0
        assert dev.planes is None and dev.n_skipped == 3
    assert fd.encode_ccs_qualities(np.array([-1.0, 0.0, 254.0])).tolist() == [
        0, 1, 255]
    assert fd.encode_ccs_qualities(np.array([-2, 3])) is None
    assert fd.encode_ccs_qualities(np.array([np.nan, 3.0])) is None
    host = _preprocess(
        monkeypatch, _make_zmw_with_insertions(length=250, seed=2), options,
        "host")
    assert host.planes is None and len(host.skipped) == 3


@pytest.mark.parametrize("max_base_quality", [93, 40])
@pytest.mark.parametrize(
    "ccs_calibration", ["skip", "10,0.99,0.15", "0,1.197654,-0.99781"])
def test_lut_equals_host_arithmetic(ccs_calibration, max_base_quality):
    """All 256 codes: the LUT entry of code q + 1 is the QV the host
    passthrough gives quality q, whatever the window it arrives in."""
    options = qi.InferenceOptions(
        max_base_quality=max_base_quality,
        ccs_calibration_values=calibration_lib.parse_calibration_string(
            ccs_calibration))
    assert options.ccs_calibration_values.enabled == (
        ccs_calibration != "skip")
    lut = qi.passthrough_quality_lut(options)
    assert lut.dtype == np.uint8 and lut.shape == (256,)
    assert lut.max() <= max_base_quality
    q = np.arange(-1, 255)
    got = []
    # The host path on windows of 100 columns, int and float qualities.
    for lo in range(0, 256, 100):
        for dtype in (np.int64, np.float64, np.int16):
            bq = q[lo : lo + 100].astype(dtype)
            out = qi._passthrough_output(
                np.ones(len(bq), np.uint8), bq, 0, "m/1/ccs", None, None,
                None, None, options)
            got.append((lo, _decode(out)[1]))
    for lo, qvs in got:
        assert np.array_equal(qvs, lut[lo : lo + len(qvs)]), lo
    if ccs_calibration == "skip":
        assert np.array_equal(
            lut, np.clip(q, 0, max_base_quality).astype(np.uint8))
    with pytest.raises(ValueError):
        qi.passthrough_quality_lut(qi.InferenceOptions(max_base_quality=94))


def _plan_zmw(monkeypatch, name, mode, seed, skip_windows=(), length=250,
              irregular=False, drop_first=False):
    """A ZMW whose windows `skip_windows` (of three) take the passthrough:
    their CCS qualities are raised above the threshold."""
    ex = (_irregular(seed) if irregular
          else _make_zmw_with_insertions(length=length, seed=seed))
    ex.name = name
    q = ex.ccs.base_quality_scores.copy()
    q[q >= 0] = 5
    for k in skip_windows:
        win = q[100 * k : 100 * (k + 1)]
        win[win >= 0] = 60
    ex.ccs.base_quality_scores = q
    options = qi.InferenceOptions(skip_windows_above=30, **DEVICE)
    z = _preprocess(monkeypatch, ex, options, mode)
    if drop_first:
        # The window at position 0 never arrives: a missing-window read.
        if z.skipped:
            del z.skipped[0]
        else:
            p = z.planes
            p.pt_start, p.pt_w, p.pt_width, p.pt_pos = (
                a[1:] for a in (p.pt_start, p.pt_w, p.pt_width, p.pt_pos))
    return z


def _resolved(plan, zmws, options, model_bytes):
    """The bytes every segment of the plan points at, in output order."""
    n_model_bytes = plan.n_model * plan.row_length
    buf = np.full((2, plan.n_source_bytes), 0xEE, np.uint8)
    buf[:, :n_model_bytes] = model_bytes
    batch = fd.pack_batch(
        [z for z in zmws if z.n_model or fd.n_table_passthrough(z)])
    assert batch.n_pt_bytes == plan.n_table_bytes
    lo = n_model_bytes + plan.n_table_bytes
    fd.passthrough_fill_numpy(
        batch.ccs, batch.ccs_q, batch.zmw_tab, batch.pt_tab,
        qi.passthrough_quality_lut(options), buf[0, n_model_bytes:lo],
        buf[1, n_model_bytes:lo])
    buf[0, lo:] = plan.extra_bases
    buf[1, lo:] = plan.extra_quals
    return [
        buf[:, o : o + n].copy() for o, n in zip(plan.seg_off, plan.seg_len)
    ]


def test_build_plan_parity_in_a_mixed_batch(monkeypatch):
    """Table passthrough, object passthrough and model windows in one
    batch give the segment bytes, read order, read_empty and metadata of
    the same batch with objects only."""
    spec = [
        # name (out of sorted order), kwargs
        ("m0/50/ccs", dict(seed=1, skip_windows=(0, 2))),  # starts skipped
        ("m0/9/ccs", dict(seed=2, skip_windows=(0, 1, 2))),  # all skipped
        ("m0/30/ccs", dict(seed=3, skip_windows=(1,), irregular=True)),
        ("m0/7/ccs", dict(seed=4, skip_windows=(0, 1), drop_first=True)),
        ("m0/40/ccs", dict(seed=5)),  # model windows only
        ("m0/20/ccs", dict(seed=6, skip_windows=(1,))),
    ]
    options = qi.InferenceOptions(skip_windows_above=30, **DEVICE)
    zmws = {
        mode: [_plan_zmw(monkeypatch, name, mode, **kw) for name, kw in spec]
        for mode in ("host", "device")
    }
    mixed, objects = zmws["device"], zmws["host"]
    assert [fd.n_table_passthrough(z) for z in mixed] == [2, 3, 0, 1, 0, 1]
    assert [len(z.skipped) for z in mixed] == [0, 0, 1, 0, 0, 0]
    assert [len(z.skipped) for z in objects] == [2, 3, 1, 1, 0, 1]
    assert [z.n_model for z in mixed] == [z.n_model for z in objects] == [
        1, 0, 2, 1, 3, 2]
    assert all(fd.n_table_passthrough(z) == 0 for z in objects)
    # A tag that differs per ZMW, so metadata cannot come from a neighbour.
    for group in (mixed, objects):
        for k, z in enumerate(group):
            z.rq = 0.9 + k / 100
            z.skipped = [
                dataclasses.replace(sk, rq=z.rq) for sk in z.skipped]
    plans = {
        "mixed": sd.build_plan(mixed, None, 100),
        "objects": sd.build_plan(objects, None, 100),
    }
    p, q = plans["mixed"], plans["objects"]
    assert p.n_model == q.n_model == 9
    assert p.n_table_bytes == 700 and q.n_table_bytes == 0
    assert len(p.extra_bases) == 100 and len(q.extra_bases) == 800
    assert p.n_source_bytes == q.n_source_bytes
    assert p.read_names == q.read_names == sorted(n for n, _ in spec)
    assert np.array_equal(p.read_empty, q.read_empty)
    assert p.read_empty.tolist() == [
        n == "m0/7/ccs" for n in p.read_names]
    assert np.array_equal(p.read_seg_start, q.read_seg_start)
    assert p.read_metadata == q.read_metadata
    assert len({m[2] for m in p.read_metadata}) == len(spec)
    assert np.array_equal(p.seg_len, q.seg_len)
    rng = np.random.default_rng(0)
    model_bytes = rng.integers(0, 5, (2, 900), dtype=np.uint8)
    got = _resolved(p, mixed, options, model_bytes)
    want = _resolved(q, objects, options, model_bytes)
    assert len(got) == len(want) == 15  # 18 windows, 3 of the empty read
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    # And the whole path: same reads out of the CPU model loop.
    runner = _cpu_runner()
    torch.manual_seed(3)
    a = qi.run_model_and_stitch_on_zmws(mixed, runner, options)
    torch.manual_seed(3)
    b = qi.run_model_and_stitch_on_zmws(objects, runner, options)
    assert (a.n_model, a.n_skipped, len(a)) == (9, 8, 17)
    assert (b.n_model, b.n_skipped) == (9, 8)
    for name in ("seq_out", "qual_out", "out_off"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    with pytest.raises(ValueError, match="device stitcher"):
        qi.run_model_on_zmws(mixed, runner, options)


def _cpu_runner():
    from deepconsensus_amd.models import config as cfg
    from deepconsensus_amd.models.model import get_model
    from deepconsensus_amd.models.runner import InferenceRunner

    params = cfg.get_config("transformer_learn_values+custom")
    cfg.modify_params(params, is_training=False)
    torch.manual_seed(11)
    return InferenceRunner(params, get_model(params), device="cpu")


def test_batch_of_passthrough_windows_only(monkeypatch):
    """No model window in the batch: the planes still get packed and the
    reads come out as in host mode."""
    options = qi.InferenceOptions(skip_windows_above=30, **DEVICE)
    zmws = {
        mode: [
            _plan_zmw(monkeypatch, f"m0/{k}/ccs", mode, seed=k,
                      skip_windows=(0, 1, 2)) for k in (3, 4)
        ] for mode in ("host", "device")
    }
    assert all(z.n_model == 0 for z in zmws["device"])
    chunks = qi._ModelChunks(zmws["device"], None, options)
    assert chunks.n_model == 0 and chunks.batch.n_pt_bytes == 600
    runner = _cpu_runner()
    a = qi.run_model_and_stitch_on_zmws(zmws["device"], runner, options)
    b = qi.run_model_and_stitch_on_zmws(zmws["host"], runner, options)
    assert a.plan.n_table_bytes == 600 and b.plan.n_table_bytes == 0
    assert a.n_skipped == b.n_skipped == 6 and len(a.seq_out) > 0
    for name in ("seq_out", "qual_out", "out_off"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.plan.read_names == b.plan.read_names


def _table_zmw(monkeypatch):
    return _plan_zmw(monkeypatch, "m0/1/ccs", "device", seed=1,
                     skip_windows=(0, 2))


def test_pack_batch_without_passthrough_is_unchanged(monkeypatch):
    """No table: the blob, its offsets and its size are what featurize
    mode alone packs; with one, ccs_q lies like ccs."""
    options = qi.InferenceOptions(skip_windows_above=0, **DEVICE)
    z = _preprocess(
        monkeypatch, _make_zmw_with_insertions(length=250, seed=1), options,
        "device")
    assert z.planes.ccs_q is None
    batch = fd.pack_batch([z])
    assert len(batch.ccs_q) == 0 and batch.pt_tab.shape == (0, 5)
    assert batch.n_pt_bytes == 0
    assert batch.offsets["pt_tab"] == batch.offsets["ccs_bq"]
    assert batch.offsets["ccs_q"] == len(batch.blob)
    z = _table_zmw(monkeypatch)
    batch = fd.pack_batch([z], pad_multiple=4)
    for name in ("pt_tab", "ccs_q"):
        arr, lo = getattr(batch, name), batch.offsets[name]
        assert lo % arr.dtype.itemsize == 0
        assert np.shares_memory(arr, batch.blob)
        assert np.array_equal(
            batch.blob[lo : lo + arr.nbytes], arr.reshape(-1).view(np.uint8))
    off, W = batch.zmw_tab[0, fd.TAB_CCS_OFF], batch.zmw_tab[0, fd.TAB_W]
    assert np.array_equal(batch.ccs_q[off : off + W], z.planes.ccs_q)
    assert batch.pt_tab.tolist() == [
        [0, 0, 100, 100, 0],
        [0, 200, z.planes.width - 200, 100, 100]]


@pytest.mark.parametrize("violation", [
    "start_negative", "w_zero", "w_above_width", "past_W", "no_ccs_q",
    "ccs_q_shape", "column_length", "total",
])
def test_pack_batch_rejects_passthrough(monkeypatch, violation):
    z = _table_zmw(monkeypatch)
    p = z.planes
    if violation == "start_negative":
        p.pt_start[0] = -1
    elif violation == "w_zero":
        p.pt_w[1] = 0
    elif violation == "w_above_width":
        p.pt_w[0], p.pt_width[0] = 100, 99
    elif violation == "past_W":
        p.pt_start[1] += 1
    elif violation == "no_ccs_q":
        p.ccs_q = None
    elif violation == "ccs_q_shape":
        p.ccs_q = p.ccs_q[:-1]
    elif violation == "column_length":
        p.pt_width = p.pt_width[:-1]
    elif violation == "total":
        p.pt_width[:] = 2**30
    with pytest.raises(ValueError, match="pack_batch"):
        fd.pack_batch([z])
    assert fd.pack_batch([_table_zmw(monkeypatch)]).n_pt_bytes == 200


def test_validate_passthrough_table():
    good = np.array([[0, 0, 100, 100, 0], [1, 7, 3, 137, 100],
                     [0, 150, 50, 100, 237]], np.int32)
    assert fd.validate_passthrough_table(good, [200, 10]) == 337
    assert fd.validate_passthrough_table(good[:0], []) == 0
    for row, col, value in ((1, fd.PT_ZMW, 2), (1, fd.PT_ZMW, -1),
                            (0, fd.PT_START, -1), (2, fd.PT_W, 0),
                            (2, fd.PT_W, 101), (2, fd.PT_START, 151),
                            (1, fd.PT_DST, 99), (2, fd.PT_DST, 236),
                            (0, fd.PT_DST, 1), (1, fd.PT_WIDTH, 2)):
        bad = good.copy()
        bad[row, col] = value
        with pytest.raises(ValueError, match="pack_batch"):
            fd.validate_passthrough_table(bad, [200, 10])
    big = np.array([[0, 0, 1, 2**30, 0], [0, 0, 1, 2**30, 2**30]], np.int64)
    with pytest.raises(ValueError, match="too large"):
        fd.validate_passthrough_table(big, [5])
    with pytest.raises(ValueError):
        fd.validate_passthrough_table(good[:, :4], [200, 10])


def test_twin_clamps_a_malformed_table(monkeypatch):
    """Entries the validator rejects are clamped or come out as id 0 /
    quality 0, and nothing outside [dst_off, dst_off + width) or outside
    the output is written."""
    options = qi.InferenceOptions(skip_windows_above=30, **DEVICE)
    batch = fd.pack_batch([_table_zmw(monkeypatch)])
    lut = qi.passthrough_quality_lut(options)
    lut[0] = 9  # tell padding from a dead entry
    W = int(batch.zmw_tab[0, fd.TAB_W])
    ccs, ccs_q = batch.ccs, batch.ccs_q

    def run(table, n=400, zmw_tab=None, ccs_q=ccs_q):
        ids = np.full(n, 0xEE, np.uint8)
        qvs = np.full(n, 0xEE, np.uint8)
        fd.passthrough_fill_numpy(
            ccs, ccs_q, batch.zmw_tab if zmw_tab is None else zmw_tab,
            np.asarray(table, np.int32).reshape(-1, 5), lut, ids, qvs)
        return ids, qvs

    ids, qvs = run([0, 20, 30, 50, 100])
    assert np.array_equal(ids[100:130], ccs[20:50])
    assert np.array_equal(qvs[100:130], lut[ccs_q[20:50]])
    assert not ids[130:150].any() and (qvs[130:150] == 9).all()
    for out in (ids, qvs):
        assert (out[:100] == 0xEE).all() and (out[150:] == 0xEE).all()
    # start < 0 -> 0; w > width -> width; w < 0 -> 0.
    ids, _ = run([0, -5, 500, 50, 0])
    assert np.array_equal(ids[:50], ccs[:50]) and (ids[50:] == 0xEE).all()
    ids, qvs = run([0, 0, -4, 50, 0])
    assert not ids[:50].any() and (qvs[:50] == 9).all()
    # Past the ZMW: w clamped to what is left / to nothing.
    ids, _ = run([0, W - 10, 100, 100, 0])
    assert np.array_equal(ids[:10], ccs[W - 10 : W]) and not ids[10:100].any()
    ids, qvs = run([0, W + 50, 10, 20, 0])
    assert not ids[:20].any() and (qvs[:20] == 9).all()
    # Segments that leave the output on either side, or have no width.
    ids, _ = run([[0, 0, 100, 100, -40], [0, 0, 100, 100, 380],
                  [0, 0, 10, -7, 200], [0, 0, 10, 10, 400],
                  [0, 0, 10, 10, -10]])
    assert np.array_equal(ids[:60], ccs[40:100])
    assert np.array_equal(ids[380:], ccs[:20])
    assert (ids[60:380] == 0xEE).all()
    # Dead entries: id 0 and quality 0, not the padding quality.
    dead = [[-1, 0, 10, 10, 0], [1, 0, 10, 10, 10]]
    for col, value in ((fd.TAB_CCS_OFF, -1), (fd.TAB_W, len(ccs) + 1),
                       (fd.TAB_CCS_OFF, len(ccs)), (fd.TAB_W, -1)):
        tab = batch.zmw_tab.copy()
        tab[0, col] = value
        ids, qvs = run([0, 0, 10, 10, 0], zmw_tab=tab)
        assert not ids[:10].any() and not qvs[:10].any(), (col, value)
    ids, qvs = run(dead)
    assert not ids[:20].any() and not qvs[:20].any()
    assert (ids[20:] == 0xEE).all()
    ids, qvs = run([0, 0, 10, 10, 0], ccs_q=ccs_q[:-1])  # ccs_q too short
    assert not ids[:10].any() and not qvs[:10].any()
    ids, _ = run(np.empty((0, 5)))  # P == 0
    assert (ids == 0xEE).all()
    with pytest.raises(ValueError):
        fd.passthrough_fill_numpy(
            ccs, ccs_q, batch.zmw_tab, batch.pt_tab, lut[:255],
            np.zeros(4, np.uint8), np.zeros(4, np.uint8))
    with pytest.raises(ValueError):
        fd.passthrough_fill_numpy(
            ccs, ccs_q, batch.zmw_tab, batch.pt_tab, lut,
            np.zeros(4, np.uint8), np.zeros(5, np.uint8))


def test_passthrough_mode_resolution(monkeypatch):
    for knob in ("DC_PASSTHROUGH_MODE", "DC_FEATURIZE_MODE",
                 "DC_STITCH_MODE"):
        monkeypatch.delenv(knob, raising=False)
    assert qi.PASSTHROUGH_MODES == ("host", "device")
    assert qi.InferenceOptions().passthrough_mode is None
    assert qi.resolve_passthrough_mode(qi.InferenceOptions()) == "host"
    assert qi.resolve_passthrough_mode(
        qi.InferenceOptions(passthrough_mode="device", **DEVICE)) == "device"
    with pytest.raises(ValueError, match="passthrough_mode"):
        qi.resolve_passthrough_mode(
            qi.InferenceOptions(passthrough_mode="gpu", **DEVICE))
    for others in (dict(), dict(featurize_mode="device"),
                   dict(stitch_mode="device"),
                   dict(featurize_mode="device", stitch_mode="serial"),
                   dict(featurize_mode="host", stitch_mode="device")):
        with pytest.raises(ValueError, match="needs featurize_mode"):
            qi.resolve_passthrough_mode(
                qi.InferenceOptions(passthrough_mode="device", **others))
        # host combines with everything.
        assert qi.resolve_passthrough_mode(
            qi.InferenceOptions(passthrough_mode="host", **others)) == "host"
    # The env knobs resolve all three.
    monkeypatch.setenv("DC_PASSTHROUGH_MODE", "device")
    with pytest.raises(ValueError, match="needs featurize_mode"):
        qi.resolve_passthrough_mode(qi.InferenceOptions())
    monkeypatch.setenv("DC_FEATURIZE_MODE", "device")
    monkeypatch.setenv("DC_STITCH_MODE", "device")
    assert qi.resolve_passthrough_mode(qi.InferenceOptions()) == "device"
    assert qi.resolve_passthrough_mode(
        qi.InferenceOptions(passthrough_mode="host")) == "host"
    monkeypatch.setenv("DC_PASSTHROUGH_MODE", "gpu")
    with pytest.raises(ValueError, match="passthrough_mode"):
        qi.resolve_passthrough_mode(qi.InferenceOptions())


def test_run_rejects_the_mode_before_any_worker_starts(tmp_path, monkeypatch):
    monkeypatch.delenv("DC_FEATURIZE_MODE", raising=False)
    monkeypatch.delenv("DC_STITCH_MODE", raising=False)
    started = []
    monkeypatch.setattr(
        pre_feeder, "create_proc_feeder",
        lambda **kw: started.append(kw) or (lambda: iter(()), {}))
    out = tmp_path / "out.fastq"
    for options in (
        qi.InferenceOptions(passthrough_mode="device"),
        qi.InferenceOptions(passthrough_mode="device",
                            featurize_mode="device", stitch_mode="serial"),
        qi.InferenceOptions(passthrough_mode="gpu", **DEVICE),
    ):
        with pytest.raises(ValueError, match="passthrough_mode"):
            qi.run(subreads_to_ccs="a.bam", ccs_bam="b.bam",
                   checkpoint="random", output=str(out), options=options,
                   device="cpu")
    assert not started and not out.exists()


def test_cli_flag(monkeypatch):
    from deepconsensus_amd import cli

    seen = {}
    monkeypatch.setattr(
        qi, "run", lambda **kw: seen.update(kw) or qi.stitch_utils
        .OutcomeCounter(success=1))
    base = ["run", "--subreads_to_ccs", "a.bam", "--ccs_bam", "b.bam",
            "--checkpoint", "random", "--output", "o.fastq"]
    cli.main(base)
    assert seen["options"].passthrough_mode is None
    cli.main(base + ["--passthrough_mode", "device", "--featurize_mode",
                     "device", "--stitch_mode", "device"])
    assert seen["options"].passthrough_mode == "device"
    assert qi.resolve_passthrough_mode(seen["options"]) == "device"
    with pytest.raises(SystemExit):
        cli.main(base + ["--passthrough_mode", "gpu"])


def _spy_windows(monkeypatch):
    """Counts, per call of the device model loop, the windows that arrived
    as table entries, as skipped objects and as model windows."""
    seen = collections.Counter()
    real = qi.run_model_and_stitch_on_zmws

    def spy(zmws, runner, options):
        seen["table"] += sum(fd.n_table_passthrough(z) for z in zmws)
        seen["objects"] += sum(len(z.skipped) for z in zmws)
        seen["model"] += sum(z.n_model for z in zmws)
        out = real(zmws, runner, options)
        seen["table_bytes"] += out.plan.n_table_bytes
        return out

    monkeypatch.setattr(qi, "run_model_and_stitch_on_zmws", spy)
    return seen


def _timing_rows(path):
    """The runtime CSV without its wall-clock column."""
    with open(path) as f:
        return [
            {k: v for k, v in row.items() if k != "runtime"}
            for row in csv.DictReader(f)
        ]


def _run_both(tmp_path, monkeypatch, sub, ccs, suffix, limit=0, **kw):
    """`run` on CPU with passthrough_mode host and device (featurize and
    stitch mode device in both); returns the two output paths after
    comparing counters, .inference.json and the timing stages."""
    for knob in ("DC_PASSTHROUGH_MODE", "DC_FEATURIZE_MODE",
                 "DC_STITCH_MODE"):
        monkeypatch.delenv(knob, raising=False)
    seen = _spy_windows(monkeypatch)
    outs, counters, stats, windows, timings = {}, {}, {}, {}, {}
    for mode in ("host", "device"):
        seen.clear()
        torch.manual_seed(7)
        out = tmp_path / f"out_{mode}.{suffix}"
        options = qi.InferenceOptions(
            cpus=0, min_quality=0, passthrough_mode=mode, **DEVICE, **kw)
        c = qi.run(subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
                   output=str(out), options=options, device="cpu",
                   limit=limit)
        outs[mode] = out
        counters[mode] = dataclasses.asdict(c)
        stats[mode] = json.load(
            open(tmp_path / f"out_{mode}.inference.json"))
        timings[mode] = _timing_rows(tmp_path / f"out_{mode}.runtime.csv")
        windows[mode] = dict(seen)
    # A run that fell back to objects cannot pass.
    assert windows["host"]["objects"] > 0
    assert windows["host"].get("table", 0) == 0
    assert windows["device"]["table"] == windows["host"]["objects"]
    assert windows["device"].get("objects", 0) == 0
    assert windows["device"]["table_bytes"] >= 100 * windows["device"]["table"]
    assert windows["device"]["model"] == windows["host"]["model"] > 0
    assert counters["host"] == counters["device"]
    assert counters["host"]["success"] > 0
    assert stats["host"] == stats["device"]
    assert timings["host"] == timings["device"]
    return outs


def test_run_device_passthrough_matches_host_fastq(tmp_path, monkeypatch):
    sub, ccs = make_test_bams(tmp_path, n_zmws=4, length=350, seed=3)
    outs = _run_both(tmp_path, monkeypatch, sub, ccs, "fastq",
                     batch_size=4, batch_zmws=3, skip_windows_above=27)
    host = outs["host"].read_bytes()
    assert host and outs["device"].read_bytes() == host


def test_run_device_passthrough_matches_host_bam(tmp_path, monkeypatch):
    sub, ccs = make_test_bams(tmp_path, n_zmws=4, length=350, seed=3)
    outs = _run_both(tmp_path, monkeypatch, sub, ccs, "bam",
                     batch_size=4, batch_zmws=3, skip_windows_above=27)
    assert outs["device"].read_bytes() == outs["host"].read_bytes()


def test_run_device_passthrough_matches_host_on_human_1m(
        tmp_path, monkeypatch):
    """Real reads; the threshold sends about half of the windows through
    the passthrough."""
    for name in ("subreads_to_ccs.bam", "ccs.bam"):
        parts = sorted(glob.glob(
            os.path.join(GOLDEN, "human_1m", name + ".part*")))
        srcs = parts or [os.path.join(GOLDEN, "human_1m", name)]
        with open(tmp_path / name, "wb") as dst:
            for src in srcs:
                with open(src, "rb") as f:
                    dst.write(f.read())
    outs = _run_both(
        tmp_path, monkeypatch, str(tmp_path / "subreads_to_ccs.bam"),
        str(tmp_path / "ccs.bam"), "fastq", batch_size=32, batch_zmws=2,
        skip_windows_above=HUMAN_1M_SKIP, ins_trim=5, limit=3,
    )
    host = outs["host"].read_bytes()
    assert host and outs["device"].read_bytes() == host


def test_worker_pool_ships_tables(tmp_path, monkeypatch):
    """cpus > 0 and the env knobs: the tables survive the pool pipe and
    the output equals the in-process host run."""
    sub, ccs = make_test_bams(tmp_path, n_zmws=3, length=250, seed=5)
    for knob in ("DC_PASSTHROUGH_MODE", "DC_FEATURIZE_MODE",
                 "DC_STITCH_MODE"):
        monkeypatch.setenv(knob, "device")
    seen = _spy_windows(monkeypatch)
    outs = {}
    for mode, cpus in (("host", 0), (None, 2)):
        seen.clear()
        torch.manual_seed(7)
        out = tmp_path / f"out_{mode}.fastq"
        qi.run(subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
               output=str(out), device="cpu",
               options=qi.InferenceOptions(
                   batch_size=4, batch_zmws=2, cpus=cpus, min_quality=0,
                   skip_windows_above=27, passthrough_mode=mode))
        outs[mode] = out.read_bytes()
    assert seen["table"] > 0 and seen["objects"] == 0
    assert outs["host"] and outs["host"] == outs[None]
