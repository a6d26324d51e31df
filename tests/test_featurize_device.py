"""Device featurization, host side (preprocess/featurize_device.py):
worker planes + pack_batch + the kernel's numpy twin against the host
featurizer's int16 rows, the host validator, and `run` on CPU with
featurize_mode device against host."""
import collections
import dataclasses
import glob
import json
import os

import numpy as np
import pytest
import torch

from deepconsensus_amd.dcio import bam as bam_lib
from deepconsensus_amd.inference import quick_inference as qi
from deepconsensus_amd.preprocess import featurize_device as fd
from deepconsensus_amd.preprocess import feeder as pre_feeder
from deepconsensus_amd.preprocess.windows import DcConfig, DcExample

from test_io_and_pipeline import make_test_bams
from test_preprocess import _make_zmw, _make_zmw_with_insertions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_CASES = 200
# avg_phred threshold between the quartiles of human_1m's first ZMWs
# (median window Q10, upper quartile Q22): the model and the CCS
# passthrough each get a good share of the windows.
HUMAN_1M_SKIP = 15


def _smart_widths(rng, length, max_length):
    """Random partition of the CCS bases into smart-window widths, some
    above max_length (overflow)."""
    widths, left = [], length
    while left:
        w = min(left, int(rng.integers(1, int(1.5 * max_length) + 1)))
        widths.append(w)
        left -= w
    return np.array(widths)


def _case(seed):
    """(build, options, tags): build() returns a fresh spaced DcExample.

    Axes: use_ccs_bq, fixed / smart windows (widths < L and overflow), a
    last partial window, n_subreads in {1, max_passes, > max_passes},
    (max_passes, max_length) in {(20, 100), (3, 25)}, a window without
    any CCS index, and the skip threshold."""
    rng = np.random.default_rng(1000 + seed)
    max_passes, max_length = [(20, 100), (3, 25), (3, 100)][seed % 3]
    use_ccs_bq = bool(rng.integers(0, 2))
    length = int(rng.choice([130, 250, 257]))
    smart = rng.random() < 0.4
    widths = _smart_widths(rng, length, max_length) if smart else None
    plain = rng.random() < 0.4
    if plain:
        n_subreads = int(rng.choice(
            [1, max_passes, max_passes + 2] if max_passes == 3 else [1, 20, 22]
        ))
    blank = rng.random() < 0.2  # blank the CCS index of the second window
    threshold = int(rng.choice([0, 18, 19, 20, 45]))
    config = DcConfig(max_passes, max_length, use_ccs_bq)

    def build():
        if plain:
            ex = _make_zmw(n_subreads=n_subreads, length=length, seed=seed)
        else:
            ex = _make_zmw_with_insertions(length=length, seed=seed)
        ex = DcExample(ex.name, ex.reads, config, window_widths=widths)
        if blank:
            lo = max_length if widths is None else int(widths[0])
            hi = lo + (max_length if widths is None else int(widths[1]))
            ex.ccs.ccs_idx[lo:hi] = -1
        return ex

    options = qi.InferenceOptions(
        max_length=max_length, max_passes=max_passes,
        use_ccs_bq=use_ccs_bq, skip_windows_above=threshold,
        example_height=fd.tensor_height(max_passes, use_ccs_bq),
    )
    return build, options


def _preprocess(monkeypatch, ex, options, mode):
    """preprocess_one_zmw on an already spaced DcExample."""
    monkeypatch.setattr(
        pre_feeder, "subreads_to_dc_example",
        lambda subreads, **kw: subreads,
    )
    options = dataclasses.replace(options, featurize_mode=mode)
    return qi.preprocess_one_zmw(
        (ex.name, ex, ex.config, ex.window_widths, options)
    )


def _expand(zmws):
    """pack_batch + twin over every window of the batch."""
    batch = fd.pack_batch(zmws)
    return batch, fd.featurize_windows_numpy(
        batch, 0, batch.n_windows, batch.n_rows, batch.max_length,
        batch.max_passes, batch.use_ccs_bq,
    )


def _assert_same_zmw(dev, host):
    np.testing.assert_array_equal(dev.window_pos, host.window_pos)
    assert dev.window_pos.dtype == host.window_pos.dtype
    assert dev.skipped == host.skipped
    assert dev.counter == host.counter
    assert (dev.name, dev.ec, dev.np_num_passes, dev.rq, dev.rg) == (
        host.name, host.ec, host.np_num_passes, host.rq, host.rg)
    assert dev.n_model == host.n_model
    assert dev.n_examples == host.n_examples


@pytest.mark.parametrize("block", range(8))
def test_property_planes_expand_to_host_rows(monkeypatch, block):
    """25 seeded ZMWs per block (200 in all): device-mode worker output +
    pack_batch + twin equals the host-mode int16 rows bit for bit, and
    window_pos, passthrough outputs, counters and scalars are equal."""
    for seed in range(block * 25, (block + 1) * 25):
        build, options = _case(seed)
        host = _preprocess(monkeypatch, build(), options, "host")
        dev = _preprocess(monkeypatch, build(), options, "device")
        assert host.planes is None and dev.rows is None, seed
        _assert_same_zmw(dev, host)
        if host.rows is None:
            assert dev.planes is None, seed
            continue
        p = dev.planes
        assert p.sub.dtype == p.strand.dtype == p.ccs.dtype == np.uint8
        assert p.sn.dtype == np.int16 and p.sn.shape == (4,)
        assert p.win_start.dtype == p.win_w.dtype == np.int32
        assert (p.ccs_bq is not None) == options.use_ccs_bq
        batch, got = _expand([dev])
        assert got.dtype == host.rows.dtype == np.int16
        assert got.shape == host.rows.shape, seed
        assert np.array_equal(got, host.rows), seed


def test_property_cases_cover_every_window_kind(monkeypatch):
    """The generator reaches: a window skipped by quality, an overflow
    window, a window without CCS index, a model window narrower than L,
    each n_subreads class, both layouts and both use_ccs_bq values."""
    seen = collections.Counter()
    for seed in range(N_CASES):
        build, options = _case(seed)
        ex = build()
        dev = _preprocess(monkeypatch, ex, options, "device")
        c = dev.counter
        seen["overflow"] += c["n_examples_overflow"] > 0
        seen["no_ccs_idx"] += c["n_examples_no_ccs_idx"] > 0
        # Every overflow window is skipped; any further skip is by quality.
        seen["quality_skip"] += len(dev.skipped) > c["n_examples_overflow"]
        if dev.planes is not None:
            seen["narrow"] += bool(
                (dev.planes.win_w < options.max_length).any())
            seen["model"] += 1
        else:
            seen["no_model"] += 1
        mp = options.max_passes
        seen["n_sub_1"] += ex.n_subreads == 1
        seen["n_sub_eq"] += ex.n_subreads == mp
        seen["n_sub_gt"] += ex.n_subreads > mp
        seen[f"layout_{mp}_{options.max_length}"] += 1
        seen[f"bq_{options.use_ccs_bq}"] += 1
    for key in ("overflow", "no_ccs_idx", "quality_skip", "narrow", "model",
                "n_sub_1", "n_sub_eq", "n_sub_gt", "layout_20_100",
                "layout_3_25", "bq_True", "bq_False"):
        assert seen[key] > 0, (key, seen)


def test_zmw_with_every_window_skipped(monkeypatch):
    """No model windows: neither rows nor planes cross the pool boundary,
    and the batch packs to an empty table."""
    ex = _make_zmw_with_insertions(length=250, seed=5)
    options = qi.InferenceOptions(skip_windows_above=1)
    host = _preprocess(monkeypatch, ex, options, "host")
    dev = _preprocess(
        monkeypatch, _make_zmw_with_insertions(length=250, seed=5),
        options, "device")
    assert host.rows is None and dev.rows is None and dev.planes is None
    assert len(dev.skipped) == 3 and dev.n_model == 0
    _assert_same_zmw(dev, host)
    batch = fd.pack_batch([dev])
    assert batch.n_windows == 0 and len(batch.win_tab) == 0
    chunks = qi._ModelChunks([dev], None, options)
    assert chunks.n_model == 0 and len(chunks.all_pos) == 0


def _irregular(seed):
    """A ZMW off the fast path: one subread three columns short."""
    ex = _make_zmw_with_insertions(length=250, seed=seed)
    ex.reads[0] = ex.reads[0][: ex.width - 3]
    return ex


def test_batch_mixing_fallback_and_fast_path_zmws(monkeypatch):
    """Fast, fallback, all-skipped, fast: the fallback ZMW keeps host rows,
    its windows are -1 in the table, and the expanded batch equals the
    host rows in ZMW order."""
    options = qi.InferenceOptions(skip_windows_above=0)
    skip_all = qi.InferenceOptions(skip_windows_above=1)
    builders = [
        (lambda: _make_zmw_with_insertions(length=250, seed=1), options),
        (lambda: _irregular(2), options),
        (lambda: _make_zmw_with_insertions(length=130, seed=3), skip_all),
        (lambda: _make_zmw(n_subreads=22, length=257, seed=4), options),
    ]
    host = [_preprocess(monkeypatch, b(), o, "host") for b, o in builders]
    dev = [_preprocess(monkeypatch, b(), o, "device") for b, o in builders]
    for d, h in zip(dev, host):
        _assert_same_zmw(d, h)
    assert dev[1].planes is None and dev[1].rows is not None
    assert np.array_equal(dev[1].rows, host[1].rows)
    assert dev[0].planes is not None and dev[3].planes is not None
    want = np.concatenate([h.rows for h in host if h.rows is not None])
    batch = fd.pack_batch(dev, pad_multiple=4)
    n = [z.n_model for z in dev]
    assert n == [3, 3, 0, 3] and batch.n_windows == 9
    assert len(batch.win_tab) == 12
    assert batch.win_tab[:, 0].tolist() == [0] * 3 + [-1] * 3 + [1] * 3 + (
        [-1] * 3)
    assert batch.fallback_idx.tolist() == [3, 4, 5]
    # Chunked at a size that splits the fallback ZMW, tail padding included.
    got = np.concatenate([
        fd.featurize_chunk_numpy(batch, lo, lo + 4) for lo in (0, 4, 8)
    ])
    assert np.array_equal(got[:9], want)
    assert not got[9:].any()
    # The twin alone leaves the fallback windows zero.
    _, bare = _expand(dev)
    assert not bare[3:6].any() and np.array_equal(bare[:3], want[:3])


def _fast_zmw(monkeypatch, **kw):
    return _preprocess(
        monkeypatch, _make_zmw_with_insertions(length=250, seed=1, **kw),
        qi.InferenceOptions(skip_windows_above=0, **kw), "device")


@pytest.mark.parametrize("violation", [
    "start_negative", "w_zero", "w_above_L", "past_W", "n_sub_above_max",
    "table_length", "sub_shape", "bq_shape", "mixed_layout", "rows_shape",
    "pad_multiple", "alloc_size",
])
def test_pack_batch_rejects(monkeypatch, violation):
    z = _fast_zmw(monkeypatch)
    other = _fast_zmw(monkeypatch)
    p = z.planes
    zmws, kw = [z, other], {}
    if violation == "start_negative":
        p.win_start[1] = -1
    elif violation == "w_zero":
        p.win_w[0] = 0
    elif violation == "w_above_L":
        p.win_start[0], p.win_w[0] = 0, 101
    elif violation == "past_W":
        p.win_start[2] = p.width - p.win_w[2] + 1
    elif violation == "n_sub_above_max":
        p.max_passes = 3
        other.planes.max_passes = 3
    elif violation == "table_length":
        p.win_w = p.win_w[:-1]
    elif violation == "sub_shape":
        p.sub = p.sub[:, :, :-1]
    elif violation == "bq_shape":
        p.ccs_bq = np.zeros(p.width - 1, np.int16)
        other.planes.ccs_bq = np.zeros(other.planes.width, np.int16)
    elif violation == "mixed_layout":
        other.planes.max_length = 50
    elif violation == "rows_shape":
        other.planes = None
        other.rows = np.zeros((3, 86, 100), np.int16)
    elif violation == "pad_multiple":
        kw["pad_multiple"] = 0
    elif violation == "alloc_size":
        kw["alloc"] = lambda n: np.empty(n + 1, np.uint8)
    with pytest.raises(ValueError, match="pack_batch"):
        fd.pack_batch(zmws, **kw)
    # The same batch is accepted without the violation.
    fresh = [_fast_zmw(monkeypatch), _fast_zmw(monkeypatch)]
    assert fd.pack_batch(fresh).n_windows == 6


def test_pack_batch_offsets_and_alloc(monkeypatch):
    """Arrays are views of one buffer at the recorded offsets, the table
    offsets point at each ZMW's planes, and alloc's buffer is the one
    packed into."""
    zmws = [_fast_zmw(monkeypatch, use_ccs_bq=True),
            _fast_zmw(monkeypatch, use_ccs_bq=True)]
    given = []

    def alloc(n):
        given.append(np.full(n, 0xEE, np.uint8))
        return given[0]

    batch = fd.pack_batch(zmws, pad_multiple=4, alloc=alloc)
    assert batch.blob is given[0]
    for name in ("zmw_tab", "win_tab", "ccs_bq", "sub", "ccs"):
        arr = getattr(batch, name)
        lo = batch.offsets[name]
        assert lo % arr.dtype.itemsize == 0
        assert np.shares_memory(arr, batch.blob)
        assert np.array_equal(
            batch.blob[lo : lo + arr.nbytes], arr.reshape(-1).view(np.uint8))
    assert batch.zmw_tab.dtype == np.int64
    assert batch.zmw_tab.shape == (2, 5 + 20 + 4)
    assert batch.win_tab.shape == (8, 3) and batch.n_windows == 6
    for i, z in enumerate(zmws):
        p = z.planes
        sub_off, ccs_off, bq_off, n_sub, W = batch.zmw_tab[i, :5]
        assert (n_sub, W) == (p.n_sub, p.width)
        assert np.array_equal(
            batch.sub[sub_off : sub_off + p.sub.size], p.sub.reshape(-1))
        assert np.array_equal(batch.ccs[ccs_off : ccs_off + W], p.ccs)
        assert np.array_equal(batch.ccs_bq[bq_off : bq_off + W], p.ccs_bq)
        assert np.array_equal(batch.zmw_tab[i, 5 : 5 + n_sub], p.strand)
        assert not batch.zmw_tab[i, 5 + n_sub : 25].any()
        assert np.array_equal(batch.zmw_tab[i, 25:], p.sn)


def test_twin_clamps_a_malformed_table(monkeypatch):
    """The twin (like the kernel) never reads outside the planes: entries
    pack_batch would reject are clamped or come out as zero windows."""
    z = _fast_zmw(monkeypatch, use_ccs_bq=True)
    batch, good = _expand([z])
    W = int(batch.zmw_tab[0, fd.TAB_W])
    args = (batch.n_rows, 100, 20, True)

    def run(win_tab, zmw_tab=None):
        b = dataclasses.replace(
            batch, win_tab=np.asarray(win_tab, np.int32),
            zmw_tab=batch.zmw_tab if zmw_tab is None else zmw_tab)
        return fd.featurize_windows_numpy(b, 0, len(win_tab), *args)

    out = run([[0, -7, 100], [0, 0, 1000], [0, W + 50, 10], [5, 0, 100],
               [0, W - 10, 100], [0, 0, -3]])
    assert np.array_equal(out[0], good[0])  # start clamped to 0
    assert np.array_equal(out[1], good[0])  # w clamped to L
    assert not out[3].any()  # zmw_index outside the table
    # w clamped to what is left of the ZMW / to nothing: the data columns
    # are zero past w, strand and SN rows stay, ccs_bq pads with -1.
    for o, w in ((out[2], 0), (out[4], 10), (out[5], 0)):
        assert not o[:60, w:].any() and not o[80, w:].any()
        assert (o[81, w:] == -1).all()
        assert np.array_equal(o[60:80], good[0][60:80])
        assert np.array_equal(o[82:], good[0][82:])
    # Planes that do not lie inside the packed arrays: a zero window.
    for col, value in ((fd.TAB_SUB_OFF, len(batch.sub)),
                       (fd.TAB_CCS_OFF, -1), (fd.TAB_BQ_OFF, 1),
                       (fd.TAB_W, W + 1), (fd.TAB_N_SUB, -1),
                       (fd.TAB_N_SUB, 21)):
        tab = batch.zmw_tab.copy()
        tab[0, col] = value
        assert not run([[0, 0, 100]], tab).any(), col
    with pytest.raises(ValueError):
        fd.featurize_windows_numpy(batch, 0, 1, 85, 100, 20, True)
    with pytest.raises(ValueError):
        fd.featurize_windows_numpy(batch, 0, 99, *args)


def test_featurize_mode_resolution(monkeypatch):
    monkeypatch.delenv("DC_FEATURIZE_MODE", raising=False)
    assert qi.FEATURIZE_MODES == ("host", "device")
    assert qi.InferenceOptions().featurize_mode is None
    assert qi.resolve_featurize_mode(qi.InferenceOptions()) == "host"
    monkeypatch.setenv("DC_FEATURIZE_MODE", "device")
    assert qi.resolve_featurize_mode(qi.InferenceOptions()) == "device"
    assert qi.resolve_featurize_mode(
        qi.InferenceOptions(featurize_mode="host")) == "host"
    with pytest.raises(ValueError):
        qi.resolve_featurize_mode(qi.InferenceOptions(featurize_mode="gpu"))
    monkeypatch.setenv("DC_FEATURIZE_MODE", "gpu")
    with pytest.raises(ValueError):
        qi.resolve_featurize_mode(qi.InferenceOptions())


def test_cli_flag(monkeypatch):
    from deepconsensus_amd import cli

    seen = {}
    monkeypatch.setattr(
        qi, "run", lambda **kw: seen.update(kw) or qi.stitch_utils
        .OutcomeCounter(success=1))
    cli.main(["run", "--subreads_to_ccs", "a.bam", "--ccs_bam", "b.bam",
              "--checkpoint", "random", "--output", "o.fastq",
              "--featurize_mode", "device"])
    assert seen["options"].featurize_mode == "device"
    with pytest.raises(SystemExit):
        cli.main(["run", "--subreads_to_ccs", "a.bam", "--ccs_bam", "b.bam",
                  "--checkpoint", "random", "--output", "o.fastq",
                  "--featurize_mode", "gpu"])


def _spy_planes(monkeypatch):
    """Counts, per call of the two model loops, the windows that arrived
    as planes and as host rows."""
    seen = collections.Counter()
    for fn in ("run_model_on_zmws", "run_model_and_stitch_on_zmws"):
        real = getattr(qi, fn)

        def spy(zmws, runner, options, real=real):
            seen["planes"] += sum(
                z.n_model for z in zmws if z.planes is not None)
            seen["rows"] += sum(
                len(z.rows) for z in zmws if z.rows is not None)
            seen["skipped"] += sum(len(z.skipped) for z in zmws)
            return real(zmws, runner, options)

        monkeypatch.setattr(qi, fn, spy)
    return seen


def _run_both(tmp_path, monkeypatch, sub, ccs, suffix, stitch_mode,
              limit=0, **kw):
    """`run` on CPU with featurize_mode host and device; returns the two
    output paths after comparing counters and .inference.json."""
    monkeypatch.delenv("DC_FEATURIZE_MODE", raising=False)
    monkeypatch.delenv("DC_STITCH_MODE", raising=False)
    seen = _spy_planes(monkeypatch)
    outs, counters, stats, windows = {}, {}, {}, {}
    for mode in ("host", "device"):
        seen.clear()
        torch.manual_seed(7)
        out = tmp_path / f"out_{stitch_mode}_{mode}.{suffix}"
        options = qi.InferenceOptions(
            cpus=0, min_quality=0, stitch_mode=stitch_mode,
            featurize_mode=mode, **kw,
        )
        c = qi.run(subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
                   output=str(out), options=options, device="cpu",
                   limit=limit)
        outs[mode] = out
        counters[mode] = dataclasses.asdict(c)
        stats[mode] = json.load(
            open(tmp_path / f"out_{stitch_mode}_{mode}.inference.json"))
        windows[mode] = dict(seen)
    assert windows["host"]["rows"] > 0
    assert windows["host"].get("planes", 0) == 0
    assert windows["device"]["planes"] == windows["host"]["rows"]
    assert windows["device"].get("rows", 0) == 0
    assert windows["device"]["skipped"] == windows["host"]["skipped"] > 0
    assert counters["host"] == counters["device"]
    assert counters["host"]["success"] > 0
    assert stats["host"] == stats["device"]
    return outs


@pytest.mark.parametrize("stitch_mode", ["serial", "device"])
def test_run_device_featurize_matches_host_fastq(
        tmp_path, monkeypatch, stitch_mode):
    sub, ccs = make_test_bams(tmp_path, n_zmws=4, length=350, seed=3)
    outs = _run_both(tmp_path, monkeypatch, sub, ccs, "fastq", stitch_mode,
                     batch_size=4, batch_zmws=3, skip_windows_above=27)
    host = outs["host"].read_bytes()
    assert host and outs["device"].read_bytes() == host


@pytest.mark.parametrize("stitch_mode", ["serial", "device"])
def test_run_device_featurize_matches_host_bam(
        tmp_path, monkeypatch, stitch_mode):
    sub, ccs = make_test_bams(tmp_path, n_zmws=4, length=350, seed=3)
    outs = _run_both(tmp_path, monkeypatch, sub, ccs, "bam", stitch_mode,
                     batch_size=4, batch_zmws=3, skip_windows_above=27)
    assert outs["device"].read_bytes() == outs["host"].read_bytes()
    records = list(bam_lib.BamReader(str(outs["device"])))
    assert len(records) == 4 and all(len(r.seq) > 0 for r in records)


@pytest.fixture(scope="module")
def human_1m(tmp_path_factory):
    """The golden human_1m BAMs, their .partN pieces joined (as
    test_golden_reference.py assembles them)."""
    root = tmp_path_factory.mktemp("human_1m")
    for name in ("subreads_to_ccs.bam", "ccs.bam"):
        parts = sorted(glob.glob(
            os.path.join(GOLDEN, "human_1m", name + ".part*")))
        srcs = parts or [os.path.join(GOLDEN, "human_1m", name)]
        with open(root / name, "wb") as dst:
            for src in srcs:
                with open(src, "rb") as f:
                    dst.write(f.read())
    return root


@pytest.mark.parametrize("stitch_mode", ["serial", "device"])
def test_run_device_featurize_matches_host_on_human_1m(
        tmp_path, monkeypatch, human_1m, stitch_mode):
    """Real reads: insertions, both strands, varied pw/ip/SN. The skip
    threshold sends about half of the windows through the model."""
    outs = _run_both(
        tmp_path, monkeypatch, str(human_1m / "subreads_to_ccs.bam"),
        str(human_1m / "ccs.bam"), "fastq", stitch_mode,
        batch_size=32, batch_zmws=2, skip_windows_above=HUMAN_1M_SKIP,
        ins_trim=5, limit=3,
    )
    host = outs["host"].read_bytes()
    assert host and outs["device"].read_bytes() == host


def test_env_knob_and_end_after_stage(tmp_path, monkeypatch):
    """DC_FEATURIZE_MODE selects the mode (with the stitch knob next to
    it); run_model still stops before any read is written."""
    sub, ccs = make_test_bams(tmp_path, n_zmws=2, length=150, seed=3)
    monkeypatch.setenv("DC_FEATURIZE_MODE", "device")
    monkeypatch.setenv("DC_STITCH_MODE", "device")
    seen = _spy_planes(monkeypatch)
    out = tmp_path / "out.fastq"
    c = qi.run(
        subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
        output=str(out), device="cpu",
        options=qi.InferenceOptions(
            batch_size=8, batch_zmws=2, cpus=0, min_quality=0,
            skip_windows_above=0, end_after_stage=qi.DebugStage.RUN_MODEL,
        ),
    )
    assert seen["planes"] == 4 and seen["rows"] == 0
    assert c.total == 0 and out.read_bytes() == b""
    # Earlier stages never reach the model loop.
    seen.clear()
    qi.run(
        subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
        output=str(out), device="cpu",
        options=qi.InferenceOptions(
            cpus=0, end_after_stage=qi.DebugStage.TF_EXAMPLES),
    )
    assert not seen
    monkeypatch.setenv("DC_FEATURIZE_MODE", "gpu")
    with pytest.raises(ValueError, match="featurize_mode"):
        qi.run(subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
               output=str(out), device="cpu")


def test_worker_pool_ships_planes(tmp_path, monkeypatch):
    """cpus > 0: planes survive the pool pipe and the output still equals
    the in-process host run."""
    sub, ccs = make_test_bams(tmp_path, n_zmws=3, length=250, seed=5)
    monkeypatch.delenv("DC_FEATURIZE_MODE", raising=False)
    outs = {}
    for mode, cpus in (("host", 0), ("device", 2)):
        torch.manual_seed(7)
        out = tmp_path / f"out_{mode}.fastq"
        qi.run(subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
               output=str(out), device="cpu",
               options=qi.InferenceOptions(
                   batch_size=4, batch_zmws=2, cpus=cpus, min_quality=0,
                   skip_windows_above=0, featurize_mode=mode))
        outs[mode] = out.read_bytes()
    assert outs["host"] and outs["host"] == outs["device"]
