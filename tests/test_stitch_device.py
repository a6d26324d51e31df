"""Device-stitch host side (postprocess/stitch_device.py) against the
Python stitcher: plan ordering, numpy compaction, outcome taxonomy, and
`run` in DC_STITCH_MODE=device on CPU vs serial."""
import collections
import dataclasses
import io
import json

import numpy as np
import pytest
import torch

from deepconsensus_amd.dcio import bam as bam_lib
from deepconsensus_amd.inference import quick_inference as qi
from deepconsensus_amd.postprocess import stitch, stitch_device
from deepconsensus_amd.utils import constants, phred

from test_io_and_pipeline import make_test_bams

_VOCAB = np.frombuffer(constants.SEQ_VOCAB.encode("ascii"), np.uint8)


def _zmw(name, pos, ids, quals, skipped, tag):
    """ZmwWindows whose `rows` stand in for the model output: row 0 of
    window i carries its base ids, row 1 its QVs."""
    rows = None
    if len(pos):
        rows = np.stack([np.stack([i, q]) for i, q in zip(ids, quals)])
    return qi.ZmwWindows(
        name=name, window_pos=np.asarray(pos, np.int64), rows=rows,
        skipped=skipped, counter=collections.Counter(),
        ec=float(tag), np_num_passes=tag, rq=0.9, rg=f"rg{tag}",
    )


def _passthrough(name, pos, ids, quals, tag):
    return stitch.DCModelOutput(
        molecule_name=name, window_pos=pos,
        sequence=_VOCAB[ids].tobytes().decode("ascii"),
        quality_string=phred.quality_scores_to_string(quals),
        ec=100.0 + tag, np_num_passes=100 + tag, rq=0.5, rg=f"sk{tag}",
    )


def _predictions(zmws):
    """The DCModelOutput list run_model_on_zmws builds: every skipped
    window first, then the model windows in concatenation order."""
    preds = [sk for z in zmws for sk in z.skipped]
    for z in zmws:
        if z.rows is None:
            continue
        for pos, row in zip(z.window_pos, z.rows):
            preds.append(stitch.DCModelOutput(
                molecule_name=z.name, window_pos=int(pos),
                sequence=_VOCAB[row[0]].tobytes().decode("ascii"),
                quality_string=phred.quality_scores_to_string(row[1]),
                ec=z.ec, np_num_passes=z.np_num_passes, rq=z.rq, rg=z.rg,
            ))
    return preds


def _serial(zmws, options):
    counter = stitch.OutcomeCounter()
    out = io.StringIO()
    qi._write_outputs(_predictions(zmws), out, None, options, counter)
    return out.getvalue(), counter


def _device_host(zmws, options):
    """build_plan + numpy compaction + finish_reads through the writer the
    orchestrator uses."""
    model = [z for z in zmws if z.rows is not None]
    all_pos = (np.concatenate([z.window_pos for z in model])
               if model else np.empty(0, np.int64))
    plan = stitch_device.build_plan(zmws, all_pos, options.max_length)
    if model:
        rows = np.concatenate([z.rows for z in model]).astype(np.uint8)
        flat_b, flat_q = rows[:, 0].reshape(-1), rows[:, 1].reshape(-1)
    else:
        flat_b = flat_q = np.empty(0, np.uint8)
    bases = np.concatenate([flat_b, plan.extra_bases])
    quals = np.concatenate([flat_q, plan.extra_quals])
    assert len(bases) == plan.n_source_bytes
    seq_out, qual_out, seg_kept, out_off = (
        stitch_device.compact_segments_numpy(
            bases, quals, plan.seg_off, plan.seg_len
        )
    )
    assert out_off[0] == 0 and (np.diff(out_off) == seg_kept).all()
    assert len(seq_out) == len(qual_out) == out_off[-1]
    counter = stitch.OutcomeCounter()
    out = io.StringIO()
    batch = qi.StitchedBatch(
        plan=plan, seq_out=seq_out, qual_out=qual_out, out_off=out_off,
        n_model=plan.n_model, n_skipped=sum(len(z.skipped) for z in zmws),
    )
    qi._write_stitched(batch, out, None, options, counter)
    return out.getvalue(), counter


def _random_case(seed):
    rng = np.random.default_rng(seed)
    max_length = int(rng.choice([8, 100]))
    options = qi.InferenceOptions(
        max_length=max_length,
        min_quality=int(rng.choice([0, 10, 20])),
        min_length=int(rng.choice([0, 50])),
    )
    n_reads = int(rng.integers(1, 7))
    # Names whose string order differs from their numeric order.
    numbers = rng.choice(np.arange(1, 1200), size=n_reads, replace=False)
    zmws = []
    for tag, number in enumerate(numbers):
        name = f"m{int(rng.integers(0, 2))}/{int(number)}/ccs"
        n_win = int(rng.integers(0, 13))
        q_hi = int(rng.choice([6, 25, 94]))
        pos, ids, quals, skipped = [], [], [], []
        for k in range(n_win):
            if rng.random() < 0.08:
                continue  # window removed: a later one makes it "missing"
            kind = rng.random()
            passthrough = rng.random() < 0.25
            length = max_length
            if passthrough:
                length = int(rng.choice(
                    [1, 137, max_length, int(rng.integers(0, 150))]
                ))
            if kind < 0.15:
                w_ids = np.zeros(length, np.int64)  # all gap
            elif kind < 0.3:
                w_ids = rng.integers(1, 5, length)  # no gap
            else:
                w_ids = rng.integers(0, 5, length)
            w_q = rng.integers(0, q_hi, length)
            if passthrough:
                skipped.append(
                    _passthrough(name, k * max_length, w_ids, w_q, tag)
                )
                if rng.random() < 0.1:
                    # A model window at the same position: tie order.
                    pos.append(k * max_length)
                    ids.append(rng.integers(0, 5, max_length))
                    quals.append(rng.integers(0, q_hi, max_length))
            else:
                pos.append(k * max_length)
                ids.append(w_ids)
                quals.append(w_q)
        zmws.append(_zmw(name, pos, ids, quals, skipped, tag))
    return zmws, options


@pytest.mark.parametrize("block", range(10))
def test_property_matches_python_stitcher(block):
    """25 seeded cases per block (250 in all): FASTQ text and every
    OutcomeCounter field equal _write_outputs on the same windows."""
    for seed in range(block * 25, (block + 1) * 25):
        zmws, options = _random_case(seed)
        want_text, want_counter = _serial(zmws, options)
        got_text, got_counter = _device_host(zmws, options)
        assert got_text == want_text, seed
        assert dataclasses.asdict(got_counter) == dataclasses.asdict(
            want_counter
        ), seed


def test_property_cases_cover_every_outcome():
    """The generator reaches each outcome, passthrough lengths 1 and 137,
    and batches with and without model windows."""
    total = stitch.OutcomeCounter()
    lengths = set()
    for seed in range(250):
        zmws, options = _random_case(seed)
        _, c = _serial(zmws, options)
        for f in dataclasses.fields(c):
            setattr(total, f.name,
                    getattr(total, f.name) + getattr(c, f.name))
        lengths.update(len(sk.sequence) for z in zmws for sk in z.skipped)
    assert all(v > 0 for v in dataclasses.asdict(total).values()), total
    assert {1, 137} <= lengths


def _both(zmws, **kw):
    options = qi.InferenceOptions(**kw)
    want = _serial(zmws, options)
    got = _device_host(zmws, options)
    assert got[0] == want[0]
    assert dataclasses.asdict(got[1]) == dataclasses.asdict(want[1])
    return got


def test_all_q10_read_passes_min_quality_10():
    """The rounding case stitch.py documents: all-Q10 averages 9.99999..."""
    ids = [np.full(100, 1 + k) for k in range(3)]
    quals = [np.full(100, 10)] * 3
    z = _zmw("m0/7/ccs", [0, 100, 200], ids, quals, [], 0)
    text, counter = _both([z], min_quality=10)
    assert counter.success == 1 and text.count("\n") == 4


def test_all_q0_read():
    z = _zmw("m0/7/ccs", [0], [np.full(100, 2)], [np.zeros(100, int)], [], 0)
    _, counter = _both([z], min_quality=0)
    assert counter.success == 1
    _, counter = _both([z], min_quality=10)
    assert counter.failed_quality_filter == 1


def test_only_gaps_read():
    zeros = np.zeros(100, int)
    sk = _passthrough("m0/7/ccs", 100, np.zeros(37, int), np.full(37, 5), 0)
    z = _zmw("m0/7/ccs", [0], [zeros], [np.full(100, 30)], [sk], 0)
    text, counter = _both([z], min_quality=0)
    assert text == "" and counter.only_gaps == 1 and counter.total == 1


def test_batch_without_model_windows():
    rng = np.random.default_rng(3)
    zmws = []
    for tag, name in enumerate(["m0/9/ccs", "m0/10/ccs"]):
        skipped = [
            _passthrough(name, k * 100, rng.integers(0, 5, n),
                         rng.integers(20, 60, n), tag)
            for k, n in enumerate([100, 137, 1])
        ]
        zmws.append(_zmw(name, [], [], [], skipped, tag))
    text, counter = _both(zmws, min_quality=0)
    assert counter.success == 2
    # String order: "m0/10/ccs" sorts before "m0/9/ccs".
    assert text.index("@m0/10/ccs") < text.index("@m0/9/ccs")


def test_first_window_metadata_follows_sorted_order():
    """BAM tags come from the read's first window after sorting: the
    passthrough window at position 0 here, not the model window."""
    sk = _passthrough("m0/7/ccs", 0, np.full(5, 1), np.full(5, 30), 4)
    z = _zmw("m0/7/ccs", [100], [np.full(100, 2)], [np.full(100, 30)],
             [sk], 9)
    plan = stitch_device.build_plan([z], None, 100)
    assert plan.read_metadata == [(104.0, 104, 0.5, "sk4")]
    assert plan.seg_off.tolist() == [100, 0]
    assert plan.seg_len.tolist() == [5, 100]


def test_max_base_quality_above_93_rejected():
    z = _zmw("m0/7/ccs", [], [], [], [], 0)
    with pytest.raises(ValueError, match="max_base_quality"):
        qi.run_model_and_stitch_on_zmws(
            [z], None, qi.InferenceOptions(max_base_quality=94)
        )


def test_stitch_mode_resolution(monkeypatch):
    monkeypatch.delenv("DC_STITCH_MODE", raising=False)
    assert qi.resolve_stitch_mode(qi.InferenceOptions()) == "serial"
    monkeypatch.setenv("DC_STITCH_MODE", "device")
    assert qi.resolve_stitch_mode(qi.InferenceOptions()) == "device"
    assert qi.resolve_stitch_mode(
        qi.InferenceOptions(stitch_mode="serial")) == "serial"
    with pytest.raises(ValueError):
        qi.resolve_stitch_mode(qi.InferenceOptions(stitch_mode="gpu"))


def _run_modes(tmp_path, monkeypatch, suffix):
    """`run` on CPU in serial and device mode on the same BAMs; records
    how many model and passthrough windows each mode saw."""
    sub, ccs = make_test_bams(tmp_path, n_zmws=4, length=350, seed=3)
    seen = {}
    for mode, fn in (("serial", "run_model_on_zmws"),
                     ("device", "run_model_and_stitch_on_zmws")):
        real = getattr(qi, fn)
        counts = seen[mode] = collections.Counter()

        def spy(zmws, runner, options, real=real, counts=counts):
            counts["model"] += sum(
                len(z.rows) for z in zmws if z.rows is not None)
            counts["skipped"] += sum(len(z.skipped) for z in zmws)
            return real(zmws, runner, options)

        monkeypatch.setattr(qi, fn, spy)
    monkeypatch.delenv("DC_STITCH_MODE", raising=False)
    outs, counters, stats = {}, {}, {}
    for mode in ("serial", "device"):
        torch.manual_seed(7)
        out = tmp_path / f"out_{mode}.{suffix}"
        options = qi.InferenceOptions(
            batch_size=4, batch_zmws=3, cpus=0, min_quality=0,
            skip_windows_above=27, stitch_mode=mode,
        )
        c = qi.run(subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
                   output=str(out), options=options, device="cpu")
        outs[mode] = out
        counters[mode] = dataclasses.asdict(c)
        stats[mode] = json.load(
            open(tmp_path / f"out_{mode}.inference.json"))
    assert seen["serial"] == seen["device"]
    assert seen["device"]["model"] > 0 and seen["device"]["skipped"] > 0
    assert counters["serial"] == counters["device"]
    assert counters["device"]["success"] == 4
    assert stats["serial"] == stats["device"]
    return outs


def test_run_device_mode_matches_serial_fastq(tmp_path, monkeypatch):
    outs = _run_modes(tmp_path, monkeypatch, "fastq")
    serial = outs["serial"].read_bytes()
    assert serial and outs["device"].read_bytes() == serial


def test_run_device_mode_matches_serial_bam(tmp_path, monkeypatch):
    outs = _run_modes(tmp_path, monkeypatch, "bam")
    serial = list(bam_lib.BamReader(str(outs["serial"])))
    device = list(bam_lib.BamReader(str(outs["device"])))
    assert len(serial) == len(device) == 4
    for a, b in zip(serial, device):
        assert (a.qname, a.flag, a.ref_id, a.pos, a.mapq) == (
            b.qname, b.flag, b.ref_id, b.pos, b.mapq)
        assert a.seq == b.seq and len(a.seq) > 0
        assert list(a.query_qualities) == list(b.query_qualities)
        assert a.tags == b.tags
        assert set(a.tags) >= {"ec", "np", "rq", "RG", "zm"}


def test_run_device_mode_env_knob_and_end_after_stage(tmp_path, monkeypatch):
    """The env knob selects the mode; run_model still stops before any
    read is written."""
    sub, ccs = make_test_bams(tmp_path, n_zmws=2, length=150, seed=3)
    monkeypatch.setenv("DC_STITCH_MODE", "device")
    called = []
    real = qi.run_model_and_stitch_on_zmws
    monkeypatch.setattr(
        qi, "run_model_and_stitch_on_zmws",
        lambda *a: called.append(1) or real(*a),
    )
    out = tmp_path / "out.fastq"
    c = qi.run(
        subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
        output=str(out), device="cpu",
        options=qi.InferenceOptions(
            batch_size=8, batch_zmws=2, cpus=0, min_quality=0,
            skip_windows_above=0, end_after_stage=qi.DebugStage.RUN_MODEL,
        ),
    )
    assert called and c.total == 0 and out.read_bytes() == b""
