"""Device subread spacing, host side: the closed form against the spacing
state machine, build_unspaced + pack_batch + the kernel's numpy twin against
the host path (space_out_subreads -> DcExample -> build_planes ->
pack_batch), the fallback causes, the host validator, mode resolution, and
`run` on CPU with spacing_mode device against host."""
import collections
import copy
import dataclasses
import glob
import os

import numpy as np
import pytest
import torch

from deepconsensus_amd.inference import quick_inference as qi
from deepconsensus_amd.preprocess import featurize_device as fd
from deepconsensus_amd.preprocess import feeder as pre_feeder
from deepconsensus_amd.preprocess import read as read_lib
from deepconsensus_amd.preprocess import spacing_device as spd
from deepconsensus_amd.preprocess.windows import DcConfig
from deepconsensus_amd.utils import constants

from test_io_and_pipeline import make_test_bams

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HUMAN_1M_SKIP = 15  # as tests/test_featurize_device.py
M, I, D, N = (constants.CMATCH, constants.CINS, constants.CDEL,
              constants.CREF_SKIP)
KNOBS = ("DC_SPACING_MODE", "DC_PASSTHROUGH_MODE", "DC_FEATURIZE_MODE",
         "DC_STITCH_MODE")


def make_read(ops, rng, name="m/7/0", strand=constants.Strand.FORWARD,
              sn=(5.0, 6.0, 7.0, 8.0)):
    """An expanded subread from a per-element cigar op list: a base on M
    and I, a gap with pw = ip = 0 on D and N, as expand_clip_indent
    leaves them."""
    ops = np.asarray(ops, np.uint8)
    n = len(ops)
    has_base = (ops == M) | (ops == I)
    bases = np.full(n, constants.GAP, "<U1")
    bases[has_base] = rng.choice(list("ACGT"), size=int(has_base.sum()))
    pw = np.where(has_base, rng.integers(1, 256, n), 0).astype(np.uint8)
    ip = np.where(has_base, rng.integers(1, 256, n), 0).astype(np.uint8)
    ccs_idx = np.where(ops == I, -1, np.cumsum(ops != I) - 1)
    ccs_idx[~has_base] = -1
    return read_lib.Read(
        name=name, bases=bases, cigar=ops, pw=pw, ip=ip, sn=np.array(sn),
        strand=strand, ccs_idx=ccs_idx,
    )


def make_ccs(Lc, rng, quals=None):
    bases = rng.choice(list("ACGT"), size=Lc).astype("<U1")
    if quals is None:
        quals = rng.integers(1, 60, Lc)
    return read_lib.Read(
        name="m/7/ccs", bases=bases,
        cigar=np.repeat(np.uint8(M), Lc),
        pw=np.zeros(Lc, np.uint8), ip=np.zeros(Lc, np.uint8),
        sn=np.repeat(0, 4), strand=constants.Strand.UNKNOWN,
        base_quality_scores=np.asarray(quals), ccs_idx=np.arange(Lc),
        ec=12.0, np_num_passes=10, rq=0.999, rg="rg1",
    )


def random_ops(rng, Lc):
    """Inference read: indent, early end, leading / trailing insertion
    runs, deletions."""
    start = int(rng.integers(0, Lc)) if rng.random() < 0.4 else 0
    end = int(rng.integers(start + 1, Lc + 1)) if rng.random() < 0.4 else Lc
    ops = [N] * start
    if rng.random() < 0.3:
        ops += [I] * int(rng.integers(1, 4))
    for _ in range(start, end):
        ops.append(D if rng.random() < 0.1 else M)
        if rng.random() < 0.15:
            ops += [I] * int(rng.integers(1, 5))
    if rng.random() < 0.3:
        ops += [I] * int(rng.integers(1, 4))
    return ops


def random_zmw(seed, Lc=None, n_reads=None):
    rng = np.random.default_rng(9000 + seed)
    Lc = int(rng.integers(1, 60)) if Lc is None else Lc
    n_reads = int(rng.integers(1, 7)) if n_reads is None else n_reads
    reads = [
        make_read(random_ops(rng, Lc), rng, name=f"m/7/{i}",
                  strand=(constants.Strand.REVERSE if i % 2
                          else constants.Strand.FORWARD))
        for i in range(n_reads)
    ]
    return reads, make_ccs(Lc, rng)


@pytest.mark.parametrize("block", range(6))
def test_closed_form_equals_the_state_machine(block):
    """_seq_indices of every read (CCS row included) and the width."""
    for seed in range(block * 60, block * 60 + 60):  # 360 ZMWs
        reads, ccs = random_zmw(seed)
        counter = collections.Counter()
        u = spd.build_unspaced(reads, ccs, DcConfig(3, 25), None, counter)
        assert u is not None, (seed, counter)
        host = copy.deepcopy(reads + [ccs])
        for r in host:
            r.setup_spacing()
        width = read_lib._space_out_python(host)
        assert u.W == width, seed
        for r in host:
            np.testing.assert_array_equal(
                spd.column_of_elements(r.cigar, u.ins_max), r._seq_indices,
                err_msg=f"seed {seed} read {r.name}")


def _options(config, **kw):
    kw.setdefault("featurize_mode", "device")
    kw.setdefault("stitch_mode", "device")
    return qi.InferenceOptions(
        max_length=config.max_length, max_passes=config.max_passes,
        use_ccs_bq=config.use_ccs_bq,
        example_height=fd.tensor_height(config.max_passes,
                                        config.use_ccs_bq), **kw)


def _preprocess(zmw, config, options, mode, name="m/7/ccs"):
    reads, ccs = copy.deepcopy(zmw)
    options = dataclasses.replace(options, spacing_mode=mode)
    return qi.preprocess_one_zmw(
        (name, reads + [ccs], config, None, options))


def _packed(zmws, **kw):
    batch = fd.pack_batch(zmws, **kw)
    spd.space_batch_numpy(batch)
    return batch


def _assert_batches_equal(dev, host):
    for name in ("zmw_tab", "win_tab", "pt_tab", "sub", "ccs", "ccs_bq",
                 "ccs_q"):
        np.testing.assert_array_equal(
            getattr(dev, name), getattr(host, name), err_msg=name)
    assert dev.offsets == host.offsets
    assert dev.n_pt_bytes == host.n_pt_bytes
    assert dev.n_windows == host.n_windows


def _assert_zmw_equal(dev, host):
    np.testing.assert_array_equal(dev.window_pos, host.window_pos)
    assert dev.counter == host.counter
    assert (dev.planes is None) == (host.planes is None)
    assert [dataclasses.astuple(s) for s in dev.skipped] == [
        dataclasses.astuple(s) for s in host.skipped]
    if dev.planes is not None:
        for name in ("win_start", "win_w", "pt_start", "pt_w", "pt_width",
                     "pt_pos"):
            np.testing.assert_array_equal(
                getattr(dev.planes, name), getattr(host.planes, name),
                err_msg=name)


@pytest.mark.parametrize("passthrough", ["host", "device"])
@pytest.mark.parametrize("use_ccs_bq", [False, True])
@pytest.mark.parametrize("skip", [0, 30])
def test_unspaced_plus_twin_equals_host_planes(passthrough, use_ccs_bq,
                                               skip, monkeypatch):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    config = DcConfig(3, 25, use_ccs_bq)
    options = _options(config, skip_windows_above=skip,
                       passthrough_mode=passthrough)
    zmws = [random_zmw(seed, Lc=Lc) for seed, Lc in
            ((1, 1), (2, 37), (3, 130), (4, 77), (5, 25))]
    dev = [_preprocess(z, config, options, "device") for z in zmws]
    host = [_preprocess(z, config, options, "host") for z in zmws]
    assert all(getattr(z.planes, "unspaced", False)
               for z in dev if z.planes is not None)
    for d, h in zip(dev, host):
        _assert_zmw_equal(d, h)
    if skip:  # the threshold splits the windows
        assert sum(z.n_skipped for z in host) > 0
        assert sum(z.n_model for z in host) > 0
    _assert_batches_equal(_packed(dev), _packed(host))
    _assert_batches_equal(_packed(dev, pad_multiple=4),
                          _packed(host, pad_multiple=4))


def _hand_zmw(read_ops, Lc, seed=0):
    rng = np.random.default_rng(seed)
    reads = [
        make_read(ops, rng, name=f"m/7/{i}",
                  strand=(constants.Strand.REVERSE if i == 1
                          else constants.Strand.FORWARD))
        for i, ops in enumerate(read_ops)
    ]
    return reads, make_ccs(Lc, rng)


HAND_CASES = {
    "Lc_1": ([[M], [I, M, I, I]], 1),
    "leading_insertion_run": ([[I, I, M, M, M], [M, M, M]], 3),
    "trailing_run_in_a_read_that_ends_early": (
        [[M, M, I, I, I], [M, M, M, M, M, M]], 6),
    "indented_read": ([[N, N, N, M, I, M], [M, M, M, M, M]], 5),
    "deletion": ([[M, D, D, M, I, M], [M, M, M, M, M]], 5),
    "reverse_strand": ([[M, M, M], [M, I, M, M]], 3),
    "longest_run_in_a_dropped_read": (
        [[M, M, M, M], [M, I, M, M, M], [M, M, M, M],
         [M, I, I, I, I, M, M, M], [M, M, I, I, M, M]], 4),
    "no_insertions": ([[M, M, M, M], [N, M, D, M]], 4),
}


@pytest.mark.parametrize("case", sorted(HAND_CASES))
def test_hand_made_cases(case, monkeypatch):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    read_ops, Lc = HAND_CASES[case]
    config = DcConfig(3, 4, True)
    zmw = _hand_zmw(read_ops, Lc)
    if case == "longest_run_in_a_dropped_read":
        assert len(read_ops) > config.max_passes
    for passthrough, skip in (("host", 0), ("device", 1)):
        options = _options(config, skip_windows_above=skip,
                           passthrough_mode=passthrough)
        dev = _preprocess(zmw, config, options, "device")
        host = _preprocess(zmw, config, options, "host")
        assert getattr(dev.planes, "unspaced", False)
        _assert_zmw_equal(dev, host)
        _assert_batches_equal(_packed([dev]), _packed([host]))
    if case == "longest_run_in_a_dropped_read":
        kept = np.max([spd.insertion_runs(r.cigar, Lc) for r in zmw[0][:3]],
                      axis=0)
        assert dev.planes.ins_max.sum() > kept.sum()
    if case == "no_insertions":
        assert dev.planes.W == Lc and not dev.planes.ins_max.any()


def test_ins_trim_through_the_feeder(tmp_path, monkeypatch):
    """Real records, ins_trim > 0: the deferred job is expanded in the
    worker and ships unspaced."""
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    sub, ccs = make_test_bams(tmp_path, n_zmws=3, length=250, seed=11)
    config = DcConfig(20, 100, False)
    options = _options(config, skip_windows_above=27, ins_trim=2)
    feeder, _ = pre_feeder.create_proc_feeder(
        subreads_to_ccs=sub, ccs_bam=ccs, dc_config=config, ins_trim=2,
        defer_expansion=True)
    out = {}
    jobs = list(feeder())
    assert jobs
    for mode in ("host", "device"):
        o = dataclasses.replace(options, spacing_mode=mode)
        out[mode] = [
            qi.preprocess_one_zmw((zmw, copy.deepcopy(job), dcc, ww, o))
            for job, zmw, dcc, _, ww in jobs
        ]
    assert all(getattr(z.planes, "unspaced", False) for z in out["device"])
    for d, h in zip(out["device"], out["host"]):
        _assert_zmw_equal(d, h)
    _assert_batches_equal(_packed(out["device"]), _packed(out["host"]))


def _fallback_case(cause):
    reads, ccs = random_zmw(40, Lc=30, n_reads=3)
    widths = None
    if cause == "smart_windows":
        widths = np.array([10, 20])
    elif cause == "label":
        reads[1].truth_range = dict(contig="c", begin=0, end=5)
    elif cause == "empty_read":
        reads[2] = make_read([], np.random.default_rng(0))
    elif cause == "pw_ip_dtype":
        reads[0].pw = reads[0].pw.astype(np.int32)
    elif cause == "sn_shape":
        reads[0].sn = np.zeros(3)
    elif cause == "ccs_quality":
        ccs.base_quality_scores = ccs.base_quality_scores + 0.5
    elif cause == "past_ccs":
        reads[1] = make_read([M] * 31, np.random.default_rng(0))
    elif cause == "long_run":
        reads[1] = make_read([M] + [I] * (spd.MAX_RUN + 1),
                             np.random.default_rng(0))
    return reads, ccs, widths


@pytest.mark.parametrize("cause", spd.FALLBACK_CAUSES)
def test_each_fallback_cause_is_counted(cause):
    reads, ccs, widths = _fallback_case(cause)
    counter = collections.Counter()
    assert spd.build_unspaced(
        reads, ccs, DcConfig(3, 25), widths, counter) is None
    assert counter == {spd.fallback_counter(cause): 1}


def test_all_zero_qualities_fall_back():
    reads, ccs = random_zmw(41, Lc=12)
    ccs.base_quality_scores = np.zeros(12, np.int64)
    counter = collections.Counter()
    assert spd.build_unspaced(reads, ccs, DcConfig(3, 25), None,
                              counter) is None
    assert counter == {spd.fallback_counter("ccs_quality"): 1}


@pytest.mark.parametrize("device_planes", [False, True])
def test_mixed_batch_with_fallback_zmws(device_planes, monkeypatch):
    """Fallback ZMWs at the first, a middle and the last position: a read
    past the CCS end and pw not uint8 (both: host spacing, planes)."""
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    config = DcConfig(3, 25, True)
    options = _options(config, skip_windows_above=30,
                       passthrough_mode="device")
    zmws = [random_zmw(50 + i, Lc=40 + 7 * i) for i in range(5)]
    rng = np.random.default_rng(1)
    for i in (0, 4):
        Lc = len(zmws[i][1].bases)
        zmws[i][0][0] = make_read([M] * (Lc + 2), rng)
    zmws[2][0][0].pw = zmws[2][0][0].pw.astype(np.int16)
    dev = [_preprocess(z, config, options, "device") for z in zmws]
    host = [_preprocess(z, config, options, "host") for z in zmws]
    kinds = [getattr(z.planes, "unspaced", False) for z in dev]
    assert kinds == [False, True, False, True, False]
    for i in (0, 4):
        assert dev[i].counter[spd.fallback_counter("past_ccs")] == 1
        assert dev[i].planes is not None
    assert dev[2].counter[spd.fallback_counter("pw_ip_dtype")] == 1
    # put_spacing rebuilds pw as uint8, so this one ships planes as well.
    assert dev[2].planes is not None
    want = _packed(host)
    if not device_planes:
        got = _packed(dev)
        for name in ("zmw_tab", "win_tab", "pt_tab", "sub", "ccs",
                     "ccs_bq", "ccs_q"):
            np.testing.assert_array_equal(
                getattr(got, name), getattr(want, name), err_msg=name)
        return
    # Device planes: the region is left out of the blob; zero-filled by the
    # caller, host pieces copied in, twin run on it.
    got = fd.pack_batch(dev, device_planes=True)
    assert got.device_planes and got.sub.size == 0 and got.ccs.size == 0
    region = np.zeros(got.plane_nbytes, np.uint8)
    views = {}
    for name, (lo, dtype, count) in got.plane_layout.items():
        views[name] = region[
            lo : lo + count * np.dtype(dtype).itemsize].view(dtype)
    for name, off, array in got.host_planes:
        views[name][off : off + array.size] = array
    sp = got.spacing
    spd.space_planes_numpy(
        sp.src, sp.ins_max, sp.sp_tab, sp.read_tab, got.zmw_tab,
        views["sub"], views["ccs"], views["ccs_q"], views["ccs_bq"], True)
    for name in ("sub", "ccs", "ccs_bq", "ccs_q"):
        np.testing.assert_array_equal(
            views[name], getattr(want, name), err_msg=name)
    np.testing.assert_array_equal(got.zmw_tab, want.zmw_tab)


def _valid_tables(monkeypatch):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    config = DcConfig(3, 25, True)
    options = _options(config, skip_windows_above=30,
                       passthrough_mode="device")
    dev = [_preprocess(random_zmw(60 + i, Lc=30 + i), config, options,
                       "device") for i in range(3)]
    return fd.pack_batch(dev)


@pytest.mark.parametrize("violation", [
    "ins_off_past_the_end", "ccs_src_past_the_end", "read_off_past_the_end",
    "negative_read_length", "negative_Lc", "ins_max_sum", "zmw_index",
    "read_of_another_zmw",
])
def test_validator_rejects(violation, monkeypatch):
    batch = _valid_tables(monkeypatch)
    sp = batch.spacing
    sp_tab, read_tab = sp.sp_tab.copy(), sp.read_tab.copy()
    ins_max = sp.ins_max.copy()
    args = lambda: (sp_tab, read_tab, ins_max, len(sp.src),  # noqa: E731
                    batch.zmw_tab, len(batch.sub), len(batch.ccs))
    spd.validate_spacing_tables(*args())  # valid as packed
    if violation == "ins_off_past_the_end":
        sp_tab[2, spd.SP_INS_OFF] += 1
    elif violation == "ccs_src_past_the_end":
        sp_tab[2, spd.SP_CCS_SRC] += 1
    elif violation == "read_off_past_the_end":
        read_tab[-1, spd.RD_SRC] = len(sp.src) - 2
    elif violation == "negative_read_length":
        read_tab[1, spd.RD_N] = -3
    elif violation == "negative_Lc":
        sp_tab[1, spd.SP_LC] = -1
    elif violation == "ins_max_sum":
        ins_max[sp_tab[1, spd.SP_INS_OFF] + 2] += 1
    elif violation == "zmw_index":
        sp_tab[0, spd.SP_ZMW] = len(batch.zmw_tab)
    elif violation == "read_of_another_zmw":
        read_tab[0, spd.RD_SP] = 2
    with pytest.raises(ValueError, match="pack_spacing"):
        spd.validate_spacing_tables(*args())


def test_twin_with_a_corrupted_table_stays_inside_the_planes(monkeypatch):
    batch = _valid_tables(monkeypatch)
    sp = batch.spacing
    rng = np.random.default_rng(3)
    G = 64

    def guarded(a):
        g = G // a.itemsize
        full = np.empty(len(a) + 2 * g, a.dtype)
        full.view(np.uint8)[:] = 0xA5
        full[g : g + len(a)] = 0
        return full, full[g : g + len(a)]

    def intact(full, a):
        raw, g = full.view(np.uint8), G
        return (raw[:g] == 0xA5).all() and (raw[-g:] == 0xA5).all()

    corruptions = []
    for _ in range(40):
        sp_tab, read_tab = sp.sp_tab.copy(), sp.read_tab.copy()
        zmw_tab, ins_max = batch.zmw_tab.copy(), sp.ins_max.copy()
        kind = int(rng.integers(0, 4))
        value = int(rng.choice([-5, -1, 0, 1, 7, 10**6, 2**40]))
        if kind == 0:
            sp_tab[rng.integers(0, len(sp_tab)),
                   rng.integers(0, spd.SP_COLS)] = value
        elif kind == 1:
            read_tab[rng.integers(0, len(read_tab)),
                     rng.integers(0, spd.RD_COLS)] = value
        elif kind == 2:
            zmw_tab[rng.integers(0, len(zmw_tab)),
                    rng.integers(0, fd.TAB_FIXED)] = value
        else:
            ins_max[rng.integers(0, len(ins_max))] = 65535
        corruptions.append((sp_tab, read_tab, zmw_tab, ins_max))
    for sp_tab, read_tab, zmw_tab, ins_max in corruptions:
        outs = [guarded(a) for a in (batch.sub, batch.ccs, batch.ccs_q,
                                     batch.ccs_bq)]
        spd.space_planes_numpy(
            sp.src, ins_max, sp_tab, read_tab, zmw_tab,
            *(view for _, view in outs), True)
        assert all(intact(full, view) for full, view in outs)


def test_spacing_mode_resolution(monkeypatch):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    assert qi.SPACING_MODES == ("host", "device")
    assert qi.InferenceOptions().spacing_mode is None
    assert qi.resolve_spacing_mode(qi.InferenceOptions()) == "host"
    assert qi.resolve_spacing_mode(qi.InferenceOptions(
        spacing_mode="device", featurize_mode="device")) == "device"
    with pytest.raises(ValueError, match="spacing_mode"):
        qi.resolve_spacing_mode(qi.InferenceOptions(
            spacing_mode="gpu", featurize_mode="device"))
    for others in (dict(), dict(featurize_mode="host"),
                   dict(stitch_mode="device")):
        with pytest.raises(ValueError, match="needs featurize_mode"):
            qi.resolve_spacing_mode(
                qi.InferenceOptions(spacing_mode="device", **others))
        assert qi.resolve_spacing_mode(
            qi.InferenceOptions(spacing_mode="host", **others)) == "host"
    # Every combination stitch and passthrough mode already allow.
    for stitch in ("serial", "pool", "device"):
        assert qi.resolve_spacing_mode(qi.InferenceOptions(
            spacing_mode="device", featurize_mode="device",
            stitch_mode=stitch)) == "device"
    monkeypatch.setenv("DC_SPACING_MODE", "device")
    with pytest.raises(ValueError, match="needs featurize_mode"):
        qi.resolve_spacing_mode(qi.InferenceOptions())
    monkeypatch.setenv("DC_FEATURIZE_MODE", "device")
    assert qi.resolve_spacing_mode(qi.InferenceOptions()) == "device"
    assert qi.resolve_spacing_mode(
        qi.InferenceOptions(spacing_mode="host")) == "host"
    monkeypatch.setenv("DC_SPACING_MODE", "gpu")
    with pytest.raises(ValueError, match="spacing_mode"):
        qi.resolve_spacing_mode(qi.InferenceOptions())


def test_run_rejects_the_mode_before_any_worker_starts(tmp_path,
                                                       monkeypatch):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    started = []
    monkeypatch.setattr(
        pre_feeder, "create_proc_feeder",
        lambda **kw: started.append(kw) or (lambda: iter(()), {}))
    out = tmp_path / "out.fastq"
    for options in (qi.InferenceOptions(spacing_mode="device"),
                    qi.InferenceOptions(spacing_mode="gpu",
                                        featurize_mode="device")):
        with pytest.raises(ValueError, match="spacing_mode"):
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
    assert seen["options"].spacing_mode is None
    cli.main(base + ["--spacing_mode", "device", "--featurize_mode",
                     "device"])
    assert seen["options"].spacing_mode == "device"
    with pytest.raises(SystemExit):
        cli.main(base + ["--spacing_mode", "gpu"])


def _spy_unspaced(monkeypatch):
    seen = collections.Counter()
    real = fd.pack_batch

    def spy(zmws, **kw):
        for z in zmws:
            if getattr(z, "planes", None) is not None:
                kind = ("unspaced" if getattr(z.planes, "unspaced", False)
                        else "planes")
                seen[kind] += 1
        return real(zmws, **kw)

    monkeypatch.setattr(fd, "pack_batch", spy)
    return seen


MODE_COMBINATIONS = [
    dict(stitch_mode="serial"),
    dict(stitch_mode="device"),
    dict(stitch_mode="device", passthrough_mode="device"),
]


def _run_both(tmp_path, monkeypatch, sub, ccs, suffix, modes, limit=0,
              **kw):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    seen = _spy_unspaced(monkeypatch)
    outs, counters, kinds = {}, {}, {}
    for mode in ("host", "device"):
        seen.clear()
        torch.manual_seed(7)
        out = tmp_path / f"out_{mode}.{suffix}"
        options = qi.InferenceOptions(
            cpus=0, min_quality=0, featurize_mode="device",
            spacing_mode=mode, **modes, **kw)
        c = qi.run(subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
                   output=str(out), options=options, device="cpu",
                   limit=limit)
        outs[mode] = out.read_bytes()
        counters[mode] = dataclasses.asdict(c)
        kinds[mode] = dict(seen)
        with open(tmp_path / f"out_{mode}.inference.json") as f:
            outs[mode + "_stats"] = f.read()
    # A run that fell back to host spacing cannot pass.
    assert kinds["host"].get("unspaced", 0) == 0
    assert kinds["device"].get("planes", 0) == 0
    assert kinds["device"]["unspaced"] == kinds["host"]["planes"] > 0
    assert counters["host"] == counters["device"]
    assert counters["host"]["success"] > 0
    assert outs["host_stats"] == outs["device_stats"]
    assert outs["host"] and outs["device"] == outs["host"]


@pytest.mark.parametrize("modes", MODE_COMBINATIONS,
                         ids=["serial", "stitch", "stitch+passthrough"])
@pytest.mark.parametrize("suffix", ["fastq", "bam"])
def test_run_device_spacing_matches_host(tmp_path, monkeypatch, modes,
                                         suffix):
    sub, ccs = make_test_bams(tmp_path, n_zmws=4, length=350, seed=3)
    _run_both(tmp_path, monkeypatch, sub, ccs, suffix, modes,
              batch_size=4, batch_zmws=3, skip_windows_above=27)


@pytest.mark.parametrize("modes", MODE_COMBINATIONS[1:],
                         ids=["stitch", "stitch+passthrough"])
def test_run_device_spacing_matches_host_on_human_1m(tmp_path, monkeypatch,
                                                     modes):
    for name in ("subreads_to_ccs.bam", "ccs.bam"):
        parts = sorted(glob.glob(
            os.path.join(GOLDEN, "human_1m", name + ".part*")))
        srcs = parts or [os.path.join(GOLDEN, "human_1m", name)]
        with open(tmp_path / name, "wb") as dst:
            for src in srcs:
                with open(src, "rb") as f:
                    dst.write(f.read())
    _run_both(
        tmp_path, monkeypatch, str(tmp_path / "subreads_to_ccs.bam"),
        str(tmp_path / "ccs.bam"), "fastq", modes, batch_size=32,
        batch_zmws=2, skip_windows_above=HUMAN_1M_SKIP, ins_trim=5, limit=3,
    )


def test_worker_pool_ships_unspaced_zmws(tmp_path, monkeypatch):
    """cpus > 0 and the env knobs: ZmwUnspaced survives the pool pipe."""
    sub, ccs = make_test_bams(tmp_path, n_zmws=3, length=250, seed=5)
    for knob in KNOBS:
        monkeypatch.setenv(knob, "device")
    seen = _spy_unspaced(monkeypatch)
    outs = {}
    for mode, cpus in (("host", 0), (None, 2)):
        seen.clear()
        torch.manual_seed(7)
        out = tmp_path / f"out_{mode}.fastq"
        qi.run(subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
               output=str(out), device="cpu",
               options=qi.InferenceOptions(
                   batch_size=4, batch_zmws=2, cpus=cpus, min_quality=0,
                   skip_windows_above=27, spacing_mode=mode))
        outs[mode] = out.read_bytes()
    assert seen["unspaced"] > 0 and seen["planes"] == 0
    assert outs["host"] and outs["host"] == outs[None]
