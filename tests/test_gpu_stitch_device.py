"""GPU tests for device-side window stitching: the stitch_compact kernel
against its numpy twin, and the device stitch path of `run` against the
serial Python stitcher on the same runner."""
import collections
import dataclasses
import io

import numpy as np
import pytest
import torch

from deepconsensus_amd.postprocess import stitch, stitch_device

from test_io_and_pipeline import make_test_bams

pytestmark = pytest.mark.gpu

_LENGTHS = [0, 1, 63, 64, 65, 100, 128, 257]
_GUARD = 64


@pytest.fixture(scope="module")
def ext():
    from deepconsensus_amd import ops

    return ops.get_ext(required=True)


def _table(n_seg, seed, all_gap=False):
    """Source buffers + a segment table mixing every length in _LENGTHS,
    odd offsets, slack bytes between segments, and all-gap / no-gap
    segments next to each other."""
    rng = np.random.default_rng(seed)
    seg_len = np.array(
        [_LENGTHS[(i + seed) % len(_LENGTHS)] for i in range(n_seg)]
    )
    if n_seg == 1:
        seg_len[:] = 257
    slack = rng.integers(0, 4, n_seg)
    seg_off = 3 + np.cumsum(seg_len + slack) - seg_len
    n_src = int(seg_off[-1] + seg_len[-1] + 5)
    bases = rng.integers(0, 5, n_src).astype(np.uint8)
    quals = rng.integers(0, 94, n_src).astype(np.uint8)
    for i in range(n_seg):
        lo, hi = seg_off[i], seg_off[i] + seg_len[i]
        if all_gap or i % 5 == 1:
            bases[lo:hi] = 0
        elif i % 5 == 2:
            bases[lo:hi] = rng.integers(1, 5, hi - lo)
    # Output order is not source order.
    perm = rng.permutation(n_seg)
    return (bases, quals, seg_off[perm].astype(np.int32),
            seg_len[perm].astype(np.int32))


def _guarded(n, dtype):
    """A view of n elements followed by _GUARD bytes of 0xA5."""
    item = torch.empty(0, dtype=dtype).element_size()
    big = torch.full((n * item + _GUARD,), 0xA5, dtype=torch.uint8,
                     device="cuda")
    return big, big[: n * item].view(dtype)


def _launch_guarded(ext, bases, quals, seg_off, seg_len, n_kept):
    n_seg = len(seg_off)
    # One leading byte makes the source pointers odd.
    src = torch.from_numpy(np.stack([
        np.concatenate([[7], bases]), np.concatenate([[7], quals])
    ]).astype(np.uint8)).cuda()
    bufs = [_guarded(n_kept, torch.uint8), _guarded(n_kept, torch.uint8),
            _guarded(n_seg, torch.int32), _guarded(n_seg + 1, torch.int32)]
    total = ext.stitch_compact_into(
        src[0, 1:], src[1, 1:],
        torch.from_numpy(seg_off).cuda(), torch.from_numpy(seg_len).cuda(),
        *[view for _, view in bufs],
    )
    torch.cuda.synchronize()
    assert total == n_kept
    for big, _ in bufs:
        assert (big[-_GUARD:] == 0xA5).all().item()
    return [view.cpu().numpy() for _, view in bufs]


@pytest.mark.parametrize("n_seg", [1, 5, 300])
def test_kernel_matches_numpy_twin(ext, n_seg):
    bases, quals, seg_off, seg_len = _table(n_seg, seed=n_seg)
    want = stitch_device.compact_segments_numpy(
        bases, quals, seg_off, seg_len
    )
    assert want[3][-1] > 0
    got = _launch_guarded(ext, bases, quals, seg_off, seg_len,
                          int(want[3][-1]))
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    # The allocating entry point gives the same four outputs, twice.
    dev = [torch.from_numpy(a).cuda()
           for a in (bases, quals, seg_off, seg_len)]
    first = ext.stitch_compact(*dev)
    second = ext.stitch_compact(*dev)
    for a, b, w in zip(first, second, want):
        assert torch.equal(a, b)
        assert np.array_equal(a.cpu().numpy(), w)


def test_kernel_table_with_nothing_kept(ext):
    bases, quals, seg_off, seg_len = _table(9, seed=2, all_gap=True)
    want = stitch_device.compact_segments_numpy(
        bases, quals, seg_off, seg_len
    )
    assert want[3][-1] == 0 and not want[2].any()
    got = _launch_guarded(ext, bases, quals, seg_off, seg_len, 0)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    seq_out, qual_out, seg_kept, out_off = ext.stitch_compact(
        *[torch.from_numpy(a).cuda()
          for a in (bases, quals, seg_off, seg_len)]
    )
    assert seq_out.numel() == 0 and qual_out.numel() == 0
    assert not out_off.cpu().numpy().any()


def test_kernel_rejects_bad_arguments(ext):
    u8 = torch.zeros(8, dtype=torch.uint8, device="cuda")
    i32 = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="uint8"):
        ext.stitch_compact(u8.int(), u8, i32, i32)
    with pytest.raises(RuntimeError, match="int32"):
        ext.stitch_compact(u8, u8, i32.long(), i32)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.stitch_compact(u8[::2], u8[::2], i32, i32)
    with pytest.raises(RuntimeError, match="device"):
        ext.stitch_compact(u8.cpu(), u8, i32, i32)


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


def _rows(rng, n, params):
    rows = np.zeros((n, params.total_rows, params.max_length), np.int16)
    mp = params.max_passes
    rows[:, 0:mp] = rng.integers(0, 5, (n, mp, params.max_length))
    rows[:, mp:3 * mp] = rng.integers(0, 256, (n, 2 * mp, params.max_length))
    rows[:, 3 * mp:4 * mp] = rng.integers(0, 3, (n, mp, params.max_length))
    rows[:, 4 * mp] = rng.integers(0, 5, (n, params.max_length))
    rows[:, -4:] = rng.integers(3, 30, (n, 4, 1))
    return rows


def test_runner_path_matches_serial_stitch(runner):
    """3 hand-built ZMWs, 12 model windows at batch_size 5: the windows of
    one ZMW come from two replays of the graph, whose output buffer the
    second replay overwrites. One overflow passthrough (137 bases), one
    ZMW with a missing window."""
    from deepconsensus_amd.inference import quick_inference as qi

    rng = np.random.default_rng(5)
    vocab = np.frombuffer(b" ATCG", np.uint8)
    passthrough = stitch.DCModelOutput(
        molecule_name="m0/12/ccs", window_pos=300,
        sequence=vocab[rng.integers(0, 5, 137)].tobytes().decode("ascii"),
        quality_string="".join(
            chr(33 + q) for q in rng.integers(0, 94, 137)),
        ec=3.0, np_num_passes=3, rq=0.9, rg="rg",
    )
    layout = [
        ("m0/12/ccs", [0, 100, 200], [passthrough]),
        ("m0/9/ccs", [0, 100, 200, 300, 400], []),
        ("m0/100/ccs", [0, 200, 300, 400], []),  # window 100 is missing
    ]
    zmws = [
        qi.ZmwWindows(
            name=name, window_pos=np.asarray(pos, np.int64),
            rows=_rows(rng, len(pos), runner.params), skipped=skipped,
            counter=collections.Counter(), ec=1.5, np_num_passes=4,
            rq=0.99, rg="rg0",
        )
        for name, pos, skipped in layout
    ]
    options = qi.InferenceOptions(batch_size=5, min_quality=0)

    want_counter, want = stitch.OutcomeCounter(), io.StringIO()
    qi._write_outputs(
        qi.run_model_on_zmws(zmws, runner, options), want, None, options,
        want_counter,
    )
    got_counter, got = stitch.OutcomeCounter(), io.StringIO()
    stitched = qi.run_model_and_stitch_on_zmws(zmws, runner, options)
    assert (stitched.n_model, stitched.n_skipped) == (12, 1)
    qi._write_stitched(stitched, got, None, options, got_counter)

    assert want_counter.empty_sequence == 1 and want_counter.total == 3
    assert "@m0/12/ccs" in want.getvalue()
    assert got.getvalue() == want.getvalue()
    assert dataclasses.asdict(got_counter) == dataclasses.asdict(
        want_counter)


def test_run_device_mode_matches_serial_on_gpu(tmp_path):
    from deepconsensus_amd.inference import quick_inference as qi

    sub, ccs = make_test_bams(tmp_path, n_zmws=4, length=300)
    outs, counters = {}, {}
    for mode in ("serial", "device"):
        torch.manual_seed(7)
        out = tmp_path / f"out_{mode}.fastq"
        options = qi.InferenceOptions(
            batch_size=64, batch_zmws=2, cpus=0, min_quality=0,
            skip_windows_above=0, stitch_mode=mode,
        )
        counters[mode] = dataclasses.asdict(qi.run(
            subreads_to_ccs=sub, ccs_bam=ccs, checkpoint="random",
            output=str(out), options=options, device="cuda",
        ))
        outs[mode] = out.read_bytes()
    assert counters["serial"]["success"] == 4
    assert counters["serial"] == counters["device"]
    assert outs["serial"] and outs["serial"] == outs["device"]
