"""alignment_calib.hip (window QV calibration on device) against its
numpy twin, against K14 on left-shifted inputs, and through `eval`."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from deepconsensus_amd.calibration import window_calibration as wc
from deepconsensus_amd.models import config as cfg
from deepconsensus_amd.models import losses as losses_lib

import calib_cases

pytestmark = pytest.mark.gpu

# 63/64/65: wave boundary of the in-kernel compaction; 129: its 128-lane
# chunk boundary; 158: the largest accepted window.
LENGTHS = (1, 2, 63, 64, 65, 100, 129, 158)
BATCHES = (1, 3, 48)


@functools.lru_cache(maxsize=None)
def _case(length, b):
    """Inputs and the twin's answer, computed once and left unchanged."""
    label, bases, quals = calib_cases.make_pairs(
        1000 * length + b, b, length
    )
    ref = wc.window_calibration_numpy(label, bases, quals)
    for a in (label, bases, quals, ref[0], ref[2], ref[3]):
        a.setflags(write=False)
    return label, bases, quals, ref


def _ext():
    from deepconsensus_amd import ops as dc_ops

    return dc_ops.get_ext(required=True)


def _device_raw(label, bases, quals):
    m = losses_lib.AlignmentMetric()
    out = _ext().alignment_calib(
        torch.tensor(label).cuda(), torch.tensor(bases).cuda(),
        torch.tensor(quals).cuda(),
        m.matching_score, m.mismatch_penalty,
        m.gap_open_penalty, m.gap_extend_penalty,
    )
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("b", BATCHES)
@pytest.mark.parametrize("length", LENGTHS)
def test_kernel_matches_twin(length, b):
    label, bases, quals, (v_ref, mv_ref, cls_ref, hist_ref) = _case(length, b)
    v, counts, cls, hist = _device_raw(label, bases, quals)
    assert v.dtype == torch.float32 and counts.dtype == torch.int32
    assert cls.dtype == torch.uint8 and hist.dtype == torch.int64
    assert hist.shape == (100, 2) and cls.shape == (b, length)
    counts = counts.cpu().numpy()
    for col, key in enumerate(("num_matches", "num_insertions",
                               "num_deletions", "num_correct_matches")):
        np.testing.assert_array_equal(counts[:, col], mv_ref[key],
                                      err_msg=key)
    np.testing.assert_array_equal(cls.cpu().numpy(), cls_ref)
    np.testing.assert_array_equal(hist.cpu().numpy(), hist_ref)
    # Every score is a small integer: fp32 and fp64 agree exactly.
    np.testing.assert_array_equal(
        v.cpu().numpy().astype(np.float64), v_ref
    )


def test_dispatch_runs_the_kernel_for_cuda_tensors():
    label, bases, quals, (v_ref, mv_ref, cls_ref, hist_ref) = _case(100, 48)
    v, mv, cls, hist = wc.window_calibration(
        torch.tensor(label).cuda(), torch.tensor(bases).cuda(),
        torch.tensor(quals).cuda(),
    )
    np.testing.assert_array_equal(v, v_ref)
    np.testing.assert_array_equal(cls, cls_ref)
    np.testing.assert_array_equal(hist, hist_ref)
    for key, val in mv_ref.items():
        np.testing.assert_array_equal(mv[key], val, err_msg=key)


@pytest.mark.parametrize("length", (65, 100, 158))
def test_counts_and_v_opt_equal_k14_on_left_shifted_inputs(length):
    label, bases, quals, _ = _case(length, 48)
    v, counts, _, _ = _device_raw(label, bases, quals)
    yt = losses_lib.left_shift_sequence(
        torch.tensor(label).cuda().long()
    ).int()
    yp = losses_lib.left_shift_sequence(
        torch.tensor(bases).cuda().long()
    ).int()
    m = losses_lib.AlignmentMetric()
    v14, counts14 = _ext().alignment_metric_counts(
        yt, yp, (yt != 0).sum(-1).int(), (yp != 0).sum(-1).int(),
        m.matching_score, m.mismatch_penalty,
        m.gap_open_penalty, m.gap_extend_penalty,
    )
    assert torch.equal(counts, counts14)
    assert torch.equal(v, v14)


def test_too_long_window_raises():
    z = torch.zeros((2, 159), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="too long"):
        _ext().alignment_calib(z, z, z, 2.0, 5.0, 9.0, 4.0)


def test_wrong_dtype_or_shape_raises():
    z = torch.zeros((2, 10), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        _ext().alignment_calib(z.int(), z, z, 2.0, 5.0, 9.0, 4.0)
    with pytest.raises(RuntimeError):
        _ext().alignment_calib(z, z[:, :5], z, 2.0, 5.0, 9.0, 4.0)


def test_hist_is_reproducible():
    label, bases, quals, _ = _case(100, 48)
    h1 = _device_raw(label, bases, quals)[3]
    h2 = _device_raw(label, bases, quals)[3]
    assert torch.equal(h1, h2)


def test_second_call_into_accumulator_doubles_hist():
    label, bases, quals, (_, _, _, hist_ref) = _case(100, 48)
    names = np.array([f"m/{i % 5}/ccs" for i in range(48)])
    args = (names, np.arange(48), torch.tensor(label).cuda(),
            torch.tensor(bases).cuda(), torch.tensor(quals).cuda())
    acc = wc.WindowCalibrationAccumulator()
    acc.update(*args)
    assert acc.backend == "device"
    np.testing.assert_array_equal(acc.hist, hist_ref)
    once = {k: list(v) for k, v in acc.molecules.items()}
    acc.update(*args)
    np.testing.assert_array_equal(acc.hist, 2 * hist_ref)
    assert acc.molecules == {k: [2 * x for x in v] for k, v in once.items()}


def test_eval_cuda_alignment_layer_matches_twin(tmp_path, monkeypatch):
    """`eval --device cuda` with the flags: the (bases, quals) the runner
    produced on the GPU, fed to the twin on the host, give the same CSVs
    and JSON counts as the device run. Only the alignment layer is under
    test; native and torch model paths are not compared."""
    from deepconsensus_amd.models import infer_eval

    corpus, _ = calib_cases.build_corpus(str(tmp_path / "corpus"))
    params = cfg.get_config("transformer_learn_values+custom")
    params.batch_size = 16
    cfg.modify_params(params, is_training=False)

    host_model = wc.WindowCalibrationAccumulator()
    host_ccs = wc.WindowCalibrationAccumulator()
    natives = []
    real_update = infer_eval.EmqEvaluator.update

    def recording_update(self, batch, rows, label):
        bases, quals = real_update(self, batch, rows, label)
        natives.append(self.runner.native)
        name, pos = batch["name"], batch["window_pos"]
        lab = label.cpu().numpy().astype(np.uint8)
        host_model.update(name, pos, lab, bases.cpu().numpy(),
                          quals.cpu().numpy())
        ccs_bases = rows[:, 4 * params.max_passes, :].cpu().numpy()
        ccs_quals = np.clip(batch["ccs_base_quality_scores"], 0, 255)
        host_ccs.update(name, pos, lab, ccs_bases.astype(np.uint8),
                        ccs_quals.astype(np.uint8))
        return bases, quals

    monkeypatch.setattr(infer_eval.EmqEvaluator, "update", recording_update)
    out = str(tmp_path / "out")
    cal = os.path.join(out, "calibration.csv")
    yj = os.path.join(out, "yield.json")
    torch.manual_seed(5)
    infer_eval.run_inference(
        out, "random", [corpus], params=params, device="cuda",
        calibration_csv=cal, yield_json=yj,
        dc_calibration="0,1.197654,-0.99781",
    )
    assert natives and all(natives)
    assert host_model.backend == "numpy" and host_ccs.backend == "numpy"

    host_model.write_csv(str(tmp_path / "host.csv"))
    host_ccs.write_csv(str(tmp_path / "host.ccs.csv"))
    assert open(cal).read() == open(str(tmp_path / "host.csv")).read()
    assert (open(infer_eval.ccs_path(cal)).read()
            == open(str(tmp_path / "host.ccs.csv")).read())
    result = json.load(open(yj))
    assert result["backend"] == "device"
    for key, acc in (("model", host_model), ("ccs", host_ccs)):
        host = acc.yield_metrics((20, 30, 40))
        assert host["table_bases"] > 0
        for k, v in host.items():
            assert result[key][k] == v, (key, k)
