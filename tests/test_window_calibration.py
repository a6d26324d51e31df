"""Window-level QV calibration and emQ yield (CPU): the numpy twin
against hand cases, against the `calibrate` tool's cigar walk and against
AlignmentMetric; the accumulator, the linear fit and `eval` end to end."""
import json
import os
import types

import numpy as np
import pytest
import torch

from deepconsensus_amd.calibration import calculate_baseq_calibration as cbc
from deepconsensus_amd.calibration import calibration as calibration_lib
from deepconsensus_amd.calibration import window_calibration as wc
from deepconsensus_amd.models import config as cfg
from deepconsensus_amd.models import losses as losses_lib
from deepconsensus_amd.utils import constants

import calib_cases

VOCAB = " ATCG"


def _u8(*rows):
    return np.array(rows, dtype=np.uint8)


def _table(entries):
    hist = np.zeros((100, 2), dtype=np.int64)
    for q, col, n in entries:
        hist[q, col] += n
    return hist


# --------------------------------------------------------------------------
# Hand cases with a unique optimal alignment.
# --------------------------------------------------------------------------


def test_identical_pair_all_match_at_own_bin():
    label = _u8([1, 0, 2, 3, 0, 4, 1, 2])
    quals = _u8([10, 77, 11, 12, 78, 13, 10, 99])
    v, mv, cls, hist = wc.window_calibration_numpy(label, label, quals)
    np.testing.assert_array_equal(cls, _u8([1, 0, 1, 1, 0, 1, 1, 1]))
    np.testing.assert_array_equal(
        hist, _table([(10, 0, 2), (11, 0, 1), (12, 0, 1), (13, 0, 1),
                      (99, 0, 1)])
    )
    assert v[0] == 6 * 2.0
    assert mv["num_correct_matches"][0] == 6
    assert mv["alignment_length"][0] == 6


def test_one_substitution_is_one_mismatch_at_its_bin():
    label = _u8([1, 2, 3, 4, 1, 2, 3, 4])
    bases = label.copy()
    bases[0, 3] = 1
    quals = _u8([30, 31, 32, 7, 34, 35, 36, 37])
    _, mv, cls, hist = wc.window_calibration_numpy(label, bases, quals)
    np.testing.assert_array_equal(cls, _u8([1, 1, 1, 2, 1, 1, 1, 1]))
    expect = _table([(q, 0, 1) for q in (30, 31, 32, 34, 35, 36, 37)]
                    + [(7, 1, 1)])
    np.testing.assert_array_equal(hist, expect)
    assert mv["num_matches"][0] == 8 and mv["num_correct_matches"][0] == 7


def test_window_coordinates_survive_different_gap_layouts():
    # Same sequences, gaps in different columns: classes land on the
    # prediction's own columns.
    label = _u8([0, 1, 2, 0, 3, 4, 0, 0])
    bases = _u8([1, 0, 0, 2, 0, 3, 0, 4])
    quals = _u8([1, 50, 50, 2, 50, 3, 50, 4])
    _, _, cls, hist = wc.window_calibration_numpy(label, bases, quals)
    np.testing.assert_array_equal(cls, _u8([1, 0, 0, 1, 0, 1, 0, 1]))
    np.testing.assert_array_equal(
        hist, _table([(1, 0, 1), (2, 0, 1), (3, 0, 1), (4, 0, 1)])
    )


def test_inserted_base_is_class_three_and_a_mismatch():
    label = _u8([1, 2, 3, 4, 1, 2, 3, 0])
    bases = _u8([1, 2, 3, 3, 4, 1, 2, 3])  # extra 3 inside a 3-run
    quals = _u8([20, 20, 21, 22, 20, 20, 20, 20])
    _, mv, cls, hist = wc.window_calibration_numpy(label, bases, quals)
    assert mv["num_insertions"][0] == 1 and mv["num_correct_matches"][0] == 7
    assert sorted(cls[0].tolist()) == [1] * 7 + [3]
    assert cls[0, 2] + cls[0, 3] == 4  # one of the two 3s is the insertion
    assert hist[:, 1].sum() == 1 and hist[:, 0].sum() == 7


@pytest.mark.parametrize("label_row, bases_row", [
    ([1, 2, 3, 4], [0, 0, 0, 0]),   # prediction empty
    ([0, 0, 0, 0], [0, 0, 0, 0]),   # both empty
])
def test_empty_prediction_gives_empty_table(label_row, bases_row):
    quals = _u8([5, 6, 7, 8])
    _, mv, cls, hist = wc.window_calibration_numpy(
        _u8(label_row), _u8(bases_row), quals
    )
    assert hist.sum() == 0
    assert not cls.any()
    assert mv["num_matches"][0] == 0 and mv["num_insertions"][0] == 0


def test_empty_truth_charges_every_base_as_insertion():
    _, mv, cls, hist = wc.window_calibration_numpy(
        _u8([0, 0, 0, 0]), _u8([1, 0, 2, 3]), _u8([5, 6, 7, 100])
    )
    np.testing.assert_array_equal(cls, _u8([3, 0, 3, 3]))
    np.testing.assert_array_equal(hist, _table([(5, 1, 1), (7, 1, 1)]))
    assert mv["num_insertions"][0] == 3


def test_all_gap_row_in_a_batch_is_all_zero():
    label = _u8([1, 2, 3, 4], [0, 0, 0, 0])
    _, _, cls, _ = wc.window_calibration_numpy(
        label, label, _u8([1, 2, 3, 4], [9, 9, 9, 9])
    )
    np.testing.assert_array_equal(cls, _u8([1, 1, 1, 1], [0, 0, 0, 0]))


def test_quality_bin_edges():
    label = _u8([1, 2, 3, 4])
    _, _, cls, hist = wc.window_calibration_numpy(
        label, label, _u8([0, 99, 100, 255])
    )
    np.testing.assert_array_equal(cls, _u8([1, 1, 1, 1]))
    np.testing.assert_array_equal(hist, _table([(0, 0, 1), (99, 0, 1)]))


# --------------------------------------------------------------------------
# Twin against the `calibrate` tool's cigar walk.
# --------------------------------------------------------------------------


def _cigar_from_path(path, yt, yp):
    """Walks AlignmentMetric's path matrix back from (len(yt), len(yp))."""
    i, j = len(yt), len(yp)
    ops = []
    while True:
        edge = path[i, j]
        if edge == 1:
            ops.append(constants.CEQUAL if yt[i - 1] == yp[j - 1]
                       else constants.CDIFF)
            i, j = i - 1, j - 1
        elif edge in (2, 3):
            ops.append(constants.CINS)
            j -= 1
        elif edge in (4, 5):
            ops.append(constants.CDEL)
            i -= 1
        else:
            break
    assert (i, j) == (0, 0)
    ops.reverse()
    cigar = []
    for op in ops:
        if cigar and cigar[-1][0] == op:
            cigar[-1][1] += 1
        else:
            cigar.append([op, 1])
    return [tuple(c) for c in cigar]


def test_twin_matches_calibrate_cigar_walk():
    label, bases, quals = calib_cases.make_pairs(23, 40, 100)
    metric = losses_lib.AlignmentMetric()
    onehot = np.eye(constants.SEQ_VOCAB_SIZE, dtype=np.float32)[bases]
    _, paths, _ = metric.alignment(label, onehot)
    skip = calibration_lib.parse_calibration_string("skip")
    total = np.zeros((100, 2), dtype=np.int64)
    for r in range(label.shape[0]):
        yt = label[r][label[r] != 0]
        keep = bases[r] != 0
        yp = bases[r][keep]
        read = types.SimpleNamespace(
            flag=0, is_unmapped=False, is_supplementary=False, mapq=60,
            reference_start=0,
            query_qualities=quals[r][keep].astype(np.int64),
            query_sequence="".join(VOCAB[t] for t in yp),
            cigartuples=_cigar_from_path(paths[r], yt, yp),
        )
        counts = cbc.get_quality_calibration_stats(
            [read], "".join(VOCAB[t] for t in yt),
            cbc.RegionRecord("truth", 0, len(yt)), 0, skip,
        )
        total += np.array([[c["M"], c["X"]] for c in counts])
    _, _, _, hist = wc.window_calibration_numpy(label, bases, quals, metric)
    assert total.sum() > 1000
    np.testing.assert_array_equal(hist, total)


# --------------------------------------------------------------------------
# Invariants on random pairs.
# --------------------------------------------------------------------------


def test_invariants_on_random_pairs():
    label, bases, quals = calib_cases.make_pairs(31, 200, 100, max_q=99)
    metric = losses_lib.AlignmentMetric()
    v, mv, cls, hist = wc.window_calibration_numpy(label, bases, quals, metric)
    assert hist[:, 0].sum() == mv["num_correct_matches"].sum()
    assert hist[:, 1].sum() == (
        mv["num_matches"] - mv["num_correct_matches"] + mv["num_insertions"]
    ).sum()
    assert not cls[bases == 0].any()
    assert cls.max() <= 3
    onehot = np.eye(constants.SEQ_VOCAB_SIZE, dtype=np.float32)[bases]
    v_ref, _, mv_ref = metric.alignment(label, onehot)
    np.testing.assert_array_equal(v, v_ref)
    for k, val in mv_ref.items():
        np.testing.assert_array_equal(mv[k], val, err_msg=k)
    # Per row: every emitted base is classified exactly once.
    np.testing.assert_array_equal(
        (cls != 0).sum(1), mv["num_matches"] + mv["num_insertions"]
    )
    np.testing.assert_array_equal((cls == 1).sum(1),
                                  mv["num_correct_matches"])
    np.testing.assert_array_equal((cls == 3).sum(1), mv["num_insertions"])


def test_dispatch_uses_twin_for_host_tensors():
    label, bases, quals = calib_cases.make_pairs(2, 6, 30)
    ref = wc.window_calibration_numpy(label, bases, quals)
    got = wc.window_calibration(
        torch.from_numpy(label), torch.from_numpy(bases),
        torch.from_numpy(quals),
    )
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[2], ref[2])
    np.testing.assert_array_equal(got[3], ref[3])


# --------------------------------------------------------------------------
# Accumulator.
# --------------------------------------------------------------------------


def test_accumulator_split_batches_equal_one_batch():
    label, bases, quals = calib_cases.make_pairs(41, 12, 50)
    names = np.array(["m/1/ccs"] * 5 + ["m/2/ccs"] * 7)
    pos = np.arange(12) * 50
    one = wc.WindowCalibrationAccumulator()
    one.update(names, pos, label, bases, quals)
    two = wc.WindowCalibrationAccumulator()
    two.update(names[:3], pos[:3], label[:3], bases[:3], quals[:3])
    two.update(names[3:], pos[3:], label[3:], bases[3:], quals[3:])
    np.testing.assert_array_equal(one.hist, two.hist)
    assert one.molecules == two.molecules
    assert one.yield_metrics() == two.yield_metrics()
    assert one.backend == "numpy"


def _windows_with_errors(rng, n_windows, n_errors, length=100):
    """n_windows full windows; the first n_errors carry one substitution."""
    label = rng.integers(1, 5, size=(n_windows, length)).astype(np.uint8)
    bases = label.copy()
    for r in range(n_errors):
        bases[r, 50] = label[r, 50] % 4 + 1
    return label, bases


def test_emq_thresholds_at_exact_identities():
    rng = np.random.default_rng(7)
    acc = wc.WindowCalibrationAccumulator()
    quals = np.full((10, 100), 40, dtype=np.uint8)
    # identity 0.99: 100 bases, one substitution.
    label, bases = _windows_with_errors(rng, 1, 1)
    acc.update(["q20"], [0], label, bases, quals[:1])
    # identity 0.999: 1000 bases in ten windows, one substitution.
    label, bases = _windows_with_errors(rng, 10, 1)
    acc.update(["q30"] * 10, np.arange(10) * 100, label, bases, quals)
    # identity 1.0.
    label, bases = _windows_with_errors(rng, 2, 0)
    acc.update(["perfect"] * 2, [0, 100], label, bases, quals[:2])
    # identity 0.98: below every threshold.
    label, bases = _windows_with_errors(rng, 1, 0)
    bases[0, 10] = label[0, 10] % 4 + 1
    bases[0, 80] = label[0, 80] % 4 + 1
    acc.update(["q17"], [0], label, bases, quals[:1])
    assert acc.molecules["q20"] == [99, 100, 100]
    assert acc.molecules["q30"] == [999, 1000, 1000]
    assert acc.molecules["perfect"] == [200, 200, 200]
    assert acc.molecules["q17"] == [98, 100, 100]
    y = acc.yield_metrics((20, 30, 40))
    assert y["yield@emQ20"] == 100 + 1000 + 200
    assert y["yield@emQ30"] == 1000 + 200
    assert y["yield@emQ40"] == 200
    assert y["n_molecules"] == 4 and y["n_molecules_empty"] == 0
    assert y["emitted_bases"] == 1400 == y["table_bases"]
    assert wc.empirical_quality(200, 200) == float("inf")
    assert abs(wc.empirical_quality(99, 100) - 20.0) < 1e-9


def test_empty_molecule_is_counted_not_divided_by():
    acc = wc.WindowCalibrationAccumulator()
    zeros = np.zeros((1, 20), dtype=np.uint8)
    acc.update([b"empty"], [0], zeros, zeros, zeros)
    y = acc.yield_metrics()
    assert y["n_molecules"] == 1 and y["n_molecules_empty"] == 1
    assert y["yield@emQ20"] == y["yield@emQ30"] == y["yield@emQ40"] == 0


def test_write_csv_is_calibrate_format(tmp_path):
    label, bases, quals = calib_cases.make_pairs(43, 8, 40)
    acc = wc.WindowCalibrationAccumulator()
    acc.update(["a"] * 8, np.arange(8), label, bases, quals)
    path = str(tmp_path / "cal.csv")
    acc.write_csv(path)
    lines = open(path).read().split("\n")
    assert lines[0] == "baseq,total_match,total_mismatch"
    assert lines[-1] == "" and len(lines) == 102
    rows = np.array([[int(x) for x in ln.split(",")] for ln in lines[1:101]])
    np.testing.assert_array_equal(rows[:, 0], np.arange(100))
    np.testing.assert_array_equal(rows[:, 1:], acc.hist)


# --------------------------------------------------------------------------
# Linear fit.
# --------------------------------------------------------------------------


def test_fit_recovers_planted_line():
    w, b = 0.75, 2.5
    # Exactly linear table: X/(M+X) = 10^-(w q + b)/10, kept as floats so
    # that no rounding of the counts bends the line.
    hist = np.zeros((100, 2), dtype=np.float64)
    for q in range(10, 50, 4):
        total = 1e9 * (1 + q % 3)
        x = total * 10.0 ** (-(w * q + b) / 10.0)
        hist[q] = (total - x, x)
    fit = wc.fit_linear_calibration(hist, min_count=100)
    vals = calibration_lib.parse_calibration_string(fit)
    assert vals.enabled and vals.threshold == 0
    assert abs(vals.w - w) < 1e-9
    assert abs(vals.b - b) < 1e-9


def test_fit_needs_two_bins():
    hist = np.zeros((100, 2), dtype=np.int64)
    assert wc.fit_linear_calibration(hist) is None
    hist[30] = (9990, 10)
    assert wc.fit_linear_calibration(hist, min_count=100) is None
    hist[40] = (50, 1)       # below min_count
    hist[41] = (10000, 0)    # no mismatch: no finite empirical quality
    assert wc.fit_linear_calibration(hist, min_count=100) is None
    hist[20] = (990, 10)
    assert wc.fit_linear_calibration(hist, min_count=100) is not None


# --------------------------------------------------------------------------
# `eval` end to end on the CPU.
# --------------------------------------------------------------------------


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("calib_corpus")
    return calib_cases.build_corpus(str(tmp))[0]


def _eval_params():
    params = cfg.get_config("transformer_learn_values+custom")
    params.batch_size = 16
    cfg.modify_params(params, is_training=False)
    return params


def _parent_inference_csv(eval_path, params, seed):
    """What `eval` wrote before the calibration flags existed."""
    from deepconsensus_amd.models import data as data_lib
    from deepconsensus_amd.models.model import get_model
    from deepconsensus_amd.models.train import _prepare_batch

    torch.manual_seed(seed)
    model = get_model(params).to("cpu")
    model.eval()
    ds = data_lib.DatasetIterator(
        [eval_path], params, params.batch_size, shuffle=False, limit=-1,
    )
    loss_fn = losses_lib.AlignmentLoss(
        del_cost=params.del_cost, loss_reg=params.loss_reg,
        width=params.get("band_width"), reduction="mean",
    )
    acc = losses_lib.PerExampleAccuracy()
    per_class = {v: losses_lib.PerClassAccuracy(k)
                 for k, v in enumerate(" ATCG")}
    total_loss, n = 0.0, 0
    with torch.no_grad():
        for batch in ds.iterate():
            rows, label = _prepare_batch(batch, "cpu")
            probs = model(rows, training=False)
            total_loss += float(loss_fn(label, probs.float()))
            n += 1
            acc.update_state(label.cpu(), probs.cpu())
            for m in per_class.values():
                m.update_state(label.cpu(), probs.cpu())
    metrics = {"loss": total_loss / max(n, 1),
               "per_example_accuracy": acc.result()}
    for sym, m in per_class.items():
        key = "gap_or_pad" if sym == " " else sym.lower()
        metrics[f"per_class_accuracy_{key}"] = m.result()
    return "metric,value\n" + "".join(
        f"{k},{v}\n" for k, v in metrics.items()
    )


def _read_table(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "baseq,total_match,total_mismatch"
    rows = np.array([[int(x) for x in ln.split(",")] for ln in lines[1:]])
    assert rows.shape == (100, 3)
    np.testing.assert_array_equal(rows[:, 0], np.arange(100))
    return rows[:, 1:]


def test_eval_cpu_end_to_end(corpus, tmp_path):
    from deepconsensus_amd.models import infer_eval

    params = _eval_params()
    expected = _parent_inference_csv(corpus, params, seed=5)

    plain = str(tmp_path / "plain")
    torch.manual_seed(5)
    infer_eval.run_inference(plain, "random", [corpus], params=params,
                             device="cpu")
    assert open(os.path.join(plain, "inference.csv")).read() == expected
    assert os.listdir(plain) == ["inference.csv"]

    flagged = str(tmp_path / "flagged")
    cal = os.path.join(flagged, "calibration.csv")
    yj = os.path.join(flagged, "yield.json")
    torch.manual_seed(5)
    infer_eval.run_inference(
        flagged, "random", [corpus], params=params, device="cpu",
        calibration_csv=cal, yield_json=yj,
        dc_calibration="0,1.197654,-0.99781", max_base_quality=60,
    )
    assert open(os.path.join(flagged, "inference.csv")).read() == expected

    model_tab = _read_table(cal)
    ccs_tab = _read_table(infer_eval.ccs_path(cal))
    assert infer_eval.ccs_path(cal).endswith("calibration.ccs.csv")
    result = json.load(open(yj))
    assert result["backend"] == "numpy"
    assert result["dc_calibration"] == "0,1.197654,-0.99781"
    assert model_tab.sum() == result["model"]["table_bases"] > 0
    assert ccs_tab.sum() == result["ccs"]["table_bases"] > 0
    # Every QV is below 100 here, so every emitted base is in the table.
    assert result["model"]["emitted_bases"] == model_tab.sum()
    assert result["ccs"]["emitted_bases"] == ccs_tab.sum()
    assert model_tab[61:].sum() == 0  # --max_base_quality clamp
    assert result["model"]["n_molecules"] == result["ccs"]["n_molecules"] > 1
    for t in (20, 30, 40):
        assert f"yield@emQ{t}" in result["model"]
        assert f"yield@emQ{t}/ccs" in result
    assert "fitted_calibration" in result["ccs"]
    # The synthetic draft CCS is 1 % wrong: it yields at emQ20 only where
    # a molecule stays under that, never at emQ40 for every molecule.
    assert result["ccs"]["yield@emQ20"] >= result["ccs"]["yield@emQ30"]
    assert result["ccs"]["yield@emQ30"] >= result["ccs"]["yield@emQ40"]


def test_eval_cli_flags_default_off_and_parse(monkeypatch):
    from deepconsensus_amd.models import infer_eval

    seen = []
    monkeypatch.setattr(
        infer_eval, "run_inference",
        lambda *a, **kw: seen.append((a, kw)),
    )
    base = ["--checkpoint", "c", "--eval_path", "e", "--out_dir", "o",
            "--device", "cpu"]
    infer_eval.main(base)
    kw = seen[-1][1]
    assert kw["calibration_csv"] is None and kw["yield_json"] is None
    assert kw["dc_calibration"] is None and kw["max_base_quality"] is None
    infer_eval.main(base + [
        "--calibration_csv", "a.csv", "--yield_json", "y.json",
        "--dc_calibration", "skip", "--max_base_quality", "50",
        "--emq_thresholds", "20,35",
    ])
    kw = seen[-1][1]
    assert kw["calibration_csv"] == "a.csv" and kw["yield_json"] == "y.json"
    assert kw["dc_calibration"] == "skip" and kw["max_base_quality"] == 50
    assert kw["emq_thresholds"] == (20.0, 35.0)
