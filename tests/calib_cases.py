"""Shared inputs for the window-calibration tests (CPU and GPU)."""
import os
import sys

import numpy as np

_SCRIPTS = os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"
)


def make_pairs(seed: int, b: int, length: int, max_q: int = 110):
    """Random gapped (label, bases, quals) uint8 [b, length] after the
    K14 device test's recipe: 20 % extra gaps in the truth, one empty
    row, one near-empty row, up to 16 near-identical rows; QVs uniform in
    0..max_q."""
    rng = np.random.default_rng(seed)
    label = rng.integers(0, 5, size=(b, length)).astype(np.uint8)
    label[rng.random((b, length)) < 0.2] = 0
    bases = rng.integers(0, 5, size=(b, length)).astype(np.uint8)
    n_close = min(16, b)
    keep = rng.random((n_close, length)) < 0.9
    bases[:n_close] = np.where(keep, label[:n_close], bases[:n_close])
    label[0] = 0
    if b > 1:
        label[1, 2:] = 0
    quals = rng.integers(0, max_q + 1, size=(b, length)).astype(np.uint8)
    return label, bases, quals


def build_corpus(tmp_dir: str, n_zmws: int = 10):
    """Small synthetic labeled corpus, built the way the yield harness
    builds one; returns the train-split TFRecord path."""
    if _SCRIPTS not in sys.path:
        sys.path.insert(0, _SCRIPTS)
    import yield_harness

    train_path, _eval, n_train, _n_eval = yield_harness.build_synthetic_corpus(
        tmp_dir, n_zmws, seed=11, err_rate=0.02, n_ins=1,
        ccs_err_rate=0.01, n_subreads=4, length=400,
    )
    return train_path, n_train
