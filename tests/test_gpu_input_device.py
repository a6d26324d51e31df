"""batch_assemble / pool_store on the GPU against their numpy twins, the
device iterator on cuda against the host iterator, and train on cuda in
device input mode."""
import numpy as np
import pytest
import torch

from deepconsensus_amd import ops
from deepconsensus_amd.models import config as cfg
from deepconsensus_amd.models import data_device as dd

from input_device_cases import (assert_same_batches, host_batches,
                                make_corpus, make_params)

pytestmark = pytest.mark.gpu

GUARD = 64  # floats on either side of an output
GUARD_VALUE = -12345.5


@pytest.fixture(scope="module")
def ext():
    return ops.get_ext(required=True)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return make_corpus(tmp_path_factory.mktemp("gpu_input_device"))


def _slots(n, R, L, rng):
    S = dd.slot_floats(R, L)
    a = np.zeros((n, S), dtype=np.float32)
    # Integers and halves below 0 and above every maximum; no NaN, no -0.
    a[:, :R * L] = rng.integers(-100, 1400, size=(n, R * L)) / 2.0
    a[a == 0] = 1.0
    off = (R * L + 3) // 4 * 4
    lab = rng.integers(0, 5, size=(n, L)).astype(np.float32)
    if n > 0:
        lab[0] = 0                          # all gap
    if n > 1:
        lab[1] = rng.integers(1, 5, size=L)  # gap free
    a[:, off:off + L] = lab
    a[:, R * L:off] = 0
    return a


def _guarded(shape, lead):
    """A contiguous device view with GUARD floats around it; lead extra
    floats in front shift its address off 16-byte alignment."""
    n = int(np.prod(shape))
    buf = torch.full((lead + 2 * GUARD + n,), GUARD_VALUE,
                     dtype=torch.float32, device="cuda")
    view = buf[lead + GUARD:lead + GUARD + n].view(*shape)
    return buf, view, lead + GUARD, n


def _assert_guards(buf, start, n):
    host = buf.cpu().numpy()
    assert (host[:start] == GUARD_VALUE).all()
    assert (host[start + n:] == GUARD_VALUE).all()


def _run_assemble(ext, R, L, mp, use_ccs_bq, B, shift, maxima, seed, lead=0):
    rng = np.random.default_rng(seed)
    pool = _slots(3, R, L, rng)
    upload = _slots(4, R, L, rng)
    n_in = 3  # row 3 of upload is not live
    sources = [2, ~1, 0, ~2, 2][:B]  # pool and upload mixed, one repeated
    if B == 1:
        sources = [~1]
    gather = np.array(sources, dtype=np.int32)
    dd.validate_tables(gather, np.full(n_in, -1), 3, n_in)
    want_rows, want_label = dd.batch_assemble_numpy(
        pool, upload, n_in, gather, R, L, mp, use_ccs_bq, *maxima, shift)
    rbuf, rows, r0, rn = _guarded((B, R, L), lead)
    lbuf, label, l0, ln = _guarded((B, L), lead)
    ext.batch_assemble_into(
        torch.from_numpy(pool).cuda(), torch.from_numpy(upload).cuda(), n_in,
        torch.from_numpy(gather).cuda(), rows, label, mp, use_ccs_bq,
        float(maxima[0]), float(maxima[1]), float(maxima[2]), shift)
    torch.cuda.synchronize()
    assert rows.cpu().numpy().tobytes() == want_rows.tobytes()
    assert label.cpu().numpy().tobytes() == want_label.tobytes()
    _assert_guards(rbuf, r0, rn)
    _assert_guards(lbuf, l0, ln)


@pytest.mark.parametrize("B", (1, 5))
@pytest.mark.parametrize("R,L,use_ccs_bq", [
    (85, 100, False),  # production
    (86, 100, True),   # ccs_bq layout
    (85, 37, False),   # row bytes not a multiple of 16
])
def test_batch_assemble_matches_twin(ext, R, L, use_ccs_bq, B):
    for shift in (False, True):
        for maxima in ((255, 255, 500), (0, 255, 0)):
            _run_assemble(ext, R, L, 20, use_ccs_bq, B, shift, maxima,
                          seed=R + L + B)
    # An output that is not 16-byte aligned takes the dword-store path.
    _run_assemble(ext, R, L, 20, use_ccs_bq, B, True, (255, 255, 500),
                  seed=7, lead=1)


@pytest.mark.parametrize("L", (1, 63, 64, 65, 100, 129, 255, 256, 257, 600))
def test_label_shift_lengths(ext, L):
    """Wave boundaries (64), the issue's 128 boundary and this kernel's own
    256-column pass boundary."""
    for B in (1, 5):
        _run_assemble(ext, 5, L, 0, False, B, True, (255, 255, 500), seed=L)


def test_slot_floats_agree(ext):
    for R, L in ((85, 100), (86, 100), (85, 37), (5, 1), (7, 3)):
        assert ext.batch_assemble_slot_floats(R, L) == dd.slot_floats(R, L)


def test_pool_store_matches_twin(ext):
    R, L = 85, 37
    rng = np.random.default_rng(9)
    pool = _slots(3, R, L, rng)
    upload = _slots(6, R, L, rng)
    # Duplicate destinations (last writer wins) and -1 entries.
    scatter = np.array([1, -1, 1, 0, -1, 1], dtype=np.int32)
    want = pool.copy()
    dd.pool_store_numpy(want, upload, scatter)
    S = pool.shape[1]
    buf = torch.full((2 * GUARD + 3 * S,), GUARD_VALUE, dtype=torch.float32,
                     device="cuda")
    dev_pool = buf[GUARD:GUARD + 3 * S].view(3, S)
    dev_pool.copy_(torch.from_numpy(pool))
    ext.pool_store(dev_pool, torch.from_numpy(upload).cuda(),
                   torch.from_numpy(scatter).cuda())
    torch.cuda.synchronize()
    assert dev_pool.cpu().numpy().tobytes() == want.tobytes()
    assert (want[1] == upload[5]).all() and (want[2] == pool[2]).all()
    _assert_guards(buf, GUARD, 3 * S)


def test_iterator_on_cuda_equals_host(corpus):
    pattern, _ = corpus
    params = make_params(6)
    ds = dd.DeviceInputIterator([pattern], params, 4, device="cuda",
                                shuffle=True, seed=5, input_workers=2,
                                drop_remainder=False)
    try:
        for epoch in (0, 1):
            got = [(r.cpu().numpy(), l.cpu().numpy())
                   for r, l in ds.iterate(epoch)]
            want = host_batches(pattern, params, 4, epoch, shuffle=True,
                                seed=5, drop_remainder=False)
            assert_same_batches(got, want)
        # Both staging buffers went round more than once: the events that
        # guard their reuse were waited on.
        assert min(ds.stage_uses) >= 3, ds.stage_uses
    finally:
        ds.close()


def test_train_device_mode_on_cuda(corpus, tmp_path):
    import json
    import os

    from deepconsensus_amd.models import train as train_lib

    pattern, n = corpus
    params = cfg.get_config("transformer_learn_values+test")
    params.train_path = [pattern]
    params.eval_path = [pattern]
    params.batch_size = 4
    params.num_epochs = 1
    params.buffer_size = 6
    params.n_examples_train = n
    params.n_examples_eval = n
    params.warmup_steps = 2
    cfg.modify_params(params)
    fed = []
    out_dir = str(tmp_path / "model")
    summary = train_lib.train_model(
        out_dir, params, device="cuda", eval_every=100, limit_steps=3,
        input_mode="device", input_workers=2,
        batch_hook=lambda r, l: fed.append((r.cpu().numpy(),
                                            l.cpu().numpy())))
    assert np.isfinite(summary["eval/loss"])
    assert json.load(open(os.path.join(out_dir, "training_summary.json")))
    want = host_batches(pattern, params, 4, 0, seed=params.seed)
    assert len(fed) == 3
    assert_same_batches(fed, want[:3])
