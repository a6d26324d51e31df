"""Shared helpers of the device-input tests (CPU and GPU files)."""
import os

import numpy as np

from deepconsensus_amd.dcio import tfrecord
from deepconsensus_amd.models import config as cfg
from deepconsensus_amd.models import data as data_lib
from deepconsensus_amd.models import data_device as dd
from deepconsensus_amd.models.train import _prepare_batch

SPLIT = (3, None, 5)  # records in file 0, file 1 (the rest), file 2


def make_corpus(tmp_path):
    """Training records from the real preprocess pipeline, split over three
    files of unequal length. Returns (glob pattern, record count)."""
    from test_train import make_training_data

    train_file, _ = make_training_data(tmp_path, n_zmws=6)
    recs = list(tfrecord.read_tfrecords(train_file))
    assert len(recs) >= 14, len(recs)
    a, c = SPLIT[0], SPLIT[2]
    parts = [recs[:a], recs[a:len(recs) - c], recs[len(recs) - c:]]
    assert len({len(p) for p in parts}) == 3
    out = tmp_path / "split"
    os.makedirs(out)
    for i, part in enumerate(parts):
        with tfrecord.TFRecordWriter(str(out / f"part-{i}.tfrecord.gz")) as w:
            for r in part:
                w.write(r)
    return str(out / "part-*.tfrecord.gz"), len(recs)


def make_params(buffer_size):
    params = cfg.get_config("transformer_learn_values+test")
    cfg.modify_params(params)
    params.buffer_size = buffer_size
    return params


def host_batches(pattern, params, batch_size, epoch=0, **kw):
    ds = data_lib.DatasetIterator([pattern], params, batch_size, **kw)
    return [tuple(t.numpy() for t in _prepare_batch(b, "cpu"))
            for b in ds.iterate(epoch)]


def device_batches(pattern, params, batch_size, epoch=0, device="cpu",
                   input_workers=0, **kw):
    ds = dd.DeviceInputIterator([pattern], params, batch_size, device=device,
                                input_workers=input_workers, **kw)
    try:
        return [(r.cpu().numpy(), l.cpu().numpy())
                for r, l in ds.iterate(epoch)]
    finally:
        ds.close()


def assert_same_batches(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for i, ((gr, gl), (wr, wl)) in enumerate(zip(got, want)):
        assert gr.shape == wr.shape and gl.shape == wl.shape, i
        assert gr.dtype == wr.dtype == np.float32
        assert gr.tobytes() == wr.tobytes(), f"rows of batch {i} differ"
        assert gl.tobytes() == wl.tobytes(), f"label of batch {i} differ"


def our_shm_segments():
    prefix = f"{dd.SHM_PREFIX}_{os.getpid()}_"
    return [n for n in os.listdir("/dev/shm") if n.startswith(prefix)]
