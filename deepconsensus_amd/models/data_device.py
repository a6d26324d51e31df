"""Device-side training input (--input_mode device).

The host path (models/data.py + train._prepare_batch) decodes, formats,
stacks and uploads every example on the main thread between steps. Here the
per-element work leaves the host:

  * reader workers (spawned processes that never touch the GPU) un-gzip and
    frame their files, locate the two tensor payloads of every kept record
    with dcio/example_scan.py and copy the raw bytes into fixed-size slots
    of a shared-memory ring;
  * a feeder thread consumes the chunks in file order -- so the record
    stream is DatasetIterator._record_stream's whatever the worker count --
    copies the slots into one of two staging buffers and uploads them;
  * ShufflePlanner replays DatasetIterator.iterate on slot numbers: the
    shuffle buffer is a pool of slots (in HBM on a GPU), and every step is
    an upload chunk, a gather table and a scatter table;
  * ops/hip/batch_assemble.hip gathers a batch out of pool and upload,
    doing format_rows' clips and the optional label left shift on the way,
    and pool_store moves the uploads into their slots.

The batches are bitwise those of DatasetIterator + _prepare_batch, in the
same order, for the same files, seed, epoch, rank/world, buffer_size, limit
and drop_remainder. On a CPU device the numpy twins below are the
implementation; on a GPU they are the kernels' oracle.

Slot layout (fp32): R*L subread floats padded to a multiple of 4, then L
label floats padded likewise. Gather entries: g >= 0 is pool slot g, g < 0
is upload row ~g. Scatter entries: the pool slot upload row i moves into,
or -1; when several rows name one slot the last wins.

Only training input is covered: infer_eval needs names and window
positions and keeps the host path.
"""
from __future__ import annotations

import atexit
import glob as globlib
import multiprocessing as mp
import os
import queue
import random
import struct
import threading
import time
import traceback
import weakref
from multiprocessing import shared_memory
from typing import Callable, Dict, Iterator, List, NamedTuple, Optional, Tuple

import numpy as np

from deepconsensus_amd.dcio import tfrecord
from deepconsensus_amd.dcio.example_scan import scan_example
from deepconsensus_amd.models.config import Params, get_indices
from deepconsensus_amd.utils import phred

INPUT_MODES = ("host", "device")
POOL_CAP = 100_000  # DatasetIterator's cap on buffer_size
SHM_PREFIX = "dcin"
_POLL_S = 0.05


def resolve_input_mode(mode: Optional[str] = None) -> str:
    """Flag value, else DC_INPUT_MODE, else host."""
    mode = mode or os.environ.get("DC_INPUT_MODE") or "host"
    if mode not in INPUT_MODES:
        raise ValueError(
            f"unknown input mode {mode!r}; choices: {', '.join(INPUT_MODES)}"
        )
    return mode


def default_input_workers() -> int:
    """Half the visible CPUs, at most 8: with the main process, its feeder
    thread and torch's own threads this stays inside a 16-CPU allotment
    even where os.cpu_count() reports a much larger machine."""
    return max(1, min(8, (os.cpu_count() or 2) // 2))


def _pad4(n: int) -> int:
    return (n + 3) & ~3


def slot_floats(R: int, L: int) -> int:
    return _pad4(R * L) + _pad4(L)


# ---------------------------------------------------------------------------
# Shuffle plan (integers only)


class Step(NamedTuple):
    n_in: int            # live rows of the upload chunk
    gather: np.ndarray   # int32 [n_out]
    scatter: np.ndarray  # int32 [n_in]
    out_off: int         # first row of the current batch the gather fills
    done: bool           # the batch is complete after this step


class ShufflePlanner:
    """DatasetIterator.iterate's control flow on slot numbers.

    Same random.Random(seed * 7919 + epoch), same calls in the same order.
    Feed it one add() per incoming record, after checking want_more() (the
    per-record limit test), then drain finish(). A step closes when the
    batch completes or the upload chunk is full, whichever is first, so a
    batch may be assembled by several steps (out_off says where).
    """

    def __init__(self, pool_slots: int, batch_size: int, shuffle: bool,
                 seed: int, epoch: int, limit: int = -1,
                 chunk_cap: Optional[int] = None):
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        if shuffle and pool_slots < 1:
            raise ValueError("shuffling needs a buffer_size of at least 1")
        self.rng = random.Random(seed * 7919 + epoch)
        self.P = pool_slots if shuffle else 0
        self.B = batch_size
        self.shuffle = shuffle
        self.limit = limit
        self.cap = chunk_cap or batch_size
        self.filled = 0      # len(buffer) of the host path
        self.n_yielded = 0
        self.out_off = 0
        self._new_chunk()

    def _new_chunk(self):
        self.n_in = 0
        self._gather: List[int] = []
        self._scatter: List[int] = []
        self._pending: Dict[int, int] = {}  # slot -> upload row holding it

    def want_more(self) -> bool:
        return not (self.limit >= 0
                    and self.n_yielded * self.B >= self.limit)

    @property
    def remainder(self) -> int:
        """Examples of the incomplete batch (after finish())."""
        return self.out_off

    def _emit(self, slot: int):
        u = self._pending.get(slot)
        self._gather.append(slot if u is None else ~u)

    def _close(self, done: bool) -> Step:
        step = Step(self.n_in, np.asarray(self._gather, dtype=np.int32),
                    np.asarray(self._scatter, dtype=np.int32),
                    self.out_off, done)
        if done:
            self.out_off = 0
            self.n_yielded += 1
        else:
            self.out_off += len(self._gather)
        self._new_chunk()
        return step

    def _maybe_close(self) -> Optional[Step]:
        done = self.out_off + len(self._gather) == self.B
        if done or self.n_in == self.cap:
            return self._close(done)
        return None

    def add(self) -> Optional[Step]:
        """One incoming record; it is upload row n_in of the open chunk."""
        u = self.n_in
        self.n_in += 1
        if not self.shuffle:
            self._scatter.append(-1)
            self._gather.append(~u)
        elif self.filled < self.P:
            self._scatter.append(self.filled)
            self._pending[self.filled] = u
            self.filled += 1
        else:
            j = self.rng.randrange(self.filled)
            self._emit(j)
            self._scatter.append(j)
            self._pending[j] = u
        return self._maybe_close()

    def finish(self) -> Iterator[Step]:
        """The drain: rng.shuffle over the slots, then whatever is open."""
        if self.shuffle:
            order = list(range(self.filled))
            self.rng.shuffle(order)
            for j in order:
                self._emit(j)
                step = self._maybe_close()
                if step is not None:
                    yield step
        if self.n_in or self._gather:
            yield self._close(False)


def validate_tables(gather: np.ndarray, scatter: np.ndarray, pool_slots: int,
                    n_in: int) -> None:
    """Host check before every launch: slots < P, upload rows < n_in."""
    gather = np.asarray(gather)
    scatter = np.asarray(scatter)
    if gather.ndim != 1 or scatter.ndim != 1:
        raise ValueError("gather and scatter tables must be 1-D")
    if scatter.shape[0] != n_in:
        raise ValueError(
            f"scatter table has {scatter.shape[0]} entries for {n_in} "
            "upload rows")
    pool_g = gather[gather >= 0]
    if pool_g.size and int(pool_g.max()) >= pool_slots:
        raise ValueError(
            f"gather table names pool slot {int(pool_g.max())} of "
            f"{pool_slots}")
    up_g = ~gather[gather < 0]
    if up_g.size and int(up_g.max()) >= n_in:
        raise ValueError(
            f"gather table names upload row {int(up_g.max())} of {n_in}")
    if scatter.size and (int(scatter.min()) < -1
                         or int(scatter.max()) >= pool_slots):
        raise ValueError(
            f"scatter table entry outside [-1, {pool_slots})")


# ---------------------------------------------------------------------------
# Numpy twins of ops/hip/batch_assemble.hip


def batch_assemble_numpy(
    pool: np.ndarray, upload: np.ndarray, n_in: int, gather: np.ndarray,
    R: int, L: int, max_passes: int, use_ccs_bq: bool, pw_max: float,
    ip_max: float, sn_max: float, remove_label_gaps: bool,
) -> Tuple[np.ndarray, np.ndarray]:
    """rows fp32 [B, R, L], label fp32 [B, L] for a valid gather table."""
    gather = np.asarray(gather)
    validate_tables(gather, np.full(n_in, -1), pool.shape[0], n_in)
    S = slot_floats(R, L)
    assert pool.shape[1] == S and upload.shape[1] == S, (pool.shape, S)
    B = gather.shape[0]
    slots = np.empty((B, S), dtype=np.float32)
    from_pool = gather >= 0
    slots[from_pool] = pool[gather[from_pool]]
    slots[~from_pool] = upload[~gather[~from_pool]]
    rows = slots[:, :R * L].reshape(B, R, L).copy()
    _, pw_idx, ip_idx, _, _, _, sn_idx = get_indices(max_passes, use_ccs_bq)
    for (lo, hi), vmax in ((pw_idx, pw_max), (ip_idx, ip_max),
                           (sn_idx, sn_max)):
        if vmax:
            rows[:, lo:hi] = np.clip(rows[:, lo:hi], 0, vmax)
    off = _pad4(R * L)
    label = slots[:, off:off + L].copy()
    if remove_label_gaps:
        for b in range(B):
            label[b] = phred.left_shift_seq(label[b])
    return rows, label


def pool_store_numpy(pool: np.ndarray, upload: np.ndarray,
                     scatter: np.ndarray) -> None:
    """In place; rows in ascending order, so the last writer wins."""
    scatter = np.asarray(scatter)
    validate_tables(np.zeros(0, np.int32), scatter, pool.shape[0],
                    scatter.shape[0])
    for i in np.nonzero(scatter >= 0)[0]:
        pool[scatter[i]] = upload[i]


# ---------------------------------------------------------------------------
# Records: framing, scanning, copying raw payloads into slots


class SlotSpec(NamedTuple):
    R: int
    L: int

    @property
    def rows_bytes(self) -> int:
        return self.R * self.L * 4

    @property
    def label_bytes(self) -> int:
        return self.L * 4

    @property
    def label_off(self) -> int:
        return _pad4(self.R * self.L) * 4

    @property
    def slot_bytes(self) -> int:
        return slot_floats(self.R, self.L) * 4


def read_file_bytes(path: str) -> bytes:
    with tfrecord._open(path, "rb", None) as fh:
        return fh.read()


def frame_records(data: bytes, path: str = "") -> List[Tuple[int, int]]:
    """(start, end) of every record payload: lengths only, nothing parsed."""
    spans = []
    off, n = 0, len(data)
    while off < n:
        if off + 12 > n:
            raise ValueError(f"truncated TFRecord header in {path}")
        (length,) = struct.unpack_from("<Q", data, off)
        start = off + 12
        end = start + length
        if end + 4 > n:
            raise ValueError(
                f"truncated TFRecord in {path}: record {len(spans)}")
        spans.append((start, end))
        off = end + 4
    return spans


def count_records(path: str) -> int:
    return len(frame_records(read_file_bytes(path), path))


def copy_record(data: bytes, data_u8: np.ndarray, start: int, end: int,
                spec: SlotSpec, dst: np.ndarray, path: str, index: int
                ) -> None:
    """Scans record [start, end) of data and copies its two payloads into
    the slot dst (uint8 [slot_bytes]); pad bytes are left as they are."""
    try:
        sp = scan_example(data, start, end)
    except ValueError as e:
        raise ValueError(f"{path}: record {index}: {e}") from None
    want = [spec.R, spec.L, 1]
    if list(sp.subreads_shape) != want or sp.subreads[1] != spec.rows_bytes:
        raise ValueError(
            f"{path}: record {index}: subreads shape "
            f"{list(sp.subreads_shape)} ({sp.subreads[1]} bytes), expected "
            f"{want}")
    if sp.label is None:
        raise ValueError(f"{path}: record {index}: no label/encoded")
    if list(sp.label_shape) != [spec.L] or sp.label[1] != spec.label_bytes:
        raise ValueError(
            f"{path}: record {index}: label shape {list(sp.label_shape)} "
            f"({sp.label[1]} bytes), expected {[spec.L]}")
    o, n = sp.subreads
    dst[:n] = data_u8[o:o + n]
    o, n = sp.label
    dst[spec.label_off:spec.label_off + n] = data_u8[o:o + n]


class FileJob(NamedTuple):
    pos: int    # position in the epoch's file order
    path: str
    first: int  # global index of the file's first record


def _file_chunks(job: FileJob, rank: int, world: int, spec: SlotSpec,
                 chunk_records: int, acquire: Callable[[], Optional[np.ndarray]]
                 ) -> Iterator[Tuple[np.ndarray, int]]:
    """Fills buffers obtained from acquire() (uint8 [chunk_records,
    slot_bytes]; None stops) with the kept records of one file."""
    data = read_file_bytes(job.path)
    data_u8 = np.frombuffer(data, dtype=np.uint8)
    spans = frame_records(data, job.path)
    first_kept = (rank - job.first) % world
    buf = None
    n = 0
    for index in range(first_kept, len(spans), world):
        if buf is None:
            buf = acquire()
            if buf is None:
                return
            n = 0
        start, end = spans[index]
        copy_record(data, data_u8, start, end, spec, buf[n], job.path, index)
        n += 1
        if n == chunk_records:
            yield buf, n
            buf = None
    if buf is not None and n:
        yield buf, n


def _worker_main(shm_name: str, n_chunks: int, chunk_records: int,
                 spec: SlotSpec, jobs: List[FileJob], rank: int, world: int,
                 free_q, out_q) -> None:
    """Reader process: owns jobs, fills ring slots, posts (file, chunk, n)."""
    shm = None
    ring = None
    try:
        shm = shared_memory.SharedMemory(name=shm_name)
        ring = np.ndarray((n_chunks, chunk_records, spec.slot_bytes),
                          dtype=np.uint8, buffer=shm.buf)
        held = [None]  # ring slot being filled; None once told to stop

        def acquire():
            held[0] = free_q.get()
            return None if held[0] is None else ring[held[0]]

        for job in jobs:
            for _buf, n in _file_chunks(job, rank, world, spec,
                                        chunk_records, acquire):
                out_q.put(("chunk", job.pos, held[0], n))
            out_q.put(("eof", job.pos))
    except BaseException:  # noqa: BLE001 - reported to the main process
        out_q.put(("error", traceback.format_exc()))
    finally:
        del ring
        if shm is not None:
            shm.close()


_LIVE_READERS: "weakref.WeakSet" = weakref.WeakSet()


@atexit.register
def _close_live_readers():
    # An epoch normally ends in its generator's finally (exhaustion, close()
    # or an exception); this covers a generator still alive at exit.
    for readers in list(_LIVE_READERS):
        readers.close()


class _Readers:
    """The record source of one epoch: chunks of slots in file order."""

    def __init__(self, jobs: List[FileJob], rank: int, world: int,
                 spec: SlotSpec, n_workers: int, chunk_records: int,
                 ring_chunks: int = 32):
        self.jobs = jobs
        self.rank, self.world = rank, world
        self.spec = spec
        self.chunk_records = chunk_records
        self.n_workers = min(n_workers, len(jobs))
        # The feeder drains one file at a time, so a worker whose file is
        # not up yet reads ahead only as far as its ring reaches: the ring
        # is what lets the workers inflate and scan in parallel. 32 chunks
        # of 64 records are 70 MB per worker in the production layout; the
        # rings together take at most half of what /dev/shm has free.
        if self.n_workers:
            chunk_bytes = chunk_records * spec.slot_bytes
            try:
                st = os.statvfs("/dev/shm")
                room = st.f_bavail * st.f_frsize // 2
                ring_chunks = min(
                    ring_chunks, room // (chunk_bytes * self.n_workers))
            except OSError:
                pass
        self.ring_chunks = max(2, ring_chunks)
        self.procs: List = []
        self.shms: List[shared_memory.SharedMemory] = []
        self.rings: List[np.ndarray] = []
        self.free_qs: List = []
        self.out_qs: List = []
        self.stop = threading.Event()
        if self.n_workers:
            try:
                self._start()
            except BaseException:
                self.close()
                raise

    def _start(self):
        _LIVE_READERS.add(self)
        ctx = mp.get_context("spawn")
        size = self.ring_chunks * self.chunk_records * self.spec.slot_bytes
        for k in range(self.n_workers):
            name = f"{SHM_PREFIX}_{os.getpid()}_{id(self) & 0xFFFFFF:x}_{k}"
            shm = shared_memory.SharedMemory(name=name, create=True,
                                             size=size)
            self.shms.append(shm)
            self.rings.append(np.ndarray(
                (self.ring_chunks, self.chunk_records, self.spec.slot_bytes),
                dtype=np.uint8, buffer=shm.buf))
            free_q, out_q = ctx.Queue(), ctx.Queue()
            for c in range(self.ring_chunks):
                free_q.put(c)
            self.free_qs.append(free_q)
            self.out_qs.append(out_q)
            proc = ctx.Process(
                target=_worker_main,
                args=(name, self.ring_chunks, self.chunk_records, self.spec,
                      self.jobs[k::self.n_workers], self.rank, self.world,
                      free_q, out_q),
                daemon=True)
            proc.start()
            self.procs.append(proc)

    def _get(self, k: int):
        while True:
            if self.stop.is_set():
                return None
            try:
                return self.out_qs[k].get(timeout=_POLL_S)
            except queue.Empty:
                if not self.procs[k].is_alive():
                    try:
                        return self.out_qs[k].get(timeout=_POLL_S)
                    except queue.Empty:
                        raise RuntimeError(
                            f"input worker {k} died (exit code "
                            f"{self.procs[k].exitcode})") from None

    def chunks(self) -> Iterator[np.ndarray]:
        """uint8 [n, slot_bytes] blocks; a block is valid until the next
        one is asked for."""
        if not self.n_workers:
            local = np.zeros((self.chunk_records, self.spec.slot_bytes),
                             dtype=np.uint8)
            for job in self.jobs:
                for buf, n in _file_chunks(
                        job, self.rank, self.world, self.spec,
                        self.chunk_records,
                        lambda: None if self.stop.is_set() else local):
                    yield buf[:n]
                if self.stop.is_set():
                    return
            return
        for job in self.jobs:
            k = job.pos % self.n_workers
            while True:
                msg = self._get(k)
                if msg is None:
                    return
                if msg[0] == "error":
                    raise RuntimeError(
                        "input worker failed:\n" + msg[1])
                if msg[1] != job.pos:
                    raise RuntimeError(
                        f"input worker {k} posted file {msg[1]}, expected "
                        f"{job.pos}")
                if msg[0] == "eof":
                    break
                _, _, c, n = msg
                yield self.rings[k][c, :n]
                self.free_qs[k].put(c)

    def close(self):
        """Stops and joins the workers, unlinks the shared memory."""
        self.stop.set()
        for q_ in self.free_qs:
            try:
                q_.put(None)
            except (OSError, ValueError):
                pass
        for p in self.procs:
            p.join(timeout=2.0)
            if p.is_alive():
                p.terminate()
                p.join()
        self.procs = []
        for q_ in self.free_qs + self.out_qs:
            q_.cancel_join_thread()
            q_.close()
        self.free_qs, self.out_qs = [], []
        self.rings = []
        for shm in self.shms:
            try:
                shm.close()
            except BufferError:
                pass
            try:
                shm.unlink()
            except FileNotFoundError:
                pass
        self.shms = []


# ---------------------------------------------------------------------------
# The iterator


class DeviceInputIterator:
    """DatasetIterator's training twin: yields (rows, label) tensors on
    `device`, rows fp32 [B, R, L], label fp32 [B, L]."""

    def __init__(
        self,
        file_patterns: List[str],
        params: Params,
        batch_size: int,
        device: str = "cpu",
        shuffle: bool = True,
        seed: int = 1,
        rank: int = 0,
        world_size: int = 1,
        limit: int = -1,
        drop_remainder: bool = True,
        input_workers: Optional[int] = None,
        chunk_records: int = 64,
    ):
        import torch

        if isinstance(file_patterns, str):
            file_patterns = [file_patterns]
        self.files: List[str] = []
        for p in file_patterns:
            self.files.extend(sorted(globlib.glob(p)))
        if not self.files:
            raise FileNotFoundError(f"no files match {file_patterns}")
        self.params = params
        self.batch_size = batch_size
        self.device = torch.device(device)
        self.shuffle = shuffle
        self.seed = seed
        self.rank = rank
        self.world_size = world_size
        self.limit = limit
        self.drop_remainder = drop_remainder
        self.input_workers = (default_input_workers() if input_workers is None
                              else int(input_workers))
        if self.input_workers < 0:
            raise ValueError("input_workers must be >= 0")
        self.chunk_records = max(1, min(chunk_records, batch_size))
        self.pool_slots = min(int(params.get("buffer_size", 1000)), POOL_CAP)
        if not shuffle:
            self.pool_slots = 0
        self.remove_label_gaps = bool(params.get("remove_label_gaps"))
        self.spec = self._peek_spec()
        self._counts: Dict[str, int] = {}
        self._readers: Optional[_Readers] = None
        self._thread: Optional[threading.Thread] = None
        self.stage_uses = [0, 0]
        self.wait_s = 0.0  # main thread blocked on the feeder, all epochs
        self._bufs = None
        self._pool = None

    # -- set-up ------------------------------------------------------------

    def _peek_spec(self) -> SlotSpec:
        for path in self.files:
            for rec in tfrecord.read_tfrecords(path):
                try:
                    sp = scan_example(rec)
                except ValueError as e:
                    raise ValueError(f"{path}: record 0: {e}") from None
                shape = list(sp.subreads_shape)
                if (len(shape) != 3 or shape[2] != 1
                        or shape[0] != self.params.total_rows):
                    raise ValueError(
                        f"{path}: record 0: subreads shape {shape} does not "
                        f"match total_rows={self.params.total_rows}")
                return SlotSpec(shape[0], shape[1])
        raise ValueError(f"no records in {self.files}")

    def _jobs(self, epoch: int) -> List[FileJob]:
        files = list(self.files)
        rng = random.Random(self.seed + epoch)
        if self.shuffle:
            rng.shuffle(files)
        jobs, first = [], 0
        for pos, path in enumerate(files):
            jobs.append(FileJob(pos, path, first))
            if self.world_size > 1:
                # The rank filter needs global record indices: one framing
                # pass per file, cached for the run.
                if path not in self._counts:
                    self._counts[path] = count_records(path)
                first += self._counts[path]
        return jobs

    def _alloc(self):
        import torch

        if self._bufs is not None:
            return
        S = slot_floats(self.spec.R, self.spec.L)
        cap, B = self.batch_size, self.batch_size
        cuda = self.device.type == "cuda"
        bufs = []
        for _ in range(2):
            stage = torch.zeros((cap, S), dtype=torch.float32)
            tabs = torch.zeros(B + cap, dtype=torch.int32)
            buf = {"stage": stage, "tabs": tabs}
            if cuda:
                buf["stage"] = stage = stage.pin_memory()
                buf["tabs"] = tabs = tabs.pin_memory()
                buf["dev"] = torch.zeros((cap, S), dtype=torch.float32,
                                         device=self.device)
                buf["dev_tabs"] = torch.zeros(B + cap, dtype=torch.int32,
                                              device=self.device)
                buf["h2d"] = torch.cuda.Event()
                buf["consumed"] = torch.cuda.Event()
                buf["used"] = False
            buf["stage_u8"] = stage.numpy().view(np.uint8)
            buf["tabs_np"] = tabs.numpy()
            bufs.append(buf)
        self._bufs = bufs
        if cuda:
            self._copy_stream = torch.cuda.Stream(device=self.device)
            self._pool = torch.zeros((self.pool_slots, S),
                                     dtype=torch.float32, device=self.device)
            from deepconsensus_amd import ops

            self._ext = ops.get_ext(required=True)
        else:
            self._pool = np.zeros((self.pool_slots, S), dtype=np.float32)

    # -- feeder thread -----------------------------------------------------

    def _acquire_stage(self) -> Optional[int]:
        while not self._stop.is_set():
            try:
                k = self._free_q.get(timeout=_POLL_S)
            except queue.Empty:
                continue
            buf = self._bufs[k]
            if self.device.type == "cuda" and buf["used"]:
                # The upload out of this pinned buffer must have finished
                # before the host writes into it again.
                buf["h2d"].synchronize()
            self.stage_uses[k] += 1
            return k
        return None

    def _post(self, k: int, step: Step):
        validate_tables(step.gather, step.scatter, self.pool_slots,
                        step.n_in)
        buf = self._bufs[k]
        B = self.batch_size
        n_out = step.gather.shape[0]
        buf["tabs_np"][:n_out] = step.gather
        buf["tabs_np"][B:B + step.n_in] = step.scatter
        if self.device.type == "cuda":
            import torch

            with torch.cuda.stream(self._copy_stream):
                if buf["used"]:
                    # The kernels that read this upload buffer last time.
                    self._copy_stream.wait_event(buf["consumed"])
                if step.n_in:
                    buf["dev"][:step.n_in].copy_(
                        buf["stage"][:step.n_in], non_blocking=True)
                buf["dev_tabs"].copy_(buf["tabs"], non_blocking=True)
                buf["h2d"].record(self._copy_stream)
            buf["used"] = True
        self._out_q.put(("step", k, step))

    def _feed(self, epoch: int):
        try:
            planner = ShufflePlanner(
                self.pool_slots, self.batch_size, self.shuffle, self.seed,
                epoch, self.limit, chunk_cap=self.batch_size)
            k = self._acquire_stage()
            limited = False
            for block in self._readers.chunks():
                for i in range(block.shape[0]):
                    if not planner.want_more():
                        limited = True
                        break
                    if k is None:
                        return
                    self._bufs[k]["stage_u8"][planner.n_in] = block[i]
                    step = planner.add()
                    if step is not None:
                        self._post(k, step)
                        k = self._acquire_stage()
                if limited:
                    break
            if limited:
                self._readers.stop.set()
            for step in planner.finish():
                if k is None:
                    return
                self._post(k, step)
                k = self._acquire_stage()
            self._out_q.put(("end", planner.remainder, limited))
        except BaseException as e:  # noqa: BLE001 - re-raised by iterate()
            self._out_q.put(("error", e))

    # -- main thread -------------------------------------------------------

    def _assemble(self, k: int, step: Step, rows, label):
        p = self.params
        buf = self._bufs[k]
        B = self.batch_size
        n_out = step.gather.shape[0]
        lo, hi = step.out_off, step.out_off + n_out
        args = (int(p.max_passes), bool(p.use_ccs_bq), float(p.PW_MAX or 0),
                float(p.IP_MAX or 0), float(p.SN_MAX or 0),
                self.remove_label_gaps)
        if self.device.type == "cuda":
            import torch

            torch.cuda.current_stream(self.device).wait_event(buf["h2d"])
            if n_out:
                self._ext.batch_assemble_into(
                    self._pool, buf["dev"], step.n_in,
                    buf["dev_tabs"][:n_out], rows[lo:hi], label[lo:hi],
                    *args)
            if step.n_in and self.pool_slots:
                self._ext.pool_store(self._pool, buf["dev"],
                                     buf["dev_tabs"][B:B + step.n_in])
            buf["consumed"].record(torch.cuda.current_stream(self.device))
        else:
            upload = buf["stage"].numpy()
            if n_out:
                r, l = batch_assemble_numpy(
                    self._pool, upload, step.n_in, step.gather, self.spec.R,
                    self.spec.L, *args)
                rows[lo:hi] = torch_from(r)
                label[lo:hi] = torch_from(l)
            if step.n_in and self.pool_slots:
                pool_store_numpy(self._pool, upload, step.scatter)
        self._free_q.put(k)

    def __iter__(self):
        return self.iterate(epoch=0)

    def iterate(self, epoch: int = 0):
        """One epoch of (rows, label) batches."""
        import torch

        if self._thread is not None:
            raise RuntimeError("another epoch of this iterator is running")
        self._alloc()
        self._stop = threading.Event()
        self._free_q: "queue.Queue[int]" = queue.Queue()
        self._out_q: "queue.Queue[tuple]" = queue.Queue()
        for k in range(2):
            self._free_q.put(k)
        try:
            self._readers = _Readers(
                self._jobs(epoch), self.rank, self.world_size, self.spec,
                self.input_workers, self.chunk_records)
            self._thread = threading.Thread(
                target=self._feed, args=(epoch,), daemon=True,
                name="dc-input-feeder")
            self._thread.start()
            B, R, L = self.batch_size, self.spec.R, self.spec.L
            rows = label = None
            while True:
                t0 = time.perf_counter()
                msg = self._out_q.get()
                self.wait_s += time.perf_counter() - t0
                if msg[0] == "error":
                    raise msg[1]
                if msg[0] == "end":
                    n = msg[1]
                    if n and not self.drop_remainder:
                        yield rows[:n], label[:n]
                    return
                _, k, step = msg
                if rows is None:
                    rows = torch.empty((B, R, L), dtype=torch.float32,
                                       device=self.device)
                    label = torch.empty((B, L), dtype=torch.float32,
                                        device=self.device)
                self._assemble(k, step, rows, label)
                if step.done:
                    out = (rows, label)
                    rows = label = None
                    yield out
        finally:
            self._end_epoch()

    def _end_epoch(self):
        if getattr(self, "_stop", None) is not None:
            self._stop.set()
        if self._readers is not None:
            self._readers.stop.set()
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        if self._readers is not None:
            self._readers.close()
            self._readers = None
        if self.device.type == "cuda" and self._bufs is not None:
            import torch

            # The next epoch's feeder starts from idle buffers.
            torch.cuda.current_stream(self.device).synchronize()
            self._copy_stream.synchronize()

    def close(self):
        """Stops the feeder, joins the workers, unlinks the shared memory.
        Closing the generator of a running epoch does the same."""
        self._end_epoch()

    def count_examples(self) -> int:
        return sum(count_records(f) for f in self.files)


def torch_from(a: np.ndarray):
    import torch

    return torch.from_numpy(a)


# ---------------------------------------------------------------------------
# One entry point for train / distill


class HostInput:
    """Today's path: DatasetIterator + train._prepare_batch."""

    def __init__(self, file_patterns, params, batch_size, device, **kw):
        from deepconsensus_amd.models import data as data_lib

        self.ds = data_lib.DatasetIterator(file_patterns, params, batch_size,
                                           **kw)
        self.device = device

    def iterate(self, epoch: int = 0):
        from deepconsensus_amd.models.train import _prepare_batch

        for batch in self.ds.iterate(epoch):
            yield _prepare_batch(batch, self.device)

    def close(self):
        pass


def make_input(file_patterns, params: Params, batch_size: int, device,
               input_mode: Optional[str] = None,
               input_workers: Optional[int] = None, **kw):
    """The (rows, label) batch source of train and distill: an object with
    iterate(epoch) and close(). kw are DatasetIterator's keyword arguments
    (shuffle, seed, rank, world_size, limit, drop_remainder)."""
    mode = resolve_input_mode(input_mode)
    if mode == "host":
        return HostInput(file_patterns, params, batch_size, device, **kw)
    return DeviceInputIterator(file_patterns, params, batch_size,
                               device=device, input_workers=input_workers,
                               **kw)
