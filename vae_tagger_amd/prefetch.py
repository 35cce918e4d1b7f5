"""Input side of the pipelined CLIs: image files -> device batches, ahead of the encoder.

The reference's loops (infer_full.py:95-128, infer_vae.py:53-72) open, resize, normalise and run ONE image at a time on one
thread.  Here a bounded thread pool decodes (`Image.open(p).convert("RGB")`: Pillow releases the GIL inside its decoders), the
decoded uint8 pixels are copied into pinned staging buffers by the workers, cross PCIe at 1 B per sample on a SIDE stream, and
the resize (Pillow's resample, bit for bit: vt_resize_u8) + ToTensor + Normalize (vt_preprocess_u8) run there too, so batch
n + 1's input is being built while batch n is in the encoder.  Skip-and-count is preserved: a file that fails to open or decode
yields (path, exception) and the loop goes on (infer_full.py:130-132).

`host_resize=True` is the reference's own route (PIL transforms on the CPU, fp32 tensors over PCIe): same bits, slower.

With `bucketing=` (an AspectRatioBucketing) the feeder groups by aspect-ratio bucket instead of squashing to a square: every decoded
image goes to the bucket of its own size (`bucket_for_ratio(w / h)`), a batch leaves when a bucket holds `batch_size` images, and at
most `max_pending` images wait -- beyond that the fullest bucket leaves short (ties: the bucket whose oldest image came first); the
end flushes every bucket, oldest first.  The order of the batches is a function of the path list and the image sizes only.  A batch
is staged by ONE vt_resize_normalize_batch call (SmartResize's centre crop + LANCZOS + normalise, two launches whatever the batch
size).  `labels=` (path -> fp32 row) adds the batch's [b, N] label tensor, copied on the side stream, as a fifth element.
`FeederLoader` presents a feeder as the loader of {"pixel_values", "labels"} batches that evaluation.py iterates over.
"""
import collections
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch


def default_workers():
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(16, n))


class _PinnedPool:
    """Pinned uint8 staging buffers: taken by the decode workers, returned once the H2D copy that read them has completed.
    Allocated on demand; the feeder's window of outstanding decodes bounds how many exist."""

    def __init__(self):
        self.free = queue.LifoQueue()

    def get(self, nbytes):
        try:
            buf = self.free.get_nowait()
        except queue.Empty:
            buf = None
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, 1 << 20) * 5 // 4, dtype=torch.uint8).pin_memory()    # (rounded up: one size class serves the run)
        return buf

    def put(self, buf):
        self.free.put(buf)


class BucketGrouper:
    """The grouping policy of the bucket feeder, free of any device work: `add(key, bucket, item)` queues one image under its bucket
    and returns the groups that leave because of it -- the bucket itself once it holds `batch_size` images, else, when more than
    `max_pending` images wait, the fullest bucket, short (ties: the bucket whose oldest image arrived first); `flush()` returns what
    is left, the bucket with the oldest image first.  A group is (bucket, [(key, item), ...]) in arrival order.  The sequence of
    groups depends on the sequence of (key, bucket) pairs only."""

    def __init__(self, batch_size, max_pending):
        self.bs, self.max_pending = max(1, int(batch_size)), max(1, int(max_pending))
        self.pending = {}                            # bucket -> [(arrival number, key, item)]
        self.count = self.seq = self.high_water = 0

    def _pop(self, bucket):
        group = self.pending.pop(bucket)
        self.count -= len(group)
        return bucket, [(k, it) for _, k, it in group]

    def add(self, key, bucket, item):
        self.pending.setdefault(bucket, []).append((self.seq, key, item))
        self.seq += 1
        self.count += 1
        out = []
        if len(self.pending[bucket]) >= self.bs:
            out.append(self._pop(bucket))
        elif self.count > self.max_pending:
            out.append(self._pop(min(self.pending, key=lambda b: (-len(self.pending[b]), self.pending[b][0][0]))))
        self.high_water = max(self.high_water, self.count)
        return out

    def flush(self):
        return [self._pop(b) for b in sorted(self.pending, key=lambda b: self.pending[b][0][0])]


class BatchFeeder:
    """Iterates over `paths` in order and yields, per batch of up to `batch_size` successfully decoded images:

        (names, x, ready, failed)

    names: the paths of the batch's images; x: fp32 [b,3,res,res] on `pipe.device`, normalised to [-1,1]; ready: a
    torch.cuda.Event recorded on the side stream behind the last kernel that wrote x (the consumer's stream must wait on it);
    failed: [(path, exception)] for the files of this stretch that could not be opened / decoded.  A batch may be empty
    (names == [], x is None) when every file of its stretch failed.

    The consumer enqueues batch n and only then asks for batch n + 1: the side stream uploads and resizes it while the consumer's
    stream is in the encoder.  Staging buffers recycle when the copy that read them has completed.
    """

    def __init__(self, pipe, paths, batch_size, resolution, workers=None, host_resize=False, transform=None, bucketing=None, labels=None,
                 max_pending=None):
        self.pipe, self.paths, self.bs, self.res = pipe, list(paths), max(1, int(batch_size)), int(resolution)
        self.host_resize = bool(host_resize)
        self.transform = transform
        self.bucketing, self.labels = bucketing, labels
        # bucket mode: images waiting in partly filled buckets, at most (4 batches by default; never less than one batch)
        self.max_pending = max(self.bs, int(max_pending) if max_pending is not None else 4 * self.bs)
        self.grouper = None
        self._bucket_transforms = {}
        self.workers = workers or default_workers()
        self.pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="vt-decode")
        self.side = torch.cuda.Stream(device=pipe.device)
        self.staging = _PinnedPool()
        self._busy = collections.deque()            # (event, [pinned buffers]) of uploads in flight
        self._next_submit = 0
        self._futures = collections.deque()
        self._window = self.workers + 2 * self.bs    # decoded images held at most (bounds host memory: ~3 MB each at 1024^2)

    # ---- worker side (no GPU calls) ----
    def _decode(self, p):
        from PIL import Image
        img = Image.open(p).convert("RGB")
        if self.bucketing is not None:
            bucket = self.bucketing.bucket_for_ratio(img.size[0] / img.size[1])
            if self.host_resize:
                return self._bucket_transform(bucket)(img), bucket      # fp32 [3,th,tw]: get_image_transform(res, True, bucket)
        elif self.host_resize:
            return self.transform(img)               # fp32 [3,res,res], the reference's get_image_transform
        a = np.asarray(img, dtype=np.uint8)
        h, w, _ = a.shape
        buf = self.staging.get(a.size)
        np.copyto(buf.numpy()[: a.size].reshape(h, w, 3), a)
        if self.bucketing is not None:
            return (buf, h, w), bucket
        return buf, h, w

    def _bucket_transform(self, bucket):
        tf = self._bucket_transforms.get(bucket)
        if tf is None:
            from .modules import get_image_transform
            tf = self._bucket_transforms[bucket] = get_image_transform(self.res, True, bucket)
        return tf

    def _submit_more(self):
        while self._next_submit < len(self.paths) and len(self._futures) < self._window:
            p = self.paths[self._next_submit]
            self._futures.append((p, self.pool.submit(self._decode, p)))
            self._next_submit += 1

    def _recycle(self, block=False):
        while self._busy and (block or len(self._busy) > 2 or self._busy[0][0].query()):
            ev, bufs = self._busy.popleft()
            ev.synchronize()
            for b in bufs:
                self.staging.put(b)

    def __iter__(self):
        if self.bucketing is not None:
            return self._iter_buckets()
        return self._iter_square()

    def _with_labels(self, names, x, ready, failed):
        """The batch tuple; with `labels`, the [b, N] fp32 label tensor of `names` rides along (uploaded on the side stream)."""
        if self.labels is None:
            return names, x, ready, failed
        y = None
        if names:
            rows = torch.stack([torch.as_tensor(self.labels[p], dtype=torch.float32) for p in names])
            with torch.cuda.stream(self.side):
                y = rows.pin_memory().to(self.pipe.device, non_blocking=True)
                ready = torch.cuda.Event()
                ready.record(self.side)
        return names, x, ready, failed, y

    def _iter_square(self):
        try:
            self._submit_more()
            while self._futures:
                take = [self._futures.popleft() for _ in range(min(self.bs, len(self._futures)))]
                self._submit_more()
                names, items, failed = [], [], []
                for p, f in take:
                    try:
                        items.append(f.result())
                        names.append(p)
                    except Exception as e:  # noqa: BLE001 - skip-and-count (infer_full.py:130-132)
                        failed.append((p, e))
                self._submit_more()
                if not names:
                    yield self._with_labels([], None, None, failed)
                    continue
                yield self._with_labels(names, *self._stage(items), failed)
                self._recycle()
        finally:
            self.close()

    # ---- bucket mode ----
    def _iter_buckets(self):
        """Decoded images are taken in path order and handed to the BucketGrouper; every group it releases is staged and yielded."""
        grouper = self.grouper = BucketGrouper(self.bs, self.max_pending)
        failed = []

        def emit(bucket, group):
            nonlocal failed
            names, x, ready = self._stage_bucket(bucket, [p for p, _ in group], [it for _, it in group], failed)
            out, failed = failed, []
            return self._with_labels(names, x, ready, out)

        try:
            self._submit_more()
            while self._futures:
                p, f = self._futures.popleft()
                self._submit_more()
                try:
                    item, bucket = f.result()
                except Exception as e:  # noqa: BLE001 - skip-and-count (infer_full.py:130-132)
                    failed.append((p, e))
                    continue
                for group in grouper.add(p, bucket, item):
                    yield emit(*group)
                    self._recycle()
            for group in grouper.flush():
                yield emit(*group)
                self._recycle()
            if failed:
                yield self._with_labels([], None, None, failed)
        finally:
            self.close()

    def _stage_bucket(self, bucket, names, items, failed):
        """One bucket's images -> (names, x [b,3,th,tw], ready).  Device route: the decoded pixels of the batch are uploaded into ONE raw
        buffer (an upload that fails costs that image: it is appended to `failed`) and resized + normalised by ONE load_batch call."""
        dev = self.pipe.device
        with torch.cuda.stream(self.side):
            if self.host_resize:
                x = torch.stack(items).to(dev)
            else:
                offs, total = [], 0
                for _, h, w in items:
                    offs.append(total)
                    total += (h * w * 3 + 255) // 256 * 256
                raw = torch.empty(total, dtype=torch.uint8, device=dev)
                kept, views, bufs = [], [], []
                for p, (buf, h, w), off in zip(names, items, offs):
                    n = h * w * 3
                    try:
                        raw[off: off + n].copy_(buf[:n], non_blocking=True)
                        views.append(raw[off: off + n].view(h, w, 3))
                        kept.append(p)
                    except Exception as e:  # noqa: BLE001 - skip-and-count: the upload of ONE image failed
                        failed.append((p, e))
                    bufs.append(buf)
                names = kept
                x = self.pipe.load_batch(views, bucket=bucket, tag="feeder_batch") if views else None
                ev = torch.cuda.Event()
                ev.record(self.side)
                self._busy.append((ev, bufs))
            ready = torch.cuda.Event()
            ready.record(self.side)
        return names, x, ready

    # ---- main thread: H2D + device resize / normalise on the side stream ----
    def _stage(self, items):
        dev = self.pipe.device
        with torch.cuda.stream(self.side):
            if self.host_resize:
                x = torch.stack(items).to(dev)                                   # pageable fp32: the reference's own route
            else:
                u8 = torch.empty(len(items), self.res, self.res, 3, dtype=torch.uint8, device=dev)
                bufs = []
                for k, (buf, h, w) in enumerate(items):
                    raw = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
                    raw.copy_(buf[: h * w * 3].view(h, w, 3), non_blocking=True)
                    self.pipe.resize_u8_into(raw, u8[k], self.pipe.FILTER_BILINEAR, tag="feeder")
                    bufs.append(buf)
                x = self.pipe.normalize_u8(u8)
                ev = torch.cuda.Event()
                ev.record(self.side)
                self._busy.append((ev, bufs))
            ready = torch.cuda.Event()
            ready.record(self.side)
        return x, ready

    def close(self):
        for _, f in self._futures:
            f.cancel()
        self._futures.clear()
        self.pool.shutdown(wait=True)
        self._recycle(block=True)


class FeederLoader:
    """A BatchFeeder with labels, seen as the loader evaluation.py expects: iterating yields {"pixel_values": x, "labels": y} with the
    consumer's CURRENT stream made to wait for the side stream's work on the batch.  Every iteration is a fresh pass over the paths
    (find_optimal_threshold and evaluate_model each make one).  `failed` collects the (path, exception) pairs of the last pass and
    `batches` its (names, shape) sequence; `len(loader.dataset)` bounds the number of samples (the evaluator sizes its store by it).
    An empty path list -- a rank without a share under `evaluate --sharded` -- yields no batch."""

    def __init__(self, pipe, paths, labels, batch_size, resolution, **feeder_kwargs):
        self.pipe, self.dataset, self.labels = pipe, list(paths), labels
        self.args = (batch_size, resolution)
        self.kwargs = feeder_kwargs
        self.failed, self.batches = [], []

    def __iter__(self):
        self.failed, self.batches = [], []
        feeder = BatchFeeder(self.pipe, self.dataset, *self.args, labels=self.labels, **self.kwargs)
        for names, x, ready, failed, y in feeder:
            self.failed.extend(failed)
            if not names:
                continue
            cur = torch.cuda.current_stream(self.pipe.device)
            cur.wait_event(ready)
            x.record_stream(cur)
            y.record_stream(cur)
            self.batches.append((list(names), tuple(x.shape)))
            yield {"pixel_values": x, "labels": y, "names": names}
