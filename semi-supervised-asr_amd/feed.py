"""Input pipeline of the training loops.

The reference feeds a step with `for data in loader: xs, ilens, ys = to_gpu(data)` (solver.py:365-367, utils.py:154-158,
dataloader.py:6-12): collate on the host, then one synchronous pageable upload for the features and one per label tensor,
on the compute stream.  With every other host wait gone from the step (Solver._step) that upload was the last one: the
host could not enqueue step i + 1 before step i had drained.  `DeviceFeed` keeps the reference's batch (same order, same
zero padding, `ilens` a host list, `ys` a list of int64 tensors) and changes how it reaches HBM:

  * batches are collated ONE STEP AHEAD, straight into a ring of pinned host buffers (no intermediate padded tensor), by
    a background thread (or inline, `thread=False`);
  * the labels of a batch travel as ONE packed int64 tensor; the `ys` list handed to the model are views of it;
  * the upload runs on a side stream; the compute stream only waits for its event - which has long fired;
  * under data parallelism every rank pads and uploads ITS strided rows only (parallel.shard_indices) and takes the
    global constants the exact-parity rules need (B_global, T_max, olength, the judge's normaliser) from the
    lengths of the whole batch, which every rank sees (the samplers are seeded identically): a `parallel.LocalShard`.

The optional Gaussian input noise (solver.py:370-373) is drawn here and added on the host before the upload: one numpy
generator per GLOBAL row of a batch, seeded from (the feed's seed - taken from the process's numpy stream when the feed is
built, so data-parallel ranks agree -, the batch's index, the row).  A rank draws only the rows it uploads, and the union of
the rank-local batches is the one-process batch.

With a front end (`frontend=`, frontend.Frontend) an utterance's `feature` is a 1-D int16 or float32 WAVEFORM: the collate
packs this rank's samples into the pinned slot (longest first), uploads them on the side stream and runs the front end's
kernels there; the yielded `Batch` is the one a feed of precomputed features yields.  SpecAugment masks are drawn like the
noise - one generator per global row - and only in training feeds (`train=True`).

With `speed_perturb` in the front end's config a training feed also draws a speed factor per utterance (`plan_speed_batch`:
every rank draws the factors of ALL rows of the global batch, in collated order), sorts the batch by PERTURBED sample count,
takes `ilens`, `T_max` and the masks' `T_b` from the perturbed counts and uploads its own rows' raw samples with their factor
indices and output offsets; the resampler runs on the side stream in front of the fbank.  Validation, test and align feeds
never perturb.

With `reverb` or `noise` in the front end's config a training feed also draws, for each row it uploads, an RIR, a noise clip,
its start and an SNR (frontend.draw_augment on the row's COLLATED index, from `augment_seed`) and the two passes of
csrc/augment.hip run on the side stream between the resampler and the fbank.  Neither changes a sample count: the sort,
`ilens`, `T_max` and the masks are those of a feed without the keys.  Validation, test and align feeds never augment.
"""
import queue
import threading

import numpy as np
import torch

import parallel


class Batch(object):
    """One batch in HBM.  Unpacks like the reference's to_gpu(data): `xs, ilens, ys = batch` (speech-only: xs, ilens;
    text-only: iterating gives the label tensors).  Under data parallelism `xs` is a parallel.LocalShard (this rank's rows
    + the global constants), which the Solver's step methods accept wherever they accept the global tensor.
    `ys_host`: the labels as host lists (validation's references: no read back from the device)."""
    __slots__ = ("kind", "xs", "ilens", "ys", "ys_host")

    def __init__(self, kind, xs, ilens, ys, ys_host):
        self.kind, self.xs, self.ilens, self.ys, self.ys_host = kind, xs, ilens, ys, ys_host

    def __iter__(self):
        if self.kind == "text":
            return iter(self.ys)
        return iter((self.xs, self.ilens) if self.kind == "speech" else (self.xs, self.ilens, self.ys))

    def __len__(self):
        return len(self.ys) if self.kind == "text" else (2 if self.kind == "speech" else 3)


def _round_up(n, q):
    return (int(n) + q - 1) // q * q


class _Slot(object):
    """Pinned staging of one batch in flight: a float32 area (features, or float32 samples), an int64 area (labels), and -
    for a feed with a front end - an int16 area (samples) and a second int64 area (offsets, frame counts, masks), grown on
    demand."""

    def __init__(self, pin):
        self.pin, self.f, self.i, self.event = pin, None, None, None
        self.s, self.m = None, None

    def _area(self, old, n, dtype, quantum):
        if old is not None and old.numel() >= n:
            return old
        return torch.empty(_round_up(max(n, 1), quantum), dtype=dtype, pin_memory=self.pin)

    def floats(self, n):
        self.f = self._area(self.f, n, torch.float32, 1 << 18)
        return self.f[:n]

    def ints(self, n):
        self.i = self._area(self.i, n, torch.int64, 1 << 10)
        return self.i[:n]

    def shorts(self, n):
        self.s = self._area(self.s, n, torch.int16, 1 << 19)
        return self.s[:n]

    def meta(self, n):
        self.m = self._area(self.m, n, torch.int64, 1 << 10)
        return self.m[:n]


# Pinning host memory is slow (hipHostMalloc: of the order of 100 ms for the 8 MB of a cfg-2 batch), so the staging slots
# outlive the feed that first needed them: a feed borrows its slots for the length of one iteration (an epoch) and hands them
# back, and the next epoch's feed finds them pinned and large enough.
_SLOT_POOL = {True: [], False: []}
_SLOT_LOCK = threading.Lock()


def _borrow_slots(n, pin):
    with _SLOT_LOCK:
        free = _SLOT_POOL[pin]
        out = [free.pop() for _ in range(min(n, len(free)))]
    return out + [_Slot(pin) for _ in range(n - len(out))]


def _return_slots(slots):
    for slot in slots:
        if slot.event is not None:
            slot.event.synchronize()                    # its last upload has left the pinned area
            slot.event = None
    with _SLOT_LOCK:
        _SLOT_POOL[slots[0].pin].extend(slots)


def plan_speed_batch(frontend, speed_seed, batch_index, sample_counts):
    """Host arithmetic of a speed-perturbed batch.  sample_counts: the raw sample counts of ALL rows of the global batch in
    collated order -> (order, factor_index, perturbed): `order` sorts the rows by perturbed sample count descending (stable),
    and factor_index / perturbed are the draws (frontend.draw_speed on the COLLATED row, so the draw does not depend on the
    sort) and the perturbed counts IN THAT SORTED ORDER.  Every rank computes the same three lists and takes its strided
    rows of them, so the union of the rank-local batches is the one-process batch."""
    draws = [frontend.draw_speed(speed_seed, batch_index, i) for i in range(len(sample_counts))]
    counts = [frontend.perturbed_samples(n, f) for n, f in zip(sample_counts, draws)]
    order = sorted(range(len(counts)), key=lambda i: -counts[i])
    return order, [draws[i] for i in order], [counts[i] for i in order]


def draw_feed_seeds(frontend, train):
    """The seeds a feed with a front end takes from the process's numpy stream when it is built (the consumer's thread, so
    identically seeded data-parallel ranks agree) -> (mask seed, speed seed, augment seed), None where the feed does not draw.
    The order is fixed - masks, then speed, then reverb / noise - and a seed is taken only in a training feed whose front end
    has the feature on: the streams of every other feed stay where they are."""
    mask = int(np.random.randint(0, 2 ** 31 - 1)) if train and frontend.n_masks > 0 else None
    speed = int(np.random.randint(0, 2 ** 31 - 1)) if train and frontend.n_speeds > 0 else None
    augment = int(np.random.randint(0, 2 ** 31 - 1)) if train and frontend.augments else None
    return mask, speed, augment


class DeviceFeed(object):
    """Iterate `source` (batches of raw utterances: lists of (feature [T, D] float32, token_ids), in the collated order -
    dataloader.get_data_loader(raw=True), or any iterable of such lists) and yield `Batch`es on `device`, prepared `depth`
    batches ahead.

      kind        "labeled" (features + labels), "speech" (features only), "text" (labels only)
      rank/world  data-parallel position: world > 1 yields this rank's strided rows as a parallel.LocalShard
      noise_std   > 0: add N(0, noise_std) noise to the features (a generator per global row, see the module docstring)
      thread      collate + upload in a background thread (default) or inline in next()
      frontend    a frontend.Frontend: features are 1-D waveforms and the front end runs on the side stream (GPU only)
      train       with a front end that has SpecAugment masks: draw them; with one that has `speed_perturb`: draw a speed
                  factor per utterance and resample; with one that has `reverb` / `noise`: draw and apply them (training
                  feeds only)
    """

    def __init__(self, source, device, kind="labeled", rank=0, world=1, depth=2, noise_std=0.0, thread=True, frontend=None,
                 train=False):
        assert kind in ("labeled", "speech", "text")
        self.frontend = frontend
        if frontend is not None:
            if torch.device(device).type != "cuda":
                raise RuntimeError("DeviceFeed: the front end runs on the GPU only: the HIP path has no CPU fallback")
            if float(noise_std) > 0:
                raise ValueError("DeviceFeed: the host-side input noise needs precomputed features (noise_std with a front end)")
            self.mask_seed, self.speed_seed, self.augment_seed = draw_feed_seeds(frontend, train)
        self.source, self.kind, self.rank, self.world = source, kind, int(rank), int(world)
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        if self.cuda and self.device.index is None:      # the producer thread needs the index (set_device)
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.depth = max(1, int(depth))
        self.noise_std = float(noise_std)
        # the noise seed: taken from the process's numpy stream HERE (the consumer's thread), so that identically seeded
        # data-parallel ranks draw identical noise whatever the interleaving of the threads
        self.noise_seed = int(np.random.randint(0, 2 ** 31 - 1)) if self.noise_std > 0 else None
        self.thread = bool(thread)
        self._slots = None                               # borrowed for the length of one iteration
        self._side = torch.cuda.Stream(device=self.device) if self.cuda else None
        self._n = 0

    def __len__(self):
        return len(self.source)

    # ---------------------------------------------------------------- one batch: host lists -> pinned -> device
    def _prepare(self, items):
        """-> (Batch, copy-done event or None).  Runs in the producer (thread or inline)."""
        if self.frontend is not None and self.kind != "text":
            return self._prepare_waveforms(items)
        slot = self._slots[self._n % len(self._slots)]
        self._n += 1
        if slot.event is not None:
            slot.event.synchronize()                    # the upload that last read this pinned area has finished
            slot.event = None
        rows = parallel.shard_indices(len(items), self.rank, self.world)
        sharded = self.world > 1
        xs_h = ys_h = None
        ilens = ys_lens = ys_host = None
        info = dict(b_global=len(items))
        if self.kind != "text":
            lens_all = [int(f.shape[0]) for f, _ in items]
            t_max = max(lens_all)
            dim = int(items[0][0].shape[1])
            ilens = [lens_all[i] for i in rows]
            xs_h = slot.floats(len(rows) * t_max * dim).view(len(rows), t_max, dim)
            xs_n = xs_h.numpy()                          # (numpy row assignments: a third less host time than tensor copies,
            for r, i in enumerate(rows):                 #  and they release the GIL)
                n = lens_all[i]
                xs_n[r, :n] = items[i][0]
                xs_n[r, n:] = 0.0
            if self.noise_seed is not None:
                # one generator per GLOBAL row, seeded from (feed, batch, row): a rank draws its own rows only - the work
                # per rank does not grow with the world size - and every rank would draw the same values for a given row
                for r, i in enumerate(rows):
                    rs = np.random.RandomState([self.noise_seed, self._n - 1, i])
                    xs_n[r] += rs.normal(0.0, self.noise_std, (t_max, dim)).astype(np.float32)
            info.update(t_max=t_max, olength=None)
        if self.kind != "speech":
            tok_all = [items[i][1] for i in range(len(items))]
            len_all = [len(t) for t in tok_all]
            ys_lens = [len_all[i] for i in rows]
            ys_host = [list(tok_all[i]) for i in rows]
            ys_h = slot.ints(sum(ys_lens))
            if ys_lens:
                ys_h.numpy()[:] = np.concatenate([np.asarray(t, dtype=np.int64) for t in ys_host]) if sum(ys_lens) else 0
            info.update(olength=max(len_all) + 1, text_norm=float(sum(n + 5 for n in len_all)))
        event = None
        if self.cuda:
            with torch.cuda.stream(self._side):
                xs_d = xs_h.to(self.device, non_blocking=True) if xs_h is not None else None
                ys_d = ys_h.to(self.device, non_blocking=True) if ys_h is not None else None
                event = torch.cuda.Event()
                event.record(self._side)
            slot.event = event
        else:
            xs_d = xs_h.clone() if xs_h is not None else None      # (CPU: tests of the host logic)
            ys_d = ys_h.clone() if ys_h is not None else None
        ys = list(torch.split(ys_d, ys_lens)) if ys_d is not None else None       # views of the one label tensor
        flat = (xs_d, ys_d)
        if sharded:
            xs_out = parallel.LocalShard(xs_d, ilens, ys, info)
        else:
            xs_out = xs_d
        return Batch(self.kind, xs_out, ilens, ys, ys_host), event, flat

    def _prepare_waveforms(self, items):
        """_prepare for a feed with a front end: samples -> pinned -> device -> features, all on the side stream."""
        fe = self.frontend
        slot = self._slots[self._n % len(self._slots)]
        self._n += 1
        if slot.event is not None:
            slot.event.synchronize()
            slot.event = None
        speed = self.speed_seed is not None
        if speed:
            # perturbed sample count descending (stable); n_all stays the RAW count of a row, p_all is what the fbank sees
            order, f_all, p_all = plan_speed_batch(fe, self.speed_seed, self._n - 1, [int(f.shape[0]) for f, _ in items])
        else:
            order = sorted(range(len(items)), key=lambda i: -int(items[i][0].shape[0]))   # sample count descending (stable)
        items = [items[i] for i in order]
        rows = parallel.shard_indices(len(items), self.rank, self.world)
        sharded = self.world > 1
        n_all = [int(f.shape[0]) for f, _ in items]
        if not speed:
            p_all = n_all
        lens_all = [fe.num_frames(n) for n in p_all]
        t_max = max(lens_all)
        if t_max < 1:
            raise ValueError("DeviceFeed: no utterance of the batch has a whole frame")
        ilens = [lens_all[i] for i in rows]
        B, nm = len(rows), (fe.n_masks if self.mask_seed is not None else 0)
        short = np.asarray(items[0][0]).dtype == np.int16
        total = sum(n_all[i] for i in rows)
        wav_h = slot.shorts(total) if short else slot.floats(total)
        wav_n = wav_h.numpy()
        offs = [0]
        for i in rows:
            wav_n[offs[-1]:offs[-1] + n_all[i]] = items[i][0]
            offs.append(offs[-1] + n_all[i])
        # one int64 area: offsets [B + 1] | frame counts int32 [B] (padded to a whole word) | masks int32 [B, nm, 2]; with
        # speed perturbation behind them: output offsets [B + 1] | factor indices int32 [B] (padded to a whole word); with
        # reverb / noise behind those: RIR indices int32 [B] | clip indices int32 [B] | scales float32 [B] (each padded to a
        # whole word) | noise starts int64 [B]
        augment = self.augment_seed is not None
        lw = (B + 1) // 2
        base = B + 1 + lw + B * nm
        abase = base + (B + 1 + lw if speed else 0)
        meta_h = slot.meta(abase + (3 * lw + B if augment else 0))
        meta_n = meta_h.numpy()
        meta_n[:B + 1] = offs
        meta_n[B + 1:] = 0
        i32 = meta_n[B + 1:base].view(np.int32)
        i32[:B] = ilens
        if speed:
            meta_n[base:base + B + 1] = np.concatenate([[0], np.cumsum([p_all[i] for i in rows])])
            meta_n[base + B + 1:abase].view(np.int32)[:B] = [f_all[i] for i in rows]
        if augment:
            # a rank draws its own rows only, each by its index in the collated batch: the draw does not depend on the sort
            draws = [fe.draw_augment(self.augment_seed, self._n - 1, order[i]) for i in rows]
            meta_n[abase:abase + lw].view(np.int32)[:B] = [a[0] for a in draws]
            meta_n[abase + lw:abase + 2 * lw].view(np.int32)[:B] = [a[1] for a in draws]
            meta_n[abase + 2 * lw:abase + 3 * lw].view(np.float32)[:B] = [fe.snr_scale(a[3]) for a in draws]
            meta_n[abase + 3 * lw:abase + 3 * lw + B] = [a[2] for a in draws]
        if nm:
            for r, i in enumerate(rows):
                i32[2 * lw + r * nm * 2:2 * lw + (r + 1) * nm * 2] = fe.draw_masks(self.mask_seed, self._n - 1, i,
                                                                                   lens_all[i]).reshape(-1)
        ys_h = ys_lens = ys_host = None
        info = dict(b_global=len(items), t_max=t_max, olength=None)
        if self.kind != "speech":
            tok_all = [items[i][1] for i in range(len(items))]
            len_all = [len(t) for t in tok_all]
            ys_lens = [len_all[i] for i in rows]
            ys_host = [list(tok_all[i]) for i in rows]
            ys_h = slot.ints(sum(ys_lens))
            if ys_lens:
                ys_h.numpy()[:] = np.concatenate([np.asarray(t, dtype=np.int64) for t in ys_host]) if sum(ys_lens) else 0
            info.update(olength=max(len_all) + 1, text_norm=float(sum(n + 5 for n in len_all)))
        with torch.cuda.stream(self._side):
            wav_d = wav_h.to(self.device, non_blocking=True)
            meta_d = meta_h.to(self.device, non_blocking=True)
            ys_d = ys_h.to(self.device, non_blocking=True) if ys_h is not None else None
            i32_d = meta_d[B + 1:base].view(torch.int32)
            masks_d = i32_d[2 * lw:2 * lw + B * nm * 2].view(B, nm, 2) if nm else None
            speed_d = None
            if speed:
                speed_d = (meta_d[base + B + 1:abase].view(torch.int32)[:B], meta_d[base:base + B + 1],
                           sum(p_all[i] for i in rows), max(p_all[i] for i in rows))
            augment_d = None
            if augment:
                augment_d = (meta_d[abase:abase + lw].view(torch.int32)[:B], meta_d[abase + lw:abase + 2 * lw].view(torch.int32)[:B],
                             meta_d[abase + 3 * lw:abase + 3 * lw + B], meta_d[abase + 2 * lw:abase + 3 * lw].view(torch.float32)[:B],
                             sum(p_all[i] for i in rows), max(p_all[i] for i in rows))
            xs_d = fe.run(wav_d, meta_d[:B + 1], i32_d[:B], t_max, masks_d, speed_d, augment_d)
            event = torch.cuda.Event()
            event.record(self._side)
        slot.event = event
        ys = list(torch.split(ys_d, ys_lens)) if ys_d is not None else None
        xs_out = parallel.LocalShard(xs_d, ilens, ys, info) if sharded else xs_d
        return Batch(self.kind, xs_out, ilens, ys, ys_host), event, (xs_d, ys_d)

    def _hand_over(self, prepared):
        """Consumer side: order the compute stream behind the upload and tell the allocator who uses the memory."""
        batch, event, flat = prepared
        if event is not None:
            main = torch.cuda.current_stream(self.device)
            main.wait_event(event)
            for t in flat:
                if t is not None:
                    t.record_stream(main)
        return batch

    # ---------------------------------------------------------------- iteration
    def __iter__(self):
        if not self.thread:
            return self._iter_inline()
        return self._iter_threaded()

    def _iter_inline(self):
        ahead = []
        self._slots = _borrow_slots(self.depth + 2, self.cuda)
        try:
            for items in self.source:
                ahead.append(self._prepare(items))
                if len(ahead) > self.depth - 1:
                    yield self._hand_over(ahead.pop(0))
            while ahead:
                yield self._hand_over(ahead.pop(0))
        finally:
            slots, self._slots = self._slots, None
            _return_slots(slots)

    def _iter_threaded(self):
        q = queue.Queue(maxsize=self.depth)
        stop = threading.Event()
        done = object()

        def put(x):
            while not stop.is_set():
                try:
                    q.put(x, timeout=0.1)
                    return True
                except queue.Full:
                    continue
            return False

        def produce():
            try:
                if self.cuda:
                    torch.cuda.set_device(self.device)
                for items in self.source:
                    if not put(self._prepare(items)):
                        return
                put(done)
            except BaseException as exc:                 # surfaces in the consumer
                put(exc)

        self._slots = _borrow_slots(self.depth + 2, self.cuda)
        worker = threading.Thread(target=produce, name="asr-device-feed", daemon=True)
        worker.start()
        try:
            while True:
                item = q.get()
                if item is done:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield self._hand_over(item)
        finally:
            stop.set()                                   # the consumer left early (break / exception): release the producer
            # the producer may be inside _prepare; let it finish so that no upload is in flight from a slot we drop
            worker.join(timeout=5.0)
            slots, self._slots = self._slots, None
            if not worker.is_alive():                    # (a producer stuck in its source keeps its slots: they are dropped)
                _return_slots(slots)
