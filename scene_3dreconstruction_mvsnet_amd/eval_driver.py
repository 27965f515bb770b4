"""Sharded depth-generation driver: the MI355X counterpart of the reference's `save_depth`
(eval.py:283-500) for the files the downstream `filter_depth` stage reads.

Per sample it runs the drop-in MVSNet forward and writes, under `outdir`:
    {scan}/depth_est/{view:08d}.pfm     <- outputs["depth"][b]                  (eval.py:387)
    {scan}/confidence/{view:08d}.pfm    <- outputs["photometric_confidence"][b] (eval.py:392)
    {scan}/cams/{view:08d}_cam.txt      <- write_cam(K, E, ["000","2.5","",""]) (eval.py:396,107-126)
    {scan}/images/{view:08d}.png        <- uint8(ref image * 255), RGB          (eval.py:346-350)
with `filename = "{scan}/{{}}/{view:08d}{{}}"` as the reference datasets produce it
(datasets/dataloader_eval.py:176).  The grey PNG previews next to the PFMs (eval.py:388,393) are written with PIL (cv2 is absent; same
pixel values as cv2.imwrite would store).  Not reproduced (flagged, not silently changed): the
point-cloud accumulation of the debug view (eval.py:409-440, needs open3d).

Sharding replaces `nn.DataParallel` (eval.py:309): rank r of R processes dataset items r::R
(scene_3dreconstruction_mvsnet_amd.sharding); every rank writes its own files, so no collective is
needed here.  Loading + H2D of the next sample, the forward pass and the D2H + file encoding of the
previous ones run concurrently (loader thread + copy stream, compute stream, writer pool).

`reuse_features=True` keeps a device bank of FeatureNet outputs keyed by image path (FeatureSlots):
each view's image is copied to the device and run through FeatureNet once while it stays resident,
instead of once per sample that reads it (reference models/mvsnet.py:125).
"""
from __future__ import annotations

import os
import queue
import threading

import numpy as np
import torch
from PIL import Image

from . import data_io, sharding


def write_cam(file: str, K, R, depth_params) -> None:
    """cams/{view}_cam.txt in the layout the filter stage parses back (reference eval.py:107-126):
    an `extrinsic` block of four rows, an `intrinsic` block of three rows -- every number followed by
    one blank, as `str()` prints it -- and a last line with the four depth parameters."""
    def block(title, mat, n):
        rows = ["".join(str(mat[i][j]) + " " for j in range(n)) for i in range(n)]
        return title + "\n" + "\n".join(rows) + "\n\n"

    text = block("extrinsic", R, 4) + block("intrinsic", K, 3) + " ".join(str(p) for p in depth_params[:4]) + "\n"
    with open(file, "w") as f:
        f.write(text)


def _write_sample(job) -> None:
    outdir, filename, K, E, img, depth, conf = job
    t0 = _now()
    depth, conf = depth.numpy(), conf.numpy()                                  # utils.py:55
    depth_fn, conf_fn = data_io.depth_map_paths(outdir, filename)
    cam_fn = os.path.join(outdir, filename.format("cams", "_cam.txt"))
    img_fn = os.path.join(outdir, filename.format("images", ".png"))
    for fn in (depth_fn, conf_fn, cam_fn, img_fn):
        os.makedirs(os.path.dirname(fn), exist_ok=True)
    if img is not None:
        # eval.py:346-350: the two BGR<->RGB swaps there cancel, the file holds uint8(img*255) RGB
        # compress_level 1 = OpenCV's default IMWRITE_PNG_COMPRESSION (same pixels, 4x faster than 6)
        Image.fromarray(np.uint8(np.transpose(img, (1, 2, 0)) * 255)).save(img_fn, compress_level=1)
    data_io.save_pfm(depth_fn, depth)
    data_io.save_pfm(conf_fn, conf)
    # grey previews next to the PFMs (eval.py:388,393).  The reference writes them with cv2.imwrite:
    # depth as uint8(min-max normalised * 255); the confidence array is handed over as float32, which
    # OpenCV converts with saturate_cast<uchar> (round-half-even), i.e. to 0 / 1
    with np.errstate(all="ignore"):
        span = np.max(depth) - np.min(depth)
        prev = np.uint8((depth - np.min(depth)) / span * 255) if span > 0 else np.zeros(depth.shape, np.uint8)
    Image.fromarray(prev).save(depth_fn.replace(".pfm", ".png"), compress_level=1)
    Image.fromarray(np.uint8(np.clip(np.rint(conf), 0, 255))).save(conf_fn.replace(".pfm", ".png"), compress_level=1)
    if K is not None and E is not None:
        write_cam(cam_fn, K=K, R=E, depth_params=["000", "2.5", "", ""])
    _tick("writer.files", t0)


_TRACE = os.environ.get("MVS_DRIVER_TRACE") == "1"
_trace_lock = threading.Lock()
_trace = {}


def _tick(name, t0):
    """Accumulate wall time per driver stage (MVS_DRIVER_TRACE=1 prints the totals at the end)."""
    if _TRACE:
        import time
        with _trace_lock:
            _trace[name] = _trace.get(name, 0.0) + (time.perf_counter() - t0)


def _now():
    if _TRACE:
        import time
        return time.perf_counter()
    return 0.0


def _completer(cq: "queue.Queue", pool, futures: list, device, errors: list):
    """Single thread that copies each finished sample's maps to the host (own stream, ordered after
    the forward by an event) and hands them to the writer pool.  A failure is stored in `errors`
    (re-raised by save_depth_sharded); the thread then keeps draining the queue so that the
    producer never blocks on a full queue behind a dead consumer."""
    d2h = None
    while True:
        job = cq.get()
        if job is None:
            return
        if errors:
            continue
        try:
            if d2h is None:
                d2h = torch.cuda.Stream(device)
            done, out, payload = job
            t0 = _now()
            with torch.cuda.stream(d2h):
                d2h.wait_event(done)
                depth = out["depth"][0].to("cpu", non_blocking=False)
                conf = out["photometric_confidence"][0].to("cpu", non_blocking=False)
            _tick("completer.d2h", t0)
            futures.append(pool.submit(_write_sample, payload + (depth, conf)))
        except BaseException as e:  # noqa: BLE001 - re-raised by save_depth_sharded
            errors.append(e)


def _pin_pool_memory(pool) -> bool:
    """Page-lock the pool's shared-memory segment (hipHostRegister) so that the per-view copies to the
    device are DMA transfers at PCIe rate instead of staged pageable copies (~8 GB/s here).  The
    segment exists only after the pool's first item; returns whether it is pinned now."""
    shm = getattr(pool, "_shm", None)
    if shm is None or getattr(pool, "_pinned_name", None) == shm.name:
        return shm is not None
    import ctypes
    addr = ctypes.addressof(ctypes.c_char.from_buffer(shm.buf))
    cudart = torch.cuda.cudart()
    rc = cudart.cudaHostRegister(addr, shm.size, 0)
    if int(rc) != 0:
        return False            # not fatal: the copies stay pageable
    pool._pinned_name = shm.name

    def unpin():                # called by the pool's close() before it unmaps the segment
        cudart.cudaHostUnregister(addr)
        pool._pinned_name = None
    pool._unpin = unpin
    return True


def _decoded_samples(dataset, indices, decoders, decoder_pool):
    """Dataset items in order, decoded ahead of time: by the worker processes of a DecoderPool
    (yields (sample, release)), else by `decoders` helper threads (PIL's PNG/JPEG decoding releases
    the GIL; the numpy part does not, which caps this path at ~50 cfg2 maps/s)."""
    if decoder_pool is not None:
        for s in decoder_pool.imap(indices):
            yield s, (lambda s=s: decoder_pool.release(s))
        return
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=max(1, decoders)) as pool:
        ahead = 2 * max(1, decoders)
        futs = {}
        nxt = 0
        for pos in range(len(indices)):
            while nxt < len(indices) and nxt < pos + ahead:
                futs[nxt] = pool.submit(dataset.__getitem__, indices[nxt])
                nxt += 1
            yield futs.pop(pos).result(), (lambda: None)


class FeatureSlots:
    """Assigns the slots of a feature bank of `capacity` views to view keys (image paths), least
    recently used out.  Pure bookkeeping: `plan(keys)` for one sample returns
      slots  the bank slot of each of the sample's views (entry 0 = reference view), and
      new    [(i, slot)]: views not resident before, whose features must be written into `slot` from
             the sample's image i (once per distinct key, even if the sample repeats it).
    A view of the sample being planned is never evicted for another view of the same sample.
    """

    def __init__(self, capacity: int):
        if capacity < 1:
            raise ValueError(f"a feature bank needs at least one slot, got {capacity}")
        self.capacity = capacity
        self._slot_of = {}       # key -> slot, least recently used first
        self._free = list(range(capacity - 1, -1, -1))

    def plan(self, keys):
        keys = list(keys)
        if len(set(keys)) > self.capacity:
            raise ValueError(f"a sample with {len(set(keys))} distinct views does not fit a feature bank of "
                             f"{self.capacity} slots")
        mine = set(keys)
        slots, new = [], []
        for i, k in enumerate(keys):
            slot = self._slot_of.pop(k, None)
            if slot is None:
                if not self._free:
                    victim = next(v for v in self._slot_of if v not in mine)   # oldest entry of another sample
                    self._free.append(self._slot_of.pop(victim))
                slot = self._free.pop()
                new.append((i, slot))
            self._slot_of[k] = slot            # (re-)inserted last = most recently used
            slots.append(slot)
        return slots, new

    def resident(self):
        """Keys with a slot, least recently used first."""
        return list(self._slot_of)


def _loader(dataset, indices, device, copy_stream, q: "queue.Queue", decoders: int = 16, decoder_pool=None,
            keep_ref_image: bool = True, feature_slots: int = 0, extra_keys=()):
    """Producer thread: decoded samples (see _decoded_samples) are handed over in order and copied to
    the device on `copy_stream` while the GPU computes the previous sample.  The device list is
    [images, proj, depth_values] followed by the float32 arrays of `extra_keys` (e.g. GT depth and mask), each
    with a leading batch dimension of 1.
    feature_slots > 0 (reuse_features): the slot bookkeeping of the feature bank runs here, in sample
    order; only the images of views that are not resident are copied, and the item carries
    (new images or None, proj, depth_values) plus (their slots, the sample's slot ids)."""
    in_flight = []      # (copy-done event, release callback) of samples whose pinned-slot copies may still run
    planner = FeatureSlots(feature_slots) if feature_slots > 0 else None
    try:
        it = _decoded_samples(dataset, indices, decoders, decoder_pool)
        for pos, idx in enumerate(indices):
            while in_flight and in_flight[0][0].query():
                in_flight.pop(0)[1]()
            t0 = _now()
            s, release = next(it)
            _tick("loader.dataset_wait", t0)
            t0 = _now()
            per_view = isinstance(s["imgs"], (list, tuple))     # ViewDecoderPool: one shared-memory array per view
            pinned = False
            plan, pick = None, None
            if planner is not None:
                slot_ids, new = planner.plan([p for p, _ in dataset.view_plan(idx)[1]])
                pick = [i for i, _ in new]      # the sample's images that go to FeatureNet
                plan = ([slot for _, slot in new], slot_ids)
            # uint8 pixels (EvalDataset(image_dtype="uint8")) travel as they are: the model divides by 255 on the device
            u8 = (np.asarray(s["imgs"][0]) if per_view else np.asarray(s["imgs"])).dtype == np.uint8
            idt = torch.uint8 if u8 else torch.float32
            if per_view or pick == []:
                first = None                    # per-view copies below / every view resident
            elif pick is not None:
                first = torch.as_tensor(np.ascontiguousarray(np.asarray(s["imgs"])[pick]), dtype=idt)
            else:
                first = torch.as_tensor(np.asarray(s["imgs"]), dtype=idt)[None]
            src = [first] + \
                  [torch.as_tensor(np.asarray(s[k]), dtype=torch.float32)[None]
                   for k in ("proj_matrices", "depth_values") + tuple(extra_keys)]
            _tick("loader.prep", t0)
            t0 = _now()
            with torch.cuda.stream(copy_stream):
                # pageable -> device: the HIP runtime stages through its own pinned chunks; measured
                # faster here than an explicit host copy into a torch pinned buffer (1.5-2 GB/s)
                if per_view:   # N copies straight from the cache slots into the [1,N,3,H,W] device tensor
                    pinned = _pin_pool_memory(decoder_pool)
                    views = [torch.from_numpy(s["imgs"][i]) for i in (range(len(s["imgs"])) if pick is None else pick)]
                    small = [t.to(device) for t in src[1:]]   # pageable (synchronous) copies first: behind the
                    imgs_dev = None                           # asynchronous ones they would wait for them
                    if views:                                 # (reuse_features: [k,3,H,W], only the new views)
                        shape = ((1, len(views)) if pick is None else (len(views),)) + tuple(views[0].shape)
                        imgs_dev = torch.empty(shape, dtype=idt, device=device)
                        flat = imgs_dev[0] if pick is None else imgs_dev
                        for i, v in enumerate(views):
                            flat[i].copy_(v, non_blocking=pinned)
                    dev = [imgs_dev] + small
                else:
                    dev = [None if t is None else t.to(device) for t in src]
                ready = torch.cuda.Event()
                ready.record(copy_stream)
            _tick("loader.h2d", t0)
            if decoder_pool is not None:
                # what the writers need later (the reference image) is copied out before a slot is reused
                s = dict(s)
                s["imgs"] = np.array(s["imgs"][0])[None] if keep_ref_image else None
            if per_view and pinned:
                in_flight.append((ready, release))   # asynchronous copies from pinned slots: release when done
                while len(in_flight) > 4:
                    in_flight[0][0].synchronize()
                    in_flight.pop(0)[1]()
            else:
                release()                            # pageable copies have left the slot when .to() returns
            t0 = _now()
            q.put((idx, s, dev, ready, plan))
            _tick("loader.q_put", t0)
        for ev, rel in in_flight:
            ev.synchronize()
            rel()
    except BaseException as e:  # noqa: BLE001 - re-raised by the consumer
        q.put(e)
    q.put(None)


def _loaded(q: "queue.Queue", compute):
    """Consumer half of the pipeline: the items _loader put on `q`, in order, up to its closing None; an exception it
    forwarded is re-raised here.  Before an item is handed on, `compute` waits for the item's copies and its device
    tensors (allocated on the copy stream) are recorded on `compute`.  Yields (index, sample, device list, plan)."""
    while True:
        t0 = _now()
        item = q.get()
        _tick("main.q_get", t0)
        if item is None:
            return
        if isinstance(item, BaseException):
            raise item
        idx, s, dev, ready, plan = item
        compute.wait_event(ready)
        for t in dev:
            if t is not None:
                t.record_stream(compute)
        yield idx, s, dev, plan


def _check_reuse_features(model, dataset, first, feature_slots):
    """reuse_features' refusals about the model and the bank's size, made before any work starts (the caller has
    checked that the dataset has view_plan).  `first`: the indices whose view count the bank must hold."""
    if not all(hasattr(model, a) for a in ("extract_features", "forward_features")):
        raise ValueError("reuse_features needs a model with extract_features / forward_features (MVSNet)")
    n_max = max((len(dataset.view_plan(i)[1]) for i in first), default=0)
    if feature_slots < max(1, n_max):
        raise ValueError(f"feature_slots={feature_slots} is below the {n_max} views of one sample")


class _FeatureBank:
    """The device side of reuse_features: FeatureNet outputs [slots, 32, h, w], allocated at the first sample."""

    def __init__(self, model, slots, device):
        self.model, self.slots, self.device = model, slots, device
        self.bank = None

    def forward(self, dev, plan):
        """One sample's map from the bank: `dev` = [images of its new views or None, proj, depth_values] and `plan` =
        (the new views' slots, the sample's slot ids), as _loader hands them over.  Returns forward_features' dict."""
        # Slot reuse is safe because everything that touches the bank is enqueued here, on the one compute stream,
        # map by map in sample order: a slot the planner gave to a new view is overwritten only after every earlier
        # map that read its old view was enqueued.
        new_slots, slot_ids = plan
        if dev[0] is not None:
            feats = self.model.extract_features(dev[0])
            if self.bank is None:
                self.bank = torch.empty((self.slots,) + tuple(feats.shape[1:]), dtype=feats.dtype, device=self.device)
            elif self.bank.shape[1:] != feats.shape[1:]:
                raise RuntimeError(f"reuse_features: image size changed within the run (features "
                                   f"{tuple(feats.shape[1:])}, bank {tuple(self.bank.shape[1:])})")
            for j, slot in enumerate(new_slots):
                self.bank[slot].copy_(feats[j])
        return self.model.forward_features(self.bank, [slot_ids], dev[1], dev[2])


def save_depth_sharded(model, dataset, outdir: str, rank: int = 0, world: int = 1, device=None,
                       writers: int = 16, save_images: bool = True, decoders: int = 16, decoder_procs: int = 0,
                       decoder_pool=None, reuse_features: bool = False, feature_slots: int = 64):
    """Run `model` over dataset items rank::world and write the reference's per-view files.

    dataset[i] -> dict with "imgs" [N,3,H,W], "proj_matrices" [N,4,4], "depth_values" [D],
    "filename" and optionally "intrinsics" / "extrinsics" (lists; entry 0 = reference view), as
    the reference's eval datasets return them (datasets/dataloader_eval.py:171-176).
    Stages that overlap: `decoders` threads running dataset[i] ahead of time, a loader thread (H2D on
    a copy stream), the forward passes
    on the current stream, one completion thread (D2H of finished samples on its own stream) and
    `writers` threads that encode the PFM / PNG / cam files.  MVS_DRIVER_TRACE=1 prints where the
    host time went.  `decoder_procs` > 0 (or a ready `decoder_pool`) decodes in worker processes with a
    shared-memory ring instead of threads (decoder_pool.DecoderPool: the counterpart of the reference's
    DataLoader workers, eval.py:305).
    `reuse_features` runs FeatureNet once per view while the view stays in a device bank of
    `feature_slots` feature maps (keyed by image path from `dataset.view_plan`, least recently used
    out) and computes each map from that bank (model.extract_features / model.forward_features).  The
    files and the return value are byte-identical to reuse_features=False.  It needs a dataset with
    `view_plan` and at least one sample's views of slots.  Reuse happens within this rank's items: with
    the interleaved rank::world sharding, many ranks see few common views.
    Returns the list of dataset indices this rank processed.
    """
    device = device or torch.device("cuda", torch.cuda.current_device())
    mine = sharding.shard_units(len(dataset), rank, world)
    if reuse_features:   # refused before any work starts
        if not hasattr(dataset, "view_plan"):
            raise ValueError("reuse_features needs a dataset with view_plan() (image path of every view), "
                             "e.g. dataset_eval.EvalDataset")
        _check_reuse_features(model, dataset, mine[:1], feature_slots)
    model = model.to(device).eval()
    from concurrent.futures import ThreadPoolExecutor
    q: "queue.Queue" = queue.Queue(maxsize=4)
    with torch.cuda.device(device):
        copy_stream = torch.cuda.Stream(device)
        compute = torch.cuda.current_stream(device)
        own_pool = None
        if decoder_pool is None and decoder_procs > 0:
            from .decoder_pool import DecoderPool, ViewDecoderPool
            # datasets that can decode single views (EvalDataset) get the view-level pool: each image once
            by_view = all(hasattr(dataset, a) for a in ("view_plan", "decode_view", "assemble"))
            own_pool = decoder_pool = (ViewDecoderPool if by_view else DecoderPool)(dataset, procs=decoder_procs)
        th = threading.Thread(target=_loader, args=(dataset, mine, device, copy_stream, q, decoders, decoder_pool,
                                                    save_images, feature_slots if reuse_features else 0),
                              daemon=True)
        th.start()
        futures = []
        cq: "queue.Queue" = queue.Queue(maxsize=4 * max(1, writers))
        bank = _FeatureBank(model, feature_slots, device)    # used when reuse_features gives the items a plan
        with ThreadPoolExecutor(max_workers=max(1, writers)) as pool, torch.no_grad():
            errors: list = []
            comp = threading.Thread(target=_completer, args=(cq, pool, futures, device, errors), daemon=True)
            comp.start()
            try:
                for _, s, dev, plan in _loaded(q, compute):
                    if errors:      # the completer failed: stop enqueuing forwards
                        break
                    t0 = _now()
                    out = model(*dev) if plan is None else bank.forward(dev, plan)
                    _tick("main.forward_enqueue", t0)
                    t0 = _now()
                    done = torch.cuda.Event()
                    done.record(compute)
                    K = np.asarray(s["intrinsics"][0]) if "intrinsics" in s else None
                    E = np.asarray(s["extrinsics"][0]) if "extrinsics" in s else None
                    img = None
                    if save_images and s.get("imgs") is not None:
                        img = np.asarray(s["imgs"][0])
                        img = img.astype(np.float32) / np.float32(255.0) if img.dtype == np.uint8 else np.asarray(img, np.float32)
                    _tick("main.d2h_submit", t0)
                    t0 = _now()
                    cq.put((done, out, (outdir, s["filename"], K, E, img)))   # bounded: back-pressure
                    _tick("main.wait_writers", t0)
            finally:
                cq.put(None)
                comp.join()
            if errors:
                raise RuntimeError("save_depth_sharded: copying a finished depth map to the host / handing "
                                   "it to the writers failed; the output tree is incomplete") from errors[0]
            for f in futures:
                f.result()
        th.join()
        if own_pool is not None:
            own_pool.close()
    if _TRACE:
        print("[driver trace, seconds] " + ", ".join(f"{k}={v:.3f}" for k, v in sorted(_trace.items())), flush=True)
        _trace.clear()
    return mine
