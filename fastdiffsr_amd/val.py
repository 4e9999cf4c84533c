"""The val phase of the reference's driver (`python sr_mfe.py -p val -c config/sr_fastdiffsr_test_64_256.json`,
FastDiffSR/sr_mfe.py:257-378) on the HIP engine:

    python -m fastdiffsr_amd.val -c config/sr_fastdiffsr_test_64_256.json [--batch 16] [--cond-from-lr]
    python -m fastdiffsr_amd.val -c config/sr_fastdiffsr_infer_x4.json --infer        # infer.py

    python -m fastdiffsr_amd.val -c ... --lpips-backbone alexnet-owt-7be5be79.pth --lpips-lin lpips/weights/v0.1/alex.pth
    python -m fastdiffsr_amd.val -c ... --fid-weights pt_inception-2015-12-05-6726825d.pth

Same config files, same dataset folders, same per-image metrics and log lines (MSE / PSNR / SSIM as
skimage.measure computes them, ERGAS as core/metrics.py:147-152), same `{results}/{step}_{idx}_sr.tif` outputs.
LPIPS (core/metrics.py:154-163, AlexNet + the v0.1 heads) is the reference's fifth metric: it needs the user's own weight
files and runs when asked for (`--lpips` looks where the reference's users have them, metrics.LPIPS.default_paths; or
`--lpips-backbone PATH --lpips-lin PATH`); the two log lines then carry `bic_lpips` / `sr_lpips` as the reference's do.
FID (FID.py, pytorch_fid's Inception pool3, dims=2048) is scored over the whole val set when asked for (`--fid` reads the
weights from pytorch_fid's hub cache, metrics.FID.default_path; `--fid-weights PATH`): `bic_fid` / `sr_fid` follow on the lines.
Differences, all opt-in or harmless:
  * `--batch N` samples N images per loop (the reference's val loader is batch 1 and its sampler crashes for
    more); every image is still its own independent chain
  * `continous=False`: the reference asks for the 8 intermediate frames and keeps only the last
  * `--cond-from-lr`: the conditioning image is resized from `lr_*` on the GPU (bit-identical to the offline PIL
    bicubic) instead of being read from `sr_*`
  * under `torch.distributed.run` the images are sharded over the ranks and the metric sums all-reduced
"""
import argparse
import itertools
import logging
import os
import queue
import sys
import threading
import time
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import torch

from . import metrics as M
from .config import load_config
from .data import lr_to_sr
from .dataset import create_dataset
from .model import create_model
from .parallel import host_threads_per_rank, shard_range

logger = logging.getLogger('base')


class HipOps:
    """The device side of the loop: uint8 batches in, model tensors / uint8 images / metric sums out, all on the GPU
    (csrc/fdsr_val.hip, fdsr_kernels.hip) -- there is no host implementation behind it.  run() takes the object as a parameter so
    that the sharding / reduction logic of the driver can be exercised on a GPU-less box with a stand-in the TESTS provide
    (tests/test_dist_gloo.py); the product always runs this one."""

    def __init__(self, device):
        if torch.device(device).type != 'cuda':
            raise RuntimeError('fastdiffsr_amd.val runs on the GPU only')
        import threading
        self.device = torch.device(device)
        self._cond = threading.Condition()
        self._owners = itertools.count(1)
        self._up = {}       # (owner, key, shape) -> ring of pinned staging buffers (H2D)
        self._down = {}     # (tag, shape, dtype) -> ring of pinned landing buffers (D2H)

    RING = 6            # pinned staging buffers per (owner, key, shape): more than any loader keeps staged ahead of its consumer (depth + 1 <= 4)
    STAGE_TIMEOUT = 120.0   # seconds a loader thread waits for a free staging buffer before it raises (a consumer that died with batches staged)

    def new_owner(self):
        """A token naming one loader's rings: monotonically increasing, never reused (id() of a dead loader can come back)."""
        with self._cond:
            return next(self._owners)

    def release(self, owner):
        """Drop the staging rings of a finished loader (pinned memory; a validation pass inside a training run makes a new loader
        every time).  Copies still in flight keep their buffers alive through the caching host allocator's stream bookkeeping."""
        with self._cond:
            for rkey in [k for k in self._up if k[0] == owner]:
                del self._up[rkey]
            self._cond.notify_all()

    def stage_host(self, key, arrays, owner=None):
        """Stack a batch's uint8 images (list of numpy arrays, or one stacked array) into a pinned staging buffer -- called on a
        LOADER thread, so that the sampling thread's share of the staging is one asynchronous copy.  A ring of RING buffers per
        (owner, key, shape); a buffer is OWNED by the batch staged into it until to_device() has issued its copy (batches may be
        staged out of order and stay staged for a while: a slot is never handed out again on call order alone), and rewritten only
        after that copy has completed.  `owner` names the loader: two loaders with the same batch shape never share a ring."""
        arr0 = arrays if isinstance(arrays, np.ndarray) else arrays[0]
        shape = tuple(arrays.shape) if isinstance(arrays, np.ndarray) else (len(arrays),) + tuple(arr0.shape)
        rkey = (owner, key, shape)
        with self._cond:
            ring = self._up.get(rkey)
            if ring is None:
                ring = self._up[rkey] = {'buf': [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(self.RING)],
                                         'ev': [None] * self.RING, 'held': [False] * self.RING, 'next': 0}
            while True:
                free = [(ring['next'] + i) % self.RING for i in range(self.RING) if not ring['held'][(ring['next'] + i) % self.RING]]
                if free:
                    break
                # every buffer holds a staged batch that has not been uploaded yet
                if not self._cond.wait(self.STAGE_TIMEOUT):
                    raise RuntimeError('no free staging buffer for %r after %.0f s: its %d staged batches were never uploaded '
                                       '(did the consumer stop?)' % (rkey, self.STAGE_TIMEOUT, self.RING))
            slot = free[0]
            ring['held'][slot] = True
            ring['next'] = (slot + 1) % self.RING
            ev = ring['ev'][slot]
        if ev is not None:
            ev.synchronize()
        dst = ring['buf'][slot].numpy()
        if isinstance(arrays, np.ndarray):
            dst[...] = arrays
        else:
            for j, a in enumerate(arrays):
                dst[j] = a
        return (rkey, slot)

    def to_device(self, staged):
        """The asynchronous H2D copy of a staged batch (sampling thread, current stream); releases the batch's hold on its buffer."""
        rkey, slot = staged
        ring = self._up[rkey]
        out = ring['buf'][slot].to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        with self._cond:
            ring['ev'][slot] = ev
            ring['held'][slot] = False
            self._cond.notify_all()
        return out

    def upload(self, key, arr):
        return self.to_device(self.stage_host(key, arr))

    to_tensor = staticmethod(M.u8_to_tensor)              # data/util.py:66-75 on the device
    tensor2img_batch = staticmethod(M.tensor2img_batch)   # core/metrics.py:16-42 on the device
    metric_sums = staticmethod(M.image_metric_sums)       # sr_mfe.py:313-345's per-pixel work on the device

    def lpips(self, model, truth_u8, test_a_u8, test_b_u8):
        """core/metrics.py:154-163 for both test images against one truth -> [2, B, 6] fp64 on the device (metrics.LPIPS)."""
        return model.lpips_u8(truth_u8, test_a_u8, test_b_u8)

    def fid_features(self, model, imgs_u8):
        """FID.py's pool3 features of each [B,H,W,3] uint8 batch in `imgs_u8`, stacked -> [len(imgs_u8) * B, 2048] fp32 on the
        device (metrics.FID)"""
        return model.features_u8(torch.cat(imgs_u8) if len(imgs_u8) > 1 else imgs_u8[0])

    def lr_to_sr(self, lr_u8, h, w):
        return lr_to_sr(lr_u8, h, w)

    def new_sums(self, b):
        return torch.empty(2, b, 8, dtype=torch.float64, device=self.device)

    def land(self, tag, slot, t):
        """Asynchronous D2H of `t` into pinned buffer `slot` of its ring; valid once the event of mark() has passed."""
        key = (tag, tuple(t.shape), t.dtype)
        ring = self._down.get(key)
        if ring is None:      # (setdefault would build -- and pin -- three buffers on EVERY call: 1.6 ms each, round 6)
            ring = self._down[key] = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for _ in range(3)]
        ring[slot].copy_(t, non_blocking=True)
        return ring[slot]

    def mark(self):
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def sync(self):
        torch.cuda.synchronize()


class _Loader:
    """The reference feeds its loop from a DataLoader (data/__init__.py:7-21: batch 1, one worker).  Here worker THREADS decode
    the image files of the next `depth` batches (PIL releases the GIL while it decodes) into uint8 arrays; the batch is stacked,
    crosses PCIe as bytes and becomes the model tensors on the device (ops.to_tensor, bit-identical to the dataset's own host
    transform)."""

    def __init__(self, dataset, lo, hi, batch, pool, ops, depth=2):
        self.ds, self.pool, self.depth, self.ops = dataset, pool, depth, ops
        self.owner = ops.new_owner() if hasattr(ops, 'new_owner') else id(self)
        self.batches = [list(range(b0, min(b0 + batch, hi))) for b0 in range(lo, hi, batch)]
        self.futs = {}
        self.next = 0

    def _collate(self, item_futs):
        """Loader thread: the batch's decoded images -> pinned staging buffers (its item jobs were queued before this job, so they are
        running or done: the wait cannot starve the pool)."""
        items = [f.result() for f in item_futs]
        out = {'Index': [it['Index'] for it in items]}
        for key in ('HR', 'SR', 'LR'):
            if key in items[0]:
                out[key] = self.ops.stage_host(key, [it[key] for it in items], owner=self.owner)
        return out

    def _submit_until(self, k):
        while self.next < len(self.batches) and self.next <= k:
            item_futs = [self.pool.submit(self.ds.load_u8, i) for i in self.batches[self.next]]
            self.futs[self.next] = self.pool.submit(self._collate, item_futs)
            self.next += 1

    def __len__(self):
        return len(self.batches)

    def close(self):
        """End of the pass (also an aborted one): wait for the collate jobs still queued, then give the staging rings back."""
        for f in list(self.futs.values()):
            try:
                f.result()
            except Exception:
                pass
        self.futs.clear()
        if hasattr(self.ops, 'release'):
            self.ops.release(self.owner)

    def prefetch(self, k):
        """Hand the decode + collate jobs of batches <= k to the pool.  Called by the loop right BEFORE it enters a long GPU call: the
        workers then run their Python sections while this thread sits in C without the GIL, instead of time-slicing it nine ways
        with this thread's own code (measured: 29 ms instead of 4 ms per batch on the sampling thread)."""
        self._submit_until(k)

    def get(self, k):
        """Batch k as {'HR','SR','LR': [B,H,W,3] uint8 device tensors (those the dataset has), 'Index': [...]}."""
        self._submit_until(k)
        staged = self.futs.pop(k).result()
        return {key: (v if key == 'Index' else self.ops.to_device(v)) for key, v in staged.items()}


def _prepare(opt, cond_from_lr, max_images, rank, world, diffusion, precision, rng, graph, step, epoch, fid_cache):
    """What a pass works on: the val set and this rank's shard of it, the model under the val schedule in the asked-for mode, the
    step / epoch it reports under, and how much of the FID reference the caller's cache already holds."""
    val_opt = opt['datasets']['val']
    dataset = create_dataset(val_opt, 'val', cond_from_lr=cond_from_lr)
    n_total = len(dataset) if max_images is None else min(len(dataset), max_images)
    lo, hi = shard_range(n_total, rank, world)
    rres = int(val_opt['r_resolution'])
    if diffusion is None:
        diffusion = create_model(opt)                                                 # sr_mfe.py:60
    diffusion.netG.precision = precision
    if rng is not None:
        diffusion.netG.rng = rng
    if graph is not None:
        diffusion.netG.graph = graph
    diffusion.set_new_noise_schedule(opt['model']['beta_schedule']['val'], schedule_phase='val')   # sr_mfe.py:66-67, :131-132
    fid_ref = fid_cache if fid_cache is not None else {}
    if fid_ref.get('images') not in (None, n_total):
        fid_ref.clear()                # another val set: its statistics do not apply
    return SimpleNamespace(dataset=dataset, n_total=n_total, lo=lo, hi=hi, rres=rres, scale=rres // int(val_opt['l_resolution']),
                           diffusion=diffusion, step=diffusion.begin_step if step is None else step,
                           epoch=diffusion.begin_epoch if epoch is None else epoch, fid_ref=fid_ref,
                           fid_sets=1 if 'hr' in fid_ref else 3)    # (HR, INF, SR) or, with the reference statistics cached, SR only


# The two sides scored against HR (the bicubic image, the sampled image) and the per-image fields of each.  A pass's columns are
# sides x fields (LPIPS, when on, is a fifth field): its rows, sums, `res` keys and log lines are all laid out from that list.
METRICS = (('bic', 'sr'), ('mse', 'psnr', 'ssim', 'ergas'))
# One batch's results on their way to the host: the pinned landing buffers of one slot (None: not asked for), valid once `event`
# has passed; the finisher sets `done` when it no longer reads them.
_Landed = namedtuple('_Landed', 'event idxs sr done sums hr inf lpips fid', defaults=(None,) * 5)


def _save(img, path):
    from PIL import Image
    Image.fromarray(img).save(path)


class _Finisher:
    """The thread behind the sampling loop: waits for a batch's copies, turns them into the reference's per-image numbers and hands
    the images to the pool to be written.  It owns its queue, the ring of landing slots and what it fills: per_image (index -> one
    number per column, zeros under infer), per_fid (index -> [fid_sets, D] fp32 features), saves (the write futures) and errors."""

    def __init__(self, pool, columns, save_images, infer, host_metrics, scale, result_path, current_step, fid_sets):
        self.pool, self.columns, self.save_images, self.infer, self.host_metrics = pool, columns, save_images, infer, host_metrics
        self.scale, self.result_path, self.current_step, self.fid_sets = scale, result_path, current_step, fid_sets
        self.per_image, self.per_fid, self.saves, self.errors, self.jobs = {}, {}, [], [], queue.Queue()
        self.slot_done = [None] * 3       # as many slots as HipOps.land keeps buffers per ring
        self.thread = threading.Thread(target=self._work, daemon=True)
        self.thread.start()

    def slot(self, k):
        """Batch k's landing slot, once the finisher is done with its previous contents (the sampling thread asks BEFORE it lands)."""
        slot = k % len(self.slot_done)
        if self.slot_done[slot] is not None:
            self.slot_done[slot].wait()
        return slot

    def put(self, slot, job):
        self.slot_done[slot] = job.done
        self.jobs.put(job)

    def close(self):
        self.jobs.put(None)
        self.thread.join()

    def _work(self):
        for job in iter(self.jobs.get, None):       # None: close()'s sentinel
            try:
                job.event.synchronize()
                sr_np = job.sr.numpy()
                fd = None if job.fid is None else job.fid.numpy().reshape(self.fid_sets, len(job.idxs), -1)
                for j, index in enumerate(job.idxs):
                    if fd is not None:
                        self.per_fid[index] = fd[:, j].copy()
                    if self.save_images:                                             # sr_mfe.py:274 counts from 1
                        name = '{}_{}_sr.{}'.format(self.current_step, index + 1, 'png' if self.infer else 'tif')
                        self.saves.append(self.pool.submit(_save, sr_np[j].copy(), '{}/{}'.format(self.result_path, name)))
                    self.per_image[index] = [0.0] * len(self.columns) if self.infer else self._row(job, j, sr_np[j])
            except Exception as e:       # surfaced by run() after the drain
                self.errors.append(e)
            finally:
                job.done.set()           # this slot's landing buffers may be refilled

    def _row(self, job, j, sr):
        """Image j of the batch as one number per column: from the device's sums, or (host_metrics) from the landed images."""
        if self.host_metrics:
            hr = job.hr.numpy()[j]
            m = {side: {'mse': M.compare_mse(t, hr), 'psnr': M.compare_psnr(t, hr), 'ssim': M.compare_ssim(t, hr),
                        'ergas': M.calculate_ergas(t, hr, scale=self.scale)}
                 for side, t in zip(METRICS[0], (job.inf.numpy()[j], sr))}
        else:
            m = {side: M.metrics_from_sums(job.sums.numpy()[s, j], sr.shape, self.scale) for s, side in enumerate(METRICS[0])}
        if job.lpips is not None:
            for s, side in enumerate(METRICS[0]):
                m[side]['lpips'] = float(job.lpips.numpy()[s, j, 0])                # sr_mfe.py:324, :345
        return [m[side][f] for side, f in self.columns]


def _score(ops, slot, hr_u8, inf_u8, sr_u8, host_metrics, lpips, fid, fid_sets):
    """One batch's metric work in stream order: the sums (host_metrics: the images), LPIPS, FID features, each landed into `slot`."""
    if host_metrics:
        out = dict(hr=ops.land('hr', slot, hr_u8), inf=ops.land('inf', slot, inf_u8))
    else:
        sums = ops.new_sums(len(sr_u8))
        ops.metric_sums(inf_u8, hr_u8, out=sums[0])
        ops.metric_sums(sr_u8, hr_u8, out=sums[1])
        out = dict(sums=ops.land('sums', slot, sums))
    if lpips is not None:
        out['lpips'] = ops.land('lpips', slot, ops.lpips(lpips, hr_u8, inf_u8, sr_u8))
    if fid is not None:
        out['fid'] = ops.land('fid', slot, ops.fid_features(fid, (hr_u8, inf_u8, sr_u8) if fid_sets == 3 else (sr_u8,)))
    return out


def _sample_batches(diffusion, loader, ops, finisher, clock, cond_from_lr, rres, infer, host_metrics, lpips, fid, fid_sets):
    """The sampling thread's loop -> seconds inside the sampling calls; clock['stage'] / ['post'] take its host seconds around them."""
    def stage(k):
        """Batch k on the device as the model tensors: issued BEFORE the previous batch is sampled, so the bytes are
        there when its loop ends (the copies and the two small kernels sit in front of that loop on the stream)."""
        if k >= len(loader):
            return None
        ts = time.perf_counter()
        raw = loader.get(k)
        idxs = raw.pop('Index')
        data = {key: ops.to_tensor(v) for key, v in raw.items()}
        if cond_from_lr:
            data['SR'] = ops.lr_to_sr(raw['LR'], rres, rres)
        clock['stage'] += time.perf_counter() - ts
        return idxs, data

    t_sample = 0.0
    loader.prefetch(1)
    staged = stage(0)
    for k in range(len(loader)):
        idxs, data = staged
        diffusion.feed_data(data)
        staged = stage(k + 1)
        loader.prefetch(k + 1 + loader.depth)
        ops.sync()
        t0 = time.time()
        diffusion.test(continous=False)
        ops.sync()
        t_sample += time.time() - t0
        logger.info('inference time (s): {:.4f} for {} image(s)'.format(time.time() - t0, len(idxs)))   # sr_mfe.py:279-284
        tp = time.perf_counter()
        sr_batch = diffusion.SR
        if sr_batch.dim() == 3:       # the ddpm / tesr siblings return ret_img[-1]: one image (their own convention)
            if len(idxs) != 1:
                raise ValueError("which_model_G in ('ddpm', 'tesr') returns one image per call: use --batch 1")
            sr_batch = sr_batch[None]
        sr_u8 = ops.tensor2img_batch(sr_batch)                                    # Metrics.tensor2img, on the device
        slot = finisher.slot(k)
        sr_host = ops.land('sr', slot, sr_u8)
        scores = {}
        if not infer:
            hr_u8 = ops.tensor2img_batch(diffusion.data['HR'])
            inf_u8 = ops.tensor2img_batch(diffusion.data['SR'])                   # the bicubic image ('INF')
            scores = _score(ops, slot, hr_u8, inf_u8, sr_u8, host_metrics, lpips, fid, fid_sets)
        finisher.put(slot, _Landed(ops.mark(), idxs, sr_host, threading.Event(), **scores))
        clock['post'] += time.perf_counter() - tp
    return t_sample


def _reduce(per_image, columns, world):
    """-> (images, {column name: average}) over all ranks; summed in index order, so the averages do not depend on the batch size."""
    sums = np.zeros(len(columns) + 1, dtype=np.float64)      # one sum per column, then the image count
    for index in sorted(per_image):
        sums += np.array(per_image[index] + [1.0])
    if world > 1:
        import torch.distributed as dist
        t = torch.from_numpy(sums).cuda() if dist.get_backend() == 'nccl' else torch.from_numpy(sums)
        dist.all_reduce(t)
        sums = t.cpu().numpy()
    return int(sums[-1]), {s + '_' + f: v for (s, f), v in zip(columns, sums[:-1] / max(sums[-1], 1.0))}


def run(opt, batch=1, cond_from_lr=False, precision='f16x3', results=None, max_images=None, rank=0, world=1,
        save_images=True, log=print, infer=False, diffusion=None, step=None, epoch=None, workers=None, rng=None, graph=None,
        host_metrics=False, ops=None, lpips=None, fid=None, fid_cache=None):
    """infer=True is the reference's infer.py (:62-110): the same loop, `{step}_{idx}_sr.png` outputs, timing, no metrics.
    diffusion: an existing model (the validation pass inside the training loop, sr_mfe.py:122-244); else one is created.

    The loop is a pipeline: loader threads decode the next batches while the GPU samples this one; tensor2img, MSE / PSNR /
    SSIM / ERGAS run on the device on the uint8 images (csrc/fdsr_val.hip; 2 x B x 8 doubles and the uint8 SR images come back
    through pinned memory), and a finisher thread turns the sums into the reference's per-image numbers and hands the images
    to the pool to be written -- none of which the sampling loop waits for.  host_metrics=True scores the landed uint8 images
    with metrics.compare_* instead (what the tests hold the device kernels against).
    rng: 'torch' (default; the reference's draws, reproducible under torch.manual_seed) or 'engine' (Philox inside the loop);
    graph: 'auto' | 'on' | 'off' -- replay the 20-step loop as a captured hipGraph (None: the model's default, 'auto').
    ops: the device side (HipOps; see there).
    lpips: a metrics.LPIPS, or None (the default: no LPIPS, the log lines and `res` exactly as without the feature).  With it
    every image also gets bic_lpips / sr_lpips from the device (host_metrics included: there is no host LPIPS).
    fid: a metrics.FID, or None (no FID).  With it the pool3 features of the HR, bicubic and SR uint8 images (the ones the
    metrics score and the .tif files hold) are kept per image index, gathered to rank 0 in index order, and bic_fid = FID(INF,
    HR), sr_fid = FID(SR, HR) are computed there in fp64 (FID.py's order: generated set first) and broadcast.
    fid_cache: a dict the caller keeps between passes over the same val set (the training loop): the HR / INF statistics and
    bic_fid are computed by the first pass and reused, later passes compute SR features only."""
    t_run0 = time.perf_counter()
    clock = {'stage': 0.0, 'post': 0.0}      # host seconds of this thread outside the sampling calls (returned in res['host_seconds'])
    lpips, fid = (None, None) if infer else (lpips, fid)         # infer.py scores nothing
    p = _prepare(opt, cond_from_lr, max_images, rank, world, diffusion, precision, rng, graph, step, epoch, fid_cache)
    result_path = results or (opt.get('path') or {}).get('results') or 'results'
    if save_images:
        os.makedirs(result_path, exist_ok=True)
    if ops is None:
        ops = HipOps(p.diffusion.device)
    columns = [(side, f) for side in METRICS[0] for f in METRICS[1] + (('lpips',) if lpips is not None else ())]
    # loader / writer threads of THIS rank: its share of the cores the job may use (affinity, cgroup quota, ranks on the host)
    n_workers = workers if workers else host_threads_per_rank(cap=8, floor=2)
    pool = ThreadPoolExecutor(max_workers=n_workers)
    finisher = _Finisher(pool, columns, save_images, infer, host_metrics, p.scale, result_path, p.step, p.fid_sets)
    # the sampling thread hands the GIL over around every launch / synchronisation; with Python's default 5 ms switch interval each
    # hand-back can cost it up to 5 ms while a loader / writer thread is in a Python section: ask for 0.2 ms while the loop runs
    old_switch = sys.getswitchinterval()
    sys.setswitchinterval(2e-4)
    clock['setup'] = time.perf_counter() - t_run0
    loader = None
    try:
        loader = _Loader(p.dataset, p.lo, p.hi, batch, pool, ops)
        t_sample = _sample_batches(p.diffusion, loader, ops, finisher, clock, cond_from_lr, p.rres, infer, host_metrics,
                                   lpips, fid, p.fid_sets)
    finally:
        tt = time.perf_counter()
        finisher.close()               # the drain, also of an aborted pass: the finisher first (it still queues writes)
        if loader is not None:
            loader.close()
        for f in finisher.saves:
            f.result()
        pool.shutdown(wait=True)
        sys.setswitchinterval(old_switch)
        clock['tail'] = time.perf_counter() - tt
    if finisher.errors:
        raise finisher.errors[0]
    images, averages = _reduce(finisher.per_image, columns, world)
    res = dict(images=images, **averages, sample_seconds_this_rank=t_sample, result_path=result_path,
               host_seconds=dict(clock, total=time.perf_counter() - t_run0, workers=n_workers))
    if fid is not None:
        tf = time.perf_counter()
        res.update(_fid_scores(finisher.per_fid, p.fid_ref, p.n_total, p.fid_sets, rank, world))
        res['host_seconds']['fid_statistics'] = time.perf_counter() - tf      # gather + fp64 statistics + sqrtm (rank 0)
    if rank == 0 and infer:
        log('inference: {} images, {:.4f} s per image on this rank (batch {})'.format(images, t_sample / max(p.hi - p.lo, 1), batch))
    elif rank == 0:       # sr_mfe.py:375-378 (and :230-235): one line per side, LPIPS last on it, then FID (FID.py) when asked for
        for side in METRICS[0]:
            names = [s + '_' + f for s, f in columns if s == side] + ([side + '_fid'] if fid is not None else [])
            log('<epoch:{:3d}, iter:{:8,d}> '.format(p.epoch, p.step) + ', '.join('{}: {:.5e}'.format(n, res[n]) for n in names))
    return res


def _fid_scores(per_fid, fid_ref, n_total, fid_sets, rank, world):
    """bic_fid / sr_fid of one pass: this rank's per-image features are gathered to rank 0, put in index order (so the value does
    not depend on the rank count or the batch), turned into fp64 statistics there and the two distances broadcast."""
    import torch.distributed as dist
    local = {i: per_fid[i] for i in sorted(per_fid)}
    if world > 1:
        parts = [None] * world if rank == 0 else None
        dist.gather_object(local, parts, dst=0)
        if rank == 0:
            for p in parts[1:]:
                local.update(p)
    out = [None]
    if rank == 0:
        feats = np.stack([local[i] for i in sorted(local)])          # [N, fid_sets, D], index order
        if fid_sets == 3:
            fid_ref.clear()
            fid_ref.update(images=n_total, hr=M.activation_statistics(feats[:, 0]))
            fid_ref['bic_fid'] = M.frechet_distance(*M.activation_statistics(feats[:, 1]), *fid_ref['hr'])
        sr = M.activation_statistics(feats[:, -1])
        out = [dict(bic_fid=fid_ref['bic_fid'], sr_fid=M.frechet_distance(*sr, *fid_ref['hr']))]
    if world > 1:
        dist.broadcast_object_list(out, src=0)
        if rank != 0 and fid_sets == 3:
            fid_ref.update(images=n_total, hr=None, bic_fid=out[0]['bic_fid'])    # later passes: SR features only, as on rank 0
    return out[0]


def add_fid_args(ap):
    ap.add_argument('--fid', action='store_true',
                    help="also score FID (FastDiffSR/FID.py: pytorch_fid, dims=2048) of the bicubic and SR images against HR, with "
                         "the weights where pytorch_fid caches them: torch.hub.get_dir()/checkpoints/pt_inception-2015-12-05-6726825d.pth")
    ap.add_argument('--fid-weights', default=None, metavar='PATH', help="pytorch_fid's FID Inception state dict (implies --fid)")


def fid_from_args(a):
    """The metrics.FID the flags ask for, or None.  Built once per run (a training run's val passes share it)."""
    if not (a.fid or a.fid_weights):
        return None
    return M.FID(a.fid_weights or M.FID.default_path())


def add_lpips_args(ap):
    ap.add_argument('--lpips', action='store_true',
                    help="also score LPIPS (the reference's calculate_lpips) with the weight files where the reference's users have "
                         "them: $TORCH_HOME/hub/checkpoints/alexnet-owt-7be5be79.pth and the lpips package's weights/v0.1/alex.pth")
    ap.add_argument('--lpips-backbone', default=None, metavar='PATH', help="torchvision's AlexNet state dict (implies --lpips)")
    ap.add_argument('--lpips-lin', default=None, metavar='PATH', help="lpips' v0.1 alex.pth heads (implies --lpips)")


def lpips_from_args(a):
    """The metrics.LPIPS the flags ask for, or None.  Built once per run (a training run's val passes share it)."""
    if not (a.lpips or a.lpips_backbone or a.lpips_lin):
        return None
    backbone, lin = a.lpips_backbone, a.lpips_lin
    if backbone is None or lin is None:
        d_backbone, d_lin = M.LPIPS.default_paths()
        backbone, lin = backbone or d_backbone, lin or d_lin
    return M.LPIPS(backbone, lin)


def main(argv=None, diffusion=None, ops=None):
    """diffusion / ops: injection points of tests/test_dist_gloo.py (a stand-in model and device side on a GPU-less box)."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('-c', '--config', required=True, help='JSON file for configuration (the reference\'s own)')
    ap.add_argument('-p', '--phase', choices=['val'], default='val')
    ap.add_argument('-gpu', '--gpu_ids', default=None)
    ap.add_argument('-debug', '-d', action='store_true')
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--cond-from-lr', action='store_true')
    ap.add_argument('--precision', default='f16x3', choices=['f32', 'f16x3', 'bf16', 'f16'])
    ap.add_argument('--results', default=None)
    ap.add_argument('--max-images', type=int, default=None)
    ap.add_argument('--no-save', action='store_true')
    ap.add_argument('--infer', action='store_true', help="the reference's infer.py: png outputs and timing, no metrics")
    ap.add_argument('--workers', type=int, default=None, help='loader / writer threads of this rank (default: its share of the usable cores, 2 .. 8)')
    ap.add_argument('--rng', default=None, choices=['torch', 'engine'],
                    help="sampling noise: 'torch' (default; torch.randn in the reference's order, reproducible under torch.manual_seed) "
                         "or 'engine' (Philox inside the HIP loop: nothing pre-drawn)")
    ap.add_argument('--graph', default=None, choices=['auto', 'on', 'off'],
                    help='replay the T-step loop as a captured hipGraph (default auto: from the second call of a shape on)')
    ap.add_argument('--host-metrics', action='store_true', help='score on the host (numpy) instead of the device kernels')
    add_lpips_args(ap)
    add_fid_args(ap)
    a = ap.parse_args(argv)
    rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
    if world > 1:
        from .parallel import init_process_group
        init_process_group()
    opt = load_config(a.config, phase=a.phase, gpu_ids=a.gpu_ids, debug=a.debug)
    log = print
    if not a.no_save and rank == 0 and (opt.get('path') or {}).get('log'):
        # sr_mfe.py:50-54: experiments/<name>_<timestamp>/logs/{train,val}.log; the two summary lines go to val.log
        from .config import setup_logger
        setup_logger(None, opt['path']['log'], 'train', screen=True)
        val_logger = setup_logger('val', opt['path']['log'], 'val')
        log = lambda msg: (print(msg), val_logger.info(msg))     # noqa: E731
        if a.results is None:
            a.results = opt['path'].get('results')
    lpips = None if a.infer else lpips_from_args(a)
    fid = None if a.infer else fid_from_args(a)
    res = run(opt, batch=a.batch, cond_from_lr=a.cond_from_lr, precision=a.precision, results=a.results,
              max_images=a.max_images, rank=rank, world=world, save_images=not a.no_save, infer=a.infer, log=log,
              workers=a.workers, rng=a.rng, graph=a.graph, host_metrics=a.host_metrics, diffusion=diffusion, ops=ops,
              lpips=lpips, fid=fid)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return res


if __name__ == '__main__':
    main()
