"""The reference's TEST pipeline for a batch of images, on the device, built from the config's own list:

    LoadImageFromFile -> MultiScaleFlipAug(img_scale | scale_factor, flip, flip_direction, transforms=[
        Resize(keep_ratio=True), RandomFlip, Normalize(0, 1), Pad(size | size_divisor, pad_val=0),
        ImageToTensor | DefaultFormatBundle, Collect])
    (configs/yunet_n.py:57-102 there, mmdet/datasets/pipelines/test_time_aug.py:54-114, transforms.py:643-703)

    pipe = DeviceTestPipeline(cfg.data.test.pipeline)
    src = TestSource(dataset, cache='device', device=dev)          # decoded once, kept across evaluations
    img, metas = pipe(src.fetch(idx), view=0)                      # [N, 3, Hc, Wc] fp32, one launch (yunet_test_pixels)

The geometry (resized size, padded shape, scale_factor) is host arithmetic on the (h, w) table; the pixels are one
launch of csrc/test_pipeline.hip.  At B = 1 the tensor and the metas are those of evaluation.prepare_test_image.
`run_test` is what evaluation.single_gpu_test / multi_gpu_test run when samples_per_gpu, pipeline or
cache is given.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import imresize

INNER_ORDER = ['Resize', 'RandomFlip', 'Normalize', 'Pad', 'ImageToTensor', 'Collect']


def _is_scale(v):
    return isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(x, (int, float, np.integer)) for x in v)


def round_up(v, d):
    return (int(v) + d - 1) // d * d


class DeviceTestPipeline:
    """Parses the list (raising, with the reason, for what the kernel does not implement) and runs it.

    `pipeline` None / [] or a MultiScaleFlipAug with transforms=[]: the pipeline evaluation.prepare_test_image
    hard-codes (one view at `scale`, zero padding up to the scale and to a multiple of 32).

    views: [(scale, flip)] in the reference's loop order (for scale: for flip), scale = an (a, b) tuple
    (mmcv.imrescale: long / short edge), a float factor, or None (original size).
    pad: ('scale',) = prepare_test_image's rule (up to the view's own scale), ('size', (a, b)), ('divisor', d)."""

    def __init__(self, pipeline=None, scale=(640, 640)):
        self.views = [(tuple(scale) if scale is not None else None, False)]
        self.pad = ('scale',)
        self.pad_fixed_size, self.pad_size_divisor = None, None
        self.batched_bundle = False
        msfa = self._outer(pipeline or [])
        if msfa is not None:
            self._views(msfa)
            if msfa.get('transforms'):
                self._inner(msfa['transforms'])

    # ------------------------------------------------------------------ parsing
    @staticmethod
    def _outer(pipeline):
        names = [t.get('type') for t in pipeline]
        for n in set(names):
            if names.count(n) > 1:
                raise NotImplementedError(f'DeviceTestPipeline: {n} appears {names.count(n)} times in {names}')
        unknown = [n for n in names if n not in ('LoadImageFromFile', 'MultiScaleFlipAug')]
        if unknown:
            raise NotImplementedError(f'DeviceTestPipeline implements LoadImageFromFile -> MultiScaleFlipAug(transforms='
                                      f'{INNER_ORDER}); {unknown} is not built')
        if not names:
            return None
        if 'MultiScaleFlipAug' not in names or names[-1] != 'MultiScaleFlipAug':
            raise NotImplementedError(f'DeviceTestPipeline: the list must end in MultiScaleFlipAug, got {names}')
        return pipeline[-1]

    def _views(self, m):
        known = {'type', 'img_scale', 'scale_factor', 'flip', 'flip_direction', 'transforms'}
        extra = sorted(set(m) - known)
        if extra:
            raise NotImplementedError(f'MultiScaleFlipAug options {extra} are not built')
        img_scale, factor = m.get('img_scale'), m.get('scale_factor')
        if (img_scale is None) == (factor is None):       # test_time_aug.py:60-61
            raise ValueError('MultiScaleFlipAug: exactly one of img_scale and scale_factor must be given')
        if img_scale is not None:
            scales = [tuple(img_scale)] if _is_scale(img_scale) else [tuple(s) for s in img_scale]
            if not scales or not all(_is_scale(s) and min(s) >= 1 for s in scales):
                raise ValueError(f'MultiScaleFlipAug(img_scale={img_scale!r}): (a, b) tuples of positive sizes')
            scales = [tuple(int(v) for v in s) for s in scales]
        else:
            scales = [float(f) for f in (factor if isinstance(factor, (list, tuple)) else [factor])]
            if not scales or not all(np.isfinite(f) and f > 0 for f in scales):
                raise ValueError(f'MultiScaleFlipAug(scale_factor={factor!r}): positive finite factors')
        flip = bool(m.get('flip', False))
        direction = m.get('flip_direction', 'horizontal')
        directions = list(direction) if isinstance(direction, (list, tuple)) else [direction]
        if flip and directions != ['horizontal']:
            raise NotImplementedError(f"MultiScaleFlipAug(flip_direction={direction!r}): only 'horizontal' is built")
        self.views = [(s, f) for s in scales for f in ([False, True] if flip else [False])]

    def _inner(self, transforms):
        names = ['ImageToTensor' if t.get('type') == 'DefaultFormatBundle' else t.get('type') for t in transforms]
        for n in set(names):
            if names.count(n) > 1:
                raise NotImplementedError(f'MultiScaleFlipAug.transforms: {n} appears {names.count(n)} times')
        unknown = [n for n in names if n not in INNER_ORDER]
        if unknown:
            raise NotImplementedError(f'MultiScaleFlipAug.transforms: {unknown} is not built (implemented: {INNER_ORDER} '
                                      f'/ DefaultFormatBundle)')
        if names != [n for n in INNER_ORDER if n in names]:
            raise NotImplementedError(f'MultiScaleFlipAug.transforms must keep the order {INNER_ORDER}, got {names}')
        cfg = {n: dict(t) for n, t in zip(names, transforms)}
        if 'Resize' not in cfg:
            raise NotImplementedError('MultiScaleFlipAug.transforms needs Resize(keep_ratio=True)')
        r = cfg['Resize']
        if not r.get('keep_ratio', True):
            raise NotImplementedError('Resize(keep_ratio=False) in the test pipeline: only keep_ratio=True is built')
        if r.get('img_scale') is not None or r.get('ratio_range') is not None:
            raise NotImplementedError('Resize inside MultiScaleFlipAug takes its scale from the wrapper (img_scale / '
                                      'ratio_range must not be set)')
        if r.get('interpolation', 'bilinear') != 'bilinear':
            raise NotImplementedError(f"Resize(interpolation={r.get('interpolation')!r}): only 'bilinear' is built")
        if any(f for _, f in self.views):
            if 'RandomFlip' not in cfg:
                raise ValueError('MultiScaleFlipAug(flip=True) without RandomFlip in its transforms flips nothing')
            if cfg['RandomFlip'].get('direction', 'horizontal') != 'horizontal':
                raise NotImplementedError("RandomFlip(direction=...): only 'horizontal' is built")
        if 'Normalize' in cfg:
            from .pipelines import Normalize
            n = cfg['Normalize']
            Normalize(n.get('mean', [0.0]), n.get('std', [1.0]), n.get('to_rgb', True))      # same rule and message
        self.pad = ('divisor', 32)            # no Pad: the collate alone pads (and the stack needs multiples of 32)
        if 'Pad' in cfg:
            p = cfg['Pad']
            if p.get('pad_to_square', False):
                raise NotImplementedError('Pad(pad_to_square=True) is not built')
            pv = p.get('pad_val', 0)
            pv = pv.get('img', 0) if isinstance(pv, dict) else pv
            if float(pv) != 0.0:
                raise NotImplementedError(f'Pad(pad_val={pv!r}): the kernel pads with 0 (as the collate does)')
            size, div = p.get('size'), p.get('size_divisor')
            if (size is None) == (div is None):       # transforms.py:659-660
                raise ValueError('Pad: exactly one of size and size_divisor must be given')
            if size is not None:
                if not _is_scale(size) or min(size) < 1:
                    raise ValueError(f'Pad(size={size!r}): an (a, b) tuple of positive sizes')
                self.pad = ('size', (int(size[0]), int(size[1])))
                self.pad_fixed_size = self.pad[1]
            else:
                if int(div) < 1:
                    raise ValueError(f'Pad(size_divisor={div!r})')
                self.pad = ('divisor', int(div))
                self.pad_size_divisor = int(div)
        self.batched_bundle = any(t.get('type') == 'DefaultFormatBundle' for t in transforms)

    # ------------------------------------------------------------------ geometry (host)
    def geometry(self, h, w, view=0):
        """-> (nh, nw, ph, pw) of an h x w image in view `view`: the resized size (mmcv.imrescale) and the padded shape,
        computed as evaluation.prepare_test_image computes them (a Pad size is read as it reads the scale: [0] against
        the height, [1] against the width; an image larger than the size is not cropped), rounded up to 32."""
        scale, _ = self.views[view]
        h, w = int(h), int(w)
        if scale is None:
            nh, nw = h, w
        elif isinstance(scale, float):
            nw, nh = int(w * scale + 0.5), int(h * scale + 0.5)          # mmcv.imrescale with a float (_scale_size)
        else:
            nw, nh = imresize.rescale_size(w, h, scale)
        if nh < 1 or nw < 1:
            raise ValueError(f'test pipeline: a {h} x {w} image resizes to the empty size {nh} x {nw} at scale {scale}')
        kind = self.pad[0]
        if kind == 'scale':
            fixed = scale if isinstance(scale, tuple) else None
        else:
            fixed = self.pad[1] if kind == 'size' else None
        ph, pw = (max(nh, fixed[0]), max(nw, fixed[1])) if fixed is not None else (nh, nw)
        if kind == 'divisor':
            ph, pw = round_up(ph, self.pad[1]), round_up(pw, self.pad[1])
        return nh, nw, round_up(ph, 32), round_up(pw, 32)

    def meta(self, h, w, view=0, filename=None):
        nh, nw, ph, pw = self.geometry(h, w, view)
        h, w = int(h), int(w)
        sf = np.array([nw / w, nh / h, nw / w, nh / h], dtype=np.float32)
        m = dict(ori_shape=(h, w, 3), img_shape=(nh, nw, 3), pad_shape=(ph, pw, 3), scale_factor=sf,
                 flip=bool(self.views[view][1]), flip_direction='horizontal',
                 pad_fixed_size=self.pad_fixed_size, pad_size_divisor=self.pad_size_divisor)
        if filename is not None:
            m['ori_filename'] = filename
        return m

    def canvas(self, hw, view=0):
        """Batch canvas of images hw [N, 2]: the largest padded shape, rounded up to 32 (mmcv's collate)."""
        g = [self.geometry(h, w, view) for h, w in np.asarray(hw).reshape(-1, 2)]
        return round_up(max(x[2] for x in g), 32), round_up(max(x[3] for x in g), 32)

    # ------------------------------------------------------------------ pixels (device)
    def __call__(self, fetched, view=0, filenames=None):
        """fetched = (src uint8 device tensor, byte offsets int64 [N] (host), hw int32 [N, 2] (host)) -> (img
        [N, 3, Hc, Wc] fp32 on src's device, [meta] * N).  One H2D copy of the tables and one launch."""
        src, off, hw = fetched
        if not (torch.is_tensor(src) and src.is_cuda and src.dtype == torch.uint8):
            raise RuntimeError('DeviceTestPipeline needs decoded uint8 sources on the GPU (TestSource / SourceStore('
                               "placement='device')): HIP kernels only, no CPU fallback")
        hw = np.asarray(hw, dtype=np.int32).reshape(-1, 2)
        n = hw.shape[0]
        metas = [self.meta(h, w, view, None if filenames is None else filenames[i]) for i, (h, w) in enumerate(hw)]
        Hc = round_up(max(m['pad_shape'][0] for m in metas), 32)
        Wc = round_up(max(m['pad_shape'][1] for m in metas), 32)
        flip = 1 if self.views[view][1] else 0
        table = np.array([[m['img_shape'][0], m['img_shape'][1], flip, 0] for m in metas], dtype=np.int32)
        img = torch.empty(n, 3, Hc, Wc, dtype=torch.float32, device=src.device)
        launch_pixels(src, off, hw, table, img)
        return img, metas


def launch_pixels(src, off, hw, table, out):
    """yunet_test_pixels on the current stream.  off int64 [N], hw int32 [N,2], table int32 [N,4]: host arrays (one
    pinned block, one copy) or, all three, device tensors."""
    n, _, Hc, Wc = out.shape
    dev = src.device
    if torch.is_tensor(off):
        d_off, d_hw, d_tab = off, hw, table
    else:
        host = torch.empty(4 * n, dtype=torch.int64).pin_memory()
        host[:n] = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64).reshape(n))
        host[n:2 * n].view(torch.int32)[:] = torch.from_numpy(np.ascontiguousarray(hw, dtype=np.int32).reshape(2 * n))
        host[2 * n:].view(torch.int32)[:] = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32).reshape(4 * n))
        d = host.to(dev, non_blocking=True)
        d_off, d_hw, d_tab = d[:n], d[n:2 * n].view(torch.int32), d[2 * n:].view(torch.int32)
    p = lambda x: C.c_void_p(x.data_ptr())      # noqa: E731
    L.check(L.load().yunet_test_pixels(p(src), p(d_off), p(d_hw), p(d_tab), n, Hc, Wc, p(out),
                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), 'yunet_test_pixels')
    return out


class TestSource:
    """Decoded uint8 sources of a test-mode dataset for DeviceTestPipeline.

    cache='device': a SourceStore(placement='device') over the (h, w) of the images that are evaluated (`reserve`:
                    the indices of a run -- max_images, or a rank's shard -- not the whole dataset); an image is
                    decoded (worker pool, PIL) the first time a batch needs it and stays in HBM -- a second
                    evaluation decodes nothing.  The buffer stays allocated until `close()`.
    cache=None    : every batch is decoded again, the next batch ahead of time on the worker pool, and travels as one
                    packed uint8 upload from pinned memory."""
    __test__ = False

    def __init__(self, dataset, cache=None, device='cuda', workers=4):
        if cache not in (None, 'device'):
            raise ValueError(f"test sources: cache must be None or 'device', got {cache!r} (a host-placement store "
                             f'or a window feed is not built for the test pipeline)')
        self.ds, self.cache, self.device, self.workers = dataset, cache, torch.device(device), int(workers)
        self.store, self._slot, self._pool, self._ahead = None, {}, None, {}
        if self.device.type != 'cuda':
            raise RuntimeError('test sources live on the GPU: HIP kernels only, no CPU fallback')

    def reserve(self, indices):
        """cache='device': make the store hold exactly room for dataset images `indices` (plus those it holds already).
        A run over indices the store was not sized for builds a new store over the union; what was decoded is dropped."""
        if self.cache != 'device':
            return
        want = sorted({int(i) for i in indices})
        if self.store is not None and all(i in self._slot for i in want):
            return
        from .source_store import SourceStore
        want = sorted(set(want) | set(self._slot))
        infos = self.ds.data_infos
        self.store = None                   # release the old buffer before the new one is allocated
        self._slot = {i: k for k, i in enumerate(want)}
        self.store = SourceStore([(infos[i]['height'], infos[i]['width']) for i in want], placement='device',
                                 device=self.device)

    def release_workers(self):
        """Shut the decode pool down (it is started again when a batch needs it)."""
        if self._pool is not None:
            self._pool.shutdown(wait=True, cancel_futures=True)
        self._pool, self._ahead = None, {}

    def close(self):
        """Release the worker pool and the device store."""
        self.release_workers()
        self.store, self._slot = None, {}

    def _submit(self, i):
        if self._pool is None and self.workers:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(self.workers)
        if self._pool is not None and i not in self._ahead:
            self._ahead[i] = self._pool.submit(self.ds.load_image, i)

    def _image(self, i):
        fut = self._ahead.pop(i, None)
        return fut.result() if fut is not None else self.ds.load_image(i)

    def fetch(self, idx, ahead=()):
        """-> (src, off [N] int64, hw [N,2] int32) of dataset images idx; `ahead`: the next batch's indices, whose
        decoding is queued on the worker pool now."""
        idx = [int(i) for i in idx]
        if self.cache == 'device':
            self.reserve(list(idx) + list(ahead))
            slot, store = self._slot, self.store
            for i in list(idx) + list(ahead):
                if not store.has(slot[i]):
                    self._submit(i)
            for i in dict.fromkeys(idx):
                if not store.has(slot[i]):
                    store.put(slot[i], self._image(i), np.zeros((0, 4), np.float32), np.zeros((0, 15), np.float32))
            k = [slot[i] for i in idx]
            return store.data, store.offsets[k], store.hw[k]
        for i in list(idx) + list(ahead):
            self._submit(i)
        imgs = [np.ascontiguousarray(self._image(i)) for i in idx]
        for im in imgs:
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError('source images must be uint8 [h, w, 3]')
        sizes = np.array([im.size for im in imgs], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        host = torch.empty(int(sizes.sum()), dtype=torch.uint8).pin_memory()
        flat = host.numpy()
        for o, im in zip(off, imgs):
            flat[o:o + im.size] = im.reshape(-1)
        hw = np.array([[im.shape[0], im.shape[1]] for im in imgs], dtype=np.int32)
        return host.to(self.device, non_blocking=True), off, hw


def shard_indices(n, rank=0, world=1):
    """The images of rank `rank`: rank, rank + world, ... (mmdet's multi_gpu_test sharding, as evaluation.multi_gpu_test)."""
    return list(range(int(rank), int(n), int(world)))


def batches_of(indices, samples_per_gpu):
    """Consecutive images of a (rank's) list in batches of samples_per_gpu, the last one short (the reference's
    sequential test sampler)."""
    b = int(samples_per_gpu)
    if b < 1:
        raise ValueError(f'samples_per_gpu must be >= 1, got {samples_per_gpu}')
    indices = list(indices)
    return [indices[k:k + b] for k in range(0, len(indices), b)]


def reassemble(parts, n, world):
    """Per-rank result lists (rank r holds images r, r + world, ...) -> one list in dataset order."""
    out = [None] * n
    for r, p in enumerate(parts):
        for k, res in enumerate(p):
            out[r + k * world] = res
    return out


def plan_batches(pipe, hw, indices, samples_per_gpu, max_plans=None, log=None, resident=()):
    """Batches of `indices` whose distinct geometries (B, Hc, Wc) fit the engine's plan cache: batches of
    samples_per_gpu if they do, else one image per batch, with the reason logged (origin-size evaluation walks
    hundreds of canvases; an evicted plan drains the device, Engine.get_plan).  `resident`: the (n, h, w) of the plans
    the engine holds already -- under the EvalHook the training plans share the cache; those that are not among the
    run's own geometries count against the room."""
    if max_plans is None:
        from . import engine
        max_plans = engine.MAX_PLANS
    batches = batches_of(indices, samples_per_gpu)
    if int(samples_per_gpu) > 1:
        geoms = {(len(b),) + pipe.canvas([hw[i] for i in b]) for b in batches}
        others = len({tuple(r) for r in resident} - geoms)
        if len(geoms) + others > max_plans:
            if log is not None:
                log(f'test pipeline: samples_per_gpu={samples_per_gpu} gives {len(geoms)} batch geometries but the engine '
                    f'keeps {max_plans} plans ({others} held by other shapes) -- running one image per batch (use a '
                    f'fixed-size mode, or set YUNET_MAX_PLANS)')
            batches = batches_of(indices, 1)
    return batches


def run_test(model, dataset, device, indices, pipe, source, samples_per_gpu=1, log=None):
    """The detector over dataset images `indices` -> [[dets [n, 5]]] per image, in the order of `indices`.  One view:
    batches through simple_test; several views (MultiScaleFlipAug with scales / flip): each image's views through
    aug_test, one image per view."""
    infos = dataset.data_infos
    hw = {i: (infos[i]['height'], infos[i]['width']) for i in indices}
    out = []
    source.reserve(indices)
    try:
        if len(pipe.views) == 1:
            eng = getattr(model, 'engine', None)
            resident = [key[:3] for key in eng.plans] if eng is not None else ()
            batches = plan_batches(pipe, hw, indices, samples_per_gpu, log=log, resident=resident)
            for k, b in enumerate(batches):
                nxt = batches[k + 1] if k + 1 < len(batches) else ()
                img, metas = pipe(source.fetch(b, ahead=nxt), 0, [infos[i]['filename'] for i in b])
                out.extend(model(return_loss=False, rescale=True, img=[img], img_metas=[metas]))
            return out
        for k, i in enumerate(indices):
            nxt = indices[k + 1:k + 2]
            fetched = source.fetch([i], ahead=nxt)
            imgs, metas = [], []
            for v in range(len(pipe.views)):
                img, m = pipe(fetched, v, [infos[i]['filename']])
                imgs.append(img)
                metas.append(m)
            out.extend(model(return_loss=False, rescale=True, img=imgs, img_metas=metas))
        return out
    finally:
        source.release_workers()        # no decode threads outlive a run; a device store does (TestSource.close)


def source_for(dataset, cache, device, workers=4):
    """The TestSource of (dataset, cache, device), kept on the dataset so that a device store outlives one evaluation
    (the EvalHook fires every interval; the images are decoded the first time only).  The store's HBM stays held
    until `release_sources(dataset)`."""
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    held = getattr(dataset, '_test_sources', None)
    if held is None:
        held = {}
        try:
            dataset._test_sources = held
        except AttributeError:
            pass
    key = (cache, str(dev))
    if key not in held:
        held[key] = TestSource(dataset, cache=cache, device=dev, workers=workers)
    return held[key]


def release_sources(dataset):
    """Close every TestSource `source_for` put on the dataset (worker pools, device stores)."""
    for src in (getattr(dataset, '_test_sources', None) or {}).values():
        src.close()
    if getattr(dataset, '_test_sources', None):
        dataset._test_sources.clear()
