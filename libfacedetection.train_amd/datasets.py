"""RetinaFace / WIDER-Face `labelv2` annotations and decoded image sources.

Reference: mmdet/datasets/retinaface.py:17-150 (`RetinaFaceDataset`: `_parse_ann_line`,
`load_annotations`, `get_ann_info`) on the text format

    # <relative image path> <width> <height>
    x1 y1 x2 y2 [ 5 x (kx ky kflag) [score] | ignore-flag ]

The reference feeds every sample through cv2 worker processes (LoadImageFromFile + the
augmentation pipeline on the CPU).  Here the dataset only DECODES (PIL; BGR channel order like
cv2.imread) and hands decoded uint8 sources to `pipelines.DevicePipeline`, which runs
RandomSquareCrop -> Resize -> RandomFlip -> collate as HIP kernels
(`RetinaFaceSource.batch`, the counterpart of `runner.SyntheticSourceImages`).
"""
import logging
import os

import numpy as np
import torch

from .builder import DATASETS

NK = 5
_log = logging.getLogger(__name__)


def parse_ann_line(line, min_size=None, test_mode=False):
    """One annotation row -> dict(bbox [4], kps [5,3], ignore, cat)  (retinaface.py:29-56).
    Landmark rows are (x, y, flag): all -1 -> weight 0, else weight 1; a row with a single
    fifth value carries an ignore flag instead of landmarks."""
    values = [float(x) for x in line.strip().split()]
    bbox = np.array(values[0:4], dtype=np.float32)
    kps = np.zeros((NK, 3), dtype=np.float32)
    ignore = False
    if min_size is not None:
        if test_mode:
            raise AssertionError('min_size is a training-time filter')
        if bbox[2] - bbox[0] < min_size or bbox[3] - bbox[1] < min_size:
            ignore = True
    if len(values) > 5:
        kps = np.array(values[4:19], dtype=np.float32).reshape(NK, 3)
        for row in kps:
            if (row == -1).all():
                row[2] = 0.0
            else:
                if row[2] < 0:
                    raise AssertionError(f'negative landmark flag in {line!r}')
                row[2] = 1.0
    elif len(values) == 5:
        ignore = ignore or values[4] == 1
    elif not test_mode:
        raise AssertionError('boxes without landmarks / flags are test annotations')
    return dict(bbox=bbox, kps=kps, ignore=ignore, cat='FG')


def load_labelv2(ann_file, min_size=None, test_mode=False):
    """-> [dict(filename, width, height, objs=[...])]  (retinaface.py:58-99).  Images without
    any object are dropped in training mode."""
    infos, cur = [], None
    with open(ann_file) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            if line.startswith('#'):
                name, w, h = line[1:].strip().split()[:3]
                cur = dict(filename=name, width=int(w), height=int(h), objs=[])
                infos.append(cur)
                continue
            if cur is None:
                raise AssertionError(f'{ann_file}: annotation row before the first "# image" header')
            cur['objs'].append(parse_ann_line(line, min_size, test_mode))
    # the reference keys images by name: a repeated header REPLACES the earlier entry in place
    by_name = {}
    for it in infos:
        by_name[it['filename']] = it
    infos = list(by_name.values())
    if not test_mode:
        infos = [it for it in infos if it['objs']]
    return infos


def ann_info(info):
    """retinaface.py:101-150: kept / ignored boxes, labels, landmarks of one image."""
    keep = [o for o in info['objs'] if not o['ignore']]
    ign = [o for o in info['objs'] if o['ignore']]
    return dict(
        bboxes=np.array([o['bbox'] for o in keep], dtype=np.float32).reshape(-1, 4),
        labels=np.zeros(len(keep), dtype=np.int64),
        keypointss=np.array([o['kps'] for o in keep], dtype=np.float32).reshape(-1, NK, 3),
        bboxes_ignore=np.array([o['bbox'] for o in ign], dtype=np.float32).reshape(-1, 4),
        labels_ignore=np.zeros(len(ign), dtype=np.int64))


def imread_bgr(path):
    """cv2.imread(path, IMREAD_COLOR) stand-in: uint8 [h, w, 3], BGR.  Like cv2 (and mmcv.imread's
    'color' flag) the EXIF orientation tag is APPLIED, so a rotated JPEG decodes in the frame its
    annotations were made in."""
    from PIL import Image, ImageOps
    with Image.open(path) as im:
        im = ImageOps.exif_transpose(im)
        return np.ascontiguousarray(np.asarray(im.convert('RGB'), dtype=np.uint8)[:, :, ::-1])


@DATASETS.register_module()
class RetinaFaceDataset:
    """configs/yunet_n.py:28-35,87-100: dict(type='RetinaFaceDataset', ann_file=..., img_prefix=...,
    pipeline=[...], min_size=...)."""
    CLASSES = ('FG',)

    def __init__(self, ann_file, img_prefix='', pipeline=None, min_size=None, test_mode=False,
                 gt_path=None, **_):
        if int(_.get('samples_per_gpu') or 1) > 1:
            # the reference's tools pop data.test.samples_per_gpu before they build the dataset; one that arrives here
            # was not read by whoever built the dataset, and the images will be evaluated one at a time
            import warnings
            warnings.warn(f"RetinaFaceDataset: samples_per_gpu={_['samples_per_gpu']} reached the dataset unread -- this "
                          f'caller evaluates one image at a time; tools/widerface_batched.py and evaluation.'
                          f'single_gpu_test(samples_per_gpu=...) run the batched device test pipeline')
        if _.get('group_by') is not None:          # tools/widerface_batched.py pops data.test.group_by the same way
            import warnings
            warnings.warn(f"RetinaFaceDataset: group_by={_['group_by']!r} reached the dataset unread -- this caller does "
                          f'not group its batches; tools/widerface_batched.py and evaluation.single_gpu_test('
                          f'group_by=...) do')
        self.ann_file, self.img_prefix, self.pipeline_cfg = ann_file, img_prefix, pipeline
        self.min_size, self.test_mode, self.gt_path = min_size, test_mode, gt_path
        self.NK = NK
        self.cat2label = {c: i for i, c in enumerate(self.CLASSES)}
        self.data_infos = load_labelv2(ann_file, min_size, test_mode)
        if not test_mode:
            # CustomDataset._filter_imgs (mmdet/datasets/custom.py:119-122, 176-185): training drops
            # images whose shorter side is below 32 px
            self.data_infos = [it for it in self.data_infos if min(it['width'], it['height']) >= 32]
        self.flag = np.array([1 if it['width'] / it['height'] > 1 else 0 for it in self.data_infos],
                             dtype=np.uint8)      # CustomDataset._set_group_flag

    def __len__(self):
        return len(self.data_infos)

    def get_ann_info(self, idx):
        return ann_info(self.data_infos[idx])

    def load_image(self, idx):
        return imread_bgr(os.path.join(self.img_prefix, self.data_infos[idx]['filename']))

    def evaluate(self, results, metric='mAP', logger=None, iou_thr=0.5, device=None, rank=None, **_):
        """CustomDataset.evaluate (mmdet/datasets/custom.py:310-367) for the metric the shipped configs ask
        for (`evaluation = dict(interval=..., metric='mAP')`): AP of the face class at each IoU threshold.
        device: a CUDA device scores tp / fp there (evaluation.eval_map_single_class); None: on the host.
        rank='device' (with a device) also ranks the detections and builds the precision curve there."""
        from collections import OrderedDict
        from .evaluation import eval_map_single_class
        if not isinstance(metric, str):
            assert len(metric) == 1
            metric = metric[0]
        if metric != 'mAP':
            raise KeyError(f'metric {metric} is not supported')
        anns = [self.get_ann_info(i) for i in range(len(results))]
        thrs = [iou_thr] if isinstance(iou_thr, float) else list(iou_thr)
        how = {} if rank is None else dict(rank=rank)
        res, aps = OrderedDict(), []
        for t in thrs:
            ap, _ = eval_map_single_class(results, anns, t, device=device, **how)
            aps.append(ap)
            res[f'AP{int(t * 100):02d}'] = round(ap, 3)
        res['mAP'] = sum(aps) / len(aps)
        return res

    def __getitem__(self, idx):
        """Decoded sample (what LoadImageFromFile + LoadAnnotations deliver, before augmentation)."""
        info = self.data_infos[idx]
        ann = self.get_ann_info(idx)
        return dict(img=self.load_image(idx), filename=info['filename'],
                    ori_shape=(info['height'], info['width'], 3), gt_bboxes=ann['bboxes'],
                    gt_labels=ann['labels'], gt_keypointss=ann['keypointss'],
                    gt_bboxes_ignore=ann['bboxes_ignore'])


@DATASETS.register_module()
class MultiImageMixDataset:
    """mmdet/datasets/dataset_wrappers.py:338-444 as a configuration carrier: `dataset` (its pipeline loads: LoadImageFromFile,
    LoadAnnotations) wrapped with the mixing `pipeline` (Mosaic, then the usual train transforms).  The device pipeline runs
    the two lists as one (`flat_pipeline`); the wrapper itself moves no data."""

    def __init__(self, dataset, pipeline, dynamic_scale=None, skip_type_keys=None, max_refetch=15):
        if dynamic_scale is not None:
            raise RuntimeError('dynamic_scale is deprecated. Please use Resize pipeline to achieve similar functions')
        if skip_type_keys is not None:
            assert all(isinstance(skip_type_key, str) for skip_type_key in skip_type_keys)
        self._skip_type_keys = skip_type_keys
        self.dataset = DATASETS.build(dataset) if isinstance(dataset, dict) else dataset
        self.pipeline_cfg, self.max_refetch = list(pipeline), max_refetch
        self.CLASSES = getattr(self.dataset, 'CLASSES', None)
        if hasattr(self.dataset, 'flag'):
            self.flag = self.dataset.flag

    def __len__(self):
        return len(self.dataset)

    def update_skip_type_keys(self, skip_type_keys):
        """dataset_wrappers.py:446-456: a sequence of type strings; those steps are skipped from then on."""
        assert all(isinstance(skip_type_key, str) for skip_type_key in skip_type_keys)
        self._skip_type_keys = skip_type_keys


def flatten_multi_image_mix(dcfg):
    """data.train = dict(type='MultiImageMixDataset', dataset=dict(...), pipeline=[...]) -> the inner dataset's
    configuration with pipeline = its own loading steps + the wrapper's list (the flat list DevicePipeline takes); the
    wrapper's other keys (cache, host_fed, ... given with --cfg-options) travel to the inner configuration.  The flat
    configuration has no place for skip_type_keys: take them off first with split_skip_type_keys, which hands them to
    the source."""
    if dcfg.get('dynamic_scale') is not None:
        raise RuntimeError('dynamic_scale is deprecated. Please use Resize pipeline to achieve similar functions')
    if dcfg.get('skip_type_keys') is not None:
        raise NotImplementedError('MultiImageMixDataset(skip_type_keys=...) is not carried by the flat configuration: '
                                  'split_skip_type_keys(cfg) takes the keys off for the source (skip_type_keys=)')
    inner = dict(dcfg['dataset'])
    if inner.get('type') == 'MultiImageMixDataset':
        raise NotImplementedError('nested MultiImageMixDataset')
    inner['pipeline'] = list(inner.get('pipeline') or []) + list(dcfg['pipeline'])
    for k, v in dcfg.items():
        if k not in ('type', 'dataset', 'pipeline', 'dynamic_scale', 'skip_type_keys', 'max_refetch'):
            inner[k] = v
    return inner


def split_skip_type_keys(dcfg):
    """A MultiImageMixDataset configuration -> (the configuration without skip_type_keys, the keys as a list or None).
    The keys keep the reference's assertion, a sequence of str (dataset_wrappers.py:354-366); the caller hands them to
    the source it builds from the flattened rest (RetinaFaceSource / SyntheticSourceImages skip_type_keys=), which
    switches those steps off from the first batch on."""
    keys = dcfg.get('skip_type_keys')
    if keys is None:
        return dcfg, None
    assert all(isinstance(skip_type_key, str) for skip_type_key in keys)
    return type(dcfg)({k: v for k, v in dcfg.items() if k != 'skip_type_keys'}), list(keys)


def ignore_counts(dataset):
    """Ignored faces per image of dataset.data_infos -- the rows get_ann_info returns as `bboxes_ignore` (labelv2's
    ignore flag, and every face below min_size); read from the annotations, no image is decoded."""
    return [int(len(dataset.get_ann_info(i)['bboxes_ignore'])) for i in range(len(getattr(dataset, 'data_infos', ())))]


def gt_counts(dataset):
    """Non-ignored faces per image of dataset.data_infos -- the rows get_ann_info returns as `bboxes`; read from the
    annotations, no image is decoded."""
    return [int(len(dataset.get_ann_info(i)['bboxes'])) for i in range(len(getattr(dataset, 'data_infos', ())))]


class RetinaFaceSource:
    """Training data source over a RetinaFaceDataset: iteration `it` of rank r is batch it % iters_per_epoch of the
    reference's DistributedGroupSampler(dataset, samples_per_gpu, world, r, seed) in epoch it // iters_per_epoch
    (samplers.py; the order `tools/dist_train.sh` feeds, also used at world size 1, where the reference's
    GroupSampler draws from numpy's global generator and is not reproducible).  Samples are decoded with PIL on
    the host and augmented on the GPU by the config's own pipeline (pipelines.DevicePipeline).

    cache=None    : every use of a sample decodes it again (PIL) and uploads the whole decoded image.
    cache='device': each sample is decoded the first time the sampler yields it and kept in a device SourceStore
                    (source_store.py; decoded WIDER-Face train is ~30 GB of HBM); a batch is a gather of store indices.
    cache='host'  : the same in a PINNED host SourceStore (that many bytes of pinned RAM per rank); per batch only the
                    crop-window rectangles travel (WindowFeed).  host_fetch (cache='host' only): None or 'dma' = one
                    hipMemcpy2DAsync per rectangle after a host wait on the plan; 'kernel' = the GPU reads the
                    rectangles from the pinned store itself (yunet_fetch_windows), no host wait.
    All three give bit-identical batches; the image sizes of the labelv2 headers must be the decoded ones.

    GT rows.  Every crop's GT is padded to one width for the whole run (one engine plan per batch geometry, nothing is
    read back per batch); faces a crop keeps beyond it are dropped (status 2, counted by truncated()).
    gt_capacity=None     : 64 rows (128 for max_gt > 64); the constructor warns when the dataset has larger images.
    gt_capacity='dataset': the largest image's face count, so no crop can be truncated.
    gt_capacity=int      : that many faces.
    Both are rounded by pipelines.gt_capacity_rows (a power of two >= 64, at most 4096; with a Mosaic in the pipeline at
    most 256 per image: its merged GT stays within 1024 rows, and a larger image can still truncate a merged canvas).

    Ignore boxes (gt_bboxes_ignore: labelv2's ignore flag and the faces below min_size).
    ignore_capacity=None     : today's batches, byte for byte -- nothing is allocated or launched, no new key.
    ignore_capacity='dataset': rows for the largest ignore count of any image (from the annotations).
    ignore_capacity=int      : that many boxes.
    Both are rounded by pipelines.ignore_capacity_rows (a power of two >= 16, at most 1024); boxes a crop keeps beyond
    the rows are dropped in order.  The batch then carries `gt_bboxes_ignore` (a DeviceGT), which the model uses when
    train_cfg.assigner.ignore_iof_thr >= 0.  Not with Mosaic, RandomAffine or MixUp in the pipeline."""

    def __init__(self, dataset, pipeline, samples_per_gpu=16, rank=0, world=1, seed=0, max_gt=64, workers=4,
                 cache=None, host_fetch=None, gt_capacity=None, skip_type_keys=None, ignore_capacity=None):
        from .pipelines import DevicePipeline, gt_capacity_rows, ignore_capacity_rows
        counts = gt_counts(dataset)
        self._gt_counts = counts
        types = [(p.get('type') if isinstance(p, dict) else type(p).__name__) for p in pipeline]
        mosaic, mixup = 'Mosaic' in types, 'MixUp' in types
        if gt_capacity is None:
            rows = 64 if max_gt <= 64 else 128
        else:
            if max_gt != 64:
                raise ValueError(f'RetinaFaceSource: gt_capacity={gt_capacity!r} and max_gt={max_gt!r} both size the GT '
                                 'rows; give one of them')
            if isinstance(gt_capacity, str) and gt_capacity != 'dataset':
                raise ValueError(f"RetinaFaceSource gt_capacity must be 'dataset' or an integer >= 1 (or unset), "
                                 f'got {gt_capacity!r}')
            want = max([1] + counts) if gt_capacity == 'dataset' else gt_capacity
            rows = gt_capacity_rows(want, mosaic=mosaic, mixup=mixup)
        self.gt_rows = rows                     # padded GT rows per source image (a Mosaic merges four: pipe.gmax = 4 rows)
        over = [c for c in counts if c > rows]
        if over:
            if gt_capacity == 'dataset':        # only under Mosaic
                lift = 'Mosaic takes at most 256 rows per image (1024 merged): such an image can still truncate a canvas'
            else:
                lift = "gt_capacity='dataset' (data.train.gt_capacity=dataset) sizes the rows for the largest image"
                if mosaic and max(over) > 256:
                    lift += ', under Mosaic up to 256 per image (1024 merged)'
            _log.warning(f'RetinaFaceSource: {len(over)} images have more than {rows} faces (largest {max(over)}); '
                         f'{sum(c - rows for c in over)} faces beyond the capacity of {rows} GT rows are dropped from '
                         f'training whenever a crop keeps them -- {lift}')
        self._trunc = None                      # device int64 [2]: (images, rows) truncated so far
        if cache not in (None, 'device', 'host'):
            raise ValueError(f"RetinaFaceSource cache must be None, 'device' or 'host', got {cache!r}")
        if host_fetch not in (None, 'dma', 'kernel'):
            raise ValueError(f"RetinaFaceSource host_fetch must be 'dma' or 'kernel' (or unset), got {host_fetch!r}")
        if host_fetch is not None and cache != 'host':
            raise ValueError(f"RetinaFaceSource host_fetch applies to cache='host' only, not cache={cache!r}")
        self.host_fetch = host_fetch
        self.cache, self.store, self._feed, self._decoding = cache, None, None, {}
        self.ds, self.bs, self.rank, self.world, self.seed = dataset, samples_per_gpu, rank, world, seed
        self.ignore_rows = None                 # padded ignore rows per image; None: the option is off
        if ignore_capacity is not None:
            if isinstance(ignore_capacity, str) and ignore_capacity != 'dataset':
                raise ValueError(f"RetinaFaceSource ignore_capacity must be 'dataset' or an integer >= 0 (or unset), "
                                 f'got {ignore_capacity!r}')
            icounts = ignore_counts(dataset)
            self.ignore_rows = ignore_capacity_rows(max([0] + icounts) if ignore_capacity == 'dataset' else ignore_capacity)
            iover = [c for c in icounts if c > self.ignore_rows]
            if iover:
                _log.warning(f'RetinaFaceSource: {len(iover)} images have more than {self.ignore_rows} ignore boxes (largest '
                             f'{max(iover)}); {sum(c - self.ignore_rows for c in iover)} boxes beyond the capacity of '
                             f'{self.ignore_rows} rows are dropped, in order, whenever a crop keeps them')
        self.pipe = DevicePipeline(pipeline, seed=seed + 7919 * rank, gmax=rows, ignore_rows=self.ignore_rows)
        self.pipe.check_plan_cache()
        if skip_type_keys is not None:
            self.pipe.update_skip_type_keys(skip_type_keys)
        if cache != 'device':
            self.pipe.require_resident(f'RetinaFaceSource(cache={cache!r})')
        from .samplers import DistributedGroupSampler
        self.sampler = DistributedGroupSampler(dataset, samples_per_gpu, world, rank, seed=seed)
        self.iters_per_epoch = max(1, len(self.sampler) // samples_per_gpu)
        self._perm_epoch, self._perm = None, None
        # decode ahead: the samples of iteration it + 1 are decoded by a small thread pool (PIL releases
        # the GIL while decoding) while the GPU runs iteration it -- the role of the reference's
        # DataLoader workers (workers_per_gpu, mmdet/datasets/builder.py:87-190)
        self.workers = max(0, int(workers))
        self._pool = None
        self._ahead = {}

    @property
    def dataset(self):
        """What a hook reaches as runner.data_loader.dataset: the object that takes update_skip_type_keys."""
        return self

    def update_skip_type_keys(self, skip_type_keys):
        """MultiImageMixDataset.update_skip_type_keys: forwarded to the device pipeline."""
        self.pipe.update_skip_type_keys(skip_type_keys)

    def _indices(self, it):
        epoch, k = divmod(it, self.iters_per_epoch)
        if self._perm_epoch != epoch:
            self.sampler.set_epoch(epoch)
            self._perm = list(iter(self.sampler))
            self._perm_epoch = epoch
        return self._perm[k * self.bs:(k + 1) * self.bs]

    def _decoded(self, it):
        if self.workers == 0:
            return [self.ds[i] for i in self._indices(it)]
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(self.workers)
        for k in (it, it + 1):                              # this iteration (if not already queued) and the next
            if k not in self._ahead:
                self._ahead[k] = [self._pool.submit(self.ds.__getitem__, i) for i in self._indices(k)]
        futs = self._ahead.pop(it)
        for k in [k for k in self._ahead if k < it]:        # a caller that jumps around: drop stale work
            del self._ahead[k]
        return [f.result() for f in futs]

    def _partners(self, it, n):
        """Mosaic / MixUp: the store indices iteration it's kernels will draw as partners of its n images -- a pure
        function of (seed, it, image) and the dataset's GT counts, computed here so that they are decoded before the
        batch that reads them."""
        from .pipelines import mixup_partner, mosaic_partners
        m, out = len(self.ds.data_infos), []
        if self.pipe.mosaic is not None:
            out += [j for k in range(n) for j in mosaic_partners(self.pipe.cfg.seed, it, k, m)]
        if self.pipe.mixup is not None:     # the one MixUp partner per image: the first drawn image that has boxes
            out += [mixup_partner(self.pipe.cfg.seed, it, k, self._gt_counts, self.pipe.mixup.max_iters) for k in range(n)]
        return out

    def _fill(self, it):
        """Decode the images of iteration it that the store lacks (and queue those of it + 1), store them; -> indices."""
        idx = self._indices(it)
        need = idx + self._partners(it, len(idx))
        ahead = (self._indices(it + 1) + self._partners(it + 1, len(idx))) if self.workers else []
        if self.workers and self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(self.workers)
        for i in list(dict.fromkeys(need)) + [i for i in ahead if i not in need]:
            if not self.store.has(i) and i not in self._decoding and self.workers:
                self._decoding[i] = self._pool.submit(self.ds.load_image, i)
        for i in dict.fromkeys(need):
            if not self.store.has(i):
                fut = self._decoding.pop(i, None)
                img = fut.result() if fut is not None else self.ds.load_image(i)
                ann = self.ds.get_ann_info(i)
                self.store.put(i, img, ann['bboxes'], ann['keypointss'],
                               ann['bboxes_ignore'] if self.ignore_rows is not None else None)
        return idx

    def _cached_batch(self, it, device):
        from .source_store import SourceStore, WindowFeed
        if self.store is None:
            sizes = [(info['height'], info['width']) for info in self.ds.data_infos]
            self.store = SourceStore(sizes, placement=self.cache, device=device, ignore=self.ignore_rows is not None)
        idx = self._fill(it)
        if self.cache == 'device':
            return self.pipe(self.store.batch(idx), it)
        f = self._feed
        if f is None:       # two window buffers, each the bs largest images (a window never exceeds its image)
            big = int(np.sort(self.store.image_bytes)[::-1][:self.bs].sum())
            f = self._feed = WindowFeed(self.pipe, self.store, big, fetch=self.host_fetch or 'dma')
        if not f.uploaded(it):
            if not f.planned(it):
                f.plan(it, idx)
            f.upload(it)
        out, _ = f.run(it)
        # once every image of the next iterations is stored (from the second epoch on): the upload of it + 1 travels
        # under this step, and the plan of it + 2 is made now so that batch(it + 1) finds it done
        nxt, nxt2 = self._indices(it + 1), self._indices(it + 2)
        if all(self.store.has(i) for i in nxt) and not f.uploaded(it + 1):
            if not f.planned(it + 1):
                f.plan(it + 1, nxt)
            f.upload(it + 1)
        if all(self.store.has(i) for i in nxt2) and not f.planned(it + 2):
            f.plan(it + 2, nxt2)
        return out

    def batch(self, it, device=None):
        if device is None:
            raise RuntimeError('RetinaFaceSource augments on the GPU: a device is required')
        if self.cache is not None:
            out = self._cached_batch(it, device)
        else:
            from .pipelines import SourceBatch
            samples = self._decoded(it)
            src = SourceBatch.from_lists([s['img'] for s in samples], [s['gt_bboxes'] for s in samples],
                                         [s['gt_keypointss'] for s in samples], device,
                                         [s['gt_bboxes_ignore'] for s in samples] if self.ignore_rows is not None else None)
            out = self.pipe(src, it)
        self._count_truncated()
        return out

    def _count_truncated(self):
        """Adds the last batch's truncated images / dropped rows to the device counters: tensor ops on the batch's own
        stream, nothing is read back."""
        from . import _lib as L
        p = self.pipe.params
        cut = p[:, 6] == 2
        if self.pipe.geom is not None:          # a merged GT beyond gmax: status bit 2 of the geometry table
            cut = cut | ((self.pipe.geom[:, L.MOSAIC_STATUS] & 2) != 0)
        if self.pipe.mixup_table is not None:   # and the same bit of MixUp's table
            cut = cut | ((self.pipe.mixup_table[:, L.MIXUP_STATUS].to(torch.int64) & 2) != 0)
        rows = (p[:, 4] - self.pipe.gmax).clamp_min(0)
        add = torch.stack([cut.sum(), rows.sum()])
        self._trunc = add if self._trunc is None else self._trunc + add

    def truncated(self):
        """(images, rows): how many images of the batches so far lost GT to the padded width (status 2 of the decide;
        under Mosaic also a truncated merge), and how many kept faces lay beyond it.  Reading synchronises."""
        if self._trunc is None:
            return 0, 0
        images, rows = self._trunc.tolist()
        return int(images), int(rows)
