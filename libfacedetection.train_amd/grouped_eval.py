"""Evaluation batched by padded canvas (opt-in, group_by='canvas') on top of the batched device test pipeline.

    batches = plan_batches(pipe, hw, indices, 16, group_by='canvas')                 # one padded shape per batch
    dets = run_test(model, dataset, dev, indices, pipe, source, 16, group_by='canvas')

`test_pipeline.plan_batches` takes consecutive images and collates them onto the largest canvas of the batch; at
origin size that needs more batch geometries than the engine keeps plans and it falls back to one image per batch.
A batch whose images all share one padded shape has a canvas equal to each image's own pad_shape, so every image gets
the tensor the per-image path feeds it: grouped batches reproduce the per-image protocol (WIDER-Face "in origin
size"), not only the collate, in fewer forwards.  `plan_batches` and `run_test` here are those of test_pipeline with
the two options added; with group_by=None they are those functions, fallback and log line included.  This is what
evaluation.single_gpu_test / multi_gpu_test run."""
from . import test_pipeline as TP

GROUP_BY = (None, 'canvas')
DEFAULT_CAP = 'default'          # max_batch_pixels: samples_per_gpu * 1024 * 1024


def check_group_by(group_by):
    """The accepted values of group_by (None: consecutive batches; 'canvas': batches of one padded shape)."""
    if group_by not in GROUP_BY:
        raise ValueError(f"group_by must be None or 'canvas', got {group_by!r}")
    return group_by


def batch_pixel_cap(samples_per_gpu, max_batch_pixels=DEFAULT_CAP):
    """The pixel cap of a grouped batch: the default is samples_per_gpu * 1024 * 1024, None is no cap."""
    if isinstance(max_batch_pixels, str) and max_batch_pixels == DEFAULT_CAP:
        return int(samples_per_gpu) * 1024 * 1024
    if max_batch_pixels is None:
        return None
    if int(max_batch_pixels) < 1:
        raise ValueError(f'max_batch_pixels must be >= 1 or None, got {max_batch_pixels}')
    return int(max_batch_pixels)


def group_batches(pipe, hw, indices, samples_per_gpu, max_batch_pixels=DEFAULT_CAP):
    """Batches of `indices` in which every image has the same padded shape pipe.geometry(h, w, 0)[2:].

    Inside a group the images keep the order of `indices`; a group of canvas (ph, pw) is cut into batches of
    max(1, min(samples_per_gpu, max_batch_pixels // (ph * pw))), the last one short.  A plan owns every activation
    buffer of its shape, so the cap keeps a group of tall canvases from allocating samples_per_gpu of them; its
    default (samples_per_gpu * 1024 * 1024) is a choice, not a measurement.  Groups come by descending canvas area,
    ties by (ph, pw): a fixed order, largest allocation first so that the caching allocator can reuse its blocks
    for the smaller ones -- that reason is not measured.  Each geometry (n, ph, pw) occupies one consecutive run of
    batches, so the engine's LRU plan cache (Engine.get_plan) evicts each at most once, whatever their number."""
    b = int(samples_per_gpu)
    if b < 1:
        raise ValueError(f'samples_per_gpu must be >= 1, got {samples_per_gpu}')
    cap = batch_pixel_cap(b, max_batch_pixels)
    groups = {}
    for i in indices:
        groups.setdefault(tuple(pipe.geometry(hw[i][0], hw[i][1], 0)[2:]), []).append(i)
    batches = []
    for ph, pw in sorted(groups, key=lambda c: (-c[0] * c[1], c)):
        eff = b if cap is None else max(1, min(b, cap // (ph * pw)))
        batches.extend(TP.batches_of(groups[ph, pw], eff))
    return batches


def plan_batches(pipe, hw, indices, samples_per_gpu, max_plans=None, log=None, resident=(), group_by=None,
                 max_batch_pixels=DEFAULT_CAP):
    """group_by=None: test_pipeline.plan_batches (consecutive batches, or one image per batch with the reason logged).
    group_by='canvas': the batches of `group_batches`, in its order; this mode never falls back."""
    if check_group_by(group_by) is None:
        return TP.plan_batches(pipe, hw, indices, samples_per_gpu, max_plans=max_plans, log=log, resident=resident)
    return group_batches(pipe, hw, indices, samples_per_gpu, max_batch_pixels)


def run_test(model, dataset, device, indices, pipe, source, samples_per_gpu=1, log=None, group_by=None,
             max_batch_pixels=DEFAULT_CAP):
    """test_pipeline.run_test with the grouped mode: group_by='canvas' (one view only) runs the batches of
    `group_batches` in their planned order (decode-ahead follows it) and returns the results in the order of
    `indices`.  group_by=None is test_pipeline.run_test."""
    if check_group_by(group_by) is None:
        return TP.run_test(model, dataset, device, indices, pipe, source, samples_per_gpu, log=log)
    if len(pipe.views) > 1:
        raise NotImplementedError(f'group_by={group_by!r} with {len(pipe.views)} views: aug_test takes one image per '
                                  'view, so a multi-view run has no batches to group')
    indices = list(indices)
    infos = dataset.data_infos
    # positions in `indices`, so that a list that names an image twice still gets one result each
    pos_hw = [(infos[i]['height'], infos[i]['width']) for i in indices]
    planned = group_batches(pipe, pos_hw, range(len(indices)), samples_per_gpu, max_batch_pixels)
    batches = [[indices[p] for p in b] for b in planned]
    out = [None] * len(indices)
    source.reserve(indices)
    try:
        for k, (b, pos) in enumerate(zip(batches, planned)):
            nxt = batches[k + 1] if k + 1 < len(batches) else ()
            img, metas = pipe(source.fetch(b, ahead=nxt), 0, [infos[i]['filename'] for i in b])
            for p, res in zip(pos, model(return_loss=False, rescale=True, img=[img], img_metas=[metas])):
                out[p] = res
        return out
    finally:
        source.release_workers()        # as test_pipeline.run_test: no decode threads outlive a run
