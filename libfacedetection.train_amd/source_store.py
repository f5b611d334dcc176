"""Decoded-source store for the device train pipeline: decode once, then feed batches from the store.

    store = SourceStore([(h, w), ...], placement='device')     # capacity up front (labelv2 carries the sizes)
    store.put(i, img_uint8_hwc, boxes, kps)                    # once per image
    src = store.batch(idx)                                     # SourceBatch via yunet_aug_gather (no pixel moves)
    batch = pipe(src, iteration)

Two placements:
  device  the decoded images live in HBM; a batch is a gather of store indices (csrc/source.hip aug_gather_kernel).
  host    the decoded images live in PINNED host memory (their bytes, per rank); per batch only the rectangle of each
          image that the pixel pass can read travels (WindowFeed: yunet_aug_window_plan -> yunet_upload_windows or,
          with fetch='kernel', yunet_fetch_windows -> yunet_aug_pixels with the plan's rect).
Annotations and the per-image tables always live on the device.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

GATHER_MAX_N = 8192        # csrc/source.hip: prefix offsets of one batch in LDS


def _h2d(arr, dev):
    """Host array -> new device tensor through a pinned staging block, without synchronising the stream (torch's
    pinned-block cache keeps the block until the copy has run)."""
    return torch.from_numpy(np.ascontiguousarray(arr)).pin_memory().to(dev, non_blocking=True)


def window_plan_np(params, src_hw):
    """numpy restatement of yunet_aug_window_plan: params [N,8] (aug_decide), src_hw [N,2] ->
    (rect [N,4] int32 (row0, col0, rows, cols), win_off [N+1] int64)."""
    params = np.asarray(params, dtype=np.int64).reshape(-1, 8)
    hw = np.asarray(src_hw, dtype=np.int64).reshape(-1, 2)
    left, top, cw = params[:, 0], params[:, 1], params[:, 2]
    h, w = hw[:, 0], hw[:, 1]
    y0, y1 = np.maximum(top, 0), np.minimum(top + cw, h)
    x0, x1 = np.maximum(left, 0), np.minimum(left + cw, w)
    ok = (cw > 0) & (y1 > y0) & (x1 > x0)
    rect = np.where(ok[:, None], np.stack([y0, x0, y1 - y0, x1 - x0], 1), 0).astype(np.int32)
    nbytes = rect[:, 2].astype(np.int64) * rect[:, 3] * 3
    return rect, np.concatenate([[0], np.cumsum(nbytes)]).astype(np.int64)


class SourceStore:
    """Decoded uint8 HWC images of a dataset and their ragged GT in one store.  `sizes`: (h, w) per image, given up
    front; the pixel buffer (sum h * w * 3 bytes, device or pinned host) is allocated on the first put."""

    def __init__(self, sizes, placement='device', device='cuda', ignore=False):
        if placement not in ('device', 'host'):
            raise ValueError(f"SourceStore placement must be 'device' or 'host', got {placement!r}")
        hw = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        if hw.shape[0] < 1 or (hw < 1).any() or (hw > np.iinfo(np.int32).max // 3).any():
            raise ValueError('SourceStore needs at least one image and positive (h, w) sizes')
        self.placement, self.device = placement, torch.device(device)
        self.hw = hw.astype(np.int32)
        nbytes = hw[:, 0] * hw[:, 1] * 3
        self.offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
        self.nbytes = int(nbytes.sum())
        self.image_bytes = nbytes
        self.data = None
        self._stored = np.zeros(len(hw), dtype=bool)
        self._goff = np.zeros(len(hw), dtype=np.int32)
        self._gcnt = np.zeros(len(hw), dtype=np.int32)
        self._boxes = np.zeros((0, 4), dtype=np.float32)      # GT rows, appended by put()
        self._kps = np.zeros((0, 15), dtype=np.float32)
        self._g_used = 0
        # ignore boxes (ignore=True: put() takes them, batch() delivers ign_boxes / ign_off): they travel with the GT
        # tables, not with the pixels -- host rows per image, the batch's ragged table is built per gather
        self.ignore = bool(ignore)
        self._ign = [None] * len(hw)
        self._dev = None                                      # device tables (synced before a gather)
        self._dev_rows = 0
        self._dirty = True

    def __len__(self):
        return len(self.hw)

    def has(self, i):
        return bool(self._stored[i])

    def _alloc(self):
        if self.data is None:
            if self.placement == 'device':
                self.data = torch.empty(self.nbytes, dtype=torch.uint8, device=self.device)
            else:
                self.data = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=True)

    def put(self, i, img, boxes, kps, ign=None):
        """Store image i (uint8 [h, w, 3] at the size given up front) and its GT (boxes [G,4], kps [G,5,3]); `ign`: its
        ignore boxes [I,4] (a store built with ignore=True; None = no ignore box)."""
        i = int(i)
        if not 0 <= i < len(self.hw):
            raise IndexError(f'image {i} outside the store (capacity {len(self.hw)})')
        img = np.ascontiguousarray(np.asarray(img.cpu() if torch.is_tensor(img) else img))
        h, w = (int(v) for v in self.hw[i])
        if img.dtype != np.uint8 or img.shape != (h, w, 3):
            raise ValueError(f'image {i}: expected uint8 {(h, w, 3)} (the size the store was given), '
                             f'got {img.dtype} {img.shape}')
        b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
        k = np.asarray(kps, dtype=np.float32).reshape(-1, 15)
        if b.shape[0] != k.shape[0]:
            raise ValueError(f'image {i}: {b.shape[0]} boxes but {k.shape[0]} keypoint rows')
        self._alloc()
        o = int(self.offsets[i])
        if self.placement == 'device':
            self.data[o:o + img.size].copy_(torch.from_numpy(img.reshape(-1)).pin_memory(), non_blocking=True)
        else:
            self.data[o:o + img.size].numpy()[:] = img.reshape(-1)
        g = b.shape[0]
        need = self._g_used + g
        if need > self._boxes.shape[0]:
            cap = max(need, 2 * self._boxes.shape[0], 64)
            self._boxes = np.concatenate([self._boxes[:self._g_used], np.zeros((cap - self._g_used, 4), np.float32)])
            self._kps = np.concatenate([self._kps[:self._g_used], np.zeros((cap - self._g_used, 15), np.float32)])
        self._boxes[self._g_used:need] = b
        self._kps[self._g_used:need] = k
        self._goff[i], self._gcnt[i] = self._g_used, g
        self._g_used = need
        if self.ignore:
            self._ign[i] = np.zeros((0, 4), np.float32) if ign is None else np.asarray(ign, dtype=np.float32).reshape(-1, 4).copy()
        self._stored[i] = True
        self._dirty = True

    def _sync(self):
        """Device tables on the current stream: per-image tables in full, GT rows appended since the last sync."""
        if not self._dirty:
            return self._dev
        dev = self.device
        rows, u, t = max(1, self._g_used), self._dev_rows, self._dev
        if t is None:
            t = dict(off=_h2d(self.offsets, dev), hw=_h2d(self.hw, dev))
        if 'boxes' not in t or t['boxes'].shape[0] < rows:
            cap = max(rows, 2 * (t['boxes'].shape[0] if 'boxes' in t else 0))
            boxes, kps = torch.zeros(cap, 4, device=dev), torch.zeros(cap, 15, device=dev)
            if u:
                boxes[:u], kps[:u] = t['boxes'][:u], t['kps'][:u]
            t['boxes'], t['kps'] = boxes, kps
        if self._g_used > u:
            t['boxes'][u:self._g_used] = _h2d(self._boxes[u:self._g_used], dev)
            t['kps'][u:self._g_used] = _h2d(self._kps[u:self._g_used], dev)
            self._dev_rows = self._g_used
        t['goff'], t['gcnt'] = _h2d(self._goff, dev), _h2d(self._gcnt, dev)
        self._dev, self._dirty = t, False
        return t

    def batch(self, idx, device=None):
        """SourceBatch of the stored images idx (repeats allowed) via yunet_aug_gather on the current stream.  Device
        placement: `src` is the store itself; host placement: `src` is the pinned host store (for WindowFeed; the
        plain pipeline refuses it).  The batch also carries `host_off` / `host_hw` (numpy) of the picked images."""
        from .pipelines import SourceBatch, StoreView
        idx = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx, dtype=np.int64).reshape(-1)
        n = idx.shape[0]
        if not 1 <= n <= GATHER_MAX_N:
            raise ValueError(f'a batch has 1..{GATHER_MAX_N} images, got {n}')
        if device is not None and torch.device(device).type != self.device.type:
            raise ValueError(f'the store lives on {self.device}, not {device}')
        if (idx < 0).any() or (idx >= len(self.hw)).any():
            raise IndexError('batch index outside the store')
        missing = idx[~self._stored[idx]]
        if missing.size:
            raise KeyError(f'images {sorted(set(missing.tolist()))[:8]} are not in the store yet')
        t = self._sync()
        dev = self.device
        g = int(self._gcnt[idx].sum())
        d_idx = _h2d(idx.astype(np.int32), dev)
        src_off = torch.empty(n, dtype=torch.int64, device=dev)
        src_hw = torch.empty(n, 2, dtype=torch.int32, device=dev)
        gt_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
        mk = torch.empty if g else torch.zeros
        boxes = mk(max(1, g), 4, device=dev)
        kps = mk(max(1, g), 5, 3, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        L.check(L.load().yunet_aug_gather(p(d_idx), n, len(self.hw), p(t['off']), p(t['hw']), p(t['goff']),
                                          p(t['gcnt']), p(t['boxes']), p(t['kps']), g, p(src_off), p(src_hw),
                                          p(gt_off), p(boxes), p(kps), stream), 'yunet_aug_gather')
        view = StoreView(len(self.hw), t['off'], t['hw'], t['goff'], t['gcnt'], t['boxes'], t['kps'])
        ign = {}
        if self.ignore:
            from .pipelines import ragged_ignore
            ib, io = ragged_ignore([self._ign[i] for i in idx])
            ign = dict(ign_boxes=_h2d(ib, dev), ign_off=_h2d(io, dev))
        sb = SourceBatch(self.data, src_off, src_hw, boxes, kps, gt_off,
                         view=view if self.placement == 'device' else None, idx=d_idx, **ign)
        sb.host_off, sb.host_hw = self.offsets[idx], self.hw[idx]
        return sb


class WindowFeed:
    """Host-placement feed: per iteration it, on a plan stream, gather -> aug_decide(it) -> window plan; then the windows
    travel on a copy stream into one of two device window buffers; then, on the current stream, the pipeline on that
    window buffer.  aug_decide is keyed by (seed, iteration, image), so a plan can be made iterations ahead and the real
    aug_decide of the iteration gives the same params.  Buffer reuse waits on GPU events.  How the windows travel:

      fetch='dma'    the plan is copied back into a pinned ring and, once it has landed (the host waits on the plan
                     event), yunet_upload_windows queues one hipMemcpy2DAsync per rectangle.
      fetch='kernel' the copy stream waits on the plan event on the GPU and yunet_fetch_windows reads the rectangles
                     from the pinned store itself, with the plan taken from device memory: no host wait, no plan copy.
                     Invalid plan rows are skipped on the device and flagged in a device status word: check().

    A square_range pipeline (multi-scale training) needs each image's S_n on the host before it can allocate the batch:
    the plan carries params[:, 7] into a pinned ring with the plan's own copies, and run() hands them to the pipeline
    once the plan event has passed -- an event made iterations earlier, not a wait on the device."""

    RING = 3

    def __init__(self, pipe, store, win_bytes, timing=False, fetch='dma'):
        if store.placement != 'host':
            raise ValueError('WindowFeed feeds from a host-placement SourceStore')
        if fetch not in ('dma', 'kernel'):
            raise ValueError(f"WindowFeed fetch must be 'dma' or 'kernel', got {fetch!r}")
        pipe.require_resident('a window feed')
        dev = store.device
        self.pipe, self.store, self.timing, self.fetch = pipe, store, bool(timing), fetch
        self._plan_stream = torch.cuda.Stream(device=dev)
        self._copy = torch.cuda.Stream(device=dev)
        self._bufs = [torch.empty(int(win_bytes), dtype=torch.uint8, device=dev) for _ in range(2)]
        self._status = torch.zeros(1, dtype=torch.int32, device=dev) if fetch == 'kernel' else None
        self._consumed = [None, None]          # event: the pipeline that read buffer b has run
        self._ring = None
        self._size_ring = None                 # square_range: pinned S_n [N] per plan in flight
        self._nplans = 0
        self._planned = {}                     # it -> plan
        self._uploaded = {}                    # it -> (buffer, e0, e1, bytes)

    def planned(self, it):
        return it in self._planned

    def uploaded(self, it):
        return it in self._uploaded

    def _sizes_to_host(self, params, n):
        """On the plan stream, before the plan event: S_n of a square_range plan -> a slot of the pinned ring."""
        if self.pipe.scale_range is None:
            return None
        if self._size_ring is None or self._size_ring[0].shape[0] != n:
            self._size_ring = [torch.empty(n, dtype=torch.int32, pin_memory=True) for _ in range(self.RING)]
        sizes_h = self._size_ring[self._nplans % self.RING]
        sizes_h.copy_(params[:, 7], non_blocking=True)
        return sizes_h

    def plan(self, it, idx):
        """Enqueue the plan of iteration it (store images idx) on the plan stream."""
        st = self._plan_stream
        n = len(idx)
        if self.fetch == 'kernel':
            with torch.cuda.stream(st):
                sb = self.store.batch(idx)
                params, rect, off = self.pipe.window_plan(sb, it, self.store.device)
                sizes_h = self._sizes_to_host(params, n)
                ev = torch.cuda.Event()
                ev.record(st)
            self._nplans += 1
            self._planned[it] = dict(sb=sb, rect=rect, off=off, ev=ev, sizes_h=sizes_h)
            return
        if self._ring is None or self._ring[0][0].shape[0] != n:
            self._ring = [(torch.empty(n, 4, dtype=torch.int32, pin_memory=True),
                           torch.empty(n + 1, dtype=torch.int64, pin_memory=True)) for _ in range(self.RING)]
        rect_h, off_h = self._ring[self._nplans % self.RING]
        with torch.cuda.stream(st):
            sb = self.store.batch(idx)
            params, rect, off = self.pipe.window_plan(sb, it, self.store.device)
            rect_h.copy_(rect, non_blocking=True)
            off_h.copy_(off, non_blocking=True)
            sizes_h = self._sizes_to_host(params, n)
            ev = torch.cuda.Event()
            ev.record(st)
        self._nplans += 1
        self._planned[it] = dict(sb=sb, rect=rect, off=off, rect_h=rect_h, off_h=off_h, ev=ev, sizes_h=sizes_h)

    def upload(self, it):
        """Issue the copies of iteration it's windows (its plan must have been enqueued)."""
        if self.fetch == 'kernel':
            return self._fetch(it)
        P = self._planned[it]
        P['ev'].synchronize()
        b = it % 2
        total = int(P['off_h'][-1])
        if total > self._bufs[b].numel():
            raise RuntimeError(f'window buffer too small: {total} > {self._bufs[b].numel()} bytes')
        sb, p = P['sb'], (lambda x: C.c_void_p(x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()))
        host_off = np.ascontiguousarray(sb.host_off, dtype=np.int64)
        host_hw = np.ascontiguousarray(sb.host_hw, dtype=np.int32)
        with torch.cuda.stream(self._copy):
            if self._consumed[b] is not None:
                self._copy.wait_event(self._consumed[b])
            e0 = torch.cuda.Event(enable_timing=self.timing)
            e0.record(self._copy)
            L.check(L.load().yunet_upload_windows(p(self.store.data), p(host_off), p(host_hw), p(P['rect_h']),
                                                  p(P['off_h']), sb.n, p(self._bufs[b]), self._bufs[b].numel(),
                                                  C.c_void_p(self._copy.cuda_stream)), 'yunet_upload_windows')
            e1 = torch.cuda.Event(enable_timing=self.timing)
            e1.record(self._copy)
        self._uploaded[it] = (b, e0, e1, total)

    def _fetch(self, it):
        """fetch='kernel': yunet_fetch_windows on the copy stream, after the plan (GPU wait) and after the pipeline that
        last read the buffer.  Both callers size the buffers for the batch's largest images, and the kernel skips (and
        flags) any rectangle that would not fit.  The byte count stays on the device (win_off[N])."""
        P = self._planned[it]
        b, sb, cp = it % 2, P['sb'], self._copy
        p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        with torch.cuda.stream(cp):
            cp.wait_event(P['ev'])
            if self._consumed[b] is not None:
                cp.wait_event(self._consumed[b])
            for t in (sb.src_off, sb.src_hw, P['rect'], P['off']):
                t.record_stream(cp)
            e0 = torch.cuda.Event(enable_timing=self.timing)
            e0.record(cp)
            L.check(L.load().yunet_fetch_windows(p(self.store.data), self.store.nbytes, p(sb.src_off), p(sb.src_hw),
                                                 p(P['rect']), p(P['off']), sb.n, p(self._bufs[b]),
                                                 self._bufs[b].numel(), p(self._status), C.c_void_p(cp.cuda_stream)),
                    'yunet_fetch_windows')
            e1 = torch.cuda.Event(enable_timing=self.timing)
            e1.record(cp)
        self._uploaded[it] = (b, e0, e1, P['off'][-1])

    def check(self):
        """fetch='kernel': raise if any fetch so far met an invalid plan row (YUNET_FETCH_BAD_* bits).  Synchronises the
        copy stream: for the end of an epoch or a test, not for every iteration."""
        if self._status is None:
            return
        self._copy.synchronize()
        bits = int(self._status.item())
        if bits:
            names = [nm for nm, v in (('rectangle outside its image', L.FETCH_BAD_RECT),
                                      ('source span outside the store', L.FETCH_BAD_SRC),
                                      ('destination outside the window buffer', L.FETCH_BAD_DST)) if bits & v]
            raise RuntimeError(f'yunet_fetch_windows skipped invalid plan rows (status {bits}: {", ".join(names)})')

    def run(self, it):
        """The pipeline of iteration it on the current stream -> (batch dict, (e0, e1, bytes) of its upload; with
        fetch='kernel' bytes is a device scalar)."""
        cur = torch.cuda.current_stream(self.store.device)
        P = self._planned.pop(it)
        b, e0, e1, total = self._uploaded.pop(it)
        for k in [k for k in self._planned if k < it]:              # a caller that jumps around: drop stale plans
            del self._planned[k]
        for k in [k for k in self._uploaded if k < it]:
            del self._uploaded[k]
        cur.wait_event(P['ev'])
        cur.wait_event(e1)
        sb = P['sb']
        for t in (sb.src_off, sb.src_hw, sb.boxes, sb.kps, sb.gt_off, P['rect'], P['off']) + \
                ((sb.ign_boxes, sb.ign_off) if sb.ign_off is not None else ()):
            t.record_stream(cur)
        sizes = None
        if P['sizes_h'] is not None:
            P['ev'].synchronize()               # fetch='dma': upload() has waited on it already
            sizes = P['sizes_h'].numpy().copy()
        out = self.pipe.windowed(sb, it, self._bufs[b], P['rect'], P['off'], sizes=sizes)
        done = torch.cuda.Event(enable_timing=self.timing)
        done.record(cur)
        self._consumed[b] = done
        return out, (e0, e1, total)
