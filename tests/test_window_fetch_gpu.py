"""-m gpu: yunet_fetch_windows (csrc/source.hip) -- the GPU reading crop windows from the pinned host store itself, with
the plan in device memory -- byte-exact against numpy slicing of the store, invalid plan rows skipped and flagged on
the device, pageable memory refused, and WindowFeed(fetch='kernel') bit-identical to the other feeds without a host
wait."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_pipeline_gpu import make_pipe
from test_source_store_gpu import _same, _sources, _store, _write_labelv2

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 0xA5


def _p(x):
    return C.c_void_p(x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())


def _fetch(host, store_bytes, src_off, src_hw, rect, win_off, win, win_bytes, status):
    """One yunet_fetch_windows call on the current stream (device tables as numpy or device tensors)."""
    import yunet_amd._lib as L
    d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(DEV)   # noqa: E731
    t = [d(src_off, np.int64), d(src_hw, np.int32), d(rect, np.int32), d(win_off, np.int64)]
    n = int(t[1].shape[0])
    return L.load().yunet_fetch_windows(_p(host), int(store_bytes), *[_p(x) for x in t], n, _p(win), int(win_bytes),
                                        _p(status), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def fetch_np(store, src_off, src_hw, rect, win_off, win, win_bytes):
    """numpy restatement of yunet_fetch_windows on a copy of `win` -> (window buffer, OR of the status bits)."""
    out, bits, before = win.copy(), 0, 0
    S = store.shape[0]
    for n in range(len(rect)):
        r0, c0, rows, cols = (int(v) for v in rect[n])
        h, w = (int(v) for v in src_hw[n])
        so, a, b = int(src_off[n]), int(win_off[n]), int(win_off[n + 1])
        bad, nbytes = 0, 0
        if min(r0, c0, rows, cols) < 0 or r0 + rows > h or c0 + cols > w:
            bad |= 1
        else:
            nbytes = rows * cols * 3
        if nbytes > 0 and (so < 0 or so > S or (r0 + rows - 1) * w + c0 + cols > (S - so) // 3):
            bad |= 2
        if a < before or b < a or nbytes > b - a or a > win_bytes or nbytes > win_bytes - a:
            bad |= 4
        before = max(before, a)
        bits |= bad
        if bad or nbytes == 0:
            continue
        for r in range(rows):
            s = so + ((r0 + r) * w + c0) * 3
            out[a + r * cols * 3:a + (r + 1) * cols * 3] = store[s:s + cols * 3]
    return out, bits


def _pinned_store(sizes, seed=0, skew=0):
    """Random pixels for images of `sizes`, packed back to back after `skew` bytes of a pinned buffer; the last image ends
    exactly at the end of the buffer.  -> (pinned tensor [skew:], its numpy view, offsets)."""
    nbytes = [h * w * 3 for h, w in sizes]
    full = torch.empty(skew + sum(nbytes), dtype=torch.uint8, pin_memory=True)
    full.numpy()[:] = np.random.default_rng(seed).integers(0, 256, full.numel(), dtype=np.uint8)
    data = full[skew:]
    return data, data.numpy(), np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)


def _check(data, store, src_off, hw, rect, win_off, win_bytes, extra=64):
    """Run the kernel and the numpy restatement on the same sentinel-filled buffer; -> status bits."""
    win = torch.full((int(win_bytes) + extra,), SENTINEL, dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _fetch(data, store.shape[0], src_off, hw, rect, win_off, win, win_bytes, status)
    assert rc == 0
    torch.cuda.synchronize()
    want, bits = fetch_np(store, src_off, hw, rect, win_off, np.full(win.numel(), SENTINEL, np.uint8), win_bytes)
    got = win.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f'{bad.size} bytes differ, first at {bad[:8].tolist()}'
    assert int(status.item()) == bits
    return bits


def _pack(rect, gaps=None):
    """win_off for `rect`: packed in order, with window n starting at residue gaps[n] mod 16 when given."""
    off = [0]
    for n, (_, _, rows, cols) in enumerate(rect):
        a = off[-1]
        if gaps is not None:
            a += (int(gaps[n]) - a) % 16
        off[-1] = a
        off.append(a + rows * cols * 3)
    return np.array(off, dtype=np.int64)


def test_fetch_equals_store_slices_on_a_real_plan():
    from yunet_amd.source_store import window_plan_np
    srcs = _sources(5)
    st = _store(srcs, placement='host')
    idx = [6, 3, 3, 0, 9, 6, 8, 1, 2, 5, 4, 7, 3]
    sb = st.batch(idx)
    store = st.data.numpy()
    for it in range(3):
        params, rect, off = make_pipe(96, 5).window_plan(sb, it, torch.device(DEV))
        r_np, o_np = window_plan_np(params.cpu().numpy(), sb.src_hw.cpu().numpy())
        total = int(o_np[-1])
        win = torch.full((total + 256,), SENTINEL, dtype=torch.uint8, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        import yunet_amd._lib as L
        assert L.load().yunet_fetch_windows(_p(st.data), st.nbytes, _p(sb.src_off), _p(sb.src_hw), _p(rect), _p(off),
                                            sb.n, _p(win), win.numel(), _p(status),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        parts = []
        for n, i in enumerate(idx):
            y0, x0, rh, rw = (int(v) for v in r_np[n])
            h, w = srcs[i][0].shape[:2]
            o = int(st.offsets[i])
            parts.append(store[o:o + h * w * 3].reshape(h, w, 3)[y0:y0 + rh, x0:x0 + rw].reshape(-1))
        got = win.cpu().numpy()
        assert np.array_equal(got[:total], np.concatenate(parts))
        assert (got[total:] == SENTINEL).all()
        assert int(status.item()) == 0


@pytest.mark.parametrize('skew', [0, 7])
def test_fetch_hand_made_plans(skew):
    """Every residue of source and destination start mod 16, narrow (1, 5, 6 columns) and one-pixel-wide images, rows
    wider than a chunk, rectangles on the right / bottom edges, the last image ending at store_bytes, empty rectangles;
    skew 7: the store starts 7 bytes into its pinned allocation (blocks crossing the store's first byte)."""
    sizes = [(40, 37), (50, 1), (31, 64), (3, 20000), (300, 400), (23, 29)]
    data, store, offs = _pinned_store(sizes, seed=skew, skew=skew)
    hw = np.array(sizes, dtype=np.int32)
    base = data.data_ptr()
    img, rect, dres = [], [], []
    colset = [1, 5, 6, 7, 11, 16, 17, 21]        # <= 22: 16 start columns fit
    for s in range(16):                      # source start residue s (device address), destination residue d
        for d in range(16):
            cols = colset[(s + d) % len(colset)]
            rows = 1 + (s * 16 + d) % 4
            r0 = (s + 3 * d) % (40 - rows)
            c0 = next(c for c in range(37 - cols + 1) if (base + offs[0] + (r0 * 37 + c) * 3) % 16 == s)
            img.append(0); rect.append((r0, c0, rows, cols)); dres.append(d)
    extra = [(1, (0, 0, 50, 1)), (1, (5, 0, 3, 1)),                         # w = 1
             (2, (31 - 4, 64 - 9, 4, 9)), (0, (40 - 2, 37 - 5, 2, 5)),     # right / bottom edges
             (3, (0, 0, 3, 20000)), (3, (1, 17, 2, 19983)),                 # 60 KB rows: split across chunks
             (4, (0, 0, 300, 400)), (4, (13, 7, 250, 333)),                 # many chunks
             (5, (0, 0, 23, 29)), (5, (22, 0, 1, 29)), (5, (20, 28, 3, 1)),  # ends at store_bytes
             (0, (0, 0, 0, 0)), (2, (3, 4, 0, 5)), (4, (2, 2, 3, 0)),       # empty
             (0, (0, 0, 40, 37))]
    for i, r in extra:
        img.append(i); rect.append(r); dres.append(len(dres) % 16)
    rect = np.array(rect, dtype=np.int32)
    img = np.array(img)
    off = _pack(rect, dres)
    assert _check(data, store, offs[img], hw[img], rect, off, int(off[-1])) == 0
    # the same rectangles in another order, packed without gaps
    perm = np.random.default_rng(1).permutation(len(rect))
    assert _check(data, store, offs[img][perm], hw[img][perm], rect[perm], _pack(rect[perm]), int(off[-1]) + 5) == 0


def test_fetch_4096_images():
    sizes = [(17, 23), (64, 61), (5, 3), (90, 101), (2, 200)]
    data, store, offs = _pinned_store(sizes, seed=3)
    rng = np.random.default_rng(4)
    img = rng.integers(0, len(sizes), 4096)
    hw = np.array(sizes, dtype=np.int32)[img]
    rows = rng.integers(0, hw[:, 0] + 1)
    cols = rng.integers(0, hw[:, 1] + 1)
    r0 = rng.integers(0, hw[:, 0] - rows + 1)
    c0 = rng.integers(0, hw[:, 1] - cols + 1)
    rect = np.stack([r0, c0, rows, cols], 1).astype(np.int32)
    off = _pack(rect, rng.integers(0, 16, 4096))
    assert _check(data, store, offs[img], hw, rect, off, int(off[-1])) == 0


def test_invalid_plan_rows_are_skipped_and_flagged():
    """A rectangle past its image, a source span past the store, a destination past win_bytes and a decreasing win_off:
    the status bits are set, nothing outside the valid rectangles' destinations changes, the valid ones are exact.
    Every read of a valid row stays inside the pinned store by construction."""
    import yunet_amd._lib as L
    sizes = [(40, 37), (31, 64), (23, 29), (60, 50)]
    data, store, offs = _pinned_store(sizes, seed=5)
    hw_s = np.array(sizes, dtype=np.int32)
    rng = np.random.default_rng(6)
    img = rng.integers(0, len(sizes), 24)
    hw = hw_s[img]
    rows = rng.integers(1, hw[:, 0] + 1)
    cols = rng.integers(1, hw[:, 1] + 1)
    rect = np.stack([hw[:, 0] - rows, hw[:, 1] - cols, rows, cols], 1).astype(np.int32)
    src_off = offs[img].copy()
    off = _pack(rect, rng.integers(0, 16, 24))
    nbytes = rect[:, 2].astype(np.int64) * rect[:, 3] * 3
    assert (nbytes >= 7).all()
    win_bytes = int(off[-1])
    assert _check(data, store, src_off, hw, rect, off, win_bytes) == 0          # the valid plan first
    cases = []
    r = rect.copy(); r[3, 0] += 1                                                # one row past the bottom
    cases.append((src_off, r, off, win_bytes, L.FETCH_BAD_RECT))
    r = rect.copy(); r[5, 1] = -1                                                # negative column
    cases.append((src_off, r, off, win_bytes, L.FETCH_BAD_RECT))
    so = src_off.copy(); so[7] = store.shape[0] - 10                             # source span past the store
    cases.append((so, rect, off, win_bytes, L.FETCH_BAD_SRC))
    cases.append((src_off, rect, off, win_bytes - 1, L.FETCH_BAD_DST))          # the last window past win_bytes
    o = off.copy(); o[10] = off[9] + nbytes[9] - 7                              # decreasing: window 9 overruns
    cases.append((src_off, rect, o, win_bytes, L.FETCH_BAD_DST))
    o = off.copy(); o[12] = o[20]                                                # jumps ahead: 12..19 start before it
    cases.append((src_off, rect, o, win_bytes, L.FETCH_BAD_DST))
    for so, r, o, wb, bit in cases:
        got = _check(data, store, so, hw, r, o, wb)
        assert got == bit, (got, bit)
    # all three kinds at once
    r = rect.copy(); r[3, 0] += 1
    so = src_off.copy(); so[7] = store.shape[0] - 10
    o = off.copy(); o[10] = off[9] + nbytes[9] - 7
    assert _check(data, store, so, hw, r, o, win_bytes) == L.FETCH_BAD_RECT | L.FETCH_BAD_SRC | L.FETCH_BAD_DST


def test_pageable_memory_is_refused():
    import yunet_amd._lib as L
    store = np.random.default_rng(7).integers(0, 256, 40 * 37 * 3, dtype=np.uint8)     # plain numpy: pageable
    win = torch.full((1024,), SENTINEL, dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    rect = np.array([[0, 0, 4, 5]], np.int32)
    args = ([0], [[40, 37]], rect, [0, 60])
    assert _fetch(store, store.size, *args, win, win.numel(), status) == L.EINVAL
    torch.cuda.synchronize()
    assert (win.cpu().numpy() == SENTINEL).all() and int(status.item()) == 0
    # argument checks, also before any launch
    data, pinned, _ = _pinned_store([(40, 37)])
    assert _fetch(data, data.numel() + (1 << 40), *args, win, win.numel(), status) == L.EINVAL  # past the allocation
    assert _fetch(data, 0, *args, win, win.numel(), status) == L.EINVAL
    assert _fetch(data, data.numel(), *args, win, 0, status) == L.EINVAL
    torch.cuda.synchronize()
    assert (win.cpu().numpy() == SENTINEL).all() and int(status.item()) == 0
    assert _fetch(data, data.numel(), *args, win, win.numel(), status) == 0              # and the valid call works
    torch.cuda.synchronize()
    assert np.array_equal(win[:60].cpu().numpy(), pinned.reshape(40, 37, 3)[:4, :5].reshape(-1))


def test_synthetic_window_feed_kernel_fetch_equals_resident():
    import os
    import yunet_amd
    import yunet_amd.runner as R
    from yunet_amd.source_store import window_plan_np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yunet_amd.Config.fromfile(os.path.join(root, 'configs', 'yunet_s.py'))
    kw = dict(samples_per_gpu=12, pool=5, seed=3, src_hw=((300, 420), (512, 384), (200, 200)))
    a = R.SyntheticSourceImages(cfg.train_pipeline, **kw)
    b = R.SyntheticSourceImages(cfg.train_pipeline, host_fed='window', host_fetch='kernel', timing=True, **kw)
    totals = []
    for it in range(7):
        ba, bb = a.batch(it, DEV), b.batch(it, DEV)
        torch.cuda.synchronize()
        _same(ba, bb)
        _, off = window_plan_np(a.pipe.params.cpu().numpy(), a._src.src_hw.cpu().numpy())
        totals.append(int(off[-1]))
    b._feed.check()
    assert b._feed.fetch == 'kernel'
    rep = b.report(skip=0)
    assert rep['batches_timed'] == 7 and rep['h2d_ms'] > 0 and rep['pipeline_ms'] > 0
    assert rep['h2d_bytes'] == sum(totals) / len(totals)
    assert rep['h2d_bytes'] < rep['src_bytes'] == a._src.src.numel()


def test_feed_check_raises_on_a_flagged_fetch():
    import yunet_amd.runner as R
    import os
    import yunet_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yunet_amd.Config.fromfile(os.path.join(root, 'configs', 'yunet_s.py'))
    b = R.SyntheticSourceImages(cfg.train_pipeline, samples_per_gpu=4, pool=3, host_fed='window', host_fetch='kernel',
                                src_hw=((120, 160),))
    b.batch(0, DEV)
    b._feed.check()
    b._feed._status.fill_(4)
    with pytest.raises(RuntimeError, match='destination'):
        b._feed.check()


def test_retinaface_host_cache_kernel_fetch_bit_identical_and_decodes_once(tmp_path):
    from collections import Counter
    from yunet_amd.datasets import RetinaFaceDataset, RetinaFaceSource
    from test_pipeline_gpu import REF_PIPELINE
    ann, prefix = _write_labelv2(tmp_path)
    pipeline = [dict(p) for p in REF_PIPELINE]
    pipeline[3]['img_scale'] = (64, 64)
    srcs, calls = {}, {}
    for cache, fetch in ((None, None), ('host', 'kernel')):
        ds = RetinaFaceDataset(ann, img_prefix=prefix, pipeline=pipeline)
        c = calls[cache] = Counter()
        orig = ds.load_image

        def counted(i, orig=orig, c=c):
            c[i] += 1
            return orig(i)
        ds.load_image = counted
        srcs[cache] = RetinaFaceSource(ds, pipeline, samples_per_gpu=4, seed=2, workers=2, cache=cache,
                                       host_fetch=fetch)
    ipe = srcs[None].iters_per_epoch
    assert ipe >= 4
    for it in range(2 * ipe):
        outs = {k: s.batch(it, DEV) for k, s in srcs.items()}
        torch.cuda.synchronize()
        _same(outs[None], outs['host'])
    srcs['host']._feed.check()
    assert srcs['host']._feed.fetch == 'kernel'
    n = len(srcs[None].ds)
    assert set(calls['host']) == set(range(n)) and set(calls['host'].values()) == {1}, calls['host']


@pytest.mark.parametrize('fetch', ['kernel', 'dma'])
def test_kernel_fetch_never_waits_on_the_host(monkeypatch, fetch):
    """fetch='kernel' runs 5 iterations with Event.synchronize made to raise; the DMA feed (which waits on its plan
    event) trips the same patch, so the patch is live."""
    import os
    import yunet_amd
    import yunet_amd.runner as R
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yunet_amd.Config.fromfile(os.path.join(root, 'configs', 'yunet_s.py'))
    src = R.SyntheticSourceImages(cfg.train_pipeline, samples_per_gpu=8, pool=4, seed=1, host_fed='window',
                                  host_fetch=fetch, src_hw=((300, 420), (200, 200)))

    def no_wait(self):
        raise AssertionError('host wait on a CUDA event')
    monkeypatch.setattr(torch.cuda.Event, 'synchronize', no_wait)
    if fetch == 'dma':
        with pytest.raises(AssertionError, match='host wait'):
            src.batch(0, DEV)
        monkeypatch.undo()
        torch.cuda.synchronize()
        return
    outs = [src.batch(it, DEV)['img'].sum() for it in range(5)]
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(torch.isfinite(o) for o in outs)
    src._feed.check()
