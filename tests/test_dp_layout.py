"""tests/dp_layout.py on the CPU: the gather / scatter helper of the strided-descriptor kernel tests."""
import pytest
import torch

import dp_layout as D


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('n,per,stride,off', [(1, 12, 12, 0), (3, 12, 16, 0), (2, 3840, 3840 + 1028, 0),
                                              (5, 1600, 525 * 16, 400 * 16), (19, 1600, 2100 * 16, 0)])
def test_round_trip_and_gaps(dtype, n, per, stride, off):
    g = torch.Generator().manual_seed(n + per)
    dense = torch.randn(n, per // 4, 4, generator=g).to(dtype)
    for pattern in (None, D.SENTINEL[dtype]):
        buf = D.scatter(dense, stride, off, pattern)
        assert buf.numel() == n * stride and buf.dtype == dtype
        back = D.gather(buf, dense.shape, stride, off)
        assert torch.equal(D.bits(back), D.bits(dense))
        m = D.gap_mask(buf.numel(), n, stride, per, off)
        assert int(m.sum()) == n * (stride - per)
        # image i occupies exactly [i * stride + off, i * stride + off + per)
        for i in (0, n - 1):
            assert not bool(m[i * stride + off:i * stride + off + per].any())
            assert off == 0 or bool(m[i * stride:i * stride + off].all())
            assert bool(m[i * stride + off + per:(i + 1) * stride].all())
        if pattern is None:
            assert bool(torch.isnan(buf[m].float()).all()) and not bool(torch.isnan(buf[~m].float()).any())
        else:
            assert D.gaps_hold(buf, n, stride, per, off)
            assert bool(torch.isnan(buf[m].float()).all())          # the sentinel poisons whatever reads it
            assert stride == per or not D.gaps_hold(buf, n, stride, per, off, pattern=0)


def test_a_touched_gap_is_seen():
    """one gap element changed in one bit, anywhere -- in front of the first image, between two, behind the last"""
    n, per, stride, off = 3, 8, 20, 4
    dense = torch.arange(n * per, dtype=torch.float32).reshape(n, per)
    for pos in (0, off - 1, off + per, stride + 1, 2 * stride + off + per, n * stride - 1):
        buf = D.scatter(dense, stride, off, D.SENTINEL[torch.float32])
        assert D.gaps_hold(buf, n, stride, per, off)
        D.bits(buf)[pos] ^= 1
        assert not D.gaps_hold(buf, n, stride, per, off), pos
    # ... and a write into an image is not a gap write
    buf = D.scatter(dense, stride, off, D.SENTINEL[torch.float32])
    buf[stride + off] = 5.0
    assert D.gaps_hold(buf, n, stride, per, off)
    # a NaN of another payload is not the sentinel
    buf[0] = float('nan')
    assert not D.gaps_hold(buf, n, stride, per, off)


def test_views_and_bounds():
    buf = D.filled(40, torch.float32, pattern=D.SENTINEL[torch.float32])
    v = D.images(buf[4:], 2, 16, 8)                    # a level's pointer = the buffer from its base offset on
    v.fill_(1.0)
    assert float(buf[4:12].min()) == 1.0 and float(buf[20:28].min()) == 1.0
    assert D.gaps_hold(buf, 2, 16, 8, off=4)
    with pytest.raises(AssertionError):
        D.images(buf, 3, 16, 9)                        # the last image would end past the buffer
    with pytest.raises(AssertionError):
        D.images(buf, 2, 8, 9)                         # images overlap
    u8 = D.filled(10, torch.uint8, pattern=D.SENTINEL[torch.uint8])
    assert D.gaps_hold(u8, 1, 10, 4, off=2)
