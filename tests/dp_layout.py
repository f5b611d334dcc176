"""Strided image layouts of the ConvDPUnit descriptor (YunetDP.x_img_stride / z_img_stride) on the host: scatter a dense
[N, ...] tensor into a flat buffer whose images lie `stride` elements apart (optionally `off` elements into every
image's slot: a pyramid level inside the [N, P, 16] head output), gather it back, and check that the elements between
the images -- the gaps -- still hold the bit pattern they were filled with.  Host-only helper module (no GPU, no pytest
fixtures): tests/test_dp_layout.py checks it on the CPU, tests/test_dp_descriptor_gpu.py uses it around the kernels.

Gaps of INPUT buffers are filled with NaN (a kernel that reads one as halo or as a neighbour image poisons its output),
gaps of OUTPUT buffers with SENTINEL, a NaN with a payload no kernel produces, compared bit for bit afterwards."""
import torch

# quiet NaNs with a recognisable payload (fp32 / bf16 bit patterns, as signed integers of the same width)
SENTINEL = {torch.float32: 0x7FE5C3A1, torch.bfloat16: 0x7FE5, torch.uint8: 0xA5}
_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}


def bits(t):
    """the tensor's elements as integers of the same width (a view)"""
    return t.view(_BITS[t.dtype])


def filled(numel, dtype, device='cpu', pattern=None):
    """a flat buffer of `numel` elements: NaN everywhere (pattern None) or the given bit pattern"""
    buf = torch.empty(numel, dtype=dtype, device=device)
    if pattern is None:
        buf.fill_(float('nan'))
    else:
        bits(buf).fill_(pattern)
    return buf


def images(buf, n, stride, dense, off=0):
    """[n, dense] view of the image elements of a flat buffer: image i at i * stride + off"""
    assert buf.dim() == 1 and buf.is_contiguous()
    assert off >= 0 and stride >= off + dense and buf.numel() >= (n - 1) * stride + off + dense, \
        (buf.numel(), n, stride, dense, off)
    return buf.as_strided((n, dense), (stride, 1), buf.storage_offset() + off)


def scatter(dense, stride, off=0, pattern=None, numel=None):
    """dense [N, ...] -> flat buffer of N * stride elements (or `numel`), gaps NaN or `pattern`"""
    n = dense.shape[0]
    per = dense[0].numel()
    buf = filled(n * stride if numel is None else numel, dense.dtype, dense.device, pattern)
    images(buf, n, stride, per, off).copy_(dense.reshape(n, per))
    return buf


def gather(buf, shape, stride, off=0):
    """the images of a flat buffer as a dense tensor of `shape` = [N, ...] (a copy)"""
    n = shape[0]
    per = 1
    for s in shape[1:]:
        per *= s
    return images(buf, n, stride, per, off).clone().reshape(shape)


def gap_mask(numel, n, stride, dense, off=0, device='cpu'):
    """bool [numel]: True where no image element lies"""
    m = torch.ones(numel, dtype=torch.bool, device=device)
    images(m, n, stride, dense, off).fill_(False)
    return m


def gaps_hold(buf, n, stride, dense, off=0, pattern=None):
    """every gap element still has the bit pattern (default: the SENTINEL of the buffer's type)"""
    pattern = SENTINEL[buf.dtype] if pattern is None else pattern
    m = gap_mask(buf.numel(), n, stride, dense, off, buf.device)
    return bool((bits(buf)[m] == pattern).all())
