"""Shared by tests/test_oneshot_cases.py (CPU) and tests/test_oneshot_pieces_gpu.py: the message sizes at which the
one-shot all-reduce (csrc/collective.hip) is pinned, the order they are called in, and a host restatement of what the
kernel computes.  A helper module, not a test module.

The kernel sends a message of n floats in S = 1 | 2 | 4 | 8 PIECES per peer (S doubles while n * 4 > S * AR_PIECE_BYTES,
capped at AR_MAX_SUB) and reduces it in world * S SHARES.  Pieces and shares come from one partition rule, `ranges`."""
import os
import re

import torch

WORLDS = (2, 3)
COMM_BYTES = 320 * 1024          # the communicator size of tests/test_oneshot_gpu.py: a slot of 81920 floats

# last and first size of every S class, ragged sizes inside each class, the step's whole gradient (75861), a full slot
SIZES = (5, 16384, 16385, 20000, 32767, 32768, 32769, 40001, 65535, 65536, 65537, 75861, 81920)

# S along ORDER: 1 4 8 2 4 1 2 4 8 2 4 8 2 -- and round again (odd length: the second pass swaps the slot parities).
# Neighbours differ in S, so do calls two apart (the same parity, hence the same flags), also across the seam between
# two passes; 81920 (S = 8) comes two calls after 5 (S = 1), and at the seam 5 comes two calls after 65537 (S = 8), which
# leaves seven flags of that parity stale.
ORDER = (5, 40001, 81920, 32768, 32769, 16384, 20000, 65536, 75861, 32767, 65535, 65537, 16385)

GUARD = 4                        # sentinel floats in front of a message (and at least as many behind it)
SENTINEL = -7777.25


def source_path():
    import yunet_amd
    return os.path.join(list(yunet_amd.__path__)[0], 'csrc', 'collective.hip')


def source_text():
    with open(source_path()) as f:
        return f.read()


def _product(expr):
    v = 1
    for f in expr.split('*'):
        v *= int(f.strip())
    return v


def kernel_constants():
    """(AR_PIECE_BYTES, AR_MAX_SUB) as the package's own collective.hip declares them."""
    text = source_text()
    piece = re.search(r'constexpr\s+size_t\s+AR_PIECE_BYTES\s*=\s*([0-9][0-9* ]*);', text)
    sub = re.search(r'constexpr\s+int\s+AR_MAX_SUB\s*=\s*([0-9][0-9* ]*);', text)
    assert piece and sub, 'AR_PIECE_BYTES / AR_MAX_SUB not found in collective.hip'
    return _product(piece.group(1)), _product(sub.group(1))


def pieces(n):
    """S of a message of n floats (yunet_allreduce)."""
    piece_bytes, max_sub = kernel_constants()
    s = 1
    while s < max_sub and n * 4 > s * piece_bytes:
        s *= 2
    return s


def ranges(n, k):
    """The kernel's partition of n floats over k blocks: chunks of ceil(n / 4k) * 4 floats, clamped to n."""
    chunk = -(-n // (4 * k)) * 4
    return [(min(i * chunk, n), min(i * chunk + chunk, n)) for i in range(k)]


def owner(rs, i):
    """Index of the range of `rs` that element i lies in."""
    for b, (lo, hi) in enumerate(rs):
        if lo <= i < hi:
            return b
    return -1


def inputs(n, rank, it):
    g = torch.Generator().manual_seed(1000 * it + rank)
    return torch.randn(n, generator=g)


def want(xs, mean):
    """fp32, as the kernel: slots added in rank order, then (mean) MULTIPLIED by the fp32 constant 1 / world."""
    acc = xs[0].clone()
    for x in xs[1:]:
        acc += x
    if mean:
        acc *= torch.tensor(1.0 / len(xs), dtype=torch.float32)
    return acc


def schedule():
    """The calls of the bit-exact GPU test: ORDER twice, [(it, n, off, mean)].  `mean` alternates per call; `off` (floats
    between a 16-byte boundary and the message) is 0 for calls 0, 1, 4, 5, ... of the first pass and for the others of
    the second, so every size is called aligned once and unaligned once, and cycles through 1, 2, 3 otherwise."""
    calls, k = [], 0
    for it in range(2 * len(ORDER)):
        i, second = it % len(ORDER), it >= len(ORDER)
        aligned = (i % 4 < 2) != second
        off = 0
        if not aligned:
            off = 1 + k % 3
            k += 1
        calls.append((it, ORDER[i], off, bool(it % 2)))
    return calls
