"""CPU: the case table of tests/test_oneshot_pieces_gpu.py against the constants and the partition rule of
csrc/collective.hip, and its host restatement of the kernel's arithmetic against fp64.  No GPU, never skips: when the
kernel's constants change, these fail until tests/oneshot_cases.py follows."""
import re

import pytest
import torch

import oneshot_cases as K

PIECE_BYTES, MAX_SUB = K.kernel_constants()
CLASSES = [s for s in (1, 2, 4, 8) if s <= MAX_SUB]
FP64_SIZES = (16385, 40001, 65537)


def _class_bounds(s):
    """First and last n (floats) with pieces(n) == s; the last class is open-ended: None."""
    first = 1 if s == 1 else (s // 2) * PIECE_BYTES // 4 + 1
    last = None if s == MAX_SUB else s * PIECE_BYTES // 4
    return first, last


def test_constants_are_the_ones_the_table_was_written_for():
    assert (PIECE_BYTES, MAX_SUB) == (64 * 1024, 8)
    assert CLASSES == [1, 2, 4, 8]
    assert [K.pieces(n) for n in K.SIZES] == [1, 1, 2, 2, 2, 2, 4, 4, 4, 4, 8, 8, 8]
    assert sorted(K.ORDER) == sorted(K.SIZES) and len(K.ORDER) % 2 == 1
    assert K.ORDER[0] == 5, 'the first message is the smallest: a transport that cannot run shows it there'


def test_ranges_is_the_partition_rule_in_the_kernel_source():
    """`ranges` restates one rule that the kernel spells out three times: pieces over S, shares over nb = world * S in
    the reduce branch and again in the poison branch.  The rule's text is pinned here so that an edit of the kernel's
    rounding cannot leave the table's piece / share conditions describing another partition."""
    text = K.source_text()
    piece = re.findall(r'piece = \(\(n \+ \(size_t\)S \* 4 - 1\) / \(\(size_t\)S \* 4\)\) \* 4;', text)
    share = re.findall(r'share = \(\(n \+ nb \* 4 - 1\) / \(nb \* 4\)\) \* 4;', text)
    assert len(piece) == 1 and len(share) == 2
    assert len(re.findall(r'nb = \(size_t\)a\.world \* S;', text)) == 2
    # the rule itself, by hand: 40001 floats in 4 pieces of ceil(40001 / 16) * 4 = 10004, the last one 9989
    assert K.ranges(40001, 4) == [(0, 10004), (10004, 20008), (20008, 30012), (30012, 40001)]
    assert K.ranges(5, 6) == [(0, 4), (4, 5), (5, 5), (5, 5), (5, 5), (5, 5)]


@pytest.mark.parametrize('s', CLASSES)
def test_table_holds_the_edges_of_every_class(s):
    first, last = _class_bounds(s)
    assert K.pieces(first) == s and (first == 1 or K.pieces(first - 1) == s // 2)
    if s == 1:
        # the class starts at one float (tests/test_oneshot_gpu.py runs 1 and 3); the table's small message is shorter
        # than two vectors and no multiple of 4, so it has a vector part, a scalar tail and empty shares
        assert any(4 < n < 8 for n in K.SIZES)
    else:
        assert first in K.SIZES
    if last is not None:
        assert K.pieces(last) == s and K.pieces(last + 1) == 2 * s
        assert last in K.SIZES
    else:
        assert K.COMM_BYTES // 4 in K.SIZES and K.pieces(K.COMM_BYTES // 4) == s


@pytest.mark.parametrize('s', [s for s in CLASSES if s >= 2])
def test_table_has_a_short_ragged_last_piece_in_every_class(s):
    """The scalar tail of the send loop: a last piece shorter than the others whose length is no multiple of 4."""
    hits = []
    for n in K.SIZES:
        if K.pieces(n) != s:
            continue
        rs = K.ranges(n, s)
        lens = [hi - lo for lo, hi in rs]
        if 0 < lens[-1] < lens[0] and lens[-1] % 4 and all(l == lens[0] for l in lens[:-1]):
            hits.append(n)
    assert hits, f'S = {s}'
    if s == 4:
        assert 40001 in hits and K.ranges(40001, 4)[-1] == (30012, 40001)


def _shares_spanning_two_pieces(n, s, world):
    seams = {lo for lo, hi in K.ranges(n, s) if 0 < lo < n}
    return sum(1 for lo, hi in K.ranges(n, world * s) if any(lo < c < hi for c in seams))


@pytest.mark.parametrize('world', K.WORLDS)
@pytest.mark.parametrize('s', [s for s in CLASSES if s >= 2])
def test_table_has_a_share_that_spans_two_pieces(s, world):
    """A block that reduces data sent by two different workgroups of a peer: the seam between two pieces lies strictly
    inside its share (so a share boundary lies strictly inside a piece as well)."""
    assert any(K.pieces(n) == s and _shares_spanning_two_pieces(n, s, world) for n in K.SIZES)
    if s == 4:
        assert _shares_spanning_two_pieces(40001, 4, world) == 3


@pytest.mark.parametrize('world', (2, 3, 4, 8))
def test_pieces_and_shares_tile_the_message(world):
    for n in K.SIZES:
        s = K.pieces(n)
        for k in (s, world * s):
            rs = K.ranges(n, k)
            assert len(rs) == k and rs[0][0] == 0 and rs[-1][1] == n
            for (lo, hi), (lo2, _) in zip(rs, rs[1:] + [(n, n)]):
                assert lo <= hi == lo2, (n, k)
            assert all(lo % 4 == 0 or lo == n for lo, _ in rs), (n, k)
            covered = torch.zeros(n, dtype=torch.int32)
            for lo, hi in rs:
                covered[lo:hi] += 1
            assert bool((covered == 1).all()), (n, k)


def test_schedule_meets_every_class_in_every_way():
    calls = K.schedule()
    assert [c[1] for c in calls] == list(K.ORDER) * 2
    assert [c[3] for c in calls] == [bool(i % 2) for i in range(len(calls))]
    assert {c[2] for c in calls} == {0, 1, 2, 3}
    ss = [K.pieces(c[1]) for c in calls]
    assert all(a != b for a, b in zip(ss, ss[1:])), 'neighbouring calls differ in S'
    assert all(a != b for a, b in zip(ss, ss[2:])), 'calls two apart (one parity, one set of flags) differ in S'
    assert any(a == MAX_SUB and b == 1 for a, b in zip(ss, ss[2:])), 'stale flags: S = 1 on the parity of an S = 8 call'
    assert any(a == 1 and b == MAX_SUB for a, b in zip(ss, ss[2:]))
    for n in K.SIZES:
        mine = [c for c in calls if c[1] == n]
        assert sorted(c[0] % 2 for c in mine) == [0, 1], 'both slot parities'
        assert sorted(c[3] for c in mine) == [False, True], 'the sum and the mean'
        assert sorted(c[2] > 0 for c in mine) == [False, True], 'a 16-byte aligned buffer and an unaligned one'
    for s in CLASSES:
        combos = {(c[2] > 0, c[3]) for c in calls if K.pieces(c[1]) == s}
        assert len(combos) == 4, f'S = {s}: aligned / unaligned x sum / mean'


def _xs(n, world):
    return [K.inputs(n, r, 31) for r in range(world)]


@pytest.mark.parametrize('world', K.WORLDS)
@pytest.mark.parametrize('n', FP64_SIZES)
def test_restatement_against_fp64(n, world):
    """Each of the world - 1 additions rounds once and no partial sum exceeds sum |x_r|; the mean adds the rounding of
    the constant 1 / world and that of the product."""
    xs = _xs(n, world)
    exact = torch.stack([x.double() for x in xs]).sum(0)
    mag = torch.stack([x.double().abs() for x in xs]).sum(0)
    u = 2.0 ** -24
    err = (K.want(xs, False).double() - exact).abs()
    bound = (world - 1) * u * mag
    print(f'n={n} world={world} sum: worst error / bound = {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all())
    err = (K.want(xs, True).double() - exact / world).abs()
    bound = (world + 1) * u * mag / world
    print(f'n={n} world={world} mean: worst error / bound = {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all())


@pytest.mark.parametrize('n', FP64_SIZES)
def test_cases_tell_summation_orders_and_the_division_apart(n):
    """With three addends a kernel that adds the slots in another order, or divides by world where this one multiplies
    by the fp32 constant 1 / world, gives other bits in a large part of the message."""
    xs = _xs(n, 3)
    w = K.want(xs, False)
    for other in ((xs[2] + xs[1]) + xs[0], (xs[0] + xs[2]) + xs[1]):
        frac = float((w != other).float().mean())
        print(f'n={n}: {frac:.3f} of the elements differ in another order')
        assert frac > 0.10
    frac = float((K.want(xs, True) != w / 3).float().mean())
    print(f'n={n}: {frac:.3f} of the means differ from a division')
    assert frac > 0.10
    assert torch.equal(K.want(xs, True), w * torch.tensor(1.0 / 3.0, dtype=torch.float32))
    assert torch.equal(K.want(xs[:2], True), (xs[0] + xs[1]) * 0.5)
