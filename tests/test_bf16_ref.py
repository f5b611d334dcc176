"""CPU: the checkers of tests/bf16_ref.py reject the defects a bf16 kernel could have and accept legitimate rounding.

Each case builds a result from the fp64 reference of the contract, adds the rounding a correct kernel may show (fp32
accumulation noise, RNE storage, the other neighbour for an ambiguous operand) and shows it passes; then injects one
defect at a time and shows the checker that guards it fails."""
import pytest
import torch

import bf16_ref as R


def unit(cin, cout, g):
    return (torch.randn(cout, cin, generator=g, dtype=torch.float64) * (2.0 / (cin + cout)) ** 0.5,
            torch.randn(cout, generator=g, dtype=torch.float64) * 0.1,
            torch.randn(cout, 9, generator=g, dtype=torch.float64) * 0.3,
            torch.randn(cout, generator=g, dtype=torch.float64) * 0.1)


def noisy(t, rel, g):
    """fp32-like accumulation noise"""
    return t * (1 + rel * torch.randn(t.shape, generator=g, dtype=torch.float64))


def test_rne_bf16_matches_torch_on_fp32_values():
    g = torch.Generator().manual_seed(0)
    t = (torch.randn(100000, generator=g) * 10).float()
    assert torch.equal(R.rne_bf16(t.double()), t.to(torch.bfloat16).double())
    # exact midpoints round to even
    m = torch.tensor([1 + 2 ** -8, 1 + 3 * 2 ** -8, -(1 + 2 ** -8)], dtype=torch.float64)
    assert R.rne_bf16(m).tolist() == [1.0, 1 + 2 ** -6, -1.0]
    assert bool(R.ambiguous(m).all()) and not bool(R.ambiguous(torch.tensor([1.0, 1.5])).any())


@pytest.fixture(scope='module')
def fwd_case():
    """a 64 -> 64 unit with the input BN (the bf16-GEMM rule) and a 16 -> 16 unit (fp32 rule)"""
    g = torch.Generator().manual_seed(1)
    out = {}
    for cin in (64, 16):
        x = R.rne_bf16(torch.randn(2, 16, 32, cin, generator=g, dtype=torch.float64) * 2 + 0.5)
        w = unit(cin, cin, g)
        bn = R.BNRef(R.stats_of(x), torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * .2, x[..., 0].numel())
        ref = R.fwd_ref(x, *w, in_bn=bn, bf16_gemm=cin == 64)
        out[cin] = (x, w, bn, ref)
    return out


@pytest.mark.parametrize('cin', [64, 16])
def test_bf16_output_checker(cin, fwd_case):
    x, w, bn, ref = fwd_case[cin]
    g = torch.Generator().manual_seed(2)
    z = ref['z']
    good = R.rne_bf16(noisy(z, 2 ** -24 * 8, g))
    if cin == 64:
        assert int(R.ambiguous(bn.act(x)).sum()) > 0, 'the case must hold ambiguous operands'
        # the kernel rounding every ambiguous operand to the OTHER neighbour is still legitimate
        a = bn.act(x)
        aq = R.rne_bf16(a)
        flip = torch.where(R.ambiguous(a), aq + torch.where(aq > a, -1.0, 1.0) * R.ulp_bf16(a), aq)
        p = flip @ R.rne_bf16(w[0]).t() + w[1]
        good = R.rne_bf16(R.depthwise(p, w[2], w[3]))
    R.check_bf16('good', good, z, ref['mag'], ref['terms'], ref['amb'])
    # one element off by two bf16 ulps
    big = (z.abs() > z.abs().max() * 0.2).nonzero()[0].tolist()
    bad = good.clone()
    bad[tuple(big)] += 2 * R.ulp_bf16(z[tuple(big)])
    with pytest.raises(AssertionError):
        R.check_bf16('2 ulps', bad, z, ref['mag'], ref['terms'], ref['amb'])
    # one tile's edge column (x = 15 of the 8 x 16 tile at (8, 0)) with the depthwise tap shifted by one column
    a = bn.act(x)
    aq, wq = (R.rne_bf16(a), R.rne_bf16(w[0])) if cin == 64 else (a, w[0])
    p = aq @ wq.t() + w[1]
    shifted = torch.roll(p, shifts=-1, dims=2)
    shifted[:, :, -1] = 0
    zs = R.depthwise(shifted, w[2], w[3])             # every tap one column to the right
    bad = good.clone()
    bad[:, 8:16, 15] = R.rne_bf16(zs[:, 8:16, 15])
    with pytest.raises(AssertionError):
        R.check_bf16('halo', bad, z, ref['mag'], ref['terms'], ref['amb'])


def test_fp32_gradient_checker_at_a_walk_shape():
    """dW1 of a 64 -> 64 unit at (12, 80, 80): 600 8 x 16 tiles, more than the 256-workgroup grid; one tile's
    contribution dropped or counted twice must fail, fp32 noise must pass"""
    g = torch.Generator().manual_seed(3)
    n, h, w, c = 12, 80, 80, 64
    x = R.rne_bf16(torch.randn(n, h, w, c, generator=g, dtype=torch.float64) * 2 + 0.5)
    W = unit(c, c, g)
    dz = torch.randn(n, h, w, c, generator=g, dtype=torch.float64)
    ref = R.bwd_ref(x, *W, z=None, dy=dz, bf16_gemm=True)
    good = noisy(ref['dw1'], 2 ** -22, g)
    R.check_fp32('dw1 good', good, ref['dw1'], 5e-5, amb=ref['amb']['dw1'], ch_dim=0)
    # one tile's share: the same gradient with dz outside tile (image 5, rows 40..47, columns 16..31) zeroed
    dt = torch.zeros_like(dz)
    dt[5, 40:48, 16:32] = dz[5, 40:48, 16:32]
    tile = R.bwd_ref(x, *W, z=None, dy=dt, bf16_gemm=True)['dw1']
    for k, bad in (('dropped', ref['dw1'] - tile), ('twice', ref['dw1'] + tile)):
        with pytest.raises(AssertionError):
            R.check_fp32('dw1 ' + k, bad, ref['dw1'], 5e-5, amb=ref['amb']['dw1'], ch_dim=0)


def _tied_pool_case():
    """raw fp32 z whose windows hold values that differ in fp32 but round to the same bf16 value"""
    g = torch.Generator().manual_seed(4)
    z32 = (torch.randn(2, 8, 12, 16, generator=g) * 2).float()
    w = R.windows(z32.double())
    # window (0, 1, 2) channel 3: positions 1 and 2 tie in bf16, position 2 larger in fp32
    base = torch.tensor(1.5, dtype=torch.float32)
    w[0, 1, 2, 3] = torch.tensor([0.1, float(base), float(base + 2 ** -12), -1.0], dtype=torch.float64)
    n, ho, wo, c, _ = w.shape
    z32 = w.view(n, ho, wo, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(n, 2 * ho, 2 * wo, c).float()
    gamma = torch.rand(c, generator=g) + 0.5
    gamma[5], gamma[7] = -0.7, 0.0
    return z32, gamma


def test_pool_checker():
    z32, gamma = _tied_pool_case()
    z16 = z32.to(torch.bfloat16)
    idx = R.pool_rule_idx(z16.double(), gamma)
    winners = torch.gather(R.windows(z16), -1, idx.unsqueeze(-1)).squeeze(-1)
    assert int(idx[0, 1, 2, 3]) == 1 and int((idx[..., 7] != 0).sum()) == 0
    R.check_pool('good', z16, winners, idx.to(torch.uint8), gamma)
    # winner taken before rounding (the fp32 maximum of a bf16 tie: position 2) where the contract takes it after
    idx_pre = R.pool_rule_idx(z32.double(), gamma)
    assert int(idx_pre[0, 1, 2, 3]) == 2
    win_pre = torch.gather(R.windows(z16), -1, idx_pre.unsqueeze(-1)).squeeze(-1)
    with pytest.raises(AssertionError):
        R.check_pool('before rounding', z16, win_pre, idx_pre.to(torch.uint8), gamma)
    # the right position, but a winner value that is not the stored one (rounded from another value)
    win_raw = torch.gather(R.windows(z32), -1, idx.unsqueeze(-1)).squeeze(-1)
    bad = winners.clone()
    bad[0, 1, 2, 3] = win_raw[0, 1, 2, 3].to(torch.bfloat16) + torch.tensor(2 ** -7, dtype=torch.bfloat16)
    with pytest.raises(AssertionError):
        R.check_pool('unrounded winner', z16, bad, idx.to(torch.uint8), gamma)
    # gradient routing: the pooled gradient on the recorded element passes, on a non-maximal element it fails
    g = torch.Generator().manual_seed(5)
    dpool = torch.randn(idx.shape, generator=g, dtype=torch.float64)
    dense = R.expand_pooled(dpool, idx)
    R.check_routing('good', dense, dpool, idx)
    wrong = idx.clone()
    wrong[0, 1, 2, 3] = 0                              # value 0.1: not a maximum of its window
    with pytest.raises(AssertionError):
        R.check_routing('non-maximal', R.expand_pooled(dpool, wrong), dpool, idx)
