"""CPU: the eval-mode checkers of tests/eval_ref.py reject the defects an eval path could have.  Each test emulates the
kernel in fp32 (coefficients recovered from synthesised sums, as the kernels do), first shows that the clean emulation
passes, then injects one defect and shows the checker fails on it."""
import pytest
import torch
import torch.nn.functional as F

import bf16_ref as R
import eval_ref as E

N, H, W = 2, 8, 12
COUNT = 465920          # the stride-2 map of one 1120 x 1664 image: the count behind the stem's BatchNorm


def _state(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, H, W, cin, generator=g) * 1.5 + 0.4).to(torch.bfloat16).double()
    x[:, :, W - 3:] = 0.0                    # a zero-padded right band, as the test images have
    w1 = torch.randn(cout, cin, generator=g).double() * (2.0 / (cin + cout)) ** 0.5
    b1 = torch.randn(cout, generator=g).double() * 0.1
    w2 = torch.randn(cout, 9, generator=g).double() * 0.3
    b2 = torch.randn(cout, generator=g).double() * 0.1
    rm = (torch.randn(cin, generator=g) * 0.3 + 0.4).float()
    rv = (torch.rand(cin, generator=g) * 2 + 0.2).float()
    rv[:8] = 1e-4                             # variances where eps matters
    rm[8], rv[8] = 50.0, 1e-8                 # the cancellation case of mode 2
    rv[9] = 1e4
    gam = (torch.rand(cin, generator=g) + 0.5).float()
    gam[10], gam[11] = -0.8, 0.0
    bet = (torch.randn(cin, generator=g) * 0.2).float()
    return x, (w1, b1, w2, b2), rm, rv, gam, bet


def _kernel_act(x, bn):
    """common.h bnrelu in fp32 from the recovered (fp64) coefficients"""
    mean, inv = bn.mean_invstd()
    scale = bn.gamma.float() * inv.float()
    return torch.relu((x.float() - mean.float()) * scale + bn.beta.float())


def _kernel_unit(x, wts, bn=None, halo_shift=False):
    """ConvDPUnit forward in fp32; halo_shift: the depthwise reads the last column again in place of the zero halo
    on the right border"""
    w1, b1, w2, b2 = [t.float() for t in wts]
    a = _kernel_act(x, bn) if bn is not None else x.float()
    p = (a @ w1.t() + b1).permute(0, 3, 1, 2)
    pp = F.pad(p, (1, 1, 1, 1))
    if halo_shift:
        pp[..., 1:-1, -1] = pp[..., 1:-1, -2]
    z = F.conv2d(pp, w2.reshape(-1, 1, 3, 3), b2, groups=p.shape[1])
    return z.permute(0, 2, 3, 1)


def _eval_bn(rm, rv, gam, bet, block=None):
    """the kernels' view of a running-statistics BN: mode 2's sums (or a given block), recovered as common.h does"""
    if block is None:
        block = E.synthesised_sums(rm, rv, COUNT)
    return E.SumsBN(block, COUNT, gam, bet)


def _ref(x, wts, rm, rv, gam, bet, bf16_gemm=False):
    return E.unit_ref(x, *wts, in_bn=R.RunningBNRef(rm, rv, gam, bet), bf16_gemm=bf16_gemm)


def test_clean_emulation_passes():
    x, wts, rm, rv, gam, bet = _state(64, 64, 1)
    r = _ref(x, wts, rm, rv, gam, bet)
    E.check('clean unit', _kernel_unit(x, wts, _eval_bn(rm, rv, gam, bet)), r, 'fp32')
    E.check('clean unit bf16', _kernel_unit(x, wts, _eval_bn(rm, rv, gam, bet)).to(torch.bfloat16), r, 'bf16')
    # and the other ops: pooled tap, TFPN merge
    bn = R.RunningBNRef(rm, rv, gam, bet)
    kbn = _eval_bn(rm, rv, gam, bet)
    E.check('clean pool', R.windows(_kernel_act(x, kbn)).amax(-1), E.plain_pool_ref(x, bn), 'fp32')
    xs = x[:, ::2, ::2]
    got = _kernel_act(x, kbn) + E._up2(_kernel_act(xs, kbn))
    E.check('clean upadd', got.to(torch.bfloat16), E.upadd_ref(x, xs, bn, bn), 'bf16')


def test_rejects_batch_statistics():
    x, wts, rm, rv, gam, bet = _state(64, 64, 2)
    r = _ref(x, wts, rm, rv, gam, bet)
    batch = R.BNRef(R.stats_of(x), gam, bet, N * H * W)
    with pytest.raises(AssertionError):
        E.check('batch statistics', _kernel_unit(x, wts, batch), r, 'fp32')


def test_rejects_unbiased_running_var():
    x, wts, rm, rv, gam, bet = _state(64, 64, 3)
    r = _ref(x, wts, rm, rv, gam, bet)
    c = N * H * W
    with pytest.raises(AssertionError):
        E.check('unbiased var', _kernel_unit(x, wts, _eval_bn(rm, rv.double() * c / (c - 1), gam, bet)), r, 'fp32')


def test_rejects_dropped_eps():
    x, wts, rm, rv, gam, bet = _state(64, 64, 4)
    r = _ref(x, wts, rm, rv, gam, bet)
    bn = _eval_bn(rm, rv, gam, bet)
    bn.eps = 0.0
    with pytest.raises(AssertionError):
        E.check('eps dropped', _kernel_unit(x, wts, bn), r, 'fp32')


def test_rejects_leftover_replica_sums():
    x, wts, rm, rv, gam, bet = _state(64, 64, 5)
    r = _ref(x, wts, rm, rv, gam, bet)
    block = E.synthesised_sums(rm, rv, COUNT)
    E.check('zeroed replicas', _kernel_unit(x, wts, _eval_bn(rm, rv, gam, bet, block)), r, 'fp32')
    block[3] = R.stats_of(x)                  # a training step's sums left in slot 3
    with pytest.raises(AssertionError):
        E.check('slot 3 leftover', _kernel_unit(x, wts, _eval_bn(rm, rv, gam, bet, block)), r, 'fp32')


def test_rejects_swapped_landmark_channels():
    x, wts, rm, rv, gam, bet = _state(64, 16, 6)
    r = _ref(x, wts, rm, rv, gam, bet)
    got = _kernel_unit(x, wts, _eval_bn(rm, rv, gam, bet))
    E.check('heads', got, r, 'fp32')
    bad = got.clone()
    bad[..., [8, 9]] = got[..., [9, 8]]       # the second landmark's x and y
    with pytest.raises(AssertionError):
        E.check('landmarks swapped', bad, r, 'fp32')


def test_rejects_shifted_border_halo():
    x, wts, rm, rv, gam, bet = _state(64, 64, 7)
    r = _ref(x, wts, rm, rv, gam, bet)
    with pytest.raises(AssertionError):
        E.check('halo shifted', _kernel_unit(x, wts, _eval_bn(rm, rv, gam, bet), halo_shift=True), r, 'fp32')


def test_rejects_two_ulp_element():
    x, wts, _, _, _, _ = _state(16, 16, 8)
    r = E.unit_ref(x, *wts)
    got = _kernel_unit(x, wts).to(torch.bfloat16)
    E.check('bf16 z', got, r, 'bf16')
    m, _ = torch.frexp(r['z'])
    i = int(((m.abs() > 0.6) & (m.abs() < 0.9)).reshape(-1).nonzero()[0])     # mid-binade: ulp(ref) = ulp(got)
    bad = got.clone().reshape(-1)
    bad[i] = (bad[i].double() + 2 * R.ulp_bf16(bad[i:i + 1])[0]).to(torch.bfloat16)
    with pytest.raises(AssertionError):
        E.check('2 ulps', bad.reshape(got.shape), r, 'bf16')


def test_rejects_winner_chosen_before_rounding():
    g = torch.Generator().manual_seed(9)
    z32 = torch.randn(1, 4, 4, 8, generator=g).float()
    # window (0, 0) of channel 0: 1 and 1 + 2^-10 round to the same bf16 value; the unrounded maximum is position 3
    z32[0, 0, 0, 0], z32[0, 0, 1, 0], z32[0, 1, 0, 0], z32[0, 1, 1, 0] = 1.0, -2.0, -3.0, 1.0 + 2.0 ** -10
    gam = torch.rand(8, generator=g) + 0.5
    z16 = z32.to(torch.bfloat16)
    rule = R.pool_rule_idx(z16, gam)
    winners = torch.gather(R.windows(z16), -1, rule.unsqueeze(-1)).squeeze(-1)
    E.pool_rule(z16, winners, rule.to(torch.uint8), gam, 'rule')
    early = torch.argmax(R.windows(z32) * torch.sign(gam).view(1, 1, 1, -1, 1), dim=-1)
    assert int(early[0, 0, 0, 0]) == 3 and int(rule[0, 0, 0, 0]) == 0
    early_w = torch.gather(R.windows(z16), -1, early.unsqueeze(-1)).squeeze(-1)
    with pytest.raises(AssertionError):
        E.pool_rule(z16, early_w, early.to(torch.uint8), gam, 'before rounding')


def test_recover_matches_running_statistics():
    """mode 2's sums recovered as common.h does give back the running statistics (the cancellation at |m| = 50,
    v = 1e-8 stays within a few fp64 ulps of v + m^2)"""
    _, _, rm, rv, _, _ = _state(64, 64, 10)
    mean, var, inv = E.recover(E.synthesised_sums(rm, rv, COUNT), COUNT)
    m, v = rm.double(), rv.double()
    assert float(((mean - m).abs() / m.abs().clamp_min(1e-30)).max()) <= 1e-12
    assert bool(((var - v).abs() <= 4 * 2.0 ** -52 * (v + m * m)).all())
