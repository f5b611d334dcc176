"""-m gpu: every backward kernel under FROZEN BatchNorm (fine-tuning: engine.py Plan._reader_bn), against the fp64
references of tests/frozen_ref.py.

What is new next to every other kernel test: the statistics a kernel is handed are not those of the tensor it reads.  A
frozen layer's forward block is synthesised from its running statistics ([m count | (v + m^2) count]: frozen_ref.block,
what yunet_bn_batch mode 2 writes), the READER of its backward sums takes a zero block (common.h: c1 = c2 = 0, so
dz = k1 dy), and its consumers add [sum dy | sum dy xhat] to the layer's own block with xhat from m and v.  In this regime
the depthwise-bias gradient db2 (the stem's db) is a real gradient -- behind a training-mode BatchNorm it is identically
zero and only ever checked to be small -- so here it is compared like every other gradient: tol max-norm, 4 tol per channel.

(a) every yunet_dp_bwd instance: the rows of tests/test_dp_descriptor_gpu.py: BWD without the walks, same shapes, options,
    pooled and bf16-storage rows, same route assertions, one plain dense launch each;
(b) mixed regimes, one row per kernel family: frozen input with training-mode output (norm_eval: the first neck units
    read a frozen producer) and the reverse;
(c) the stem's two weight-gradient kernels; (d) pool_bwd, upadd_bwd and its coarse kernel, at the default grid and on two
    workgroups (grid-stride loops, the per-thread fp64 carry across iterations).
Bars: the existing ones (5e-5, 2e-5 under bwd_fp32mma, 4x per channel; bf16 rows: the checkers of tests/bf16_ref.py; stem
dw 1e-4; element-wise dx 2e-5, sums 5e-5).  The zero block is bit-for-bit zero after every launch (the engine shares ONE
between all frozen layers), and every gradient through a DEAD channel is exactly 0.0.  Errors are printed next to their
bars (pytest -s).  tests/test_frozen_ref.py shows on the CPU what the references are and that torch's own fp32 autograd
stays inside these bars."""
import functools

import pytest
import torch

import frozen_ref as FR
from test_dp_descriptor_gpu import BWD, Case, K, assert_route, lib, note, options, run_bwd
from test_kernels_gpu import rel_err, rel_err_ch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16

INSTANCES = [i for i in BWD if not i.startswith('walk-')]
FAMILIES = {'tile': 'tile-16x64-ragged', 'big16': 'big16-ragged', 'bwd64-8w': 'bwd64-8w-ragged', 'bwd64-4w': 'bwd64-4w',
            'bwd64-packed': 'bwd64-packed-5x10', 'bwd16s': 'bwd16s-ragged', 'head': 'head-unpacked'}
# (the heads have no BatchNorm behind them: their frozen-input launch is the one of (a), and there is no reverse)
MIXED = [(fam, rg) for fam in FAMILIES for rg in ('ft', 'tf') if fam != 'head'] + [('head', 'ff')]


def is_zero_bits(t):
    """bit-for-bit zero (-0.0 is not)"""
    return not bool(t.view(torch.int64).any())


@functools.lru_cache(maxsize=None)
def case(cid, regime='ff'):
    """a row of BWD under a regime, as the Case that test_dp_descriptor_gpu's run_bwd and assert_route take: sx / sz are
    the blocks the kernels derive their coefficients from, bst the block the unit's own BN backward reads"""
    spec = BWD[cid]
    u = FR.unit_case_of(spec, regime)
    cin, cout = u.cin, u.cout
    c = Case(id=cid, spec=spec, u=u, regime=regime, cin=cin, cout=cout, n=u.n, h=u.h, w=u.w, in_on=u.in_mode != 'none',
             out_on=u.out_mode != 'none', bf16=u.bf16, kind=spec['kind'], opts=spec.get('opts'), tol=spec.get('tol', 5e-5),
             cnt=u.count, family=('bf16 ' if u.bf16 else '') + spec['kind'] + ('' if regime == 'ff' else ' ' + regime))
    c.W = [u.unit[0].view(cout, cin).contiguous().to(DEV), u.unit[1].to(DEV), u.unit[2].view(cout, 9).contiguous().to(DEV),
           u.unit[3].to(DEV)]
    c.gi, c.bi, c.go, c.bo = u.inp.gamma.to(DEV), u.inp.beta.to(DEV), u.out.gamma.to(DEV), u.out.beta.to(DEV)
    c.x = FR.nhwc(u.x32).to(BF16 if u.bf16 else F32).to(DEV)
    c.z = (u.z if u.z.dtype == BF16 else u.z.float()).contiguous().to(DEV)
    c.dy = u.dy.float().contiguous().to(DEV)
    c.idx = u.idx.to(DEV) if u.idx is not None else None
    c.dy_scale = None if c.out_on else u.scale.to(DEV)
    c.base = torch.zeros(u.n, u.h, u.w, cin, device=DEV)
    c.sx = u.inp.stats.to(DEV) if c.in_on else None
    c.sz = u.out.stats.to(DEV) if c.out_on else None
    c.bst = u.out.bst.to(DEV).contiguous() if c.out_on else None
    return c


@functools.lru_cache(maxsize=None)
def plain(cid, regime='ff'):
    """the dense launch of the row's instance: out_bn = (frozen block | zero block), in_bn = (frozen block | the layer's
    own zeroed block) -- or the training-mode pair on a side the regime leaves training"""
    c = case(cid, regime)
    return run_bwd(c, opts={'bwd16s': 0} if c.kind == 'big16' else None)


def check(c, r):
    FR.check_unit(c.u, r, c.tol, note, c.family, FR.DB2_CH_BAR.get((c.id, c.regime)))
    FR.check_dead(c.u, r)
    if c.u.out_mode == 'frozen':
        assert is_zero_bits(c.bst), (c.id, 'the zero block handed in as out_bn.bstats was written')


# ------------------------------------------------------------------------------------------------ (a), (b)
@pytest.mark.parametrize('cid', INSTANCES)
def test_dp_bwd_frozen(cid):
    """(a) every instance with both of its BatchNorm layers frozen.
    Measured: db2 max-norm 6.6e-8 .. 6.2e-7 (bar 5e-5; 2e-5 under bwd_fp32mma); db2 per channel below 2.5e-5 of the
    channel's own value except where that value is the remainder of a cancellation: bwd64-8w (3, 16, 32) 1.94e-4 in
    channel 13 (db2 = 0.075 of sum |dz| = 1245; torch's fp32 CPU autograd: 6.1e-5), inside the 2e-4 bar, and
    tile-16x64-ragged 7.07e-4 in channel 28, where torch's fp32 autograd itself is at 6.31e-4 and the bar of that one
    case is 10x that (frozen_ref.DB2_CH_BAR)."""
    c = case(cid)
    assert c.u.moved * 1000 <= c.u.x32.numel()
    assert_route(c)
    check(c, plain(cid))


@pytest.mark.parametrize('family,regime', MIXED)
def test_dp_bwd_mixed_regimes(family, regime):
    """(b) frozen input / training-mode output ('ft') and the reverse ('tf'); db2 is compared where the output is frozen
    (and for the heads), and only small behind a training-mode layer"""
    c = case(FAMILIES[family], regime)
    assert c.u.moved * 1000 <= c.u.x32.numel()
    assert_route(c)
    bst = c.bst.clone() if c.out_on else None
    check(c, plain(c.id, regime))
    assert bst is None or torch.equal(c.bst, bst), 'the unit\'s own backward sums were written'


# ------------------------------------------------------------------------------------------------ (c) stem
@functools.lru_cache(maxsize=None)
def stem(n, h, w):
    return FR.stem_case(n, h, w)


@pytest.mark.parametrize('rz', [False, True], ids=['valu', 'rz'])
@pytest.mark.parametrize('n,h,w', [(2, 32, 32), (3, 64, 96), (1, 20, 36), (5, 66, 150)])
def test_stem_bwd_frozen(n, h, w, rz):
    """yunet_stem_bwd (VALU, reads z) and yunet_stem_bwd_rz (matrix cores, z recomputed from the image) behind a frozen
    bn1: dw at the existing 1e-4 and 4x per output channel; db -- which no test compared before -- at 10x the error of
    torch's fp32 CPU autograd of the same composition against fp64 on these inputs, floored at 1e-5 of max |db| (the
    project's 10x rule, test_forward_train_vs_oracle).  Measured: the fp32 autograd is off by 4.2e-7, 2.2e-7, 1.5e-7 and
    6.7e-7 of max |db| at the four shapes, so the floor is the bar at every one of them."""
    k = K()
    s = stem(n, h, w)
    img, z, dy = s.img.to(DEV), s.z.float().contiguous().to(DEV), s.dy.float().contiguous().to(DEV)
    zero = s.bn.bst.to(DEV)
    bn = k.BN(s.bn.stats.to(DEV), s.bn.gamma.to(DEV), s.bn.beta.to(DEV), s.count, bstats=zero)
    args = (s.wt.to(DEV).contiguous(), s.b.to(DEV)) if rz else ()
    dw, db = k.stem_bwd(img, z, dy, bn, *args)
    torch.cuda.synchronize()
    fam = 'stem rz' if rz else 'stem valu'
    assert note(fam, 'dw', rel_err(dw, s.dw), 1e-4) < 1e-4
    assert note(fam, 'dw/ch', rel_err_ch(dw, s.dw, dim=0), 4e-4) < 4e-4
    dbm = float(s.db.abs().max())
    bar = max(10 * s.err32[1] / dbm, 1e-5)
    note(fam, 'db fp32 cpu', s.err32[1] / dbm, bar)
    assert note(fam, 'db', rel_err(db, s.db), bar) < bar
    assert is_zero_bits(zero), 'the zero block was written'
    assert float(db[FR.DEAD]) == 0.0 and float(dw[FR.DEAD].abs().max()) == 0.0, 'dead channel'
    assert float(db[FR.ZERO]) == 0.0 and float(dw[FR.ZERO].abs().max()) == 0.0, 'gamma = 0'


# ------------------------------------------------------------------------------------------------ (d) element-wise
@functools.lru_cache(maxsize=None)
def ew(c):
    e = FR.ew_case(c)
    e.d = {name: getattr(e, name).float().contiguous().to(DEV) for name in ('za', 'zb', 'r_p', 'r_e')}
    return e


def ew_bn(e, which):
    """a frozen layer as the element-wise kernels take it: the synthesised block, the layer's own zeroed sums"""
    p, z = (e.a, e.za) if which == 'a' else (e.b, e.zb)
    return K().BN(p.stats.to(DEV), p.gamma.to(DEV), p.beta.to(DEV), z.numel() // e.c,
                  bstats=torch.zeros(2 * e.c, dtype=F64, device=DEV))


def check_ew(fam, name, dx, bn, ref_dx, ref_sums, c):
    assert note(fam, name + ' dx', rel_err(dx, ref_dx), 2e-5) < 2e-5
    assert note(fam, name + ' sums', rel_err(bn.bstats, ref_sums), 5e-5) < 5e-5
    assert not bool(dx[..., FR.DEAD].any()), 'dead channel'
    assert float(bn.bstats[FR.DEAD]) == 0.0 == float(bn.bstats[c + FR.DEAD]), 'dead channel: sums'


@pytest.fixture(params=[0, 2], ids=['default-grid', 'two-workgroups'])
def grid(request):
    """option ew_grid: 0 = the default cap (one pass at these sizes), 2 = every thread walks its grid-stride loop"""
    L = lib()
    prev = L.set_option('ew_grid', request.param)
    try:
        yield request.param
    finally:
        L.set_option('ew_grid', prev)


@pytest.mark.parametrize('c', [16, 32, 64])
def test_pool_bwd_frozen(c, grid):
    """pool_bwd behind a frozen layer: alone, with a second full-size consumer (`extra`), and accumulating (base + the
    plain dx, bit for bit).  gamma = 0, beta > 0 makes every window of that channel a four-way tie: position 0 wins, as
    in F.max_pool2d."""
    k, e = K(), ew(c)
    fam = f'pool {c} grid {grid}'
    d = e.d
    bn = ew_bn(e, 'a')
    dx = k.pool_bwd(d['za'], bn, d['r_p'])
    torch.cuda.synchronize()
    check_ew(fam, 'plain', dx, bn, *e.pool, c)
    assert torch.equal(dx[:, 0::2, 0::2, FR.ZERO], d['r_p'][..., FR.ZERO]), 'a tie does not go to position 0'
    assert not bool(dx[:, 1::2, :, FR.ZERO].any()) and not bool(dx[:, :, 1::2, FR.ZERO].any())
    bn_e = ew_bn(e, 'a')
    dx_e = torch.full(d['za'].shape, float('nan'), device=DEV)
    k.pool_bwd(d['za'], bn_e, d['r_p'], dx=dx_e, extra=d['r_e'])
    torch.cuda.synchronize()
    check_ew(fam, 'extra', dx_e, bn_e, *e.pool_extra, c)
    bn_a = ew_bn(e, 'a')
    base = torch.randn(d['za'].shape, device=DEV) * 100
    dx_a = base.clone()
    k.pool_bwd(d['za'], bn_a, d['r_p'], dx=dx_a, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(dx_a, base + dx), 'accumulate: not base + dx bit for bit'
    assert rel_err(bn_a.bstats, bn.bstats) < 1e-12


@pytest.mark.parametrize('c', [16, 32, 64])
def test_upadd_bwd_frozen(c, grid):
    """upadd_bwd (the general kernel) and upadd_bwd(skip_a=True) (the coarse kernel) behind two frozen layers: each
    layer's sums go to its own block, with xhat from its frozen statistics"""
    k, e = K(), ew(c)
    fam = f'upadd {c} grid {grid}'
    d = e.d
    bna, bnb = ew_bn(e, 'a'), ew_bn(e, 'b')
    dxa, dxb = k.upadd_bwd(d['za'], bna, d['zb'], bnb, d['r_e'])
    torch.cuda.synchronize()
    check_ew(fam, 'fine', dxa, bna, e.upadd[0], e.upadd[1], c)
    check_ew(fam, 'coarse', dxb, bnb, e.upadd[2], e.upadd[3], c)
    bna2, bnb2 = ew_bn(e, 'a'), ew_bn(e, 'b')
    none_a, dxb2 = k.upadd_bwd(d['za'], bna2, d['zb'], bnb2, d['r_e'], skip_a=True)
    torch.cuda.synchronize()
    assert none_a is None and is_zero_bits(bna2.bstats), 'skip_a: the fine layer\'s sums were written'
    check_ew(fam, 'skip_a', dxb2, bnb2, e.upadd[2], e.upadd[3], c)
