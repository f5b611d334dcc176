"""No GPU: tests/train_walk.py rejects what it exists to catch, and its GPU cases reach the benchmark's kernel instances.

The record here is the training step of the trained YuNet_n fixture in torch fp32 on the CPU, composed op by op the way
the engine composes it (fused pooling on the sole-consumer pools, one of them with its full-size z elided; the taps'
gradients written once by the pool's backward; per-image weight-gradient partials and their reduction; the BatchNorm
table ops).  Its parameter gradients are first compared with autograd through the oracle's train-mode conv stack
(finetune_ref.step_fp32), so the composition is the oracle's.  walk() passes on it; each injected wiring defect makes it
fail at the node named next to it.  The batch (2 x 64 x 64, seed SEED) keeps every tensor's ambiguous elements at or
under one in 1000 on this yardstick (asserted by the walk itself)."""
import os

import pytest
import torch
import torch.nn.functional as F

import bf16_ref as R
import finetune_ref as FR
import train_walk as TW
import yunet_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SEED, N, H, W = 31, 2, 64, 64
F64 = torch.float64


def trained(kind):
    return torch.load(os.path.join(GOLDEN, f'yunet_{kind}_synth_trained.pth'), map_location='cpu', weights_only=False)['state_dict']


def unit_w(sd, name):
    return [t.float() for t in TW.E.unit_weights(sd, name)]


def head_w(sd, level):
    return [t.float() for t in TW.E.head_weights(sd, level)]


class Step:
    """the engine's composition in torch fp32; `defect` = (kind, where) changes one wiring decision"""

    def __init__(self, kind, sd, batch, defect=(None, None)):
        import yunet_amd.synthetic  # noqa: F401
        self.arch, self.sd, self.defect = O.yunet_arch(kind), sd, defect
        self.rec = TW.Record('fp32', batch['img'], momentum=0.11 if defect[0] == 'momentum' else 0.1)
        self.batch = batch
        self.written, self.bwd, self.share = set(), [], {}
        for k in sd:
            if k.endswith('.running_mean'):
                p = k[:-len('.running_mean')]
                c = sd[k].numel()
                self.rec.layer(p, c=c, stats=torch.zeros(1, 2 * c, dtype=F64), bstats=torch.zeros(1, 2 * c, dtype=F64), slots=1,
                               gamma=sd[p + '.weight'].float(), beta=sd[p + '.bias'].float(), frozen=False,
                               rm0=sd[k].float(), rv0=sd[p + '.running_var'].float(), nbt0=int(sd[p + '.num_batches_tracked']),
                               rm1=None, rv1=None, nbt1=None, dgamma=None, dbeta=None)
        self.count = {}
        self.forward()
        self.loss()
        for fn in reversed(self.bwd):
            fn()
        self.tables()

    def hit(self, kind, where):
        return self.defect == (kind, where)

    # ---- forward
    def coef(self, layer, count=None):
        b = self.rec.bn[layer]
        return TW.bn_coef(b.stats[0], count or self.count[layer], b.gamma, b.beta, torch.float32)

    def forward(self):
        rec, sd, arch = self.rec, self.sd, self.arch
        w0 = (sd['backbone.model0.conv1.weight'].float().reshape(16, 27), sd['backbone.model0.conv1.bias'].float())
        z0 = F.conv2d(rec.img, w0[0].view(16, 3, 3, 3), w0[1], stride=2, padding=1).permute(0, 2, 3, 1).contiguous()
        t0 = rec.tensor('stem', z0, z0.shape, bn='backbone.model0.bn1')
        self.produced('backbone.model0.bn1', z0)
        nd0 = rec.node('stem', 'stem', z='stem', w=w0, out_bn='backbone.model0.bn1', bwd=True, g=None, partials=None, rows=0)
        self.bwd.append(lambda: self.stem_bwd(nd0, t0))
        cur = self.unit('stem', 'backbone.model0.conv2', pool=True)
        taps = []
        for i in range(len(arch['stage_channels'])):
            if i > 0:
                cur = self.unit(cur, f'backbone.model{i}.conv1')
                fused = i in arch['downsample_idx'] and i not in arch['out_idx']
                cur = self.unit(cur, f'backbone.model{i}.conv2', pool=fused, elide=fused)
            if i in arch['out_idx']:
                taps.append(cur)
                if i in arch['downsample_idx']:
                    cur = self.pool(cur)
        feats = list(taps)
        for i in range(len(feats) - 1, 0, -1):
            feats[i] = self.unit(feats[i], f'neck.lateral_convs.{i}')
            feats[i - 1] = self.upadd(feats[i - 1], feats[i])
        feats[0] = self.unit(feats[0], 'neck.lateral_convs.0')
        n = rec.img.shape[0]
        sizes = [(rec.tensors[f].h, rec.tensors[f].w) for f in feats]
        self.sizes, self.P = sizes, sum(a * b for a, b in sizes)
        rec.flat = torch.zeros(n, self.P, 16)
        for l, f in enumerate(feats):
            for j in range(arch['shared_stacked_convs']):
                f = self.unit(f, f'bbox_head.multi_level_share_convs.{l}.{j}')
            self.unit(f, f'head.{l}', head=l)

    def produced(self, layer, z):
        self.rec.bn[layer].stats[0] = R.stats_of(z)
        self.count[layer] = z.shape[0] * z.shape[1] * z.shape[2]

    def unit(self, xname, name, pool=False, elide=False, head=None):
        rec, sd = self.rec, self.sd
        x = rec.tensors[xname]
        w = head_w(sd, head) if head is not None else unit_w(sd, name)
        cnt = self.count.get(x.bn)
        if self.hit('bn_count', name):
            cnt -= x.w                                          # short by one image row
        in_bn = self.coef(x.bn, cnt) if x.bn else None
        z = TW.t_unit_fwd(x.buf, w, in_bn, torch.float32)
        out_bn = None if head is not None else name + '.bn'
        nd = rec.node('unit', name, x=xname, z=None if head is not None else name, w=w, out_bn=out_bn, pool_out=None,
                      pool_idx=None, flat_rows=None, dy=None, dy_scale=None, accumulate=0, zmode='stored', bwd=True,
                      g=None, partials=None, rows=0)
        ret = name
        if head is not None:
            base = sum(a * b for a, b in self.sizes[:head])
            rec.flat[:, base:base + x.h * x.w] = z.reshape(x.n, -1, 16)
            nd.flat_rows, nd.base = z, base
        else:
            zt = rec.tensor(name, z, z.shape, bn=out_bn)
            self.produced(out_bn, z)
            if pool:
                key = R.windows(z) * torch.sign(rec.bn[out_bn].gamma).view(1, 1, 1, -1, 1)
                idx = 3 - key.flip(-1).argmax(-1) if self.hit('last_max', name) else key.argmax(-1)
                win = R.windows(z).gather(-1, idx.unsqueeze(-1)).squeeze(-1)
                ret = f'pool({name})'
                rec.tensor(ret, win, win.shape, bn=out_bn)
                nd.pool_out, nd.pool_idx = ret, idx.to(torch.uint8)
                if elide:
                    zt.buf, nd.zmode = None, 'elided'
        self.bwd.append(lambda: self.unit_bwd(nd, x, w, z, in_bn))
        return ret

    def pool(self, xname):
        rec = self.rec
        x = rec.tensors[xname]
        a = TW.t_act(x.buf, self.coef(x.bn))[0]
        out = R.windows(a).amax(-1)
        name = f'pool({xname})'
        rec.tensor(name, out, out.shape)
        nd = rec.node('pool', f'pool {xname}', x=xname, out=name, extra=None, bwd=True)
        self.bwd.append(lambda: self.pool_bwd(nd, x))
        return name

    def upadd(self, aname, bname):
        rec = self.rec
        a, b = rec.tensors[aname], rec.tensors[bname]
        out = TW.t_act(a.buf, self.coef(a.bn))[0] + TW.up2(TW.t_act(b.buf, self.coef(b.bn))[0])
        name = f'upadd({aname})'
        rec.tensor(name, out, out.shape)
        nd = rec.node('upadd', f'upadd -> {name}', a=aname, b=bname, out=name, skip_a=True, bwd=True)
        self.bwd.append(lambda: self.upadd_bwd(nd, a, b))
        return name

    def loss(self):
        rec, b = self.rec, self.batch
        flat = rec.flat.clone().requires_grad_(True)
        losses, _ = O.loss_step(flat, b['gt_bboxes'], b['gt_labels'], b['gt_keypointss'], self.sizes, self.arch)
        sum(losses.values()).backward()
        rec.dflat = flat.grad
        self.dy_scale = torch.ones(16)

    # ---- backward
    def write(self, tname, dx, who):
        t = self.rec.tensors[tname]
        acc = tname in self.written and not self.hit('accumulate', who)
        t.grad = t.grad + dx if acc else dx.clone()
        self.written.add(tname)
        return int(acc)

    def add_sums(self, layer, s):
        self.rec.bn[layer].bstats[0] += s

    def reduce(self, nd, rows, widths):
        nd.partials, nd.rows = rows, rows.shape[0]
        total = (rows[:-1] if self.hit('reduce', nd.name) else rows).sum(0)
        nd.g = list(torch.split(total, widths))

    def unit_bwd(self, nd, x, w, z, in_bn):
        rec = self.rec
        cout, cin = w[0].shape
        if nd.out_bn is None:
            hw = x.h * x.w
            dy = rec.dflat[:, nd.base:nd.base + hw].reshape(x.n, x.h, x.w, 16)
            nd.dy, nd.dy_scale = ('dflat', dy), self.dy_scale
            scale = self.dy_scale.clone()
            if self.hit('dy_scale', nd.name):
                scale[3] *= 1.001
            out_bn = bst = None
        else:
            src = nd.pool_out or nd.name
            nd.dy = ('grad', src)
            dy = rec.tensors[src].grad
            if nd.pool_out:
                dy = R.expand_pooled(dy, nd.pool_idx).float()
            layer = nd.out_bn
            if self.hit('bstats', nd.name):
                names = [k for k, b in rec.bn.items() if b.c == cout]
                layer = names[names.index(nd.out_bn) + 1]
            out_bn, bst, scale = self.coef(nd.out_bn), rec.bn[layer].bstats[0].clone(), None
        dx, rows, in_sums = TW.t_unit_bwd(x.buf, w, z, dy, in_bn, out_bn, bst, scale, torch.float32,
                                          bf16_operand=self.hit('bf16_operand', nd.name))
        nd.accumulate = self.write(nd.x, dx, nd.name)
        if in_sums is not None:
            self.add_sums(x.bn, in_sums)
        self.reduce(nd, rows, [cout * cin, cout, cout * 9, cout])

    def pool_bwd(self, nd, x):
        rec = self.rec
        coef = self.coef(x.bn)
        dx = TW.t_pool_bwd(x.buf, coef, rec.tensors[nd.out].grad, torch.float32)
        _, xh, mask = TW.t_act(x.buf, coef)
        share = self.share.pop(x.name)
        nd.extra = share[0]
        if not self.hit('extra', nd.name):
            dx = dx + share[1] * mask
        self.write(x.name, dx, nd.name)
        self.add_sums(x.bn, TW.t_sums(dx, xh))

    def upadd_bwd(self, nd, a, b):
        rec = self.rec
        g = rec.tensors[nd.out].grad
        if a.name in [n.x for n in rec.nodes if n.kind == 'pool']:
            self.share[a.name] = (nd.out, g)                    # left to the tap's pool backward
        else:
            nd.skip_a = False
            _, xh, mask = TW.t_act(a.buf, self.coef(a.bn))
            self.write(a.name, g * mask, nd.name)
            self.add_sums(a.bn, TW.t_sums(g * mask, xh))
        _, xh, mask = TW.t_act(b.buf, self.coef(b.bn))
        db = TW.down2(g) * mask
        self.write(b.name, db, nd.name)
        self.add_sums(b.bn, TW.t_sums(db, xh))

    def stem_bwd(self, nd, t0):
        b = self.rec.bn[nd.out_bn]
        rows = TW.t_stem_bwd(self.rec.img, nd.w[0], nd.w[1], t0.grad, self.coef(nd.out_bn), b.bstats[0], torch.float32)
        self.reduce(nd, rows, [432, 16])

    def tables(self):
        rec = self.rec
        names = list(rec.bn)
        for i, name in enumerate(names):
            b = rec.bn[name]
            src = b
            if self.hit('bn_grad', name):
                same = [k for k in names if rec.bn[k].c == b.c]
                src = rec.bn[same[same.index(name) + 1]]
            b.dbeta, b.dgamma = src.bstats[0, :b.c].float(), src.bstats[0, b.c:].float()
            b.rm1, b.rv1 = TW.running_update(b.stats[0], self.count[name], b.rm0, b.rv0, rec.momentum)
            b.nbt1 = b.nbt0 + 1
        rec.momentum = 0.1
        rec.node('bn_run', 'bn_run', layers=names)
        rec.node('bn_grad', 'bn_grad', layers=names)

    def grads(self):
        """state_dict key -> gradient, for the comparison with the oracle's autograd"""
        out = {}
        for nd in self.rec.nodes:
            if nd.kind == 'stem':
                out['backbone.model0.conv1.weight'], out['backbone.model0.conv1.bias'] = nd.g[0].view(16, 3, 3, 3), nd.g[1]
            elif nd.kind == 'unit' and nd.out_bn:
                for k, g in zip(('conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias'), nd.g):
                    out[f'{nd.name}.{k}'] = g
            elif nd.kind == 'unit':
                lvl, r0 = nd.name.split('.')[1], 0
                for part, nr in TW.E.HEAD_PARTS:
                    for k, g, per in zip(('conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias'), nd.g, (64, 1, 9, 1)):
                        out[f'bbox_head.multi_level_{part}.{lvl}.{k}'] = g.reshape(16, per)[r0:r0 + nr]
                    r0 += nr
        for name, b in self.rec.bn.items():
            out[name + '.weight'], out[name + '.bias'] = b.dgamma, b.dbeta
        return out


@pytest.fixture(scope='module')
def setup():
    import yunet_amd.synthetic as S
    return trained('n'), S.make_batch(N, H, W, SEED)


def test_clean_record_walks_clean_and_is_the_oracles_step(setup):
    sd, batch = setup
    st = Step('n', sd, batch)
    _, g32, aux, after = FR.step_fp32(batch, sd, st.arch, lambda name: True)
    assert FR.near_tie(aux, batch) == []
    got = st.grads()
    assert set(got) == set(g32)
    scale = max(float(v.abs().max()) for v in g32.values())
    for k, g in g32.items():
        err = float((got[k].reshape(g.shape) - g).abs().max())
        assert err <= 1e-2 * float(g.abs().max()) + 1e-5 * scale, (k, err, float(g.abs().max()))
    for name, b in st.rec.bn.items():
        assert torch.allclose(b.rm1, after[name + '.running_mean'], rtol=1e-4, atol=1e-6), name
        assert torch.allclose(b.rv1, after[name + '.running_var'], rtol=1e-4, atol=1e-6), name
    worst = TW.walk(st.rec, tag='cpu fp32')
    assert max(worst.values()) <= 1.0
    kinds = [nd.kind for nd in st.rec.nodes]
    assert kinds.count('unit') == 20 and kinds.count('pool') == 2 and kinds.count('upadd') == 2
    assert sum(nd.zmode == 'elided' for nd in st.rec.nodes if nd.kind == 'unit') == 1
    assert all(n * TW.AMB_CAP <= tot for n, tot in st.rec.amb.values())


# defect -> (where it is injected, the node that must fail)
DEFECTS = {
    'reduce': ('backbone.model3.conv1', 'reduce backbone.model3.conv1'),
    'bn_count': ('backbone.model1.conv1', 'backbone.model1.conv1'),           # reads the pooled model0.conv2 output
    'extra': ('pool backbone.model4.conv2', 'grad backbone.model4.conv2'),
    'accumulate': ('upadd -> upadd(backbone.model3.conv2)', 'grad neck.lateral_convs.1'),   # second writer after share_convs.1.0
    'dy_scale': ('head.1', 'head.1'),
    'bstats': ('backbone.model3.conv2', 'backbone.model3.conv2'),
    'bn_grad': ('neck.lateral_convs.1.bn', 'bn_grad'),
    'momentum': (None, 'bn_run'),
    'bf16_operand': ('backbone.model5.conv1', 'backbone.model5.conv1'),
    'last_max': ('backbone.model0.conv2', 'backbone.model0.conv2'),
}


@pytest.mark.parametrize('kind', sorted(DEFECTS))
def test_injected_defect_fails_at_its_node(setup, kind):
    sd, batch = setup
    where, node = DEFECTS[kind]
    if kind == 'last_max':      # the two rules differ on ties only: gamma = 0 makes every window of a channel a four-way tie
        sd = dict(sd)
        sd[where + '.bn.weight'] = sd[where + '.bn.weight'].clone()
        sd[where + '.bn.weight'][4] = 0.0
        TW.walk(Step('n', sd, batch).rec, tag='gamma = 0', quiet=True)
    st = Step('n', sd, batch, defect=(kind, where))
    with pytest.raises(TW.WalkError) as e:
        TW.walk(st.rec, tag=kind, quiet=True)
    print(kind, '->', e.value.nodes)
    assert node in e.value.nodes, (kind, e.value.nodes)


@pytest.mark.parametrize('case', sorted(TW.CASES))
def test_case_geometry_selects_the_benchmarks_kernel_instances(case):
    """Every GPU case's plan at TW.GEOMETRY routes (yunet_dp_route over its forward and backward unit descriptors) to the
    same set of kernel instances as the plan of the same options at the benchmark shape."""
    import yunet_amd.engine as EN
    c = TW.CASES[case]
    prev = os.environ.get('YUNET_KEEP_POOL_Z')
    if c['keep_pool_z']:
        os.environ['YUNET_KEEP_POOL_Z'] = '1'
    try:
        sets, elided = [], []
        for shape in (TW.GEOMETRY, TW.BENCH[c['kind']]):
            eng = EN.YuNetEngine(O.yunet_arch(c['kind']), 'cpu')
            eng.set_precision(c['precision'])
            eng.set_deterministic(c['deterministic'])
            if c['finetune']:
                eng.set_frozen(*TW.finetune_signature(eng.layout))
            plan = EN.Plan(eng, *shape, 64)
            sets.append(TW.plan_routes(plan))
            elided.append(len(plan.elided_z))
    finally:
        if prev is None:
            os.environ.pop('YUNET_KEEP_POOL_Z', None)
        else:
            os.environ['YUNET_KEEP_POOL_Z'] = prev
    assert sets[0] == sets[1], (sorted(sets[1] - sets[0]), sorted(sets[0] - sets[1]))
    assert len(sets[0]) >= 10
    # the z elision as at the benchmark shape: one tensor by default, none where the backward reads z (deterministic=True),
    # where the pooled unit has no backward (the frozen prefix) or under the switch
    assert elided[0] == elided[1] == (1 if case in ('n_fp32', 's_fp32', 'n_bf16', 'n_det_fast') else 0), elided
