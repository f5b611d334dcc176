"""No GPU: the plan builder drops the full-size output of a fused-pool unit exactly where nothing reads it
(Plan._elide_pool_z), the dispatchers' answer to a null YunetDP.z (include/yunet_hip.h), and the op-list dump with and
without the elision.  Plans are built on the CPU device, as tools/dbg/plan_dump.py builds them."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import pytest
import torch

import yunet_amd._lib as L
import yunet_amd.engine as E
import yunet_amd.kernels as K
import yunet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = 'backbone.model0.conv2'          # the 16 -> 16 unit between the stem and the first max_pool2d


def plan_of(kind='n', shape=(4, 128, 128, 64), precision='fp32', det=False):
    eng = E.YuNetEngine(O.yunet_arch(kind), 'cpu')
    eng.set_precision(precision)
    eng.set_deterministic(det)
    return eng, E.Plan(eng, *shape)


def unit_ops(plan):
    """(forward record, backward record) of UNIT, from the arrays the executor runs"""
    f = [op for op in plan.c_fwd_a if op.opcode == L.OP_DP_FWD and op.dp.pool_out]
    b = [op for op in plan.c_bwd if op.opcode == L.OP_DP_BWD and op.dp.pool_idx]
    return f, b


def full_size_buffers(plan, numel):
    return sum(1 for x, z in plan.tensors.values() if z.buf is not None and z.buf.numel() == numel)


@pytest.mark.parametrize('kind', ['n', 's'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_elided_where_nobody_reads_it(kind, precision, monkeypatch):
    """N = 4 at 128 x 128: the stem's map is 64 x 64, the smallest that puts UNIT on dp_fwd16s / dp_bwd16s.  Without the
    switch both records of UNIT carry a null z and the plan holds one buffer of that size fewer; every other unit keeps
    its output (YuNet_s: also the pooled 32 -> 64 unit, whose tile backward reads z)."""
    monkeypatch.delenv('YUNET_KEEP_POOL_Z', raising=False)
    _, plan = plan_of(kind, precision=precision)
    monkeypatch.setenv('YUNET_KEEP_POOL_Z', '1')
    _, kept = plan_of(kind, precision=precision)
    assert plan.sw['keep_pool_z'] is False and kept.sw['keep_pool_z'] is True
    numel = 4 * 64 * 64 * 16
    assert [plan.tensors[UNIT][1]] == [zt for zt, _ in plan.elided_z] and kept.elided_z == []
    assert plan.tensors[UNIT][1].buf is None and kept.tensors[UNIT][1].buf.numel() == numel
    assert full_size_buffers(kept, numel) - full_size_buffers(plan, numel) == 1
    for p, null in ((plan, True), (kept, False)):
        f, b = unit_ops(p)
        assert len(f) == len(b) >= 1
        for op in f + b:
            is_unit = (op.dp.cin, op.dp.cout) == (16, 16)
            assert (op.dp.z is None) == (null and is_unit), (op.dp.cin, op.dp.cout)
        assert sum((op.dp.cin, op.dp.cout) == (16, 16) for op in f) == 1
        # nobody else lost its output
        others = [op for lst in (p.c_fwd_a, p.c_bwd, p.c_bwd_a, p.c_bwd_b, p.c_bwd_a_k) for op in lst
                  if op.opcode in (L.OP_DP_FWD, L.OP_DP_BWD) and not (op.dp.pool_out or op.dp.pool_idx)]
        assert others and all(op.dp.z for op in others)
    # the two-segment copies of the backward carry the same descriptor
    assert [op.dp.z for op in plan.c_bwd_b if op.opcode == L.OP_DP_BWD and op.dp.pool_idx and op.dp.cin == 16] == [None]


def test_keep_switch_spelled_zero_elides(monkeypatch):
    monkeypatch.setenv('YUNET_KEEP_POOL_Z', '0')          # the A/B recipe names both sides
    _, plan = plan_of()
    assert len(plan.elided_z) == 1


def test_kept_where_the_backward_reads_it(monkeypatch):
    """(b) of the rule, answered by the dispatcher's own predicate: the tile backward (option bwd16s = 0), the
    deterministic mode (tile kernels in both directions) and maps below the streaming kernels' minimum keep z."""
    monkeypatch.delenv('YUNET_KEEP_POOL_Z', raising=False)
    prev = L.set_option('bwd16s', 0)
    try:
        _, plan = plan_of()
        f, b = unit_ops(plan)
        assert plan.elided_z == [] and f[0].dp.z and b[0].dp.z and plan.tensors[UNIT][1].buf is not None
    finally:
        L.set_option('bwd16s', prev)
    _, plan = plan_of(det=True)
    f, b = unit_ops(plan)
    assert plan.elided_z == [] and f[0].dp.z and b[0].dp.z
    _, plan = plan_of(shape=(2, 64, 64, 64))               # 32 x 32 map: no fused pooling of the 16 -> 16 unit at all
    assert plan.elided_z == [] and all(op.dp.z for op in plan.c_fwd_a if op.opcode == L.OP_DP_FWD)


def test_kept_under_the_environment_option():
    """YUNET_BWD16S=0 is read once per process: a fresh one"""
    code = ('import sys; sys.path[:0] = [%r, %r]\n'
            'import yunet_oracle as O, yunet_amd.engine as E, yunet_amd._lib as L\n'
            'p = E.Plan(E.YuNetEngine(O.yunet_arch("n"), "cpu"), 4, 128, 128, 64)\n'
            'f = [op for op in p.c_fwd_a if op.opcode == L.OP_DP_FWD and op.dp.pool_out]\n'
            'print("Z", len(p.elided_z), bool(f[0].dp.z))\n') % (ROOT, os.path.join(ROOT, 'oracle'))
    env = {k: v for k, v in os.environ.items() if k != 'YUNET_KEEP_POOL_Z'}
    out = subprocess.check_output([sys.executable, '-c', code], env=dict(env, YUNET_BWD16S='0'), text=True)
    assert 'Z 0 True' in out, out


def test_eval_forward_gets_its_buffer_on_first_use(monkeypatch):
    """forward_eval leaves every tensor of Plan.tensors readable: eval_ops() allocates the dropped one and points the
    eval list at it; the training lists stay without."""
    monkeypatch.delenv('YUNET_KEEP_POOL_Z', raising=False)
    _, plan = plan_of()
    ev = [op for op in plan.c_fwd_eval if op.opcode == L.OP_DP_FWD and op.dp.pool_out]
    assert ev[0].dp.z is None and plan.tensors[UNIT][1].buf is None
    arr = plan.eval_ops()
    zt = plan.tensors[UNIT][1]
    assert arr is plan.c_fwd_eval and zt.buf.shape == (4, 64, 64, 16)
    ev = [(k, op) for k, op in enumerate(plan.c_fwd_eval) if op.opcode == L.OP_DP_FWD and op.dp.pool_out]
    assert ev[0][1].dp.z == zt.buf.data_ptr() == plan.fwd_eval[ev[0][0]].dp.z
    assert plan.eval_ops() is arr and plan.tensors[UNIT][1].buf is zt.buf
    assert unit_ops(plan)[0][0].dp.z is None


def _unit_desc(cin, cout, n, h, w, keep):
    x = torch.zeros(n, h, w, cin)
    ws = [torch.zeros(cout, cin), torch.zeros(cout), torch.zeros(cout, 9), torch.zeros(cout)]
    z = torch.zeros(n, h, w, cout)
    st = [torch.zeros(2 * c, dtype=torch.float64) for c in (cin, cin, cout, cout)]
    in_bn = K.BN(st[0], torch.ones(cin), torch.zeros(cin), n * h * w, bstats=st[1])
    out_bn = K.BN(st[2], torch.ones(cout), torch.zeros(cout), n * h * w, bstats=st[3])
    d = K._dp_desc(x, *ws, z, in_bn, out_bn)
    keep += [x, z, in_bn, out_bn] + ws
    return d


def test_query_follows_the_backward_dispatch():
    keep = []

    def bwd_desc(cin, cout, h, w, **kw):
        d = _unit_desc(cin, cout, 2, h, w, keep)
        dx = torch.zeros(2, h, w, cin)
        keep.append(dx)
        d.dx = dx.data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    q = L.load().yunet_dp_bwd_reads_z
    assert q(C.byref(bwd_desc(16, 16, 32, 64))) == 0
    assert q(C.byref(bwd_desc(16, 16, 34, 70))) == 0
    assert q(C.byref(bwd_desc(16, 16, 32, 62))) == 1                   # below the streaming kernel's minimum map
    assert q(C.byref(bwd_desc(16, 16, 30, 64))) == 1
    assert q(C.byref(bwd_desc(16, 16, 32, 64, accumulate_dx=1))) == 1
    assert q(C.byref(bwd_desc(16, 16, 32, 64, dx=None))) == 1
    assert q(C.byref(bwd_desc(16, 16, 32, 64, out_has_bn=0))) == 1
    assert q(C.byref(bwd_desc(64, 64, 32, 64))) == 1
    assert q(C.byref(bwd_desc(16, 64, 32, 64))) == 1
    d = bwd_desc(16, 16, 32, 64)
    d.in_bn.det_rows = 1024                                            # deterministic sums: the tile kernel
    assert q(C.byref(d)) == 1
    prev = L.set_option('bwd16s', 0)
    try:
        assert q(C.byref(bwd_desc(16, 16, 32, 64))) == 1
    finally:
        L.set_option('bwd16s', prev)
    assert q(None) == 1


@pytest.mark.parametrize('suffix', ['', '_bf16'])
def test_null_z_is_rejected_before_any_launch(suffix):
    """Host-side only (this test runs without a device): a unit without pool_out, the 64 -> 64 unit with pool_out, the
    deterministic form, the grouped entry and every backward that reads z return YUNET_EINVAL for a null z."""
    lib, keep = L.load(), []
    act = L.BF16 if suffix else L.F32
    fwd, bwd, grp = (getattr(lib, n + suffix) for n in ('yunet_dp_fwd', 'yunet_dp_bwd', 'yunet_dp_fwd_group'))

    def desc(cin, cout, h, w, pool):
        d = _unit_desc(cin, cout, 2, h, w, keep)
        d.x_dtype = d.z_dtype = act
        if pool:
            po, pi = torch.zeros(2, h // 2, w // 2, cout), torch.zeros(2, h // 2, w // 2, cout, dtype=torch.uint8)
            keep.extend([po, pi])
            d.pool_out, d.pool_idx = po.data_ptr(), pi.data_ptr()
        d.z = None
        return d
    for cin, cout, h, w, pool in ((16, 16, 32, 64, False), (16, 64, 32, 64, False), (64, 64, 32, 64, False),
                                  (64, 64, 32, 64, True), (32, 64, 32, 64, True), (16, 16, 16, 16, False),
                                  (64, 64, 10, 10, False)):
        assert fwd(C.byref(desc(cin, cout, h, w, pool)), None) == L.EINVAL, (cin, cout, h, w, pool)
    d = desc(16, 16, 32, 64, True)
    d.out_bn.det_rows = 1024
    assert fwd(C.byref(d), None) == L.EINVAL
    prev = L.set_option('fwd16s', 0)                     # the pooled 16 -> 16 unit on the tile kernel stores z
    try:
        assert fwd(C.byref(desc(16, 16, 32, 64, True)), None) == L.EINVAL
    finally:
        L.set_option('fwd16s', prev)
    units = [desc(64, 64, 20, 20, False), desc(64, 64, 20, 20, False)]
    arr = (C.POINTER(L.YunetDP) * 2)(C.pointer(units[0]), C.pointer(units[1]))
    assert grp(arr, 2, None) == L.EINVAL
    # backward: null z only where the selected kernel recomputes it
    for cin, cout, h, w in ((64, 64, 32, 64), (16, 64, 32, 64), (16, 16, 16, 32)):
        d = desc(cin, cout, h, w, False)
        blocks = K.dp_grid(2, h, w, cin, cout)
        part, dx = torch.zeros(blocks, K.dp_row_width(cin, cout)), torch.zeros(2, h, w, cin)
        keep.extend([part, dx])
        d.wgrad_partials, d.wgrad_blocks, d.dx, d.dy = part.data_ptr(), blocks, dx.data_ptr(), dx.data_ptr()
        assert lib.yunet_dp_bwd_reads_z(C.byref(d)) == 1
        assert bwd(C.byref(d), None) == L.EINVAL, (cin, cout, h, w)


def _plan_dump():
    spec = importlib.util.spec_from_file_location('plan_dump', os.path.join(ROOT, 'tools', 'dbg', 'plan_dump.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_differs_in_the_units_z_alone(tmp_path, monkeypatch):
    """tools/dbg/plan_dump.py with YUNET_KEEP_POOL_Z=1 (its default: the form tests/golden/plan_dump_default.sha256
    records, checked by tests/test_deterministic.py) against --elide, over both nets, both storage types, one and two
    ranks, every plan switch: same ops, same order, every field equal except `dp.z` of the records of a 16 -> 16 unit
    with fused pooling, null in one and the unit's own buffer in the other.  A pointer into the dropped buffer anywhere
    else would fail the dump itself (`lies in no known buffer`)."""
    monkeypatch.setenv('YUNET_KEEP_POOL_Z', '1')          # (main() sets it: restored after the test)
    pd = _plan_dump()
    pd.SHAPES = ((4, 128, 128, 64), (2, 160, 224, 128), (1, 32, 32, 64))
    pd.ARCHS = pd.ARCHS[:2]
    a, b = tmp_path / 'keep.txt', tmp_path / 'elide.txt'
    pd.main(str(a))
    pd.main(str(b), elide=True)
    la, lb = a.read_text().splitlines(), b.read_text().splitlines()
    assert len(la) == len(lb)
    changed = 0
    for x, y in zip(la, lb):
        if x == y:
            continue
        tx, ty = x.split(), y.split()
        assert len(tx) == len(ty)
        diff = [(p, q) for p, q in zip(tx, ty) if p != q]
        assert len(diff) == 1 and diff[0][1] == 'dp.z=None' and diff[0][0].startswith(f'dp.z={UNIT}.z+0'), diff
        assert 'dp.cin=16' in tx and 'dp.cout=16' in tx and ('dp.pool_out=None' not in tx or 'dp.pool_idx=None' not in tx)
        changed += 1
    assert changed > 0
    # maps below the streaming kernels' minimum (1 x 32 x 32) and the no-fusion switch: nothing differs
    head = None
    for x, y in zip(la, lb):
        if x.startswith('== '):
            head = x
        elif x != y:
            assert 'YUNET_NO_POOL_FUSION' not in head and '(1, 32, 32, 64)' not in head, head
