"""No GPU: yunet_dp_route (csrc/dp_route.h, the rule behind yunet_dp_fwd / yunet_dp_bwd) against

1. tests/golden/dp_routes.npz -- what the dispatchers of the commit before the rule was gathered into one place launched or
   refused for every case of tests/route_cases.py, and which triples their yunet_dp_fwd_group launched as one grid
   (yunet_dp_fwd_group_one_grid: the predicate the entry branches on);
2. bench.py's op_name, the mirror the benchmark keys its per-kernel table by, on the plans of the shipped nets."""
import ctypes as C
import hashlib
import importlib.util
import os

import numpy as np
import pytest

import route_cases as R
import yunet_amd._lib as L
import yunet_amd.engine as E
import yunet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPED = 'dp_fwd64s_kernel<false,false>'


@pytest.fixture(scope='module')
def golden():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'dp_routes.npz'))
    rows = R.cases()
    trip = R.group_triples(rows)
    assert hashlib.sha256(repr(rows).encode() + repr(trip).encode()).hexdigest() == str(g['cases_sha256']), \
        'tests/route_cases.py no longer enumerates the cases the fixture was recorded over'
    assert len(g['route']) == len(rows) and len(g['group']) == len(trip)
    return rows, trip, [str(n) for n in g['names']], g['route'], g['group']


def test_every_recorded_route_is_reproduced(golden):
    rows, _, names, route, _ = golden
    lib, opts, bad = L.load(), R.Options(L), []
    try:
        for i, case in enumerate(rows):
            opts.set(case)
            d = R.descriptor(case, L, lib.yunet_dp_bwd_blocks(case[3], case[4], case[5], case[1], case[2]))
            want = names[route[i]] if route[i] >= 0 else None
            got = R.route(lib, d, case[0])
            if got != want:
                bad.append((i, dict(zip(R.FIELDS, case)), want, got))
    finally:
        opts.restore()
    assert not bad, (len(bad), bad[:5])
    assert (route >= 0).sum() > 20000 and len(set(route[route >= 0])) == len(names) >= 90


def one_grid(lib, units):
    """yunet_dp_fwd_group_one_grid: the predicate yunet_dp_fwd_group itself branches on (dp_route.h: dp_fwd_one_grid)"""
    arr = (C.POINTER(L.YunetDP) * len(units))(*[C.pointer(d) for d in units])
    return lib.yunet_dp_fwd_group_one_grid(arr, len(units))


def test_group_predicate_reproduces_the_recorded_path(golden):
    """The predicate of yunet_dp_fwd_group, asked through yunet_dp_fwd_group_one_grid, against which path the recorded entry
    took for every triple.  The independent side: one grid exactly where n >= 2, option fwd_group is on, every unit's
    route in the build that is called is the plain non-deterministic 64 -> 64 streaming instance and no unit carries a prof
    of any kind -- the rule stated in Python over yunet_dp_route."""
    rows, trip, _, _, group = golden
    lib, opts, bad = L.load(), R.Options(L), []
    assert lib.yunet_set_option(b'fwd_group', 1) == 1          # (the default, under which the fixture was recorded)
    try:
        for t, (n, *idx) in enumerate(trip):
            opts.set(rows[idx[0]])
            units = [R.descriptor(rows[i], L, 0) for i in idx[:n]]
            build = 1 if units[0].x_dtype == 1 else 0
            stated = n >= 2 and all(d.x_dtype == build and not d.prof and R.route(lib, d, 0) == GROUPED for d in units)
            if not one_grid(lib, units) == stated == bool(group[t]):
                bad.append((t, n, idx, one_grid(lib, units), stated, int(group[t])))
    finally:
        opts.restore()
    assert not bad, (len(bad), bad[:5])
    assert 100 < group.sum() < len(group) - 100


def test_group_predicate_follows_option_and_count():
    lib = L.load()
    case = dict(zip(R.FIELDS, R.cases()[0]), cin=64, cout=64, N=4, H=20, W=20)
    units = [R.descriptor(tuple(case[k] for k in R.FIELDS), L, 0) for _ in range(4)]
    assert one_grid(lib, units[:2]) == one_grid(lib, units[:3]) == 1
    assert one_grid(lib, units[:1]) == 0 and one_grid(lib, units) == 0            # one unit; above YUNET_DP_GROUP_MAX
    assert lib.yunet_dp_fwd_group_one_grid(None, 2) == 0
    prev = L.set_option('fwd_group', 0)
    try:
        assert one_grid(lib, units[:3]) == 0
    finally:
        L.set_option('fwd_group', prev)


def test_an_ablation_mask_keeps_a_unit_out_of_the_group():
    """prof = an ablation mask (< 64): the unit still routes to dp_fwd64s on its own, and the group rule rejects it."""
    case = dict(zip(R.FIELDS, R.cases()[0]), cin=64, cout=64, N=4, H=20, W=20, prof=1)
    lib = L.load()
    d = R.descriptor(tuple(case[k] for k in R.FIELDS), L, 0)
    plain = R.descriptor(tuple(dict(case, prof=0)[k] for k in R.FIELDS), L, 0)
    assert d.prof == 1 and R.route(lib, d, 0) == R.route(lib, plain, 0) == GROUPED
    assert one_grid(lib, [plain, plain, plain]) == 1
    for units in ([d, plain, plain], [plain, d, plain], [plain, plain, d], [plain, d]):
        assert one_grid(lib, units) == 0
    d.prof = R.PTR                                              # the phase clocks: the tile kernel
    assert R.route(lib, d, 0) == 'dp_fwd_kernel<64,64,8,16,false,false,false>'
    assert one_grid(lib, [plain, d]) == 0


def test_reads_z_answers_before_the_buffers_are_bound():
    """dp_bwd_route chooses the family before it refuses anything: yunet_dp_bwd_reads_z is 0 for the streaming 16 -> 16 unit
    although the descriptor has no wgrad_partials yet (the plan builder asks at that point), while yunet_dp_route refuses it."""
    lib = L.load()
    case = dict(zip(R.FIELDS, R.cases()[0]), backward=1, cin=16, cout=16, N=2, H=32, W=64)
    d = R.descriptor(tuple(case[k] for k in R.FIELDS), L, lib.yunet_dp_bwd_blocks(2, 32, 64, 16, 16))
    assert lib.yunet_dp_bwd_reads_z(C.byref(d)) == 0 and R.route(lib, d, 1) == 'dp_bwd16s_kernel<false,false>'
    d.wgrad_partials, d.wgrad_blocks = None, 0
    assert lib.yunet_dp_bwd_reads_z(C.byref(d)) == 0 and R.route(lib, d, 1) is None


def test_name_buffer_is_respected():
    lib = L.load()
    d = R.descriptor(R.cases()[0], L, 0)
    name = R.route(lib, d, 0)
    assert name == 'dp_fwd16s_kernel<16,false,false>'
    for cap in range(-1, len(name) + 3):
        buf = C.create_string_buffer(b'\xaa' * 64, 64)
        rc = lib.yunet_dp_route(C.byref(d), 0, buf, cap)
        if cap <= len(name):                                    # no room for the terminator: refused, nothing written
            assert rc == L.EINVAL and buf.raw == b'\xaa' * 64, cap
        else:
            assert rc == 0 and buf.raw == name.encode() + b'\0' + b'\xaa' * (63 - len(name)), cap
    assert lib.yunet_dp_route(None, 0, C.create_string_buffer(64), 64) == L.EINVAL
    assert lib.yunet_dp_route(C.byref(d), 0, None, 64) == L.EINVAL


def _bench():
    spec = importlib.util.spec_from_file_location('bench_for_routes', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('kind,precision,shape', [
    (kind, precision, shape) for kind, big in (('n', 256), ('s', 512)) for precision in ('fp32', 'bf16')
    for shape in ((big, 320, 320, 64), (4, 128, 128, 64))])
def test_bench_op_names_are_the_routes(kind, precision, shape):
    """Default mode: for every ConvDPUnit op of the training plan, bench.op_name(op) is yunet_dp_route's name without its
    last argument (the deterministic form).  No exceptions."""
    bench, lib = _bench(), L.load()
    eng = E.YuNetEngine(O.yunet_arch(kind), 'cpu')
    eng.set_precision(precision)
    plan = E.Plan(eng, *shape)
    seen = 0
    for arr in (plan.c_fwd_a, plan.c_fwd_b, plan.c_bwd):
        for op in arr:
            if op.opcode in (L.OP_DP_FWD, L.OP_DP_BWD):
                name = R.route(lib, op.dp, int(op.opcode == L.OP_DP_BWD))
                assert name is not None and name.endswith(',false>'), (name, op.dp.cin, op.dp.cout, op.dp.H, op.dp.W)
                assert name[:name.rindex(',')] + '>' == bench.op_name(op, L), (op.dp.cin, op.dp.cout, op.dp.H, op.dp.W)
                seen += 1
    assert seen >= 30
