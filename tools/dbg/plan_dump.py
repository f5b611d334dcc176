"""Serialise the op lists of engine plans, built without a GPU, in a form two commits can be diffed on.

    python tools/dbg/plan_dump.py OUT.txt        # run at both commits, then `cmp` the two files
    python tools/dbg/plan_dump.py OUT.txt --elide   # the plans as a training process builds them by default

The plans are built with YUNET_KEEP_POOL_Z=1: every full-size output allocated, the form the recorded digest
(tests/golden/plan_dump_default.sha256) describes.  By default a plan drops the output of a fused-pool unit whose backward
recomputes it (Plan._elide_pool_z); --elide dumps that form, which differs from the other in those units' `dp.z` alone
(tests/test_pool_z_elision_plan.py).

A plan is a set of `YunetOp` arrays full of raw pointers; their values change from run to run, what must not change
is WHERE they point.  Every pointer is therefore written as (name of the plan / parameter buffer that contains it,
byte offset); a non-null pointer inside no known buffer is an error.  Buffers are named by how they are reached from
the plan (attribute, position in `keep`, unit name in `tensors`), so allocation order is pinned along with the ops.
Per configuration the dump holds the ten `c_*` arrays op by op (every field of the record), `reduce_jobs`, the
`bn_table_*` rows and `split_off` / `split_ops`.  The last line counts configurations and ops.
"""
import bisect
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle')]
import torch                          # noqa: E402
import yunet_oracle as O              # noqa: E402
import yunet_amd.engine as E          # noqa: E402

ARRAYS = ('c_fwd_a', 'c_fwd_b', 'c_fwd_b_loss', 'c_fwd_b_rest', 'c_bwd', 'c_bwd_a', 'c_bwd_b', 'c_bwd_a_k', 'c_tail_a',
          'c_fwd_eval')
SWITCHES = ('YUNET_LANES', 'YUNET_NO_HEAD_GROUP', 'YUNET_NO_POOL_FUSION', 'YUNET_NO_UPADD_POOL_FUSION')
SHAPES = ((1, 32, 32, 64), (4, 320, 320, 64), (2, 160, 224, 128))
ARCHS = (('n', {}), ('s', {}),
         ('n', dict(shared_stacked_convs=2)),                               # two grouped rounds of share convs
         ('n', dict(stacked_convs=2, shared_stacked_convs=2)),              # tower heads (tests/test_engine_gpu.py)
         ('n', dict(stacked_convs=1, shared_stacked_convs=0, loss_bbox='GIoULoss')))


class Buffers:
    """Address ranges of every buffer a plan's ops may point into -> (name, byte offset)."""

    def __init__(self, eng, plan):
        self.spans = {}         # start -> (end, name): the first name given to a buffer wins
        fp = eng.params
        for name in ('data', 'grad_buf', 'running_mean', 'running_var', 'num_batches_tracked'):
            self.add('params.' + name, getattr(fp, name))
        for name in sorted(vars(plan)):
            self.add(name, getattr(plan, name))
        for k, t in enumerate(plan.keep):
            self.add(f'keep[{k}]', t)
        for unit, (x, z) in plan.tensors.items():
            for t, side in ((x, 'x'), (z, 'z')):
                self.add(f'{unit}.{side}', t.buf)
                self.add(f'{unit}.{side}.grad', t.grad)
                if t.pooled_into is not None:
                    self.add(f'{unit}.{side}.pooled', t.pooled_into[0].buf)
                    self.add(f'{unit}.{side}.pooled.grad', t.pooled_into[0].grad)
        self.starts = sorted(self.spans)

    def add(self, name, t):
        if not isinstance(t, torch.Tensor) or t.numel() == 0:
            return
        st = t.untyped_storage()
        lo = st.data_ptr()
        self.spans.setdefault(lo, (lo + st.nbytes(), name))

    def where(self, ptr):
        if not ptr:
            return None
        k = bisect.bisect_right(self.starts, ptr) - 1
        if k >= 0:
            lo = self.starts[k]
            end, name = self.spans[lo]
            if ptr < end:
                return f'{name}+{ptr - lo}'
        raise RuntimeError(f'pointer {ptr:#x} lies in no known buffer')


def fields(obj, bufs, prefix, out):
    """Every field of a ctypes record, nested records and arrays flattened; pointers rewritten through `bufs`."""
    for name, typ in obj._fields_:
        v, key = getattr(obj, name), prefix + name
        if typ is C.c_void_p:
            out.append(f'{key}={bufs.where(v)}')
        elif issubclass(typ, C.Structure):
            fields(v, bufs, key + '.', out)
        elif issubclass(typ, C.Array):
            for k, e in enumerate(v):
                if isinstance(e, C.Structure):
                    fields(e, bufs, f'{key}[{k}].', out)
                elif typ._type_ is C.c_void_p:
                    out.append(f'{key}[{k}]={bufs.where(e)}')
                else:
                    out.append(f'{key}[{k}]={e.hex() if isinstance(e, float) else e}')
        else:
            out.append(f'{key}={v.hex() if isinstance(v, float) else v}')


def dump_plan(eng, plan, w):
    bufs = Buffers(eng, plan)
    n_ops = 0
    for arr_name in ARRAYS:
        arr = getattr(plan, arr_name, None)
        w(f'  {arr_name}: {"absent" if arr is None else len(arr)}')
        for k, op in enumerate(arr if arr is not None else ()):
            out = []
            fields(op, bufs, '', out)
            w(f'    [{k}] ' + ' '.join(out))
            n_ops += 1
    w('  reduce_jobs: ' + ' '.join(f'({bufs.where(p)},{bufs.where(g)},{r},{wd},{acc})' for p, g, r, wd, acc in plan.reduce_jobs))
    for name in ('bn_table_f', 'bn_table_b', 'bn_table_ba', 'bn_table_bb'):
        t = getattr(plan, name, None)
        w(f'  {name}: {"absent" if t is None else t.tolist()}')
    w(f'  split_off={plan.split_off} split_ops={getattr(plan, "split_ops", None)} lanes_used={plan.lanes_used} '
      f'assign_idx={plan.assign_idx} img_ptr_ops={plan.img_ptr_ops}')
    return n_ops


def main(path, elide=False):
    for s in SWITCHES:
        os.environ.pop(s, None)
    os.environ['YUNET_KEEP_POOL_Z'] = '0' if elide else '1'
    n_cfg = n_ops = 0
    with open(path, 'w') as f:
        def w(line):
            f.write(line + '\n')
        for kind, kw in ARCHS:
            for precision in ('fp32', 'bf16'):
                for world in (1, 2):
                    for switch in (None,) + SWITCHES:
                        if switch:
                            os.environ[switch] = '1'
                        try:
                            for n, h, wd, gmax in SHAPES:
                                eng = E.YuNetEngine(O.yunet_arch(kind, **kw), 'cpu', world_size=world)
                                eng.set_precision(precision)
                                plan = eng.get_plan(n, h, wd, gmax)
                                assert plan.gmax == gmax
                                w(f'== arch {kind} {kw} {precision} world {world} switch {switch} shape {(n, h, wd, gmax)}')
                                n_ops += dump_plan(eng, plan, w)
                                n_cfg += 1
                        finally:
                            if switch:
                                del os.environ[switch]
        w(f'{n_cfg} configurations, {n_ops} ops')
    print(f'{n_cfg} configurations, {n_ops} ops -> {path}')


if __name__ == '__main__':
    main(sys.argv[1], elide='--elide' in sys.argv[2:])
