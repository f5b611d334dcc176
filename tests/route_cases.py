"""The descriptors and options tests/golden/dp_routes.npz was recorded over, and how a row becomes a YunetDP.

A case is a tuple of small integers (FIELDS).  `cases()` enumerates the same list, in the same order, wherever it runs (its
own generator, no library state): every shape of SHAPES x PAIRS x BATCHES in both directions, with each axis moved off the
default alone and with seeded draws over all axes at once.  The fixture holds one answer per case -- the index of a kernel
name, or -1 for YUNET_EINVAL -- taken from the dispatchers of the commit it names, whose launchers were replaced by stubs
that report their template arguments; the pointers of a descriptor are made-up addresses nothing dereferences."""
import ctypes as C
import functools

FIELDS = ('backward', 'cin', 'cout', 'N', 'H', 'W', 'in_transform', 'out_has_bn', 'pool', 'z', 'z_dtype', 'x_dtype', 'det',
          'dx_null', 'accumulate_dx', 'prof', 'wgrad', 'nostats',
          'fwd16s', 'fwd64s', 'bwd16s', 'bwd_fp32mma', 'bwd32_split', 'no_pack', 'bwd64_nw')
OPTIONS = FIELDS[18:]
PAIRS = ((16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 64), (64, 16), (32, 16), (48, 64))     # the last two: no such unit
BATCHES = (1, 3, 4, 16, 17)
SHAPES = ((2, 2), (10, 10), (20, 20), (21, 20), (12, 20), (16, 32), (32, 64), (31, 64), (32, 63), (33, 65), (40, 40), (80, 80))
# axis -> its values, the default first.  pool: 0 none | 1 good | 2 pool_idx missing | 3 pool_idx misaligned | 4 gamma missing
# (backward: 0 | 1 | 3).  z: 0 a pointer | 1 NULL.  z_dtype: 0 = x_dtype | 1 fp32 | 2 bf16.  x_dtype: 2 = no such type.
# det: 0 | 1 = R | 2 = R | YUNET_DET_FAST.  prof: 0 NULL | 1 an ablation mask | 2 a pointer.  wgrad: 0 good | 1 wrong row
# count | 2 no buffer.  nostats: the sum block the deterministic form writes is missing.
AXES = {'in_transform': (1, 0, 2), 'out_has_bn': (1, 0), 'pool': (0, 1, 2, 3, 4), 'z': (0, 1), 'z_dtype': (0, 1, 2),
        'x_dtype': (0, 1, 2), 'det': (0, 1, 2), 'dx_null': (0, 1), 'accumulate_dx': (0, 1), 'prof': (0, 1, 2),
        'wgrad': (0, 1, 2), 'nostats': (0, 1),
        'fwd16s': (1, 0), 'fwd64s': (2, 1, 0), 'bwd16s': (1, 0), 'bwd_fp32mma': (0, 1), 'bwd32_split': (1, 0), 'no_pack': (0, 1),
        'bwd64_nw': (0, 4, 8)}
RANDOM_PER_SHAPE = 24
DET_ROWS, DET_FAST = 1024, 1 << 30
PTR = 0x10000


def _lcg(seed):
    x = seed
    while True:
        x = (x * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
        yield x >> 33


@functools.lru_cache(None)
def cases():
    out, rnd = [], _lcg(20240607)
    names = FIELDS[6:]
    for backward in (0, 1):
        for cin, cout in PAIRS:
            for n in BATCHES:
                for h, w in SHAPES:
                    head = (backward, cin, cout, n, h, w)
                    base = {k: AXES[k][0] for k in names}
                    rows = [dict(base)]
                    for k in names:                                      # one axis off the default
                        rows += [dict(base, **{k: v}) for v in AXES[k][1:]]
                    for det in (1, 2):                                   # ... and under both deterministic levels
                        rows += [dict(base, det=det, **{k: v}) for k in ('pool', 'prof', 'fwd64s', 'bwd_fp32mma', 'x_dtype')
                                 for v in AXES[k][1:]]
                    for _ in range(RANDOM_PER_SHAPE):                    # every axis at once; the default twice as likely
                        row = {}
                        for k in names:
                            vals = AXES[k]
                            i = next(rnd) % (len(vals) + 1)
                            row[k] = vals[0] if i == len(vals) else vals[i]
                        rows.append(row)
                    for row in rows:
                        if backward and row['pool'] in (2, 4):
                            row['pool'] = 1
                        out.append(head + tuple(row[k] for k in names))
    return tuple(out)


def group_triples(rows):
    """(n, i, j, k): yunet_dp_fwd_group over the descriptors of forward cases i, j, k (the first n of them) under the options
    of case i.  Drawn so that units which take the grouped kernel meet each other and, one at a time, every other kind."""
    fwd = [i for i, r in enumerate(rows) if not r[0]]
    likely = [i for i in fwd if rows[i][1:3] == (64, 64) and rows[i][FIELDS.index('pool')] == 0]
    rnd, out = _lcg(77), []
    for t in range(6000):
        pick = [likely[next(rnd) % len(likely)] for _ in range(3)]
        if t % 3:
            pick[next(rnd) % 3] = fwd[next(rnd) % len(fwd)]
        out.append((1 + next(rnd) % 3, *pick))
    return out


def descriptor(case, L, blocks):
    """The YunetDP of a case.  `blocks` = yunet_dp_bwd_blocks(N, H, W, cin, cout) under the case's options."""
    f = dict(zip(FIELDS, case))
    d = L.YunetDP()
    d.N, d.H, d.W, d.cin, d.cout = case[3], case[4], case[5], case[1], case[2]
    d.in_transform, d.out_has_bn, d.accumulate_dx = f['in_transform'], f['out_has_bn'], f['accumulate_dx']
    d.x_img_stride, d.z_img_stride = d.H * d.W * d.cin, d.H * d.W * d.cout
    d.x = d.w_pw = d.b_pw = d.w_dw = d.b_dw = d.dy = PTR
    d.z = None if f['z'] else PTR
    d.x_dtype = f['x_dtype']
    d.z_dtype = (f['x_dtype'], 0, 1)[f['z_dtype']]
    det = (0, DET_ROWS, DET_ROWS | DET_FAST)[f['det']]
    for bn, mine in ((d.in_bn, f['backward']), (d.out_bn, not f['backward'])):
        bn.stats = bn.bstats = bn.gamma = bn.beta = PTR
        bn.count, bn.eps, bn.slots = d.N * d.H * d.W, 1e-5, 1
        bn.det_rows = det if mine else 0
    if f['nostats']:
        if f['backward']:
            d.in_bn.bstats = None
        else:
            d.out_bn.stats = None
    d.dx = None if f['dx_null'] else PTR
    d.wgrad_partials = None if f['wgrad'] == 2 else PTR
    d.wgrad_blocks = blocks + (f['wgrad'] == 1)
    d.prof = (None, 1, PTR)[f['prof']]
    if f['pool']:
        d.pool_out = PTR
        d.pool_idx = {1: PTR, 2: None, 3: PTR + 1, 4: PTR}[f['pool']]
        if f['pool'] == 4:
            d.out_bn.gamma = None
    return d


class Options:
    """Sets the options of a case, only those that change; restore() puts back what it found."""

    def __init__(self, L):
        self.L, self.now, self.first = L, {}, {}

    def set(self, case):
        for k, v in zip(OPTIONS, case[18:]):
            if self.now.get(k) != v:
                prev = self.L.set_option(k, v)
                self.first.setdefault(k, prev)
                self.now[k] = v

    def restore(self):
        for k, v in self.first.items():
            self.L.set_option(k, v)
        self.now = {}


def route(lib, d, backward, cap=96):
    """yunet_dp_route: the name, or None where it refuses."""
    buf = C.create_string_buffer(cap)
    return buf.value.decode() if lib.yunet_dp_route(C.byref(d), backward, buf, cap) == 0 else None
