"""-m gpu: the one-shot all-reduce (csrc/collective.hip) at every piece count S = 1 | 2 | 4 | 8, with aligned and
unaligned buffers, the sum and the mean, S changing from call to call, and at world 2 AND 3 (three addends: the first
world at which "slots added in rank order" and "times the fp32 constant 1 / world" can be told from their neighbours).
Every element is compared bit for bit with the host restatement of tests/oneshot_cases.py, which
tests/test_oneshot_cases.py holds against fp64 and against the kernel's constants.  Also: a peer that arrives late but
within the time-out, and the NaN poisoning of a timed-out call at S = 4.

As in tests/test_oneshot_gpu.py the `world` processes share device 0 and use gloo only to exchange the IPC handles."""
import os
import socket
import time
import traceback

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oneshot_cases as K

pytestmark = pytest.mark.gpu

TIMEOUT_MS = 20000      # a lost flag ends as a failed assertion in seconds, not after the default of minutes


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)
    return torch.device('cuda', 0)


def _guarded(dev, n, off):
    """(base, view): n floats at GUARD + off floats into a sentinel-filled tensor, at least GUARD sentinels behind."""
    base = torch.full((K.GUARD + 3 + n + K.GUARD,), K.SENTINEL, device=dev)
    t = base[K.GUARD + off:K.GUARD + off + n]
    assert base.data_ptr() % 16 == 0 and (t.data_ptr() % 16 == 0) == (off == 0)
    return base, t


def _guards_intact(base, n, off):
    b = base.cpu().view(torch.int32)
    s = torch.full((1,), K.SENTINEL).view(torch.int32)
    return bool((b[:K.GUARD + off] == s).all()) and bool((b[K.GUARD + off + n:] == s).all())


def _run(body, rank, world, port, out):
    """Whatever happens in `body`, this rank reports and reaches the barrier, so that no peer is left behind."""
    dev = _init(rank, world, port)
    import yunet_amd._lib as L
    comm, prev = None, None
    try:
        from yunet_amd.oneshot import OneShotAllReduce
        comm = OneShotAllReduce(dev, K.COMM_BYTES)
        prev = L.set_option('oneshot_timeout_ms', TIMEOUT_MS)
        out[rank] = body(rank, world, dev, comm, L)
    except Exception:           # noqa: BLE001 -- reported to the test below
        out[rank] = dict(exc=traceback.format_exc())
    finally:
        if prev is not None:
            L.set_option('oneshot_timeout_ms', prev)
    dist.barrier()
    if comm is not None:
        comm.close()
    dist.destroy_process_group()


def _walk(rank, world, dev, comm, L):
    calls = K.schedule()
    # from the table, before anything runs: every size with S >= 2 meets an aligned and an unaligned buffer
    for n in K.SIZES:
        if K.pieces(n) >= 2:
            assert {c[2] > 0 for c in calls if c[1] == n} == {False, True}, n
    assert comm.max_bytes >= 4 * max(K.SIZES)
    ok_verify = comm.verify()       # one message with a short time-out of its own; the ranks agree on the answer
    if not ok_verify:               # no transport between these processes: do not queue 26 calls that each wait in vain
        return dict(verify=False, errs=[], status=comm.status(), counts={}, last=b'')
    bufs = []
    for it, n, off, mean in calls:
        base, t = _guarded(dev, n, off)
        t.copy_(K.inputs(n, rank, it))
        bufs.append((base, t))
    torch.cuda.synchronize()
    # the walk itself: no host synchronisation between the calls, except ONE on one rank, which lets the others run ahead
    for (it, n, off, mean), (base, t) in zip(calls, bufs):
        if comm.status() != 0:      # (host read, no synchronisation) a call gave up: the rest would only wait as well
            break
        comm.all_reduce_(t, mean=mean)
        if rank == 1 and it == len(calls) // 2:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    status = comm.status()      # set by any call whose wait gave up, and never cleared: read once for all of them
    errs, counts = [], {}
    for (it, n, off, mean), (base, t) in zip(calls, bufs):
        s = K.pieces(n)
        c = counts.setdefault(s, dict(calls=0, unaligned=0, means=0))
        c['calls'] += 1
        c['unaligned'] += off > 0
        c['means'] += mean
        w = K.want([K.inputs(n, r, it) for r in range(world)], mean)
        got = t.cpu()
        if not torch.equal(got, w):
            bad = (got.view(torch.int32) != w.view(torch.int32)).nonzero().flatten()
            i = int(bad[0])
            errs.append(dict(it=it, n=n, S=s, off=off, mean=mean, first=i, wrong=int(bad.numel()),
                             piece=K.owner(K.ranges(n, s), i), share=K.owner(K.ranges(n, world * s), i),
                             got=float(got[i]), want=float(w[i])))
        if not _guards_intact(base, n, off):
            errs.append(dict(it=it, n=n, S=s, off=off, mean=mean, guards='overwritten'))
    print(f'one-shot walk, world {world}, rank {rank}: ' + '; '.join(
        f'S={s}: {c["calls"]} calls, {c["unaligned"]} unaligned, {c["means"]} means' for s, c in sorted(counts.items())),
        flush=True)
    return dict(verify=ok_verify, errs=errs, status=status, counts=counts, last=bufs[-1][1].cpu().numpy().tobytes())


def _walk_worker(rank, world, port, out):
    _run(_walk, rank, world, port, out)


@pytest.mark.parametrize('world', K.WORLDS)
def test_every_piece_count_bit_exact(world):
    out = mp.Manager().dict()
    mp.spawn(_walk_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    for r in range(world):
        assert 'exc' not in out[r], out[r]['exc']
        assert out[r]['verify'], ('self-check against the process group failed', out[r]['status'])
        assert out[r]['errs'] == [], out[r]['errs'][:8]
        assert out[r]['status'] == 0, out[r]['status']
        assert sorted(out[r]['counts']) == [1, 2, 4, 8]
        for s, c in out[r]['counts'].items():
            assert c['calls'] > 0 and c['unaligned'] > 0 and c['means'] > 0, (s, c)
            assert c['unaligned'] < c['calls'] and c['means'] < c['calls'], (s, c)
    assert all(out[r]['last'] == out[0]['last'] for r in range(world)), 'the ranks hold different bits'


def _late(rank, world, dev, comm, L):
    n, off = 40001, 1
    base, t = _guarded(dev, n, off)
    t.copy_(K.inputs(n, rank, 5))
    torch.cuda.synchronize()
    if rank == 1:
        time.sleep(3.0)         # rank 0's kernel spins in its wait loop meanwhile
    t0 = time.time()
    comm.all_reduce_(t)
    torch.cuda.synchronize()
    return dict(result=t.cpu().numpy().tobytes(), status=comm.status(), guards=_guards_intact(base, n, off),
                waited=time.time() - t0)


def _late_worker(rank, world, port, out):
    _run(_late, rank, world, port, out)


def test_late_peer_within_the_timeout_is_waited_for():
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_late_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    w = K.want([K.inputs(40001, r, 5) for r in range(world)], False).numpy().tobytes()
    for r in range(world):
        assert 'exc' not in out[r], out[r]['exc']
        assert out[r]['status'] == 0
        assert out[r]['result'] == w
        assert out[r]['guards']
    assert out[0]['waited'] > 2.0, 'rank 0 did not have to wait: the test did not run the wait loop'


def _timeout_worker(rank, world, port, out):
    dev = _init(rank, world, port)
    from yunet_amd.oneshot import OneShotAllReduce
    import yunet_amd._lib as L
    n = 40001
    comm = OneShotAllReduce(dev, K.COMM_BYTES)
    base, t = _guarded(dev, n, 0)
    t.copy_(K.inputs(n, rank, 9))
    prev = L.set_option('oneshot_timeout_ms', 1000)
    if rank == 0:
        comm.all_reduce_(t)          # rank 1 never sends: all world * S = 8 blocks give up and poison their shares
    torch.cuda.synchronize()
    L.set_option('oneshot_timeout_ms', prev)
    out[rank] = dict(status=comm.status(), nans=int(torch.isnan(t).sum()), guards=_guards_intact(base, n, 0),
                     unchanged=torch.equal(t.cpu(), K.inputs(n, rank, 9)))
    dist.barrier()
    comm.close()
    dist.destroy_process_group()


def test_timeout_at_four_pieces_poisons_the_whole_message():
    world = 2
    assert K.pieces(40001) == 4
    out = mp.Manager().dict()
    mp.spawn(_timeout_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    # the status word names the call; every share is NaN, so the poison branch's shares tile the message, and stay in it
    assert out[0]['status'] == 1 and out[0]['nans'] == 40001 and out[0]['guards'], out[0]
    assert out[1]['status'] == 0 and out[1]['unchanged'] and out[1]['guards'], out[1]
