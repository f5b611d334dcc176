#!/usr/bin/env python
"""bench.py -- training images/sec of the YuNet hot path on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one full training iteration of YuNet_n on a 256-image 320x320 synthetic
WIDER-Face-shaped batch per GPU (BASELINE.json configs[1]): the reference's per-iteration
sequence model.train_step -> zero_grad -> loss.backward -> optimizer.step
(forward + SimOTA + 4 losses + backward + gradient all-reduce + SGD), fp32, inputs already
resident in HBM.  Rank 0 prints ONE JSON line.  Weights: the trained-checkpoint-like fixture
tests/golden/yunet_n_synth_trained.pth with structured synthetic faces (SimOTA dynamic_k 7-9);
--weights init = random initialisation on noise images.  --dtype bf16 = the second line (configs[2]);
--gpus N without a launcher re-executes under torch.distributed.run.

The timed window is exactly K = --steps steps after W = --warmup untimed ones; `ms_per_step` is its wall time over K
(a window much shorter than 0.5 s sits on the clock ramp: choose K from a first run's `ms_per_step`).
--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (float64 losses, float32 gradients and
post-update state): the inputs depend only on the arguments, so two builds can be compared output for output.

A plain run does only what the headline needs: set-up, the W warm-up steps, the K timed steps, the dump, the line.
--full measures the rest after the timed window (nothing it does changes `value`, `ms_per_step` or the dump); the
--no-* switches leave single parts of it out.  Extra objects on the line with --full (N=1 only):
  roofline     -- the dominant kernel FAMILY of the step (all template instances of one __global__ function, e.g. the
                  four of dp_bwd64_kernel), every launch timed with events on the launch stream; achieved = the family's
                  algorithmic bytes / its time; `instances` keeps the per-instance table; `step_frac` = the whole step's
                  bytes over the reference's op graph x img/s / 8 TB/s
  cpu_baseline -- the reference's own step (oracle/_ref under the mmcv stub; kind "reference") timed on this host's cores
                  over a bounded sample, `gpu_eager` = the same unmodified reference code on the MI355X through stock
                  PyTorch-ROCm ops (the "un-accelerated GPU" row of BASELINE.md)
  exact_fp32_bwd -- the step once more with every backward GEMM on the exact fp32 matrix instruction (fp32 line only)
  other_configs  -- 50-step windows of BASELINE.json configs[2..4] (after the headline configuration only)
N > 1 with --full: after the RCCL window the same window runs again through the one-shot all-reduce
(csrc/collective.hip) when its self-check passes; both are printed under `dist` (`value` stays the RCCL figure).
"""
import argparse
import ctypes as C
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
MFMA_F32_PEAK_TFLOPS = 157.3   # v_mfma_f32_16x16x4_f32: 256 CU x 4 SIMD x 64 FLOP/clk x 2.4 GHz
MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense bf16 (MI355X_MICROARCH.md; the headline 5 PF figure includes 2:1 sparsity)
KIND, H, W, BATCH = 'n', 320, 320, 256
DUMP_LIMIT_BYTES = 64 << 20


def parse():
    p = argparse.ArgumentParser()
    p.add_argument('--gpus', type=int, default=1)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--batch', type=int, default=BATCH, help='images per GPU (default 256)')
    p.add_argument('--size', type=int, default=H)
    p.add_argument('--kind', default=KIND, choices=['n', 's'])
    p.add_argument('--exact-steps', action='store_true',
                   help='accepted for older scripts: the timed window is always exactly --steps steps')
    p.add_argument('--dump-outputs', metavar='DIR', default=None,
                   help='write the last timed step\'s losses, gradients and updated state as DIR/<name>.npy')
    p.add_argument('--full', action='store_true',
                   help='after the timed window, also measure roofline + per-kernel tables, exact_fp32_bwd, '
                        'other_configs and cpu_baseline (N=1) or the one-shot all-reduce window (N>1)')
    p.add_argument('--no-cpu-baseline', action='store_true', help='--full without cpu_baseline')
    p.add_argument('--cpu-baseline-only', action='store_true', help=argparse.SUPPRESS)
    p.add_argument('--gpu-eager-only', action='store_true', help=argparse.SUPPRESS)
    p.add_argument('--no-gpu-eager', action='store_true',
                   help='--full without the un-accelerated-GPU row (the oracle\'s eager torch ops on cuda:0)')
    p.add_argument('--no-roofline', action='store_true', help='--full without roofline and the per-kernel tables')
    p.add_argument('--no-other-configs', action='store_true',
                   help='--full without the 50-step windows of BASELINE.json configs[2..4] after the headline')
    p.add_argument('--no-exact-bwd', action='store_true',
                   help='--full without the second timing with the exact-fp32 backward matrix instruction (exact_fp32_bwd)')
    p.add_argument('--no-live-traffic', action='store_true',
                   help='roofline.traffic from the committed profiles/ table instead of two live rocprofv3 --pmc passes')
    p.add_argument('--weights', default='trained', choices=['trained', 'init'],
                   help="trained: tests/golden/yunet_n_synth_trained.pth (2000 SGD iterations on structured synthetic "
                        "faces) + structured batches, so that SimOTA runs with dynamic_k of 7-9 like a real checkpoint; "
                        "init: random initialisation on noise images (dynamic_k = 1 for 90 %% of the GTs)")
    p.add_argument('--dtype', default='f32', choices=['f32', 'bf16'],
                   help="f32: the headline line (BASELINE configs[1]); bf16: activation storage + forward matrix "
                        "instruction in bf16, fp32 gradients / weights (configs[2]) -- a SECOND line, never the headline")
    return p.parse_args()


def self_launch(a):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run, one
    rank per GPU over RCCL (what tools/dist_train.sh:11-21 does for the reference)."""
    import socket
    import subprocess
    backend = os.environ.get('YUNET_DIST_BACKEND', 'nccl')
    have = torch.cuda.device_count()
    if backend == 'nccl' and have < a.gpus:
        raise SystemExit(f'--gpus {a.gpus}: only {have} GPU(s) visible; RCCL needs one device per rank '
                         '(YUNET_DIST_BACKEND=gloo lets ranks share a GPU for debugging)')
    sk = socket.socket()
    sk.bind(('127.0.0.1', 0))
    port = sk.getsockname()[1]
    sk.close()
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')     # dmabuf IPC: RCCL across processes
    env.setdefault('OMP_NUM_THREADS', '4')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={a.gpus}',
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


def dump_outputs(path, model, opt, out):
    """What one training step hands its caller, as DIR/<name>.npy: the five logged losses (float64), every parameter's
    gradient (grad.<name>, float32) and the state after the SGD update (state.<key>: parameters and BatchNorm buffers,
    float32, the integer batch counter as float64; momentum_buffer: the optimizer's flat float32 buffer)."""
    import numpy as np
    arrays = {k: np.array(float(v), dtype=np.float64) for k, v in out['log_vars'].items()}
    for name, p in model.named_parameters():
        arrays[f'grad.{name}'] = p.grad.detach().float().cpu().numpy()
    for k, v in model.state_dict().items():
        v = v.detach().cpu()
        arrays[f'state.{k}'] = (v.float() if v.is_floating_point() else v.double()).numpy()
    arrays['momentum_buffer'] = opt.state_dict()['momentum_buffer'].float().cpu().numpy()
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f'--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES} byte limit')
    os.makedirs(path, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(path, f'{k}.npy'), v)


# ----------------------------------------------------------------- algorithmic byte model
def op_bytes(op, L):
    """Algorithmic HBM bytes of one launch (SURVEY.md 8d 'unit-boundary traffic'):
    forward unit = in + out, backward unit = saved in + grad-out read + grad-in written
    (2*in + out elements); weights negligible.  fp32: 4 B per element.  bf16 mode: ACTIVATIONS
    (forward tensors, saved inputs) 2 B, gradients and the head output 4 B."""
    oc = op.opcode
    if oc in (L.OP_DP_FWD, L.OP_DP_BWD):
        d = op.dp
        px = d.N * d.H * d.W
        xb = 2 if d.x_dtype == L.BF16 else 4
        zb = 2 if d.z_dtype == L.BF16 else 4
        if oc == L.OP_DP_FWD:       # (+ the pooled winners and their position bytes when the pooling is fused)
            return px * (d.cin * xb + d.cout * zb) + ((px // 4) * d.cout * (zb + 1) if d.pool_out else 0)
        dxb = d.cin * 4 if d.dx else 0      # no input gradient is written for a leaf input
        if d.pool_idx:          # fused max_pool2d backward: dy is the pooled gradient (1/4 of the pixels) + position bytes
            return px * (d.cin * xb + dxb) + (px // 4) * d.cout * 5
        return px * (d.cin * xb + dxb + d.cout * 4)
    ab = 2 if op.i[11] == L.BF16 else 4
    if oc in (L.OP_STEM_FWD, L.OP_STEM_BWD):
        n, h, w = op.i[0], op.i[1], op.i[2]
        i, o = n * 3 * h * w * 4, n * (h // 2) * (w // 2) * 16
        # backward: the image is a leaf -- it is read once (z is recomputed from it), dy is read, NO input gradient is
        # written (rounds 1-5 charged 2 * i here: SURVEY 8d's generic 2*in + out; the counters said 773 MB, not 1 049)
        return i + o * ab if oc == L.OP_STEM_FWD else i + o * 4
    if oc in (L.OP_POOL_FWD, L.OP_POOL_BWD):
        n, h, w, c = op.i[0], op.i[1], op.i[2], op.i[3]
        i, o = n * h * w * c, n * h * w * c // 4
        if oc == L.OP_POOL_FWD:
            return (i + o) * ab
        # backward: z, the pooled gradient, dx written (+ the merge's share of a pyramid tap read, when fused: p[3])
        return i * ab + i * 4 + o * 4 + (i * 4 if op.p[3] else 0)
    if oc in (L.OP_UPADD_FWD, L.OP_UPADD_BWD):
        n, h, w, c = op.i[0], op.i[1], op.i[2], op.i[3]
        a, b = n * h * w * c, n * h * w * c // 4
        if oc == L.OP_UPADD_FWD:
            return (a + b + a) * ab
        if not op.p[3]:          # the fine tensor's share is applied by pool_bwd: dout read, zb read, dxb written
            return a * 4 + b * ab + b * 4
        return (a + b) * ab + (a + b) * 4 + a * 4
    if oc == L.OP_LOSS:
        return op.i[0] * op.i[1] * 16 * 4 * 2
    if oc == L.OP_ASSIGN:
        return op.i[0] * op.i[1] * 16 * 4
    return 0


def op_bytes_reference_graph(op, L):
    """The same model over the REFERENCE's op graph: a unit with fused pooling is charged as the plain unit
    plus the pooling kernel it replaced (forward: read z + write pooled; backward: read z + pooled gradient,
    write the full-size gradient) -- SURVEY.md 8d's 66.93 MB / image for YuNet_n 320x320."""
    b = op_bytes(op, L)
    if op.opcode == L.OP_STEM_BWD:
        # SURVEY 8d charges every backward unit 2*in + out, the stem included: keep ITS figure (66.93 MB / image) as the
        # numerator of step_frac so that the ceiling of BASELINE.md stays the yardstick; `step_frac_written_grads`
        # drops the image gradient nobody writes
        n, h, w = op.i[0], op.i[1], op.i[2]
        return 2 * n * 3 * h * w * 4 + n * (h // 2) * (w // 2) * 16 * 4
    if op.opcode in (L.OP_DP_FWD, L.OP_DP_BWD):
        d = op.dp
        px = d.N * d.H * d.W
        zb = 2 if d.z_dtype == L.BF16 else 4
        if op.opcode == L.OP_DP_FWD and d.pool_out:
            b = px * (d.cin * (2 if d.x_dtype == L.BF16 else 4) + d.cout * zb) + (px + px // 4) * d.cout * zb
        elif op.opcode == L.OP_DP_BWD and d.pool_idx:
            b = (px * (d.cin * (2 if d.x_dtype == L.BF16 else 4) + d.cin * 4 + d.cout * 4) +
                 px * d.cout * zb + px * d.cout * 4 + (px // 4) * d.cout * 4)
    return b


def op_flops(op, L):
    """Algorithmic matrix FLOPs of one launch: the 1x1 pointwise GEMM of a ConvDPUnit is
    2*cin*cout per pixel forward, and two such GEMMs (weight and input gradient) backward.
    (The backward kernel also recomputes the forward GEMM; that is not counted here.)"""
    if op.opcode in (L.OP_DP_FWD, L.OP_DP_BWD):
        d = op.dp
        f = 2 * d.N * d.H * d.W * d.cin * d.cout
        return f if op.opcode == L.OP_DP_FWD else 2 * f
    return 0


def executed_bf16(name, alg_tflops, dtype):
    """The bf16 matrix work a split-bf16 kernel EXECUTES for its algorithmic fp32 GEMM FLOPs, against the dense
    bf16 peak (= what MfmaUtil measures): the fp32 forward of 32 / 64-channel inputs runs 6 bf16 products per
    algorithmic product (exact 3-way split), dp_bwd64 runs 3 GEMMs (p recomputed, dW1, da) x 3 products for its
    2 algorithmic GEMMs; None for kernels on the exact fp32 instruction."""
    if name.startswith('dp_bwd64_kernel') or (name.startswith('dp_bwd_kernel<') and name.split(',')[5:6] == ['1']):      # template argument GEMM = 1
        mult, what = 1.5 * 3, '3 GEMMs (p recomputed, dW1, da) x 3 bf16 MFMA products each'
    elif dtype == 'f32' and (name.startswith('dp_fwd_kernel<64,') or name.startswith('dp_fwd_kernel<32,')
                             or name.startswith('dp_fwd64s_kernel')):
        mult, what = 6.0, 'exact 3-way split: 6 bf16 MFMA products per algorithmic product'
    elif dtype == 'bf16' and (name.startswith('dp_fwd_kernel<64,') or name.startswith('dp_fwd_kernel<32,')):
        mult, what = 1.0, 'one bf16 MFMA product per algorithmic product'
    else:
        return None
    return {'achieved': round(alg_tflops * mult, 1), 'peak': MFMA_BF16_PEAK_TFLOPS,
            'frac': round(alg_tflops * mult / MFMA_BF16_PEAK_TFLOPS, 4), 'what': what + ' vs the dense bf16 peak'}


def family_of(name):
    """The __global__ function a template instance belongs to: dp_bwd64_kernel<8,false,true> -> dp_bwd64_kernel."""
    return name.split('<', 1)[0]


def pmc_traffic(instances):
    """HBM bytes per launch, averaged over the launches of `instances` ({instance name: launches per step}), from the
    newest committed PMC summary (profiles/rNN_pmc_traffic.json, written by tools/profile_round.sh +
    tools/pmc_summary.py: separate FETCH_SIZE / WRITE_SIZE passes over this same bench step)."""
    import glob
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                          'profiles', 'r*_pmc_traffic.json')))
    if not files:
        return None, None
    try:
        tab = json.load(open(files[-1]))['kernels']
        tot = n = 0
        for name, launches in instances.items():
            key = name.replace(' ', '')
            if key not in tab:
                return None, None
            tot += tab[key]['traffic_bytes'] * launches
            n += launches
        return int(tot / n), os.path.basename(files[-1])
    except Exception:
        pass
    return None, None


def live_traffic(instances, a):
    """HBM bytes per launch averaged over the launches of `instances` ({instance name: launches per step}; the
    per-instance bytes come back as the second value), measured NOW: two child passes of this same bench step
    under `rocprofv3 --kernel-trace --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes, as
    MI355X_MICROARCH.md prescribes), reduced by tools/pmc_summary.per_kernel with the same unit and
    gfx950 corrections as the committed table (KiB -> bytes, FETCH_SIZE x 2).  None when rocprofv3
    is missing or a pass fails -- the caller then falls back to the committed table."""
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    if not os.path.exists(exe):
        return None, None
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, 'tools'))
    try:
        from pmc_summary import per_kernel
    finally:
        sys.path.pop(0)
    keys = {name: name.replace(' ', '') for name in instances}
    kib = {}
    for counter in ('FETCH_SIZE', 'WRITE_SIZE'):
        tmp = tempfile.mkdtemp(prefix='yunet_pmc_')
        try:
            subprocess.run([exe, '--kernel-trace', '--pmc', counter, '--output-format', 'csv', '-d', tmp, '-o', 'p',
                            '--', sys.executable, os.path.abspath(__file__), '--steps', '2', '--warmup', '1', '--exact-steps',
                            '--no-cpu-baseline', '--no-roofline', '--no-exact-bwd', '--no-other-configs', '--kind', a.kind, '--size', str(a.size),
                            '--batch', str(a.batch), '--weights', a.weights, '--dtype', a.dtype],
                           capture_output=True, timeout=90, cwd=tmp, env=dict(os.environ, TMPDIR=tmp))
            csvs = [os.path.join(r, f) for r, _, fs in os.walk(tmp) for f in fs if f.endswith('counter_collection.csv')]
            if not csvs:
                return None, None
            tab = per_kernel(csvs[0])
            if any(k not in tab for k in keys.values()):
                return None, None
            kib[counter] = {name: tab[k][1] for name, k in keys.items()}
        except Exception:
            return None, None
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    per = {name: int(2 * kib['FETCH_SIZE'][name] * 1024 + kib['WRITE_SIZE'][name] * 1024) for name in instances}
    n = sum(instances.values())
    return int(sum(per[name] * instances[name] for name in instances) / n), per


# the dispatcher options this process started with (include/yunet_hip.h: yunet_set_option reads the same variables once)
OPTS = {'no_pack': bool(os.environ.get('YUNET_NO_PACK')), 'bwd_fp32mma': bool(os.environ.get('YUNET_BWD_FP32MMA')),
        'bwd64_nw': int(os.environ.get('YUNET_BWD64_NW') or 0),
        'fwd_group': int(os.environ.get('YUNET_FWD_GROUP', '1'))}


def op_name(op, L):
    names = {L.OP_STEM_FWD: 'stem_fwd_kernel', L.OP_STEM_BWD: 'stem_bwd_kernel',
             L.OP_POOL_FWD: 'pool_fwd_kernel', L.OP_POOL_BWD: 'pool_bwd_kernel',
             L.OP_UPADD_FWD: 'upadd_fwd_kernel', L.OP_UPADD_BWD: 'upadd_bwd_kernel',
             L.OP_ASSIGN: 'assign_compact+topk+resolve_kernel', L.OP_LOSS: 'loss_kernel',
             L.OP_LOSS_NORM: 'loss_norm_kernel', L.OP_LOSS_FINALIZE: 'loss_finalize_kernel',
             L.OP_BN_RUNNING: 'bn_running_kernel', L.OP_BN_PARAM_GRAD: 'bn_param_grad_kernel',
             L.OP_REDUCE_PARTIALS: 'reduce_partials_kernel', L.OP_MEMSET: 'memset',
             L.OP_REDUCE_BATCH: 'reduce_partials_batch_kernel', L.OP_BN_BATCH: 'bn_batch_kernel'}
    if op.opcode in (L.OP_STEM_FWD, L.OP_STEM_BWD) and int(os.environ.get('YUNET_STEM_MMA', '1')):
        # round 4: the stem as matrix products (csrc/conv_stem.hip); the backward recomputes z from the image
        return 'stem_mma_kernel<false>' if op.opcode == L.OP_STEM_FWD else 'stem_mma_kernel<true>'
    if op.opcode in (L.OP_DP_FWD, L.OP_DP_BWD):
        # the template instance the C dispatcher picks (csrc/conv_fwd.hip / conv_bwd.hip / common.h):
        # 16x32 tiles for 16->16 on big maps, packed-canvas tiling for 64->{64,16} on maps <= 20x20
        d = op.dp
        big = d.cin == 16 and d.cout == 16 and d.W >= 64 and d.H >= 32
        packed = (d.cin == 64 and d.cout in (64, 16) and d.H <= 20 and d.W <= 20 and d.N >= 4
                  and not OPTS.get('no_pack'))
        kind = 'fwd' if op.opcode == L.OP_DP_FWD else 'bwd'
        # backward: template argument 1 = split-bf16 matrix path (64 -> 64 units), 0 = exact fp32; then
        # true = dy is a pooled gradient + argmax bytes (fused max_pool2d backward)
        gemm = ''
        if kind == 'bwd':
            if d.cin == 64 and d.cout == 64 and not OPTS.get('bwd_fp32mma'):
                # round 3: dp_bwd64_kernel<waves, packed, pooled dy> (csrc/conv_bwd.hip: bwd64_nw) -- 4 waves (8 x 8
                # tiles, two workgroups per CU) where the width is a multiple of 8 but not of 16, else 8 (8 x 16 tiles)
                forced = OPTS.get('bwd64_nw')
                nw = forced if forced in (4, 8) else (4 if (not packed and d.W % 16 != 0 and d.W % 8 == 0) else 8)
                return f"dp_bwd64_kernel<{nw},{'true' if packed else 'false'},{'true' if d.pool_idx else 'false'}>"
            # round 4: the fp32 16 -> 16 unit on the big maps runs on the wave-streaming kernel that recomputes z
            # (csrc/conv_bwd16.hip) unless YUNET_BWD16S=0
            if (big and d.out_has_bn and d.dx and not d.accumulate_dx
                    and int(os.environ.get('YUNET_BWD16S', '1'))):
                return f"dp_bwd16s_kernel<{'true' if d.pool_idx else 'false'}>"
            # round 5: the 32 -> 64 unit (YuNet_s) runs the split-bf16 variant (template argument 1) unless YUNET_BWD32_SPLIT=0
            gemm = ',1' if ((d.cin, d.cout) == (32, 64) and not OPTS.get('bwd_fp32mma')
                            and int(os.environ.get('YUNET_BWD32_SPLIT', '1'))) else ',0'
            gemm += ',true' if d.pool_idx else ',false'
            # last argument: the whole-tile instance (map = exact multiple of the tile, no validity tests)
            th, tw = (16, 32) if big else (8, 16)
            full = (not packed and d.H % th == 0 and d.W % tw == 0 and
                    ((d.cin, d.cout) in ((16, 16), (16, 32), (16, 64), (32, 32)) if not d.pool_idx else d.cin in (16, 32))
                    and (big or (d.cin, d.cout) != (16, 16)))
            gemm += ',true' if full else ',false'
        else:
            # round 4: the plain fp32 64 -> 64 forward unit runs on the wave-streaming kernel (csrc/conv_fwd64.hip)
            # the fp32 units with 16 input channels (16 -> 16 plain / fused pooling, 16 -> 64): csrc/conv_fwd16.hip
            if (d.cin == 16 and d.z_dtype == d.x_dtype and int(os.environ.get('YUNET_FWD16S', '1'))
                    and (d.cout == 16 or (d.cout == 64 and not d.pool_out))):
                return f"dp_fwd16s_kernel<{d.cout},{'true' if d.pool_out else 'false'}>"
            # (since the small-level measurement also on the 20 x 20 / 10 x 10 levels unless YUNET_FWD64S=1)
            f64s = int(os.environ.get('YUNET_FWD64S', '2'))
            if d.cin == 64 and d.cout == 64 and d.z_dtype == d.x_dtype and f64s >= (2 if packed else 1):
                return 'dp_fwd64s_kernel<true>' if d.pool_out else 'dp_fwd64s_kernel<false>'
            gemm = ',true' if d.pool_out else ',false'      # forward: fused pooling outputs
        return (f"dp_{kind}_kernel<{d.cin},{d.cout},{'16,32' if big else '8,16'},"
                f"{'true' if packed and not big else 'false'}{gemm}>")
    return names.get(op.opcode, f'op{op.opcode}')


def profile_ops(eng, reps=3):
    """Time every launch of the step individually: events on the launch stream around
    single-op yunet_exec calls.  Returns {kernel name: dict(launches, ms, bytes)} per step."""
    import yunet_amd._lib as L
    plan = eng.plan
    stream = torch.cuda.current_stream()
    sptr = C.c_void_p(stream.cuda_stream)
    agg = {}
    eng.lib.yunet_exec_lanes(0)        # single-op timing: everything on the launch stream, FORK / JOIN are no-ops
    for rep in range(reps + 1):
        for arr in (plan.c_fwd_a, plan.c_fwd_b, plan.c_bwd):
            evs = []
            k = 0
            while k < len(arr):
                if arr[k].opcode in (L.OP_FORK, L.OP_JOIN):
                    k += 1
                    continue
                # a group of independent units (YunetOp.i[OP_GROUP]) is ONE launch: timed as the step runs it
                g = int(arr[k].i[L.OP_GROUP]) if arr[k].opcode == L.OP_DP_FWD else 0
                g = g if 2 <= g <= L.DP_GROUP_MAX and k + g <= len(arr) else 1
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc = eng.lib.yunet_exec(C.cast(C.byref(arr, k * C.sizeof(L.YunetOp)),
                                               C.POINTER(L.YunetOp)), g, sptr)
                e1.record(stream)
                assert rc == 0, rc
                evs.append((k, g, e0, e1))
                k += g
            torch.cuda.synchronize()
            if rep == 0:
                continue            # warm-up pass
            for k, g, e0, e1 in evs:
                op = arr[k]
                members = [arr[k + j] for j in range(g)]
                name = op_name(op, L)
                if g > 1 and name == 'dp_fwd64s_kernel<false>' and OPTS.get('fwd_group', 1):
                    name = 'dp_fwd64s_group_kernel'          # (csrc/conv_fwd64.hip: the units' grids in one launch)
                a = agg.setdefault(name, dict(launches=0, ms=0.0, bytes=0, flops=0))
                a['launches'] += 1
                a['ms'] += e0.elapsed_time(e1)
                a['bytes'] += sum(op_bytes(m, L) for m in members)
                a['ref_bytes'] = a.get('ref_bytes', 0) + sum(op_bytes_reference_graph(m, L) for m in members)
                a['flops'] += sum(op_flops(m, L) for m in members)
                if op.opcode in (L.OP_DP_FWD, L.OP_DP_BWD):      # the same instance runs on several map sizes
                    label = '+'.join(f'{m.dp.H}x{m.dp.W}' for m in members)
                    sh = a.setdefault('shapes', {}).setdefault(label, dict(launches=0, ms=0.0, bytes=0))
                    sh['launches'] += 1
                    sh['ms'] += e0.elapsed_time(e1)
                    sh['bytes'] += sum(op_bytes(m, L) for m in members)
    eng.lib.yunet_exec_lanes(1)
    for a in agg.values():
        a['launches'] //= reps
        a['ms'] /= reps
        a['bytes'] //= reps
        a['ref_bytes'] //= reps
        a['flops'] //= reps
        for sh in a.get('shapes', {}).values():
            sh['launches'] //= reps
            sh['ms'] /= reps
            sh['bytes'] //= reps
    return agg


def gpu_clock_mhz(index=0):
    """Current shader clock in MHz (the starred level of pp_dpm_sclk), None where sysfs does not say.  The card numbering of
    /sys/class/drm is not the HIP device numbering (some boxes list another adapter first): on a one-GPU box the busy GPU
    is the card with the highest current level, with several GPUs the index-th card that exposes the file."""
    import glob
    vals = []
    for path in sorted(glob.glob('/sys/class/drm/card*/device/pp_dpm_sclk')):
        try:
            for line in open(path):
                if line.rstrip().endswith('*'):
                    vals.append(int(''.join(ch for ch in line.split(':', 1)[1] if ch.isdigit())))
                    break
        except Exception:
            pass
    if not vals:
        return None
    world = int(os.environ.get('WORLD_SIZE', 1))
    return vals[min(index, len(vals) - 1)] if world > 1 else max(vals)


def plan_reference_graph_bytes(eng):
    """Bytes one step moves over the REFERENCE's op graph (op_bytes_reference_graph summed over the plan)."""
    import yunet_amd._lib as L
    plan = eng.plan
    return sum(op_bytes_reference_graph(arr[k], L) for arr in (plan.c_fwd_a, plan.c_fwd_b, plan.c_bwd)
               for k in range(len(arr)))


def run_other_config(kind, size, batch, dtype, dev, steps=50, warmup=5):
    """One of BASELINE.json's other single-GPU configurations, timed in this process after the headline: the same
    full step (fwd + SimOTA + losses + bwd + SGD) on a fresh model, `steps` steps after `warmup`, inputs resident."""
    import yunet_amd
    import yunet_amd.synthetic as S
    from yunet_amd.optim import FusedSGD
    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{kind}.py'))
    torch.manual_seed(0)
    model = yunet_amd.build_detector(cfg.model).to(dev)
    model.train()
    if dtype == 'bf16':
        model.set_precision('bf16')
    opt = FusedSGD(model, lr=cfg.optimizer['lr'] * 0.001, momentum=cfg.optimizer['momentum'],
                   weight_decay=cfg.optimizer['weight_decay'])
    # trained-like weights wherever a fixture of the architecture exists (YuNet is fully convolutional: the 320x320
    # fixture also drives the 640x640 configuration); structured faces then make SimOTA run with dynamic_k > 1
    fixture = os.path.join(ROOT, 'tests', 'golden', f'yunet_{kind}_synth_trained.pth')
    trained = os.path.exists(fixture)
    if trained:
        model.load_state_dict(torch.load(fixture, map_location='cpu', weights_only=False)['state_dict'], strict=True)
    pool = []
    for i in range(2):
        b = S.make_batch(batch, size, size, S.batch_seed(0, i), with_img=not trained)
        if trained:
            gen = torch.Generator(device=dev).manual_seed(S.batch_seed(0, i))
            img = torch.rand(batch, 3, size, size, generator=gen, device=dev) * 255.0
            b['img'] = S.render_faces(img, b['gt_bboxes'], b['gt_keypointss'])
        pool.append(S.to_device(b, dev))

    def step(i):
        out = model.train_step(pool[i % 2], opt)
        opt.zero_grad()
        out['loss'].backward()
        opt.step()
        return out
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out = step(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms = 1000.0 * dt / steps
    res = {'ms_per_step': round(ms, 3), 'value': round(batch * steps / dt, 1), 'unit': 'images/sec', 'steps': steps,
           'warmup': warmup, 'dtype': dtype,
           'step_reference_graph_GBs': round(plan_reference_graph_bytes(model.engine) / (ms * 1e-3) / 1e9, 1),
           'final_loss': round(float(out['log_vars']['loss']), 4),
           'weights': 'trained fixture + structured faces' if trained else 'random init + noise images'}
    del model, opt, pool
    torch.cuda.empty_cache()
    return res


def effective_cores():
    """Host cores actually usable by this process (affinity mask, capped by the cgroup quota)."""
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except Exception:
        pass
    for path in ('/sys/fs/cgroup/cpu.max', '/sys/fs/cgroup/cpu/cpu.cfs_quota_us'):
        try:
            txt = open(path).read().split()
            if path.endswith('cpu.max'):
                if txt[0] != 'max':
                    cores = min(cores, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                per = int(open('/sys/fs/cgroup/cpu/cpu.cfs_period_us').read())
                if q > 0:
                    cores = min(cores, max(1, q // per))
        except Exception:
            pass
    return cores


def ref_vs_port(bs=None):
    """Measured ratio reference-under-stub / port on the build box (profiles/r*_cpu_ref_vs_port[_bsNN].json,
    written by tools/cpu_ref_vs_port.py where /root/reference exists) -- the file measured at the batch size
    the baseline reports if there is one, else the newest; None if never measured."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, 'profiles', f'r*_cpu_ref_vs_port_bs{bs}.json'))) if bs else []
    files = files or sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_cpu_ref_vs_port*.json')))
    if not files:
        return None
    try:
        return json.load(open(files[-1]))
    except Exception:
        return None


def cpu_baseline_worker(kind, size, seed=1234, budget_s=24.0, device='cpu'):
    """cpu_baseline: the REFERENCE's own training step -- its unmodified Python files (oracle/_ref, put there by
    oracle/make_ref.sh; /root/reference in the build container) on torch CPU under the arithmetic-free mmcv stub of
    oracle/ref_stub.py, driven the way the mmcv runner drives it (train_step -> zero_grad -> backward -> SGD step)
    -- on a bounded sample of the same workload, kind = "reference"; the oracle port (oracle/yunet_oracle.py) is
    timed beside it and reported as `port`.  Without a reference tree only the port runs (kind = "port").
    device='cuda' is the 'un-accelerated GPU' row: the port's eager ops through stock PyTorch-ROCm on the MI355X."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import yunet_oracle as O
    import yunet_amd.synthetic as S
    cores = effective_cores()
    torch.set_num_threads(cores)
    arch = O.yunet_arch(kind)
    sync = (lambda: None) if device == 'cpu' else torch.cuda.synchronize
    have_ref = False
    try:                       # (device 'cuda': the un-accelerated-GPU row runs the reference's own files too)
        import ref_stub
        have_ref = ref_stub.available()
    except Exception:
        have_ref = False

    def timed(fn, budget):
        fn()                                    # warm-up (MIOpen kernel selection on the GPU, page-in on the CPU)
        sync()
        t0 = time.time()
        iters = 0
        while iters < 2 or (time.time() - t0 < budget and iters < 50):
            fn()
            iters += 1
        sync()
        return iters, time.time() - t0

    # Two batch sizes, the better one is reported: on the MI355X host torch's CPU convolutions fall off a
    # cliff between bs 16 and bs 32 (measured 129 vs 33 img/s on 16 threads, tools/ubench/cpu_probe.py),
    # and the baseline should be the CPU's best case
    sizes = (16, 32) if device == 'cpu' else (32,)
    share = budget_s / (len(sizes) * (2 if have_ref else 1))
    runs = {'port': [], 'reference': []}
    for bs in sizes:
        sd = O.init_state(arch, seed=0)
        b = S.make_batch(bs, size, size, seed)
        if device != 'cpu':
            dev = torch.device(device)
            sd = {k: v.to(dev) for k, v in sd.items()}
            b = dict(b, img=b['img'].to(dev), gt_bboxes=[t.to(dev) for t in b['gt_bboxes']],
                     gt_labels=[t.to(dev) for t in b['gt_labels']],
                     gt_keypointss=[t.to(dev) for t in b['gt_keypointss']])
        if have_ref:
            model, _ = ref_stub.build_detector(f'yunet_{kind}.py')
            model.load_state_dict(sd, strict=True)
            if device != 'cpu':
                model.to(torch.device(device))
            model.train()
            ropt = torch.optim.SGD(model.parameters(), lr=1e-5, momentum=0.9, weight_decay=5e-4)
            data = dict(img=b['img'], img_metas=b['img_metas'], gt_bboxes=list(b['gt_bboxes']),
                        gt_labels=list(b['gt_labels']), gt_keypointss=list(b['gt_keypointss']))

            def ref_step():
                out = model.train_step(data, ropt)
                ropt.zero_grad()
                out['loss'].backward()
                ropt.step()
            iters, dt = timed(ref_step, share)
            runs['reference'].append((bs * iters / dt, bs, iters))
            del model, ropt
        sd_p = {k: v.clone() for k, v in sd.items()}
        opt = O.SGD(lr=1e-5)
        iters, dt = timed(lambda: O.train_step(b, sd_p, arch, opt), share)
        runs['port'].append((bs * iters / dt, bs, iters))

    def describe(which, what):
        rate, bs, iters = max(runs[which])
        others = '; '.join(f'bs {b_}: {r_:.1f} img/s' for r_, b_, _ in runs[which])
        return rate, (f'{what} (fwd+SimOTA+losses+bwd+SGD), YuNet_{kind} {size}x{size} bs {bs}, {iters} iters after '
                      f'1 warm-up, torch fp32 ({others})')
    prate, pwhat = describe('port', 'oracle/yunet_oracle.py train_step')
    if device != 'cpu':
        tail = ', eager PyTorch-ROCm ops on cuda:0 (un-accelerated GPU row)'
        if have_ref:
            rrate, rwhat = describe('reference', "the reference's own detector.train_step + torch.optim.SGD: its "
                                                 'unmodified files (oracle/_ref) under the mmcv stub of oracle/ref_stub.py')
            return dict(value=round(rrate, 2), unit='images/sec', kind='reference', sample=rwhat + tail,
                        port=dict(value=round(prate, 2), unit='images/sec', sample=pwhat + tail))
        return dict(value=round(prate, 2), unit='images/sec', kind='port', sample=pwhat + tail)
    cpu = platform.processor() or platform.machine()
    try:
        with open('/proc/cpuinfo') as f:
            cpu = next((ln.split(':', 1)[1].strip() for ln in f if ln.startswith('model name')), cpu)
    except OSError:
        pass
    port = dict(value=round(prate, 2), unit='images/sec', sample=pwhat + f', {cores} threads')
    if not have_ref:
        res = dict(value=port['value'], unit='images/sec', cores=cores, cpu=cpu, kind='port', sample=port['sample'])
        rp = ref_vs_port(max(runs['port'])[1])
        if rp:
            res['reference_over_port'] = rp.get('ratio')
            res['sample'] += (f"; no reference tree here (oracle/make_ref.sh) -- on the build box ({rp.get('cores')} cores) the "
                              f"reference's own files ran {rp.get('reference_img_s')} img/s vs this port {rp.get('port_img_s')} img/s")
        return res
    where = os.path.relpath(ref_stub.REF_ROOT, ROOT) if ref_stub.REF_ROOT.startswith(ROOT) else ref_stub.REF_ROOT
    rrate, rwhat = describe('reference', "the reference's own detector.train_step + torch.optim.SGD: its unmodified files "
                                         f'({where}) under the mmcv stub of oracle/ref_stub.py')
    return dict(value=round(rrate, 2), unit='images/sec', cores=cores, cpu=cpu, kind='reference',
                sample=rwhat + f', {cores} threads', port=port, reference_over_port=round(rrate / prate, 3))


def _child(flag, kind, size, timeout, env_extra):
    import subprocess
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), flag, '--kind', kind,
                              '--size', str(size)], capture_output=True, text=True, timeout=timeout,
                             env=dict(os.environ, **env_extra))
        for line in reversed(out.stdout.strip().splitlines()):
            if line.startswith('{'):
                return json.loads(line)
        return dict(value=None, unit='images/sec', kind='port',
                    sample='worker produced no result: ' + out.stderr[-200:])
    except subprocess.TimeoutExpired:
        return dict(value=None, unit='images/sec', kind='port',
                    sample=f'worker exceeded its {timeout} s bound')


def cpu_baseline(kind, size):
    """Run the worker in a child process with a hard wall-clock bound."""
    r = _child('--cpu-baseline-only', kind, size, 300, dict(HIP_VISIBLE_DEVICES=''))
    r.setdefault('cores', effective_cores())
    return r


def gpu_eager(kind, size):
    return _child('--gpu-eager-only', kind, size, 240, {})


def main():
    a = parse()
    if a.cpu_baseline_only:
        print(json.dumps(cpu_baseline_worker(a.kind, a.size)))
        return
    if a.gpu_eager_only:
        print(json.dumps(cpu_baseline_worker(a.kind, a.size, budget_s=10.0, device='cuda')))
        return
    world = int(os.environ.get('WORLD_SIZE', 1))
    rank = int(os.environ.get('RANK', 0))
    local = int(os.environ.get('LOCAL_RANK', 0))
    if a.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        self_launch(a)
    local = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        # 'nccl' is RCCL on ROCm; YUNET_DIST_BACKEND=gloo lets several ranks share one GPU (debug)
        backend = os.environ.get('YUNET_DIST_BACKEND', 'nccl')
        kw = dict(device_id=dev) if backend == 'nccl' else {}     # bind the communicator to this GPU
        dist.init_process_group(backend, rank=rank, world_size=world, **kw)

    import yunet_amd
    import yunet_amd._lib as L
    import yunet_amd.synthetic as S
    from yunet_amd.optim import FusedSGD
    from yunet_amd.parallel import YuNetDistributedDataParallel

    cfg = yunet_amd.Config.fromfile(os.path.join(ROOT, 'configs', f'yunet_{a.kind}.py'))
    torch.manual_seed(0)
    model = yunet_amd.build_detector(cfg.model).to(dev)
    model.train()
    if a.dtype == 'bf16':
        model.set_precision('bf16')
    wrapped = YuNetDistributedDataParallel(model, device_ids=[local]) if world > 1 else model
    opt = FusedSGD(model, lr=cfg.optimizer['lr'] * 0.001, momentum=cfg.optimizer['momentum'],
                   weight_decay=cfg.optimizer['weight_decay'])   # lr at warm-up iteration 0

    # trained-checkpoint-like weights: only for the architecture / size the fixture was trained on
    fixture = os.path.join(ROOT, 'tests', 'golden', f'yunet_{a.kind}_synth_trained.pth')
    trained = a.weights == 'trained' and os.path.exists(fixture)
    if trained:
        model.load_state_dict(torch.load(fixture, map_location='cpu', weights_only=False)['state_dict'], strict=True)

    # synthetic batches, resident in HBM before the timed region
    def make(i):
        if not trained:
            return S.to_device(S.make_batch(a.batch, a.size, a.size, S.batch_seed(rank, i)), dev)
        b = S.make_batch(a.batch, a.size, a.size, S.batch_seed(rank, i), with_img=False)
        gen = torch.Generator(device=dev).manual_seed(S.batch_seed(rank, i))
        img = torch.rand(a.batch, 3, a.size, a.size, generator=gen, device=dev) * 255.0
        b['img'] = S.render_faces(img, b['gt_bboxes'], b['gt_keypointss'])      # face patterns over the noise
        return S.to_device(b, dev)
    pool = [make(i) for i in range(2)]

    def step(i):
        out = wrapped.train_step(pool[i % len(pool)], opt)
        opt.zero_grad()
        out['loss'].backward()
        opt.step()
        return out

    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    if world > 1:
        model.engine.comm_timing = True      # events around the collectives: exposed / overlapped ms per step
    bar = dict(device_ids=[local]) if world > 1 and dist.get_backend() == 'nccl' else {}

    def window(nsteps):
        """Time exactly `nsteps` steps between barrier + synchronize on both sides; the job's time is the MAX over
        ranks.  Returns (dt, per-rank times, clock before / after, the last step's outputs, comm report)."""
        if world > 1:
            model.engine.comm_report(1)          # drop events recorded before this window
            dist.barrier(**bar)
        torch.cuda.synchronize()
        c0 = gpu_clock_mhz(local)
        t0 = time.perf_counter()
        o = None
        for i in range(nsteps):
            o = step(i)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier(**bar)
        torch.cuda.synchronize()
        d = time.perf_counter() - t0
        c1 = gpu_clock_mhz(local)
        rep = model.engine.comm_report(nsteps) if world > 1 else None
        every = [d]
        if world > 1:
            t = torch.tensor([d], device=dev, dtype=torch.float64)
            got = [torch.zeros_like(t) for _ in range(world)]
            dist.all_gather(got, t)
            every = [float(v.item()) for v in got]
        return max(every), every, c0, c1, o, rep            # the job is as fast as its slowest rank

    dt, per_rank, clk0, clk1, out, comm = window(a.steps)
    last_loss = float(out['log_vars']['loss'])
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, model, opt, out)      # before any later section runs another step

    res = None
    if rank == 0:
        res = {
            'metric': ('training images/sec, YuNet_n 320x320 bs=256/GPU' if (a.kind, a.size, a.batch) == (KIND, H, BATCH)
                       else f'training images/sec, YuNet_{a.kind} {a.size}x{a.size} bs={a.batch}/GPU') +
            (', bf16 fwd / fp32 grads' if a.dtype == 'bf16' else ''),
            'value': round(world * a.batch * a.steps / dt, 1), 'unit': 'images/sec',
            'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup,
            'ms_per_step': round(1000.0 * dt / a.steps, 3), 'higher_is_better': True,
            'scaling': 'weak', 'vs_baseline': None, 'dtype': a.dtype,
            'data': 'synthetic' if not trained else 'synthetic (face patterns painted over noise at the GT boxes)',
            'config': {'workload': f'YuNet_{a.kind} {a.size}x{a.size} bs={a.batch}/GPU full training step, ' +
                                   ('fp32 (64->64 backward GEMMs: two-way bf16 split -- measured against the exact-fp32 instruction: every output '
                                    'within 9e-6 of its tensor maximum, 50 SGD iterations end as far from the exact path as a '
                                    'last-bit perturbation of it does, tests/test_precision_gpu.py + profiles/r05_precision.json; '
                                    'the strictly-fp32 variant is timed in exact_fp32_bwd with --full)'
                                    if a.dtype == 'f32' else
                                    'bf16 activations + bf16 forward matrix instruction, fp32 gradients / weights') +
                                   ': fwd + SimOTA + losses + bwd + grad all-reduce + SGD, synthetic WIDER-Face-shaped '
                                   'batches; fp32 storage and accumulation everywhere, pointwise GEMMs on the matrix '
                                   'cores through bf16 splits (forward 3-way: 2.4e-7 of the exact fp32 instruction)',
                       'parallelism': f'dp{world}', 'global_batch': world * a.batch},
            'final_loss': round(last_loss, 4),
            # shader clock (sysfs pp_dpm_sclk) right before / right after the timed window: a 0.1 s window can sit on
            # the clock ramp
            'gpu_clock_mhz': {'before': clk0, 'after': clk1},
            'weights': (f'tests/golden/yunet_{a.kind}_synth_trained.pth + structured synthetic faces' if trained
                        else 'random init + noise images'),
            'per_rank_images_per_sec': [round(a.batch * a.steps / t, 1) for t in per_rank],
            'dist': {'backend': dist.get_backend() if world > 1 else None, 'world_size': world,
                     'collectives_per_step': 0 if world == 1 else 3,
                     # rank 0's events around the collectives (engine.comm_report): what the launch stream spends in /
                     # behind communication per step, and the bucket that runs under the early-stage backward kernels
                     'comm_ms_per_step': comm,
                     'note': 'num_pos (4 B) | gradient bucket A on a side stream under the backward '
                             'kernels of the early stages | bucket B + the 5 logged scalars'},
        }
    if world > 1 and a.full and os.environ.get('YUNET_BENCH_ONESHOT', '1') != '0':
        # The same window once more with the three collectives on the one-shot all-reduce over peer-mapped inboxes
        # (csrc/collective.hip), so that ONE multi-GPU run answers "RCCL or one-shot for bucket B / num_pos" (VERDICT r4
        # next 8).  `value` above stays the RCCL figure.  Guards: enable_oneshot() self-checks against the process
        # group (5 s time-out) and every rank agrees before anything is routed through it; the peer wait of the timed
        # steps is capped at 10 s; a watchdog prints the RCCL line and ends the process if this section stalls.
        import threading
        import yunet_amd._lib as L_
        done = threading.Event()

        def watchdog():
            if not done.wait(float(os.environ.get('YUNET_BENCH_ONESHOT_WATCHDOG_S', '90'))):
                if rank == 0:
                    res['dist']['oneshot'] = {'error': 'stalled: watchdog fired, RCCL result kept',
                                              'status': model.engine.oneshot_status()}
                    print(json.dumps(res), flush=True)
                os._exit(0)
        threading.Thread(target=watchdog, daemon=True).start()
        one = {}
        prev_to = L_.set_option('oneshot_timeout_ms', 10000)
        try:
            if model.engine.enable_oneshot(verify=True):
                for i in range(3):
                    step(i)
                torch.cuda.synchronize()
                dto, per_o, _, _, _, comm_o = window(a.steps)
                st = torch.tensor([model.engine.oneshot_status()], device=dev, dtype=torch.int32)
                dist.all_reduce(st, op=dist.ReduceOp.MAX)
                one = {'value': round(world * a.batch * a.steps / dto, 1), 'ms_per_step': round(1000.0 * dto / a.steps, 3),
                       'steps': a.steps, 'comm_ms_per_step': comm_o, 'status': int(st.item()),
                       'per_rank_images_per_sec': [round(a.batch * a.steps / t, 1) for t in per_o],
                       'what': 'same window, collectives through yunet_allreduce (peer-mapped inboxes over xGMI) '
                               'instead of RCCL; status 0 = no peer wait timed out'}
            else:
                one = {'error': 'self-check against the process group failed or set-up unavailable: stayed on RCCL'}
        except Exception as e:                # noqa: BLE001 -- a side measurement must not cost the headline line
            one = {'error': repr(e)[:300]}
        finally:
            L_.set_option('oneshot_timeout_ms', prev_to)
            try:
                model.engine.disable_oneshot()
            except Exception:                 # noqa: BLE001
                pass
            done.set()
        if rank == 0:
            res['dist']['oneshot'] = one
    if rank == 0 and world == 1 and a.full and not a.no_roofline:
        agg = profile_ops(model.engine)
        tot = sum(v['ms'] for v in agg.values())
        # The dominant kernel is chosen per __global__ FAMILY: one function split over template instances
        # (dp_bwd64_kernel<4,f,f> / <8,f,t> / <8,f,f> / <8,t,f>) is one kernel of the step
        fam = {}
        for kname, v in agg.items():
            f = fam.setdefault(family_of(kname), dict(launches=0, ms=0.0, bytes=0, flops=0, ref_bytes=0, instances={}, shapes={}))
            for k_ in ('launches', 'ms', 'bytes', 'flops', 'ref_bytes'):
                f[k_] += v[k_]
            f['instances'][kname] = v
            for shp, sv in v.get('shapes', {}).items():
                t_ = f['shapes'].setdefault(shp, dict(launches=0, ms=0.0, bytes=0))
                for k_ in ('launches', 'ms', 'bytes'):
                    t_[k_] += sv[k_]
        name, top = max(fam.items(), key=lambda kv: kv[1]['ms'])
        per_launch_ms = top['ms'] / top['launches']
        achieved = top['bytes'] / (top['ms'] * 1e-3) / 1e9          # the family's bytes / the family's time
        inst_launches = {k: v['launches'] for k, v in top['instances'].items()}
        traffic, traffic_src = pmc_traffic(inst_launches)
        committed = traffic
        per_inst_traffic = None
        if not a.no_live_traffic:
            live, per_inst_traffic = live_traffic(inst_launches, a)
            if live:
                traffic, traffic_src = live, 'live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this bench step'
        tflops = top['flops'] / (top['ms'] * 1e-3) / 1e12
        step_ms = 1000.0 * dt / a.steps
        ref_gbs = sum(v['ref_bytes'] for v in agg.values()) / (1e-3 * step_ms) / 1e9
        res['roofline'] = {
            'bound': 'hbm', 'achieved': round(achieved, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
            'frac': round(achieved / HBM_PEAK_GBS, 4), 'traffic': traffic, 'traffic_source': traffic_src,
            'traffic_committed_profile': committed,
            'kernel': name,
            'kernel_note': f'family of {len(top["instances"])} template instance(s) of one __global__ function; '
                           'achieved = algorithmic bytes of all its launches / their summed duration; traffic = PMC '
                           'bytes per launch averaged over the same launches',
            # the WHOLE step against the HBM peak: bytes of the reference's op graph (66.93 MB / image for
            # YuNet_n 320x320) x images/s / 8 TB/s
            'step_frac': round(ref_gbs / HBM_PEAK_GBS, 4),
            # ... without the gradient of the input image, which SURVEY's generic 2*in + out charges to the stem's
            # backward but no kernel (here or in the reference) writes
            'step_frac_written_grads': round((ref_gbs - a.batch * 3 * a.size * a.size * 4 / (1e-3 * step_ms) / 1e9)
                                             / HBM_PEAK_GBS, 4),
            # the same family's ALGORITHMIC fp32-equivalent GEMM FLOPs (dW1 and da; the recomputed forward GEMM is
            # not counted) against the exact-fp32 matrix ceiling (v_mfma_f32_16x16x4_f32: 256 CU x 4 SIMD x
            # 64 FLOP/clk x 2.4 GHz).  The split-bf16 instances EXECUTE 3 bf16 products per algorithmic product in
            # 3 GEMMs: `executed_bf16` prices those against the dense bf16 peak (= what MfmaUtil measures).
            'mfma': {'achieved': round(tflops, 1), 'peak': MFMA_F32_PEAK_TFLOPS, 'unit': 'TFLOP/s',
                     'frac': round(tflops / MFMA_F32_PEAK_TFLOPS, 4),
                     'what': 'algorithmic fp32-equivalent GEMM FLOPs vs the fp32 MFMA peak',
                     'executed_bf16': executed_bf16(name, tflops, a.dtype)},
            'launches_per_step': top['launches'], 'avg_launch_ms': round(per_launch_ms, 4),
            'ms_per_step': round(top['ms'], 4),
            # the template instances of the family (what the dispatcher picks per shape)
            'instances': {k: {'launches': v['launches'], 'ms': round(v['ms'], 4),
                              'frac': round(v['bytes'] / (v['ms'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                              'algorithmic_bytes_per_launch': v['bytes'] // v['launches'],
                              'traffic': (per_inst_traffic or {}).get(k)}
                          for k, v in sorted(top['instances'].items(), key=lambda kv: -kv[1]['ms'])},
            # ... and the family per feature-map size (the step average above mixes them)
            'by_shape': {k: {'launches': v['launches'], 'avg_launch_ms': round(v['ms'] / v['launches'], 4),
                             'frac': round(v['bytes'] / (v['ms'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
                         for k, v in top['shapes'].items()},
            'algorithmic_bytes_per_launch': top['bytes'] // top['launches'],
            'share_of_step': round(top['ms'] / tot, 3),
            # unit-boundary bytes of THIS plan (the two big pools are folded into their neighbours) ...
            'step_algorithmic_GBs': round(sum(v['bytes'] for v in agg.values()) / (1e-3 * step_ms) / 1e9, 1),
            # ... and of the reference's op graph at this rate (the numerator of step_frac)
            'step_reference_graph_GBs': round(ref_gbs, 1),
        }
        res['kernels'] = {k: {'launches': v['launches'], 'ms': round(v['ms'], 4),
                              'GBs': round(v['bytes'] / (v['ms'] * 1e-3) / 1e9, 1) if v['ms'] > 0 else 0,
                              'algorithmic_bytes_per_launch': v['bytes'] // max(1, v['launches'])}
                          for k, v in sorted(agg.items(), key=lambda kv: -kv[1]['ms'])}
        res['families'] = {k: {'launches': v['launches'], 'ms': round(v['ms'], 4),
                               'frac': round(v['bytes'] / (v['ms'] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if v['ms'] > 0 else 0}
                           for k, v in sorted(fam.items(), key=lambda kv: -kv[1]['ms'])[:8]}
    if rank == 0 and world == 1 and a.full and a.dtype == 'f32' and not a.no_exact_bwd:
        # the same step with the 64->64 backward GEMMs on the EXACT fp32 matrix instruction
        # (the dispatcher option "bwd_fp32mma", include/yunet_hip.h: yunet_set_option): the number the headline
        # would be without the split-bf16 gradient GEMMs
        L.set_option('bwd_fp32mma', 1)
        try:
            for i in range(3):
                step(i)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for i in range(a.steps):
                step(i)
            torch.cuda.synchronize()
            dte = time.perf_counter() - t1
        finally:
            L.set_option('bwd_fp32mma', 0)
        res['exact_fp32_bwd'] = {'ms_per_step': round(1000.0 * dte / a.steps, 3),
                                 'value': round(a.batch * a.steps / dte, 1), 'unit': 'images/sec',
                                 'what': 'same run, option bwd_fp32mma=1: every backward GEMM on v_mfma_f32_16x16x4_f32'}
    headline = (a.kind, a.size, a.batch, a.dtype, a.weights) == (KIND, H, BATCH, 'f32', 'trained')
    if rank == 0 and world == 1 and a.full and headline and not a.no_other_configs:
        # BASELINE.json configs[2] / [3] / [4] on one GPU, 50-step windows in this same process
        del wrapped, opt, pool
        model.engine.release() if hasattr(model.engine, 'release') else None
        del model
        torch.cuda.empty_cache()
        res['other_configs'] = {}
        for name, (k_, s_, b_, d_) in (('YuNet_n 320x320 bs=256, bf16 fwd / fp32 grads', ('n', 320, 256, 'bf16')),
                                       ('YuNet_n 640x640 bs=64, fp32', ('n', 640, 64, 'f32')),
                                       ('YuNet_s 320x320 bs=512, fp32', ('s', 320, 512, 'f32'))):
            try:
                res['other_configs'][name] = run_other_config(k_, s_, b_, d_, dev)
            except Exception as e:                           # a side measurement must not cost the headline line
                res['other_configs'][name] = {'error': repr(e)[:200]}
        model = wrapped = opt = pool = None
    if rank == 0 and world == 1 and a.full and not a.no_cpu_baseline:
        res['cpu_baseline'] = cpu_baseline(a.kind, a.size)
        if not a.no_gpu_eager:
            model = wrapped = opt = pool = None    # hand the GPU to the child process
            torch.cuda.empty_cache()
            res['cpu_baseline']['gpu_eager'] = gpu_eager(a.kind, a.size)
    if rank == 0:
        print(json.dumps(res))
    if world > 1:
        dist.barrier(**bar)
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
