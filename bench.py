#!/usr/bin/env python
"""bench.py -- MPix/s of the L3C encode hot path (net forward + fused logistic-mixture CDF head + HIP range coder) on
synthetic 768x512 RGB batches, BASELINE.json's metric.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--config headline|dataset|large|files] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

--config headline (default; BASELINE.json configs 2/3): one "step" = one pass of the hot path over one batch of B images per
GPU: the images are already resident in HBM when the timed region starts, and the step ends with every stream's bytes and
byte counts in HBM (file assembly / PCIe are not part of `value`).
--config dataset (config 4): a step = the rank's share of a set of 500 differently sized images (sizes drawn like the
reference's Open Images preprocessing), END TO END from host uint8 images to `.l3c` byte strings on the host.
--config large (config 5): RGB Shared baseline 0306_0002 (cr_rgb_shared.cf, auto_recurse 3, padding to 16): a step = forward +
bpsp of one 3000x2000 image (-> 4 auto-crops of 1500x1000) and one 2000x1500 image (not cropped: auto_crop.py:44-47).
Images shard with no data-path collective ("replicas only"): scaling is weak, `value` = all ranks'
pixels / max-over-ranks time.

`python bench.py --gpus N` without a launcher (no RANK in the environment) re-executes itself under torch.distributed.run with N
ranks, one per visible GPU (and fails loudly when fewer than N are visible): the driver's plain command works unattended.

A plain run sets up, warms up, times the K steps and prints the line; `--dump-outputs DIR` also writes what the last timed step
computed (headline: the `.l3c` files of the batch -- their sizes, image 0's file whole and a seeded sample of every file's bytes) as
DIR/<name>.npy.  The inputs are seeded: the same arguments give the same inputs in every run.

Prints ONE JSON line (rank 0).  Besides the contract fields it carries, with `--full` (headline config)
  roofline      dominant kernel = conv_wino4_kernel (Winograd F(4x4,3x3) on v_mfma_f32_16x16x4_f32): `achieved` = the FLOPs the
                matrix pipe EXECUTES (36/144 of the direct convolution's) summed over its launches in the timed region / their
                summed HIP-event durations; `peak` = 157.3 TFLOP/s dense fp32 MFMA at 2.4 GHz; the direct-convolution
                (algorithmic) rate, the HBM side of the same launches, and -- from profiles/r05_pmc_bench.json, PMC passes over THIS
                script reduced to the launches of its timed steps -- the measured HBM traffic per launch and the counter-based pipe
                occupancy ride along.  A PMC table whose launch population differs from this run's, or whose bytes are below the
                compulsory (algorithmic) bytes, is reported as `invalid`, never as `traffic`
  cpu_baseline  the oracle (or, where /root/reference exists, the reference itself) timed on this box's host cores
  parity        image 0 of the batch against the oracle: max |P - P_oracle| per scale (get_P on the oracle's bottlenecks),
                symbol flips, and the HIP `.l3c` file's size against the oracle's
  decode        the last batch decoded back from its files (outside the timed region), lossless check, batch-1 latency
  latency       ONE image: image in HBM -> .l3c bytes on the host -> pixels in HBM, seconds (the reference CLI's use case)
  ranks         world size, visible devices, rank -> device map, process-group backend, per-rank host budget
  worst_case_coder   the same step on the DEFAULT-init checkpoint (R and G streams at the 16-bit probability floor: 2.6x the bitstream
                volume of the calibrated checkpoint), a short untimed-region run: encode / decode MPix/s, bpsp
  configs       BASELINE.json configs 4 and 5 in reduced form (200 images of the dataset law; one step of the large-image RGB Shared
                workload), outside the timed region, so that the driver's default run observes them
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import l3c_pytorch_amd  # noqa: E402,F401

H, W = 512, 768
FP32_MFMA_PEAK_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense, 2.4 GHz
HBM_PEAK_GBS = 8000.0               # same guide: HBM3E, 8 TB/s
ALGO_FLOP_PER_PX = 1367796         # conv stack of the L3C forward, FLOP per image pixel
RGB_SHARED_FLOP_PER_PX = 869168    # RGB Shared with auto_recurse 3


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=None, help='ranks = GPUs (default: the launcher\'s WORLD_SIZE, else 1)')
    ap.add_argument('--steps', type=int, default=None)
    ap.add_argument('--warmup', type=int, default=None)
    ap.add_argument('--config', choices=('headline', 'dataset', 'large', 'files'), default='headline')
    ap.add_argument('--batch', type=int, default=128, help='headline: images per GPU per step')
    ap.add_argument('--checkpoint', choices=('calibrated', 'default'), default='calibrated',
                    help='synthetic checkpoint: calibrated = fitted probability heads (live model, ~6 bpsp); default = seeded default '
                         'init (R and G streams at the 16-bit probability floor: the coder\'s worst case, 16.2 bpsp)')
    ap.add_argument('--images', type=int, default=500, help='dataset: images in the set (all ranks together)')
    ap.add_argument('--max-batch', type=int, default=16, help='dataset: images of one padded shape per forward pass')
    ap.add_argument('--write-window', type=int, default=None, help='files: images the tester codes / decodes as one set (default 32 x max-batch)')
    ap.add_argument('--coder-cus', type=int, default=0, help='compute units reserved for the range coder (0 = share all CUs)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-parity', action='store_true')
    ap.add_argument('--no-decode', action='store_true', help='skip the (untimed-region) decode leg')
    ap.add_argument('--no-extra-legs', action='store_true', help='skip the worst_case_coder and configs legs of the headline line')
    ap.add_argument('--cpu-baseline-only', action='store_true',
                    help='no GPU: time the CPU path on this host (the real reference where /root/reference exists) and print it as JSON')
    ap.add_argument('--no-kernel-events', action='store_true', help='skip the per-launch HIP events of the roofline leg')
    ap.add_argument('--stub-step', action='store_true',
                    help='tests only: no GPU, gloo, a sleep instead of the hot path -- exercises the launch / barrier / max-over-ranks / JSON path')
    ap.add_argument('--full', action='store_true',
                    help='also run the secondary legs (headline: roofline HIP events, decode, latency, CPU baseline, parity, worst_case_coder '
                         'and configs; dataset: the set decode; files: the round trip).  Off: set-up, warm-up, the timed steps, the result line')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64, at most 64 MB)')
    a = ap.parse_args(argv)
    if a.gpus is None:      # under torch.distributed.run without --gpus: the launcher's world size is the truth
        a.gpus = int(os.environ.get('WORLD_SIZE', '1')) if 'RANK' in os.environ else 1
    defaults = {'headline': (6, 2), 'dataset': (3, 1), 'large': (4, 1), 'files': (2, 1)}[a.config]     # (dataset: three timed passes over the set, each reported)
    a.steps = defaults[0] if a.steps is None else a.steps
    a.warmup = defaults[1] if a.warmup is None else a.warmup
    return a


def build_path(ms_config='cr', coder_cus=0, calibrated=True):
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    from l3c_pytorch_amd.helpers import config_parser, synthetic
    cfg = config_parser.parse_builtin('ms', ms_config)
    sd = synthetic.make_state_dict(cfg, 0, calibrated=calibrated)
    bp = MultiscaleBlueprint(cfg)
    bp.net.load_state_dict(sd, strict=True)
    bp.set_eval()
    return cfg, sd, bp, Bitcoding(bp, coder_cus=coder_cus), synthetic


# ---- distributed plumbing (shared by every config and by the CPU stub the tests run) ----------------------------------------


def _compact_ranges(cpus):
    """[0, 1, 2, 3, 8, 9] -> '0-3,8-9' (None stays None)"""
    if not cpus:
        return None
    out, start, prev = [], None, None
    for c in sorted(cpus):
        if start is None:
            start = prev = c
        elif c == prev + 1:
            prev = c
        else:
            out.append((start, prev))
            start = prev = c
    out.append((start, prev))
    return ','.join(str(a) if a == b else '{}-{}'.format(a, b) for a, b in out)


def runtime_hw_queues():
    from l3c_pytorch_amd.helpers import runtime
    return runtime.hw_queues()


class Ranks(object):
    """One process per GPU under torch.distributed.run; RCCL ('nccl') for the barrier and the max-over-ranks time only."""

    def __init__(self, stub=False):
        self.world = int(os.environ.get('WORLD_SIZE', '1'))
        self.rank = int(os.environ.get('RANK', '0'))
        self.local_rank = int(os.environ.get('LOCAL_RANK', '0'))
        self.stub = stub
        self.device = None
        if not stub:
            if torch.cuda.device_count() <= self.local_rank:     # before any work: a rank without a GPU of its own must not run
                raise SystemExit('bench.py: rank {} (local rank {}) has no GPU: {} device(s) visible'.format(
                    self.rank, self.local_rank, torch.cuda.device_count()))
            torch.cuda.set_device(self.local_rank)
            self.device = torch.device('cuda', self.local_rank)
        # launched by torch.distributed.run (any world size, 1 included): a process group
        self.distributed = self.world > 1 or ('RANK' in os.environ and 'MASTER_PORT' in os.environ)
        if self.distributed:
            import torch.distributed as dist
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
            if stub:
                dist.init_process_group('gloo', rank=self.rank, world_size=self.world)
            else:
                dist.init_process_group('nccl', rank=self.rank, world_size=self.world, device_id=self.device)   # RCCL
            self.dist = dist

        # several ranks on ONE host: every rank takes its share of the host's threads / page-locked memory (helpers/sharding.host_budget)
        from l3c_pytorch_amd.helpers import sharding
        self.budget = sharding.host_budget(self.world)
        # ... and, with several ranks on the host, is pinned to the CPUs of its GPU's NUMA node before its worker threads and page-locked
        # staging buffers exist (they inherit the placement; helpers/runtime.py: sysfs numa_node of the device, else an even disjoint
        # slice of the allowed CPUs; never fatal).  A single rank stays unbound: its cpu_baseline leg wants every core.
        from l3c_pytorch_amd.helpers import runtime
        local_world = int(os.environ.get('LOCAL_WORLD_SIZE', self.world))
        if self.world > 1:
            self.affinity = runtime.bind_to_gpu_numa_node(self.local_rank, rank_in_node=self.local_rank, ranks_on_node=local_world)
            torch.set_num_threads(max(1, min(self.budget['torch_threads'], self.affinity['n_cpus'] or self.budget['torch_threads'])))
        else:
            self.affinity = {'cpus': None, 'numa_node': runtime.gpu_numa_node(self.local_rank) if not stub else None, 'bound': False,
                             'n_cpus': None, 'source': 'unbound (single rank)'}
        self._desc = self._describe()       # (a collective: every rank, here; rank 0 prints it)

    def describe(self):
        return self._desc

    def _describe(self):
        """what a SCALE record needs to show that N ranks really ran on N devices: visible devices, the rank -> device map, the
        process-group backend, the per-rank host budget"""
        devs = [self.local_rank if not self.stub else None]
        aff = {k: self.affinity.get(k) for k in ('numa_node', 'n_cpus', 'bound', 'source')}
        aff['cpus'] = _compact_ranges(self.affinity.get('cpus'))
        affs = [dict(aff, rank=self.rank)]
        if self.distributed:
            got = [None] * self.world
            self.dist.all_gather_object(got, (self.rank, self.local_rank if not self.stub else None, dict(aff, rank=self.rank)))
            devs = [d for _, d, _ in sorted(got, key=lambda g: g[0])]
            affs = [a for _, _, a in sorted(got, key=lambda g: g[0])]
        return {'world_size': self.world, 'visible_devices': 0 if self.stub else torch.cuda.device_count(), 'rank_to_device': devs,
                'backend': (self.dist.get_backend() if self.distributed else None), 'host_budget_per_rank': self.budget,
                'cpu_affinity': affs, 'hip_hw_queues': runtime_hw_queues()}

    def sync(self):
        if not self.stub:
            torch.cuda.synchronize()

    def barrier(self):
        self.sync()
        if self.distributed:
            self.dist.barrier()
        self.sync()

    def max_over_ranks(self, seconds):
        if not self.distributed:
            return seconds
        t = torch.tensor([seconds], dtype=torch.float64, device=self.device if not self.stub else 'cpu')
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def sum_over_ranks(self, values):
        if not self.distributed:
            return list(values)
        t = torch.tensor(list(values), dtype=torch.float64, device=self.device if not self.stub else 'cpu')
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return [float(v) for v in t.tolist()]

    def close(self):
        if self.distributed:
            self.dist.barrier()
            self.dist.destroy_process_group()


def timed(ranks, step, steps, warmup, before_timed=None):
    """W untimed steps, then exactly K steps between barriers; -> (max-over-ranks seconds, last step's result)."""
    res = None
    for _ in range(warmup):
        res = step()
    ranks.barrier()
    if before_timed:
        before_timed()
    t0 = time.perf_counter()
    for _ in range(steps):
        res = step()
    ranks.barrier()
    return ranks.max_over_ranks(time.perf_counter() - t0), res


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(args, ranks, arrays):
    """--dump-outputs DIR: every array as DIR/<name>.npy (float64 where the values are sizes or figures, float32 for bytes); with several
    ranks every rank writes its own, prefixed rank<r>_."""
    import numpy as np
    if not args.dump_outputs:
        return
    out = {(name if ranks.world == 1 else 'rank{}_{}'.format(ranks.rank, name)): a for name, a in arrays.items()}
    total = sum(a.nbytes for a in out.values())
    assert all(a.dtype in (np.float32, np.float64) for a in out.values()) and total <= DUMP_LIMIT_BYTES, total
    os.makedirs(args.dump_outputs, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(args.dump_outputs, name + '.npy'), a)


def file_arrays(files, sample_bytes=48 << 20):
    """`.l3c` byte strings -> their sizes, the first file whole and a seeded sample of every file's bytes (the same 0..1 positions
    of every file, scaled to its length), all within `sample_bytes` of float32."""
    import numpy as np
    sizes = np.array([len(f) for f in files], dtype=np.float64)
    first = np.frombuffer(files[0], dtype=np.uint8).astype(np.float32)
    k = max(1, min(16384, (sample_bytes - first.nbytes) // 4 // max(1, len(files))))
    u = np.random.RandomState(0).random_sample(k)
    sample = np.stack([np.frombuffer(f, dtype=np.uint8)[(u * len(f)).astype(np.int64)] for f in files]).astype(np.float32)
    return {'file_sizes': sizes, 'file0_bytes': first, 'file_bytes_sample': sample}


def contract(args, ranks, value, elapsed, **extra):
    d = {'metric': 'MPix/s encode (net+CDF+AC) on 768x512 RGB', 'value': round(value, 3), 'unit': 'MPix/s',
         'n_gpus': ranks.world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(elapsed / args.steps * 1e3, 3),
         'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
         'ranks': ranks.describe()}
    d.update(extra)
    return d


# ---- headline: batches of 768x512 ------------------------------------------------------------------------------------------------


PMC_TABLE = os.path.join('profiles', 'r06_pmc_bench.json')


def load_json(rel):
    try:
        with open(os.path.join(ROOT, rel)) as f:
            return json.load(f)
    except (OSError, ValueError):
        return None


def csrc_stamp():
    """sha256 over the kernel sources (csrc/*.hip, *.h, the public header), first 16 hex digits: profiles taken on other kernels
    are recognisably stale (there is no .git on the GPU box to ask)."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, 'l3c-pytorch_amd', 'csrc')
    files = sorted(f for f in os.listdir(csrc) if f.endswith(('.hip', '.h'))) + [os.path.join('..', '..', 'include', 'l3c_hip.h')]
    for f in files:
        with open(os.path.join(csrc, f), 'rb') as fh:
            h.update(f.encode() + b'\0' + fh.read())
    return h.hexdigest()[:16]


def csrc_file_stamps():
    """Per source file of csrc_stamp(): sha256, first 16 hex digits."""
    import hashlib
    csrc = os.path.join(ROOT, 'l3c-pytorch_amd', 'csrc')
    files = sorted(f for f in os.listdir(csrc) if f.endswith(('.hip', '.h'))) + [os.path.join('..', '..', 'include', 'l3c_hip.h')]
    out = {}
    for f in files:
        with open(os.path.join(csrc, f), 'rb') as fh:
            out[f] = hashlib.sha256(fh.read()).hexdigest()[:16]
    return out


# the sources that define the kernels `roofline` takes counters for from the PMC table: the MFMA convolutions (conv_wino4_kernel incl. its
# polyphase launches, the pointwise kernels) and, for `decode_kernels`, the range decoders and the table kernel
ROOFLINE_KERNEL_SOURCES = ('conv_wino4.hip', 'conv_pw.hip', 'conv_mfma.hip', 'l3c_common.h', 'ac_kernels.hip', 'ac_core.h', 'dmll_kernels.hip',
                           'dmll_core.h', os.path.join('..', '..', 'include', 'l3c_hip.h'))


def load_pmc_table():
    """profiles/r06_pmc_bench.json: per-launch HBM bytes (FETCH_SIZE, WRITE_SIZE passes) and SQ/GRBM counters of a rocprofv3
    --pmc run of THIS script, reduced by tools/pmc_bench.py and stamped with csrc_stamp() of the sources it was taken on.
    -> (table or None, 'current' | 'stale' | 'absent')."""
    try:
        with open(os.path.join(ROOT, PMC_TABLE)) as f:
            t = json.load(f)
    except (OSError, ValueError):
        return None, 'absent'
    if t.get('csrc_stamp') == csrc_stamp():
        return t, 'current'
    # other sources changed since the passes: the table still describes the kernels `roofline` reads from it when every source that defines
    # THEM is byte-identical to the one the passes ran on (the table's per-file stamps); what changed is listed in the line
    then, now = t.get('csrc_files') or {}, csrc_file_stamps()
    if then and all(then.get(f) == now.get(f) for f in ROOFLINE_KERNEL_SOURCES):
        t['_changed_since'] = sorted(f for f in set(then) | set(now) if then.get(f) != now.get(f))
        return t, 'current'
    return t, 'stale'


def roofline_leg(records, args, elapsed):
    by, by_var = {}, {}
    for rec in records:
        key, flops, nbytes, e0, e1 = rec[:5]
        dt = e0.elapsed_time(e1) * 1e-3
        d = by.setdefault(key, [0.0, 0.0, 0, 0.0])
        d[0] += flops
        d[1] += dt
        d[2] += 1
        d[3] += nbytes
        if len(rec) > 5 and rec[5]:
            v = by_var.setdefault(key, {}).setdefault(rec[5], [0.0, 0.0, 0, 0.0])
            v[0] += flops
            v[1] += dt
            v[2] += 1
            v[3] += nbytes
    dom = max(by, key=lambda k: by[k][1])
    flops, secs, n, nbytes = by[dom]
    all_f = sum(v[0] for v in by.values())
    all_s = sum(v[1] for v in by.values())
    # Winograd F(2x2,3x3) executes 16 multiplications per 2x2 output tile and channel pair where the direct form needs 36;
    # F(4x4,3x3) 36 per 4x4 tile where the direct form needs 144
    executed = 0.25 if dom.startswith('conv_wino4') else 16.0 / 36.0 if dom.startswith('conv_wino') else 1.0
    ach = flops * executed / secs / 1e12
    roof = {'bound': 'mfma', 'kernel': dom, 'achieved': round(ach, 2), 'peak': FP32_MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s',
            'frac': round(ach / FP32_MFMA_PEAK_TFLOPS, 4),
            'note': ('achieved = FLOPs the matrix pipe executes (Winograd {}: {} of the direct convolution\'s) / HIP-event time '
                     'of the launches in the timed region; peak = dense fp32 MFMA at 2.4 GHz'.format(
                         'F(4x4,3x3)' if executed == 0.25 else 'F(2x2,3x3)', '36/144' if executed == 0.25 else '16/36') if executed < 1 else
                     'implicit GEMM: algorithmic = executed FLOPs'),
            'algorithmic_tflops': round(flops / secs / 1e12, 2), 'algorithmic_frac': round(flops / secs / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4),
            'launches': n, 'avg_launch_us': round(secs / n * 1e6, 2), 'algorithmic_gflop_per_launch': round(flops / n / 1e9, 3),
            'algorithmic_bytes_per_launch': int(nbytes / n), 'traffic': None,
            'all_mfma_convs': {'algorithmic_tflops': round(all_f / all_s / 1e12, 2), 'seconds_per_step': round(all_s / args.steps, 5),
                               'share_of_step': round(all_s / elapsed, 3)},
            'per_kernel': {k: {'algorithmic_tflops': round(v[0] / v[1] / 1e12, 1), 'share_of_step': round(v[1] / elapsed, 3),
                               'launches_per_step': v[2] // args.steps, 'algorithmic_gb_per_launch': round(v[3] / v[2] / 1e9, 3)}
                           for k, v in sorted(by.items())}}
    names = {'false,false,false,false': 'plain (heads, dilated classifier branches)', 'true,false,false,false': 'ReLU', 'false,true,false,false': 'residual',
             'false,false,true,false': 'PixelShuffle tail'}
    for k, vs in by_var.items():
        roof['per_kernel'][k]['per_variant'] = {v: {'what': names.get(v, v), 'launches_per_step': x[2] // args.steps, 'avg_launch_us': round(x[1] / x[2] * 1e6, 1),
                                                     'algorithmic_gb_per_launch': round(x[3] / x[2] / 1e9, 3), 'algorithmic_tflops': round(x[0] / x[1] / 1e12, 1)}
                                                 for v, x in sorted(vs.items())}
    # the other side of the roofline: since F(4x4,3x3) the kernel sits at the ridge -- its algorithmic HBM bytes at the
    # HBM peak take about as long as its executed FLOPs at the MFMA peak, and the measured time is close to the SUM of the two
    hbm_s, mfma_s = nbytes / n / (HBM_PEAK_GBS * 1e9), flops * executed / n / (FP32_MFMA_PEAK_TFLOPS * 1e12)
    roof['hbm_side'] = {'algorithmic_gb_per_s': round(nbytes / secs / 1e9, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                        'frac': round(nbytes / secs / 1e9 / HBM_PEAK_GBS, 4),
                        'launch_time_at_hbm_peak_us': round(hbm_s * 1e6, 1), 'launch_time_at_mfma_peak_us': round(mfma_s * 1e6, 1),
                        'frac_of_the_larger_bound': round(max(hbm_s, mfma_s) / (secs / n), 4)}
    pmc, state = load_pmc_table()
    roof['pmc_table'] = {'file': PMC_TABLE, 'state': state, 'csrc_stamp': csrc_stamp()}
    if pmc and pmc.get('_changed_since'):
        roof['pmc_table']['sources_changed_since_the_passes'] = pmc['_changed_since']
        roof['pmc_table']['note'] = ('the sources of every kernel read from the table ({}) are byte-identical to those the passes ran on; entries of '
                                     'the table for kernels of the changed sources are not used'.format(', '.join(os.path.basename(f) for f in ROOFLINE_KERNEL_SOURCES)))
    if pmc and state == 'current' and pmc.get('batch') == args.batch:    # counters taken on OTHER kernel sources are not reported
        # Counter evidence must describe the SAME launch population as the algorithmic bytes (round-3 verdict: the round-3 table mixed
        # in the decode leg's batch-1 launches and showed the 1x1 kernel BELOW its compulsory bytes): per kernel the table must hold
        # exactly (its steps) x (this run's launches per step) launches, its average duration must agree with the HIP events, and its
        # bytes must not be below the compulsory (algorithmic) bytes.  Anything else is reported as invalid, not as traffic.
        checks = {}
        for kk, vv in pmc.get('kernels', {}).items():
            if kk not in roof['per_kernel'] or 'hbm_bytes_per_launch' not in vv:
                continue
            mine = roof['per_kernel'][kk]
            algo = mine['algorithmic_gb_per_launch'] * 1e9
            c = {'launches_match': vv.get('launches_per_step') == mine['launches_per_step'],
                 'not_below_compulsory': vv['hbm_bytes_per_launch'] >= 0.98 * algo,
                 'pmc_over_algorithmic': round(vv['hbm_bytes_per_launch'] / algo, 3)}
            ev_us = by[kk][1] / by[kk][2] * 1e6
            if 'avg_launch_us_profiled' in vv:
                c['pmc_over_event_duration'] = round(vv['avg_launch_us_profiled'] / ev_us, 3)
            checks[kk] = c
            if c['launches_match'] and c['not_below_compulsory']:
                mine['pmc_hbm_gb_per_launch'] = round(vv['hbm_bytes_per_launch'] / 1e9, 3)
                if 'per_variant' in vv:
                    mine['pmc_hbm_gb_per_launch_by_variant'] = {v: round(x['hbm_bytes_per_launch'] / 1e9, 3) for v, x in vv['per_variant'].items()}
                    for v, x in vv['per_variant'].items():      # beside each variant's ALGORITHMIC bytes (round-5 verdict: "the plain variant moves 13.8 GB -- what is its algorithmic figure?")
                        if v in mine.get('per_variant', {}):
                            mine['per_variant'][v]['pmc_hbm_gb_per_launch'] = round(x['hbm_bytes_per_launch'] / 1e9, 3)
                            mine['per_variant'][v]['pmc_over_algorithmic'] = round(x['hbm_bytes_per_launch'] / 1e9 / mine['per_variant'][v]['algorithmic_gb_per_launch'], 3)
        roof['pmc_table']['checks'] = checks
        k, c = pmc.get('kernels', {}).get(dom), checks.get(dom)
        if k and c and c['launches_match'] and c['not_below_compulsory']:
            roof['traffic'] = int(k['hbm_bytes_per_launch'])
            roof['traffic_note'] = ('PMC, rocprofv3 passes over this script with --no-decode ({}, same kernel sources): FETCH_SIZE (x2, gfx950) + '
                                    'WRITE_SIZE per launch over exactly the launches of {} timed steps ({} per step); = {:.3f} x the algorithmic '
                                    'bytes'.format(PMC_TABLE, pmc.get('steps'), k.get('launches_per_step'), k['hbm_bytes_per_launch'] / (nbytes / n)))
            for name in ('mfma_busy_frac', 'effective_clock_ghz'):
                if name in k:
                    roof['pmc_' + name] = k[name]
        elif k:
            roof['pmc_table']['state'] = 'invalid'
        if pmc.get('decode_kernels'):
            roof['decode_kernels'] = pmc['decode_kernels']
    return roof


def parity_leg(bp, bc, imgs, enc, sd, oracle_file):
    """Image 0 of the batch against the oracle (the checker): P through get_P on the oracle's bottlenecks, symbols of the
    forward pass, the share of RGB symbols coded at the probability floor, and the size of its `.l3c` file against the oracle's
    (when the CPU baseline leg produced one).  P is gated per parameter group like the tests (tests/parity_gate.py)."""
    from oracle import net as onet
    from l3c_pytorch_amd import ops
    img0 = imgs[0:1]
    with torch.no_grad():
        ref = onet.forward(img0.float().cpu(), sd)
    out = bp.net(img0.float())
    res = {'image': 0, 'max_abs_P': [], 'max_rel_P': [], 'max_value_P': [], 'P_groups': [],
           'symbol_flips': sum(int((out.S[s + 1].cpu() != ref.S[s + 1]).sum()) for s in range(3)),
           'bottleneck_levels_used': [int(torch.unique(out.S[s + 1]).numel()) for s in range(3)]}
    f_prev = None
    groups_ok = True
    # the accuracy gate (round 5; tests/parity_gate.py, tools/parity_truth.py): P against the oracle's decoder chain evaluated in DOUBLE
    # on the same bottlenecks -- flat 1e-5 for every group whose values stay below 16, 1e-6 relative above (the RGB means); the fp32
    # oracle's own distance from fp64 rides along, so the line says which side of |HIP - oracle| is the inaccurate one
    sd64 = {k: v.double() for k, v in sd.items()}
    P64, f64 = [None] * 3, None
    with torch.no_grad():
        for s in (2, 1, 0):
            P64[s], f64 = onet.get_P(s, ref.bn[s + 1].double(), f64, sd64)
    res['P_groups_vs_fp64'] = []
    for s in (2, 1, 0):
        P, f_prev = bp.net.get_P(s, ref.bn[s + 1].cuda(), f_prev)
        Pd, Rd = P.cpu().double(), ref.P[s].double()
        d = (Pd - Rd).abs().max()
        res['max_abs_P'].insert(0, float(d))
        res['max_rel_P'].insert(0, float(d / Rd.abs().max()))
        res['max_value_P'].insert(0, float(ref.P[s].abs().max()))
        # per parameter group (channel index = p * C * K + ...; 4 groups on the RGB scale, 3 on the bottleneck scales): the gate of
        # tests/parity_gate.py, restated -- |diff| < 1e-5 x max(1, largest |value| of the group / 4): absolute 1e-5 up to 4, 2.5e-6 relative above
        names = ('logit_pi', 'mu', 'log_sigma', 'lambda')[:4 if s == 0 else 3]
        n = Pd.shape[1] // len(names)
        g = {}
        for p, name in enumerate(names):
            da = float((Pd[:, p * n:(p + 1) * n] - Rd[:, p * n:(p + 1) * n]).abs().max())
            mv = float(Rd[:, p * n:(p + 1) * n].abs().max())
            tol = 1e-5 * max(1.0, mv / 4.0)
            ok = da < tol
            g[name] = {'max_abs': da, 'max_value': mv, 'tolerance': tol, 'ulp_of_max_value': round(da / (2.0 ** (math.floor(math.log2(max(mv, 1e-30))) - 23)), 1), 'ok': ok}
            groups_ok = groups_ok and ok
        res['P_groups'].insert(0, g)
        t = {}
        for p, name in enumerate(names):
            sl = slice(p * n, (p + 1) * n)
            mv = float(P64[s][:, sl].abs().max())
            tol = 1e-5 if mv <= 16.0 else 1e-6 * mv
            dh = float((Pd[:, sl] - P64[s][:, sl]).abs().max())
            t[name] = {'hip_vs_fp64': dh, 'oracle_vs_fp64': float((Rd[:, sl] - P64[s][:, sl]).abs().max()), 'max_value': mv, 'tolerance': tol, 'ok': dh < tol}
            groups_ok = groups_ok and t[name]['ok']
        res['P_groups_vs_fp64'].insert(0, t)
    # share of the RGB symbols the coder sees with a width-1 interval (c_high == c_low + 1: only the `+ l` guard term is left
    # of the probability; a default-init checkpoint has 100 % on R and G), from the HIP head's own uint16 tables
    dm = bp.losses.loss_dmol_rgb
    K = bp.net.config_ms.prob.K
    sym = out.raw.sym[0]
    floor = []
    for c in range(3):
        t = ops.dmll_cdf_table(out.raw.P[0], sym, bc._targets(dm), 3, K, True, c, 0, H * W)[0].view(-1, dm.L + 1).to(torch.int32) & 0xFFFF
        s_c = sym[0, c].reshape(-1).long()
        lo = t.gather(1, s_c[:, None])[:, 0]
        hi = torch.where(s_c == dm.L - 1, torch.full_like(lo, 65536), t.gather(1, (s_c + 1).clamp(max=dm.L)[:, None])[:, 0])
        floor.append(round(float((hi - lo == 1).float().mean()), 5))
    res['rgb_symbols_at_probability_floor'] = floor
    hip_file = enc.to_bytes()[0]
    res['hip_bytes'] = len(hip_file)
    size_ok = True
    if oracle_file is not None:
        res['oracle_bytes'] = len(oracle_file)
        res['size_delta'] = len(hip_file) - len(oracle_file)
        res['framing_equal'] = hip_file[:13] == oracle_file[:13]
        size_ok = abs(res['size_delta']) <= 64 + 1e-4 * len(oracle_file)
    res['tolerance'] = ('per parameter group of P (logit pi / mu / log sigma / lambda): |P - P_fp64| < 1e-5 flat for groups with values up to 16, 1e-6 relative '
                        'above (P_fp64: the oracle\'s decoder chain in double on the same bottlenecks); consistency with the fp32 oracle: |P - P_oracle| < '
                        '1e-5 x max(1, largest |value| of the group / 4); file within 64 B + 1e-4 of the oracle\'s')
    res['ok'] = bool(groups_ok and size_ok)
    return res


def decode_leg(bc, enc, imgs, compute_stream):
    """Secondary figure (SURVEY.md section 8d "also decode MPix/s"), outside the timed region: decode the last coded batch
    back from its `.l3c` byte strings (host) to pixels in HBM and check it is lossless; plus the latency of one image."""
    SYMBOLS_PER_PX = 4.640625           # 3 P0 + 5 (P1 + P2 + P3) symbols per image pixel, SURVEY.md section 8d
    with torch.cuda.stream(compute_stream):
        files = enc.to_bytes()
        # the first call of the process also pays the allocator's first touch and the code objects' load: reported, not the figure
        times, lossless = [], True
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec, _ = bc.decode_batch(files)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            lossless = lossless and bool(torch.equal(dec.to(torch.uint8), imgs.to(torch.uint8)))
            del dec
        dt_first, dt = times[0], sorted(times[1:])[1]
        bc.decode_batch(files[:1])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec1, _ = bc.decode_batch(files[:1])
        torch.cuda.synchronize()
        dt1 = time.perf_counter() - t0
        lossless = lossless and bool(torch.equal(dec1.to(torch.uint8), imgs[:1].to(torch.uint8)))
    B = len(files)
    return {'value': round(B * H * W / 1e6 / dt, 3), 'unit': 'MPix/s', 'batch': B, 'seconds': round(dt, 3),
            'seconds_all_calls': [round(t, 3) for t in times], 'first_call_seconds': round(dt_first, 3),
            'timing': 'median of three calls after the first one of the process', 'lossless': lossless, 'msym_per_s_aggregate': round(B * H * W * SYMBOLS_PER_PX / 1e6 / dt, 1),
            'longest_chain_symbols': H * W, 'batch1_seconds': round(dt1, 4), 'batch1_mpix_per_s': round(H * W / 1e6 / dt1, 3),
            'batch1_ns_per_symbol_upper_bound': round(dt1 / (H * W) * 1e9 / 1.0625, 1),
            'note': 'host .l3c bytes -> pixels in HBM; latency-bound: serial chains of {} symbols per RGB channel, the three '
                    'channels pipelined a chunk of pixels apart (34 chunk steps for 32 chunks: x 1.0625, two 1024-symbol probe chunks in front); the upper bound charges the whole '
                    'one-image decode -- get_P convolutions, bottleneck scales, tables -- to the RGB chain'.format(H * W)}


def latency_leg(bp, bc, img1, compute_stream, reps=5):
    """The reference's actual CLI use case (l3c.py enc / dec of ONE image): seconds from the image in HBM to its `.l3c` bytes on the
    host, and from those bytes back to pixels in HBM; median of `reps` after a warm-up, outside the timed region."""
    import statistics
    enc_s, dec_s = [], []
    with torch.cuda.stream(compute_stream):
        for k in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            data = bc.encode_batch(img1, out=bp.net(img1)).to_bytes()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            dec, _ = bc.decode_batch(data)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if k:
                enc_s.append(t1 - t0)
                dec_s.append(t2 - t1)
        lossless = bool(torch.equal(dec.to(torch.uint8), img1.to(torch.uint8)))
    e, d = statistics.median(enc_s), statistics.median(dec_s)
    return {'image': '768x512', 'encode_seconds': round(e, 5), 'decode_seconds': round(d, 5), 'encode_mpix_per_s': round(H * W / 1e6 / e, 2),
            'decode_mpix_per_s': round(H * W / 1e6 / d, 2), 'decode_ns_per_symbol_upper_bound': round(d / (H * W) * 1e9 / 1.0625, 1),
            'file_bytes': len(data[0]), 'lossless': lossless, 'reps': reps,
            'note': 'one image: image in HBM -> .l3c bytes on the host -> pixels in HBM (median); the serial interval recurrence of the '
                    'three 393 216-symbol RGB streams sets the encode time, the symbol-by-symbol decode chains the decode time'}


def run_headline(args, ranks):
    cfg, sd, bp, bc, synthetic = build_path('cr', args.coder_cus, args.checkpoint == 'calibrated')
    from l3c_pytorch_amd import _lib, ops
    B = args.batch
    # synthetic images (seed = global image index), resident in HBM before the timed region; each image is made from its own seed,
    # so making them on worker threads gives the same batch
    import concurrent.futures
    with single_thread():
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            imgs = list(pool.map(lambda i: synthetic.make_image(H, W, ranks.rank * B + i, 'natural'), range(B)))
        imgs = torch.stack(imgs).to(ranks.device)
    imgs_f = imgs.float().contiguous()
    torch.cuda.synchronize()
    compute_stream = bc.compute_stream if bc.compute_stream is not None else torch.cuda.current_stream()

    def step():
        with torch.cuda.stream(compute_stream):
            out = bp.net(imgs_f)
            return bc.encode_batch(imgs_f, out=out)

    want_events = args.full and ranks.rank == 0 and not args.no_kernel_events

    def arm():
        ops.PROFILE = [] if want_events else None

    elapsed, enc = timed(ranks, step, args.steps, args.warmup, before_timed=arm)
    records, ops.PROFILE = ops.PROFILE, None
    value = ranks.world * B * args.steps * H * W / 1e6 / elapsed

    with torch.cuda.stream(compute_stream):
        sizes = enc.file_sizes().cpu().numpy()
        if args.dump_outputs:
            dump_outputs(args, ranks, file_arrays(enc.to_bytes()))
    bits, subpx = ranks.sum_over_ranks([float(sizes.sum()) * 8, B * 3 * H * W])
    result = None
    if ranks.rank == 0:
        roofline = roofline_leg(records, args, elapsed) if records else None
        decode = decode_leg(bc, enc, imgs, compute_stream) if args.full and ranks.world == 1 and not args.no_decode else None
        cpu, oracle_file = None, None
        if args.full and ranks.world == 1 and not args.no_cpu_baseline:
            from oracle import cpu_baseline
            cpu, oracle_file = cpu_baseline.run(sd, imgs[0].cpu())
            elsewhere = (load_json(os.path.join('profiles', 'r04_cpu_reference_build_container_{}.json'.format(args.checkpoint))) or
                         load_json(os.path.join('profiles', 'r03_cpu_reference_build_container_{}.json'.format(args.checkpoint))))
            if elsewhere:     # the UNMODIFIED reference timed where /root/reference exists (python bench.py --cpu-baseline-only)
                cpu['reference_measured_elsewhere'] = elsewhere
        parity = None
        if args.full and ranks.world == 1 and not args.no_parity:
            with torch.cuda.stream(compute_stream):
                parity = parity_leg(bp, bc, imgs_f, bc.encode_batch(imgs_f[0:1]), sd, oracle_file)
        latency = None
        if args.full and ranks.world == 1 and not args.no_decode:
            latency = latency_leg(bp, bc, imgs_f[0:1].contiguous(), compute_stream)
        name, ncu, arch = _lib.device_info()
        peak_gb = round(torch.cuda.max_memory_allocated() / 1e9, 1)
        extra = {}
        if args.full and ranks.world == 1 and not args.no_extra_legs:
            del enc
            torch.cuda.empty_cache()
            extra = extra_legs(args)
        result = contract(
            args, ranks, value, elapsed,
            config={'workload': 'L3C 0306_0001 (cr.cf, synthetic seeded checkpoint), batch of 768x512 synthetic RGB per GPU: net forward + '
                                'fused logistic-mixture CDF head + HIP range coder -> bytes in HBM',
                    'checkpoint': args.checkpoint, 'batch_per_gpu': B, 'image': '768x512', 'coder_cus': args.coder_cus, 'sharding': 'images, replicas only (no collective)'},
            bpsp=round(bits / subpx, 4), flop_per_px=ALGO_FLOP_PER_PX,
            end_to_end_algorithmic_tflops=round(value * 1e6 * ALGO_FLOP_PER_PX / 1e12 / ranks.world, 2),
            device='{} ({}, {} CUs)'.format(name, arch, ncu), peak_hbm_gb=peak_gb,
            roofline=roofline, cpu_baseline=cpu, parity=parity, decode=decode, latency=latency, **extra)
    return result


def _sub_bench(extra_args, timeout=600):
    """Run this script once more in a process of its own (own HIP start-up environment, own memory) and return its JSON line."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), '--gpus', '1', '--full', '--no-extra-legs'] + extra_args
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    try:
        p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
        lines = [l for l in p.stdout.decode().splitlines() if l.startswith('{')]
        if p.returncode != 0 or not lines:
            return {'error': 'rc {}: {}'.format(p.returncode, p.stderr.decode()[-300:])}
        return json.loads(lines[-1])
    except subprocess.TimeoutExpired:
        return {'error': 'timeout after {} s'.format(timeout)}


def extra_legs(args):
    """Secondary records of the default line, each measured by a run of this script in a process of its own, OUTSIDE the timed
    region of the headline: the worst case for the coder (default-init checkpoint), and BASELINE.json configs 4 and 5 in reduced
    form."""
    def pick(d, keys):
        return {k: d[k] for k in keys if k in d} if 'error' not in d else d

    wc = _sub_bench(['--checkpoint', 'default', '--batch', str(args.batch), '--steps', '3', '--warmup', '1', '--no-cpu-baseline',
                     '--no-parity', '--no-kernel-events'])
    worst = pick(wc, ('value', 'unit', 'ms_per_step', 'bpsp', 'steps'))
    if 'decode' in wc and wc['decode']:
        worst['decode'] = {k: wc['decode'][k] for k in ('value', 'unit', 'seconds', 'lossless', 'batch1_seconds')}
    worst['note'] = ('default-init checkpoint: mixtures near 0 for pixels in 0..255, the R and G streams sit at the 16-bit probability '
                     'floor -- 2.6x the calibrated checkpoint\'s bitstream volume, ~6x a trained model\'s')
    ds = _sub_bench(['--config', 'dataset', '--images', '200', '--steps', '3', '--warmup', '1', '--checkpoint', args.checkpoint])
    lg = _sub_bench(['--config', 'large', '--steps', '4', '--warmup', '1', '--checkpoint', args.checkpoint])
    fl = _sub_bench(['--config', 'files', '--images', '200', '--steps', '1', '--warmup', '1', '--checkpoint', args.checkpoint])
    keys = ('metric', 'value', 'unit', 'ms_per_step', 'steps', 'warmup', 'bpsp', 'megapixels', 'decode', 'per_step', 'config')
    return {'worst_case_coder': worst,
            'configs': {'dataset': dict(pick(ds, keys), reduced='200 of the 500 images of BASELINE.json config 4 (python bench.py --config dataset runs all 500; the fill and drain of the host pipeline weigh more on the shorter set)'),
                        'large': dict(pick(lg, keys), reduced='4 steps of BASELINE.json config 5 (python bench.py --config large)'),
                        # the reference's own benchmark loop, FILE TO FILE (round-5 verdict, next 6): PNG files on disk -> .l3c files on disk -> decoded and compared
                        'files': dict(pick(fl, keys + ('encode', 'round_trip')), reduced='200 of the 500 images, one timed pass after one warm-up pass (python bench.py --config files runs all 500)')}}


# ---- dataset: 500 differently sized images, end to end from host images to host files ---------------------------------------------


def run_dataset(args, ranks):
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')       # (read at HIP start-up; set by main() before the first HIP call)
    cfg, sd, bp, bc, synthetic = build_path('cr', args.coder_cus, args.checkpoint == 'calibrated')
    from l3c_pytorch_amd import _lib
    from l3c_pytorch_amd.helpers import dataset_codec, pad, sharding
    sizes = dataset_codec.draw_sizes(args.images)
    # largest-first greedy assignment on pixel counts (image areas differ 4x: round robin leaves the slowest of 8 ranks 10 % above the mean)
    mine = sharding.shard_balanced([h * w for h, w in sizes], ranks.rank, ranks.world)
    with single_thread():
        imgs = {i: synthetic.make_image(sizes[i][0], sizes[i][1], i, 'natural') for i in mine}     # host uint8

    step_seconds = []          # every step ends with its files on the host: its wall time is a measurement of its own

    def step():
        t0 = time.perf_counter()
        r = dataset_codec.encode_set(bc, imgs, mine, max_batch=args.max_batch, n_pinned=ranks.budget['pinned_buffers'])
        step_seconds.append(time.perf_counter() - t0)
        return r

    elapsed, (files, n_shapes, n_launches) = timed(ranks, step, args.steps, args.warmup)
    step_seconds = step_seconds[-args.steps:]
    pixels = sum(sizes[i][0] * sizes[i][1] for i in mine)
    bits = sum(len(files[i]) for i in mine) * 8
    tot_px, tot_bits = ranks.sum_over_ranks([pixels, bits])
    value = tot_px * args.steps / 1e6 / elapsed
    if args.dump_outputs:
        import numpy as np
        dump_outputs(args, ranks, dict(file_arrays([files[i] for i in mine]), image_ids=np.array(mine, dtype=np.float64)))
    decode = None
    if args.full:
        # SET DECODE (round 6; outside the encode's timed region): EVERY file of the rank decoded back -- `.l3c` bytes on the host -> uint8 pixels
        # on the host -- and compared with its input, like the reference's folder evaluation does (multiscale_tester.py:353-381, assert_equal :373);
        # files of equal padded shape share a batch, the batches stream through Bitcoding.decode_many
        dec_seconds, lanes = [], int(os.environ.get('L3C_DECODE_LANES', '0')) or None
        ragged = {'0': False, '1': True}.get(os.environ.get('L3C_DECODE_RAGGED'))      # (development: A/B of the grouped RGB decode; None = the product's choice)
        if os.environ.get('L3C_RAGGED_GROUP'):      # (development: images per ragged group)
            bc.RAGGED_GROUP = int(os.environ['L3C_RAGGED_GROUP'])
        if os.environ.get('L3C_RAGGED_MPIX'):       # (development: pixel budget of a ragged group)
            bc.RAGGED_GROUP_PIXELS = int(os.environ['L3C_RAGGED_MPIX']) << 20
        for rep in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            back = dataset_codec.decode_set(bc, files, mine, max_batch=args.max_batch, lanes=lanes, ragged=ragged)
            torch.cuda.synchronize()
            dec_seconds.append(time.perf_counter() - t0)
        wrong = [i for i in mine if not torch.equal(back[i], imgs[i])]
        assert not wrong, 'set decode is not lossless for images {}'.format(wrong[:8])
        dec_best = min(dec_seconds[1:])
        decode = {'value': round(pixels / 1e6 / dec_best, 2), 'unit': 'MPix/s', 'images_decoded_on_rank0': len(mine), 'lossless': 'every image compared with its input',
                  'seconds_rank0': [round(t, 4) for t in dec_seconds], 'timing': 'best of the two passes after the first one of the process',
                  'lanes': lanes or bc.N_DECODE_LANES, 'ragged_rgb': True if ragged is None else ragged,
                  'note': 'host .l3c bytes -> host uint8 pixels of EVERY file the encode leg wrote (dataset_codec.decode_set): framing parsed on the host, '
                          'files uploaded as they are, batches of equal padded shape streamed through Bitcoding.decode_many'}
    result = None
    if ranks.rank == 0:
        name, ncu, arch = _lib.device_info()
        result = contract(
            args, ranks, value, elapsed, metric='MPix/s encode (host uint8 image -> .l3c bytes on the host) on a heterogeneous image set',
            config={'workload': 'L3C 0306_0001, {} synthetic natural-like images, sizes drawn like the reference\'s Open Images preprocessing '
                                '(short side 512..1024), END TO END: H2D, pad to 8, forward, fused heads, grouped range-coder launches, file '
                                'assembly on the device, one D2H'.format(args.images),
                    'images': args.images, 'images_on_rank0': len(mine), 'distinct_padded_shapes_on_rank0': n_shapes,
                    'forward_launches_on_rank0': n_launches, 'max_batch': args.max_batch,
                    'sharding': 'largest-first greedy on pixel counts (helpers/sharding.shard_balanced), replicas only',
                    'pixels_on_rank0_over_mean': round(pixels * ranks.world / tot_px, 4)},
            bpsp=round(tot_bits / (3 * tot_px), 4), megapixels=round(tot_px / 1e6, 1),
            per_step={'seconds_rank0': [round(t, 4) for t in step_seconds],
                      'mpix_per_s_rank0_best': round(pixels / 1e6 / min(step_seconds), 2),
                      'mpix_per_s_rank0_median': round(pixels / 1e6 / sorted(step_seconds)[len(step_seconds) // 2], 2),
                      'mpix_per_s_rank0_worst': round(pixels / 1e6 / max(step_seconds), 2)},
            device='{} ({}, {} CUs)'.format(name, arch, ncu), peak_hbm_gb=round(torch.cuda.max_memory_allocated() / 1e9, 1),
            **({'decode': decode} if args.full else {}))
    return result


# ---- files: the reference's own benchmark loop -- image FILES on disk -> `.l3c` files on disk -> decoded and compared -----------------------


def run_files(args, ranks):
    """`python test.py LOG_DIR 0306_0001 IMAGES --write_to_files D --time_report P` (reference test.py:44-104 ->
    test/multiscale_tester.py:272-381, timed by its StackTimeLogger, test/cuda_timer.py:107-151; image read:
    dataloaders/images_loader.py:91-129), measured file to file: N synthetic images are written as PNG files to a temporary
    directory (outside the timed region), then the tester reads and decodes them on worker threads, codes them in windows (encode_set),
    writes the `.l3c` files, reads them back, decodes them (decode_set) and compares every image with its input.  Two figures: encode
    (PNG files -> `.l3c` files on disk) and, with --full, the full round trip; the time report names the stages."""
    import concurrent.futures
    import contextlib
    import io
    import shutil
    import tempfile
    import types
    from PIL import Image
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd import _lib
    from l3c_pytorch_amd.helpers import config_parser, dataset_codec, sharding, synthetic
    from l3c_pytorch_amd.helpers.testset import Testset
    from l3c_pytorch_amd.test.multiscale_tester import MultiscaleTester
    cfg = config_parser.parse_builtin('ms', 'cr')
    sd = synthetic.make_state_dict(cfg, 0, calibrated=args.checkpoint == 'calibrated')
    sizes = dataset_codec.draw_sizes(args.images)
    mine = sharding.shard_balanced([h * w for h, w in sizes], ranks.rank, ranks.world)
    root = tempfile.mkdtemp(prefix='l3c_files_bench_')
    try:
        ckpts = os.path.join(root, 'logs', '0306_0001 cr oi', 'ckpts')
        os.makedirs(ckpts)
        torch.save({'net': sd}, os.path.join(ckpts, 'ckpt_0000000001.pt'))
        img_dir, out_dir = os.path.join(root, 'images'), os.path.join(root, 'written')
        os.makedirs(img_dir)

        def make_png(i):
            img = synthetic.make_image(sizes[i][0], sizes[i][1], i, 'natural')
            path = os.path.join(img_dir, 'img_{:05d}.png'.format(i))
            Image.fromarray(img.permute(1, 2, 0).numpy()).save(path, compress_level=1)
            return os.path.getsize(path)

        with single_thread():
            with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
                png_bytes = sum(pool.map(make_png, mine))
        io_threads = max(ranks.budget['io_threads'], min(16, (os.cpu_count() or 1) // max(1, ranks.world) // 2))
        report = os.path.join(root, 'times.txt')

        def make_tester(round_trip):
            flags = types.SimpleNamespace(log_dir=os.path.join(root, 'logs'), write_to_files=out_dir, time_report=report, batch=args.max_batch,
                                          io_threads=io_threads, write_window=args.write_window, round_trip=round_trip, recursive='0',
                                          skip_first_window=False)       # (every timed pass follows a whole warm-up pass)
            return MultiscaleTester('0306_0001', flags, -1)

        testset = Testset(img_dir)
        pixels = sum(sizes[i][0] * sizes[i][1] for i in mine)
        results = {}
        for name, round_trip in (('encode', False), ('round_trip', True))[:2 if args.full else 1]:
            tester = make_tester(round_trip)
            secs = []

            def step():
                shutil.rmtree(out_dir, ignore_errors=True)
                tester.times.times.clear()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
                    res = tester._test_write(testset)
                secs.append(time.perf_counter() - t0)
                return res

            elapsed, res = timed(ranks, step, args.steps, args.warmup)
            secs = secs[-args.steps:]
            stages = {k: round(float(sum(v)), 4) for k, v in tester.times.times.items()}     # the last pass
            slowest = max(stages, key=stages.get) if stages else None
            l3c_bytes = sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir))
            tot_px, = ranks.sum_over_ranks([pixels])
            results[name] = {'value': round(tot_px * args.steps / 1e6 / elapsed, 2), 'unit': 'MPix/s', 'seconds_rank0': [round(t, 4) for t in secs],
                             'bpsp': round(res.mean(), 4), 'l3c_bytes_rank0': l3c_bytes,
                             'stage_seconds_last_pass': stages, 'slowest_stage': slowest}
            elapsed_rt = elapsed
            if name == 'encode' and args.dump_outputs:      # the files of the last encode pass, by name
                import numpy as np
                written = sorted(os.listdir(out_dir))
                blobs = []
                for f in written:
                    with open(os.path.join(out_dir, f), 'rb') as fh:
                        blobs.append(fh.read())
                bpsp = np.array([res.per_img[k] for k in sorted(res.per_img)], dtype=np.float64)     # per image, by file name
                dump_outputs(args, ranks, dict(file_arrays(blobs), bpsp=bpsp))
        tot_px, = ranks.sum_over_ranks([pixels])
        result = None
        if ranks.rank == 0:
            name, ncu, arch = _lib.device_info()
            result = contract(
                args, ranks, results['encode']['value'], elapsed_rt,
                metric='MPix/s FILE TO FILE: image files (PNG) on disk -> .l3c files on disk (test.py --write_to_files), heterogeneous image set',
                config={'workload': 'L3C 0306_0001, {} synthetic natural-like images as PNG files ({} MB on rank 0), sizes drawn like the reference\'s '
                                    'Open Images preprocessing; the reference\'s own benchmark loop (test.py --write_to_files --time_report)'.format(
                                        args.images, round(png_bytes / 1e6, 1)),
                        'images': args.images, 'images_on_rank0': len(mine), 'max_batch': args.max_batch, 'write_window': args.write_window or 32 * args.max_batch,
                        'io_threads': io_threads, 'temporary_directory': os.path.dirname(root)},
                megapixels=round(tot_px / 1e6, 1), encode=results['encode'], device='{} ({}, {} CUs)'.format(name, arch, ncu),
                **({'round_trip': results['round_trip']} if args.full else {}))
            result['ms_per_step'] = round(results['encode']['seconds_rank0'][-1] * 1e3, 3)
        return result
    finally:
        shutil.rmtree(root, ignore_errors=True)


# ---- large: RGB Shared baseline on 3000x2000 (auto-cropped) and 2000x1500 images ----------------------------------------------------


def run_large(args, ranks):
    cfg, sd, bp, bc, synthetic = build_path('cr_rgb_shared', 0, args.checkpoint == 'calibrated')
    from l3c_pytorch_amd import _lib, auto_crop
    from l3c_pytorch_amd.helpers import pad
    recurse = 3
    fac = 2 ** (cfg.num_scales + recurse)                   # 16 (multiscale_tester.py:222-225)
    shapes = [(2000, 3000), (1500, 2000)]
    batches, px, crops_of = [], 0, []
    for k, (h, w) in enumerate(shapes):
        with single_thread():
            img = synthetic.make_image(h, w, 1000 + 2 * ranks.rank + k, 'natural').unsqueeze(0)
        crops = list(auto_crop.iter_crops(img))             # unpatched threshold: H*W > 2000*1500 -> 2x2 crops
        crops_of.append(len(crops))
        padded = [pad.pad(c, fac, mode='constant')[0] for c in crops]
        batches.append((torch.cat(padded).float().to(ranks.device), [int(c.shape[-2] * c.shape[-1]) for c in crops]))
        px += h * w
    torch.cuda.synchronize()

    def step():
        bpsps = []
        for x, areas in batches:
            comb = auto_crop.CropLossCombinator()
            for n, area in enumerate(areas):                # bpsp per crop over its unpadded sub-pixels, area-weighted (auto_crop.py:139-152)
                out = bp.forward(x[n:n + 1], recurse)
                loss = bp.get_loss(out, num_subpixels_before_pad=3 * area)
                comb.add(float(sum(loss.recursive_bpsps)), area)
            bpsps.append(comb.get_bpsp())
        return bpsps

    elapsed, bpsps = timed(ranks, step, args.steps, args.warmup)
    if args.dump_outputs:
        import numpy as np
        dump_outputs(args, ranks, {'bpsp': np.array(bpsps, dtype=np.float64)})
    value = ranks.world * px * args.steps / 1e6 / elapsed
    result = None
    if ranks.rank == 0:
        name, ncu, arch = _lib.device_info()
        result = contract(
            args, ranks, value, elapsed, metric='MPix/s forward + bpsp (RGB Shared baseline, auto_recurse 3) on large images',
            config={'workload': 'RGB Shared 0306_0002 (cr_rgb_shared.cf, synthetic seeded checkpoint), auto_recurse 3, pad to 16: per GPU and '
                                'step one 3000x2000 image (auto-cropped into {} crops) and one 2000x1500 image ({} crop): Pillow-exact bicubic '
                                'pyramid on the device + decoder + heads + NLL; forward + bpsp only, like the reference'.format(*crops_of),
                    'images_per_gpu_per_step': 2, 'crop_threshold_px': auto_crop._NEEDS_CROP_DIM, 'sharding': 'images, replicas only'},
            bpsp=[round(b, 4) for b in bpsps], flop_per_px=RGB_SHARED_FLOP_PER_PX,
            end_to_end_algorithmic_tflops=round(value * 1e6 * RGB_SHARED_FLOP_PER_PX / 1e12 / ranks.world, 2),
            device='{} ({}, {} CUs)'.format(name, arch, ncu), peak_hbm_gb=round(torch.cuda.max_memory_allocated() / 1e9, 1))
    return result


# ---- stub (tests): the launch / timing / reduction / JSON path without a GPU --------------------------------------------------------


def run_stub_dataset(args, ranks):
    """--config dataset --stub-step: config 4's host side on any number of gloo ranks -- the REAL size law, the REAL shard plan and
    the real reductions; the step is a sleep proportional to the rank's pixels and every image 'costs' (2 + index mod 3) bits per
    sub-pixel, so that the aggregate bpsp has a closed form the test can check."""
    from l3c_pytorch_amd.helpers import dataset_codec, sharding
    sizes = dataset_codec.draw_sizes(args.images)
    costs = [h * w for h, w in sizes]
    mine = sharding.shard_balanced(costs, ranks.rank, ranks.world)
    pixels = sum(costs[i] for i in mine)
    bits = sum(3 * costs[i] * (2 + i % 3) for i in mine)

    def step():
        time.sleep(pixels * 1e-9)          # 1 ns per pixel
        return None

    elapsed, _ = timed(ranks, step, args.steps, args.warmup)
    tot_px, tot_bits = ranks.sum_over_ranks([pixels, bits])
    shards = [None] * ranks.world
    if ranks.distributed:
        ranks.dist.all_gather_object(shards, {'rank': ranks.rank, 'items': mine, 'pixels': pixels})
    else:
        shards = [{'rank': 0, 'items': mine, 'pixels': pixels}]
    if ranks.rank != 0:
        return None
    return contract(args, ranks, tot_px * args.steps / 1e6 / elapsed, elapsed, data='stub (no GPU work)',
                    bpsp=tot_bits / (3 * tot_px), megapixels=round(tot_px / 1e6, 3),
                    config={'workload': 'stub dataset step: sleep 1 ns per pixel of the rank\'s shard', 'images': args.images,
                            'sharding': 'largest-first greedy on pixel counts (helpers/sharding.shard_balanced)', 'shards': shards,
                            'max_rank_pixels_over_mean': round(max(s['pixels'] for s in shards) * ranks.world / tot_px, 5)})


def run_stub(args, ranks):
    if args.config == 'dataset':
        return run_stub_dataset(args, ranks)
    from l3c_pytorch_amd.helpers import sharding
    mine = sharding.shard_indices(4 * ranks.world + 1, ranks.rank, ranks.world)      # uneven on purpose

    def step():
        time.sleep(0.01 * (1 + ranks.rank))              # rank r is slower than rank r - 1: the reduction must pick the slowest
        return len(mine)

    elapsed, n = timed(ranks, step, args.steps, args.warmup)
    px, = ranks.sum_over_ranks([n * H * W])
    if ranks.rank != 0:
        return None
    return contract(args, ranks, px * args.steps / 1e6 / elapsed, elapsed, data='stub (no GPU work)',
                    config={'workload': 'stub step: sleep 10 ms x (rank + 1)', 'items': 4 * ranks.world + 1})


class single_thread(object):
    """Synthetic images are made of small torch / numpy operations: on a 256-thread host torch's intra-op pool makes each of them
    SLOWER (0.32 s per 768x512 image with 8 threads, 0.11 s with one [measured in the build container]) -- set-up time only, outside the
    timed region, but it is most of the wall time of `--config dataset`."""

    def __enter__(self):
        self.saved = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.saved)


def spawn_ranks(args, argv):
    """`python bench.py --gpus N` without a launcher: re-execute under torch.distributed.run, one rank per GPU (RCCL over xGMI
    for the barrier and the reductions only; images shard with no data-path collective).  Fails loudly when fewer than N GPUs are
    visible: a line that says n_gpus = N must have run on N GPUs."""
    import socket
    import subprocess
    if not args.stub_step:
        n = torch.cuda.device_count()
        if n < args.gpus:
            raise SystemExit('bench.py: --gpus {} requested but only {} GPU(s) visible (HIP_VISIBLE_DEVICES={!r})'.format(
                args.gpus, n, os.environ.get('HIP_VISIBLE_DEVICES')))
    sock = socket.socket()
    sock.bind(('127.0.0.1', 0))
    port = sock.getsockname()[1]
    sock.close()
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    env.setdefault('OMP_NUM_THREADS', '8')
    return subprocess.call(cmd, cwd=os.getcwd(), env=env)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse_args(argv)
    if args.cpu_baseline_only:
        import l3c_pytorch_amd  # noqa: F401
        from l3c_pytorch_amd.helpers import config_parser, synthetic
        from oracle import cpu_baseline
        cfg = config_parser.parse_builtin('ms', 'cr')
        sd = synthetic.make_state_dict(cfg, 0, calibrated=args.checkpoint == 'calibrated')
        cpu, _ = cpu_baseline.run(sd, synthetic.make_image(H, W, 0, 'natural'))
        cpu['checkpoint'] = args.checkpoint
        cpu['host'] = 'build container' if os.path.isdir('/root/reference') else 'GPU box host'
        print(json.dumps(cpu))
        return cpu
    if args.gpus > 1 and 'RANK' not in os.environ:
        rc = spawn_ranks(args, argv)
        if rc != 0:
            raise SystemExit(rc)
        return None
    if args.config in ('dataset', 'files'):
        from l3c_pytorch_amd.helpers import runtime as _runtime
        _runtime.configure_hip_queues()                   # several small forward passes side by side, see Bitcoding.encode_many (before HIP starts)
    ranks = Ranks(stub=args.stub_step)
    if args.gpus != ranks.world:
        raise SystemExit('bench.py: --gpus {} but the launcher started {} rank(s) (WORLD_SIZE)'.format(args.gpus, ranks.world))
    run = run_stub if args.stub_step else {'headline': run_headline, 'dataset': run_dataset, 'large': run_large, 'files': run_files}[args.config]
    result = run(args, ranks)
    if ranks.rank == 0:
        print(json.dumps(result))
        sys.stdout.flush()
    ranks.close()
    return result


if __name__ == '__main__':
    main()
