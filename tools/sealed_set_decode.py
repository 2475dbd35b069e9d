#!/usr/bin/env python
"""What verifying a sealed SET costs (dataset_codec.decode_set(..., sealed=True): per ragged group one l3c_sym_to_u8 and one
l3c_u8_crc32_spans, one D2H of all CRC words at the end), in ONE process and session: the 200-image leg of config 4
(dataset_codec.draw_sizes) is coded once with Bitcoding(seal=True); `decode_set` then reads, ALTERNATELY,

    bodies          the unsealed bodies of those files                 -- the path without this feature
    sealed          the sealed files with sealed=True
    bodies again    the unsealed bodies once more                      -- the two unsealed legs show the spread a difference has to exceed
    verify_set      dataset_codec.verify_set on the sealed files       -- the same decode, no pixel leaves the device

and every decoded image of every run is compared with its input (verify_set: every status must be 'ok').  Medians of --runs rounds.

Then the kernel alone, from a kernel trace of its own (rocprofv3 --kernel-trace around a child process started here, --no-trace skips it):
l3c_u8_crc32_spans on 128 spans of 768x512 frames beside l3c_u8_crc32 on the same bytes, call by call in the same run, and
l3c_u8_crc32_spans on 200 spans of the set's mixed padded frame sizes.  Prints one JSON object per row.

    python tools/sealed_set_decode.py [--images 200] [--runs 5] [--warmup 1] [--trace-dir DIR] [--no-trace]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES, H, W = 128, 512, 768
KERNEL_CALLS = 20
SPANS_KERNELS = ('u8_crc32_spans_prepare_kernel', 'u8_crc32_span_tiles_kernel', 'u8_crc32_spans_combine_kernel')
UNIFORM_KERNELS = ('u8_crc32_tiles_kernel', 'u8_crc32_combine_kernel')


def kernels_child(images):
    """Under the profiler: KERNEL_CALLS calls of each form after three warm-up calls.  The order of the launches is what kernel_rates
    relies on: per round the uniform call, the spans call on the same frames, the spans call on the mixed frames."""
    import zlib
    import numpy as np
    import torch
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd import _lib, ops
    from l3c_pytorch_amd.helpers import dataset_codec
    _lib.require_gpu()
    g = torch.Generator(device='cuda').manual_seed(0)
    n = 3 * H * W
    pix = torch.randint(0, 256, (FRAMES * n,), generator=g, device='cuda', dtype=torch.uint8)
    offs, lens = np.arange(FRAMES, dtype=np.int64) * n, np.full(FRAMES, n, dtype=np.int64)
    mixed_lens = np.asarray([3 * (-(-h // 8) * 8) * (-(-w // 8) * 8) for h, w in dataset_codec.draw_sizes(images)], dtype=np.int64)
    mixed_offs = np.cumsum(mixed_lens) - mixed_lens
    mixed = torch.randint(0, 256, (int(mixed_lens.sum()),), generator=g, device='cuda', dtype=torch.uint8)
    for _ in range(3 + KERNEL_CALLS):
        a = ops.u8_crc32(pix, FRAMES, n)
        b = ops.u8_crc32_spans(pix, offs, lens)
        c = ops.u8_crc32_spans(mixed, mixed_offs, mixed_lens)
        torch.cuda.synchronize()
    assert torch.equal(a, b)
    host = mixed.cpu().numpy()
    assert c.cpu().numpy().view('uint32').tolist() == [zlib.crc32(host[o:o + m].tobytes()) for o, m in zip(mixed_offs, mixed_lens)]
    print(json.dumps({'mixed_bytes': int(mixed_lens.sum())}), flush=True)
    return 0


def kernel_rates(trace_dir, images):
    """Runs the child under rocprofv3 and reduces its kernel trace -> rows."""
    trace_dir = tempfile.mkdtemp(prefix='sealed_set_trace_') if trace_dir is None else os.path.join(trace_dir, 'pid{}'.format(os.getpid()))
    cmd = ['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', trace_dir, '-o', 'spans', '--', sys.executable, os.path.abspath(__file__),
           '--kernels-child', '--images', str(images)]
    out = subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.PIPE).stdout.decode()
    mixed_bytes = [json.loads(line)['mixed_bytes'] for line in out.splitlines() if line.startswith('{"mixed_bytes"')][0]
    dur = {}
    for f in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        for r in sorted(csv.DictReader(open(f)), key=lambda r: int(r['Start_Timestamp'])):
            for key in SPANS_KERNELS + UNIFORM_KERNELS:
                if key in r['Kernel_Name']:
                    dur.setdefault(key, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    for key in UNIFORM_KERNELS:
        assert len(dur[key]) == 3 + KERNEL_CALLS, (key, len(dur[key]))
    for key in SPANS_KERNELS:                           # two spans calls per round: the same frames, then the mixed ones
        assert len(dur[key]) == 2 * (3 + KERNEL_CALLS), (key, len(dur[key]))
    uniform = [sum(dur[k][i] for k in UNIFORM_KERNELS) for i in range(3, 3 + KERNEL_CALLS)]
    same = [sum(dur[k][2 * i] for k in SPANS_KERNELS) for i in range(3, 3 + KERNEL_CALLS)]
    mixed = [sum(dur[k][2 * i + 1] for k in SPANS_KERNELS) for i in range(3, 3 + KERNEL_CALLS)]
    nbytes = FRAMES * 3 * H * W

    def row(name, spans, total, us, parts, which):
        r = {'kernel': name, 'spans': spans, 'bytes_hashed': total, 'us_median': round(statistics.median(us), 2), 'us_min': round(min(us), 2),
             'us_max': round(max(us), 2), 'TB_per_s_hashed': round(total / statistics.median(us) / 1e6, 3), 'calls': KERNEL_CALLS}
        for k in parts:
            v = dur[k][3:] if which is None else dur[k][2 * 3 + which::2]
            r[k + '_us_median'] = round(statistics.median(v), 2)
        return r

    return [row('l3c_u8_crc32 (both launches)', FRAMES, nbytes, uniform, UNIFORM_KERNELS, None),
            row('l3c_u8_crc32_spans (three launches), the same frames', FRAMES, nbytes, same, SPANS_KERNELS, 0),
            row('l3c_u8_crc32_spans (three launches), the set\'s mixed frames', images, mixed_bytes, mixed, SPANS_KERNELS, 1)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=200)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--trace-dir', default=None, help='where the kernel trace goes (default: a fresh temporary directory)')
    ap.add_argument('--no-trace', action='store_true', help='skip the kernel trace (no rocprofv3 child)')
    ap.add_argument('--kernels-child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.kernels_child:
        return kernels_child(args.images)
    assert args.runs >= 5, 'a median of at least 5 runs per leg'
    import l3c_pytorch_amd
    l3c_pytorch_amd.configure_hip_queues()
    import torch
    import bench
    from l3c_pytorch_amd.bitcoding import container
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.helpers import dataset_codec

    cfg, sd, bp, bc, synthetic = bench.build_path('cr', 0, True)
    sizes = dataset_codec.draw_sizes(args.images)
    imgs = {i: synthetic.make_image(sizes[i][0], sizes[i][1], i, 'natural') for i in range(args.images)}
    order = list(range(args.images))
    mpix = sum(h * w for h, w in sizes) / 1e6
    sealed, _, _ = dataset_codec.encode_set(Bitcoding(bp, seal=True), imgs, order, max_batch=16)
    bodies = {i: bytes(container.split_seal(sealed[i])[0]) for i in order}
    assert all(container.is_sealed(sealed[i]) and len(sealed[i]) == len(bodies[i]) + container.SEAL_BYTES for i in order)
    print('{} images, {:.1f} MPix, {} bytes sealed'.format(args.images, mpix, sum(len(f) for f in sealed.values())), flush=True)
    dec = Bitcoding(bp)                      # ONE decoder object for every leg: the same streams, lanes and page-locked buffers
    dec.model_id()                           # hashed once per object: not part of a call

    def decode(files, **kw):
        def run():
            back = dataset_codec.decode_set(dec, files, order, max_batch=16, **kw)
            torch.cuda.synchronize()
            return lambda: [i for i in order if not torch.equal(back[i], imgs[i])]
        return run

    def verify():
        status = dataset_codec.verify_set(dec, sealed, order, max_batch=16)
        torch.cuda.synchronize()
        return lambda: [i for i in order if status[i] != 'ok']

    legs = [('bodies', decode(bodies)), ('sealed', decode(sealed, sealed=True)), ('bodies again', decode(bodies)), ('verify_set', verify)]
    times = {name: [] for name, _ in legs}
    for r in range(args.warmup + args.runs):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            check = fn()
            dt = time.perf_counter() - t0
            wrong = check()
            if wrong:
                raise AssertionError('{}: images that differ from their inputs / files not ok: {}'.format(name, wrong[:10]))
            tag = 'warm-up' if r < args.warmup else 'run {}'.format(r - args.warmup)
            print('{:>8} {:>13}: {:.4f} s  {:.1f} MPix/s'.format(tag, name, dt, mpix / dt), flush=True)
            if r >= args.warmup:
                times[name].append(dt)
    res = {'images': args.images, 'mpix': round(mpix, 3), 'runs': args.runs}
    for name, _ in legs:
        med = statistics.median(times[name])
        res[name] = {'median_ms': round(med * 1e3, 2), 'mpix_per_s': round(mpix / med, 1), 'runs_ms': [round(t * 1e3, 2) for t in times[name]]}
        print('{:>13}: median {:.2f} ms = {:.1f} MPix/s over {} runs (min {:.2f}, max {:.2f})'.format(
            name, med * 1e3, mpix / med, args.runs, min(times[name]) * 1e3, max(times[name]) * 1e3), flush=True)
    a, s, b = (res[k]['median_ms'] for k in ('bodies', 'sealed', 'bodies again'))
    res['sealed_minus_mean_unsealed_ms'] = round(s - (a + b) / 2, 2)
    res['unsealed_legs_differ_by_ms'] = round(abs(a - b), 2)
    res['sealed_inside_the_unsealed_spread'] = bool(min(a, b) <= s <= max(a, b))
    print('sealed - mean(unsealed) = {:+.2f} ms = {:+.2%} of the unsealed leg; the unsealed legs differ by {:.2f} ms{}'.format(
        s - (a + b) / 2, (s - (a + b) / 2) / ((a + b) / 2), abs(a - b), '' if res['sealed_inside_the_unsealed_spread'] else '  (outside their spread)'),
        flush=True)
    print(json.dumps(res), flush=True)
    if not args.no_trace:
        for row in kernel_rates(args.trace_dir, args.images):
            print(json.dumps(row), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
