#!/usr/bin/env python
"""Set decode of legacy against banded `.l3c` files on the same images, in ONE process and session: the 200-image leg of config 4
(dataset_codec.draw_sizes) is coded once with Bitcoding() and once with Bitcoding(bands=K); `decode_set` then reads the two sets
ALTERNATELY (legacy, banded, legacy, ...) -- the machines of a pool differ by a few per cent, runs of one process on one machine do not --
and every decoded image of every run is compared with its input.  Reported per format: the median and all run times, MPix/s, the peak
device memory of a run and the kernel launches of one decode (torch.profiler, a run of its own outside the timed ones).

    python tools/banded_set_decode.py [--images 200] [--bands 64] [--runs 5] [--warmup 1] [--json OUT]
    rocprofv3 --kernel-trace --stats -- python tools/banded_set_decode.py --only banded --no-launch-count    # where one format's time goes
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import l3c_pytorch_amd  # noqa: E402

l3c_pytorch_amd.configure_hip_queues()
import torch  # noqa: E402
import bench  # noqa: E402
from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding  # noqa: E402
from l3c_pytorch_amd.helpers import dataset_codec  # noqa: E402


def count_launches(fn):
    """Kernel launches of one call of fn (torch.profiler's device activity; None when the profiler reports none)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return n or None
    except Exception as exc:   # the profiler is a convenience here, the timing is the result
        print('launch count unavailable: {}'.format(exc), flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=200)
    ap.add_argument('--bands', type=int, default=64)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--only', choices=['legacy', 'banded'], default=None,
                    help='decode this format only (under rocprofv3 --kernel-trace --stats: one format per trace); no ratio is reported')
    ap.add_argument('--json', type=str, default=None)
    args = ap.parse_args()
    assert args.runs >= 5, 'a median of at least 5 runs per format'

    cfg, sd, bp, bc, synthetic = bench.build_path('cr', 0, True)
    sizes = dataset_codec.draw_sizes(args.images)
    imgs = {i: synthetic.make_image(sizes[i][0], sizes[i][1], i, 'natural') for i in range(args.images)}
    order = list(range(args.images))
    mpix = sum(h * w for h, w in sizes) / 1e6
    coders = {'legacy': Bitcoding(bp), 'banded': Bitcoding(bp, bands=args.bands)}
    files = {}
    for name, c in coders.items():
        files[name], _, _ = dataset_codec.encode_set(c, imgs, order, max_batch=16)
    nbytes = {name: sum(len(f) for f in fs.values()) for name, fs in files.items()}
    print('{} images, {:.1f} MPix; legacy {} bytes, banded (K = {}) {} bytes ({:+.2f} %)'.format(
        args.images, mpix, nbytes['legacy'], args.bands, nbytes['banded'], 100.0 * (nbytes['banded'] / nbytes['legacy'] - 1)), flush=True)

    dec = Bitcoding(bp)                      # ONE decoder object for both formats: the same streams, lanes and page-locked buffers

    def run(name):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        back = dataset_codec.decode_set(dec, files[name], order, max_batch=16, banded=(name == 'banded'))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated()
        wrong = [i for i in order if not torch.equal(back[i], imgs[i])]
        if wrong:
            raise AssertionError('{}: decoded images differ from their inputs: {}'.format(name, wrong[:10]))
        return dt, peak

    times, peaks = {'legacy': [], 'banded': []}, {'legacy': 0, 'banded': 0}
    formats = (args.only,) if args.only else ('legacy', 'banded')
    for r in range(args.warmup + args.runs):
        for name in formats:
            dt, peak = run(name)
            tag = 'warm-up' if r < args.warmup else 'run {}'.format(r - args.warmup)
            print('{:>8} {:>8}: {:.4f} s  {:.1f} MPix/s  peak {:.2f} GB  (all {} images equal their inputs)'.format(
                tag, name, dt, mpix / dt, peak / 2.0 ** 30, args.images), flush=True)
            if r >= args.warmup:
                times[name].append(dt)
                peaks[name] = max(peaks[name], peak)
    launches = {name: None if args.no_launch_count else count_launches(lambda n=name: run(n)) for name in formats}
    res = {'images': args.images, 'mpix': round(mpix, 3), 'bands': args.bands, 'runs': args.runs, 'bytes': nbytes}
    for name in formats:
        med = sorted(times[name])[len(times[name]) // 2]
        res[name] = {'median_s': round(med, 4), 'mpix_per_s': round(mpix / med, 1), 'runs_s': [round(t, 4) for t in times[name]],
                     'peak_gb': round(peaks[name] / 2.0 ** 30, 2), 'kernel_launches': launches[name]}
        print('{:>8}: median {:.4f} s = {:.1f} MPix/s over {} runs (min {:.4f}, max {:.4f}); peak {:.2f} GB; {} kernel launches'.format(
            name, med, mpix / med, args.runs, min(times[name]), max(times[name]), peaks[name] / 2.0 ** 30, launches[name]), flush=True)
    if not args.only:
        res['banded_over_legacy'] = round(res['banded']['mpix_per_s'] / res['legacy']['mpix_per_s'], 3)
        print('banded / legacy set decode throughput: {:.3f}'.format(res['banded_over_legacy']), flush=True)
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
