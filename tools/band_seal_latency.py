#!/usr/bin/env python
"""What a BAND seal costs beside a version-1 seal (include/l3c_hip.h "band seals"), on the calibrated checkpoint, host to host.

    python tools/band_seal_latency.py              the latencies (below)
    python tools/band_seal_latency.py --kernels    the kernel alone, from a `rocprofv3 --kernel-trace --stats` run of its own

Latencies, through NativeCodec(bp, bands=64): one 768x512 image and a batch (--batch, default 16),

    encode   uint8 pixels on the host -> the files' bytes on the host     NativeCodec.encode_batch
    decode   the files' bytes on the host -> uint8 pixels on the host     NativeCodec.decode_batch(...).cpu()

and through Bitcoding(bp, bands=64).decode_region a 64-row and a 256-row region of one 512x768 and one 2048x3072 image (rows x columns), on a
version-1 sealed file (the pixels come back unverified, the last band is cut) against a band-sealed one (verified, the last band whole).
The legs of a measurement run in one process, alternated -- version-1 sealed, band-sealed, version-1 sealed again: the version-1 leg runs
TWICE per round, so its two rows show the run-to-run spread a difference has to exceed.  Medians of --runs rounds after --warmup.

--kernels: a child process under the profiler calls, on 128 frames of 768x512 at L = 6144 and on 16 frames of 2048x3072 at L = 98304,
l3c_u8_crc32_bands and beside it the two calls it replaces -- l3c_u8_crc32_spans over the same band spans plus l3c_u8_crc32 over the frames
--, checks that they agree, and the parent (which never opens the GPU) reduces the kernel trace: per call the median of the summed
durations of its launches.  Prints one JSON object per row and a table at the end."""
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
H, W, K = 512, 768, 64
KERNEL_CASES = [(128, 512, 768, 6144), (16, 2048, 3072, 98304)]          # frames, H, W, band length
KERNEL_CALLS, KERNEL_WARMUP = 20, 3
NEW = ('u8_crc32_band_chunks_kernel', 'u8_crc32_bands_combine_kernel')
OLD = ('u8_crc32_spans_prepare_kernel', 'u8_crc32_span_tiles_kernel', 'u8_crc32_spans_combine_kernel', 'u8_crc32_tiles_kernel', 'u8_crc32_combine_kernel')


def kernels_child():
    """Under the profiler: per case KERNEL_WARMUP + KERNEL_CALLS rounds of the new call and of the two calls it replaces."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd import _lib, ops
    _lib.require_gpu()
    g = torch.Generator(device='cuda').manual_seed(0)
    for F, h, w, L in KERNEL_CASES:
        hw = h * w
        n = -(-hw // L)
        frames = torch.randint(0, 256, (F * 3 * hw,), generator=g, device='cuda', dtype=torch.uint8)
        start = (np.arange(3 * F, dtype=np.int64)[:, None] * hw + np.arange(n, dtype=np.int64)[None, :] * L).reshape(-1)
        length = np.tile(np.minimum(L, hw - np.arange(n, dtype=np.int64) * L), 3 * F)
        for _ in range(KERNEL_WARMUP + KERNEL_CALLS):
            bands, whole = ops.u8_crc32_bands(frames, F, hw, L)
            spans = ops.u8_crc32_spans(frames, start, length)
            items = ops.u8_crc32(frames, F, 3 * hw)
            torch.cuda.synchronize()
        assert torch.equal(bands.view(-1), spans) and torch.equal(whole, items)
        del frames
        torch.cuda.empty_cache()
    return 0


def kernel_rows(trace_dir):
    """Runs the child under rocprofv3 and reduces its kernel trace -> rows."""
    trace_dir = tempfile.mkdtemp(prefix='band_seal_trace_') if trace_dir is None else os.path.join(trace_dir, 'pid{}'.format(os.getpid()))
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', trace_dir, '-o', 'bands', '--', sys.executable,
           os.path.abspath(__file__), '--kernels-child']
    subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
    dur = {}
    for f in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        for r in sorted(csv.DictReader(open(f)), key=lambda r: int(r['Start_Timestamp'])):
            for key in NEW + OLD:
                if key in r['Kernel_Name']:
                    dur.setdefault(key, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    per = KERNEL_WARMUP + KERNEL_CALLS
    for key in NEW + OLD:
        assert len(dur.get(key, [])) == per * len(KERNEL_CASES), (key, len(dur.get(key, [])))
    rows = []
    for k, (F, h, w, L) in enumerate(KERNEL_CASES):
        take = {key: v[k * per + KERNEL_WARMUP:(k + 1) * per] for key, v in dur.items()}
        new = [sum(take[key][i] for key in NEW) for i in range(KERNEL_CALLS)]
        old = [sum(take[key][i] for key in OLD) for i in range(KERNEL_CALLS)]
        nbytes = F * 3 * h * w
        row = {'frames': F, 'H': h, 'W': w, 'band_bytes': L, 'bytes': nbytes, 'calls': KERNEL_CALLS,
               'bands_us_median': round(statistics.median(new), 2), 'bands_us_min': round(min(new), 2), 'bands_us_max': round(max(new), 2),
               'spans_plus_crc32_us_median': round(statistics.median(old), 2), 'spans_plus_crc32_us_min': round(min(old), 2),
               'bands_TB_per_s': round(nbytes / statistics.median(new) / 1e6, 3)}
        for key in NEW + OLD:
            row[key + '_us_median'] = round(statistics.median(take[key]), 2)
            row[key + '_us_spread'] = round(max(take[key]) - min(take[key]), 2)
        rows.append(row)
    return rows


def alternate(legs, check, runs, warmup, sync):
    """legs: [(name, fn -> (seconds, result))] run alternately -> per leg the list of milliseconds."""
    times = [[] for _ in legs]
    for it in range(warmup + runs):
        for k, (name, fn) in enumerate(legs):
            sync()
            t, out = fn()
            check(name, out)
            if it >= warmup:
                times[k].append(t * 1e3)
    return times


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16, help='the second batch size (0: one image only)')
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-large', action='store_true', help='skip the 2048x3072 region decodes')
    ap.add_argument('--kernels', action='store_true', help='the kernel trace alone (a rocprofv3 child; this process does not open the GPU)')
    ap.add_argument('--trace-dir', default=None, help='where the kernel trace goes (default: a fresh temporary directory)')
    ap.add_argument('--kernels-child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.kernels_child:
        return kernels_child()
    if args.kernels:
        rows = kernel_rows(args.trace_dir)
        for row in rows:
            print(json.dumps(row), flush=True)
        print('\n{:>7} {:>11} {:>9} {:>18} {:>26} {:>10}'.format('frames', 'size', 'L', 'crc32_bands us', 'crc32_spans + crc32 us', 'TB/s'))
        for r in rows:
            print('{:>7} {:>11} {:>9} {:>18.2f} {:>26.2f} {:>10.3f}'.format(r['frames'], '{}x{}'.format(r['H'], r['W']), r['band_bytes'],
                                                                            r['bands_us_median'], r['spans_plus_crc32_us_median'], r['bands_TB_per_s']))
        return 0
    sys.path.insert(0, ROOT)
    import torch
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd import _lib
    from l3c_pytorch_amd.bitcoding import container
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    from l3c_pytorch_amd.helpers import config_parser, synthetic
    from l3c_pytorch_amd.native_codec import NativeCodec
    _lib.require_gpu()
    cfg = config_parser.parse_builtin('ms', 'cr')
    bp = MultiscaleBlueprint(cfg)
    bp.net.load_state_dict(synthetic.make_state_dict(cfg, 0, calibrated=True), strict=True)
    bp.set_eval()
    plain, v1, v2 = NativeCodec(bp, bands=K), NativeCodec(bp, bands=K, seal=True), NativeCodec(bp, bands=K, seal='bands')
    for c in (v1, v2):
        c.model_id()                                                     # hashed once per codec object: not part of a call
    clock = time.perf_counter
    rows = []

    def report(what, names, times, nbytes):
        for name, t in zip(names, times):
            row = dict(what, leg=name, bytes=nbytes[name.split()[0]], ms_median=round(statistics.median(t), 3), ms_min=round(min(t), 3), runs=args.runs)
            rows.append(row)
            print(json.dumps(row), flush=True)

    for B in [1] + ([args.batch] if args.batch else []):
        imgs = torch.stack([synthetic.make_image(H, W, i, 'natural') for i in range(B)]).to(torch.uint8)          # on the host
        files = {'v1': v1.encode_batch(imgs), 'bands': v2.encode_batch(imgs)}
        unsealed = plain.encode_batch(imgs)
        n = container.split_seal(files['bands'][0])[1].band_crcs.shape[1]
        assert [len(f) - len(u) for f, u in zip(files['bands'], unsealed)] == [20 + 12 * n + 24] * B
        assert [container.split_seal(f)[0] for f in files['bands']] == unsealed == [f[:-24] for f in files['v1']]
        nbytes = {k: sum(len(f) for f in v) for k, v in files.items()}
        print(json.dumps({'batch': B, 'bands_per_channel': n, 'unsealed_bytes': sum(len(u) for u in unsealed), 'v1_bytes': nbytes['v1'],
                          'band_sealed_bytes': nbytes['bands'], 'band_sealed_over_unsealed': round(nbytes['bands'] / sum(len(u) for u in unsealed), 5)}))

        def encode(codec):
            def run():
                t0 = clock()
                out = codec.encode_batch(imgs)
                return clock() - t0, out
            return run

        def decode(which):
            def run():
                t0 = clock()
                out = plain.decode_batch(files[which])[0].cpu()
                return clock() - t0, out
            return run
        names = ['v1', 'bands', 'v1 again']
        t = alternate(list(zip(names, [encode(v1), encode(v2), encode(v1)])), lambda name, out: out == files[name.split()[0]] or sys.exit('files differ'),
                      args.runs, args.warmup, torch.cuda.synchronize)
        report({'batch': B, 'what': 'encode'}, names, t, nbytes)
        t = alternate(list(zip(names, [decode('v1'), decode('bands'), decode('v1')])), lambda name, out: torch.equal(out, imgs) or sys.exit('pixels differ'),
                      args.runs, args.warmup, torch.cuda.synchronize)
        report({'batch': B, 'what': 'decode'}, names, t, nbytes)
        del imgs
        torch.cuda.empty_cache()

    bcs = {'v1': Bitcoding(bp, bands=K, seal=True), 'bands': Bitcoding(bp, bands=K, seal='bands')}
    for h, w in [(512, 768)] + ([] if args.no_large else [(2048, 3072)]):
        img = synthetic.make_image(h, w, 3, 'natural').to(torch.uint8).unsqueeze(0)
        files = {k: bc.encode_batch(img.cuda()).to_bytes() for k, bc in bcs.items()}
        nbytes = {k: len(v[0]) for k, v in files.items()}
        for n_rows in (64, 256):
            y0 = (h - n_rows) // 2 // 64 * 64 + 5                       # in the middle, not on a band's first row
            box = (y0, y0 + n_rows)
            infos = {}

            def region(which):
                def run():
                    t0 = clock()
                    out, info = bcs['v1'].decode_region(files[which], box)
                    out = out.cpu()
                    infos[which] = info
                    return clock() - t0, out
                return run
            names = ['v1', 'bands', 'v1 again']
            t = alternate(list(zip(names, [region('v1'), region('bands'), region('v1')])),
                          lambda name, out: torch.equal(out, img[:, :, box[0]:box[1]]) or sys.exit('region differs'), args.runs, args.warmup,
                          torch.cuda.synchronize)
            assert infos['bands'].pixel_crc_checked is True and infos['v1'].pixel_crc_checked is False
            report({'image': '{}x{}'.format(h, w), 'what': 'region of {} rows'.format(n_rows), 'sym_rows_v1': infos['v1'].sym_rows,
                    'sym_rows_bands': infos['bands'].sym_rows}, names, t, nbytes)

    print('\n{:>28} {:>24} {:>10} {:>12} {:>10}'.format('case', 'what', 'leg', 'median ms', 'min ms'))
    for r in rows:
        print('{:>28} {:>24} {:>10} {:>12.3f} {:>10.3f}'.format('batch {}'.format(r['batch']) if 'batch' in r else r['image'], r['what'], r['leg'],
                                                                r['ms_median'], r['ms_min']))
    for i in range(0, len(rows), 3):
        a, s, b = (r['ms_median'] for r in rows[i:i + 3])
        r = rows[i]
        print('{} {}: band-sealed - mean(version 1) = {:+.3f} ms = {:+.2%}; the version-1 legs differ by {:.3f} ms{}'.format(
            'batch {}'.format(r['batch']) if 'batch' in r else r['image'], r['what'], s - (a + b) / 2, (s - (a + b) / 2) / ((a + b) / 2), abs(a - b),
            '' if min(a, b) <= s <= max(a, b) else '  (outside their spread)'))
    return 0


if __name__ == '__main__':
    sys.exit(main())
