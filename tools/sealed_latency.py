#!/usr/bin/env python
"""What a seal costs (NativeCodec(bp, seal=True): l3c_u8_crc32 + l3c_seal_append behind the encode; l3c_u8_crc32 and one D2H of B words
behind the decode) on 768x512 images of the calibrated checkpoint, legacy format, host to host:

    encode   uint8 pixels on the host -> the files' bytes on the host     NativeCodec.encode_batch
    decode   the files' bytes on the host -> uint8 pixels on the host     NativeCodec.decode_batch(...).cpu()

for one image and a batch (--batch, default 16).  The legs of a direction run in one process, alternated -- unsealed, sealed, unsealed
again: the unsealed leg runs TWICE per round, so its two rows show the run-to-run spread a difference has to exceed.  Medians of --runs rounds
after --warmup; `enqueued` = until the call that enqueues the work has returned, `done` = until the result is on the host (for a sealed decode
the enqueue already includes the D2H of the CRC words: the comparison is part of the call).

Then the kernel alone, from a kernel trace of its own (rocprofv3 --kernel-trace around a child process started here, --no-trace skips it):
l3c_u8_crc32 on 128 frames of 768x512 in one call -- both launches, bytes hashed per second -- beside l3c_sym_to_u8 on the same pixels (bytes
read + written per second).  Prints one JSON object per row and a table at the end.

    python tools/sealed_latency.py [--trace-dir DIR]
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
FRAMES, H, W = 128, 512, 768
KERNEL_CALLS = 20


def kernels_child():
    """Under the profiler: KERNEL_CALLS calls of each entry on 128 frames, after three warm-up calls."""
    sys.path.insert(0, ROOT)
    import torch
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd import _lib, ops
    _lib.require_gpu()
    g = torch.Generator(device='cuda').manual_seed(0)
    sym = torch.randint(0, 256, (FRAMES, 3, H, W), generator=g, device='cuda', dtype=torch.int16)
    pix = torch.empty(FRAMES, 3, H, W, dtype=torch.uint8, device='cuda')
    n = 3 * H * W
    n_ws = _lib.load().l3c_u8_crc32_workspace_bytes(FRAMES, n)
    ws = torch.empty(n_ws, dtype=torch.uint8, device='cuda')
    out = torch.empty(FRAMES, dtype=torch.int32, device='cuda')
    for _ in range(3 + KERNEL_CALLS):
        _lib.call('l3c_sym_to_u8', sym.data_ptr(), sym.numel(), pix.data_ptr(), _lib.stream())
        ops.u8_crc32(pix.view(-1), FRAMES, n, out=out, workspace=ws)
        torch.cuda.synchronize()
    import zlib
    host = pix.cpu().numpy()
    assert out.cpu().numpy().view('uint32').tolist() == [zlib.crc32(host[i].tobytes()) for i in range(FRAMES)]
    return 0


def kernel_rates(trace_dir):
    """Runs the child under rocprofv3 and reduces its kernel trace -> rows."""
    # a directory of this run's own: nothing of an earlier trace is read
    trace_dir = tempfile.mkdtemp(prefix='sealed_latency_trace_') if trace_dir is None else os.path.join(trace_dir, 'pid{}'.format(os.getpid()))
    cmd = ['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', trace_dir, '-o', 'sealed', '--', sys.executable, os.path.abspath(__file__),
           '--kernels-child']
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    dur = {}
    for f in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        for r in sorted(csv.DictReader(open(f)), key=lambda r: int(r['Start_Timestamp'])):
            for key in ('u8_crc32_tiles_kernel', 'u8_crc32_combine_kernel', 'sym_to_u8'):
                if key in r['Kernel_Name']:
                    dur.setdefault(key, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    for key, v in dur.items():
        assert len(v) == 3 + KERNEL_CALLS, (key, len(v))
    med = {k: statistics.median(v[3:]) for k, v in dur.items()}
    lo = {k: min(v[3:]) for k, v in dur.items()}
    pixels = FRAMES * 3 * H * W
    crc_us = med['u8_crc32_tiles_kernel'] + med['u8_crc32_combine_kernel']
    return [{'kernel': 'l3c_u8_crc32 (both launches)', 'frames': FRAMES, 'bytes_hashed': pixels, 'tiles_us_median': round(med['u8_crc32_tiles_kernel'], 2),
             'combine_us_median': round(med['u8_crc32_combine_kernel'], 2), 'tiles_us_min': round(lo['u8_crc32_tiles_kernel'], 2),
             'TB_per_s_hashed': round(pixels / crc_us / 1e6, 3), 'calls': KERNEL_CALLS},
            {'kernel': 'l3c_sym_to_u8', 'frames': FRAMES, 'bytes_read_and_written': 3 * pixels, 'us_median': round(med['sym_to_u8'], 2),
             'us_min': round(lo['sym_to_u8'], 2), 'TB_per_s_read_and_written': round(3 * pixels / med['sym_to_u8'] / 1e6, 3),
             'TB_per_s_of_pixels': round(pixels / med['sym_to_u8'] / 1e6, 3), 'calls': KERNEL_CALLS}]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16, help='the second batch size (0: one image only)')
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--trace-dir', default=None, help='where the kernel trace goes (default: a fresh temporary directory)')
    ap.add_argument('--no-trace', action='store_true', help='skip the kernel trace (no rocprofv3 child)')
    ap.add_argument('--kernels-child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.kernels_child:
        return kernels_child()
    sys.path.insert(0, ROOT)
    import torch
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd import _lib
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    from l3c_pytorch_amd.helpers import config_parser, synthetic
    from l3c_pytorch_amd.native_codec import NativeCodec
    _lib.require_gpu()
    cfg = config_parser.parse_builtin('ms', 'cr')
    bp = MultiscaleBlueprint(cfg)
    bp.net.load_state_dict(synthetic.make_state_dict(cfg, 0, calibrated=True), strict=True)
    bp.set_eval()
    plain, sealed = NativeCodec(bp), NativeCodec(bp, seal=True)
    sealed.model_id()                                                    # hashed once per codec object: not part of a call
    clock = time.perf_counter

    rows = []
    for B in [1] + ([args.batch] if args.batch else []):
        imgs = torch.stack([synthetic.make_image(H, W, i, 'natural') for i in range(B)]).to(torch.uint8)          # on the host
        files = {'unsealed': plain.encode_batch(imgs), 'sealed': sealed.encode_batch(imgs)}
        assert [f[:-24] for f in files['sealed']] == files['unsealed']
        assert torch.equal(plain.decode_batch(files['sealed'])[0].cpu(), imgs)

        def encode(codec):
            def run():
                t0 = clock()
                dev = codec.encode_device(imgs)
                t1 = clock()
                out = codec.to_bytes(*dev)
                return t1 - t0, clock() - t0, out
            return run

        def decode(which):
            def run():
                t0 = clock()
                out, _ = plain.decode_batch(files[which])
                t1 = clock()
                out = out.cpu()
                return t1 - t0, clock() - t0, out
            return run

        for direction, legs in (('encode', [('unsealed', encode(plain)), ('sealed', encode(sealed)), ('unsealed again', encode(plain))]),
                                ('decode', [('unsealed', decode('unsealed')), ('sealed', decode('sealed')), ('unsealed again', decode('unsealed'))])):
            times = [([], []) for _ in legs]
            for it in range(args.warmup + args.runs):
                for k, (name, fn) in enumerate(legs):
                    torch.cuda.synchronize()
                    enq, done, out = fn()
                    assert (out == files[name.split()[0]]) if direction == 'encode' else torch.equal(out, imgs)
                    if it >= args.warmup:
                        times[k][0].append(enq * 1e3)
                        times[k][1].append(done * 1e3)
            for (name, _), (enq, done) in zip(legs, times):
                row = {'batch': B, 'direction': direction, 'leg': name, 'bytes': sum(len(f) for f in files[name.split()[0]]),
                       'enqueued_ms_median': round(statistics.median(enq), 3), 'done_ms_median': round(statistics.median(done), 3),
                       'done_ms_min': round(min(done), 3), 'runs': args.runs}
                rows.append(row)
                print(json.dumps(row), flush=True)
        del imgs
        torch.cuda.empty_cache()

    print('\n{:>6} {:>8} {:>16} {:>14} {:>12} {:>12}'.format('batch', 'dir', 'leg', 'enqueued ms', 'done ms', 'done min'))
    for r in rows:
        print('{:>6} {:>8} {:>16} {:>14.3f} {:>12.3f} {:>12.3f}'.format(r['batch'], r['direction'], r['leg'], r['enqueued_ms_median'],
                                                                        r['done_ms_median'], r['done_ms_min']))
    for i in range(0, len(rows), 3):
        a, s, b = (r['done_ms_median'] for r in rows[i:i + 3])
        print('batch {:>3} {}: sealed - mean(unsealed) = {:+.3f} ms = {:+.2%} of the unsealed leg; the unsealed legs differ by {:.3f} ms{}'.format(
            rows[i]['batch'], rows[i]['direction'], s - (a + b) / 2, (s - (a + b) / 2) / ((a + b) / 2), abs(a - b),
            '' if min(a, b) <= s <= max(a, b) else '  (outside their spread)'))
    if not args.no_trace:
        print()
        for row in kernel_rates(args.trace_dir):
            print(json.dumps(row), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
