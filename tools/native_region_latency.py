#!/usr/bin/env python
"""Latency of the region decode through the C ABI (NativeCodec.decode_region: l3c_decode_region_plan + l3c_decode_region) against the
Python host layer (Bitcoding.decode_region) on the same files, the method of tools/region_latency.py: one image of the calibrated
checkpoint, K = --bands (default 64), host to host -- the file's bytes -> uint8 pixels on the host, ending in a device synchronise -- for
512x768 and 2048x3072 (H x W), each with a box of 64 rows, of 256 rows (both in the middle of the image) and of all rows.

    A1   Bitcoding.decode_region
    B    NativeCodec.decode_region
    A2   Bitcoding.decode_region again: the spread between A1 and A2 is the yardstick for the difference between A and B

The three legs of a box run alternated in one process (A1, B, A2, A1, ...); median of --runs rounds after --warmup rounds of every leg of
every box of the shape.  Beside the median: the time after which everything is ENQUEUED (the decode call has returned; the device may
still be working).  Every leg is checked against the crop of the input before it is timed, and B's RegionInfo against A's.  Prints one
JSON object per row and a table at the end.

    python tools/native_region_latency.py
"""
import argparse
import json
import os
import statistics
import sys
import time


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--bands', type=int, default=64)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--shapes', default='512x768,2048x3072', help='comma-separated HxW')
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd import _lib
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    from l3c_pytorch_amd.helpers import config_parser, synthetic
    from l3c_pytorch_amd.native_codec import NativeCodec
    _lib.require_gpu()
    cfg = config_parser.parse_builtin('ms', 'cr')
    bp = MultiscaleBlueprint(cfg)
    bp.net.load_state_dict(synthetic.make_state_dict(cfg, 0, calibrated=True), strict=True)
    bp.set_eval()
    bc = Bitcoding(bp, bands=args.bands)
    nc = NativeCodec(bp, bands=args.bands)

    rows = []
    for shape in args.shapes.split(','):
        H, W = (int(v) for v in shape.split('x'))
        imgs = synthetic.make_image(H, W, 0, 'natural').unsqueeze(0)                      # uint8 on the host
        files = bc.encode_batch(imgs).to_bytes()
        infos = {}

        def leg(codec, key, box):
            def fn():
                out, infos[key] = codec.decode_region(files, box)
                t_enqueued = time.perf_counter()
                host = out.cpu()
                torch.cuda.synchronize()
                return host, t_enqueued
            assert torch.equal(fn()[0], imgs[:, :, box[0]:box[1]]), key
            return fn

        legs = []
        for name, box in (('64 rows', (H // 2 - 32, H // 2 + 32)), ('256 rows', (H // 2 - 128, H // 2 + 128)), ('all rows', (0, H))):
            legs += [(name, 'A1', leg(bc, (name, 'A'), box)), (name, 'B', leg(nc, (name, 'B'), box)), (name, 'A2', leg(bc, (name, 'A'), box))]
            assert infos[name, 'A'].as_dict() == infos[name, 'B'].as_dict(), name
        total, enq = {k[:2]: [] for k in legs}, {k[:2]: [] for k in legs}
        for it in range(args.warmup + args.runs):
            for name, which, fn in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, t_enqueued = fn()
                t1 = time.perf_counter()
                if it >= args.warmup:
                    total[name, which].append((t1 - t0) * 1e3)
                    enq[name, which].append((t_enqueued - t0) * 1e3)
        for name, which, _ in legs:
            info = infos[name, 'A']
            t = total[name, which]
            rows.append({'image': '{}x{}'.format(H, W), 'bands': args.bands, 'file_bytes': len(files[0]), 'box': name, 'leg': which,
                         'ms_median': round(statistics.median(t), 3), 'ms_min': round(min(t), 3), 'ms_max': round(max(t), 3),
                         'ms_enqueued_median': round(statistics.median(enq[name, which]), 3), 'runs': args.runs,
                         'bands_used': '{} of {}'.format(info.bands[1] - info.bands[0], info.n_bands),
                         'conv_rows': '{} of {}'.format(info.conv_rows[1] - info.conv_rows[0], info.frame_rows),
                         'decoder_rows': '{} of {}'.format(info.decoder_rows[1] - info.decoder_rows[0], info.frame_rows)})
            print(json.dumps(rows[-1]), flush=True)
        del legs, imgs, files
        torch.cuda.empty_cache()

    print('\n{:>10} {:>9} {:>4} {:>10} {:>9} {:>9} {:>12} {:>10} {:>13} {:>13}'.format('image', 'box', 'leg', 'median ms', 'min', 'max', 'enqueued ms',
                                                                                     'bands', 'conv rows', 'decoder rows'))
    for r in rows:
        print('{:>10} {:>9} {:>4} {:>10.2f} {:>9.2f} {:>9.2f} {:>12.2f} {:>10} {:>13} {:>13}'.format(
            r['image'], r['box'], r['leg'], r['ms_median'], r['ms_min'], r['ms_max'], r['ms_enqueued_median'], r['bands_used'], r['conv_rows'],
            r['decoder_rows']))
    # B against the two A legs of the same run: above either of them by more than they differ from each other?
    print()
    by = {(r['image'], r['box'], r['leg']): r['ms_median'] for r in rows}
    for image, box in [(r['image'], r['box']) for r in rows if r['leg'] == 'B']:
        a1, b, a2 = by[image, box, 'A1'], by[image, box, 'B'], by[image, box, 'A2']
        verdict = 'B at or below both A legs' if b <= min(a1, a2) else (
            'B ABOVE an A leg by more than the A legs differ' if b - min(a1, a2) > abs(a1 - a2) else 'B inside the spread of the A legs')
        print('{:>10} {:>9}: A1 {:.2f}  B {:.2f}  A2 {:.2f}  (A spread {:.2f}, B - min A {:+.2f}): {}'.format(image, box, a1, b, a2, abs(a1 - a2),
                                                                                                      b - min(a1, a2), verdict))
    return 0


if __name__ == '__main__':
    sys.exit(main())
