#!/usr/bin/env python
"""Latency of the region decode (Bitcoding.decode_region) on banded files of the calibrated checkpoint, host to host: the file's bytes ->
uint8 pixels on the host, for one 512x768 (H x W) and one 2048x3072 image, K = --bands (default 64):

    full A / B   decode_batch, twice per round: the spread between the two is the yardstick for every other difference
    preview      decode_preview from 3 of the 4 scale records: what a region cannot go below (it decodes those records too)
    region 64    decode_region of 64 rows in the middle of the image
    region 256   decode_region of 256 rows in the middle
    region all   decode_region of every row (the entries path where decode_batch takes l3c_decode_rgb_banded)

All legs of an image run in one process, alternated (leg 1, leg 2, ..., leg 1, ...); median of --runs rounds after --warmup.  Every region
leg is checked against the crop of the input before it is timed.  Prints one JSON object per row and a table at the end.

    python tools/region_latency.py
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
    from l3c_pytorch_amd.bitcoding import container
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    from l3c_pytorch_amd.helpers import config_parser, synthetic
    _lib.require_gpu()
    cfg = config_parser.parse_builtin('ms', 'cr')
    bp = MultiscaleBlueprint(cfg)
    bp.net.load_state_dict(synthetic.make_state_dict(cfg, 0, calibrated=True), strict=True)
    bp.set_eval()
    bc = Bitcoding(bp, bands=args.bands)
    total = bc.n_predicted_scales() + 1

    rows = []
    for shape in args.shapes.split(','):
        H, W = (int(v) for v in shape.split('x'))
        imgs = synthetic.make_image(H, W, 0, 'natural').unsqueeze(0)                      # uint8 on the host
        files = bc.encode_batch(imgs).to_bytes()
        prefix = [f[:container.prefix_bytes(f, total - 1)] for f in files]
        infos = {}

        def full():
            return bc.decode_batch(files, out_dtype=torch.uint8)[0].cpu()

        def preview():
            return bc.decode_preview(prefix, records=total - 1)[0].cpu()

        def region_leg(name, box):
            def fn():
                out, infos[name] = bc.decode_region(files, box)
                return out.cpu()
            assert torch.equal(fn(), imgs[:, :, box[0]:box[1]]), name
            return fn

        assert torch.equal(full(), imgs)
        legs = [('full A', full), ('full B', full), ('preview {}/{}'.format(total - 1, total), preview),
                ('region 64', region_leg('region 64', (H // 2 - 32, H // 2 + 32))),
                ('region 256', region_leg('region 256', (H // 2 - 128, H // 2 + 128))),
                ('region all', region_leg('region all', (0, H)))]
        ms = {name: [] for name, _ in legs}
        for it in range(args.warmup + args.runs):
            for name, fn in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if it >= args.warmup:
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        for name, _ in legs:
            info = infos.get(name)
            row = {'image': '{}x{}'.format(H, W), 'bands': args.bands, 'file_bytes': len(files[0]), 'leg': name,
                   'ms_median': round(statistics.median(ms[name]), 3), 'ms_min': round(min(ms[name]), 3), 'ms_max': round(max(ms[name]), 3),
                   'runs': args.runs}
            if info is not None:
                row.update(bands_used='{} of {}'.format(info.bands[1] - info.bands[0], info.n_bands),
                           conv_rows='{} of {}'.format(info.conv_rows[1] - info.conv_rows[0], info.frame_rows),
                           bytes_used=info.bytes_used, bytes_total=info.bytes_total)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del legs, imgs, files
        torch.cuda.empty_cache()

    print('\n{:>10} {:>14} {:>10} {:>10} {:>10} {:>12} {:>14} {:>22}'.format('image', 'leg', 'median ms', 'min', 'max', 'bands', 'conv rows',
                                                                              'finest-record bytes'))
    for r in rows:
        print('{:>10} {:>14} {:>10.2f} {:>10.2f} {:>10.2f} {:>12} {:>14} {:>22}'.format(
            r['image'], r['leg'], r['ms_median'], r['ms_min'], r['ms_max'], r.get('bands_used', ''), r.get('conv_rows', ''),
            '{} of {}'.format(r['bytes_used'], r['bytes_total']) if 'bytes_used' in r else ''))
    return 0


if __name__ == '__main__':
    sys.exit(main())
