#!/usr/bin/env python
"""One-image latency of the legacy and the banded `.l3c` format (Bitcoding(bands=K)), host to host, on the calibrated checkpoint:

    encode  uint8 (3, 512, 768) on the host -> the file's bytes on the host
    decode  the file's bytes -> uint8 pixels on the host

Median of --runs runs after --warmup, for the legacy format and every K of --bands, with each K's file size relative to the legacy file;
then, for information, batch-8 and batch-128 decodes.  Prints one JSON object per row and a table at the end.

    python tools/banded_latency.py                        # legacy + K in 16 32 64 128 256
    python tools/banded_latency.py --root OLD_TREE --bands   # the legacy rows only, with another checkout's package (APIs of that tree)
"""
import argparse
import json
import os
import statistics
import sys
import time


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help='tree whose l3c_pytorch_amd package is measured')
    ap.add_argument('--bands', type=int, nargs='*', default=[16, 32, 64, 128, 256], help='band counts (none: legacy rows only)')
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batches', type=int, nargs='*', default=[8, 128], help='batch decodes for information')
    ap.add_argument('--batch-bands', type=int, default=64, help='band count of the batch decodes (0: legacy only)')
    ap.add_argument('--tag', default='')
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    from l3c_pytorch_amd.helpers import config_parser, synthetic
    cfg = config_parser.parse_builtin('ms', 'cr')
    bp = MultiscaleBlueprint(cfg)
    bp.net.load_state_dict(synthetic.make_state_dict(cfg, 0, calibrated=True), strict=True)
    bp.set_eval()
    img = synthetic.make_image(512, 768, 0, 'natural').unsqueeze(0)          # uint8 on the host

    def timed(fn, runs, warmup):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts) * 1e3, min(ts) * 1e3

    rows, legacy_bytes = [], None
    for K in [0] + list(args.bands):
        bc = Bitcoding(bp, bands=K) if K else Bitcoding(bp)
        data = bc.encode_batch(img).to_bytes()[0]
        enc_ms, enc_min = timed(lambda: bc.encode_batch(img).to_bytes()[0], args.runs, args.warmup)

        def dec():
            out, _ = bc.decode_batch([data], out_dtype=torch.uint8)
            return out.cpu()
        assert torch.equal(dec()[0], img[0]), K
        dec_ms, dec_min = timed(dec, args.runs, args.warmup)
        if not K:
            legacy_bytes = len(data)
        row = {'tag': args.tag, 'format': 'banded' if K else 'legacy', 'bands': K, 'bytes': len(data),
               'size_vs_legacy': len(data) / float(legacy_bytes), 'encode_ms_median': round(enc_ms, 3), 'encode_ms_min': round(enc_min, 3),
               'decode_ms_median': round(dec_ms, 3), 'decode_ms_min': round(dec_min, 3), 'runs': args.runs}
        rows.append(row)
        print(json.dumps(row), flush=True)
    for B in args.batches:
        imgs = torch.stack([synthetic.make_image(512, 768, 100 + i, 'natural') for i in range(B)])
        for K in [0] + ([args.batch_bands] if args.batch_bands and args.bands else []):
            bc = Bitcoding(bp, bands=K) if K else Bitcoding(bp)
            files = bc.encode_batch(imgs).to_bytes()

            def dec_b():
                out, _ = bc.decode_batch(files, out_dtype=torch.uint8)
                return out.cpu()
            assert torch.equal(dec_b(), imgs)
            ms, mn = timed(dec_b, 3, 1)
            row = {'tag': args.tag, 'format': 'banded' if K else 'legacy', 'bands': K, 'batch': B, 'decode_ms_median': round(ms, 2),
                   'decode_mpix_s': round(B * 512 * 768 / (ms * 1e3), 1)}
            print(json.dumps(row), flush=True)
            del files
        del imgs
        torch.cuda.empty_cache()
    print('\n{:>8} {:>8} {:>10} {:>12} {:>12}'.format('format', 'K', 'size', 'encode ms', 'decode ms'))
    for r in rows:
        print('{:>8} {:>8} {:>10.4f} {:>12.2f} {:>12.2f}'.format(r['format'], r['bands'], r['size_vs_legacy'], r['encode_ms_median'],
                                                               r['decode_ms_median']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
