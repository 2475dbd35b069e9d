#!/usr/bin/env python
"""Latency and quality of the preview decode (Bitcoding.decode_preview) on 768x512 images of the calibrated checkpoint, host to host:

    full      the file's bytes -> uint8 pixels on the host                                (decode_batch)
    preview   the PREFIX holding the first r of the 4 scale records -> uint8 pixels       (decode_preview, r = 3, 2, 1)

for the legacy format and banded files (--bands, default 64), one image and a batch (--batch, default 16).  All legs of a batch size run
in one process, alternated (leg 1, leg 2, ..., leg 1, ...); median of --runs rounds after --warmup.  Each leg reports its prefix's share
of the file and its PSNR against the input.  Then the HIP-event times of dmll_mean_kernel and encode_intervals_kernel on the same
RGB-scale P (the same 480 bytes read per pixel), alternated, as bytes over time against the 8.0 TB/s HBM peak of the MI355X.  Prints one
JSON object per row and a table at the end.

    python tools/preview_latency.py
"""
import argparse
import json
import os
import statistics
import sys
import time

HBM_PEAK = 8.0e12        # bytes / s, HBM3E spec (6.3e12 measured with a float4 copy)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--bands', type=int, default=64, help='band count of the banded legs (0: legacy only)')
    ap.add_argument('--batch', type=int, default=16, help='the second batch size (0: one image only)')
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--kernel-launches', type=int, default=50, help='launches per timed window of the kernel rows')
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd import _lib, ops
    from l3c_pytorch_amd.bitcoding import container
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    from l3c_pytorch_amd.helpers import config_parser, synthetic
    _lib.require_gpu()
    cfg = config_parser.parse_builtin('ms', 'cr')
    bp = MultiscaleBlueprint(cfg)
    bp.net.load_state_dict(synthetic.make_state_dict(cfg, 0, calibrated=True), strict=True)
    bp.set_eval()
    H, W = 512, 768

    def psnr(a, b):
        mse = float(((a.double() - b.double()) ** 2).mean())
        return 10 * np.log10(255.0 ** 2 / mse) if mse else float('inf')

    rows = []
    for B in [1] + ([args.batch] if args.batch else []):
        imgs = torch.stack([synthetic.make_image(H, W, i, 'natural') for i in range(B)])          # uint8 on the host
        legs = []
        for K in [0] + ([args.bands] if args.bands else []):
            bc = Bitcoding(bp, bands=K) if K else Bitcoding(bp)
            files = bc.encode_batch(imgs).to_bytes()
            total = bc.n_predicted_scales() + 1
            size = sum(len(f) for f in files)

            def full(bc=bc, files=files):
                return bc.decode_batch(files, out_dtype=torch.uint8)[0].cpu()
            assert torch.equal(full(), imgs)
            legs.append({'format': 'banded' if K else 'legacy', 'bands': K, 'leg': 'full', 'records': total, 'fn': full, 'bytes': size,
                         'share': 1.0})
            for r in (total - 1, total - 2, 1):
                pieces = [f[:container.prefix_bytes(f, r)] for f in files]

                def preview(bc=bc, pieces=pieces, r=r):
                    return bc.decode_preview(pieces, records=r)[0].cpu()
                legs.append({'format': 'banded' if K else 'legacy', 'bands': K, 'leg': 'preview', 'records': r, 'fn': preview,
                             'bytes': sum(len(p) for p in pieces), 'share': sum(len(p) for p in pieces) / float(size)})
        for leg in legs:
            leg['psnr'] = psnr(leg['fn'](), imgs)
            leg['ms'] = []
        for it in range(args.warmup + args.runs):
            for leg in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg['fn']()
                if it >= args.warmup:
                    leg['ms'].append((time.perf_counter() - t0) * 1e3)
        for leg in legs:
            row = {'batch': B, 'format': leg['format'], 'bands': leg['bands'], 'leg': leg['leg'], 'records_decoded': leg['records'],
                   'bytes_read': leg['bytes'], 'share_of_file': round(leg['share'], 4), 'psnr_db': round(leg['psnr'], 2),
                   'ms_median': round(statistics.median(leg['ms']), 3), 'ms_min': round(min(leg['ms']), 3), 'runs': args.runs}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del legs, imgs
        torch.cuda.empty_cache()

    # ---- the two head kernels on the same RGB-scale P: bytes read (4 Kp per pixel) + written over HIP-event time
    C, Kmix = 3, cfg.prob.K
    Kp = 4 * C * Kmix
    dmll = bp.losses.loss_dmol_rgb
    targets = dmll.coding_targets('cuda')
    krows = []
    for B in [1] + ([args.batch] if args.batch else []):
        imgs = torch.stack([synthetic.make_image(H, W, i, 'natural') for i in range(B)])
        out = bp.net(imgs.to('cuda', torch.float32))
        P, sym = out.raw.P[0], out.raw.sym[0].contiguous()
        assert tuple(P.shape) == (B, H, W, Kp)
        del out
        n = args.kernel_launches
        kernels = {'dmll_mean_kernel': (lambda: ops.dmll_mean(P, C, Kmix, True, dmll.x_min, dmll.x_max, dmll.L), 4 * Kp + 2 * C),
                   'encode_intervals_kernel': (lambda: ops.dmll_encode_intervals(P, sym, targets, C, Kmix, True), 4 * Kp + 2 * C + 8 * C)}
        times = {k: [] for k in kernels}
        for it in range(2 + 5):
            for name, (fn, _) in kernels.items():
                fn()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(n):
                    fn()
                b.record()
                torch.cuda.synchronize()
                if it >= 2:
                    times[name].append(a.elapsed_time(b) / n)          # (includes the output tensor's cached allocation: microseconds)
        for name, (_, per_pixel) in kernels.items():
            ms = statistics.median(times[name])
            nbytes = B * H * W * per_pixel
            row = {'kernel': name, 'batch': B, 'P_bytes': B * H * W * 4 * Kp, 'bytes_moved': nbytes, 'ms_per_launch': round(ms, 4),
                   'TB_s': round(nbytes / (ms * 1e-3) / 1e12, 3), 'share_of_hbm_peak': round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}
            krows.append(row)
            print(json.dumps(row), flush=True)
        del P, sym, imgs
        torch.cuda.empty_cache()

    print('\n{:>6} {:>8} {:>8} {:>8} {:>10} {:>8} {:>10}'.format('batch', 'format', 'leg', 'records', 'share', 'PSNR', 'ms'))
    for r in rows:
        print('{:>6} {:>8} {:>8} {:>8} {:>10.4f} {:>8.2f} {:>10.2f}'.format(r['batch'], r['format'], r['leg'], r['records_decoded'],
                                                                           r['share_of_file'], r['psnr_db'], r['ms_median']))
    print('\n{:>26} {:>6} {:>12} {:>8} {:>10}'.format('kernel', 'batch', 'ms / launch', 'TB/s', 'of 8 TB/s'))
    for r in krows:
        print('{:>26} {:>6} {:>12.4f} {:>8.3f} {:>10.3f}'.format(r['kernel'], r['batch'], r['ms_per_launch'], r['TB_s'], r['share_of_hbm_peak']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
