#!/usr/bin/env python
"""What a salvage decode costs beside decode_batch (INTEGRATION.md "Salvage decode"), on the calibrated checkpoint, host to host.

    python tools/salvage_latency.py [--runs 20] [--warmup 3] [--band 30]

One 768x512 image, K = 64 bands, band-sealed, through NativeCodec(bp, bands=64): the file's bytes on the host -> uint8 pixels on the host.
The legs run in ONE process, alternated, the decode_batch leg TWICE per round -- its two rows show the run-to-run spread a difference has to
exceed:

    decode_batch                       the intact file
    decode_salvage, intact             the intact file: the same decode with the symbols kept, the same band CRCs, no conceal launch
    decode_salvage, one band damaged   all three streams of band --band complemented: the band is concealed
    decode_batch(verify=False), damaged  the same damaged file decoded and nothing checked: what the range decoder costs on a garbage stream
    decode_batch again

Medians of --runs rounds after --warmup.  Then the PSNR of the concealed rows against the input (and of flat grey on the same rows, for
scale), and the conceal kernel alone from HIP events: ops.dmll_conceal on one band of a 768x512 P (three channels and G alone) and on the
whole frame, medians of --runs calls.  Prints one JSON object per row and a table at the end."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, K = 512, 768, 64


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float('inf') if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--band', type=int, default=30, help='the band whose three streams are complemented')
    args = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd import _lib, ops
    from l3c_pytorch_amd.bitcoding import container
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    from l3c_pytorch_amd.helpers import config_parser, synthetic
    from l3c_pytorch_amd.native_codec import NativeCodec
    _lib.require_gpu()
    cfg = config_parser.parse_builtin('ms', 'cr')
    bp = MultiscaleBlueprint(cfg)
    bp.net.load_state_dict(synthetic.make_state_dict(cfg, 0, calibrated=True), strict=True)
    bp.set_eval()
    codec = NativeCodec(bp, bands=K, seal='bands')
    codec.model_id()                                                       # hashed once per codec object: not part of a call
    img = synthetic.make_image(H, W, 0, 'natural').to(torch.uint8).unsqueeze(0)          # on the host
    intact = codec.encode_batch(img)
    body = container.split_seal(intact[0])[0]
    parsed = container.parse_banded(body)
    data = np.frombuffer(intact[0], dtype=np.uint8).copy()
    for c in range(3):
        a, n = int(parsed.offset[-1][c, args.band]), int(parsed.nbytes[-1][c, args.band])
        data[a:a + n] ^= 0xFF
    damaged = [data.tobytes()]
    L = container.split_seal(intact[0])[1].band_len
    clock = time.perf_counter
    infos = {}

    def leg_batch():
        t0 = clock()
        out = codec.decode_batch(intact)[0].cpu()
        return clock() - t0, out

    def leg_unverified():
        t0 = clock()
        out = codec.decode_batch(damaged, verify=False)[0].cpu()
        return clock() - t0, out

    def leg_salvage(name, files):
        def run():
            t0 = clock()
            out, _, info = codec.decode_salvage(files)
            out = out.cpu()
            infos[name] = info
            return clock() - t0, out
        return run
    legs = [('decode_batch', leg_batch), ('decode_salvage, intact', leg_salvage('intact', intact)),
            ('decode_salvage, one band damaged', leg_salvage('damaged', damaged)), ('decode_batch(verify=False), damaged', leg_unverified),
            ('decode_batch again', leg_batch)]
    times = [[] for _ in legs]
    outs = {}
    for it in range(args.warmup + args.runs):
        for k, (name, fn) in enumerate(legs):
            torch.cuda.synchronize()
            t, out = fn()
            outs[name] = out
            if 'damaged' not in name and not torch.equal(out, img):
                sys.exit('pixels differ: ' + name)
            if it >= args.warmup:
                times[k].append(t * 1e3)
    assert infos['intact'].concealed == {} and infos['intact'].lost == []
    assert infos['damaged'].concealed == {0: [(c, args.band) for c in range(3)]}, infos['damaged']
    rows = []
    for (name, _), t in zip(legs, times):
        rows.append({'leg': name, 'file_bytes': len(intact[0]), 'ms_median': round(statistics.median(t), 3), 'ms_min': round(min(t), 3),
                     'ms_max': round(max(t), 3), 'runs': args.runs})
        print(json.dumps(rows[-1]), flush=True)

    # the concealed rows against the input
    got = outs['decode_salvage, one band damaged']
    flat = lambda t: t.reshape(3, -1)       # noqa: E731
    lo, hi = args.band * L, min((args.band + 1) * L, H * W)
    outside = torch.ones(H * W, dtype=torch.bool)
    outside[lo:hi] = False
    assert torch.equal(flat(got[0])[:, outside], flat(img[0])[:, outside])
    y0, y1 = infos['damaged'].rows[0]
    q = {'what': 'concealed band', 'band': args.band, 'rows': [y0, y1], 'pixels': hi - lo,
         'psnr_db_concealed': round(psnr(flat(got[0])[:, lo:hi], flat(img[0])[:, lo:hi]), 2),
         'psnr_db_flat_grey': round(psnr(torch.full((3, hi - lo), 128.0), flat(img[0])[:, lo:hi]), 2),
         'psnr_db_per_channel': [round(psnr(flat(got[0])[c, lo:hi], flat(img[0])[c, lo:hi]), 2) for c in range(3)]}
    print(json.dumps(q), flush=True)

    # the kernel alone, from HIP events
    Kmix = cfg.prob.K
    loss = bp.losses.loss_dmol_rgb
    g = torch.Generator(device='cuda').manual_seed(0)
    P = torch.randn(1, H, W, 12 * Kmix, generator=g, device='cuda')
    sym = torch.randint(0, 256, (1, 3, H, W), generator=g, device='cuda').to(torch.int16)
    kernel_rows = []
    for what, spans in (('one band, three channels', [(0, lo, hi - lo, 7)]), ('one band, G alone', [(0, lo, hi - lo, 2)]),
                        ('the whole frame, three channels', [(0, j * L, min(L, H * W - j * L), 7) for j in range(container.n_bands(H * W, L))])):
        table = ops.conceal_spans(spans)
        us = []
        for it in range(args.warmup + args.runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            table_d = ops.upload_small(table.view(np.int64))
            torch.cuda.synchronize()
            a.record()
            _lib.call('l3c_dmll_conceal', ops.ptr(P), 1, H * W, Kmix, float(loss.x_min), float(loss.x_max), int(loss.L), table.ctypes.data,
                      ops.ptr(table_d), len(table), ops.ptr(sym), ops.stream())
            b.record()
            b.synchronize()
            if it >= args.warmup:
                us.append(a.elapsed_time(b) * 1e3)
        pixels = int(table['npix'].sum())
        kernel_rows.append({'kernel': 'dmll_conceal_kernel', 'what': what, 'spans': len(table), 'pixels': pixels, 'P_bytes': pixels * 12 * Kmix * 4,
                            'us_median': round(statistics.median(us), 2), 'us_min': round(min(us), 2), 'us_max': round(max(us), 2), 'calls': args.runs})
        print(json.dumps(kernel_rows[-1]), flush=True)

    print('\n{:>36} {:>12} {:>10} {:>10}'.format('leg', 'median ms', 'min ms', 'max ms'))
    for r in rows:
        print('{:>36} {:>12.3f} {:>10.3f} {:>10.3f}'.format(r['leg'], r['ms_median'], r['ms_min'], r['ms_max']))
    a, s, d, u, b = (r['ms_median'] for r in rows)
    print('decode_salvage on the intact file - mean(decode_batch) = {:+.3f} ms; the decode_batch legs differ by {:.3f} ms{}'.format(
        s - (a + b) / 2, abs(a - b), '' if min(a, b) <= s <= max(a, b) else '  (outside their spread)'))
    print('decode_salvage with one damaged band - mean(decode_batch) = {:+.3f} ms; - decode_batch(verify=False) of the same file = {:+.3f} ms'.format(
        d - (a + b) / 2, d - u))
    print('concealed rows [{}, {}): {} dB (flat grey: {} dB)'.format(y0, y1, q['psnr_db_concealed'], q['psnr_db_flat_grey']))
    for r in kernel_rows:
        print('{:>36}: {:.2f} us (HIP events, median of {})'.format(r['what'], r['us_median'], r['calls']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
