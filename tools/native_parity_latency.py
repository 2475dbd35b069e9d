#!/usr/bin/env python
"""What a parity-sealed file costs through the native codec (l3c_encode_batch_banded_parity: the whole tail assembled on the device,
INTEGRATION.md "Parity-sealed files through the C ABI") beside the band-sealed native encode, and beside the same files through Bitcoding
(the tail built per file on the host), on the calibrated checkpoint, host to host.

    python tools/native_parity_latency.py [--images 1] [--runs 20] [--warmup 3]

--images 768x512 images (1, or a batch of 16), K = 64 bands, G = 16: the images' bytes on the host -> the files on the host.  The legs run in
ONE process, alternated; each family's baseline leg runs TWICE per round -- its two rows show the run-to-run spread a difference has to exceed:

    native      NativeCodec(seal='bands') | parity=16 | parity=16, parity_streams=2 | parity=16, parity_streams=2, parity_head=True |
                NativeCodec(seal='bands') again
    Bitcoding   Bitcoding(seal='bands') | the same three settings | Bitcoding(seal='bands') again

Every native file is compared with Bitcoding's, byte for byte, before anything is reported.  Medians of --runs rounds after --warmup.  Prints
one JSON object per row, a table, and per setting the excess over the mean of its family's two baseline legs beside their spread."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, K, G = 512, 768, 64, 16
SETTINGS = [('parity=16', dict(parity=G)), ('parity=16, R = 2', dict(parity=G, parity_streams=2)),
            ('parity=16, R = 2, head', dict(parity=G, parity_streams=2, parity_head=True))]


def setup(n_images):
    sys.path.insert(0, ROOT)
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
    native = {'bands': NativeCodec(bp, bands=K, seal='bands')}
    python = {'bands': Bitcoding(bp, bands=K, seal='bands')}
    for name, kw in SETTINGS:
        native[name] = NativeCodec(bp, bands=K, seal='bands', **kw)
        python[name] = Bitcoding(bp, bands=K, seal='bands', **kw)
    for c in list(native.values()) + list(python.values()):
        c.model_id()                                                     # hashed once per object: not part of a call
    images = torch.stack([synthetic.make_image(H, W, b, 'natural').to(torch.uint8) for b in range(n_images)])          # on the host
    return torch, native, python, images


def alternate(legs, runs, warmup, sync):
    """legs: [(name, fn -> seconds)] run alternately -> per leg the list of milliseconds."""
    times = [[] for _ in legs]
    for it in range(warmup + runs):
        for k, (name, fn) in enumerate(legs):
            sync()
            t = fn()
            if it >= warmup:
                times[k].append(t * 1e3)
    return times


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=1)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args(argv)
    torch, native, python, img = setup(args.images)
    clock = time.perf_counter
    B = args.images
    pads, made = [(0, 0, 0, 0)] * B, {}

    def native_leg(key, name):
        def run():
            t0 = clock()
            made['native', key] = native[key].encode_batch(img.cuda())
            return clock() - t0
        return 'native, ' + name, run

    def python_leg(key, name):
        def run():
            t0 = clock()
            made['python', key] = python[key].encode_batch(img.cuda()).to_bytes(pads)
            return clock() - t0
        return 'Bitcoding, ' + name, run
    legs = []
    for leg in (native_leg, python_leg):
        legs += [leg('bands', "seal='bands'")] + [leg(name, name) for name, _ in SETTINGS] + [leg('bands', "seal='bands' again")]
    times = alternate(legs, args.runs, args.warmup, torch.cuda.synchronize)
    sizes = {}
    for key in ['bands'] + [name for name, _ in SETTINGS]:
        if made['native', key] != made['python', key]:
            sys.exit('the native files differ from Bitcoding\'s: ' + key)
        sizes[key] = sum(len(f) for f in made['native', key])
    rows = []
    for (name, _), t in zip(legs, times):
        rows.append({'images': B, 'leg': name, 'ms_median': round(statistics.median(t), 3), 'ms_min': round(min(t), 3), 'ms_max': round(max(t), 3),
                     'runs': args.runs})
        print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({'images': B, 'file_bytes': sizes}), flush=True)
    print('\n{:>48} {:>12} {:>10} {:>10}'.format('leg', 'median ms', 'min ms', 'max ms'))
    for r in rows:
        print('{:>48} {:>12.3f} {:>10.3f} {:>10.3f}'.format(r['leg'], r['ms_median'], r['ms_min'], r['ms_max']))
    t = {r['leg']: r['ms_median'] for r in rows}
    excess = {}
    for family in ('native', 'Bitcoding'):
        a, b = t[family + ", seal='bands'"], t[family + ", seal='bands' again"]
        print("{}: the two seal='bands' legs differ by {:.3f} ms (mean {:.3f} ms)".format(family, abs(a - b), (a + b) / 2))
        for name, _ in SETTINGS:
            excess[family, name] = t['{}, {}'.format(family, name)] - (a + b) / 2
            print('{}: {} - mean(seal=\'bands\') = {:+.3f} ms; files x{:.4f} ({} -> {} bytes)'.format(
                family, name, excess[family, name], sizes[name] / sizes['bands'], sizes['bands'], sizes[name]))
    for name, _ in SETTINGS:
        n, p = excess['native', name], excess['Bitcoding', name]
        print('{}: native excess {:+.3f} ms, Bitcoding excess {:+.3f} ms: the native path is {}'.format(
            name, n, p, 'below the Python path' if n < p else 'NOT below the Python path'))
    return 0


if __name__ == '__main__':
    sys.exit(main())
