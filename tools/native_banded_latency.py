#!/usr/bin/env python
"""Latency of the BANDED codec through the Python schedule (Bitcoding(bands=K)) and through the library's own (NativeCodec(bands=K):
l3c_encode_batch_banded / l3c_decode_plan_banded + l3c_decode_batch_banded) on 768x512 images of the calibrated checkpoint, K = 64 bands,
host to host (the banded sibling of tools/native_codec_latency.py):

    encode   uint8 pixels on the host -> the files' bytes on the host     Bitcoding.encode_batch(...).to_bytes()  |  NativeCodec.encode_batch
    decode   the files' bytes on the host -> uint8 pixels on the host     Bitcoding.decode_batch(...).cpu()       |  NativeCodec.decode_batch(...).cpu()

for one image, the case the banded format exists for (and a batch with --batch N).  The legs of a direction run in one process, alternated -- Python, native, Python again:
the Python leg runs TWICE per round, so the two Python rows show the run-to-run spread a difference has to exceed.  Every leg reports two
times, medians of --runs rounds after --warmup: `enqueued` = until the call that enqueues the work has returned (read before anything
synchronises), `done` = until the result is on the host.  Prints one JSON object per row and a table at the end.

    python tools/native_banded_latency.py
"""
import argparse
import json
import os
import statistics
import sys
import time


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=0, help='a second batch size (0: one image only)')
    ap.add_argument('--bands', type=int, default=64)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
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
    bc, nc = Bitcoding(bp, bands=args.bands), NativeCodec(bp, bands=args.bands)
    H, W = 512, 768
    clock = time.perf_counter

    rows = []
    for B in [1] + ([args.batch] if args.batch else []):
        imgs = torch.stack([synthetic.make_image(H, W, i, 'natural') for i in range(B)]).to(torch.uint8)          # on the host
        files = bc.encode_batch(imgs).to_bytes()
        assert nc.encode_batch(imgs) == files
        assert torch.equal(nc.decode_batch(files)[0].cpu(), imgs)

        def py_encode():
            t0 = clock()
            enc = bc.encode_batch(imgs)
            t1 = clock()
            out = enc.to_bytes()
            return t1 - t0, clock() - t0, out

        def native_encode():
            t0 = clock()
            dev = nc.encode_device(imgs)
            t1 = clock()
            out = nc.to_bytes(*dev)
            return t1 - t0, clock() - t0, out

        def py_decode():
            t0 = clock()
            out, _ = bc.decode_batch(files, out_dtype=torch.uint8)
            t1 = clock()
            out = out.cpu()
            return t1 - t0, clock() - t0, out

        def native_decode():
            t0 = clock()
            out, _ = nc.decode_batch(files)
            t1 = clock()
            out = out.cpu()
            return t1 - t0, clock() - t0, out

        for direction, legs in (('encode', [('python', py_encode), ('native', native_encode), ('python again', py_encode)]),
                                ('decode', [('python', py_decode), ('native', native_decode), ('python again', py_decode)])):
            times = [([], []) for _ in legs]
            for it in range(args.warmup + args.runs):
                for k, (_, fn) in enumerate(legs):
                    torch.cuda.synchronize()
                    enq, done, out = fn()
                    assert (out == files) if direction == 'encode' else torch.equal(out, imgs)
                    if it >= args.warmup:
                        times[k][0].append(enq * 1e3)
                        times[k][1].append(done * 1e3)
            for (name, _), (enq, done) in zip(legs, times):
                row = {'batch': B, 'bands': args.bands, 'direction': direction, 'leg': name, 'bytes': sum(len(f) for f in files),
                       'enqueued_ms_median': round(statistics.median(enq), 3), 'done_ms_median': round(statistics.median(done), 3),
                       'done_ms_min': round(min(done), 3), 'runs': args.runs}
                rows.append(row)
                print(json.dumps(row), flush=True)
        del imgs
        torch.cuda.empty_cache()

    print('\n{:>6} {:>8} {:>14} {:>14} {:>12} {:>12}'.format('batch', 'dir', 'leg', 'enqueued ms', 'done ms', 'done min'))
    for r in rows:
        print('{:>6} {:>8} {:>14} {:>14.3f} {:>12.3f} {:>12.3f}'.format(r['batch'], r['direction'], r['leg'], r['enqueued_ms_median'],
                                                                        r['done_ms_median'], r['done_ms_min']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
