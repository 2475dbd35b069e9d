#!/usr/bin/env python
"""Latency of coding pictures AS THEY COME -- interleaved H x W x 3 host arrays of sizes that are no multiple of 8 -- host to host, by the
two routes a caller of NativeCodec has:

    leg A  the caller pads and crops with torch on the host:
           encode   permute + zero padding into a (B,3,Hp,Wp) batch + NativeCodec.encode_batch(batch, paddings)
           decode   NativeCodec.decode_batch + one D2H + crop + permute
    leg B  the library pads and crops on the device (l3c_encode_images / l3c_decode_images):
           encode   NativeCodec.encode_images(list, 'hwc')
           decode   NativeCodec.decode_images(files, 'hwc') + D2H of every image

on one 511 x 767 image and on a list of --batch (16) images of mixed sizes that share the 512 x 768 padded shape, calibrated checkpoint,
legacy format.  The legs of a direction run in one process, alternated -- A, B, A again: leg A runs TWICE per round, so its two rows show
the run-to-run spread a difference has to exceed.  Medians of --runs rounds after --warmup.  One JSON object per row, a table at the end.

    python tools/native_images_latency.py
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/native_images_latency.py --kernels

--kernels: nothing but l3c_u8_gather, l3c_u8_scatter and l3c_sym_to_u8 on 128 frames of 512 x 768 (151 MB of pixels), 10 launches each, for
a kernel trace of their own: gather from / scatter to RGB images of 511 x 767 and planar images of 512 x 768; the bytes a launch moves
(read + written) are printed for the division.
"""
import argparse
import json
import os
import statistics
import sys
import time


def kernels():
    import numpy as np
    import torch
    from l3c_pytorch_amd import _lib
    from l3c_pytorch_amd.native_codec import IMAGE_DTYPE, image_entry
    B, Hp, Wp = 128, 512, 768
    frames = torch.randint(0, 256, (B, 3, Hp, Wp), dtype=torch.uint8, device='cuda')
    out = torch.empty_like(frames)
    sym = torch.randint(0, 256, (B * 3 * Hp * Wp,), dtype=torch.int16, device='cuda')
    for name, layout, h, w in (('rgb 511x767', 'hwc', 511, 767), ('planar 512x768', 'chw', 512, 768)):
        table = np.zeros(B, dtype=IMAGE_DTYPE)
        n = 3 * h * w
        for b in range(B):
            table[b] = image_entry(layout, (3, h, w) if layout == 'chw' else (h, w, 3), b * n, (Hp - h) // 2, (Wp - w) // 2)
        tab = torch.from_numpy(table.view(np.uint8)).cuda()
        buf = torch.randint(0, 256, (B * n,), dtype=torch.uint8, device='cuda')
        for _ in range(10):
            _lib.call('l3c_u8_gather', buf.data_ptr(), B * n, table.ctypes.data, tab.data_ptr(), B, Hp, Wp, out.data_ptr(), None, _lib.stream())
        for _ in range(10):
            _lib.call('l3c_u8_scatter', frames.data_ptr(), B, Hp, Wp, buf.data_ptr(), B * n, table.ctypes.data, tab.data_ptr(), _lib.stream())
        torch.cuda.synchronize()
        print(json.dumps({'kernels': name, 'gather_bytes_per_launch': B * n + frames.numel(), 'scatter_bytes_per_launch': 2 * B * n}), flush=True)
    for _ in range(10):
        _lib.call('l3c_sym_to_u8', sym.data_ptr(), sym.numel(), out.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    print(json.dumps({'kernels': 'l3c_sym_to_u8', 'bytes_per_launch': 3 * sym.numel()}), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16, help='images in the list (0: one image only)')
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--kernels', action='store_true', help='only the two kernels and l3c_sym_to_u8, for a kernel trace')
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd import _lib
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    from l3c_pytorch_amd.helpers import config_parser, pad, synthetic
    from l3c_pytorch_amd.native_codec import NativeCodec
    _lib.require_gpu()
    if args.kernels:
        return kernels()
    cfg = config_parser.parse_builtin('ms', 'cr')
    bp = MultiscaleBlueprint(cfg)
    bp.net.load_state_dict(synthetic.make_state_dict(cfg, 0, calibrated=True), strict=True)
    bp.set_eval()
    nc = NativeCodec(bp)
    Hp, Wp = 512, 768
    clock = time.perf_counter
    rng = np.random.RandomState(0)

    rows = []
    workloads = [('one 511x767', [(511, 767)])]
    if args.batch:
        workloads.append(('{} mixed -> 512x768'.format(args.batch), [(int(rng.randint(505, 513)), int(rng.randint(761, 769))) for _ in range(args.batch)]))
    for name, sizes in workloads:
        B = len(sizes)
        # H x W x 3 host arrays, as an image reader hands them over
        imgs = [synthetic.make_image(Hp, Wp, i, 'natural').to(torch.uint8)[:, :h, :w].permute(1, 2, 0).contiguous() for i, (h, w) in enumerate(sizes)]
        pads = [pad.padding_for(h, w, 8) for h, w in sizes]

        def a_encode():
            t0 = clock()
            batch = torch.zeros(B, 3, Hp, Wp, dtype=torch.uint8)
            for b, (im, (left, _, top, _)) in enumerate(zip(imgs, pads)):
                batch[b, :, top:top + im.shape[0], left:left + im.shape[1]] = im.permute(2, 0, 1)
            out = nc.encode_batch(batch, pads)
            return clock() - t0, out

        def b_encode():
            t0 = clock()
            out = nc.encode_images(imgs, layout='hwc', max_batch=max(B, 1))
            return clock() - t0, out

        files = a_encode()[1]
        assert b_encode()[1] == files

        def a_decode():
            t0 = clock()
            pixels, got = nc.decode_batch(files)
            host = pixels.cpu()
            out = [pad.undo_pad(host[b:b + 1], *got[b])[0].permute(1, 2, 0).contiguous() for b in range(B)]
            return clock() - t0, out

        def b_decode():
            t0 = clock()
            out = [t.cpu() for t in nc.decode_images(files, layout='hwc', max_batch=max(B, 1))]
            return clock() - t0, out

        for direction, legs in (('encode', [('A torch pad', a_encode), ('B library', b_encode), ('A again', a_encode)]),
                                ('decode', [('A torch crop', a_decode), ('B library', b_decode), ('A again', a_decode)])):
            times = [[] for _ in legs]
            for it in range(args.warmup + args.runs):
                for k, (_, fn) in enumerate(legs):
                    torch.cuda.synchronize()
                    done, out = fn()
                    assert (out == files) if direction == 'encode' else all(torch.equal(o, im) for o, im in zip(out, imgs))
                    if it >= args.warmup:
                        times[k].append(done * 1e3)
            for (leg, _), done in zip(legs, times):
                row = {'workload': name, 'direction': direction, 'leg': leg, 'pixels': sum(h * w for h, w in sizes),
                       'done_ms_median': round(statistics.median(done), 3), 'done_ms_min': round(min(done), 3), 'runs': args.runs}
                rows.append(row)
                print(json.dumps(row), flush=True)

    print('\n{:>22} {:>8} {:>14} {:>12} {:>12}'.format('workload', 'dir', 'leg', 'done ms', 'done min'))
    for r in rows:
        print('{:>22} {:>8} {:>14} {:>12.3f} {:>12.3f}'.format(r['workload'], r['direction'], r['leg'], r['done_ms_median'], r['done_ms_min']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
