#!/usr/bin/env python
"""What parity bands cost and what a repair costs (INTEGRATION.md "Parity bands"), on the calibrated checkpoint, host to host.

    python tools/repair_latency.py [--runs 20] [--warmup 3] [--band 30] [--batch 16]
    python tools/repair_latency.py --kernels      the two kernels alone, from a `rocprofv3 --kernel-trace` run of its own

768x512 images, K = 64 bands, G = 16, through Bitcoding: the images' bytes on the host -> files on the host, and the files' bytes on the host
-> uint8 pixels on the host.  The legs run in ONE process, alternated, the baseline leg TWICE per round -- its two rows show the run-to-run
spread a difference has to exceed:

    encode                 parity=0 | parity=16 | parity=0 again; and the file-size ratio
    decode, intact         decode_batch | decode_repair | decode_batch again          (decode_repair makes decode_salvage's library calls)
    decode, damaged        decode_salvage | decode_repair on the file with the R payload of band --band complemented

for one image and for a batch of --batch (every file of the batch damaged in the damaged legs).  Medians of --runs rounds after --warmup.
--kernels: l3c_band_parity on the coder output of one image's finest record, l3c_u8_xor_spans folding the same groups from the uploaded
streams, and l3c_container_read cutting the same streams out of the file (the yardstick: the project's other streaming kernel over these
bytes), kernel times from the trace, rates in bytes read + written per second.  Prints one JSON object per row and a table at the end."""
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
H, W, K, G = 512, 768, 64, 16
KERNEL_WARMUP, KERNEL_CALLS = 5, 20
KERNELS = ('band_parity_kernel', 'u8_xor_spans_kernel', 'container_read_kernel')


def setup():
    sys.path.insert(0, ROOT)
    import torch
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd import _lib
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    from l3c_pytorch_amd.helpers import config_parser, synthetic
    _lib.require_gpu()
    cfg = config_parser.parse_builtin('ms', 'cr')
    bp = MultiscaleBlueprint(cfg)
    bp.net.load_state_dict(synthetic.make_state_dict(cfg, 0, calibrated=True), strict=True)
    bp.set_eval()
    plain, parity = Bitcoding(bp, bands=K, seal='bands'), Bitcoding(bp, bands=K, seal='bands', parity=G)
    for bc in (plain, parity):
        bc.model_id()                                                    # hashed once per object: not part of a call

    def images(B):
        return torch.stack([synthetic.make_image(H, W, b, 'natural').to(torch.uint8) for b in range(B)])      # on the host
    return torch, plain, parity, images


def kernels_child():
    """Under the profiler: KERNEL_WARMUP + KERNEL_CALLS rounds of the three kernels on one image's finest record; the byte counts go to
    stdout as one JSON line."""
    torch, plain, parity, images = setup()
    import numpy as np
    from l3c_pytorch_amd import ops
    from l3c_pytorch_amd.bitcoding import container
    enc = parity.encode_batch(images(1).cuda()).wait()
    C, Hs, Ws, L, groups = enc.banded_scales[-1]
    n = container.n_bands(Hs * Ws, L)
    m = container.parity_groups(n, G)
    file = enc.to_bytes()[0]
    body, seal = container.split_seal(file)
    parsed = container.parse_banded(body)
    offset, nbytes = parsed.offset[-1].reshape(-1), parsed.nbytes[-1].reshape(-1)         # stream c n + j
    padded = (nbytes + 3) // 4 * 4 + 4
    dst = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    files_d = torch.from_numpy(np.frombuffer(bytes(body) + b'\0' * 8, dtype=np.uint8).copy()).cuda()
    src_d, dst_d, len_d = ops.upload_small(offset), ops.upload_small(dst), ops.upload_small(nbytes.astype(np.int32))
    streams = torch.zeros(int(padded.sum()), dtype=torch.uint8, device='cuda')
    plen = np.asarray([[len(p) for p in row] for row in seal.parity], dtype=np.int64)
    slot = (plen.reshape(-1) + 3) // 4 * 4 + 4 + 12
    out_at = (np.concatenate([[0], np.cumsum(slot)[:-1]]) + 15) // 16 * 16
    out = torch.zeros(int(out_at[-1] + slot[-1] + 16), dtype=torch.uint8, device='cuda')
    offs, lens, first = [], [], [0]
    for c in range(3):
        for g in range(m):
            for j in range(g, n, m):
                offs.append(int(dst[c * n + j]))
                lens.append(int(nbytes[c * n + j]))
            first.append(len(offs))
    for _ in range(KERNEL_WARMUP + KERNEL_CALLS):
        ops.container_read(files_d, src_d, dst_d, len_d, int(nbytes.max()), streams)
        ops.band_parity(1, Hs, Ws, L, groups, G)
        ops.u8_xor_spans(streams, offs, lens, first, out, out_at.tolist(), plen.reshape(-1).tolist())
        torch.cuda.synchronize()
    host = out.cpu().numpy()
    for k, p in enumerate(p for row in seal.parity for p in row):                          # the fold of the uploaded streams IS the file's parity
        assert host[out_at[k]:out_at[k] + len(p)].tobytes() == bytes(p), k
    read = int(((nbytes + 3) // 4 * 4).sum())
    print(json.dumps({'streams': int(nbytes.size), 'payload_bytes': int(nbytes.sum()), 'parity_streams': 3 * m, 'parity_bytes': int(plen.sum()),
                      'band_parity_kernel': read + int(((plen + 3) // 4 * 4).sum()), 'u8_xor_spans_kernel': read + int((slot - 12).sum()),
                      'container_read_kernel': int(nbytes.sum()) + int(padded.sum())}), flush=True)
    return 0


def kernel_rows(trace_dir):
    """Runs the child under rocprofv3 and reduces its kernel trace -> rows."""
    trace_dir = tempfile.mkdtemp(prefix='repair_trace_') if trace_dir is None else os.path.join(trace_dir, 'pid{}'.format(os.getpid()))
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', trace_dir, '-o', 'parity', '--', sys.executable,
           os.path.abspath(__file__), '--kernels-child']
    said = subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.PIPE, text=True).stdout
    counts = json.loads([line for line in said.splitlines() if line.startswith('{')][-1])
    dur = {}
    for f in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        for r in sorted(csv.DictReader(open(f)), key=lambda r: int(r['Start_Timestamp'])):
            for key in KERNELS:
                if key in r['Kernel_Name']:
                    dur.setdefault(key, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    rows = []
    for key in KERNELS:
        take = dur.get(key, [])[-KERNEL_CALLS:]                                            # (the encode of the set-up ran each of them before)
        assert len(take) == KERNEL_CALLS, (key, len(dur.get(key, [])))
        rows.append({'kernel': key, 'bytes_read_and_written': counts[key], 'calls': KERNEL_CALLS, 'us_median': round(statistics.median(take), 2),
                     'us_min': round(min(take), 2), 'us_max': round(max(take), 2),
                     'GB_per_s': round(counts[key] / statistics.median(take) / 1e3, 1)})
    return counts, rows


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
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--band', type=int, default=30, help='the band whose R payload is complemented')
    ap.add_argument('--batch', type=int, default=16, help='the second batch size (0: one image only)')
    ap.add_argument('--kernels', action='store_true', help='the kernel trace alone (a rocprofv3 child; this process does not open the GPU)')
    ap.add_argument('--trace-dir', default=None, help='where the kernel trace goes (default: a fresh temporary directory)')
    ap.add_argument('--kernels-child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.kernels_child:
        return kernels_child()
    if args.kernels:
        counts, rows = kernel_rows(args.trace_dir)
        print(json.dumps(counts), flush=True)
        for row in rows:
            print(json.dumps(row), flush=True)
        print('\n{:>24} {:>12} {:>10} {:>10} {:>10} {:>9}'.format('kernel', 'bytes r + w', 'median us', 'min us', 'max us', 'GB/s'))
        for r in rows:
            print('{:>24} {:>12} {:>10.2f} {:>10.2f} {:>10.2f} {:>9.1f}'.format(r['kernel'], r['bytes_read_and_written'], r['us_median'], r['us_min'],
                                                                             r['us_max'], r['GB_per_s']))
        return 0
    torch, plain, parity, images = setup()
    import numpy as np
    from l3c_pytorch_amd.bitcoding import container
    clock = time.perf_counter
    rows = []
    for B in [1] + ([args.batch] if args.batch > 1 else []):
        img = images(B)
        pads = [(0, 0, 0, 0)] * B
        made = {}

        def enc_leg(bc, name):
            def run():
                t0 = clock()
                made[name] = bc.encode_batch(img.cuda()).to_bytes(pads)
                return clock() - t0
            return run
        legs = [('encode, parity=0', enc_leg(plain, 'plain')), ('encode, parity={}'.format(G), enc_leg(parity, 'parity')),
                ('encode, parity=0 again', enc_leg(plain, 'plain'))]
        times = alternate(legs, args.runs, args.warmup, torch.cuda.synchronize)
        v2, v3 = made['plain'], made['parity']
        assert all(container.split_seal(a)[0] == container.split_seal(b)[0] for a, b in zip(v2, v3))
        sizes = {'file_bytes_band_sealed': sum(map(len, v2)), 'file_bytes_with_parity': sum(map(len, v3))}
        sizes['size_ratio'] = round(sizes['file_bytes_with_parity'] / sizes['file_bytes_band_sealed'], 4)
        damaged = []
        for f in v3:
            parsed = container.parse_banded(container.split_seal(f)[0])
            data = np.frombuffer(f, dtype=np.uint8).copy()
            a, n = int(parsed.offset[-1][0, args.band]), int(parsed.nbytes[-1][0, args.band])
            data[a:a + n] ^= 0xFF
            damaged.append(data.tobytes())
        infos = {}

        def dec_leg(name, fn, files, exact):
            def run():
                t0 = clock()
                res = fn(files)
                out = res[0].cpu()
                t = clock() - t0
                if len(res) == 3:
                    infos[name] = res[2]
                if exact and not torch.equal(out, img):
                    sys.exit('pixels differ: ' + name)
                return t
            return name, run
        batch = lambda files: parity.decode_batch(files, out_dtype=torch.uint8)      # noqa: E731
        legs += [dec_leg('decode_batch, intact', batch, v3, True), dec_leg('decode_repair, intact', parity.decode_repair, v3, True),
                 dec_leg('decode_batch, intact again', batch, v3, True), dec_leg('decode_salvage, damaged', parity.decode_salvage, damaged, False),
                 dec_leg('decode_repair, damaged', parity.decode_repair, damaged, True)]
        times += alternate(legs[3:], args.runs, args.warmup, torch.cuda.synchronize)
        info = infos['decode_repair, damaged']
        assert info.repaired == {b: [(0, args.band)] for b in range(B)} and info.files == v3 and info.rounds == 1, info
        assert infos['decode_repair, intact'].repaired == {} and infos['decode_repair, intact'].rounds == 0
        for (name, _), t in zip(legs, times):
            rows.append(dict({'images': B, 'leg': name, 'ms_median': round(statistics.median(t), 3), 'ms_min': round(min(t), 3),
                              'ms_max': round(max(t), 3), 'runs': args.runs}, **sizes))
            print(json.dumps(rows[-1]), flush=True)
    print('\n{:>7} {:>30} {:>12} {:>10} {:>10}'.format('images', 'leg', 'median ms', 'min ms', 'max ms'))
    for r in rows:
        print('{:>7} {:>30} {:>12.3f} {:>10.3f} {:>10.3f}'.format(r['images'], r['leg'], r['ms_median'], r['ms_min'], r['ms_max']))
    for B in sorted({r['images'] for r in rows}):
        t = {r['leg']: r['ms_median'] for r in rows if r['images'] == B}
        r0 = next(r for r in rows if r['images'] == B)
        e0, e1, e2 = t['encode, parity=0'], t['encode, parity={}'.format(G)], t['encode, parity=0 again']
        d0, d1, d2 = t['decode_batch, intact'], t['decode_repair, intact'], t['decode_batch, intact again']
        print('{} image(s): file size x{} ({} -> {} bytes)'.format(B, r0['size_ratio'], r0['file_bytes_band_sealed'], r0['file_bytes_with_parity']))
        print('  encode with parity - mean(encode without) = {:+.3f} ms; the two baseline legs differ by {:.3f} ms'.format(e1 - (e0 + e2) / 2, abs(e0 - e2)))
        print('  decode_repair on intact files - mean(decode_batch) = {:+.3f} ms; the decode_batch legs differ by {:.3f} ms{}'.format(
            d1 - (d0 + d2) / 2, abs(d0 - d2), '' if min(d0, d2) <= d1 <= max(d0, d2) else '  (outside their spread)'))
        print('  decode_repair on damaged files - decode_salvage on the same files = {:+.3f} ms; - mean(decode_batch, intact) = {:+.3f} ms'.format(
            t['decode_repair, damaged'] - t['decode_salvage, damaged'], t['decode_repair, damaged'] - (d0 + d2) / 2))
    return 0


if __name__ == '__main__':
    sys.exit(main())
