#!/usr/bin/env python
"""What R parity streams per group cost beside one (INTEGRATION.md "Parity bands"), on the calibrated checkpoint, host to host.

    python tools/rs_parity_latency.py [--runs 20] [--warmup 3] [--band 30]
    python tools/rs_parity_latency.py --kernels      the kernels alone, from a `rocprofv3 --kernel-trace` run of its own

One 768x512 image, K = 64 bands, G = 16 (m = 4 groups per channel), through Bitcoding: the image's bytes on the host -> the file on the host,
and the file's bytes on the host -> uint8 pixels on the host.  The legs run in ONE process, alternated, the baseline leg TWICE per round --
its two rows show the run-to-run spread a difference has to exceed:

    encode                 band-sealed | R = 1 | R = 2 | R = 4 | band-sealed again; and the file-size ratios
    decode, intact         decode_batch | decode_repair | decode_batch again, on the R = 2 file (decode_repair makes decode_salvage's calls)
    decode, damaged        decode_salvage | decode_repair on the R = 2 file with the R payloads of bands --band and --band + m complemented:
                           two erasures of one group

Medians of --runs rounds after --warmup.
--kernels: on the coder output of the image's finest record l3c_band_parity and l3c_band_parity_rs at R = 2 and R = 4; on the uploaded streams
l3c_u8_xor_spans folding the groups and l3c_u8_gf_spans folding the same spans with the weights alpha^k (row 1 of the section, checked against
the file).  Kernel times from the trace, rates in bytes read + written per second.  Prints one JSON object per row and a table at the end."""
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
# row name -> the spellings of the kernel in a trace (demangled, mangled)
KERNELS = {'band_parity_kernel': ('band_parity_kernel',),
           'band_parity_rs_kernel<2>': ('band_parity_rs_kernel<2>', 'band_parity_rs_kernelILi2E'),
           'band_parity_rs_kernel<4>': ('band_parity_rs_kernel<4>', 'band_parity_rs_kernelILi4E'),
           'u8_xor_spans_kernel': ('u8_xor_spans_kernel',),
           'u8_gf_spans_kernel': ('u8_gf_spans_kernel',)}


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
    codecs = {0: Bitcoding(bp, bands=K, seal='bands')}
    for R in (1, 2, 4):
        codecs[R] = Bitcoding(bp, bands=K, seal='bands', parity=G, parity_streams=R)
    for bc in codecs.values():
        bc.model_id()                                                    # hashed once per object: not part of a call
    image = synthetic.make_image(H, W, 0, 'natural').to(torch.uint8)[None]          # on the host
    return torch, codecs, image


def kernels_child():
    """Under the profiler: KERNEL_WARMUP + KERNEL_CALLS rounds of the five kernels on one image's finest record; the byte counts go to
    stdout as one JSON line."""
    torch, codecs, image = setup()
    import numpy as np
    from l3c_pytorch_amd import ops
    from l3c_pytorch_amd.bitcoding import container
    enc = codecs[2].encode_batch(image.cuda()).wait()
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
    ops.container_read(files_d, src_d, dst_d, len_d, int(nbytes.max()), streams)
    plen = np.asarray([[len(p[0]) for p in row] for row in seal.parity], dtype=np.int64)
    slot = (plen.reshape(-1) + 3) // 4 * 4 + 4 + 12
    out_at = (np.concatenate([[0], np.cumsum(slot)[:-1]]) + 15) // 16 * 16
    out_x = torch.zeros(int(out_at[-1] + slot[-1] + 16), dtype=torch.uint8, device='cuda')
    out_g = torch.zeros_like(out_x)
    offs, lens, coefs, first = [], [], [], [0]
    for c in range(3):
        for g in range(m):
            for k, j in enumerate(range(g, n, m)):
                offs.append(int(dst[c * n + j]))
                lens.append(int(nbytes[c * n + j]))
                coefs.append(container.gf_pow_alpha(k))
            first.append(len(offs))
    for _ in range(KERNEL_WARMUP + KERNEL_CALLS):
        ops.band_parity(1, Hs, Ws, L, groups, G)
        ops.band_parity_rs(1, Hs, Ws, L, groups, G, 2)
        ops.band_parity_rs(1, Hs, Ws, L, groups, G, 4)
        ops.u8_xor_spans(streams, offs, lens, first, out_x, out_at.tolist(), plen.reshape(-1).tolist())
        ops.u8_gf_spans(streams, offs, lens, coefs, first, out_g, out_at.tolist(), plen.reshape(-1).tolist())
        torch.cuda.synchronize()
    host_x, host_g = out_x.cpu().numpy(), out_g.cpu().numpy()
    for k, rows in enumerate(rows for row in seal.parity for rows in row):                 # the folds of the uploaded streams ARE rows 0 and 1
        assert host_x[out_at[k]:out_at[k] + len(rows[0])].tobytes() == bytes(rows[0]), k
        assert host_g[out_at[k]:out_at[k] + len(rows[1])].tobytes() == bytes(rows[1]), k
    read, row = int(((nbytes + 3) // 4 * 4).sum()), int(((plen + 3) // 4 * 4).sum())
    print(json.dumps({'streams': int(nbytes.size), 'payload_bytes': int(nbytes.sum()), 'groups': 3 * m, 'row_bytes': int(plen.sum()),
                      'band_parity_kernel': read + row, 'band_parity_rs_kernel<2>': read + 2 * row, 'band_parity_rs_kernel<4>': read + 4 * row,
                      'u8_xor_spans_kernel': read + int((slot - 12).sum()), 'u8_gf_spans_kernel': read + int((slot - 12).sum())}), flush=True)
    return 0


def kernel_rows(trace_dir):
    """Runs the child under rocprofv3 and reduces its kernel trace -> rows."""
    trace_dir = tempfile.mkdtemp(prefix='rs_parity_trace_') if trace_dir is None else os.path.join(trace_dir, 'pid{}'.format(os.getpid()))
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', trace_dir, '-o', 'rs_parity', '--', sys.executable,
           os.path.abspath(__file__), '--kernels-child']
    said = subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.PIPE, text=True).stdout
    counts = json.loads([line for line in said.splitlines() if line.startswith('{')][-1])
    dur = {}
    for f in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        for r in sorted(csv.DictReader(open(f)), key=lambda r: int(r['Start_Timestamp'])):
            for key, spellings in KERNELS.items():
                if any(s in r['Kernel_Name'] for s in spellings):
                    dur.setdefault(key, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    rows = []
    for key in KERNELS:
        take = dur.get(key, [])[-KERNEL_CALLS:]                                            # (the encode of the set-up ran one of them before)
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
    ap.add_argument('--band', type=int, default=30, help='the R payloads of this band and of the next member of its group are complemented')
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
        print('\n{:>26} {:>12} {:>10} {:>10} {:>10} {:>9}'.format('kernel', 'bytes r + w', 'median us', 'min us', 'max us', 'GB/s'))
        for r in rows:
            print('{:>26} {:>12} {:>10.2f} {:>10.2f} {:>10.2f} {:>9.1f}'.format(r['kernel'], r['bytes_read_and_written'], r['us_median'], r['us_min'],
                                                                             r['us_max'], r['GB_per_s']))
        t = {r['kernel']: r['us_median'] for r in rows}
        print('band_parity_rs_kernel / band_parity_kernel: R = 2 x{:.2f}, R = 4 x{:.2f}; u8_gf_spans_kernel / u8_xor_spans_kernel: x{:.2f}'.format(
            t['band_parity_rs_kernel<2>'] / t['band_parity_kernel'], t['band_parity_rs_kernel<4>'] / t['band_parity_kernel'],
            t['u8_gf_spans_kernel'] / t['u8_xor_spans_kernel']))
        return 0
    torch, codecs, img = setup()
    import numpy as np
    from l3c_pytorch_amd.bitcoding import container
    clock = time.perf_counter
    pads, made, rows = [(0, 0, 0, 0)], {}, []

    def enc_leg(R, name):
        def run():
            t0 = clock()
            made[R] = codecs[R].encode_batch(img.cuda()).to_bytes(pads)
            return clock() - t0
        return name, run
    legs = [enc_leg(0, 'encode, band-sealed'), enc_leg(1, 'encode, R = 1'), enc_leg(2, 'encode, R = 2'), enc_leg(4, 'encode, R = 4'),
            enc_leg(0, 'encode, band-sealed again')]
    times = alternate(legs, args.runs, args.warmup, torch.cuda.synchronize)
    assert all(container.split_seal(made[R][0])[0] == container.split_seal(made[0][0])[0] for R in (1, 2, 4))
    sizes = {'file_bytes_band_sealed': len(made[0][0])}
    for R in (1, 2, 4):
        sizes['file_bytes_R{}'.format(R)] = len(made[R][0])
        sizes['size_ratio_R{}'.format(R)] = round(len(made[R][0]) / len(made[0][0]), 4)
    q = made[2]
    body, seal = container.split_seal(q[0])
    parsed = container.parse_banded(body)
    m = seal.parity_groups
    pair = [(0, args.band), (0, args.band + m)]
    data = np.frombuffer(q[0], dtype=np.uint8).copy()
    for c, j in pair:
        a, nb = int(parsed.offset[-1][c, j]), int(parsed.nbytes[-1][c, j])
        data[a:a + nb] ^= 0xFF
    damaged = [data.tobytes()]
    infos, bc = {}, codecs[2]

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
    batch = lambda files: bc.decode_batch(files, out_dtype=torch.uint8)      # noqa: E731
    legs += [dec_leg('decode_batch, intact', batch, q, True), dec_leg('decode_repair, intact', bc.decode_repair, q, True),
             dec_leg('decode_batch, intact again', batch, q, True), dec_leg('decode_salvage, 2 damaged', bc.decode_salvage, damaged, False),
             dec_leg('decode_repair, 2 damaged', bc.decode_repair, damaged, True)]
    times += alternate(legs[5:], args.runs, args.warmup, torch.cuda.synchronize)
    info = infos['decode_repair, 2 damaged']
    assert info.repaired == {0: pair} and info.files == q and info.rounds == 1, info
    assert infos['decode_repair, intact'].repaired == {} and infos['decode_repair, intact'].rounds == 0
    for (name, _), t in zip(legs, times):
        rows.append(dict({'images': 1, 'leg': name, 'ms_median': round(statistics.median(t), 3), 'ms_min': round(min(t), 3),
                          'ms_max': round(max(t), 3), 'runs': args.runs}, **sizes))
        print(json.dumps(rows[-1]), flush=True)
    print('\n{:>32} {:>12} {:>10} {:>10}'.format('leg', 'median ms', 'min ms', 'max ms'))
    for r in rows:
        print('{:>32} {:>12.3f} {:>10.3f} {:>10.3f}'.format(r['leg'], r['ms_median'], r['ms_min'], r['ms_max']))
    t = {r['leg']: r['ms_median'] for r in rows}
    base = (t['encode, band-sealed'] + t['encode, band-sealed again']) / 2
    print('file size: band-sealed {} bytes; R = 1 x{}, R = 2 x{}, R = 4 x{}'.format(sizes['file_bytes_band_sealed'], sizes['size_ratio_R1'],
                                                                                  sizes['size_ratio_R2'], sizes['size_ratio_R4']))
    print('encode - mean(band-sealed): R = 1 {:+.3f} ms, R = 2 {:+.3f} ms, R = 4 {:+.3f} ms; R = 2 - R = 1 {:+.3f} ms, R = 4 - R = 1 {:+.3f} ms; '
          'the two baseline legs differ by {:.3f} ms'.format(t['encode, R = 1'] - base, t['encode, R = 2'] - base, t['encode, R = 4'] - base,
                                                             t['encode, R = 2'] - t['encode, R = 1'], t['encode, R = 4'] - t['encode, R = 1'],
                                                             abs(t['encode, band-sealed'] - t['encode, band-sealed again'])))
    d0, d1, d2 = t['decode_batch, intact'], t['decode_repair, intact'], t['decode_batch, intact again']
    print('decode_repair on the intact file - mean(decode_batch) = {:+.3f} ms; the decode_batch legs differ by {:.3f} ms{}'.format(
        d1 - (d0 + d2) / 2, abs(d0 - d2), '' if min(d0, d2) <= d1 <= max(d0, d2) else '  (outside their spread)'))
    print('decode_repair, two payloads of one group damaged - decode_salvage of the same file = {:+.3f} ms; - mean(decode_batch, intact) = {:+.3f} ms'.format(
        t['decode_repair, 2 damaged'] - t['decode_salvage, 2 damaged'], t['decode_repair, 2 damaged'] - (d0 + d2) / 2))
    return 0


if __name__ == '__main__':
    sys.exit(main())
