#!/usr/bin/env python
"""What head parity (the 'L3CH' section, INTEGRATION.md "Head parity") costs beside the 'L3CP' / 'L3CQ' file, on the calibrated checkpoint, host to host.

    python tools/head_parity_latency.py [--images 1] [--runs 20] [--warmup 3]
    python tools/head_parity_latency.py --kernels      the kernels alone, from a `rocprofv3 --kernel-trace` run of its own

--images 768x512 images (1, or a batch of 16), K = 64 bands, G = 16, R = 1 and R = 2, through Bitcoding: the images' bytes on the host -> the
files on the host, and the files' bytes on the host -> uint8 pixels on the host.  The legs run in ONE process, alternated, the baseline leg
TWICE per round -- its two rows show the run-to-run spread a difference has to exceed:

    encode                 parity_head=False | parity_head=True | parity_head=False again, per R; and the file-size ratios
    decode_repair, intact  the 'L3CQ' file | the 'L3CH' file | the 'L3CQ' file again (R = 2): heal_head's fast path
    decode_repair, hurt    the 'L3CH' file with one payload of the second-finest record complemented in every file: heal_head's slow path
    host, one file         make_seal without / with the head, zlib.crc32 over the coarser records, heal_head on the intact and on the hurt
                           file, split_seal on the 'L3CQ' and the 'L3CH' file and with heal_head's head part handed on: where the host time goes

Medians of --runs rounds after --warmup.
--kernels: on the coder output of one image l3c_band_parity_rs over the finest record, l3c_head_parity and l3c_band_payload_crc32 over all
coarser records, R = 2, in one trace.  Kernel times from the trace, rates in bytes read + written per second.  Prints one JSON object per row
and a table at the end."""
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
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, K, G = 512, 768, 64, 16
KERNEL_WARMUP, KERNEL_CALLS = 5, 20
# row name -> the spellings of the kernel in a trace (demangled, mangled)
KERNELS = {'band_parity_rs_kernel<2>': ('band_parity_rs_kernel<2>', 'band_parity_rs_kernelILi2E'),
           'head_parity_kernel<2>': ('head_parity_kernel<2>', 'head_parity_kernelILi2E'),
           'band_payload_crc32_kernel': ('band_payload_crc32_kernel',)}


def setup(n_images):
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
    codecs = {(R, head): Bitcoding(bp, bands=K, seal='bands', parity=G, parity_streams=R, parity_head=head) for R in (1, 2) for head in (False, True)}
    for bc in codecs.values():
        bc.model_id()                                                    # hashed once per object: not part of a call
    images = torch.stack([synthetic.make_image(H, W, b, 'natural').to(torch.uint8) for b in range(n_images)])          # on the host
    return torch, codecs, images


def kernels_child():
    """Under the profiler: KERNEL_WARMUP + KERNEL_CALLS rounds of the three kernels on one image's records; the byte counts go to stdout as
    one JSON line."""
    torch, codecs, image = setup(1)
    import numpy as np
    from l3c_pytorch_amd import ops
    from l3c_pytorch_amd.bitcoding import container
    enc = codecs[2, True].encode_batch(image.cuda()).wait()
    file = enc.to_bytes()[0]
    body, seal = container.split_seal(file)
    parsed = container.parse_banded(body)
    _, Hs, Ws, L, groups = enc.banded_scales[-1]
    coarser = list(enc.banded_scales[:-1])
    for _ in range(KERNEL_WARMUP + KERNEL_CALLS):
        ops.band_parity_rs(1, Hs, Ws, L, groups, G, 2)
        crc = ops.band_payload_crc32(1, coarser)
        rows, lens = ops.head_parity(1, coarser, G, 2)
        torch.cuda.synchronize()
    # what the loop computed is what the file holds
    want = np.concatenate([c.reshape(-1) for c in seal.head.crcs])
    assert np.array_equal(crc.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(lens.cpu().numpy(), np.concatenate([p.reshape(-1) for p in seal.head.hplen]))
    r4 = lambda a: int(((np.asarray(a) + 3) // 4 * 4).sum())                                  # noqa: E731
    finest_read, finest_rows = r4(parsed.nbytes[-1]), r4([[len(p[0]) for p in row] for row in seal.parity])
    head_read, head_rows = sum(r4(nb) for nb in parsed.nbytes[:-1]), sum(r4(p) for p in seal.head.hplen)
    print(json.dumps({'finest_payload_bytes': int(parsed.nbytes[-1].sum()), 'head_payload_bytes': int(sum(nb.sum() for nb in parsed.nbytes[:-1])),
                      'head_payloads': int(sum(nb.size for nb in parsed.nbytes[:-1])), 'head_groups': int(sum(p.size for p in seal.head.hplen)),
                      'band_parity_rs_kernel<2>': finest_read + 2 * finest_rows, 'head_parity_kernel<2>': head_read + 2 * head_rows,
                      'band_payload_crc32_kernel': head_read + 4 * int(sum(nb.size for nb in parsed.nbytes[:-1]))}), flush=True)
    return 0


def kernel_rows(trace_dir):
    """Runs the child under rocprofv3 and reduces its kernel trace -> rows."""
    trace_dir = tempfile.mkdtemp(prefix='head_parity_trace_') if trace_dir is None else os.path.join(trace_dir, 'pid{}'.format(os.getpid()))
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', trace_dir, '-o', 'head_parity', '--', sys.executable,
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
        take = dur.get(key, [])[-KERNEL_CALLS:]                                            # (the encode of the set-up ran each of them before)
        assert len(take) == KERNEL_CALLS, (key, len(dur.get(key, [])))
        rows.append({'kernel': key, 'bytes_read_and_written': counts[key], 'calls': KERNEL_CALLS, 'us_median': round(statistics.median(take), 2),
                     'us_min': round(min(take), 2), 'us_max': round(max(take), 2),
                     'GB_per_s': round(counts[key] / statistics.median(take) / 1e3, 2)})
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
    ap.add_argument('--images', type=int, default=1)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
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
        print('\n{:>28} {:>12} {:>10} {:>10} {:>10} {:>9}'.format('kernel', 'bytes r + w', 'median us', 'min us', 'max us', 'GB/s'))
        for r in rows:
            print('{:>28} {:>12} {:>10.2f} {:>10.2f} {:>10.2f} {:>9.2f}'.format(r['kernel'], r['bytes_read_and_written'], r['us_median'], r['us_min'],
                                                                             r['us_max'], r['GB_per_s']))
        return 0
    torch, codecs, img = setup(args.images)
    import numpy as np
    from l3c_pytorch_amd.bitcoding import container
    clock = time.perf_counter
    B = args.images
    pads, made, rows = [(0, 0, 0, 0)] * B, {}, []

    def enc_leg(key, name):
        def run():
            t0 = clock()
            made[key] = codecs[key].encode_batch(img.cuda()).to_bytes(pads)
            return clock() - t0
        return name, run
    legs = []
    for R in (1, 2):
        legs += [enc_leg((R, False), 'encode, R = {}'.format(R)), enc_leg((R, True), 'encode, R = {}, head'.format(R)),
                 enc_leg((R, False), 'encode, R = {} again'.format(R))]
    times = alternate(legs, args.runs, args.warmup, torch.cuda.synchronize)
    sizes = {}
    for R in (1, 2):
        assert all(container.split_seal(a)[0] == container.split_seal(b)[0] for a, b in zip(made[R, True], made[R, False]))
        plain, head = sum(len(f) for f in made[R, False]), sum(len(f) for f in made[R, True])
        sizes.update({'file_bytes_R{}'.format(R): plain, 'file_bytes_R{}_head'.format(R): head, 'size_ratio_R{}_head'.format(R): round(head / plain, 4)})
    q, h = made[2, False], made[2, True]
    hurt = []
    for f in h:                                                          # one payload of the second-finest record complemented
        parsed = container.parse_banded(container.split_seal(f)[0])
        data = np.frombuffer(f, dtype=np.uint8).copy()
        a, nb = int(parsed.offset[-2][1, 5]), int(parsed.nbytes[-2][1, 5])
        data[a:a + nb] ^= 0xFF
        hurt.append(data.tobytes())
    infos, bc = {}, codecs[2, True]

    def dec_leg(name, files):
        def run():
            t0 = clock()
            res = bc.decode_repair(files)
            out = res[0].cpu()
            t = clock() - t0
            infos[name] = res[2]
            if not torch.equal(out, img):
                sys.exit('pixels differ: ' + name)
            return t
        return name, run

    def host_leg(name, fn):
        def run():
            t0 = clock()
            fn()
            return clock() - t0
        return name + ' (host, one file)', run
    # the host parts of one file alone: what make_seal adds for the head, heal_head's two paths, split_seal on either file
    body, s = container.split_seal(h[0])
    fine = [[[bytes(r) for r in s.rows(c, g)] for g in range(s.parity_groups)] for c in range(3)]
    coarse = [(s.head.crcs[k], [[[bytes(r) for r in grp] for grp in ch] for ch in s.head.rows[k]]) for k in range(len(s.head.crcs))]
    seal_args = (body, s.generation, s.frame_crc, s.model_id, s.band_crcs, s.band_len)
    assert body + container.make_seal(*seal_args, parity=(G, fine), head=coarse, head_framing=(s.head.records, s.head.nbytes)) == h[0]
    part = container.heal_head(h[0])[1].part
    first = len(legs)
    legs += [dec_leg('decode_repair, intact L3CQ', q), dec_leg('decode_repair, intact L3CH', h), dec_leg('decode_repair, intact L3CQ again', q),
             dec_leg('decode_repair, 1 coarse payload hurt', hurt),
             host_leg('make_seal without the head', lambda: container.make_seal(*seal_args, parity=(G, fine))),
             host_leg('make_seal with the head', lambda: container.make_seal(*seal_args, parity=(G, fine), head=coarse,
                                                                               head_framing=(s.head.records, s.head.nbytes))),
             host_leg('zlib.crc32 of the coarser records', lambda: zlib.crc32(memoryview(body)[:s.head.positions(len(s.head.records) - 1)[0]])),
             host_leg('heal_head, intact', lambda: container.heal_head(h[0])),
             host_leg('heal_head, hurt', lambda: container.heal_head(hurt[0])),
             host_leg('split_seal, L3CQ', lambda: container.split_seal(q[0], view=True)),
             host_leg('split_seal, L3CH', lambda: container.split_seal(h[0], view=True)),
             host_leg('split_seal, L3CH, head part handed on', lambda: container.split_seal(h[0], view=True, head=part))]
    times += alternate(legs[first:], args.runs, args.warmup, torch.cuda.synchronize)
    info = infos['decode_repair, 1 coarse payload hurt']
    assert all(hd.repaired == [(len(parsed.scales) - 2, 1, 5)] and not hd.failed for hd in info.head) and info.files == h, info
    assert not any(infos['decode_repair, intact L3CH'].head) and infos['decode_repair, intact L3CQ'].head == [None] * B
    for (name, _), t in zip(legs, times):
        rows.append(dict({'images': B, 'leg': name, 'ms_median': round(statistics.median(t), 3), 'ms_min': round(min(t), 3),
                          'ms_max': round(max(t), 3), 'runs': args.runs}, **sizes))
        print(json.dumps(rows[-1]), flush=True)
    print('\n{:>58} {:>12} {:>10} {:>10}'.format('leg', 'median ms', 'min ms', 'max ms'))
    for r in rows:
        print('{:>58} {:>12.3f} {:>10.3f} {:>10.3f}'.format(r['leg'], r['ms_median'], r['ms_min'], r['ms_max']))
    t = {r['leg']: r['ms_median'] for r in rows}
    for R in (1, 2):
        a, b = t['encode, R = {}'.format(R)], t['encode, R = {} again'.format(R)]
        print('R = {}: file size x{} ({} -> {} bytes); encode with the head - mean(without) = {:+.3f} ms; the two baseline legs differ by {:.3f} ms'.format(
            R, sizes['size_ratio_R{}_head'.format(R)], sizes['file_bytes_R{}'.format(R)], sizes['file_bytes_R{}_head'.format(R)],
            t['encode, R = {}, head'.format(R)] - (a + b) / 2, abs(a - b)))
    d0, d1, d2 = t['decode_repair, intact L3CQ'], t['decode_repair, intact L3CH'], t['decode_repair, intact L3CQ again']
    print('decode_repair on the intact L3CH file - mean(L3CQ file) = {:+.3f} ms; the L3CQ legs differ by {:.3f} ms{}'.format(
        d1 - (d0 + d2) / 2, abs(d0 - d2), '' if min(d0, d2) <= d1 <= max(d0, d2) else '  (outside their spread)'))
    print('decode_repair, one coarse payload hurt per file - mean(intact L3CQ) = {:+.3f} ms; heal_head alone on one such file {:.3f} ms'.format(
        t['decode_repair, 1 coarse payload hurt'] - (d0 + d2) / 2, t['heal_head, hurt (host, one file)']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
