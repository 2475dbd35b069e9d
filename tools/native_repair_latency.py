#!/usr/bin/env python
"""What the repair of a parity-sealed file costs through the C ABI beside Bitcoding's (INTEGRATION.md "Repair through the C ABI"), on the
calibrated checkpoint, host to host.

    python tools/native_repair_latency.py [--runs 20] [--warmup 3] [--band 30] [--batch 16]
    python tools/native_repair_latency.py --kernels      the kernels alone, from a `rocprofv3 --kernel-trace` run of its own

768x512 images, K = 64 bands, G = 16 (m = 4 groups per channel), R = 2: the file's bytes on the host -> uint8 pixels on the host, ending in
a device synchronise.  The legs run in ONE process, alternated, the Python leg TWICE per round -- its two rows show the run-to-run spread a
difference has to exceed:

    damaged        Bitcoding.decode_repair | NativeCodec.decode_repair | Bitcoding.decode_repair again, the R payloads of bands --band and
                   --band + m complemented: two erasures of one group
    intact         the same three legs on the intact file (both codecs then make decode_salvage's calls)
    batch          the same two cases on --batch copies of the file (every file damaged alike)

Medians of --runs rounds after --warmup.
--kernels: on one image's uploaded streams and its R = 4 section, every group of every channel with t = 1, 2, 4 erased members:
l3c_u8_gf_spans (t output groups per group, the rows copied to aligned slots: what Bitcoding._repair launches) beside l3c_band_rebuild (one
group, the rows where they lie in the section), on the same spans; both give back the file's payloads.  Kernel times from the trace.  Prints
one JSON object per row and a table at the end."""
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
H, W, K, G, R = 512, 768, 64, 16, 2
KERNEL_WARMUP, KERNEL_CALLS, TS = 5, 20, (1, 2, 4)
KERNELS = ('u8_gf_spans_kernel', 'band_rebuild_kernel')


def setup(streams=R):
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
    bc = Bitcoding(bp, bands=K, seal='bands', parity=G, parity_streams=streams)
    nat = NativeCodec(bp, bands=K, seal='bands', parity=G, parity_streams=streams)
    bc.model_id(), nat.model_id()                                        # hashed once per object: not part of a call
    image = synthetic.make_image(H, W, 0, 'natural').to(torch.uint8)[None]          # on the host
    return torch, bc, nat, image


def kernels_child():
    """Under the profiler: KERNEL_WARMUP + KERNEL_CALLS rounds of the two kernels at t = 1, 2, 4; the byte counts go to stdout as one JSON line."""
    torch, bc, nat, image = setup(4)
    import numpy as np
    from l3c_pytorch_amd import ops
    from l3c_pytorch_amd.bitcoding import container
    file = bc.encode_batch(image.cuda()).to_bytes([(0, 0, 0, 0)])[0]
    body, seal = container.split_seal(file)
    parsed = container.parse_banded(body)
    n = parsed.nbytes[-1].shape[1]
    m = seal.parity_groups
    offset, nbytes = parsed.offset[-1].reshape(-1), parsed.nbytes[-1].reshape(-1)         # stream c n + j
    padded = (nbytes + 3) // 4 * 4 + 4
    dst = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    files_d = torch.from_numpy(np.frombuffer(bytes(body) + b'\0' * 8, dtype=np.uint8).copy()).cuda()
    src_d, dst_d, len_d = ops.upload_small(offset), ops.upload_small(dst), ops.upload_small(nbytes.astype(np.int32))
    streams = torch.zeros(int(padded.sum()), dtype=torch.uint8, device='cuda')
    ops.container_read(files_d, src_d, dst_d, len_d, int(nbytes.max()), streams)
    intact = streams.clone()
    # the section as it lies in the file (l3c_band_rebuild), and its rows again in aligned slots behind the streams (l3c_u8_gf_spans)
    section = np.frombuffer(file, dtype=np.uint8)[len(body):]
    rows_d = torch.from_numpy(section.copy()).cuda()
    row_at, aligned, at, pos = {}, {}, 12 + 12 * m, (int(padded.sum()) + 15) // 16 * 16
    for c in range(3):
        for g in range(m):
            for r, p in enumerate(seal.rows(c, g)):
                row_at[c, g, r], aligned[c, g, r] = at, pos
                at += len(p)
                pos = (pos + len(p) + 4 + 15) // 16 * 16
    data = torch.zeros(pos, dtype=torch.uint8, device='cuda')
    host = np.zeros(pos, dtype=np.uint8)
    for key, a in aligned.items():
        p = np.frombuffer(bytes(seal.rows(*key[:2])[key[2]]), dtype=np.uint8)
        host[a:a + p.size] = p
    data.copy_(torch.from_numpy(host))
    calls, counts = {}, {}
    for t in TS:
        gf = dict(offs=[], lens=[], coefs=[], first=[0], out_at=[], out_len=[])
        rb = dict(offs=[], lens=[], coefs=[], groups=[])
        out_pos, read_gf, read_rb, written = 0, 0, 0, 0
        for c in range(3):
            for g in range(m):
                count = len(range(g, n, m))
                gone = [(3 + 5 * i) % count for i in range(t)]
                gone = sorted(set(gone))
                assert len(gone) == t
                present = [k for k in range(count) if k not in gone]
                plen = len(seal.rows(c, g)[0])
                solved = container.rs_repair_coefficients(gone, present, 0)
                spans = [(int(dst[c * n + g + k * m]), int(nbytes[c * n + g + k * m])) for k in present]
                first = len(rb['offs'])
                rb['offs'] += [row_at[c, g, r] for r in range(t)] + [a for a, _ in spans]
                rb['lens'] += [plen] * t + [k for _, k in spans]
                for i in range(t):
                    rb['coefs'].append([solved[e][0][i] if e < t else 0 for e in range(4)])
                for p in range(len(present)):
                    rb['coefs'].append([solved[e][1][p] if e < t else 0 for e in range(4)])
                rb['groups'].append((first, t, len(present), [(int(dst[c * n + g + k * m]), int(nbytes[c * n + g + k * m])) for k in gone]))
                read_rb += t * plen + sum(k for _, k in spans)
                for e, k in enumerate(gone):
                    gf['offs'] += [aligned[c, g, r] for r in range(t)] + [a for a, _ in spans]
                    gf['lens'] += [plen] * t + [nb for _, nb in spans]
                    gf['coefs'] += list(solved[e][0]) + list(solved[e][1])
                    gf['first'].append(len(gf['offs']))
                    gf['out_at'].append(out_pos)
                    gf['out_len'].append(int(nbytes[c * n + g + k * m]))
                    out_pos = (out_pos + int(padded[c * n + g + k * m]) + 15) // 16 * 16
                    read_gf += t * plen + sum(nb for _, nb in spans)
                    written += int(padded[c * n + g + k * m])
        calls[t] = (gf, rb, torch.zeros(out_pos + 16, dtype=torch.uint8, device='cuda'))
        counts['u8_gf_spans_kernel t={}'.format(t)] = read_gf + written
        counts['band_rebuild_kernel t={}'.format(t)] = read_rb + written
    data[:streams.numel()] = streams
    for it in range(KERNEL_WARMUP + KERNEL_CALLS):
        for t in TS:
            gf, rb, out = calls[t]
            ops.u8_gf_spans(data, gf['offs'], gf['lens'], gf['coefs'], gf['first'], out, gf['out_at'], gf['out_len'])
            for _, _, _, outs in rb['groups']:                          # the erased members: gone before every rebuild
                for a, k in outs:
                    streams[a:a + k] = 0xEE
            ops.band_rebuild(rows_d, streams, rb['offs'], rb['lens'], rb['coefs'], rb['groups'])
            torch.cuda.synchronize()
    assert torch.equal(streams, intact), 'l3c_band_rebuild did not give back the payloads'
    for t in TS:
        gf, rb, out = calls[t]
        got, want = out.cpu().numpy(), intact.cpu().numpy()
        flat = [o for _, _, _, outs in rb['groups'] for o in outs]
        for (a, k), at_out in zip(flat, gf['out_at']):
            assert (got[at_out:at_out + k] == want[a:a + k]).all(), 'l3c_u8_gf_spans did not give back the payloads'
    print(json.dumps(dict(counts, groups=3 * m, members_per_group=n // m)), flush=True)
    return 0


def kernel_rows(trace_dir):
    """Runs the child under rocprofv3 and reduces its kernel trace -> rows."""
    trace_dir = tempfile.mkdtemp(prefix='native_repair_trace_') if trace_dir is None else os.path.join(trace_dir, 'pid{}'.format(os.getpid()))
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', trace_dir, '-o', 'native_repair', '--', sys.executable,
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
        take = dur.get(key, [])[-KERNEL_CALLS * len(TS):]
        assert len(take) == KERNEL_CALLS * len(TS), (key, len(dur.get(key, [])))
        for i, t in enumerate(TS):
            mine, name = take[i::len(TS)], '{} t={}'.format(key, t)
            rows.append({'kernel': name, 'bytes_read_and_written': counts[name], 'calls': KERNEL_CALLS, 'us_median': round(statistics.median(mine), 2),
                         'us_min': round(min(mine), 2), 'us_max': round(max(mine), 2)})
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
    ap.add_argument('--batch', type=int, default=16)
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
        print('\n{:>28} {:>12} {:>10} {:>10} {:>10}'.format('kernel', 'bytes r + w', 'median us', 'min us', 'max us'))
        for r in rows:
            print('{:>28} {:>12} {:>10.2f} {:>10.2f} {:>10.2f}'.format(r['kernel'], r['bytes_read_and_written'], r['us_median'], r['us_min'], r['us_max']))
        t = {r['kernel']: r['us_median'] for r in rows}
        print('band_rebuild_kernel / u8_gf_spans_kernel: ' + ', '.join('t = {} x{:.2f}'.format(
            k, t['band_rebuild_kernel t={}'.format(k)] / t['u8_gf_spans_kernel t={}'.format(k)]) for k in TS))
        return 0
    torch, bc, nat, img = setup()
    import numpy as np
    from l3c_pytorch_amd.bitcoding import container
    clock = time.perf_counter
    q = bc.encode_batch(img.cuda()).to_bytes([(0, 0, 0, 0)])
    body, seal = container.split_seal(q[0])
    parsed = container.parse_banded(body)
    m = seal.parity_groups
    pair = [(0, args.band), (0, args.band + m)]
    data = np.frombuffer(q[0], dtype=np.uint8).copy()
    for c, j in pair:
        a, nb = int(parsed.offset[-1][c, j]), int(parsed.nbytes[-1][c, j])
        data[a:a + nb] ^= 0xFF
    damaged = [data.tobytes()]
    infos, rows = {}, []

    def leg(name, fn, files):
        want = img.expand(len(files), -1, -1, -1)

        def run():
            t0 = clock()
            res = fn(files)
            out = res[0].cpu()
            torch.cuda.synchronize()
            t = clock() - t0
            infos[name] = res[2]
            if not torch.equal(out, want):
                sys.exit('pixels differ: ' + name)
            return t
        return name, run

    def case(images, what, files):
        tag = '{} image{}, {}'.format(images, '' if images == 1 else 's', what)
        legs = [leg(tag + ': Bitcoding', bc.decode_repair, files), leg(tag + ': NativeCodec', nat.decode_repair, files),
                leg(tag + ': Bitcoding again', bc.decode_repair, files)]
        times = alternate(legs, args.runs, args.warmup, torch.cuda.synchronize)
        for (name, _), t in zip(legs, times):
            info = infos[name]
            assert info.rounds == (1 if what == 'damaged' else 0) and info.repaired == ({i: pair for i in range(images)} if what == 'damaged' else {}), info
            rows.append({'images': images, 'case': what, 'leg': name, 'ms_median': round(statistics.median(t), 3), 'ms_min': round(min(t), 3),
                         'ms_max': round(max(t), 3), 'runs': args.runs})
            print(json.dumps(rows[-1]), flush=True)
        a, b, c = (statistics.median(t) for t in times)
        spread, diff = abs(a - c), b - (a + c) / 2
        print('{}: NativeCodec - mean(Bitcoding) = {:+.3f} ms; the Bitcoding legs differ by {:.3f} ms{}'.format(
            tag, diff, spread, '' if abs(diff) > spread else '  (not resolved)'), flush=True)

    case(1, 'damaged', damaged)
    case(1, 'intact', q)
    case(args.batch, 'damaged', damaged * args.batch)
    case(args.batch, 'intact', q * args.batch)
    print('\n{:>44} {:>12} {:>10} {:>10}'.format('leg', 'median ms', 'min ms', 'max ms'))
    for r in rows:
        print('{:>44} {:>12.3f} {:>10.3f} {:>10.3f}'.format(r['leg'], r['ms_median'], r['ms_min'], r['ms_max']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
