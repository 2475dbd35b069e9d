#!/usr/bin/env python
"""The network forward two ways in ONE process, alternating: the Python schedule (MultiscaleNetwork.forward: 129 library calls from
Python) and the C schedule (NativeNet.forward: one l3c_net_forward call), 768x512 images, seeded synthetic L3C checkpoint.

    python tools/net_forward_probe.py [--runs1 60] [--runs128 6]          # timings, one JSON line per leg + a summary table
    python tools/net_forward_probe.py --trace python|native               # one B = 2 forward after a warm-up (run under rocprofv3)
    python tools/net_forward_probe.py --compare-traces A.csv B.csv        # kernel names / grids / order of the last forward of each

B = 1: `enqueue` = host time until the call returns (everything enqueued, no synchronisation), `complete` = host time from the call
to the end of a synchronise; median and spread (min, max) over the runs after a warm-up.  B = 128: device time between events
recorded around the call, median and spread.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 512, 768


def _nets():
    import torch
    import l3c_pytorch_amd  # noqa: F401
    from l3c_pytorch_amd.blueprints.multiscale_blueprint import MultiscaleBlueprint
    from l3c_pytorch_amd.helpers import config_parser, synthetic
    from l3c_pytorch_amd.native_net import NativeNet
    cfg = config_parser.parse_builtin('ms', 'cr')
    bp = MultiscaleBlueprint(cfg)
    bp.net.load_state_dict(synthetic.make_state_dict(cfg, 0, calibrated=True), strict=True)
    bp.set_eval()
    net = bp.net
    native = NativeNet(net)
    torch.cuda.synchronize()
    return {'python': lambda x: net.forward(x), 'native': lambda x: native.forward(x)}


def _image(B):
    import torch
    g = torch.Generator().manual_seed(B)
    return torch.randint(0, 256, (B, 3, H, W), generator=g).float().cuda()


def _stats(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'n': len(v)}


def timings(runs1, runs128):
    import torch
    fns = _nets()
    res = {}
    x = _image(1)
    for name in fns:                 # warm-up: weights packed, allocator primed, kernels loaded
        for _ in range(5):
            fns[name](x)
    torch.cuda.synchronize()
    enq = {k: [] for k in fns}
    done = {k: [] for k in fns}
    for _ in range(runs1):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(x)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            enq[name].append((t1 - t0) * 1e3)
            done[name].append((t2 - t0) * 1e3)
            del out
    for name in fns:
        res[(name, 1)] = {'enqueue_ms': _stats(enq[name]), 'complete_ms': _stats(done[name])}
        print(json.dumps({'leg': 'B1', 'schedule': name, 'shape': [1, 3, H, W], 'enqueue_ms': res[(name, 1)]['enqueue_ms'],
                          'complete_ms': res[(name, 1)]['complete_ms']}), flush=True)
    del x
    x = _image(128)
    dev = {k: [] for k in fns}
    for name in fns:                 # warm-up at this size
        out = fns[name](x)
        del out
    torch.cuda.synchronize()
    for _ in range(runs128):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(x)
            e1.record()
            torch.cuda.synchronize()
            dev[name].append(e0.elapsed_time(e1))
            del out
    for name in fns:
        res[(name, 128)] = {'device_ms': _stats(dev[name])}
        mpix = 128 * H * W / 1e6 / (res[(name, 128)]['device_ms']['median'] / 1e3)
        print(json.dumps({'leg': 'B128', 'schedule': name, 'shape': [128, 3, H, W], 'device_ms': res[(name, 128)]['device_ms'],
                          'mpix_per_s': mpix}), flush=True)
    print('\n{:<8} {:>26} {:>26} {:>26}'.format('', 'B=1 enqueue ms', 'B=1 complete ms', 'B=128 device ms'))
    for name in fns:
        row = [res[(name, 1)]['enqueue_ms'], res[(name, 1)]['complete_ms'], res[(name, 128)]['device_ms']]
        print('{:<8} '.format(name) + ' '.join('{:>9.3f} [{:.3f}, {:.3f}]'.format(r['median'], r['min'], r['max']).rjust(26) for r in row))


def trace(which):
    import torch
    fns = _nets()
    x = _image(2)
    fns[which](x)
    torch.cuda.synchronize()
    fns[which](x)
    torch.cuda.synchronize()


def _last_forward(path):
    """(name, grid) of the library kernels of the LAST forward in a rocprofv3 kernel trace: from the last rgb_head_kernel on (the
    torch kernels that surround the calls -- the image's rounding in Out.append_input_image, Out's int64 symbol copies -- dropped)."""
    rows = list(csv.DictReader(open(path)))
    key = 'Start_Timestamp' if 'Start_Timestamp' in rows[0] else None
    if key:
        rows.sort(key=lambda r: int(r[key]))
    ks = [(r['Kernel_Name'], tuple(int(r.get('Grid_Size_' + a, r.get('Grid_' + a, 0)) or 0) for a in 'XYZ')) for r in rows]
    start = max(i for i, k in enumerate(ks) if k[0].startswith('rgb_head_kernel') or 'rgb_head_kernel' in k[0])
    return [k for k in ks[start:] if 'at::' not in k[0] and 'elementwise' not in k[0]]


def compare(a, b):
    ka, kb = _last_forward(a), _last_forward(b)
    print('{}: {} library kernels from rgb_head on; {}: {}'.format(a, len(ka), b, len(kb)))
    same = ka == kb
    for i in range(max(len(ka), len(kb))):
        x = ka[i] if i < len(ka) else ('-', ())
        y = kb[i] if i < len(kb) else ('-', ())
        if x != y:
            print('differ at {}: {} {} | {} {}'.format(i, x[0][:70], x[1], y[0][:70], y[1]))
    print('identical names, grids and order' if same else 'NOT identical')
    if same:
        for i, (name, grid) in enumerate(ka):
            print('{:4d}  {:<60} grid {}'.format(i, name.replace('(anonymous namespace)::', '').split('(')[0][:60], 'x'.join(map(str, grid))))
    return 0 if same else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs1', type=int, default=60)
    ap.add_argument('--runs128', type=int, default=6)
    ap.add_argument('--trace', choices=['python', 'native'])
    ap.add_argument('--compare-traces', nargs=2)
    a = ap.parse_args()
    if a.compare_traces:
        sys.exit(compare(*a.compare_traces))
    if a.trace:
        trace(a.trace)
    else:
        timings(a.runs1, a.runs128)
