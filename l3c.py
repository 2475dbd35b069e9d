#!/usr/bin/env python
"""Encoder / decoder CLI -- same arguments as the reference's src/l3c.py:74-125:

    python l3c.py LOG_DIR LOG_DATE [--device auto|gpu|cpu] [-i ITR] enc IMG_P OUT_P [--overwrite]
    python l3c.py LOG_DIR LOG_DATE [--device auto|gpu|cpu] [-i ITR] dec [--region Y0:Y1[,X0:X1]] [--salvage] [--repair [--write-repaired OUT.l3c]] IMG_P OUT_P_PNG
    python l3c.py LOG_DIR LOG_DATE [--device auto|gpu|cpu] [-i ITR] preview IMG_P OUT_P_PNG [--records R] [--bytes N]

Everything runs on the MI355X path; `--device cpu` is refused (there is no CPU back end in this build).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import l3c_pytorch_amd  # noqa: E402,F401

l3c_pytorch_amd.configure_hip_queues()      # image sets / auto-crops run several forward passes side by side (before the first HIP call)
from l3c_pytorch_amd import torchac  # noqa: E402
from l3c_pytorch_amd.test.multiscale_tester import DecodeError, EncodeError, MultiscaleTester  # noqa: E402

# `enc --bands` without a value: the smallest band count within 5 % of the fastest one-image decode (profiles/r07_banded_latency.log)
DEFAULT_BANDS = 64
DEFAULT_PARITY = 16


def parse_device_flag(flag):
    import torch
    gpu = torch.cuda.is_available()
    print('Status: torchac-backend-gpu (HIP) available: {} // torchac-backend-cpu available: {} // GPU available: {}'.format(
        torchac.CUDA_SUPPORTED, torchac.CPU_SUPPORTED, gpu))
    if flag == 'auto':
        flag = 'gpu'
    if flag == 'cpu':
        raise ValueError('torchac-backend-cpu is not available: this build only has the MI355X (HIP) path.')
    if not gpu:
        raise ValueError('Selected GPU backend but no GPU is visible!')
    print('*** Using the HIP back end on', torch.cuda.get_device_name(0))


def parse_region(text):
    """'Y0:Y1' or 'Y0:Y1,X0:X1' -> (y0, y1) or (y0, y1, x0, x1): rows [Y0, Y1) and columns [X0, X1) of the image."""
    try:
        parts = [tuple(int(v) for v in part.split(':')) for part in text.split(',')]
    except ValueError:
        parts = []
    if len(parts) not in (1, 2) or any(len(part) != 2 for part in parts):
        raise argparse.ArgumentTypeError('expected Y0:Y1 or Y0:Y1,X0:X1, got {!r}'.format(text))
    return tuple(v for part in parts for v in part)


def main(argv=None):
    p = argparse.ArgumentParser(description='Encoder/Decoder for L3C')
    p.add_argument('log_dir', help='Directory of experiments.')
    p.add_argument('log_date', help='A log_date, such as 0104_1345.')
    p.add_argument('--device', type=str, choices=['auto', 'gpu', 'cpu'], default='auto')
    p.add_argument('--restore_itr', '-i', default=-1, type=int,
                   help='Which iteration to restore. -1 means latest iteration. Default: -1')
    p.add_argument('--compare_theory', action='store_true', help='print cross-entropy bpsp next to the on-disk bpsp')
    mode = p.add_subparsers(title='mode', dest='mode')
    enc = mode.add_parser('enc', help='Encode image: enc IMG_P OUT_P [--overwrite | -f]')
    dec = mode.add_parser('dec', help='Decode image: dec IMG_P OUT_P_PNG')
    enc.add_argument('img_p')
    enc.add_argument('out_p')
    enc.add_argument('--overwrite', '-f', action='store_true')
    enc.add_argument('--bands', type=int, nargs='?', const=DEFAULT_BANDS, default=0, metavar='K',
                     help='write a BANDED file: every channel cut into at most K independently coded bands, for fast one-image '
                          'encode / decode (1..1024; the flag alone: {}).  Without the flag: the legacy format.'.format(DEFAULT_BANDS))
    enc.add_argument('--seal', action='store_true',
                     help='write a SEALED file: 24 bytes behind the last record that state the bitstream generation, the checkpoint and the '
                          'CRC-32 of the image, so that dec refuses to return wrong pixels')
    enc.add_argument('--seal-bands', dest='seal_bands', action='store_true',
                     help='with --bands: write a BAND-SEALED file, a seal with one CRC-32 per band of the finest record in front of it: dec then '
                          'names the damaged rows of a file that fails, and dec --region verifies the pixels it returns')
    enc.add_argument('--parity', type=int, nargs='?', const=DEFAULT_PARITY, default=0, metavar='G',
                     help='with --bands --seal-bands: add PARITY BANDS, an XOR parity stream per group of G bands of the finest record (about '
                          '1 / G more bytes; the flag alone: {}): dec --repair then rebuilds one damaged band per group, bit for '
                          'bit'.format(DEFAULT_PARITY))
    enc.add_argument('--parity-streams', dest='parity_streams', type=int, default=1, choices=(1, 2, 3, 4), metavar='R',
                     help='with --parity: R parity streams per group over GF(2^8) instead of one (about R / G more bytes): dec --repair then '
                          'rebuilds up to R damaged bands per group, and a damaged parity stream leaves R - 1 usable')
    enc.add_argument('--parity-head', dest='parity_head', action='store_true',
                     help='with --parity: protect the HEAD of the file as well -- the file header, the coarser records and every length field '
                          '(a copy of the framing, a CRC-32 per coarse payload and the same R streams per group over them): dec --repair then '
                          'heals damaged framing and coarse payloads before it decodes')
    dec.add_argument('img_p')
    dec.add_argument('out_p_png')
    dec.add_argument('--no-verify', dest='no_verify', action='store_true', help='do not check the seal of a sealed file')
    dec.add_argument('--region', type=parse_region, default=None, metavar='Y0:Y1[,X0:X1]',
                     help='decode only rows [Y0, Y1) (and columns [X0, X1)) of the image: of a banded file only the bands and rows that '
                          'box needs are decoded; OUT_P_PNG receives the box')
    dec.add_argument('--salvage', action='store_true',
                     help='a damaged BAND-SEALED file: write the picture all the same -- every verified pixel exact, the damaged bands '
                          'concealed by the mean of the predicted distribution -- and say which rows are which')
    dec.add_argument('--repair', action='store_true',
                     help='a damaged file written with --parity: rebuild the damaged bands from the parity, bit for bit, where one band per '
                          'group is damaged; what cannot be rebuilt is concealed as --salvage conceals it; says which rows are which')
    dec.add_argument('--write-repaired', dest='write_repaired', default=None, metavar='OUT.l3c',
                     help='with --repair: write the healed file (the rebuilt payloads spliced in) when something was repaired')
    pre = mode.add_parser('preview', help='Picture from the coarse scale records of a file: preview IMG_P OUT_P_PNG [--records R] [--bytes N]')
    pre.add_argument('img_p')
    pre.add_argument('out_p_png')
    pre.add_argument('--records', type=int, default=None, metavar='R',
                     help='scale records to decode, coarsest first; the finer scales are estimated (default: all but the finest)')
    pre.add_argument('--bytes', type=int, default=None, metavar='N', help='read at most the first N bytes of the file')
    flags = p.parse_args(argv)
    if flags.mode is None:
        p.error('mode (enc | dec | preview) required')
    parse_device_flag(flags.device)
    print('Testing {} at {} ---'.format(flags.log_date, flags.restore_itr))
    tester = MultiscaleTester(flags.log_date, flags, flags.restore_itr, l3c=True)
    if flags.mode == 'enc':
        try:
            tester.encode(flags.img_p, flags.out_p, flags.overwrite)
        except EncodeError as e:
            print('*** EncodeError:', e)
            return 1
    elif flags.mode == 'preview':
        try:
            tester.preview(flags.img_p, flags.out_p_png, flags.records, flags.bytes)
        except DecodeError as e:
            print('*** DecodeError:', e)
            return 1
    else:
        try:
            if flags.write_repaired and not flags.repair:
                raise DecodeError('--write-repaired needs --repair')
            tester.decode(flags.img_p, flags.out_p_png, flags.region, flags.salvage, flags.repair, flags.write_repaired)
        except DecodeError as e:
            print('*** DecodeError:', e)
            return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
