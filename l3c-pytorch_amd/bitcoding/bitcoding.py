"""Bitcoding -- `.l3c` container encode / decode with the whole data path on the GPU.

Same surface as the reference's bitcoding/bitcoding.py (`Bitcoding(blueprint, times, compare_with_theory)`,
`encode(img, pout) -> bpsp` :50-123, `decode(pin) -> 1CHW long` :125-161) and the same byte format (:326-375; the host side of the framing,
and of the opt-in banded files beside it, is container.py).

What changed is WHERE the work happens.  The reference loops over scales and channels in Python, builds one CDF table per
channel, and range-codes it on one CPU thread (coders.py:38-66 -> torchac.cpp).  Here a batch of B equally sized images
is pushed through
    encoder:  net forward  ->  per scale ONE fused kernel P,symbols -> coding intervals of all B*C streams
              ->  ONE grouped range-coder launch over all scales (and, with encode_many, over all batches of a
                  heterogeneous image set)                                         -> bytes + lengths in HBM
    decoder:  per scale get_P -> parameters -> uint16 tables -> ONE range-decoder launch (a stream per wavefront);
              only the RGB scale is serial in its channels (R -> G -> B, the lambda coupling of logistic_mixture.py:262-272)
and only finished byte strings cross PCIe.  `encode_batch` / `decode_batch` are the native entry points; `encode` /
`decode` are the reference's one-image file API on top of them (auto-crop parts included).
"""
import os

import numpy as np
import torch

from .. import auto_crop, ops
from ..helpers import pad
from ..modules import schema
from . import container, part_suffix_helper, region, upload
from .container import (_MAGIC_VALUE_SEP, BANDED_SIGNATURE, MAX_BANDS, band_len, count_scale_records, is_banded, n_bands,  # noqa: F401
                        parse_banded, parse_containers)
from .set_decode import SetDecoder


class _NullTimes(object):
    """Stand-in for the reference's StackTimeLogger when no timing is requested."""

    class _Ctx(object):
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    def run(self, *a, **kw):
        return self._Ctx()

    prefix_scope = combine = run


def uniform_cdf_row(L):
    """The coarsest scale's table: round(cumsum(1/L) * 2^16) with a leading 0, as int16 (bitcoding.py:297-323).
    Same fp32 torch ops as the reference so the row is bit-identical (L=25: 0, 2621, 5243, ...)."""
    histo = torch.ones(L, dtype=torch.float32) / L
    cdf = torch.cumsum(torch.ones(1, L) * histo, -1).mul_(2 ** 16).round()
    cdf = torch.cat((torch.zeros(1, 1), cdf), dim=-1)
    return cdf.to(torch.int16).reshape(-1)


_STAGING = [None]


def _staging(nbytes):
    """Host staging buffer for the D2H copy of finished files: ONE page-locked buffer, grown geometrically and reused (page-
    locking costs far more than the copy itself); the caller consumes the returned view before the next call."""
    buf = _STAGING[0]
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 2 * (buf.numel() if buf is not None else 0), 64 << 20), dtype=torch.uint8, pin_memory=True)
        _STAGING[0] = buf
    return buf[:nbytes]


def coder_group_cuts(n_passes, n_groups):
    """After which forward passes (1-based counts, ascending, the last one == n_passes) `encode_many` launches the range coder:
    n_groups equal groups (int), or cut points given as cumulative fractions of the passes (list / tuple, e.g. (0.5, 0.75, 1.0))."""
    if n_passes <= 0:
        return []
    if isinstance(n_groups, (list, tuple)):
        return sorted({min(n_passes, max(1, int(round(f * n_passes)))) for f in n_groups} | {n_passes})
    per_group = -(-n_passes // max(1, int(n_groups)))
    return list(range(per_group, n_passes, per_group)) + [n_passes]


def rgb_pipeline_schedule(n_chunks, C, D):
    """Steps of the chunk-pipelined RGB decode: step t handles chunk t - D c of channel c.  Returns a list (one entry per
    step) of lists of (channel, chunk).  Channel c's chunk j needs the symbols of the channels < c in chunk j: with D = 1
    they come from the previous step, with D = 2 from two steps back -- the tables of step t + 1 then do not depend on the
    decode launch of step t and the two can overlap."""
    return [[(c, t - D * c) for c in range(C) if 0 <= t - D * c < n_chunks] for t in range(n_chunks + D * (C - 1))]


class EncodedBatch(object):
    """Device-resident result of `Bitcoding.encode_batch`: per scale (coarse -> fine) the coder output of its B*C streams.
    Nothing has been synchronised or copied to the host until `payloads()` / `to_bytes()` is called."""

    def __init__(self, B, padded_shape, bands=0):
        self.B = B
        self.padded_shape = padded_shape     # (H, W) of the padded images
        self.bands = bands                   # 0: legacy files; K > 0: banded files (band_len(HW, K) per scale)
        self.scales = []                     # (C, H, W, out uint8 (B*C, stride), nbytes int32 (B*C,))
        self.banded_scales = []              # bands > 0: (C, H, W, L, [(out, nbytes) of the full bands (if n > 1), of the last bands])
        self.pending = []                    # (C, H, W, intervals) of prepare_batch, consumed by Bitcoding.code
        self.done = []                       # events on the coder streams; wait() orders the current stream after them
        self.coder_stream = None             # the side stream of the last `code` call (the natural place for the D2H of the files)
        self.frame_crc = None                # Bitcoding(seal=True): int32 (B,) device tensor, CRC-32 of every padded frame (ops.u8_crc32)
        self.seal = None                     # ... and (bitstream generation, model id) of the encoder: every whole file is then sealed
        self.band_crc = None                 # Bitcoding(seal='bands'): int32 (B, 3, n) device tensor, CRC-32 of every band of the finest record's
        self.band_len = None                 # ... planes (ops.u8_crc32_bands, with frame_crc from the same pass), and that record's band length
        self.parity_group = 0                # Bitcoding(parity=G): the group size asked for (the seal states min(G, n)) ...
        self.parity = None                   # ... and (uint8 (B, 3, m, R, stride), int32 (B, 3, m)) on the finest record's coder output: of
        self.parity_streams = 1              # ops.band_parity_rs for Bitcoding(parity_streams=R) above 1, a view of ops.band_parity's slots for R = 1
        self.parity_head = False             # Bitcoding(parity_head=True): the 'L3CH' section ...
        self.head = None                     # ... and (int32 payload CRCs, uint8 slots, int32 lengths) of ops.band_payload_crc32 / ops.head_parity
                                             # over every record but the finest (ops.head_parity_layout)

    def _coder_outputs(self):
        """(C, H, W, out, nbytes) of every coder group, nbytes reshaped to (B, streams per image of that group)."""
        for C, H, W, out, nbytes in self.scales:
            yield C, H, W, out, nbytes.reshape(self.B, C)
        for C, H, W, L, groups in self.banded_scales:
            for out, nbytes in groups:
                yield C, H, W, out, nbytes.reshape(self.B, -1)

    def wait(self):
        """Make the current stream wait for the range-coder launches (they run on side streams)."""
        cur = torch.cuda.current_stream()
        for ev in self.done:
            cur.wait_event(ev)
        for _, _, _, out, nbytes in self._coder_outputs():     # allocated under the coder's side stream, consumed on this one
            out.record_stream(cur)
            nbytes.record_stream(cur)
        if self.frame_crc is not None:
            self.frame_crc.record_stream(cur)
        if self.band_crc is not None:
            self.band_crc.record_stream(cur)
        if self.parity is not None:
            for t in self.parity:
                t.record_stream(cur)
        if self.head is not None:
            for t in self.head:
                t.record_stream(cur)
        return self

    def total_payload_bytes(self):
        """int64 device tensor (B,): entropy-coded bytes per image (no host sync)."""
        self.wait()
        tot = None
        for C, H, W, out, nbytes in self._coder_outputs():
            t = nbytes.to(torch.int64)
            t = torch.where(t < 0, torch.full_like(t, -(1 << 40)), t).sum(dim=1)    # L3C_AC_OVERRUN stays visible in the sum
            tot = t if tot is None else tot + t
        return tot

    def scale_payload_bytes(self):
        """Host list over scales (coarse -> fine) of the batch's entropy-coded bytes (synchronises)."""
        self.wait()
        if self.bands:
            return [sum(int(nb.to(torch.int64).sum().item()) for _, nb in groups) for _, _, _, _, groups in self.banded_scales]
        return [int(n.to(torch.int64).sum().item()) for _, _, _, _, n in self.scales]

    def file_sizes(self):
        """(B,) file size in bytes incl. the fixed framing (container.framing_bytes)."""
        scales = [s[:4] for s in self.banded_scales] if self.bands else [s[:3] for s in self.scales]
        return self.total_payload_bytes() + container.framing_bytes(scales, bool(self.bands))

    @staticmethod
    def _checked_nbytes(n):
        """Host-side stream lengths (numpy) -> the same, or L3CError when a stream reported L3C_AC_OVERRUN (int32 -1: its intervals
        violated c_high > c_low, i.e. table rows not strictly increasing).  The ONE place that turns the device-side marker into an
        error: `payloads`, `many_to_host_buffer` (through the file sizes) and therefore every file writer go through it."""
        if (np.asarray(n) < 0).any():
            from .. import _lib
            raise _lib.L3CError('range coder overrun: a stream asked for more than 16 bits per symbol (table rows not strictly increasing)')
        return n

    def payloads(self):
        """list over scales (coarse -> fine) of [B][C] bytes objects (one D2H copy per scale); banded: [B][C] lists of the n band payloads."""
        self.wait()
        res = []
        if self.bands:
            for C, H, W, L, groups in self.banded_scales:
                n = n_bands(H * W, L)
                hosts = []
                for out, nbytes in groups:
                    nb = self._checked_nbytes(nbytes.cpu().numpy())
                    hosts.append((out[:, :max(1, int(nb.max()))].cpu().numpy(), nb))
                (full, nf), (last, nl) = (hosts[0] if n > 1 else (None, None)), hosts[-1]

                def band(b, c, j):
                    if j + 1 < n:
                        i = (b * C + c) * (n - 1) + j
                        return full[i, :nf[i]].tobytes()
                    return last[b * C + c, :nl[b * C + c]].tobytes()
                res.append([[[band(b, c, j) for j in range(n)] for c in range(C)] for b in range(self.B)])
            return res
        for C, H, W, out, nbytes in self.scales:
            n = self._checked_nbytes(nbytes.cpu().numpy())
            host = out[:, :int(n.max())].cpu().numpy()
            res.append([[host[b * C + c, :n[b * C + c]].tobytes() for c in range(C)] for b in range(self.B)])
        return res

    def to_bytes(self, padding_tuples=None):
        """-> list of B `.l3c` byte strings.  The files are assembled ON THE DEVICE (l3c_container_write: headers, length
        fields, payloads re-aligned to their byte offsets, all files back to back) and cross PCIe as one copy of exactly
        their size; the only host work left is cutting the buffer into B bytes objects."""
        return EncodedBatch.many_to_bytes([self], [padding_tuples])[0]

    def to_host_buffer(self, padding_tuples=None):
        """-> (uint8 numpy array holding the B files back to back, file offsets, file sizes).  The array is a view of a
        reused staging buffer: consume it before the next call."""
        return EncodedBatch.many_to_host_buffer([self], [padding_tuples])

    @staticmethod
    def _seals(encs, bodies, host_head=False):
        """The seal of every file of `encs` (b'' for a batch encoded without): ONE D2H of the frame CRCs (and the band CRCs of
        seal='bands' batches, the parity lengths and slots of parity=G batches, the payload CRCs, lengths and slots of parity_head=True
        batches), the band tables, parity sections and check words on the host.  host_head: the head parts come from the numpy references
        on the bodies (container.head_from_body) instead of the device's words."""
        sealed = [e for e in encs if e.seal is not None]
        if not sealed:
            return [[b''] * len(files) for files in bodies]

        def parts(e):
            e.wait()
            if e.band_crc is None:
                return (e.frame_crc,)
            if e.parity is None:
                return (e.frame_crc, e.band_crc)
            main = (e.frame_crc, e.band_crc, e.parity[1], e.parity[0].view(torch.int32))      # (the slots' stride is a multiple of 16)
            if e.head is None or host_head:
                return main
            return main + (e.head[0], e.head[2], e.head[1].view(torch.int32)) + tuple(nb for s in e.banded_scales for _, nb in s[4])
        words = torch.cat([t.reshape(-1) for e in sealed for t in parts(e)])
        words, at, res = words.cpu().numpy().view(np.uint32), 0, []
        for e, files in zip(encs, bodies):
            if e.seal is None:
                res.append([b''] * len(files))
                continue
            frame = words[at:at + e.B].tolist()
            at += e.B
            bands = [None] * e.B
            if e.band_crc is not None:
                assert e.band_len == e.banded_scales[-1][3], (e.band_len, e.banded_scales[-1][3])
                per = e.band_crc[0].numel()
                bands = [words[at + b * per:at + (b + 1) * per].reshape(3, -1) for b in range(e.B)]
                at += e.B * per
            parity = [None] * e.B
            if e.parity is not None:
                slots, lens = e.parity
                m, R = slots.shape[2], slots.shape[3]
                nb = EncodedBatch._checked_nbytes(words[at:at + lens.numel()].view(np.int32)).reshape(e.B, 3, m)
                at += lens.numel()
                host = words[at:at + slots.numel() // 4].view(np.uint8).reshape(slots.shape)
                at += slots.numel() // 4
                G = min(e.parity_group, bands[0].shape[1])
                parity = [(G, [[[host[b, c, g, r, :nb[b, c, g]].tobytes() for r in range(R)] for g in range(m)] for c in range(3)])
                          for b in range(e.B)]
            head, framing = [None] * e.B, [None] * e.B
            if e.head is not None and host_head:
                head = [container.head_from_body(body, e.parity_group, e.parity_streams) for body in files]
            elif e.head is not None:
                crc_d, slots, lens = e.head
                R, scales = e.parity_streams, list(e.banded_scales[:-1])
                shapes, offsets, stride, _, first = ops.head_parity_layout(e.B, scales, e.parity_group, R)
                crc_h = words[at:at + crc_d.numel()]
                at += crc_d.numel()
                nb = EncodedBatch._checked_nbytes(words[at:at + lens.numel()].view(np.int32))
                at += lens.numel()
                host = words[at:at + slots.numel() // 4].view(np.uint8)
                at += slots.numel() // 4
                head, crc_at = [[] for _ in range(e.B)], 0
                for (C, n, m), off, f in zip(shapes, offsets, first):
                    crcs = crc_h[crc_at:crc_at + e.B * C * n].reshape(e.B, C, n)
                    crc_at += e.B * C * n
                    rows = host[off:off + e.B * C * m * R * stride].reshape(e.B, C, m, R, stride)
                    lk = nb[f:f + e.B * C * m].reshape(e.B, C, m)
                    for b in range(e.B):
                        head[b].append((crcs[b], [[[rows[b, c, g, r, :lk[b, c, g]].tobytes() for r in range(R)] for g in range(m)]
                                                  for c in range(C)]))
                lengths = []                                     # every record's (B, C, n) length fields: the framing copy needs no walk of the files
                for C, Hs, Ws, Ls, groups in e.banded_scales:
                    per = []
                    for _, nb_d in groups:                       # the full bands (B C (n - 1)), then the last bands (B C)
                        per.append(EncodedBatch._checked_nbytes(words[at:at + nb_d.numel()].view(np.int32)).reshape(e.B, C, -1))
                        at += nb_d.numel()
                    lengths.append(np.concatenate(per, axis=2))
                framing = [([s[:4] for s in e.banded_scales], [nb[b] for nb in lengths]) for b in range(e.B)]
            res.append([container.make_seal(body, e.seal[0], frame[b], e.seal[1], bands[b], e.band_len, parity=parity[b], head=head[b], head_framing=framing[b])
                        for b, body in enumerate(files)])
        return res

    def _write_container(self, dst, offsets, padding_tuples):
        """Enqueue the assembly of this batch's files into `dst` at the (device, int64) byte `offsets`."""
        from .. import _lib
        B = self.B
        pads = np.asarray(padding_tuples if padding_tuples else [(0, 0, 0, 0)] * B, dtype=np.uint16).reshape(B, 4)
        pads = torch.from_numpy(pads.view(np.int16)).cuda()
        if self.bands:
            arr = (_lib.BandedScale * len(self.banded_scales))()
            for k, (C, H, W, L, groups) in enumerate(self.banded_scales):
                (out_f, nb_f), (out_l, nb_l) = (groups[0] if len(groups) == 2 else (None, None)), groups[-1]
                arr[k] = _lib.BandedScale(ops.ptr(out_f, torch.uint8), ops.ptr(nb_f, torch.int32), out_f.shape[1] if out_f is not None else 0,
                                          ops.ptr(out_l, torch.uint8), ops.ptr(nb_l, torch.int32), out_l.shape[1], C, H, W, L)
            n_ws = _lib.load().l3c_container_write_banded_workspace_bytes(arr, len(arr), B)
            _lib.check(min(0, n_ws))
            ws = torch.empty(n_ws, dtype=torch.uint8, device='cuda')
            ops.call('l3c_container_write_banded', arr, len(arr), B, ops.ptr(pads), ops.ptr(offsets, torch.int64), ops.ptr(dst), ops.ptr(ws),
                     n_ws, ops.stream())
            return
        arr = (_lib.ContainerScale * len(self.scales))()
        for k, (C, H, W, out, nbytes) in enumerate(self.scales):
            arr[k] = _lib.ContainerScale(ops.ptr(out, torch.uint8), ops.ptr(nbytes, torch.int32), out.shape[1], C, H, W)
        ops.call('l3c_container_write', arr, len(self.scales), B, ops.ptr(pads), ops.ptr(offsets, torch.int64), ops.ptr(dst),
                 ops.stream())

    @staticmethod
    def many_to_host_buffer(encs, padding_lists=None):
        """The files of several EncodedBatches in ONE device buffer, ONE host synchronisation (their sizes) and ONE D2H copy.
        -> (uint8 numpy array, file offsets, file sizes); files in the order of `encs`, batch order inside."""
        if any(e.seal is not None for e in encs):
            raise ValueError('the packed host buffer holds unsealed files back to back and cannot carry a seal: to_bytes / many_to_bytes '
                             'return the sealed files of Bitcoding(seal=True)')
        return EncodedBatch._many_to_host_buffer(encs, padding_lists)

    @staticmethod
    def _many_to_host_buffer(encs, padding_lists=None):
        for e in encs:
            e.wait()
        sizes = torch.cat([e.file_sizes() for e in encs])
        offs = torch.cumsum(sizes, 0) - sizes
        # the synchronisation: how many bytes there are (an overrun stream makes its file's size hugely negative: total_payload_bytes)
        sizes_h = EncodedBatch._checked_nbytes(sizes.cpu().numpy().astype(np.int64))
        total = int(sizes_h.sum())
        dst = torch.empty(total, dtype=torch.uint8, device='cuda')
        first = 0
        for i, e in enumerate(encs):
            e._write_container(dst, offs[first:first + e.B].contiguous(), padding_lists[i] if padding_lists else None)
            first += e.B
        host = _staging(total)
        host.copy_(dst)
        torch.cuda.current_stream().synchronize()
        offs_h = np.concatenate([[0], np.cumsum(sizes_h)[:-1]]).astype(np.int64)
        return host.numpy(), offs_h, sizes_h

    @staticmethod
    def many_to_bytes(encs, padding_lists=None):
        """-> per EncodedBatch the list of its `.l3c` byte strings."""
        host, offs, sizes = EncodedBatch._many_to_host_buffer(encs, padding_lists)
        res, k = [], 0
        for e in encs:
            res.append([host[offs[k + b]:offs[k + b] + sizes[k + b]].tobytes() for b in range(e.B)])
            k += e.B
        if any(e.seal is not None for e in encs):
            res = [[f + s for f, s in zip(files, seals)] for files, seals in zip(res, EncodedBatch._seals(encs, res))]
        return res

    def to_bytes_host_assembled(self, padding_tuples=None):
        """Reference implementation of `to_bytes` on the host (per-scale copies + Python joins; the head part of a parity_head=True batch from
        container.rs_parity and zlib.crc32 on the payloads); kept for the tests."""
        pl = self.payloads()
        scales = [s[:4] for s in self.banded_scales] if self.bands else [s[:3] for s in self.scales]
        files = [container.write_file(padding_tuples[b] if padding_tuples else (0, 0, 0, 0), scales, [p[b] for p in pl], bool(self.bands))
                 for b in range(self.B)]
        return [f + s for f, s in zip(files, EncodedBatch._seals([self], [files], host_head=True)[0])]


class Bitcoding(object):
    def __init__(self, blueprint, times=None, compare_with_theory=False, coder_cus=0, auto_recurse=0, file_writer=None,
                 coder_streams=4, forward_streams=3, decode_overlap=None, rgb_window='auto', bands=0, seal=False, parity=0, parity_streams=1,
                 parity_head=False):
        """coder_streams: side streams the range-coder launches rotate over; forward_streams: streams `encode_many` spreads the forward
        passes of a heterogeneous set over (used when the HIP runtime runs with >= 8 hardware queues -- helpers/runtime.py; the package
        does NOT ask for them on import: applications that code image sets call l3c_pytorch_amd.configure_hip_queues() before their
        first HIP call -- else one, with a warning); decode_overlap: None = the chunk-pipelined RGB decode overlaps its table
        and decoder launches from 16 images on, True / False force either; rgb_window: 'auto' = the RGB decoder builds 64-entry table
        rows around the mixture mean where the previous chunks of the stream say that pays, 'always' / 'never' force either form
        (_decode_rgb_pipelined).  None of these changes a bit of a file or of a decoded image.
        coder_cus > 0: reserve that many compute units for the range coder.  `self.compute_stream` is then a stream
        confined to the remaining CUs -- run the network under `torch.cuda.stream(bc.compute_stream)` so the MFMA-bound
        conv kernels and the latency-bound coder wavefronts never share a SIMD (they slow the coder down 2.3x).
        auto_recurse: RGB Shared baseline only -- how many times the coarsest scale is applied again (the reference evaluates it
        with 3, multiscale_tester.py:50, and has no file coding for it, :187-188; here the `.l3c` layout simply carries one more
        scale record per recursion, and the decoder counts the records).
        file_writer: an AsyncFileWriter -- `encode` then hands the finished bytes to its worker threads instead of writing them
        itself, `decode` waits for a pending write of the path it is asked to read.
        bands: 0 = the legacy format (byte for byte); K in 1..1024 = BANDED files: every channel of every scale cut into at most K
        independently coded bands (band_len), so that one image's serial coder chains are K times shorter.  The decoder reads either
        format whatever this says.
        seal: True = every whole file this object returns or writes (to_bytes, many_to_bytes, encode and its .partN files) ends with a
        24-byte SEAL (container.make_seal): the bitstream generation, the checkpoint's id and the CRC-32 of the padded frame, computed on the
        device (ops.u8_crc32) while the encode is enqueued; the body of a sealed file is the unsealed file.  The decoder verifies every
        sealed file whatever this says (decode_batch).
        seal='bands' (banded files only: ValueError with bands=0): a BAND SEAL instead (container.make_seal with band_crcs; INTEGRATION.md
        "Band seals"): in front of the 24 bytes a table of one CRC-32 per band of the finest record -- ops.u8_crc32_bands on the input
        frames, the frame CRC from the same pass.  decode_batch then names the damaged bands and rows of a file that fails, and
        decode_region verifies exactly the bands it decoded.
        parity=G (G >= 1; needs seal='bands': ValueError otherwise; INTEGRATION.md "Parity bands"): seal version 3 -- in front of the band table
        an XOR parity over the band payloads of the finest record, one parity stream per group of min(G, n) bands of a channel
        (ops.band_parity on the coder's output, enqueued with the encode), about 1 / G of the file's size.  decode_repair then rebuilds
        one damaged band per group bit-exactly; every other reader reads the file as the band-sealed file it contains.  0: every byte
        written is the band-sealed file's.
        parity_streams=R (1..4; R > 1 needs parity=G, and min(G, bands) <= 255: ValueError otherwise): R parity rows per group over GF(2^8)
        (ops.band_parity_rs; container.rs_parity), the 'L3CQ' section, about R / G of the file's size.  decode_repair then rebuilds up to R
        damaged bands per group, and a damaged parity row still leaves R - 1 usable.  1: every byte written is today's 'L3CP' file's.
        parity_head=True (needs parity=G: ValueError otherwise; INTEGRATION.md "Head parity"): the section becomes an 'L3CH' section, which
        also protects the HEAD of the file -- the file header, every coarser record, and the finest record's header, length fields and
        separator: a copy of the framing, a CRC-32 per coarse band payload (ops.band_payload_crc32) and R parity rows per group of
        min(G, n_k) of them (ops.head_parity), both one launch over all coarser records behind the coder.  decode_repair heals the head
        first (container.heal_head); every other reader reads the file as the band-sealed file it contains.  The model must write 1..8
        scale records in front of the finest (ops.HEAD_MAX_RECORDS, what one launch takes; the format itself allows 16): prepare_batch
        raises ValueError otherwise, before anything is coded.  False: every byte written and every library call made is the 'L3CP' /
        'L3CQ' file's."""
        if seal not in (False, True, 'bands'):
            raise ValueError("seal must be False, True or 'bands', got {!r}".format(seal))
        if isinstance(parity, bool) or not isinstance(parity, int) or parity < 0:
            raise ValueError('parity must be 0 or a group size >= 1, got {!r}'.format(parity))
        if parity and seal != 'bands':
            raise ValueError("parity needs seal='bands': the band seal is what turns damage into erasures of known position")
        self.parity = parity
        if isinstance(parity_streams, bool) or not isinstance(parity_streams, int) or not 1 <= parity_streams <= container.MAX_PARITY_STREAMS:
            raise ValueError('parity_streams must be in 1..{}, got {!r}'.format(container.MAX_PARITY_STREAMS, parity_streams))
        if parity_streams > 1 and not parity:
            raise ValueError('parity_streams > 1 needs parity=G: the rows are computed over the parity groups')
        if parity_streams > 1:
            container.check_parity_streams(parity_streams, parity, int(bands))
        self.parity_streams = parity_streams
        if not isinstance(parity_head, bool):
            raise ValueError('parity_head must be True or False, got {!r}'.format(parity_head))
        if parity_head and not parity:
            raise ValueError('parity_head needs parity=G: the head rows are computed over groups of min(G, n) bands with its parity_streams')
        self.parity_head = parity_head
        if seal == 'bands' and not bands:
            raise ValueError("seal='bands' needs banded files: a band seal holds a CRC per band of the finest record (bands=K, K >= 1)")
        if bands and not 1 <= int(bands) <= MAX_BANDS:
            raise ValueError('bands must be 0 (legacy format) or in 1..{}, got {}'.format(MAX_BANDS, bands))
        self.bands = int(bands)
        self.seal = bool(seal)
        self.seal_bands = seal == 'bands'
        self._model_id = None
        self.blueprint = blueprint
        self.auto_recurse = int(auto_recurse)
        if self.auto_recurse and not blueprint.net.config_ms.rgb_bicubic_baseline:
            raise ValueError('auto_recurse is only defined for the RGB baselines')
        if self.auto_recurse and blueprint.net.scales != 1:
            # the decoder accepts extra scale records only for the single-scale RGB Shared model (decode_batch), like the tester's
            # --recursive flag (multiscale_tester.py:123-132): a file written otherwise could never be read back
            raise ValueError('auto_recurse needs the single-scale RGB Shared model (num_scales == 1)')
        self.file_writer = file_writer
        self.compare_with_theory = compare_with_theory
        self.times = times if times is not None else _NullTimes()
        self._const = {}
        # streams and helpers created on first use (_side_stream, encode_many, set_decoder)
        self._coder_streams = None
        self._fwd_streams = None
        self._set_decoder = None
        self.coder_cus = coder_cus
        self.compute_stream = None
        self.N_SIDE_STREAMS = max(1, int(coder_streams))
        self.N_FORWARD_STREAMS = max(1, int(forward_streams))
        self.decode_overlap = decode_overlap
        if rgb_window not in ('auto', 'always', 'never'):
            raise ValueError('rgb_window must be auto, always or never')
        self.rgb_window = rgb_window
        if coder_cus:
            from .. import _lib
            _, n_cu, _ = _lib.device_info()
            self.compute_stream = _lib.cu_range_stream(0, n_cu - coder_cus)
            self._coder_range = (n_cu - coder_cus, coder_cus)

    # [measured, profiles/r02_coder_streams_small_batches.log] 8 or 12 side streams do not help with the runtime's default of four
    # hardware queues (they alias); with GPU_MAX_HW_QUEUES=8, four streams reach 27.8 / 75.7 MPix/s at 1 / 4 images per step
    N_SIDE_STREAMS = 4        # (instances: the constructor's coder_streams)

    def _side_stream(self):
        """Side stream for the range coder: its launches are a handful of long-running wavefronts (a lane per stream),
        so they are overlapped with whatever the main stream does next (the next batch's convolutions).  Consecutive
        calls rotate over N_SIDE_STREAMS streams so that the coder launches of successive batches may overlap too."""
        if self._coder_streams is None:
            if self.coder_cus:
                from .. import _lib
                make = lambda: _lib.cu_range_stream(*self._coder_range)   # noqa: E731
            else:
                make = torch.cuda.Stream
            self._coder_streams = [make() for _ in range(self.N_SIDE_STREAMS)]
            self._stream_turn = 0
        self._stream_turn = (self._stream_turn + 1) % self.N_SIDE_STREAMS
        return self._coder_streams[self._stream_turn]

    # ---- constants --------------------------------------------------------------------------------------------------

    def _targets(self, dmll):
        key = ('t', dmll.x_min, dmll.x_max, dmll.L)
        if key not in self._const:
            self._const[key] = dmll.coding_targets('cuda')
        return self._const[key]

    def _uniform_row(self, L):
        key = ('u', L)
        if key not in self._const:
            self._const[key] = uniform_cdf_row(L).cuda()
        return self._const[key]

    def model_id(self):
        """The checkpoint's id in a seal (modules/schema.model_id), computed on first use."""
        if self._model_id is None:
            net = self.blueprint.net
            self._model_id = schema.model_id(net.state_dict(), net.config_ms)
        return self._model_id

    @staticmethod
    def generation():
        from .. import _lib
        return _lib.load().l3c_bitstream_generation()

    def n_predicted_scales(self):
        """Scales coded with the network's prediction (the coarsest one on top of them is coded with the uniform prior)."""
        return self.blueprint.net.scales + self.auto_recurse

    def padding_factor(self):
        return 2 ** self.n_predicted_scales()

    def iter_scale_dmll(self, n_predicted=None):
        """coarsest -> finest: (scale, dmll, uniform)   (reference :163-169; for the RGB baselines every scale is an RGB scale)"""
        losses = self.blueprint.losses
        n = self.n_predicted_scales() if n_predicted is None else n_predicted
        for scale in reversed(range(n + 1)):
            yield (scale, losses.loss_dmol_rgb if scale == 0 else losses.loss_dmol_n, scale == n)

    # ---- native batched API -----------------------------------------------------------------------------------------

    def prepare_batch(self, imgs, out=None):
        """First half of `encode_batch`: network forward (unless `out` is given) and, per scale, the fused head that
        turns P and the symbols into the coding intervals of all B*C streams.  Everything is enqueued on the current
        stream.  -> EncodedBatch whose `pending` list awaits `code()`."""
        net = self.blueprint.net
        fac = self.padding_factor()
        B, _, H, W = imgs.shape
        assert H % fac == 0 and W % fac == 0, 'pad first: {}x{} not divisible by {}'.format(H, W, fac)
        if out is None:
            out = net(imgs.to('cuda', torch.float32), self.auto_recurse)
        assert len(out.raw.P) == self.n_predicted_scales(), (len(out.raw.P), self.n_predicted_scales())
        raw = out.raw
        K = net.config_ms.prob.K
        enc = EncodedBatch(B, (H, W), self.bands)
        if self.seal_bands:
            enc.band_len = band_len(H * W, self.bands)
            enc.band_crc, enc.frame_crc = ops.u8_crc32_bands(imgs.to('cuda').to(torch.uint8).contiguous().view(-1), B, H * W, enc.band_len)
            enc.seal = (self.generation(), self.model_id())
            enc.parity_group, enc.parity_streams, enc.parity_head = self.parity, self.parity_streams, self.parity_head
        elif self.seal:
            enc.frame_crc = ops.u8_crc32(imgs.to('cuda').to(torch.uint8).contiguous().view(-1), B, 3 * H * W)
            enc.seal = (self.generation(), self.model_id())
        for scale, dmll, uniform in self.iter_scale_dmll():
            sym = raw.sym[scale]
            _, C, Hs, Ws = sym.shape
            if uniform:
                iv = ops.intervals_from_table(self._uniform_row(dmll.L), sym.reshape(B * C, Hs * Ws), B * C, Hs * Ws,
                                              broadcast_row=True)
            else:
                iv = ops.dmll_encode_intervals(raw.P[scale], sym.contiguous(), self._targets(dmll), C, K, dmll.rgb_scale)
            enc.pending.append((C, Hs, Ws, iv))
        if enc.parity_head and not 1 <= len(enc.pending) - 1 <= ops.HEAD_MAX_RECORDS:
            raise ValueError('parity_head needs 1..{} scale records in front of the finest (one l3c_head_parity launch takes that many), this '
                             'model writes {} record(s)'.format(ops.HEAD_MAX_RECORDS, len(enc.pending)))
        return enc

    def code(self, batches):
        """Second half: ONE grouped range-coder launch (l3c_ac_encode_groups) over every scale of every prepared batch
        -- all their streams are coded concurrently, whatever the image sizes -- on a side stream that the current
        stream does not wait for.  Returns `batches`.
        Banded batches: l3c_ac_band_intervals first re-lays every scale's intervals into its full bands and its last bands -- two groups of
        equally long streams -- and the same grouped launch pair codes every band of every scale."""
        if not any(enc.pending for enc in batches):
            return batches
        main, side = torch.cuda.current_stream(), self._side_stream()
        ready = torch.cuda.Event()
        ready.record(main)
        with torch.cuda.stream(side):
            side.wait_event(ready)
            groups, owners = [], []
            for enc in batches:
                for C, Hs, Ws, iv in enc.pending:
                    iv.record_stream(side)
                    if enc.bands:
                        L = band_len(Hs * Ws, enc.bands)
                        gs = ops.band_intervals(iv, enc.B * C, Hs * Ws, L)
                        owners.append((enc, (C, Hs, Ws, L), len(gs)))
                        groups += gs
                    else:
                        owners.append((enc, (C, Hs, Ws), 1))
                        groups.append((iv, enc.B * C, Hs * Ws))
            results, ws = ops.ac_encode_groups(groups)
            g, finest, coarser = 0, {}, {}
            for enc, shape, n_groups in owners:                 # (coarse -> fine: the last record of a batch is its finest)
                if id(enc) in finest and enc.parity_head:
                    coarser.setdefault(id(enc), []).append(finest[id(enc)][1] + (finest[id(enc)][2],))
                finest[id(enc)] = (enc, shape, results[g:g + n_groups])
                g += n_groups
            for enc, shape, coded in finest.values():
                if enc.parity_group:                             # behind the coder on its stream: nothing waits
                    _, Hs, Ws, L = shape
                    G = min(enc.parity_group, n_bands(Hs * Ws, L))
                    if enc.parity_streams > 1:
                        container.check_parity_streams(enc.parity_streams, G, G)
                        enc.parity = ops.band_parity_rs(enc.B, Hs, Ws, L, coded, G, enc.parity_streams)
                    else:
                        slots, nb = ops.band_parity(enc.B, Hs, Ws, L, coded, G)
                        enc.parity = (slots.unsqueeze(3), nb)
                    if enc.parity_head:                          # all coarser records at once: two launches, whatever their count
                        scales = coarser[id(enc)]
                        enc.head = (ops.band_payload_crc32(enc.B, scales),) + ops.head_parity(enc.B, scales, enc.parity_group, enc.parity_streams)
            done = torch.cuda.Event()
            done.record(side)
        g = 0
        for enc, shape, n_groups in owners:
            if enc.bands:
                enc.banded_scales.append(shape + (results[g:g + n_groups],))
            else:
                enc.scales.append(shape + results[g])
            g += n_groups
        for enc in batches:
            enc.pending = []
            enc.done.append(done)
            enc.coder_stream = side
        return batches

    def encode_batch(self, imgs, out=None):
        """imgs: (B,3,H,W), H and W multiples of 2**num_scales, values 0..255 (any dtype / device).
        Enqueues the whole encode and returns an EncodedBatch (no host sync).
        `out`: a network output for `imgs` computed earlier (avoids a second forward)."""
        return self.code([self.prepare_batch(imgs, out)])[0]

    N_FORWARD_STREAMS = 3     # (instances: the constructor's forward_streams) used when the HIP runtime was given >= 8 hardware queues, see encode_many
    N_CODER_GROUPS = 4

    def encode_many(self, batches, upload=None, on_group=None, n_groups=None, weights=None):
        """batches: list of (B_i,3,H_i,W_i) tensors (shapes may differ between entries).  -> list, in the order given, of EncodedBatch.
        Small batches leave most of the machine idle (one 768x512 image is 192 tiles at the first scale, 12 at the
        coarsest, for 256 CUs) and their serial coder chains are as long as ever, so
          * the forward passes + heads of different batches run on N_FORWARD_STREAMS streams side by side, largest
            batches first -- only if the process runs with GPU_MAX_HW_QUEUES >= 8: with the runtime's default of 4
            hardware queues the extra streams alias the coder's queue and the long coder kernel stalls them
            [measured: 64 images of 36 shapes end to end: 42 MPix/s on one stream, 38-43 on three with 4 queues, 52 with 8];
          * the range coder is launched N_CODER_GROUPS times (one grouped launch per quarter of the set, on the side
            streams), so that the long chains of the early, large images overlap the later forward passes and only the
            short chains of the smallest images are left at the end.
        Host pipelining (helpers/dataset_codec.encode_set): `upload(entry)` turns an entry of `batches` into its device tensor
        right before that forward pass is enqueued, under the forward stream (staging + H2D of batch k+1 then overlap the GPU's
        work on batch k; `weights[i]` = the entry's pixel count, for the largest-first order); `on_group(list of (index,
        EncodedBatch))` is called for a coder group as soon as its launch has completed (polled after every enqueued pass; the
        rest at the end), under the side stream that coded it -- the D2H and the host's slicing of finished files overlap the
        later groups' forward passes."""
        if not batches:
            return []
        self.blueprint.net._prepare()                  # pack the weights before forking streams
        if weights is None:
            weights = [b.shape[0] * b.shape[2] * b.shape[3] for b in batches]
        order = sorted(range(len(batches)), key=lambda i: -weights[i])
        main = torch.cuda.current_stream()
        from ..helpers import runtime
        if runtime.forward_streams_allowed(self.N_FORWARD_STREAMS) > 1:
            if self._fwd_streams is None:
                self._fwd_streams = [torch.cuda.Stream() for _ in range(self.N_FORWARD_STREAMS)]
            fwd = self._fwd_streams
        else:
            fwd = [main]
        start = torch.cuda.Event()
        start.record(main)
        for st in fwd:
            if st is not main:
                st.wait_event(start)
        cuts = set(coder_group_cuts(len(order), n_groups or self.N_CODER_GROUPS))
        result = [None] * len(batches)
        pending, coded = [], []

        def flat(k):
            return [result[k]]

        def collect_finished(block):
            # oldest group first; without `block` only groups whose coder launch has COMPLETED (the host must never sit waiting for a
            # latency-bound coder launch while the forward streams run dry)
            while coded and (block or flat(coded[0][0])[0].done[-1].query()):
                self._collect(coded.pop(0), result, on_group)

        for n, i in enumerate(order):
            st = fwd[n % len(fwd)]
            with torch.cuda.stream(st):
                x = batches[i] if upload is None else upload(batches[i])
                if x.is_cuda:
                    x.record_stream(st)
                result[i] = self.prepare_batch(x)
                ev = torch.cuda.Event()
                ev.record(st)
            pending.append((i, ev))
            if n + 1 in cuts:
                for _, ev in pending:
                    main.wait_event(ev)            # `code` orders its side stream after the current stream
                self.code([e for k, _ in pending for e in flat(k)])
                if on_group is not None:
                    coded.append([k for k, _ in pending])
                pending = []
            collect_finished(False)
        collect_finished(True)
        return result

    @staticmethod
    def _collect(indices, result, on_group):
        first = result[indices[0]]
        with torch.cuda.stream(first.coder_stream):
            on_group([(k, result[k]) for k in indices])

    def decode_batch(self, files, out_dtype=torch.int64, verify=True):
        """files: list of B `.l3c` byte strings of equally sized (padded) images -> ((B,3,H,W) int64 on the GPU (the reference's
        dtype, bitcoding.py:125-161; out_dtype: torch.uint8 / int16 for callers that want the pixels without the 8-byte form),
        list of padding tuples).
        Round 6: the host only parses the FRAMING (a few length fields per file, `parse_containers`); the files cross PCIe as they
        are, in one copy from a page-locked buffer, and one kernel (l3c_container_read) cuts every stream out of them in the
        aligned, zero-padded form the range decoders read -- before, 14 `pack_streams` calls copied every payload on the host
        and uploaded it from pageable memory.
        (Tried and dropped [measured, batch 128]: cutting the batch into 2-4 parts that run the same chain on streams of their
        own, so that one part's latency-bound decoder launches would leave room for another part's convolutions and tables:
        0.70 s became 0.87 - 2.98 s with the runtime's four hardware queues (the parts' main and side streams alias and serialise
        each other's long decoder launches) and 0.76 / 1.00 s with 8 or 16 queues -- a decoder wavefront that shares its SIMD
        with MFMA wavefronts runs 2.3x slower, which costs more than the overlap saves; profiles/r02_decode_parts_tried.log.)
        SEALED files (container.split_seal; a batch may mix sealed and unsealed ones): the seals are split off, then -- verify=True --
        every seal's generation and, where both sides state one, its model id are checked BEFORE anything is enqueued
        (container.SealError, reason 'generation' / 'model'); after the decode ops.u8_crc32 hashes the decoded frames on the device and ONE
        D2H of B words is compared with the seals (SealError, reason 'pixels').  verify=False strips the seals and checks nothing.
        BAND-SEALED files among them (Bitcoding(seal='bands')): ONE ops.u8_crc32_bands on the decoded frames instead, one D2H; every
        band-sealed file is compared band by band -- SealError('pixels') then carries .bands and .rows, the damaged bands and their
        rows in the unpadded image; every other row is verified and can be fetched with decode_region --, the version-1 sealed files of
        the batch against the same call's frame words."""
        split = [container.split_seal(f, view=True) for f in files]
        files, seals = [b for b, _ in split], [s for _, s in split]
        check = verify and any(s is not None for s in seals)
        if check:
            container.check_seals(seals, self.generation(), self.model_id)
        out, padding = self._decode_batch(files, torch.uint8 if check else out_dtype, None)
        if check:
            self._check_pixels(seals, out, padding)
            out = out.to(out_dtype)
        return out, padding

    @staticmethod
    def _check_pixels(seals, out, padding):
        """The decoded uint8 frames `out` (B, 3, H, W) against their seals: one hash call, one D2H; SealError('pixels')."""
        B, _, H, W = out.shape
        band_lens = {s.band_len for s in seals if s is not None and s.band_crcs is not None}
        if not band_lens:
            container.check_frame_crcs(seals, ops.u8_crc32(out.view(-1), B, out.numel() // B).cpu().numpy())
            return
        L, = band_lens                       # (the files of a batch share every record's band length: container.parse_batch)
        bands, frames = ops.u8_crc32_bands(out.view(-1), B, H * W, L)
        words = torch.cat([frames, bands.view(-1)]).cpu().numpy()
        container.check_band_crcs(seals, words[B:].reshape(B, 3, -1), (H, W), padding, 0, words[:B])

    def decode_salvage(self, files, out_dtype=torch.uint8):
        """decode_batch(verify=True) that CONCEALS what does not verify instead of raising -> ((B,3,H,W) out_dtype on the GPU, list of padding
        tuples, container.SalvageInfo).  The pre-decode checks still raise (SealError 'generation' / 'model' are not damage), and so does
        an invalid file.  The decode is decode_batch's; this entry point alone keeps the finest scale's P and the int16 symbols alive past
        the CRC check: ONE ops.u8_crc32_bands and its D2H, container.failing_bands, then for every band position j of a band-sealed file
        with a failing channel one span (file, j L, min(L, HW - j L), mask of the failing channels) of ONE ops.dmll_conceal call -- the
        mixture's mean, conditioned on the channels of the pixel that verified -- and one ops.sym_to_u8.  Every verified pixel comes back
        exact; info says which is which (concealed, rows, lost, unverified).  An intact batch: no conceal launch, the pixels of
        decode_batch.  Legacy files among banded ones are refused as decode_batch refuses them."""
        seals, records, framing, streams, sym, P, dmll = self._decode_keeping_finest(files)
        pixels, info = self._salvage(seals, sym.to(torch.uint8), sym, P, framing.padding, self.blueprint.net.config_ms.prob.K,
                                     (dmll.x_min, dmll.x_max, dmll.L))
        return pixels.to(out_dtype), framing.padding, info

    def _decode_keeping_finest(self, files, heads=None):
        """What decode_salvage and decode_repair open with: the seals split off and checked (SealError 'generation' / 'model'), the files
        parsed and uploaded, decode_batch's walk with the finest scale's P and mixture kept
        -> (seals, records, framing, streams, int16 symbols (B, 3, H, W), P, dmll)."""
        parts = [None if h is None else h.part for h in heads or [None] * len(files)]      # (decode_repair: what heal_head has read already)
        split = [container.split_seal(f, view=True, head=p) for f, p in zip(files, parts)]
        files, seals = [b for b, _ in split], [s for _, s in split]
        if any(s is not None for s in seals):
            container.check_seals(seals, self.generation(), self.model_id)
        records, framing, banded = container.parse_batch(files)
        n_pred = self._n_predicted(len(records))
        self._check_coarsest(records[0], banded, int(framing.nbytes[0].max()))
        streams = upload._upload_streams(files, framing)
        kept = {}
        sym = self._walk_records(records, framing, banded, streams, n_pred, len(records), None, keep_finest=kept)
        return seals, records, framing, streams, sym, kept['P'], kept['dmll']

    @staticmethod
    def _salvage(seals, pixels, sym, P, padding, K, alphabet, words=None):
        """The decoded uint8 frames `pixels` (B, 3, H, W) against their seals, as _check_pixels -- one hash call, one D2H --, then the
        concealment of what failed in `sym` (int16, the same values) from P (the finest scale's, a tensor or a device pointer)
        -> (pixels, container.SalvageInfo); `pixels` itself where nothing was concealed.  words (decode_repair): the hash call's words as
        _band_words returns them, already on the host: nothing is hashed here."""
        B, _, H, W = pixels.shape
        HW = H * W
        unverified = [i for i, s in enumerate(seals) if s is None]
        band_lens = {s.band_len for s in seals if s is not None and s.band_crcs is not None}
        if not band_lens:
            lost = []
            if len(unverified) < B:
                crcs = ops.u8_crc32(pixels.view(-1), B, pixels.numel() // B).cpu().numpy()
                lost = [i for i, s in enumerate(seals) if s is not None and (int(crcs[i]) & 0xffffffff) != s.frame_crc]
            return pixels, container.SalvageInfo({}, {}, lost, unverified, {}, B)
        L, = band_lens                       # (the files of a batch share every record's band length: container.parse_batch)
        if words is None:
            words = Bitcoding._band_words(pixels, L)
        failed, concealed, rows = container.failing_bands(seals, words[B:].reshape(B, 3, -1), (H, W), padding, 0, words[:B])
        n = container.n_bands(HW, L)
        lost, spans = [], []
        for i in failed:
            if i not in concealed:           # a version-1 seal: the frame CRC says that something is wrong, not where
                lost.append(i)
                continue
            masks = {}
            for c, j in concealed[i]:
                masks[j] = masks.get(j, 0) | (1 << c)
            if len(masks) == n:
                lost.append(i)
            spans += [(i, j * L, min(L, HW - j * L), m) for j, m in sorted(masks.items())]
        if spans:
            ops.dmll_conceal(P, sym, spans, K, *alphabet)
            pixels = ops.sym_to_u8(sym)
        total = {i: 3 * n for i, s in enumerate(seals) if s is not None and s.band_crcs is not None}
        return pixels, container.SalvageInfo(concealed, rows, lost, unverified, total, B)

    @staticmethod
    def _band_words(pixels, L):
        """The frame words (B) and band words (B 3 n) of the uint8 frames `pixels` (B, 3, H, W) on the host: one hash call, one D2H."""
        B, _, H, W = pixels.shape
        bands, frames = ops.u8_crc32_bands(pixels.view(-1), B, H * W, L)
        return torch.cat([frames, bands.view(-1)]).cpu().numpy()

    def decode_repair(self, files, out_dtype=torch.uint8):
        """decode_salvage that first REBUILDS what the parity of a version-3 file (Bitcoding(parity=G)) can rebuild, bit-exactly
        -> ((B,3,H,W) out_dtype on the GPU, list of padding tuples, container.RepairInfo).
        The decode, the hash call and container.failing_bands are decode_salvage's; an intact batch makes the same library calls: no
        parity is uploaded, no XOR kernel launched.  A failing band position's ERASURE is its lowest failing channel c (the channels below
        verified, so with the right P that payload is the damaged one).  A group (file, c, g) -- the bands { j : j % m == g } of channel
        c -- is rebuilt when it holds exactly one erasure and every other member verifies at channel c.  A ROUND: the parity payloads
        of those groups go up (a small H2D), ONE ops.u8_xor_spans rebuilds every payload of the round from its parity stream and the
        group's other members (which are on the device already) in the decoders' aligned form, the positions' symbols are zeroed, ONE
        ops.decode_rgb_entries decodes them against the kept P, ops.sym_to_u8, and ONE ops.u8_crc32_spans hashes their bands again.
        Rounds repeat while one verified a band more and failures remain (a band whose other channel is damaged too, in another group,
        takes a second round); no payload is rebuilt twice.  The band CRCs stay the arbiter: a payload counts as repaired only when all
        three channels of its position verify.  What still fails is concealed as decode_salvage conceals it (info.salvage).
        Files with R = 2..4 parity rows per group ('L3CQ', Bitcoding(parity_streams=R)): a group is rebuilt when it holds t = 1..R erasures
        and every other member verifies.  The rows r0 .. r0 + t - 1 go up, container.rs_repair_coefficients inverts the t x t system on the
        host, and every rebuilt payload is one group of ONE ops.u8_gf_spans call per round (the 'L3CP' files of the batch keep their ONE
        ops.u8_xor_spans call).  r0 = 0 first; where the group's positions still fail and t < R, a later round takes r0 = 1 .. R - t -- what
        survives a damaged parity row.  No (group, erasure set, window) is tried twice.
        info.files: per file the HEALED file -- the rebuilt payloads spliced in at their framing offsets, the same length, section, table
        and seal --, None where nothing was repaired.  Files without parity, intact files and unsealed files: decode_salvage.
        Files with an 'L3CH' section (Bitcoding(parity_head=True)): container.heal_head runs on every file BEFORE anything else, on the host
        -- it rewrites damaged framing fields from the section's copy and rebuilds damaged payloads of the coarser records --, so everything
        above sees a file with valid framing and coarse records; info.head says per file what it did, info.files holds the healed file.
        An intact file costs one zlib.crc32 over its coarser records and makes exactly the library calls of the 'L3CQ' file."""
        mended = [container.heal_head(f) for f in files]          # host only; an intact file comes back as the object it is
        given, files, heads = files, [f for f, _ in mended], [h for _, h in mended]
        seals, records, framing, streams, sym, P, dmll = self._decode_keeping_finest(files, heads)
        K = self.blueprint.net.config_ms.prob.K
        pixels, B = sym.to(torch.uint8), len(files)
        band_lens = {s.band_len for s in seals if s is not None and s.band_crcs is not None}
        words, repaired, healed, rounds = None, {}, [None] * B, 0
        if band_lens:
            L, = band_lens
            words = self._band_words(pixels, L)
            if any(s is not None and s.parity is not None for s in seals):
                pixels, repaired, healed, rounds = self._repair(files, seals, records[-1], framing, streams, pixels, sym, P, dmll, K, words)
        pixels, salvage = self._salvage(seals, pixels, sym, P, framing.padding, K, (dmll.x_min, dmll.x_max, dmll.L), words)
        rows = {i: container.band_rows(sorted({j for _, j in got}), seals[i].band_len, records[-1][1:3], framing.padding[i])
                for i, got in repaired.items()}
        healed = [f if h is None and f is not g else h for h, f, g in zip(healed, files, given)]       # a head fix alone heals a file too
        return pixels.to(out_dtype), framing.padding, container.RepairInfo(repaired, rows, salvage, healed, rounds, head=heads)

    def _repair(self, raw, seals, record, framing, streams, pixels, sym, P, dmll, K, words):
        """The rounds of decode_repair on the finest record (C, H, W, L) of B decoded files; `words` (_band_words) is updated in place
        with the words of the bands hashed again -> (pixels, {file: [(c, j)]} repaired, healed files, rounds run)."""
        C, H, W, L = record
        B, HW = len(seals), H * W
        n = n_bands(HW, L)
        band_words = words[B:].reshape(B, 3, n)                              # (a view: what _salvage reads afterwards)
        k = len(framing.offset) - 1
        buf, _, _ = streams.scale(k)
        o_h, l_h = streams.scale_host(k)                                     # stream (c n + j) B + b
        at = o_h.reshape(3, n, B).transpose(2, 0, 1).copy()                  # [b, c, j]: where the payload lies in `work`
        lens = l_h.reshape(3, n, B).transpose(2, 0, 1).astype(np.int64)
        work, tried, rebuilt, rounds = buf, set(), [], 0
        al16 = lambda v: (int(v) + 15) // 16 * 16                            # noqa: E731
        Kp = P.shape[-1]
        while True:
            _, failing, _ = container.failing_bands(seals, band_words, (H, W), framing.padding)
            # (file, c, g, erased bands, r0): rows r0 .. r0 + t - 1 of the group rebuild its t erased bands; one row ('L3CP'): t = 1, r0 = 0
            groups = []
            for i, bad in failing.items():
                if seals[i].parity is None:
                    continue
                bad, m, R = set(bad), seals[i].parity_groups, seals[i].parity_streams
                erasures = {}
                for j in sorted({j for _, j in bad}):
                    c = min(c for c, jj in bad if jj == j)
                    erasures.setdefault((c, j % m), []).append(j)
                for (c, g), js in sorted(erasures.items()):
                    if len(js) > R or any((c, o) in bad for o in range(g, n, m) if o not in js):
                        continue
                    # a window of len(js) consecutive rows, r0 = 0 first; a later one only where an earlier one left the positions failing
                    r0 = next((r for r in range(R - len(js) + 1) if (i, c, g, tuple(js), r) not in tried), None)
                    if r0 is not None:
                        groups.append((i, c, g, tuple(js), r0))
            if not groups:
                break
            rounds += 1
            tried.update(groups)
            groups.sort(key=lambda group: seals[group[0]].parity_streams > 1)    # (stable) the files of one row first: the XOR call's part
            jobs = [(i, c, j) for i, c, g, js, r0 in groups for j in js]
            # `work` grows by this round's region: the groups' parity rows (uploaded), then the output slots, all 16-byte aligned
            taken = [seals[i].rows(c, g)[r0:r0 + len(js)] for i, c, g, js, r0 in groups]
            row_at, o_at, pos = [], [], al16(work.numel())
            for rows in taken:
                row_at.append([])
                for p in rows:
                    row_at[-1].append(pos)
                    pos = al16(pos + len(p) + 4)
            src_end = pos
            for i, c, j in jobs:
                o_at.append(pos)
                pos = al16(pos + (lens[i, c, j] + 3) // 4 * 4 + 4)
            up = np.zeros(pos - work.numel(), dtype=np.uint8)
            for rows, ats in zip(taken, row_at):
                for p, a in zip(rows, ats):
                    up[a - work.numel():a - work.numel() + len(p)] = np.frombuffer(p, dtype=np.uint8)
            work = torch.cat([work, ops.upload_small(up)])
            # every rebuilt payload is ONE linear combination of its group's uploaded rows and present members; with one row every weight is 1
            offs, lns, coefs, first = [], [], [], [0]
            for (i, c, g, js, r0), rows, ats in zip(groups, taken, row_at):
                m = seals[i].parity_groups
                present = [o for o in range(g, n, m) if o not in js]
                if seals[i].parity_streams == 1:
                    solved = [([1], [1] * len(present))]
                else:
                    solved = container.rs_repair_coefficients([(j - g) // m for j in js], [(o - g) // m for o in present], r0)
                for row_weights, member_weights in solved:
                    offs += ats + [int(at[i, c, o]) for o in present]
                    lns += [len(p) for p in rows] + [int(lens[i, c, o]) for o in present]
                    coefs += list(row_weights) + list(member_weights)
                    first.append(len(offs))
            # ... the slots of the files of one row by ONE XOR call, the others by ONE call with the coefficients
            nx = sum(1 for i, _, _ in jobs if seals[i].parity_streams == 1)
            sx, gf_out, out_lens = first[nx], (o_at[nx] if nx < len(jobs) else pos), [int(lens[i, c, j]) for i, c, j in jobs]
            if nx:
                ops.u8_xor_spans(work[:src_end], offs[:sx], lns[:sx], first[:nx + 1], work[src_end:gf_out], [a - src_end for a in o_at[:nx]], out_lens[:nx])
            if nx < len(jobs):
                ops.u8_gf_spans(work[:src_end], offs[sx:], lns[sx:], coefs[sx:], [f - sx for f in first[nx:]], work[gf_out:],
                                [a - gf_out for a in o_at[nx:]], out_lens[nx:])
            for (i, c, j), a in zip(jobs, o_at):
                at[i, c, j] = a
            # the positions of the round, decoded again: their symbols zeroed, one entry each
            spots = sorted({(i, j) for i, _, j in jobs})
            flat = sym.view(B, 3, HW)
            for i, j in spots:
                flat[i, :, j * L:min((j + 1) * L, HW)] = 0
            e_i = np.asarray([i for i, _ in spots], dtype=np.int64)
            e_j = np.asarray([j for _, j in spots], dtype=np.int64)
            length = np.minimum(L, HW - e_j * L)
            chunks = max(1, min(self.RGB_BAND_CHUNKS, int(length.min()) // 64))
            hold = ops.decode_rgb_entries(P.view(-1, Kp), self._targets(dmll), sym.view(-1), work, at[e_i, :, e_j].T, lens[e_i, :, e_j].T,
                                          e_i * HW, np.full(len(spots), HW, dtype=np.int64), e_j * L, length, chunks, K,
                                          *self._rgb_schedule(len(spots), None))
            pixels = ops.sym_to_u8(sym)
            plane = (e_i[None, :] * 3 + np.arange(3, dtype=np.int64)[:, None])           # (3, S)
            again = ops.u8_crc32_spans(pixels.view(-1), (plane * HW + e_j[None, :] * L).reshape(-1), np.broadcast_to(length, plane.shape).reshape(-1))
            band_words[e_i[None, :], np.arange(3)[:, None], e_j[None, :]] = again.cpu().numpy().view(words.dtype).reshape(3, -1)
            del hold
            rebuilt += jobs
        _, failing, _ = container.failing_bands(seals, band_words, (H, W), framing.padding)
        repaired, healed = {}, [None] * B
        for i, c, j in sorted(set(rebuilt)):                                 # (a payload tried with a second window is listed twice)
            if all((cc, j) not in failing.get(i, ()) for cc in range(3)):
                repaired.setdefault(i, []).append((c, j))
        for i, got in repaired.items():
            got.sort()
            f = bytearray(raw[i])
            for c, j in got:
                a, nb, to = int(at[i, c, j]), int(lens[i, c, j]), int(framing.offset[k][i, c * n + j])
                f[to:to + nb] = work[a:a + nb].cpu().numpy().tobytes()
            healed[i] = bytes(f)
        return pixels, repaired, healed, rounds

    # ---- the walk over a file's scale records, coarse -> fine: what decode_batch (legacy and banded files) and the set decoder share -----
    # The headers are untrusted input: a wrong C / H / W would make the table and decoder kernels index P and the symbol buffers out of
    # bounds (the reference fails with a shape error here, bitcoding.py:248-266).  What needs only the framing is checked before the first
    # upload (_n_predicted, _check_coarsest), a predicted record against the network where its P is (_check_header, _get_P).

    def _n_predicted(self, n_records):
        """Predicted scales of a file of n_records scale records; ValueError when the model codes another number."""
        net = self.blueprint.net
        n_pred = n_records - 1
        if n_pred < net.scales or (n_pred != net.scales and not (net.config_ms.rgb_bicubic_baseline and net.scales == 1)):
            raise ValueError('invalid file: {} scale records, the model codes {}'.format(n_pred + 1, net.scales + 1))
        return n_pred

    def _check_coarsest(self, record, banded, max_nbytes):
        """The coarsest record (uniform prior): the model's bottleneck channels, and no stream longer than its symbols can be."""
        C, H, W = record[:3]
        n_sym = record[3] if banded else H * W                    # symbols per stream: a band of a banded file, else the plane
        if C != self.blueprint.net.config_ms.q.C or H < 1 or W < 1:
            raise ValueError('invalid file: coarsest scale header (C={}, H={}, W={})'.format(C, H, W))
        if max_nbytes > 2 * n_sym + 64:                           # > 16 bits per symbol: not a stream of this coder
            raise ValueError('invalid file: coarsest scale payload longer than {} symbols can be'.format(n_sym))

    def _check_header(self, scale, dmll, record, prev_hw):
        """A predicted record's (C, H, W) against what the network will predict from the scale above -> channels of P per pixel."""
        Cs = 3 if dmll.rgb_scale else self.blueprint.net.config_ms.q.C
        expect = (Cs, 2 * prev_hw[0], 2 * prev_hw[1])
        if tuple(record[:3]) != expect:
            raise ValueError('invalid file: scale {} header (C, H, W) = {} but the network predicts {}'.format(scale, tuple(record[:3]), expect))
        return (4 if dmll.rgb_scale else 3) * Cs * self.blueprint.net.config_ms.prob.K

    def _get_P(self, scale, n_pred, bn, F, shape):
        """net.get_P in the pixel-major form the table kernels read, checked against `shape` = (B, H, W, channels of P) -> P, F."""
        P, F = self.blueprint.net.get_P(scale, bn, F, n_scales_total=n_pred)
        P = ops.as_pixel_major(P)
        if tuple(P.shape) != tuple(shape):
            raise ValueError('invalid file: the network predicts {} at scale {}, the file says {}'.format(tuple(P.shape), scale, tuple(shape)))
        return P, F

    def _next_input(self, sym, dmll):
        """Decoded symbols of a scale -> what the decoder of the next finer scale is fed."""
        bn = ops.sym_to_bn(sym, dmll.bin_width, dmll.x_min)
        if self.blueprint.net.config_ms.rgb_bicubic_baseline:      # BicubicDownsamplingEnc: the decoder is fed value - mean (net.py:72-80)
            bn = bn - _rgb_mean_tensor(bn.device)
        return bn

    def _rgb_schedule(self, n_streams, side):
        """(lag, window mode, side stream or None) of an RGB chunk pipeline over n_streams streams per channel in lock step.  The two extra
        steps of lag 2 cost more than the overlap saves while the tables are small (they grow with the batch, a decode step does not):
        lag 2 from 16 streams on [measured at 128 images: 0.726 s instead of 0.825 s]; the constructor's decode_overlap forces.
        side: the stream the decoders of lag 2 run on (a lane's, the set decoder's); None = the next of the coder's side streams."""
        overlap = n_streams >= 16 if self.decode_overlap is None else bool(self.decode_overlap)
        mode = {'never': 0, 'auto': 1, 'always': 2}[self.rgb_window]
        return (2 if overlap else 1), mode, ((side or self._side_stream()) if overlap else None)

    def _decode_batch(self, files, out_dtype, side):
        """decode_batch on the current stream; `side`: see _rgb_schedule."""
        records, framing, banded = container.parse_batch(files)
        n_pred = self._n_predicted(len(records))
        self._check_coarsest(records[0], banded, int(framing.nbytes[0].max()))
        streams = upload._upload_streams(files, framing)
        return self._walk_records(records, framing, banded, streams, n_pred, len(records), side).to(out_dtype), framing.padding

    def _walk_records(self, records, framing, banded, streams, n_pred, n_decoded, side, finest=None, keep_finest=None):
        """The walk over the n_pred + 1 scale records of B files, coarse -> fine, on the current stream -> the finest scale's symbols
        (B, 3, H, W) int16.  records / framing / banded: what container.parse_batch or parse_prefix gave, streams: the files on the device
        (upload._upload_streams).  The first n_decoded records are decoded by the range decoder; every record past them takes the MEAN of
        the mixture the network predicts for it (ops.dmll_mean) in the shape the network predicts.  side: see _rgb_schedule.
        finest (decode_region): the walk ends BEFORE the finest record and returns finest(k, dmll, record, hw, bn, F) -- the record's index,
        loss and header, the (H, W) of the record before it, and the decoder's inputs for it.
        keep_finest (decode_salvage): a dict that receives the finest scale's P and loss; every other caller lets P go with the walk."""
        B = len(framing.padding)
        symbols = self._scale_symbols_of(banded)
        K = self.blueprint.net.config_ms.prob.K
        bn, F, P, hw, keep = None, None, None, None, []
        for k, (scale, dmll, uniform) in enumerate(self.iter_scale_dmll(n_pred)):
            Cs = 3 if dmll.rgb_scale else self.blueprint.net.config_ms.q.C
            record = records[k] if k < n_decoded else (Cs, 2 * hw[0], 2 * hw[1])
            H, W = record[1:3]
            if finest is not None and scale == 0:
                return finest(k, dmll, record, hw, bn, F)
            if not uniform:
                Kp = self._check_header(scale, dmll, record, hw)
                P, F = self._get_P(scale, n_pred, bn, F, (B, H, W, Kp))
            if k < n_decoded:
                sym, hold = symbols(streams, k, record, dmll, uniform, P, B, side)    # (the last record's streams are staged and uploaded HERE: behind the convolutions just enqueued)
                keep.append(hold)                                       # workspaces and tables live until the whole decode is enqueued
            else:
                sym = ops.dmll_mean(P, Cs, K, dmll.rgb_scale, dmll.x_min, dmll.x_max, dmll.L)
            hw = (H, W)
            if scale > 0:                                               # the finest scale's symbols ARE the pixel values (to_bn of the RGB scale: x 1 + 0)
                bn = self._next_input(sym, dmll)
        if keep_finest is not None:
            keep_finest['P'], keep_finest['dmll'] = P, dmll
        return sym

    def decode_preview(self, files, records=None, out_dtype=torch.uint8):
        """A picture from the COARSE records of B files -- whole files or prefixes of them (container.prefix_bytes), legacy or banded, of
        equally sized images -> ((B,3,H,W) out_dtype on the GPU, list of padding tuples).
        The first `records` scale records, coarsest first, are decoded as decode_batch decodes them; every finer scale takes the MEAN of the
        mixture the network predicts for it (ops.dmll_mean: sum_k pi_k mu'_k per pixel and channel, snapped to a symbol) in place of the
        range decoder's symbols and feeds it on the same way.  records == total is therefore the exact decode.
        A prefix cannot say how many records its file has: the total is this model's, n_predicted_scales() + 1 (RGB Shared: build Bitcoding
        with the file's auto_recurse); data holding more complete records than that raises ValueError.  records: 1 .. total, default every
        complete record present but the finest; more than the data holds raises ValueError.  Only the bytes of the records decoded cross
        PCIe; nothing synchronises with the host."""
        total = self.n_predicted_scales() + 1
        files = [container.split_seal(f, view=True)[0] for f in files]     # a preview is not lossless: nothing to verify
        recs, framing, banded, n = container.parse_prefix(files, total + 1)
        if n > total:
            raise ValueError('invalid file: more than {} scale records, the model codes {}'.format(total, total))
        if records is None:
            records = min(n, total - 1)
        records = int(records)
        if not 1 <= records <= total:
            raise ValueError('records must be in 1..{}, got {}'.format(total, records))
        if records > n:
            raise ValueError('{} record(s) asked for, the data holds {} complete one(s)'.format(records, n))
        self._check_coarsest(recs[0], banded, int(framing.nbytes[0].max()))
        # the upload path sends "the rest of the file" with its last record: the files cut behind record `records` (prefix_bytes)
        ends = framing.offset[records - 1][:, -1] + framing.nbytes[records - 1][:, -1] + 4
        framing = container.ParsedFraming(framing.padding, framing.scales[:records], framing.offset[:records], framing.nbytes[:records])
        streams = upload._upload_streams([f[:int(e)] for f, e in zip(files, ends)], framing)
        return self._walk_records(recs, framing, banded, streams, total - 1, records, None).to(out_dtype), framing.padding

    def decode_region(self, files, box, out_dtype=torch.uint8, verify=True):
        """The pixels of a BOX of B files of equally padded images, banded or legacy, without decoding the rest of their finest record
        -> ((B, 3, y1 - y0, x1 - x0) out_dtype on the GPU, region.RegionInfo).
        box: (y0, y1) or (y0, y1, x0, x1) in the coordinates of the UNPADDED image (frame row = top padding + y); the files must share one
        padding tuple; ValueError for an empty box or one that leaves the image.
        The coarser records (5 % of the bytes, a quarter of the convolution work) are decoded whole, as _walk_records decodes them.  Of the
        finest record only the bands that hold a pixel of the box rows are range-decoded (region.region_plan; the last of them stops at the
        box's last row), as ONE ops.decode_rgb_entries call over the B (j1 - j0) band entries, and the scale's convolutions run on the rows
        those symbols need plus the halo -- its decoder stage, at half resolution, on an apron of 192 rows more beyond every cut edge, which
        keeps the last bits of P (MultiscaleNetwork.get_P_rows, region.apron_rows): a full-frame P is never built, and in a frame of a few
        hundred rows the decoder stage is the whole frame.  Columns are cropped at the end.  A
        LEGACY file is one band: its one entry per image is pixels [0, y1 W) -- the rows below the box are saved, the rows above are not.
        Every file still crosses PCIe whole (the banded framing interleaves length fields and payloads).
        SEALED files: generation and model are checked as decode_batch checks them (verify=True), before anything is enqueued; the frame CRC
        covers the whole frame and is NOT checked -- the info says so.
        BAND-SEALED files (Bitcoding(seal='bands')) and verify=True: the pixels ARE verified.  The plan then decodes the last band whole
        (region_plan(cut=False): at most one band more), ops.sym_to_u8 turns the window into bytes and ONE ops.u8_crc32_spans hashes the
        3 B (j1 - j0) decoded bands where they lie in it; the words are compared with the files' band tables: SealError('pixels') with
        .bands and .rows, or info.verified = ('generation', 'model', 'bands') and info.pixel_crc_checked = True -- True exactly when every
        sealed file of the call was checked this way.  L3C only: the RGB baselines raise NotImplementedError."""
        net = self.blueprint.net
        if net.config_ms.rgb_bicubic_baseline:
            raise NotImplementedError('decode_region: the RGB baselines are not windowed (every scale of theirs is an RGB scale)')
        if not files:
            raise ValueError('decode_region: no files')
        split = [container.split_seal(f, view=True) for f in files]
        files, seals = [b for b, _ in split], [s for _, s in split]
        sealed = sum(s is not None for s in seals)
        check = bool(verify and sealed)
        if check:
            container.check_seals(seals, self.generation(), self.model_id)
        band_sealed = [s is not None and s.band_crcs is not None for s in seals]
        check_bands = check and any(band_sealed)
        records, framing, banded = container.parse_batch(files)
        n_pred = self._n_predicted(len(records))
        self._check_coarsest(records[0], banded, int(framing.nbytes[0].max()))
        Hf, Wf = records[-1][1:3]
        rows, cols = region.parse_box(box, region.shared_padding(framing.padding), (Hf, Wf))
        B = len(files)
        streams = upload._upload_streams(files, framing)
        K = net.config_ms.prob.K
        found = {}

        def finest(k, dmll, record, hw, bn, F):
            Kp = self._check_header(0, dmll, record, hw)
            C, H, W = record[:3]
            L = record[3] if banded else H * W
            n = n_bands(H * W, L)
            plan = region.region_plan(H, W, L, rows, region.halo_rows(net.config_ms), cut=not check_bands)
            c0, c1 = plan.conv_rows
            P = net.get_P_rows(0, bn, F, plan.conv_rows)
            if tuple(P.shape) != (B, c1 - c0, W, Kp):
                raise ValueError('invalid file: the network predicts {} on rows {}, the file says {}'.format(
                    tuple(P.shape), plan.conv_rows, (B, c1 - c0, W, Kp)))
            j0, j1 = plan.bands
            buf, _, _ = streams.scale(k)                                       # (the finest record's streams are staged and uploaded HERE)
            o_h, l_h = streams.scale_host_channel_image_band(k, C, B)         # (C, B n): an image's bands adjacent
            pick = (np.arange(B)[:, None] * n + np.arange(j0, j1)[None, :]).reshape(-1)
            o_h, l_h = o_h[:, pick], l_h[:, pick]
            pixbase, hw_e, pix0, length = region.entry_table(plan, B)
            # chunks per entry: a banded file's rule (RGB_BAND_CHUNKS, 64 symbols per chunk at least); the one long entry of a legacy file is
            # chunked as its whole-image decode chunks a channel
            chunks = (max(1, min(self.RGB_BAND_CHUNKS, int(length.min()) // 64)) if banded else
                      max(1, min(self.RGB_CHUNKS_FEW, int(length.min()) // 4096)))
            sym = torch.zeros(B, C, c1 - c0, W, dtype=torch.int16, device='cuda')
            ops.decode_rgb_entries(P.view(-1, Kp), self._targets(dmll), sym.view(-1), buf, o_h, l_h, pixbase, hw_e, pix0, length, chunks, K,
                                   *self._rgb_schedule(B * (j1 - j0), None))             # (everything is enqueued when it returns)
            found.update(plan=plan, n=n, streams_used=int(l_h.size), bytes_used=int(l_h.sum()))
            return sym

        sym = self._walk_records(records, framing, banded, streams, n_pred, len(records), None, finest)
        plan = found['plan']
        c0 = plan.conv_rows[0]
        if check_bands:
            self._check_region_bands(seals, sym, plan, records[-1], framing.padding)
        out = sym[:, :, rows[0] - c0:rows[1] - c0, cols[0]:cols[1]].to(out_dtype)
        left, _, top, _ = framing.padding[0]
        info = region.RegionInfo(box=(rows[0] - top, rows[1] - top, cols[0] - left, cols[1] - left), bands=plan.bands, n_bands=found['n'],
                                 sym_rows=plan.sym_rows, conv_rows=plan.conv_rows, valid_rows=plan.valid_rows,
                                 decoder_rows=region.decoder_rows(Hf, plan.conv_rows, region.apron_rows(net.config_ms)), frame_rows=Hf,
                                 streams_used=found['streams_used'], streams_total=int(framing.nbytes[-1].size),
                                 bytes_used=found['bytes_used'], bytes_total=int(framing.nbytes[-1].sum()), sealed=sealed,
                                 verified=(('generation', 'model', 'bands') if check_bands else ('generation', 'model')) if check else (),
                                 pixel_crc_checked=check_bands and sum(band_sealed) == sealed)
        return out, info

    @staticmethod
    def _check_region_bands(seals, sym, plan, record, padding):
        """decode_region on band-sealed files: the bands [j0, j1) the window holds WHOLE (region_plan(cut=False)) against the files' band
        tables.  Band (b, c, j) lies at byte ((3 b + c)(c1 - c0) - c0) W + j L of the window's pixels, min(L, HW - j L) bytes long."""
        _, H, W, L = record
        B = sym.shape[0]
        (j0, j1), (c0, c1) = plan.bands, plan.conv_rows
        pixels = ops.sym_to_u8(sym.contiguous())
        plane = np.arange(3 * B, dtype=np.int64)[:, None]
        j = np.arange(j0, j1, dtype=np.int64)[None, :]
        offsets = (plane * (c1 - c0) - c0) * W + j * L
        lengths = np.broadcast_to(np.minimum(L, H * W - j * L), offsets.shape)
        assert (offsets % 4 == 0).all() and (offsets >= 0).all(), (W, L, c0)      # W a multiple of the padding factor, L of 64
        words = ops.u8_crc32_spans(pixels.view(-1), offsets.reshape(-1), lengths.reshape(-1)).cpu().numpy().reshape(B, 3, j1 - j0)
        container.check_band_crcs(seals, words, (H, W), padding, j0)

    def _scale_symbols_of(self, banded):
        """The decoder of one scale record of a batch, by the files' format (the walk and the set decoder's coarsest scale)."""
        return self._scale_symbols_banded if banded else self._scale_symbols

    def _scale_symbols(self, streams, k, record, dmll, uniform, P, B, side):
        """-> (symbols (B, C, H, W) int16 of record k of legacy files, tensors to keep alive); uniform: the coarsest record, no P."""
        C, H, W = record
        if uniform:
            buf, offs, lens = streams.scale(k)
            return ops.ac_decode(self._uniform_row(dmll.L), buf, offs, lens, B * C, H * W, True, broadcast_row=True).reshape(B, C, H, W), None
        K = self.blueprint.net.config_ms.prob.K
        targets = self._targets(dmll)
        if dmll.rgb_scale:
            return self._decode_rgb_pipelined(P, targets, streams.scale(k), B, C, K, H, W, side), None
        return self._decode_z_scale(P, targets, streams.scale(k), B, C, K, H, W), None

    RGB_BAND_CHUNKS = 8      # chunks per band of the banded RGB decode (every band must hold 64 symbols per chunk: fewer for short bands)

    def _scale_symbols_banded(self, streams, k, record, dmll, uniform, P, B, side):
        """-> (symbols, tensors to keep alive) of record k of BANDED files (the same band length in every file): every band of every channel and image is a stream
        of its own --
            coarsest scale  the uniform row: one decoder launch over the full bands, one over the last bands
            bottleneck      one ragged table launch + one ragged decoder launch over all B C n bands (ops.decode_z_entries)
            RGB scale(s)    the chunk pipeline over all B n bands of each channel in lock step (l3c_decode_rgb_banded)."""
        C, H, W, L = record
        HW, n = H * W, n_bands(H * W, L)
        buf, _, _ = streams.scale(k)
        if uniform:
            o_h, l_h = streams.scale_host(k)
            o3, l3 = o_h.reshape(B * C, n), l_h.reshape(B * C, n).astype(np.int32)       # image-major: stream (b C + c) n + j
            row = self._uniform_row(dmll.L)
            sym = torch.empty(B * C, HW, dtype=torch.int16, device='cuda')
            if n > 1:
                full = ops.ac_decode(row, buf, ops.upload_small(o3[:, :n - 1].reshape(-1)), ops.upload_small(l3[:, :n - 1].reshape(-1)),
                                     B * C * (n - 1), L, True, broadcast_row=True)
                sym[:, :(n - 1) * L].copy_(full.view(B * C, (n - 1) * L))
            last = ops.ac_decode(row, buf, ops.upload_small(o3[:, n - 1].copy()), ops.upload_small(l3[:, n - 1].copy()), B * C,
                                 HW - (n - 1) * L, True, broadcast_row=True)
            sym[:, (n - 1) * L:].copy_(last)
            return sym.view(B, C, H, W), None
        K = self.blueprint.net.config_ms.prob.K
        o_h, l_h = streams.scale_host_channel_image_band(k, C, B)
        offs = ops.upload_small(o_h.reshape(-1))
        lens = ops.upload_small(l_h.reshape(-1).astype(np.int32))
        targets = self._targets(dmll)
        if dmll.rgb_scale:
            sym = torch.zeros(B, C, H, W, dtype=torch.int16, device='cuda')
            chunks = max(1, min(self.RGB_BAND_CHUNKS, (HW - (n - 1) * L) // 64))
            hold = ops.decode_rgb_banded(P, targets, sym, buf, offs, lens, L, chunks, K, *self._rgb_schedule(B * n, side))
        else:
            sym = torch.empty(B, C, H, W, dtype=torch.int16, device='cuda')
            # every band (b, j) is an entry: pixels [j L, j L + len_j) of image b
            hold = ops.decode_z_entries(P, targets, sym, buf, offs, lens, *container.band_entry_table(B, HW, L), B * HW, C, K)
        return sym, hold

    N_DECODE_LANES = SetDecoder.N_DECODE_LANES      # (read by the benchmark's report and by callers that size their buffers; the knobs of the set decode are SetDecoder's)

    @property
    def set_decoder(self):
        """The SetDecoder behind decode_many, created on first use: its knobs (N_DECODE_LANES, RAGGED_GROUP, RAGGED_GROUP_PIXELS, ENTRY_LIMIT)
        are set on it, and it owns the streams of the set decode."""
        if self._set_decoder is None:
            self._set_decoder = SetDecoder(self)
        return self._set_decoder

    def decode_many(self, batches, on_batch=None, lanes=None, chain_cus=0, out_dtype=torch.int64, ragged=None, banded=False, sealed=False):
        """batches: list of lists of `.l3c` byte strings; the files of ONE entry are equally sized (padded) images (a forward pass of
        `encode_many`), entries may differ in shape.  -> list, in the order given, of ((B_i,3,H_i,W_i) int64 on the GPU, padding tuples),
        or None per entry when `on_batch(index, pixels, padding)` consumes the results as they are enqueued (called under the stream
        that decodes the entry; then nothing is kept on the device).  The reference decodes a folder one file after the other
        (bitcoding.py:125-161 per file, multiscale_tester.py:353-381 over the folder).
        Small batches are LATENCY-bound (one 768x512 image: 93 ms whatever the machine does -- three 393 216-symbol chains, a wavefront
        each), so a set of differently sized images needs many images in flight (round 6):
          * LANES: entry i runs on lane i % lanes, a stream pair of its own -- up to the hardware queues' concurrency (8 lanes: 5.5x);
          * RAGGED RGB (ragged=True, the default for small batches): the lanes stop before the RGB scale -- two thirds of an image's
            latency --, and the RGB scales of up to RAGGED_GROUP images of DIFFERENT sizes run in lock step as ONE ragged batch
            (l3c_decode_rgb_ragged: one table launch and one decoder launch per pipeline step for all of them), on a stream pair of
            its own while the lanes work on the next group.
        Large batches (>= 64 images) run one after the other: [measured, profiles/r06_decode_lanes_probe.log] batches of 128 on two lanes
        62-146 MPix/s (erratic: the lanes' long decoder launches and convolutions alias on the hardware queues) against 142-144 for one
        lane; with the chains on 64 CUs of their own 125-147 -- the round-5 verdict's bar for keeping that overlap was 180.
        banded=True: BANDED files (Bitcoding(bands=K)) are accepted too -- an entry is then all banded (one band length per scale: what one
        `encode_many` pass writes) or all legacy.  Ragged groups are format-pure; in a banded group every BAND of every image is a ragged
        entry of its own (l3c_decode_rgb_entries, ops.decode_z_entries), so the group's chains are a band long, not an image.
        sealed=True: SEALED files (Bitcoding(seal=True)) are accepted too, alone or mixed with unsealed ones, which are decoded and not
        verified; without it a sealed file is refused.  Before anything is enqueued every seal's generation and model id are checked
        (container.SealError, reason 'generation' / 'model', .index = (entry, file)).  The frames are hashed on the device -- a ragged
        group's in ONE call over the group's pixel buffer (ops.u8_crc32_spans, a span per image), a lane's batch with ops.u8_crc32 on its
        lane -- and the words stay there: no group or lane waits for the host.  At the end of the call, when the caller's stream has waited
        for every lane and group, ONE D2H brings all words back and they are compared with the seals: SealError('pixels') with .index the
        first failing (entry, file) in call order and .failed all of them; nothing is returned.  (One lane, or batches of 64 images and
        more: decode_batch verifies each batch as it is decoded, and the error is raised there.)  set_decoder.frame_crcs then holds the
        words.  With `on_batch`, the pixels of a batch are handed over BEFORE the call has verified them -- the call still raises at its
        end: a consumer that must not act on unverified pixels waits for the call to return."""
        return self.set_decoder.decode_many(batches, on_batch, lanes, chain_cus, out_dtype, ragged, banded, sealed)

    @classmethod
    def ragged_rgb_chunk_plan(cls, hws, rgb_window):
        """(pix0, npix) of ops.ragged_rgb_plan for images of hws pixels as the legacy ragged group decode chunks them."""
        min_hw = min(hws)
        probe = cls.RGB_PROBE if (rgb_window == 'auto' and min_hw >= 16 * cls.RGB_PROBE) else 0
        n_regular = max(1, min(cls.RGB_CHUNKS, (min_hw - 2 * probe) // 4096))
        return ops.ragged_rgb_plan(hws, n_regular, probe)

    @classmethod
    def banded_rgb_chunks(cls, hws, lens, rgb_window, lag_legacy, lag):
        """Chunks per entry of a banded group's RGB scale (entries of `lens` symbols, lag `lag`): the workspace of l3c_decode_rgb_entries --
        its tables, above all -- must not exceed what the SAME images (hws pixels each) ask for as legacy files, chunked by
        ragged_rgb_chunk_plan at the lag the legacy group decode would use.  -> (chunks, fits); fits is False for the groups no chunk
        count can keep within that bound (ops.rgb_entries_chunks: a few tiny images, kilobytes of plan arrays)."""
        from .. import _lib
        pix0, npix = cls.ragged_rgb_chunk_plan(hws, rgb_window)
        budget = _lib.load().l3c_decode_rgb_ragged_workspace_bytes(len(hws), int(npix.sum(axis=1).max()), pix0.shape[0], lag_legacy)
        return ops.rgb_entries_chunks(lens, budget, lag)

    def _decode_z_scale(self, P, targets, streams, B, C, K, H, W):
        """A bottleneck scale: its C channels are independent given P, so ONE grouped table launch (fused, straight from P) and one
        grouped decoder launch handle them side by side; table validity is a device-side flag (no host synchronisation).
        streams: (buffer, offsets, lengths) with stream (c, b) at index c * B + b."""
        HW = H * W
        buf, offs, lens = streams
        sym = torch.empty(B, C, H, W, dtype=torch.int16, device='cuda')
        flag = torch.zeros(1, dtype=torch.int32, device='cuda')
        parts = []
        for k in range(0, C, 8):
            cs = list(range(k, min(C, k + 8)))
            tables = ops.dmll_cdf_table_parts(P, None, targets, C, K, False, [(c, 0, HW, flag, None) for c in cs])
            parts = [ops.ac_decode_part(t.reshape(B * HW, -1), buf, offs[c * B:(c + 1) * B], lens[c * B:(c + 1) * B], B, HW, flag,
                                        None, None, True, sym, C * HW, c * HW) for c, t in zip(cs, tables)]
            ops.ac_decode_chunks(parts)
        return sym

    RGB_PROBE = 1024         # symbols of the two probe chunks a channel starts with when window rows are in use (a multiple of 64)
    RGB_CHUNKS = 32          # chunks per RGB channel for batches of 16 images and more (round 5, with window rows: 32 instead of 16 --
    #                          the row form of a chunk follows the stream's misses two chunks earlier, and shorter chunks follow faster:
    #                          batch of 128 0.379 -> 0.365 s, the default-init checkpoint 0.585 -> 0.55 s)
    #                          64 / 96 chunks: another 1.3 / 1.7 % (0.3545 -> 0.350 / 0.3485 s) for two / three times the launches; not taken:
    #                          the host already needs 0.24 s of the 0.35 s to issue them [profiles/r05_decode_chunks_probe.log]
    RGB_CHUNKS_FEW = 32      # ... for a few images: the pipeline's fill (two extra chunk steps) weighs more than a step's launches

    def _decode_rgb_pipelined(self, P, targets, streams, B, C, K, H, W, side=None):
        """The RGB scale: channel c's means depend on the decoded values of the channels < c AT THE SAME PIXEL
        (logistic_mixture.py:262-272), so R, G and B are three serial chains of H*W symbols that only have to stay a
        chunk of pixels apart.  Pipeline step t: channel c handles chunk t - D c -- its table rows are built straight from P
        and the symbols decoded so far, then ONE grouped launch resumes the range decoders of all active channels side by side.
        Table validity is a device-side flag, nothing synchronises with the host.  Round 6: the whole schedule is ONE call into
        the library (l3c_decode_rgb, csrc/decode_pipeline.hip: a C loop over a workspace -- one grouped table launch and one decoder
        launch pair per step, a few microseconds of host time each); this method only chooses the chunks (the lag and the row form: _rgb_schedule).

        D = 1 (small batches): everything on the current stream, (chunks + 2) steps of table + decode.
        D = 2 (16 images or more): the channels stay TWO chunks apart, so the tables of step t + 1 need only the symbols of
        step t - 1 and are built on the current stream WHILE a side stream decodes step t: (chunks + 4) steps of
        max(table, decode).  [round 4, profiles/r04_decode_isolation_experiments.log: by the kernel trace the tables (0.28-0.32 s per batch
        of 128) and the decoders (0.29 s) overlap 80 %; confining the decoders to compute units of their own (CU-masked streams, balanced
        over the XCDs) or launching them on a high-priority stream did not shorten the whole decode and is not in the product]

        WINDOW ROWS (round 5; include/l3c_hip.h, l3c_ac_decode_part).  A full row has 257 entries although the symbol almost always
        lies near the mixture's mean: chunk j of a channel gets 65-entry rows around the mean for every image whose decoder missed at most
        1/64 of the symbols of chunk j - 2 (the newest chunk that is certain to be complete when the tables of chunk j are built, with either
        schedule), full rows otherwise and for chunks 0 and 1 (short PROBES on full rows) -- a quarter of the table arithmetic and bytes,
        the symbols the same (a decoder evaluates a missed pixel's full row itself).  rgb_window = 'always' / 'never' (tests) force a form."""
        assert C == 3
        HW = H * W
        buf, offs, lens = streams
        # one image: 393 216-symbol chains at ~140 ns per symbol; with c chunks the three channels take (c + 2) / c chain times
        n_chunks = max(1, min(self.RGB_CHUNKS if B >= 16 else self.RGB_CHUNKS_FEW, HW // 4096))
        step = -(-HW // n_chunks)
        step = -(-step // 64) * 64                       # chunk boundaries on the 64-symbol store blocks
        bounds = [(p0, min(step, HW - p0)) for p0 in range(0, HW, step)]
        if self.rgb_window == 'auto' and HW >= 16 * self.RGB_PROBE:
            P2 = 2 * self.RGB_PROBE
            bounds = [(0, self.RGB_PROBE), (self.RGB_PROBE, self.RGB_PROBE)] + [(p0, min(step, HW - p0)) for p0 in range(P2, HW, step)]
        sym = torch.zeros(B, C, H, W, dtype=torch.int16, device='cuda')
        ws, stats = ops.decode_rgb(P, targets, sym, buf, offs, lens, bounds, K, *self._rgb_schedule(B, side))
        self.last_rgb_window_stats = stats      # (development / tests: misses per channel, chunk + 2, image)
        return sym

    # ---- reference API: one image <-> one file -----------------------------------------------------------------------

    def encode(self, img, pout):
        """Encode image to disk at path `pout`.  img: int64 tensor CHW or 1CHW.  Returns the actual bpsp."""
        assert not os.path.isfile(pout)
        if img.dim() == 3:
            img = img.unsqueeze(0)
        assert img.dim() == 4 and img.shape[0] == 1 and img.shape[1] == 3, img.shape
        assert img.dtype == torch.int64, img.dtype

        if auto_crop.needs_crop(img):
            print('Need to encode individual crops!')
            return self._encode_crops(list(auto_crop.iter_crops(img)), pout)

        fac = self.padding_factor()
        _, _, H, W = img.shape
        if H % fac != 0 or W % fac != 0:
            print('*** INFO: image shape ({}X{}) not divisible by {}, will pad.'.format(H, W, fac))
            img, padding_tuple = pad.pad(img, fac=fac, mode=self.blueprint.get_padding_mode())
        else:
            padding_tuple = (0, 0, 0, 0)

        with self.times.run('[-] encode forwardpass'):
            out = self.blueprint.net(img.to('cuda', torch.float32), self.auto_recurse)
        loss_out = self.blueprint.get_loss(out) if self.compare_with_theory else None
        enc = self.encode_batch(img, out=out)
        data = enc.to_bytes([padding_tuple])[0]
        self._write_file(pout, data)

        num_subpixels = int(np.prod(img.shape))
        actual_bpsp = len(data) * 8 / num_subpixels
        if self.compare_with_theory:
            per_scale = [n * 8 / num_subpixels for n in enc.scale_payload_bytes()]
            tostr = lambda l: ' | '.join(map('{:.3f}'.format, l)) + ' => {:.3f}'.format(sum(l))   # noqa: E731
            theory = [float(b) for b in (loss_out.recursive_bpsps if self.auto_recurse else loss_out.nonrecursive_bpsps)]
            overhead = (sum(per_scale) / sum(theory) - 1) * 100
            print('Bitrates:\ntheory:  {}\nassumed: {} [{:.2f}%]\nactual:                                => {:.3f} '
                  '[{} bytes]'.format(tostr(theory), tostr(list(reversed(per_scale))), overhead, actual_bpsp, len(data)))
        return actual_bpsp

    def _encode_crops(self, crops, pout):
        """The auto-crops of a large image (reference :63-71 codes them one after the other): crops of equal padded shape
        share a batch, all batches share ONE grouped coder launch (encode_many); part i goes to `pout`.part<i> as before."""
        fac = self.padding_factor()
        padded, pads, groups = [], [], {}
        for i, crop in enumerate(crops):
            assert not os.path.isfile(pout + part_suffix_helper.make_part_suffix(i))
            _, _, H, W = crop.shape
            if H % fac != 0 or W % fac != 0:
                print('*** INFO: image shape ({}X{}) not divisible by {}, will pad.'.format(H, W, fac))
                crop, pt = pad.pad(crop, fac=fac, mode=self.blueprint.get_padding_mode())
            else:
                pt = (0, 0, 0, 0)
            padded.append(crop)
            pads.append(pt)
            groups.setdefault(tuple(crop.shape[-2:]), []).append(i)
        order = list(groups.values())
        with self.times.run('[-] encode forwardpass + coder, {} crops'.format(len(crops))):
            encs = self.encode_many([torch.cat([padded[i] for i in idxs]).to('cuda', torch.float32) for idxs in order])
        comb = auto_crop.CropLossCombinator()
        sizes = {}
        files = EncodedBatch.many_to_bytes(encs, [[pads[i] for i in idxs] for idxs in order])
        for idxs, datas in zip(order, files):
            for i, data in zip(idxs, datas):
                self._write_file(pout + part_suffix_helper.make_part_suffix(i), data)
                sizes[i] = len(data)
        for i, crop in enumerate(crops):     # as the reference: bpsp of a part over its PADDED sub-pixels, weighted by its area
            comb.add(sizes[i] * 8 / int(np.prod(padded[i].shape)), int(np.prod(crop.shape[-2:])))
        return comb.get_bpsp()

    def _write_file(self, path, data):
        if self.file_writer is not None:
            self.file_writer.submit(path, data)
        else:
            with open(path, 'wb') as fout:
                fout.write(data)

    def _read_file(self, path):
        if self.file_writer is not None:
            self.file_writer.wait(path)
        with open(path, 'rb') as fin:
            return fin.read()

    def _decode_parts(self, paths, verify=True):
        """Part files of one image: parts of equal (padded) shape are decoded as one batch."""
        datas = [self._read_file(p) for p in paths]
        groups = {}
        for i, d in enumerate(datas):
            groups.setdefault((is_banded(d), container.padded_shape(container.split_seal(d)[0])), []).append(i)
        parts = [None] * len(datas)
        for idxs in groups.values():
            out, padding = self.decode_batch([datas[i] for i in idxs], verify=verify)
            for k, i in enumerate(idxs):
                o = out[k:k + 1]
                parts[i] = pad.undo_pad(o, *padding[k]) if any(padding[k]) else o
        return parts

    def decode(self, pin, _recurse_part=True, verify=True, region=None):
        """-> decoded image, 1CHW long (on the GPU).  A sealed file (and every sealed part file) is verified as decode_batch verifies it;
        verify=False strips the seal and checks nothing.
        region: a box (y0, y1) or (y0, y1, x0, x1) of the image -> (its pixels, 1CHW long, region.RegionInfo): decode_region on the one
        file; an auto-cropped image (.partN files) raises NotImplementedError."""
        if region is not None:
            if part_suffix_helper.contains_part_suffix(pin):
                raise NotImplementedError('region decode of an auto-cropped image: its .partN files are images of their own, a box would have '
                                          'to be mapped onto every part ({})'.format(pin))
            return self.decode_region([self._read_file(pin)], region, out_dtype=torch.int64, verify=verify)
        if self.file_writer is not None:
            self.file_writer.wait(pin)                 # (a part suffix is resolved below: every part is waited for when read)
        if _recurse_part and part_suffix_helper.contains_part_suffix(pin):
            parts = self._decode_parts(list(part_suffix_helper.iter_part_suffixes(pin)), verify)
            print('Stitching {} parts...'.format(len(parts)))
            return auto_crop.stitch(parts)
        data = self._read_file(pin)
        out, padding = self.decode_batch([data], verify=verify)
        if any(padding[0]):
            out = pad.undo_pad(out, *padding[0])
        return out

    def preview(self, pin, records=None, max_bytes=None):
        """-> a preview of the image in file `pin`, 1CHW uint8 (on the GPU), from its first `records` scale records (decode_preview; default:
        all but the finest of those that lie within the first `max_bytes` bytes -- no more of the file is read)."""
        if part_suffix_helper.contains_part_suffix(pin):
            raise NotImplementedError('preview of an auto-cropped image: its .partN files are images of their own, a preview would have to '
                                      'decode and stitch every part ({})'.format(pin))
        if self.file_writer is not None:
            self.file_writer.wait(pin)
        with open(pin, 'rb') as fin:
            data = fin.read() if max_bytes is None else fin.read(max(0, int(max_bytes)))
        out, padding = self.decode_preview([data], records)
        if any(padding[0]):
            out = pad.undo_pad(out, *padding[0])
        return out


_RGB_MEAN_T = {}


def _rgb_mean_tensor(device):
    """(1,3,1,1) fp32 tensor of (0.4488, 0.4371, 0.4040) * 255 -- the same fp32 values the encoder side subtracts (ops.rgb_mean)."""
    key = str(device)
    if key not in _RGB_MEAN_T:
        _RGB_MEAN_T[key] = torch.tensor([float(v) for v in ops.rgb_mean()], dtype=torch.float32, device=device).reshape(1, 3, 1, 1)
    return _RGB_MEAN_T[key]


class AsyncFileWriter(object):
    """Writes finished `.l3c` byte strings on worker threads (file output is not part of the hot path: reference bitcoding.py:
    326-375 writes from the coding loop).  `wait(path)` blocks until a pending write of `path` is on disk; `close()` drains."""

    def __init__(self, n_threads=2):
        import concurrent.futures
        self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=n_threads, thread_name_prefix='l3c-write')
        self._pending = {}

    @staticmethod
    def _write(path, data):
        with open(path, 'wb') as f:
            f.write(data)

    def submit(self, path, data):
        self.wait(path)
        self._pending[path] = self._pool.submit(self._write, path, data)

    def wait(self, path=None):
        for p in ([path] if path is not None else list(self._pending)):
            fut = self._pending.pop(p, None)
            if fut is not None:
                fut.result()

    def pending(self):
        return len(self._pending)

    def close(self):
        self.wait()
        self._pool.shutdown()
