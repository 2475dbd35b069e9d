"""The codec as one library call per direction (include/l3c_hip.h: l3c_encode_batch / l3c_decode_plan + l3c_decode_batch).

`NativeCodec(blueprint)` stands next to `Bitcoding` as `NativeNet` stands next to `MultiscaleNetwork`: the library runs the schedule of
bitcoding/bitcoding.py -- the same entry points in the same order -- so the files equal `Bitcoding(bp).encode_batch(img).to_bytes(paddings)`
byte for byte and either side decodes the other's.  L3C family, equally sized padded images; the legacy `.l3c` format, or with
`NativeCodec(blueprint, bands=K)` the banded one (l3c_encode_batch_banded / l3c_decode_plan_banded + l3c_decode_batch_banded: the files of
`Bitcoding(bp, bands=K)`); `decode_batch` reads either.  torch owns the memory and the streams, nothing else.  It has no other knobs, and
no product path (Bitcoding, l3c.py, test.py, bench.py) reads it.

`decode_region` returns a BOX of the pictures without decoding the rest of their finest record, as `Bitcoding.decode_region` does
(l3c_decode_region_plan + l3c_decode_region: the region planner, the windowed network step and the finest step in the library).

`encode_images` / `decode_images` take pictures as they come -- a list of host images, each of its own size, planar or interleaved RGB /
RGBX / BGR(X) -- and leave padding and cropping to the library (l3c_encode_images / l3c_decode_images: l3c_u8_gather / l3c_u8_scatter driven
by a table of l3c_u8_image entries, one call per group of images that pad to one shape).

`NativeCodec(blueprint, seal=True)` writes SEALED files (include/l3c_hip.h "sealed files"; the files of `Bitcoding(bp, seal=True)` byte for
byte): l3c_encode_batch(_banded), l3c_u8_crc32 on the input frames, l3c_seal_append -- one stream of work, no host round trip.  The decoders
verify every sealed file they are given: generation and model id before anything is enqueued, l3c_u8_crc32 of the decoded frames after.

`NativeCodec(blueprint, bands=K, seal='bands', parity=G[, parity_streams=R][, parity_head=True])` writes PARITY-SEALED files (seal version 3,
include/l3c_hip.h "parity bands"; the files of `Bitcoding` with the same arguments byte for byte) in ONE call, l3c_encode_batch_banded_parity:
the band CRCs, the parity rows and the whole tail (l3c_seal_append_parity) are enqueued behind the coder on the device.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from ._lib import CodecModel, DecodeBatchDesc, DecodeImagesDesc, DecodeRegionDesc, EncodeBatchDesc, EncodeImagesDesc, ptr, stream
from .bitcoding import container, region, upload
from .bitcoding.bitcoding import Bitcoding, _staging
from .helpers import dataset_codec
from .modules import schema
from .native_net import NativeNet, _bytes, _size

PLAN_MAGIC = int.from_bytes(b'L3C_PLAN', 'little')
_PLAN_HEADER_WORDS = 26          # csrc/codec_plan.h: Header up to its records
_PLAN_MAX_RECORDS = _lib.NET_MAX_SCALES + 1
PLAN_BANDED_MAGIC = int.from_bytes(b'L3CBPLAN', 'little')
_PLAN_BANDED_HEADER_WORDS = 24 + _PLAN_MAX_RECORDS     # csrc/codec_plan_banded.h: BandedHeader up to its records
REGION_MAGIC = int.from_bytes(b'L3CRPLAN', 'little')
_REGION_HEADER_WORDS = 48        # csrc/codec_plan_region.h: RegionHeader
_RING = upload._H2DRing(3)


# l3c_u8_image (include/l3c_hip.h) as a numpy record: a table is an array of these
IMAGE_DTYPE = np.dtype({'names': ['offset', 'row_stride', 'chan_stride', 'pix_stride', 'h', 'w', 'top', 'left'],
                        'formats': ['<i8', '<i8', '<i8', '<i4', '<i4', '<i4', '<i4', '<i4'], 'offsets': [0, 8, 16, 24, 28, 32, 36, 40], 'itemsize': 48})
LAYOUTS = ('chw', 'hwc', 'hwcx', 'bgr')


def image_shape(layout, h, w, channels=3):
    """Array shape of a contiguous h x w image: 'chw' (3,h,w); 'hwc' (h,w,3); 'hwcx' (h,w,4); 'bgr' (h,w,channels), channels 3 or 4 (BGRX)."""
    if layout not in LAYOUTS:
        raise ValueError('layout must be one of {}, got {!r}'.format(LAYOUTS, layout))
    return (3, h, w) if layout == 'chw' else (h, w, {'hwc': 3, 'hwcx': 4, 'bgr': channels}[layout])


def image_entry(layout, shape, offset, top=0, left=0):
    """The l3c_u8_image fields of a CONTIGUOUS image of array shape `shape` lying `offset` bytes into its buffer -> (offset, row_stride,
    chan_stride, pix_stride, h, w, top, left); a row pitch or a bottom-up image is the caller's to put into row_stride."""
    if layout == 'chw':
        if len(shape) != 3 or shape[0] != 3:
            raise ValueError("layout 'chw' expects (3, h, w), got {}".format(tuple(shape)))
        _, h, w = shape
        return (offset, w, h * w, 1, h, w, top, left)
    if len(shape) != 3 or tuple(shape) != image_shape(layout, shape[0], shape[1], shape[2] if layout == 'bgr' and shape[2] in (3, 4) else 3):
        raise ValueError('layout {!r} expects {}, got {}'.format(layout, image_shape(layout, 'h', 'w'), tuple(shape)))
    h, w, px = shape
    return (offset + 2, px * w, -1, px, h, w, top, left) if layout == 'bgr' else (offset, px * w, 1, px, h, w, top, left)


def _host_u8(i, img):
    a = img.numpy() if isinstance(img, torch.Tensor) and not img.is_cuda else img
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
        raise ValueError('encode_images: image {} must be a host uint8 tensor or numpy array'.format(i))
    return np.ascontiguousarray(a)


def parse_plan(blob):
    """The blob l3c_decode_plan writes (layout: csrc/codec_plan.h) as a dict: the header's numbers, `records` = [(C, H, W, first, n_streams,
    max_nbytes)], and the arrays src_offset / dst_offset / nbytes (per stream) and chunks = [(pix0, npix)]."""
    raw = np.frombuffer(bytes(blob), dtype=np.uint8)
    w = raw[:8 * (_PLAN_HEADER_WORDS + 6 * _PLAN_MAX_RECORDS)].view(np.int64)
    names = ['magic', 'bytes', 'B', 'n_records', 'H', 'W', 'n_streams', 'files_bytes', 'dst_bytes', 'n_chunks', 'max_chunk_npix', 'lag']
    plan = {n: int(w[i]) for i, n in enumerate(names)}
    plan['cfg'] = [int(v) for v in w[12:21]]
    src_off, dst_off, nb_off, p0_off, np_off = (int(v) for v in w[21:26])
    plan['records'] = [tuple(int(v) for v in w[26 + 6 * k:32 + 6 * k]) for k in range(plan['n_records'])]
    S, n = plan['n_streams'], plan['n_chunks']
    plan['src_offset'] = raw[src_off:src_off + 8 * S].view(np.int64).copy()
    plan['dst_offset'] = raw[dst_off:dst_off + 8 * S].view(np.int64).copy()
    plan['nbytes'] = raw[nb_off:nb_off + 4 * S].view(np.uint32).copy()
    pix0, npix = raw[p0_off:p0_off + 8 * n].view(np.int64), raw[np_off:np_off + 8 * n].view(np.int64)
    plan['chunks'] = [(int(a), int(b)) for a, b in zip(pix0, npix)]
    return plan


def decode_plan(cfg, files):
    """l3c_decode_plan on host byte strings -> (blob bytes, H, W, paddings).  ValueError with the library's message for an invalid file,
    L3CError for a file outside the native codec's scope (banded)."""
    lib = _lib.load()
    B = len(files)
    n_plan = lib.l3c_decode_plan_bytes(ctypes.byref(cfg), B)
    _lib.check(min(n_plan, 0))
    sizes = np.asarray([len(f) for f in files], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    data = np.frombuffer(b''.join(bytes(f) for f in files) + b'\0' * 8, dtype=np.uint8)
    blob = np.zeros(n_plan // 8, dtype=np.int64)
    H, W, pads = ctypes.c_int(), ctypes.c_int(), np.zeros((B, 4), dtype=np.uint16)
    _check_plan(lib.l3c_decode_plan(ctypes.byref(cfg), data.ctypes.data, offs.ctypes.data_as(ctypes.POINTER(_lib.c_i64)), B, blob.ctypes.data,
                                    n_plan, ctypes.byref(H), ctypes.byref(W), pads.ctypes.data))
    return blob.tobytes(), H.value, W.value, [tuple(int(v) for v in p) for p in pads]


def parse_plan_banded(blob):
    """The blob l3c_decode_plan_banded writes (layout: csrc/codec_plan_banded.h) as a dict: the header's numbers, `records` = [(C, H, W, L, n,
    first, n_streams, max_nbytes)], the arrays src_offset / dst_offset / nbytes (per band stream) and `entries` = per record None or the
    (pixbase, hw, pix0, npix, table_off) int64 arrays of its B n bands (the bottleneck records)."""
    raw = np.frombuffer(bytes(blob), dtype=np.uint8)
    w = raw[:8 * (_PLAN_BANDED_HEADER_WORDS + 8 * _PLAN_MAX_RECORDS)].view(np.int64)
    names = ['magic', 'bytes', 'B', 'n_records', 'H', 'W', 'n_streams', 'files_bytes', 'dst_bytes', 'rgb_band_len', 'rgb_chunks', 'lag']
    plan = {n: int(w[i]) for i, n in enumerate(names)}
    plan['cfg'] = [int(v) for v in w[12:21]]
    src_off, dst_off, nb_off = (int(v) for v in w[21:24])
    ent_off = [int(v) for v in w[24:24 + _PLAN_MAX_RECORDS]]
    h = _PLAN_BANDED_HEADER_WORDS
    plan['records'] = [tuple(int(v) for v in w[h + 8 * k:h + 8 * k + 8]) for k in range(plan['n_records'])]
    S = plan['n_streams']
    plan['src_offset'] = raw[src_off:src_off + 8 * S].view(np.int64).copy()
    plan['dst_offset'] = raw[dst_off:dst_off + 8 * S].view(np.int64).copy()
    plan['nbytes'] = raw[nb_off:nb_off + 4 * S].view(np.uint32).copy()
    plan['entries'] = []
    for k, r in enumerate(plan['records']):
        E = plan['B'] * r[4]
        plan['entries'].append(tuple(raw[ent_off[k] + 8 * E * i:ent_off[k] + 8 * E * (i + 1)].view(np.int64).copy() for i in range(5))
                               if ent_off[k] else None)
    return plan


def parse_region_plan(blob):
    """The blob l3c_decode_region_plan writes (layout: csrc/codec_plan_region.h) as a dict: the header's numbers, the pairs bands / sym_rows /
    conv_rows / valid_rows / decoder_rows, the arrays src_offset / dst_offset / nbytes of the 3 S picked streams, `entries` = the (pixbase, hw,
    pix0, length) int64 arrays of the S entries, and `crop` = the B l3c_u8_image records."""
    raw = np.frombuffer(bytes(blob), dtype=np.uint8)
    w = raw[:8 * _REGION_HEADER_WORDS].view(np.int64)
    names = ['magic', 'bytes', 'plan_magic', 'B', 'H', 'W', 'L', 'n']
    plan = {n: int(w[i]) for i, n in enumerate(names)}
    plan['padding'], plan['box'] = tuple(int(v) for v in w[8:12]), tuple(int(v) for v in w[12:16])
    for i, n in enumerate(['bands', 'sym_rows', 'conv_rows', 'valid_rows', 'decoder_rows']):
        plan[n] = (int(w[16 + 2 * i]), int(w[17 + 2 * i]))
    for i, n in enumerate(['S', 'n_chunks', 'lag', 'max_nbytes', 'dst_bytes', 'streams_total', 'bytes_used', 'bytes_total']):
        plan[n] = int(w[26 + i])
    plan['cfg'] = [int(v) for v in w[34:43]]
    src_off, dst_off, nb_off, ent_off, crop_off = (int(v) for v in w[43:48])
    S, B = plan['S'], plan['B']
    plan['src_offset'] = raw[src_off:src_off + 24 * S].view(np.int64).copy()
    plan['dst_offset'] = raw[dst_off:dst_off + 24 * S].view(np.int64).copy()
    plan['nbytes'] = raw[nb_off:nb_off + 12 * S].view(np.uint32).copy()
    plan['entries'] = tuple(raw[ent_off + 8 * S * i:ent_off + 8 * S * (i + 1)].view(np.int64).copy() for i in range(4))
    plan['crop'] = raw[crop_off:crop_off + IMAGE_DTYPE.itemsize * B].view(IMAGE_DTYPE).copy()
    return plan


def _plan_banded_bytes(cfg_ref, files):
    """l3c_decode_plan_banded_bytes of host byte strings: the size function reads the framing of file 0 and the signature of every file."""
    head = np.frombuffer(bytes(files[0]) + b''.join(bytes(f[:4]) for f in files[1:]) + b'\0' * 8, dtype=np.uint8)
    offs = np.concatenate([[0, len(files[0])], len(files[0]) + np.cumsum([len(f[:4]) for f in files[1:]])]).astype(np.int64)
    return _lib.load().l3c_decode_plan_banded_bytes(cfg_ref, head.ctypes.data, offs.ctypes.data_as(ctypes.POINTER(_lib.c_i64)), len(files))


def decode_plan_banded(cfg, files):
    """l3c_decode_plan_banded on host byte strings -> (blob bytes, H, W, paddings).  ValueError with the library's message for an invalid
    file, L3CError for what is outside its scope (a legacy file, a mix of both formats, more than 65535 band streams per channel)."""
    lib = _lib.load()
    B = len(files)
    n_plan = _plan_banded_bytes(ctypes.byref(cfg), files)
    _check_plan(min(n_plan, 0))
    sizes = np.asarray([len(f) for f in files], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    data = np.frombuffer(b''.join(bytes(f) for f in files) + b'\0' * 8, dtype=np.uint8)
    blob = np.zeros(n_plan // 8, dtype=np.int64)
    H, W, pads = ctypes.c_int(), ctypes.c_int(), np.zeros((B, 4), dtype=np.uint16)
    _check_plan(lib.l3c_decode_plan_banded(ctypes.byref(cfg), data.ctypes.data, offs.ctypes.data_as(ctypes.POINTER(_lib.c_i64)), B,
                                           blob.ctypes.data, n_plan, ctypes.byref(H), ctypes.byref(W), pads.ctypes.data))
    return blob.tobytes(), H.value, W.value, [tuple(int(v) for v in p) for p in pads]


ROUND_MAGIC = int.from_bytes(b'L3CROUND', 'little')
_ROUND_NAMES = ['magic', 'bytes', 'B', 'n', 'HW', 'L', 'n_groups', 'n_src', 'S', 'n_chunks', 'lag', 'dst_bytes']
REPAIR_GROUP_DTYPE = np.dtype([('file', '<i4'), ('c', '<i4'), ('g', '<i4'), ('t', '<i4'), ('r0', '<i4'), ('bands', '<i4', (4,))])


def parse_round(blob):
    """The blob l3c_repair_round_plan writes (layout: csrc/repair_plan.h) as a dict: the header's numbers, `files` (B, 2) = m | R, `groups`
    (REPAIR_GROUP_DTYPE), the l3c_band_rebuild tables `rebuild` (ops.REBUILD_GROUP_DTYPE), `src` (ops.SPAN_DTYPE) and `coef` (n_src, 4),
    `pos` (S, 2) = file | band, `entries` (4, S), `in_offsets` / `in_nbytes` (3, S) and `crc` (3, S) spans."""
    raw = np.frombuffer(bytes(blob), dtype=np.uint8)
    w = raw[:8 * 31].view(np.int64)
    r = {name: int(w[i]) for i, name in enumerate(_ROUND_NAMES)}
    r['cfg'] = [int(v) for v in w[12:21]]
    files, groups, rebuild, src, coef, pos, entries, in_off, in_nb, crc = (int(v) for v in w[21:31])
    B, G, N, S = r['B'], r['n_groups'], r['n_src'], r['S']
    cut = lambda at, n, dtype: raw[at:at + n * np.dtype(dtype).itemsize].view(dtype).copy()       # noqa: E731
    r['files'] = cut(files, 2 * B, '<i4').reshape(B, 2)
    r['groups'] = cut(groups, G, REPAIR_GROUP_DTYPE)
    r['rebuild'] = cut(rebuild, G, ops.REBUILD_GROUP_DTYPE)
    r['src'] = cut(src, N, ops.SPAN_DTYPE)
    r['coef'] = cut(coef, 4 * N, np.uint8).reshape(N, 4)
    r['pos'] = cut(pos, 2 * S, '<i4').reshape(S, 2)
    r['entries'] = cut(entries, 4 * S, '<i8').reshape(4, S)
    r['in_offsets'] = cut(in_off, 3 * S, '<i8').reshape(3, S)
    r['in_nbytes'] = cut(in_nb, 3 * S, '<u4').reshape(3, S)
    r['crc'] = cut(crc, 3 * S, ops.SPAN_DTYPE).reshape(3, S)
    return r


def _check_plan(rc):
    if rc == 0:
        return
    msg = _lib.load().l3c_last_error().decode()
    if rc == -1:
        raise ValueError(msg)
    raise _lib.L3CError('libl3c_hip: {} (status {})'.format(msg, rc))


def _check_region(rc):
    """The region entries' refusals as Bitcoding.decode_region raises them: ValueError for a bad argument, NotImplementedError for what is
    outside the scope."""
    if rc == 0:
        return
    msg = _lib.load().l3c_last_error().decode()
    if rc == -1:
        raise ValueError(msg)
    if rc == -3:
        raise NotImplementedError(msg)
    raise _lib.L3CError('libl3c_hip: {} (status {})'.format(msg, rc))


class NativeCodec(object):
    def __init__(self, blueprint, bands=0, seal=False, parity=0, parity_streams=1, parity_head=False):
        """bands: 0 = encode writes the legacy format; K in 1..1024 = banded files, as Bitcoding(bp, bands=K).  decode_batch reads either.
        seal: True = every file the encoders return ends with a seal, as Bitcoding(bp, seal=True); the decoders verify sealed files whatever
        this says.  seal='bands' (with bands=K; ValueError with bands=0): BAND-SEALED files, as Bitcoding(bp, bands=K, seal='bands'), byte for
        byte: l3c_encode_batch_banded, ONE l3c_u8_crc32_bands on the input frames, l3c_seal_append_bands -- no host round trip.
        parity=G, parity_streams=R, parity_head (the rules and ValueErrors of Bitcoding's constructor; parity needs seal='bands'):
        PARITY-SEALED files, seal version 3, as Bitcoding(bp, bands=K, seal='bands', parity=G, parity_streams=R, parity_head=...), byte for
        byte, in ONE library call, l3c_encode_batch_banded_parity: the band CRCs, the parity rows, with parity_head the head rows and
        payload CRCs, and the whole tail (l3c_seal_append_parity) are enqueued behind the coder on the device.  The decoders read these
        files as the band-sealed files they contain; Bitcoding.decode_repair repairs them."""
        if seal not in (False, True, 'bands'):
            raise ValueError("seal must be False, True or 'bands', got {!r}".format(seal))
        if seal == 'bands' and not bands:
            raise ValueError("seal='bands' needs banded files: a band seal holds a CRC per band of the finest record (bands=K, K >= 1)")
        if bands and not 1 <= int(bands) <= container.MAX_BANDS:
            raise ValueError('bands must be 0 (legacy format) or in 1..{}, got {}'.format(container.MAX_BANDS, bands))
        if isinstance(parity, bool) or not isinstance(parity, int) or parity < 0:
            raise ValueError('parity must be 0 or a group size >= 1, got {!r}'.format(parity))
        if parity and seal != 'bands':
            raise ValueError("parity needs seal='bands': the band seal is what turns damage into erasures of known position")
        if isinstance(parity_streams, bool) or not isinstance(parity_streams, int) or not 1 <= parity_streams <= container.MAX_PARITY_STREAMS:
            raise ValueError('parity_streams must be in 1..{}, got {!r}'.format(container.MAX_PARITY_STREAMS, parity_streams))
        if parity_streams > 1 and not parity:
            raise ValueError('parity_streams > 1 needs parity=G: the rows are computed over the parity groups')
        if parity_streams > 1:
            container.check_parity_streams(parity_streams, parity, int(bands))
        if not isinstance(parity_head, bool):
            raise ValueError('parity_head must be True or False, got {!r}'.format(parity_head))
        if parity_head and not parity:
            raise ValueError('parity_head needs parity=G: the head rows are computed over groups of min(G, n) bands with its parity_streams')
        self.parity, self.parity_streams, self.parity_head = parity, parity_streams, parity_head
        self.bands = int(bands)
        self.seal = bool(seal)
        self.seal_bands = seal == 'bands'
        self._network, self._model_id = blueprint.net, None
        self._losses = blueprint.losses
        _lib.require_gpu()
        self.net = NativeNet(blueprint.net)
        self.cfg = self.net.cfg
        self._cfg_ref = ctypes.byref(self.cfg)
        bc = Bitcoding(blueprint)
        losses = blueprint.losses
        dz = losses.loss_dmol_n
        # the very tensors Bitcoding codes with: their host rounding is part of the bitstream contract
        self.targets_rgb = bc._targets(losses.loss_dmol_rgb)
        self.targets_z = bc._targets(dz)
        self.uniform_row = bc._uniform_row(dz.L)
        self.model = CodecModel(ctypes.pointer(self.cfg), ptr(self.net.packed), self.net.packed_bytes, ptr(self.targets_rgb, torch.float32),
                                ptr(self.targets_z, torch.float32), ptr(self.uniform_row, torch.int16), float(dz.x_min), float(dz.bin_width))
        self._side = None

    # ---- sizes ---------------------------------------------------------------------------------------------------------------

    def file_stride(self, H, W):
        """The slot of one file: the library's stride, and with seal=True the 32 bytes more that l3c_seal_append asks for; with
        seal='bands' l3c_seal_bands_bytes(n) rounded up to 32; with parity=G l3c_encode_banded_parity_file_stride."""
        if self.parity:
            return _size(_lib.load().l3c_encode_banded_parity_file_stride(self._cfg_ref, H, W, self.bands, ctypes.byref(self._parity_opts())))
        if self.seal_bands:
            n = container.n_bands(H * W, container.band_len(H * W, self.bands))
            return (_size(_lib.load().l3c_encode_banded_file_stride(self._cfg_ref, H, W, self.bands)) +
                    (_size(_lib.load().l3c_seal_bands_bytes(n)) + 31) // 32 * 32)
        if self.bands:
            return _size(_lib.load().l3c_encode_banded_file_stride(self._cfg_ref, H, W, self.bands)) + 32 * self.seal
        return _size(_lib.load().l3c_encode_file_stride(self._cfg_ref, H, W)) + 32 * self.seal

    def model_id(self):
        """The checkpoint's id in a seal (modules/schema.model_id), computed on first use."""
        if self._model_id is None:
            self._model_id = schema.model_id(self._network.state_dict(), self._network.config_ms)
        return self._model_id

    @staticmethod
    def generation():
        return _lib.load().l3c_bitstream_generation()

    def _parity_opts(self):
        """l3c_parity_opts of this codec (the model id is computed on first use)."""
        return _lib.ParityOpts(self.parity, self.parity_streams, int(self.parity_head), 0, self.model_id())

    def encode_workspace_bytes(self, B, H, W):
        if self.parity:
            return _size(_lib.load().l3c_encode_batch_banded_parity_workspace_bytes(self._cfg_ref, B, H, W, self.bands,
                                                                                    ctypes.byref(self._parity_opts())))
        if self.bands:
            return _size(_lib.load().l3c_encode_batch_banded_workspace_bytes(self._cfg_ref, B, H, W, self.bands))
        return _size(_lib.load().l3c_encode_batch_workspace_bytes(self._cfg_ref, B, H, W))

    def decode_workspace_bytes(self, blob):
        """Workspace of the decode of a plan blob, legacy or banded (its magic word says which)."""
        buf = np.frombuffer(bytes(blob), dtype=np.int64)
        fn = 'l3c_decode_batch_banded_workspace_bytes' if int(buf[0]) == PLAN_BANDED_MAGIC else 'l3c_decode_batch_workspace_bytes'
        return _size(getattr(_lib.load(), fn)(self._cfg_ref, buf.ctypes.data))

    # ---- encode --------------------------------------------------------------------------------------------------------------

    def encode_device(self, imgs, paddings=None, workspace=None):
        """Enqueue the encode on the current stream -> (files uint8 (B, file_stride), file_bytes int64 (B,)) on the device; no host sync."""
        if imgs.dim() != 4 or imgs.shape[1] != 3 or imgs.dtype != torch.uint8:
            raise ValueError('Expected a uint8 B3HW image batch, got {} {}'.format(imgs.dtype, tuple(imgs.shape)))
        imgs = imgs.to('cuda').contiguous()
        B = imgs.shape[0]
        pads = None
        if paddings is not None:
            pads = ops.upload_small(np.ascontiguousarray(np.asarray(paddings, dtype=np.uint16).reshape(B, 4)).view(np.int16))
        return self._encode_frames(imgs, pads, workspace)

    def _encode_frames(self, imgs, pads, workspace):
        """The batch entry on device frames (B,3,H,W) and a device padding array (int16 (B,4) or None); sealed: the frames' CRCs
        (l3c_u8_crc32) and l3c_seal_append behind it on the same stream; parity-sealed: l3c_encode_batch_banded_parity alone."""
        B, _, H, W = imgs.shape
        stride = self.file_stride(H, W)
        ws = _bytes(self.encode_workspace_bytes(B, H, W)) if workspace is None else workspace
        files = torch.empty(B, stride, dtype=torch.uint8, device='cuda')
        file_bytes = torch.empty(B, dtype=torch.int64, device='cuda')
        d = EncodeBatchDesc(ctypes.pointer(self.model), ptr(imgs), B, H, W, ptr(pads), ptr(files), stride, ptr(file_bytes), ptr(ws), ws.numel())
        if self.parity:      # the whole parity-sealed encode: one call
            _lib.call('l3c_encode_batch_banded_parity', ctypes.byref(d), self.bands, ctypes.byref(self._parity_opts()), stream())
            return files, file_bytes
        if self.bands:
            _lib.call('l3c_encode_batch_banded', ctypes.byref(d), self.bands, stream())
        else:
            _lib.call('l3c_encode_batch', ctypes.byref(d), stream())
        if self.seal_bands:
            L = container.band_len(H * W, self.bands)
            band_crc, frame_crc = ops.u8_crc32_bands(imgs.view(-1), B, H * W, L)
            ops.seal_append_bands(files, file_bytes, frame_crc, band_crc, L, pads, self.model_id())
        elif self.seal:
            ops.seal_append(files, file_bytes, ops.u8_crc32(imgs.view(-1), B, 3 * H * W), pads, self.model_id())
        return files, file_bytes

    def encode_batch(self, imgs, paddings=None):
        """imgs: (B,3,H,W) uint8, H and W multiples of 2**num_scales; paddings: B tuples (left, right, top, bottom) or None
        -> list of B `.l3c` byte strings.  One D2H of the file sizes, then one of the slots."""
        return self.to_bytes(*self.encode_device(imgs, paddings))

    @staticmethod
    def to_bytes(files, file_bytes):
        """The result of encode_device on the host: one D2H of the file sizes (the synchronisation), then one of the slots' used part."""
        sizes = file_bytes.cpu().numpy()
        if (sizes < 0).any():
            raise _lib.L3CError('range coder overrun: a stream asked for more than 16 bits per symbol (table rows not strictly increasing)')
        B, mx = files.shape[0], int(sizes.max())
        host = _staging(B * mx).view(B, mx)
        host.copy_(files[:, :mx])
        torch.cuda.current_stream().synchronize()
        h = host.numpy()
        return [h[b, :sizes[b]].tobytes() for b in range(B)]

    # ---- decode --------------------------------------------------------------------------------------------------------------

    def decode_batch(self, files, workspace=None, sym=None, verify=True):
        """files: list of B `.l3c` byte strings of equally sized (padded) images, all legacy or all banded (their first four bytes say
        which; a mix raises ValueError) -> ((B,3,H,W) uint8 on the GPU, padding tuples).  The framing is parsed on the host by the library
        (ValueError with its message for an invalid file); files and plan cross PCIe in one copy from page-locked memory.
        sym: optional int16 (B,3,H,W) device tensor that receives the same values.
        Sealed files (a batch may mix sealed and unsealed ones): as Bitcoding.decode_batch -- container.SealError('generation' / 'model')
        before anything is enqueued, l3c_u8_crc32 on `pixels` and one D2H of B words after, SealError('pixels'); verify=False strips the
        seals and checks nothing.  Band-sealed files among them: ONE l3c_u8_crc32_bands on `pixels` instead, every band-sealed file compared
        band by band (SealError('pixels') with .bands and .rows), the version-1 sealed ones against the same call's frame words."""
        files, seals = self._split(files, verify)
        pixels, pads = self._decode_bodies(files, workspace, sym)
        if seals is not None:
            Bitcoding._check_pixels(seals, pixels, pads)
        return pixels, pads

    def decode_salvage(self, files, workspace=None):
        """Bitcoding.decode_salvage as library calls -> ((B,3,H,W) uint8 on the GPU, padding tuples, container.SalvageInfo): the same
        pixels and the same info.  l3c_decode_batch_banded with desc.sym; the finest record's P is what that call leaves in its workspace
        (l3c_decode_batch_banded_p_offset), so after ONE l3c_u8_crc32_bands and its D2H the bands that fail are concealed by ONE
        l3c_dmll_conceal on workspace + offset and the symbols, and one l3c_sym_to_u8.  SealError('generation' / 'model') and invalid
        files raise as in decode_batch; an intact batch launches no conceal kernel."""
        split = [self._split_seal(f) for f in files]
        files, seals = [b for b, _ in split], [s for _, s in split]
        if any(s is not None for s in seals):
            container.check_seals(seals, self.generation(), self.model_id)
        kept = {}
        pixels, pads = self._decode_bodies(files, workspace, None, kept)
        loss = self._losses.loss_dmol_rgb
        pixels, info = Bitcoding._salvage(seals, pixels, kept['sym'], kept.get('P'), pads, self.cfg.K, (loss.x_min, loss.x_max, loss.L))
        return pixels, pads, info

    def decode_repair(self, files, workspace=None):
        """Bitcoding.decode_repair as library calls -> ((B,3,H,W) uint8 on the GPU, padding tuples, container.RepairInfo): the same pixels
        and the same info.  container.heal_head on the host first, as there; then decode_salvage's decode and its ONE l3c_u8_crc32_bands
        with its D2H.  Where a parity-sealed file has a failing band, the parity sections of those files go up in ONE H2D, each at a
        16-byte aligned place of one buffer, and the rounds run: l3c_repair_round_plan on the host (Bitcoding._repair's selection and
        coefficients), one small H2D of its blob, ONE l3c_decode_repair_round (l3c_band_rebuild in place in the decode workspace's stream
        area -- every erased member of a group in one pass, the rows read where they lie in the section --, the positions' symbols zeroed,
        one l3c_decode_rgb_entries, l3c_sym_to_u8, one l3c_u8_crc32_spans) and a D2H of its 3 S words, until a plan has nothing left to
        try.  What still fails is concealed by Bitcoding._salvage.  info.files: the rebuilt payloads come back from their stream slots in
        one D2H and are spliced in at their framing offsets.  An intact batch makes exactly the library calls of decode_salvage."""
        lib = _lib.load()
        mended = [container.heal_head(f) for f in files]          # host only; an intact file comes back as the object it is
        given, files, heads = files, [f for f, _ in mended], [h for _, h in mended]
        split = [self._split_seal(f) for f in files]
        bodies, seals = [b for b, _ in split], [s for _, s in split]
        if any(s is not None for s in seals):
            container.check_seals(seals, self.generation(), self.model_id)
        kept = {'plan': None}
        pixels, pads = self._decode_bodies(bodies, workspace, None, kept)
        sym, B, (H, W) = kept['sym'], len(files), pixels.shape[2:]
        loss = self._losses.loss_dmol_rgb
        band_lens = {s.band_len for s in seals if s is not None and s.band_crcs is not None}
        words, repaired, healed, rounds = None, {}, [None] * B, 0
        if band_lens:
            L, = band_lens
            n = container.n_bands(H * W, L)
            words = Bitcoding._band_words(pixels, L)
            band_words = words[B:].reshape(B, 3, n)                           # (a view: what _salvage reads afterwards)
            _, failing, _ = container.failing_bands(seals, band_words, (H, W), pads)
            if failing and kept['plan'] is not None:
                repaired, healed, rounds = self._repair_rounds(lib, files, seals, kept, pixels, band_words, failing, pads)
        pixels, salvage = Bitcoding._salvage(seals, pixels, sym, kept.get('P'), pads, self.cfg.K, (loss.x_min, loss.x_max, loss.L), words)
        rows = {i: container.band_rows(sorted({j for _, j in got}), seals[i].band_len, (H, W), pads[i]) for i, got in repaired.items()}
        healed = [f if h is None and f is not g else h for h, f, g in zip(healed, files, given)]       # a head fix alone heals a file too
        return pixels, pads, container.RepairInfo(repaired, rows, salvage, healed, rounds, head=heads)

    def _repair_rounds(self, lib, files, seals, kept, pixels, band_words, failing, pads):
        """The rounds of decode_repair; band_words (B, 3, n) is updated in place with the words of the bands hashed again
        -> ({file: [(c, j)]} repaired, healed files, rounds run)."""
        B, _, H, W = pixels.shape
        n = band_words.shape[2]
        bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]
        # the parity sections of the files with a failing band, in front of their payloads' end: ONE H2D
        section_at, parts, at = np.full(B, -1, dtype=np.int64), [], 0
        for i in sorted(failing):
            body, par = ctypes.c_int64(), _lib.SealParityRS()
            if lib.l3c_seal_find_parity_rs(bufs[i].ctypes.data, bufs[i].size, ctypes.byref(body), None, None, ctypes.byref(par)) != 1 or par.m == 0:
                continue
            end = par.payloads - bufs[i].ctypes.data + par.payload_bytes
            section_at[i] = at
            parts.append((at, bufs[i][body.value:end]))
            at = (at + end - body.value + 15) // 16 * 16
        if not parts:
            return {}, [None] * B, 0
        up = np.zeros(at, dtype=np.uint8)
        for a, sec in parts:
            up[a:a + sec.size] = sec
        rows = ops.upload_small(up)
        plan, ws, sym = kept['plan'], kept['ws'], kept['sym']
        plan_host = plan.ctypes.data
        cap = _size(lib.l3c_repair_round_plan_bytes(self._cfg_ref, plan_host))
        blob = np.zeros(cap // 8 + 1, dtype=np.int64)
        file_ptrs = (ctypes.c_void_p * B)(*[b.ctypes.data for b in bufs])
        sizes = np.asarray([b.size for b in bufs], dtype=np.int64)
        tried, jobs, rounds = np.zeros(0, dtype=np.int32), [], 0
        while True:
            now = np.ascontiguousarray(band_words).view(np.uint32)
            n_groups = ctypes.c_int64()
            _check_plan(lib.l3c_repair_round_plan(self._cfg_ref, plan_host, file_ptrs, sizes.ctypes.data, now.ctypes.data, section_at.ctypes.data,
                                                  tried.ctypes.data if tried.size else None, tried.size // 9, blob.ctypes.data, cap,
                                                  ctypes.byref(n_groups)))
            if n_groups.value == 0:
                break
            rounds += 1
            groups_p, n_g, pos_p, S = ctypes.POINTER(_lib.RepairGroup)(), ctypes.c_int64(), ctypes.POINTER(ctypes.c_int32)(), ctypes.c_int64()
            _lib.check(lib.l3c_repair_round_groups(blob.ctypes.data, ctypes.byref(groups_p), ctypes.byref(n_g), ctypes.byref(pos_p), ctypes.byref(S)))
            groups = np.ctypeslib.as_array(ctypes.cast(groups_p, ctypes.POINTER(ctypes.c_int32)), shape=(n_g.value, 9)).copy()
            spots = np.ctypeslib.as_array(pos_p, shape=(S.value, 2)).astype(np.int64)
            tried = np.concatenate([tried.reshape(-1, 9), groups]).reshape(-1)
            jobs += [(int(g[0]), int(g[1]), int(j)) for g in groups for j in g[5:5 + g[3]]]
            n_blob = int(blob[1])                                             # word 1 of the header: the blob's size
            blob_d = ops.upload_small(blob[:n_blob // 8])
            rws = _bytes(_size(lib.l3c_decode_repair_round_workspace_bytes(self._cfg_ref, plan_host, blob.ctypes.data)))
            again = torch.empty(3 * S.value, dtype=torch.int32, device='cuda')
            side = self._side_stream(2 if S.value >= 16 else 1, [blob_d, rows, ws, sym, pixels, again, rws, self.targets_rgb])
            d = _lib.DecodeRepairRoundDesc(ctypes.pointer(self.model), plan_host, blob.ctypes.data, ptr(blob_d), n_blob, ptr(rows), rows.numel(),
                                           ptr(ws), ws.numel(), ptr(sym), ptr(pixels), ptr(again), ptr(rws), rws.numel())
            _lib.call('l3c_decode_repair_round', ctypes.byref(d), stream(), side)
            band_words[spots[None, :, 0], np.arange(3)[:, None], spots[None, :, 1]] = again.cpu().numpy().view(band_words.dtype).reshape(3, -1)
        _, failing, _ = container.failing_bands(seals, band_words, (H, W), pads)
        repaired, healed = {}, [None] * B
        for i, c, j in sorted(set(jobs)):                                     # (a payload tried with a second window is listed twice)
            if all((cc, j) not in failing.get(i, ()) for cc in range(3)):
                repaired.setdefault(i, []).append((c, j))
        # the repaired payloads from their stream slots, ONE D2H, spliced in at their framing offsets
        area = (ws.data_ptr() + 255) // 256 * 256 - ws.data_ptr() + _size(lib.l3c_decode_batch_banded_streams_offset(self._cfg_ref, plan_host))
        where = []
        for i, got in sorted(repaired.items()):
            for c, j in sorted(got):
                src, dst, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_uint32()
                _lib.check(lib.l3c_decode_plan_banded_stream(plan_host, self.cfg.num_scales, (c * B + i) * n + j, ctypes.byref(src), ctypes.byref(dst),
                                                             ctypes.byref(nb)))
                where.append((i, src.value - int(kept['offs'][i]), area + dst.value, nb.value))
        if where:
            back = torch.cat([ws[a:a + nb] for _, _, a, nb in where]).cpu().numpy()
            out, at = {}, 0
            for i, to, _, nb in where:
                f = out.setdefault(i, bytearray(files[i]))
                f[to:to + nb] = back[at:at + nb].tobytes()
                at += nb
            for i, f in out.items():
                healed[i] = bytes(f)
        for got in repaired.values():
            got.sort()
        return repaired, healed, rounds

    def _decode_bodies(self, files, workspace, sym, keep=None):
        """decode_batch behind the seals: the unsealed files -> (pixels, padding tuples), enqueued on the current stream.
        keep (decode_salvage): a dict that receives 'sym', the int16 symbols, 'ws', the workspace, and -- banded files -- 'P', the device
        address of the finest record's P in it, valid while 'ws' is held and not reused."""
        lib = _lib.load()
        B = len(files)
        banded = [container.is_banded(f) for f in files]
        if any(banded) and not all(banded):
            raise ValueError('decode_batch: a batch mixes banded and legacy .l3c files')
        banded = bool(banded and banded[0])
        plan_fn, decode_fn, ws_fn = ((lib.l3c_decode_plan_banded, 'l3c_decode_batch_banded', lib.l3c_decode_batch_banded_workspace_bytes) if banded
                                     else (lib.l3c_decode_plan, 'l3c_decode_batch', lib.l3c_decode_batch_workspace_bytes))
        if banded:
            n_plan = _plan_banded_bytes(self._cfg_ref, files)
            _check_plan(min(n_plan, 0))
        else:
            n_plan = _size(lib.l3c_decode_plan_bytes(self._cfg_ref, B))
        sizes = np.asarray([len(f) for f in files], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        plan_at = (int(offs[-1]) + 4 + 15) // 16 * 16
        k, stage = _RING.take(plan_at + n_plan)
        st = stage.numpy()
        for b, f in enumerate(files):
            st[offs[b]:offs[b + 1]] = np.frombuffer(f, dtype=np.uint8)
        st[offs[-1]:plan_at] = 0
        H, W, pads = ctypes.c_int(), ctypes.c_int(), np.zeros((B, 4), dtype=np.uint16)
        plan_host = stage.data_ptr() + plan_at
        _check_plan(plan_fn(self._cfg_ref, stage.data_ptr(), offs.ctypes.data_as(ctypes.POINTER(_lib.c_i64)), B, plan_host, n_plan,
                            ctypes.byref(H), ctypes.byref(W), pads.ctypes.data))
        dev = torch.empty(plan_at + n_plan, dtype=torch.uint8, device='cuda')
        dev.copy_(stage, non_blocking=True)
        _RING.sent(k)
        ws_bytes = _size(ws_fn(self._cfg_ref, plan_host))
        lag = int(np.frombuffer(stage.numpy()[plan_at + 88:plan_at + 96].tobytes(), dtype=np.int64)[0])      # word 11 of either header
        ws = _bytes(ws_bytes) if workspace is None else workspace
        pixels = torch.empty(B, 3, H.value, W.value, dtype=torch.uint8, device='cuda')
        if keep is not None:
            sym = torch.empty(B, 3, H.value, W.value, dtype=torch.int16, device='cuda')
            keep.update(sym=sym, ws=ws)
            if banded:      # (the plan is read here: its staging buffer goes back to the ring with this call)
                keep['P'] = (ws.data_ptr() + 255) // 256 * 256 + _size(lib.l3c_decode_batch_banded_p_offset(self._cfg_ref, plan_host))
                if 'plan' in keep:      # (decode_repair: the blob itself and where the files' bodies start in the plan's offsets)
                    keep.update(plan=st[plan_at:plan_at + n_plan].view(np.int64).copy(), offs=offs)
        if sym is not None and (sym.dtype != torch.int16 or tuple(sym.shape) != tuple(pixels.shape) or not sym.is_contiguous()):
            raise ValueError('sym must be a contiguous int16 tensor of shape {}'.format(tuple(pixels.shape)))
        side = None
        if lag == 2:
            if self._side is None:
                self._side = torch.cuda.Stream()
            side = self._side
            for t in (dev, ws, pixels, self.net.packed, self.targets_rgb) + (() if sym is None else (sym,)):
                t.record_stream(side)
        d = DecodeBatchDesc(ctypes.pointer(self.model), ptr(dev), plan_host, ptr(dev) + plan_at, n_plan, ptr(pixels), ptr(sym), ptr(ws), ws.numel())
        _lib.call(decode_fn, ctypes.byref(d), stream(), side.cuda_stream if side is not None else None)
        return pixels, [tuple(int(v) for v in p) for p in pads]

    def decode_region(self, files, box, verify=True):
        """The pixels of a BOX of B files of equally padded images, banded or legacy, without decoding the rest of their finest record
        -> ((B, 3, y1 - y0, x1 - x0) uint8 on the GPU, region.RegionInfo): Bitcoding.decode_region as library calls (l3c_decode_plan[_banded],
        l3c_decode_region_plan, l3c_decode_region).  box: (y0, y1) or (y0, y1, x0, x1) in the coordinates of the UNPADDED image.  Files,
        plan blob and region blob cross PCIe in one copy from page-locked memory; the library's refusals are ValueError /
        NotImplementedError with its message.  Sealed files: generation and model are checked (verify=True) before anything is enqueued;
        a seal's CRC covers the whole frame and is NOT checked -- the info says so.  A BAND-SEALED file is treated here as a version-1
        sealed one: generation and model checked, pixel_crc_checked False (l3c_decode_region plans the cut last band and keeps the window's
        pixels in its workspace; Bitcoding.decode_region verifies the decoded bands)."""
        lib = _lib.load()
        if not files:
            raise ValueError('decode_region: no files')
        try:
            box = tuple(int(v) for v in box)
        except (TypeError, ValueError):
            raise ValueError('box must be (y0, y1) or (y0, y1, x0, x1), got {!r}'.format(box))
        if len(box) not in (2, 4):
            raise ValueError('box must be (y0, y1) or (y0, y1, x0, x1), got {!r}'.format(box))
        B = len(files)
        sealed = sum(container.is_sealed(f) for f in files)
        files, seals = self._split(files, verify)
        banded = [container.is_banded(f) for f in files]
        if any(banded) and not all(banded):
            raise ValueError('decode_region: a batch mixes banded and legacy .l3c files')
        if banded[0]:
            plan_fn = lib.l3c_decode_plan_banded
            n_plan = _plan_banded_bytes(self._cfg_ref, files)
            _check_plan(min(n_plan, 0))
        else:
            plan_fn, n_plan = lib.l3c_decode_plan, _size(lib.l3c_decode_plan_bytes(self._cfg_ref, B))
        offs = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
        plan_at = (int(offs[-1]) + 4 + 15) // 16 * 16
        region_at = plan_at + (n_plan + 15) // 16 * 16
        region_cap = 3 * n_plan + 4096          # at least l3c_decode_region_plan_bytes: every array of the region blob is shorter than the plan's
        k, stage = _RING.take(region_at + region_cap)
        st = stage.numpy()
        for b, f in enumerate(files):
            st[offs[b]:offs[b + 1]] = np.frombuffer(f, dtype=np.uint8)
        st[offs[-1]:plan_at] = 0
        H, W, pads = ctypes.c_int(), ctypes.c_int(), np.zeros((B, 4), dtype=np.uint16)
        plan_host, region_host = stage.data_ptr() + plan_at, stage.data_ptr() + region_at
        _check_plan(plan_fn(self._cfg_ref, stage.data_ptr(), offs.ctypes.data_as(ctypes.POINTER(_lib.c_i64)), B, plan_host, n_plan,
                            ctypes.byref(H), ctypes.byref(W), pads.ctypes.data))
        if len(box) == 2:
            box = box + (0, W.value - int(pads[0, 0]) - int(pads[0, 1]))
        cbox = _lib.RegionBox(*(min(max(v, -2 ** 31), 2 ** 31 - 1) for v in box))
        info = _lib.RegionInfo()
        n_max = lib.l3c_decode_region_plan_bytes(self._cfg_ref, plan_host)
        _check_region(min(n_max, 0))
        if n_max > region_cap:
            raise _lib.L3CError('decode_region: a region blob of {} bytes beside a plan blob of {}'.format(n_max, n_plan))
        _check_region(lib.l3c_decode_region_plan(self._cfg_ref, plan_host, n_plan, pads.ctypes.data, ctypes.byref(cbox), region_host, region_cap,
                                                 ctypes.byref(info)))
        n_region = int(st[region_at + 8:region_at + 16].view(np.int64)[0])      # word 1 of the header: the blob's size
        dev = torch.empty(region_at + n_region, dtype=torch.uint8, device='cuda')
        dev.copy_(stage[:region_at + n_region], non_blocking=True)
        _RING.sent(k)
        ws_bytes = lib.l3c_decode_region_workspace_bytes(self._cfg_ref, plan_host, region_host)
        _check_region(min(ws_bytes, 0))
        ws = _bytes(ws_bytes)
        pixels = torch.empty(B, 3, info.out_rows, info.out_cols, dtype=torch.uint8, device='cuda')
        side = self._side_stream(info.lag, [dev, ws, pixels, self.net.packed, self.targets_rgb])
        d = DecodeRegionDesc(ctypes.pointer(self.model), ptr(dev), plan_host, dev.data_ptr() + plan_at, n_plan, region_host,
                             dev.data_ptr() + region_at, n_region, ptr(pixels), ptr(ws), ws.numel())
        _lib.call('l3c_decode_region', ctypes.byref(d), stream(), side)
        check = seals is not None
        pair = lambda a: (int(a[0]), int(a[1]))       # noqa: E731
        return pixels, region.RegionInfo(box=tuple(box), bands=pair(info.bands), n_bands=int(info.n_bands), sym_rows=pair(info.sym_rows),
                                         conv_rows=pair(info.conv_rows), valid_rows=pair(info.valid_rows), decoder_rows=pair(info.decoder_rows),
                                         frame_rows=int(info.frame_rows), streams_used=int(info.streams_used),
                                         streams_total=int(info.streams_total), bytes_used=int(info.bytes_used),
                                         bytes_total=int(info.bytes_total), sealed=sealed, verified=('generation', 'model') if check else (),
                                         pixel_crc_checked=False)

    @staticmethod
    def _split_seal(f):
        """container.split_seal(f, view=True) through the library (l3c_seal_find_bands: the same checks and messages; a band seal's table
        is checked against the finest record and the frame CRC in microseconds where the Python reader takes a tenth of a millisecond)."""
        if not container.is_sealed(f):
            return f, None
        lib = _lib.load()
        buf = np.frombuffer(f, dtype=np.uint8)
        body, seal, bands = ctypes.c_int64(), _lib.Seal(), _lib.SealBands()
        rc = lib.l3c_seal_find_bands(buf.ctypes.data, buf.size, ctypes.byref(body), ctypes.byref(seal), ctypes.byref(bands))
        if rc != 1:
            raise ValueError(lib.l3c_last_error().decode())
        crcs = None
        if bands.n:
            crcs = np.frombuffer(f, dtype='<u4', count=3 * bands.n, offset=bands.crc - buf.ctypes.data).reshape(3, bands.n)
        return memoryview(f)[:body.value], container.Seal(seal.generation, seal.frame_crc, seal.model_id, bands.band_len if bands.n else None, crcs)

    def _split(self, files, verify):
        """-> (the files without their seals, the seals to verify after the decode or None); generation and model id are checked here."""
        split = [self._split_seal(f) for f in files]
        seals = [s for _, s in split]
        if not verify or all(s is None for s in seals):
            return [b for b, _ in split], None
        container.check_seals(seals, self.generation(), self.model_id)
        return [b for b, _ in split], seals

    # ---- pictures as they come -----------------------------------------------------------------------------------------------

    @property
    def fac(self):
        return 1 << self.cfg.num_scales

    def encode_images_workspace_bytes(self, B, Hp, Wp):
        return _size(_lib.load().l3c_encode_images_workspace_bytes(self._cfg_ref, B, Hp, Wp, self.bands))

    def encode_images_device(self, src, table, Hp, Wp, table_dev=None, src_bytes=None, workspace=None):
        """For pixels that are already on the GPU.  src: device uint8 buffer the views of `table` (numpy array of IMAGE_DTYPE, one entry per
        image, `top` / `left` set: centre padding is l3c_image_padding / pad.padding_for) lie in; table_dev: its device copy (a device
        pointer or uint8 tensor; None: uploaded here).  Enqueues l3c_encode_images on the current stream -> (files uint8 (B, file_stride),
        file_bytes int64 (B,)) on the device, as encode_device."""
        table = np.ascontiguousarray(table, dtype=IMAGE_DTYPE)
        B = len(table)
        if table_dev is None:
            table_dev = ops.upload_small(table.view(np.uint8))
        if self.seal:      # the seal hashes the padded frames: gather them into a buffer of our own, then the batch entry on them (the same files)
            frames = torch.empty(B, 3, Hp, Wp, dtype=torch.uint8, device='cuda')
            pads = torch.empty(B, 4, dtype=torch.int16, device='cuda')
            _lib.call('l3c_u8_gather', ptr(src), src.numel() if src_bytes is None else src_bytes, table.ctypes.data,
                      table_dev if isinstance(table_dev, int) else ptr(table_dev), B, Hp, Wp, ptr(frames), ptr(pads), stream())
            return self._encode_frames(frames, pads, None)
        stride = self.file_stride(Hp, Wp)
        ws = _bytes(self.encode_images_workspace_bytes(B, Hp, Wp)) if workspace is None else workspace
        files = torch.empty(B, stride, dtype=torch.uint8, device='cuda')
        file_bytes = torch.empty(B, dtype=torch.int64, device='cuda')
        d = EncodeImagesDesc(ctypes.pointer(self.model), ptr(src), src.numel() if src_bytes is None else src_bytes, table.ctypes.data,
                             table_dev if isinstance(table_dev, int) else ptr(table_dev), B, Hp, Wp, self.bands, ptr(files), stride,
                             ptr(file_bytes), ptr(ws), ws.numel())
        _lib.call('l3c_encode_images', ctypes.byref(d), stream())
        return files, file_bytes

    def encode_images(self, images, layout='chw', max_batch=16):
        """images: list of host uint8 tensors or numpy arrays, each of its own size, all in `layout` ('chw' (3,h,w); 'hwc' (h,w,3); 'hwcx'
        (h,w,4), the fourth byte ignored; 'bgr' (h,w,3) or (h,w,4) in B, G, R[, X] order) -> list of `.l3c` byte strings in input order: the
        files of Bitcoding on the zero-padded images (dataset_codec.encode_set's).  Images that pad to one shape share a call of at most
        max_batch; each group is staged back to back in page-locked memory with its table and crosses PCIe in ONE copy."""
        arrs = [_host_u8(i, im) for i, im in enumerate(images)]
        entries = [image_entry(layout, a.shape, 0) for a in arrs]
        shapes = {i: (e[4], e[5]) for i, e in enumerate(entries)}
        chunks, padded, pads, _ = dataset_codec.plan_set(shapes, range(len(arrs)), max_batch, self.fac)
        pending = []
        for chunk, (Hp, Wp) in zip(chunks, padded):
            sizes = [arrs[i].size for i in chunk]
            table_at = (sum(sizes) + 15) // 16 * 16
            k, stage = _RING.take(table_at + IMAGE_DTYPE.itemsize * len(chunk))
            st = stage.numpy()
            table = st[table_at:].view(IMAGE_DTYPE)
            off = 0
            for b, (i, n) in enumerate(zip(chunk, sizes)):
                st[off:off + n] = arrs[i].reshape(-1)
                left, _, top, _ = pads[i]
                table[b] = image_entry(layout, arrs[i].shape, off, top, left)
                off += n
            dev = torch.empty(stage.numel(), dtype=torch.uint8, device='cuda')
            dev.copy_(stage, non_blocking=True)
            _RING.sent(k)
            pending.append((chunk, self.encode_images_device(dev, table, Hp, Wp, table_dev=dev.data_ptr() + table_at, src_bytes=table_at)))
        out = [None] * len(arrs)
        for chunk, (files, file_bytes) in pending:
            for i, f in zip(chunk, self.to_bytes(files, file_bytes)):
                out[i] = f
        return out

    def decode_images_workspace_bytes(self, blob):
        buf = np.frombuffer(bytes(blob), dtype=np.int64)
        return _size(_lib.load().l3c_decode_images_workspace_bytes(self._cfg_ref, buf.ctypes.data))

    def _side_stream(self, lag, tensors):
        if lag != 2:
            return None
        if self._side is None:
            self._side = torch.cuda.Stream()
        for t in tensors:
            if t is not None:
                t.record_stream(self._side)
        return self._side.cuda_stream

    def decode_images_device(self, files_dev, plan_blob, plan_dev, dst, table, table_dev=None, workspace=None, sym=None):
        """For callers whose buffers are already on the GPU.  files_dev: the files' bytes at the offsets the plan was made with; plan_blob:
        the planner's blob (decode_plan / decode_plan_banded) on the host, plan_dev its device copy (pointer or uint8 tensor); dst: the
        device uint8 buffer the views of `table` (numpy IMAGE_DTYPE array; top / left / h / w from the planner's paddings) lie in.
        Enqueues l3c_decode_images on the current stream; exactly the bytes the views address are written."""
        table = np.ascontiguousarray(table, dtype=IMAGE_DTYPE)
        if table_dev is None:
            table_dev = ops.upload_small(table.view(np.uint8))
        blob = np.frombuffer(bytes(plan_blob), dtype=np.int64)
        self._decode_images_call(files_dev, blob.ctypes.data, plan_dev if isinstance(plan_dev, int) else ptr(plan_dev), blob.nbytes, int(blob[11]), dst,
                                 table.ctypes.data, table_dev if isinstance(table_dev, int) else ptr(table_dev), workspace, sym, (plan_dev, table_dev))

    def _decode_images_call(self, files_dev, plan_host, plan_dev, n_plan, lag, dst, table_host, table_dev, workspace, sym, keep=()):
        ws = _bytes(_size(_lib.load().l3c_decode_images_workspace_bytes(self._cfg_ref, plan_host))) if workspace is None else workspace
        side = self._side_stream(lag, [files_dev, ws, dst, sym, self.net.packed, self.targets_rgb] + [t for t in keep if isinstance(t, torch.Tensor)])
        d = DecodeImagesDesc(ctypes.pointer(self.model), ptr(files_dev), plan_host, plan_dev, n_plan, ptr(dst), dst.numel(), table_host, table_dev,
                             ptr(sym), ptr(ws), ws.numel())
        _lib.call('l3c_decode_images', ctypes.byref(d), stream(), side)

    def decode_images(self, files, layout='chw', max_batch=16, verify=True):
        """files: list of `.l3c` byte strings, legacy and banded alike, of any sizes -> list of device uint8 tensors in input order, each the
        ORIGINAL size (the padding undone) in `layout` ('hwcx': the fourth byte is 0; 'bgr': (h,w,3)).  Files of one format and padded shape
        share a call of at most max_batch (dataset_codec.plan_decode_set); each group decodes into one packed buffer, the tensors are views
        of it.  Files, plan and table cross PCIe in one copy from page-locked memory.
        Sealed files are verified as in decode_batch: a group that holds one decodes through l3c_decode_batch(_banded) into a frame buffer,
        l3c_u8_crc32 on it, then l3c_u8_scatter -- what l3c_decode_images does, with the hash in between; the CRC words of all groups come
        back in ONE D2H at the end.  SealError.index is the file's place in `files`."""
        lib = _lib.load()
        image_shape(layout, 1, 1)
        files, seals = self._split(files, verify)
        crcs = []
        chunks, _ = dataset_codec.plan_decode_set(files, range(len(files)), max_batch)
        out = [None] * len(files)
        for chunk in chunks:
            fs = [files[i] for i in chunk]
            B = len(fs)
            if container.is_banded(fs[0]):
                plan_fn = lib.l3c_decode_plan_banded
                n_plan = _plan_banded_bytes(self._cfg_ref, fs)
                _check_plan(min(n_plan, 0))
            else:
                plan_fn, n_plan = lib.l3c_decode_plan, _size(lib.l3c_decode_plan_bytes(self._cfg_ref, B))
            offs = np.concatenate([[0], np.cumsum([len(f) for f in fs])]).astype(np.int64)
            plan_at = (int(offs[-1]) + 4 + 15) // 16 * 16
            table_at = plan_at + (n_plan + 15) // 16 * 16
            k, stage = _RING.take(table_at + IMAGE_DTYPE.itemsize * B)
            st = stage.numpy()
            for b, f in enumerate(fs):
                st[offs[b]:offs[b + 1]] = np.frombuffer(f, dtype=np.uint8)
            st[offs[-1]:plan_at] = 0
            H, W, pads = ctypes.c_int(), ctypes.c_int(), np.zeros((B, 4), dtype=np.uint16)
            plan_host = stage.data_ptr() + plan_at
            _check_plan(plan_fn(self._cfg_ref, stage.data_ptr(), offs.ctypes.data_as(ctypes.POINTER(_lib.c_i64)), B, plan_host, n_plan,
                                ctypes.byref(H), ctypes.byref(W), pads.ctypes.data))
            table = st[table_at:].view(IMAGE_DTYPE)
            views, off = [], 0
            for b, (left, right, top, bottom) in enumerate(pads.astype(np.int64).tolist()):
                h, w = H.value - top - bottom, W.value - left - right
                if h < 1 or w < 1:
                    raise ValueError('invalid file: the padding {} leaves nothing of the {} x {} image'.format((left, right, top, bottom), H.value, W.value))
                shape = image_shape(layout, h, w)
                table[b] = image_entry(layout, shape, off, top, left)
                views.append((off, shape))
                off += int(np.prod(shape))
            dev = torch.empty(stage.numel(), dtype=torch.uint8, device='cuda')
            dev.copy_(stage, non_blocking=True)
            _RING.sent(k)
            lag = int(st[plan_at + 88:plan_at + 96].view(np.int64)[0])      # word 11 of either header
            dst = (torch.zeros if layout == 'hwcx' else torch.empty)(off, dtype=torch.uint8, device='cuda')
            if seals is not None and any(seals[i] is not None for i in chunk):
                banded = container.is_banded(fs[0])
                ws = _bytes(_size((lib.l3c_decode_batch_banded_workspace_bytes if banded else lib.l3c_decode_batch_workspace_bytes)(self._cfg_ref, plan_host)))
                pixels = torch.empty(B, 3, H.value, W.value, dtype=torch.uint8, device='cuda')
                side = self._side_stream(lag, [dev, ws, pixels, self.net.packed, self.targets_rgb])
                d = DecodeBatchDesc(ctypes.pointer(self.model), ptr(dev), plan_host, dev.data_ptr() + plan_at, n_plan, ptr(pixels), None, ptr(ws), ws.numel())
                _lib.call('l3c_decode_batch_banded' if banded else 'l3c_decode_batch', ctypes.byref(d), stream(), side)
                crcs.append((chunk, ops.u8_crc32(pixels.view(-1), B, 3 * H.value * W.value)))
                _lib.call('l3c_u8_scatter', ptr(pixels), B, H.value, W.value, ptr(dst), dst.numel(), stage.data_ptr() + table_at,
                          dev.data_ptr() + table_at, stream())
            else:
                self._decode_images_call(dev, plan_host, dev.data_ptr() + plan_at, n_plan, lag, dst, stage.data_ptr() + table_at,
                                         dev.data_ptr() + table_at, None, None)
            for i, (o, shape) in zip(chunk, views):
                out[i] = dst[o:o + int(np.prod(shape))].view(shape)
        if crcs:
            words = torch.cat([c for _, c in crcs]).cpu().numpy()
            got = dict(zip([i for chunk, _ in crcs for i in chunk], words))
            container.check_frame_crcs([s if i in got else None for i, s in enumerate(seals)], [got.get(i, 0) for i in range(len(seals))])
        return out
