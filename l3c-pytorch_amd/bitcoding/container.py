"""The host side of the `.l3c` framing, both formats: what a file's bytes mean, and nothing else (no torch, no library call; the device
reader and writer of the same bytes are csrc/container.hip).

LEGACY files -- the reference's byte format (bitcoding.py:326-375):

    u16 x4  padding (left, right, top, bottom)
    for scale = coarsest .. 0:   u8 C, u16 H, u16 W;  for each channel: u32 nbytes, payload;  magic 46 E2 84 92

BANDED files (opt-in, Bitcoding(bands=K); INTEGRATION.md "Banded .l3c files"):

    'L3CB' | u8 version = 1 | u8 0 | u16 x4 padding
    for scale = coarsest .. 0:  u8 C, u16 H, u16 W, u32 L | for channel c: for band j < n = ceil(H*W / L): u32 nbytes, payload | magic

Band j of channel c is pixels [j L, min((j + 1) L, H W)) in raster order, coded as a stream of its own with the legacy format's rows.
A legacy file cannot start with the signature: its first u16 is the left padding, below the padding factor ('L3' reads 13132).
An L3C file has num_scales + 1 scale records; an RGB Shared file one more per recursion.  The headers are untrusted input: every reader
here raises ValueError('invalid file: ...') on broken framing."""
import struct

import numpy as np

_MAGIC_VALUE_SEP = b'\x46\xE2\x84\x92'
BANDED_SIGNATURE = b'L3CB'
BANDED_VERSION = 1
MAX_BANDS = 1024


def band_len(hw, bands):
    """L_s of a scale of hw symbols for the requested band count K: 64 ceil(hw / (64 K)) -- at most K bands of whole 64-symbol blocks."""
    if not 1 <= int(bands) <= MAX_BANDS:
        raise ValueError('bands must be in 1..{}, got {}'.format(MAX_BANDS, bands))
    return 64 * (-(-int(hw) // (64 * int(bands))))


def n_bands(hw, L):
    return -(-int(hw) // int(L))


def is_banded(data):
    return bytes(data[:4]) == BANDED_SIGNATURE


class _Reader(object):
    def __init__(self, data):
        self.d, self.p = data, 0

    def take(self, n):
        b = self.d[self.p:self.p + n]
        if len(b) != n:
            raise ValueError('invalid file: truncated')
        self.p += n
        return b

    def unpack(self, fmt):
        return struct.unpack(fmt, self.take(struct.calcsize(fmt)))


class ParsedFraming(object):
    """Where the payloads lie: padding, per scale record (coarsest first) its header (`scales`) and, as int64 arrays, every payload's
    position inside its file (`offset`) and its length (`nbytes`).
      parse_containers (B legacy files)   padding: B tuples, scales: (C, H, W),    arrays (B, C)
      parse_banded (one banded file)      padding: a tuple,  scales: (C, H, W, L), arrays (C, n)
      parse_batch (B files, either)       padding: B tuples, scales: (S, H, W),    arrays (B, S), S streams per image"""

    def __init__(self, padding, scales, offset, nbytes):
        self.padding, self.scales, self.offset, self.nbytes = padding, scales, offset, nbytes


def count_scale_records(data):
    """Number of scale records of a legacy `.l3c` byte string; ValueError if the framing is broken.  A BANDED file is refused
    here (and so by every reader of the legacy framing: decode_many, dataset_codec.decode_set): `parse_banded` reads those."""
    if is_banded(data):
        raise ValueError('banded .l3c file (L3CB format): only Bitcoding.decode_batch / decode read it, not the legacy-format readers')
    r = _Reader(data)
    r.take(8)
    n = 0
    while r.p < len(data):
        C, _, _ = r.unpack('<BHH')
        for _ in range(C):
            nb, = r.unpack('<I')
            r.take(nb)
        if r.take(4) != _MAGIC_VALUE_SEP:
            raise ValueError('invalid file: scale separator missing')
        n += 1
    if n < 2:
        raise ValueError('invalid file: {} scale record(s)'.format(n))
    return n


def parse_containers(files):
    """B legacy files of equally sized images, walked by their length fields only.  ValueError on broken framing, a record with C == 0,
    or when the files disagree in shape."""
    B = len(files)
    padding, scales, offset, nbytes = [], None, None, None
    for b, f in enumerate(files):
        n_rec = count_scale_records(f)
        if scales is None:
            scales = [None] * n_rec
            offset, nbytes = [None] * n_rec, [None] * n_rec
        elif n_rec != len(scales):
            raise ValueError('decode_batch needs equally sized images: {} vs {} scale records'.format(n_rec, len(scales)))
        padding.append(struct.unpack_from('<4H', f, 0))
        p = 8
        for k in range(n_rec):
            shape = struct.unpack_from('<BHH', f, p)
            p += 5
            if shape[0] == 0:
                raise ValueError('invalid file: scale record with C == 0')
            if scales[k] is None:
                scales[k] = shape
                offset[k] = np.zeros((B, shape[0]), dtype=np.int64)
                nbytes[k] = np.zeros((B, shape[0]), dtype=np.int64)
            elif shape != scales[k]:
                raise ValueError('decode_batch needs equally sized images, got shapes {}'.format(sorted({shape, scales[k]})))
            for c in range(shape[0]):
                n, = struct.unpack_from('<I', f, p)
                offset[k][b, c] = p + 4
                nbytes[k][b, c] = n
                p += 4 + n
            p += 4                                   # the separator (count_scale_records has checked it)
    return ParsedFraming(padding, scales, offset, nbytes)


def parse_banded(data):
    """One banded file, walked by its length fields.  ValueError('invalid file: ...') on an unknown version or reserved byte, C == 0, an empty
    scale, L == 0 or not a multiple of 64, more than 1024 bands, a length field or payload past the end, a missing magic."""
    if _Reader(data).take(4) != BANDED_SIGNATURE:
        raise ValueError('invalid file: not a banded .l3c file')
    _, padding, found = _walk_prefix(data)
    if (found[-1][3] if found else 14) != len(data):       # the walk stopped inside a record: data behind the last complete one (the file header: 14 bytes)
        raise ValueError('invalid file: truncated')
    if len(found) < 2:
        raise ValueError('invalid file: {} scale record(s)'.format(len(found)))
    return ParsedFraming(padding, [h for h, _, _, _ in found], [o for _, o, _, _ in found], [n for _, _, n, _ in found])


def parse_batch(files):
    """The files of one decode_batch call, either format (not mixed) -> (records, streams, banded): `records` the format's own scale
    headers -- (C, H, W), banded (C, H, W, L) --, the same in every file; `streams` the upload-ready ParsedFraming with every (channel, band) of a
    banded file as a "channel": S = C n streams per image, stream c n + j."""
    if not any(is_banded(f) for f in files):
        streams = parse_containers(files)
        return streams.scales, streams, False
    if not all(is_banded(f) for f in files):
        raise ValueError('decode_batch: a batch mixes banded and legacy .l3c files')
    parsed = [parse_banded(f) for f in files]
    records = parsed[0].scales
    for p in parsed[1:]:
        if len(p.scales) != len(records) or any(a[:3] != b[:3] for a, b in zip(p.scales, records)):
            raise ValueError('decode_batch needs equally sized images, got scale records {} and {}'.format(
                [s[:3] for s in records], [s[:3] for s in p.scales]))
        if any(a[3] != b[3] for a, b in zip(p.scales, records)):
            raise ValueError('decode_batch: banded files of one batch must share the band length of every scale, got {} and {}'.format(
                [s[3] for s in records], [s[3] for s in p.scales]))
    return records, ParsedFraming([p.padding for p in parsed], [(C * n_bands(H * W, L), H, W) for C, H, W, L in records],
                                  [np.stack([p.offset[k].reshape(-1) for p in parsed]) for k in range(len(records))],
                                  [np.stack([p.nbytes[k].reshape(-1) for p in parsed]) for k in range(len(records))]), True


# ---- a PREFIX of a file (Bitcoding.decode_preview): the first records of a file that may end anywhere after them ------------------------


class _Truncated(Exception):
    """The data ends inside the record being read: the record is not part of the prefix."""


class _PrefixReader(_Reader):
    def take(self, n):
        if self.p + n > len(self.d):
            raise _Truncated()
        return _Reader.take(self, n)


def _walk_prefix(data, max_records=None):
    """The complete scale records at the start of `data`, either format -> (banded, padding, [(header, offset (C, n), nbytes (C, n), end)]),
    `end` the position behind the record's separator.  The walk stops, without an error, where the data ends inside a record (or at
    max_records); what the full parsers reject in a record that IS complete -- and in the file header -- raises as they raise."""
    banded = is_banded(data)
    r = _PrefixReader(data)
    try:
        if banded:
            r.take(4)
            version, reserved = r.unpack('<BB')
            if version != BANDED_VERSION:
                raise ValueError('invalid file: unknown banded format version {}'.format(version))
            if reserved:
                raise ValueError('invalid file: reserved byte is {}'.format(reserved))
        padding = r.unpack('<4H')
    except _Truncated:
        raise ValueError('invalid file: truncated')
    found = []
    while max_records is None or len(found) < max_records:
        try:
            if banded:
                C, H, W, L = header = r.unpack('<BHHI')
            else:
                C, H, W = header = r.unpack('<BHH')
            if C == 0:
                raise ValueError('invalid file: scale record with C == 0')
            n = 1
            if banded:
                if H == 0 or W == 0:
                    raise ValueError('invalid file: empty scale {}x{}'.format(H, W))
                if L == 0 or L % 64:
                    raise ValueError('invalid file: band length {} is not a positive multiple of 64'.format(L))
                n = n_bands(H * W, L)
                if n > MAX_BANDS:
                    raise ValueError('invalid file: {} bands per channel (at most {})'.format(n, MAX_BANDS))
            off = np.zeros((C, n), dtype=np.int64)
            nb = np.zeros((C, n), dtype=np.int64)
            for c in range(C):
                for j in range(n):
                    nb[c, j], = r.unpack('<I')
                    off[c, j] = r.p
                    r.take(int(nb[c, j]))
            if r.take(4) != _MAGIC_VALUE_SEP:
                raise ValueError('invalid file: scale separator missing')
        except _Truncated:
            break
        found.append((header, off, nb, r.p))
    return banded, padding, found


def prefix_bytes(data, records):
    """Byte length of the shortest prefix of a file (either format) that holds its first `records` scale records: the file header, the
    records' headers, payloads and separators.  ValueError when `data` holds fewer complete records."""
    if records < 1:
        raise ValueError('records must be at least 1, got {}'.format(records))
    found = _walk_prefix(data, records)[2]
    if len(found) < records:
        raise ValueError('invalid file: {} complete scale record(s), {} asked for'.format(len(found), records))
    return found[-1][3]


def parse_prefix(files, max_records=None):
    """B files or PREFIXES of files of equally sized images, either format (not mixed) -> (records, streams, banded, n): the first n scale
    records that are complete in EVERY file (at most max_records), as parse_batch returns them.  The data may end anywhere behind them:
    a cut inside record n + 1 is not an error.  Inside the kept records everything parse_containers / parse_banded reject raises
    ValueError('invalid file: ...'), as do files that disagree in format, shape or band length, and data without one complete record."""
    if max_records is not None and max_records < 1:
        raise ValueError('max_records must be at least 1, got {}'.format(max_records))
    if len({is_banded(f) for f in files}) != 1:
        raise ValueError('decode_preview: a batch mixes banded and legacy .l3c files' if files else 'decode_preview: no files')
    walked = [_walk_prefix(f, max_records) for f in files]
    banded = walked[0][0]
    n = min(len(w[2]) for w in walked)
    if n < 1:
        raise ValueError('invalid file: not one complete scale record')
    records = [h for h, _, _, _ in walked[0][2][:n]]
    for w in walked[1:]:
        other = [h for h, _, _, _ in w[2][:n]]
        if any(a[:3] != b[:3] for a, b in zip(other, records)):
            raise ValueError('decode_preview needs equally sized images, got scale records {} and {}'.format(
                [s[:3] for s in records], [s[:3] for s in other]))
        if other != records:
            raise ValueError('decode_preview: banded files of one batch must share the band length of every scale, got {} and {}'.format(
                [s[3] for s in records], [s[3] for s in other]))
    streams = ParsedFraming([w[1] for w in walked], [(h[0] * (n_bands(h[1] * h[2], h[3]) if banded else 1), h[1], h[2]) for h in records],
                            [np.stack([w[2][k][1].reshape(-1) for w in walked]) for k in range(n)],
                            [np.stack([w[2][k][2].reshape(-1) for w in walked]) for k in range(n)])
    return records, streams, banded, n


def parse_set_entry(files):
    """The banded files of ONE entry of a set decode (equally sized images written with one band count: Bitcoding.decode_many(banded=True))
    -> (records, streams): `records` every scale's (C, H, W, L), the same in every file; `streams` the upload-ready band stream table of
    parse_batch -- per scale the (B, C n) positions and lengths of every file's band payloads, band j of channel c at column c n + j.
    ValueError for a legacy file among them, broken framing, or files that disagree in a shape or a band length."""
    if not all(is_banded(f) for f in files):
        raise ValueError('decode_many: an entry mixes banded and legacy .l3c files')
    records, streams, _ = parse_batch(files)
    return records, streams


def band_lengths(data):
    """(L per scale record, coarsest first) of a banded file, None for a legacy one."""
    return tuple(s[3] for s in parse_banded(data).scales) if is_banded(data) else None


def padded_shape(data):
    """(H, W) of the PADDED image a file of either format holds: 2**(records - 1) times its first (coarsest) scale record's H, W.
    Cheap: the record count comes from walking the length fields, no payload is touched."""
    if is_banded(data):
        scales = parse_banded(data).scales
        n, (_, H, W, _) = len(scales), scales[0]
    else:
        n = count_scale_records(data)
        _, H, W = struct.unpack_from('<BHH', data, 8)
    return (H << (n - 1), W << (n - 1))


def framing_bytes(scales, banded):
    """Bytes of a file that are not payload.  scales: the headers (C, H, W), banded (C, H, W, L)."""
    if banded:
        return 14 + sum(9 + 4 * C * n_bands(H * W, L) + 4 for C, H, W, L in scales)
    return 8 + sum(5 + 4 * C + 4 for C, _, _ in scales)


def write_file(padding, scales, payloads, banded):
    """-> the bytes of one file.  scales: (C, H, W) headers for a legacy file, payloads[k][c] the bytes of channel c of record k;
    (C, H, W, L) headers for a banded file, payloads[k][c] the list of that channel's band payloads."""
    chunks = [BANDED_SIGNATURE, struct.pack('<BB4H', BANDED_VERSION, 0, *padding)] if banded else [struct.pack('<4H', *padding)]
    for header, channels in zip(scales, payloads):
        chunks.append(struct.pack('<BHHI' if banded else '<BHH', *header))
        for c in channels:
            for p in (c if banded else [c]):
                chunks += [struct.pack('<I', len(p)), p]
        chunks.append(_MAGIC_VALUE_SEP)
    return b''.join(chunks)


# ---- ENTRY tables of the ragged decoders (ops.decode_z_entries, ops.decode_rgb_entries): entry e is pixels [pix0, pix0 + length) of an image
# of hw pixels that starts at pixel pixbase of the group's P and symbol buffers -> (pixbase, hw, pix0, length), int64 arrays of one row per entry


def band_entry_table(B, HW, L, pixbase0=0):
    """Every band of B images of HW pixels, band length L, the first image at pixel pixbase0: B n entries in the order (image, band);
    band j of image b is pixels [j L, min((j + 1) L, HW)) of the image at pixbase0 + b HW."""
    n = n_bands(HW, L)
    pix0 = np.tile(np.arange(n, dtype=np.int64), B) * L
    return (pixbase0 + np.repeat(np.arange(B, dtype=np.int64), n) * HW, np.full(B * n, HW, dtype=np.int64), pix0, np.minimum(L, HW - pix0))


def image_entry_table(hws, pixbase0=0):
    """Whole images of hws pixels, one after the other from pixel pixbase0: an entry per image, pix0 = 0 and length = hw."""
    hw = np.asarray(hws, dtype=np.int64)
    return pixbase0 + np.cumsum(hw) - hw, hw, np.zeros(hw.shape[0], dtype=np.int64), hw


# ---- SEALED files (opt-in, Bitcoding(seal=True); INTEGRATION.md "Sealed files"; the C side is csrc/seal.h) -----------------------------------
#
# 24 bytes behind the last separator of a file of either format, little-endian:
#     'L3CS' | u8 version = 1 | u8 flags = 0 | u16 bitstream generation | u32 frame CRC | u64 model id | u32 check
# frame CRC: zlib.crc32 of the padded planar frame [3][H][W]; model id: 0 = not stated; check: zlib.crc32 of the file's 8 padding bytes
# followed by seal bytes 0..19.  The parsers above never see a seal: callers split it off first.
#
# BAND SEALS (opt-in, Bitcoding(bands=K, seal='bands'); INTEGRATION.md "Band seals"), banded files only: seal version 2 with a BAND TABLE in
# front of the 24 bytes, T = 20 + 12 n bytes:
#     'L3CT' | u16 n | u16 0 | u32 L | u32 crc[3][n] (channel-major) | u32 T | separator 46 E2 84 92
# n, L: bands per channel and band length of the finest record; crc[c][j]: zlib.crc32 of bytes [c HW + j L, c HW + min((j + 1) L, HW)) of
# the padded planar frame.  The check word runs over the padding bytes, the whole table and seal bytes 0..19; the frame CRC stays and must
# be the combination of the band CRCs (combine_band_crcs).  The recognition rule (is_sealed) is the same: the table ends with the separator.

#
# PARITY BANDS (opt-in, Bitcoding(bands=K, seal='bands', parity=G); INTEGRATION.md "Parity bands"): seal version 3, a band seal with a PARITY
# SECTION between the body and the band table, S = 16 + 12 m + sum(plen) bytes:
#     'L3CP' | u16 G | u16 m | u32 plen[3][m] (channel-major) | the 3 m parity payloads, (c, g) order, back to back | u32 S | separator
# m = ceil(n / G) groups per channel of the finest record's n bands; group g of channel c holds the bands { j : j % m == g } (interleaved:
# adjacent bands lie in different groups), its parity payload is the XOR of its members' payloads, each zero-extended to plen[c][g], the
# longest member's byte count (band_parity).  The check word runs over the padding bytes, the section's head (bytes [0, 8 + 12 m)), its
# last 8 bytes, the band table and seal bytes 0..19 -- NOT over the parity payloads: a damaged parity stream can only make a repair fail,
# which the band CRCs then notice.  The section ends with the separator, so the band table still starts behind one.
#
# R = 2..4 PARITY STREAMS PER GROUP (Bitcoding(parity=G, parity_streams=R)): the same seal version with a section of a second kind,
# S = 20 + 12 m + R sum(plen) bytes:
#     'L3CQ' | u16 G | u16 m | u16 R | u16 0 | u32 plen[3][m] | the 3 m R payloads, (c, g, r) order, plen[c][g] bytes each | u32 S | separator
# Row r of a group is the XOR over its members k (band g + k m) of alpha^(k r) d_k in GF(2^8), polynomial 0x11D, alpha = 0x02 (rs_parity);
# row 0 is the 'L3CP' payload; G <= 255.  The check word covers section bytes [0, 12 + 12 m) and the last 8.  R = 1 is always 'L3CP'.
#
# The code below knows ONE section of R rows per group: 'L3CP' is R = 1, and differs in its signature and the length of its head
# (_SECTION_KINDS) alone.  A Seal keeps the rows as [c][g][r]; band_parity is rs_parity with one row.

#
# HEAD PARITY (Bitcoding(parity=G, parity_head=True); INTEGRATION.md "Head parity"): the same seal version with a section of a third kind,
# 'L3CH' -- an 'L3CQ' section (R = 1..4, all written in this shape) with a HEAD PART between the finest record's rows and the last 8 bytes:
#     'L3CH' | u16 G | u16 m | u16 R | u16 0 | u32 plen[3][m] | the 3 m R finest rows | A = 12 + 12 m + R sum(plen): HEAD PART | u32 S | separator
#     HEAD PART: u16 n_records | u16 0 | FRAMING COPY: body[0:14], per record (coarsest first) its 9 header bytes and u32 nbytes[C][n] |
#         u32 head_crc = crc32(body[0:P0)), P0 where the finest record's header starts |
#         per head record k (all but the finest): u32 crc[C][n_k] of the band payloads | u16 G_k = min(G, n_k) | u16 m_k | u32 hplen[C][m_k] |
#         the rows: per head record, (c, g, r) order, hplen[k][c][g] bytes each (rs_parity per channel) |
#         u32 head_check = crc32 of the head part up to the first row byte
# The seal's check word covers what it covers for 'L3CQ'; the head part is guarded by head_check alone, and a damaged one never makes a
# file unreadable: split_seal returns a Seal with head=None, head_damaged=True.  heal_head restores a file's head from it.

SEAL_SIGNATURE = b'L3CS'
SEAL_VERSION = 1
SEAL_VERSION_BANDS = 2
SEAL_VERSION_PARITY = 3
SEAL_BYTES = 24
TABLE_SIGNATURE = b'L3CT'
PARITY_SIGNATURE = b'L3CP'
PARITY_RS_SIGNATURE = b'L3CQ'
HEAD_SIGNATURE = b'L3CH'
_SECTION_KINDS = {PARITY_SIGNATURE: 8, PARITY_RS_SIGNATURE: 12, HEAD_SIGNATURE: 12}        # signature -> where plen starts inside the section
MAX_HEAD_RECORDS = 16


def _section_signature(R):
    return PARITY_SIGNATURE if R == 1 else PARITY_RS_SIGNATURE


def seal_bands_bytes(n):
    """Bytes a band seal adds to a file of n bands per channel: the table and the 24 seal bytes."""
    return 20 + 12 * int(n) + SEAL_BYTES


class Seal(object):
    """band_len, band_crcs: None for a version-1 seal; for a band seal the finest record's band length and the (3, n) uint32 band CRCs.
    parity_group, parity: None but for a version-3 seal: G, and parity[c][g] the parity payload of group g of channel c (m = ceil(n / G)
    groups per channel; bytes, or views of the file split_seal read them from).
    parity_streams: None without parity, 1 for an 'L3CP' section, R = 2..4 for an 'L3CQ' section -- then parity[c][g] is the LIST of the
    group's R row payloads (rs_parity), all plen[c][g] bytes long.  rows(c, g): the group's row payloads as a list in either case.
    head: the HeadPart of an 'L3CH' section whose head_check holds, else None; head_damaged: True for an 'L3CH' section whose head part
    could not be read (such a file reads as the 'L3CQ' file it contains).  Neither takes part in ==: the seal is the same seal."""

    def __init__(self, generation, frame_crc, model_id, band_len=None, band_crcs=None, parity_group=None, parity=None, parity_streams=None,
                 head=None, head_damaged=False):
        self.head, self.head_damaged = head, bool(head_damaged)
        self.generation, self.frame_crc, self.model_id = int(generation), int(frame_crc), int(model_id)
        self.band_len = None if band_crcs is None else int(band_len)
        self.band_crcs = None if band_crcs is None else np.array(band_crcs, dtype=np.uint32).reshape(3, -1)
        self.parity_group = None if parity is None else int(parity_group)
        self.parity_streams = None if parity is None else int(parity_streams or 1)
        # the rows in ONE shape, [c][g][r]; `parity` in the documented one
        self._rows = None if parity is None else [[list(p) if isinstance(p, (list, tuple)) else [p] for p in row] for row in parity]
        self.parity = self._rows if parity is None or self.parity_streams > 1 else [[p[0] for p in row] for row in self._rows]

    @property
    def parity_groups(self):
        """m, the parity streams per channel; 0 without parity."""
        return 0 if self.parity is None else len(self.parity[0])

    def rows(self, c, g):
        """The parity_streams row payloads of group g of channel c, row 0 first."""
        return self._rows[c][g]

    def _key(self):
        key = (self.generation, self.frame_crc, self.model_id, self.band_len, None if self.band_crcs is None else self.band_crcs.tobytes())
        if self.parity is not None:
            key += (self.parity_group, self.parity_streams, tuple(bytes(p) for row in self._rows for rows in row for p in rows))
        return key

    def __eq__(self, other):
        return isinstance(other, Seal) and self._key() == other._key()

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def __repr__(self):
        bands = '' if self.band_crcs is None else ', band_len={}, band_crcs=<3 x {}>'.format(self.band_len, self.band_crcs.shape[1])
        if self.parity is not None:
            bands += ', parity_group={}, parity=<3 x {}>'.format(self.parity_group, self.parity_groups)
            if self.parity_streams > 1:
                bands += ', parity_streams={}'.format(self.parity_streams)
        return 'Seal(generation={}, frame_crc=0x{:08x}, model_id=0x{:016x}{})'.format(self.generation, self.frame_crc, self.model_id, bands)


class SealError(ValueError):
    """A sealed file that this decoder must not, or did not, decode to the pixels that were encoded.  reason: 'generation' (written by
    another bitstream generation), 'model' (by another checkpoint) -- both raised before anything is decoded --, 'pixels' (the decoded
    frame does not hash to the seal's CRC: a damaged payload, or a checkpoint the seal does not state).  index: the file's place in the call
    (the set readers: (entry, file), or the caller's key); failed: the places of ALL files known to have failed for that reason when the
    error was raised, in call order -- `index` is the first of them.
    bands, rows: None, except on the 'pixels' error of band-sealed files (check_band_crcs): bands = {file: [(channel, band), ...]} the
    bands whose pixels do not hash to their table word, rows = {file: (y0, y1)} their hull in rows of the UNPADDED image, None where they
    lie in the padding rows alone.  Every row outside the hull decoded to the sealed pixels."""

    def __init__(self, reason, index, message, failed=None, bands=None, rows=None):
        ValueError.__init__(self, message)
        self.reason, self.index = reason, index
        self.failed = [index] if failed is None else list(failed)
        self.bands, self.rows = bands, rows


class SalvageInfo(object):
    """What decode_salvage (Bitcoding, NativeCodec) returned for B files: which pixels are verified and which are estimates.
    concealed: {file: [(channel, band), ...]} the bands of band-sealed files whose decoded pixels did not hash to their table word, the
    pairs and order of SealError.bands; their pixels are the mixture's mean, conditioned on the channels of the same pixels that did
    verify (ops.dmll_conceal).  rows: {file: (y0, y1) or None} their hull in rows of the UNPADDED image (None: the padding rows alone), as
    SealError.rows; every row outside it is verified, exact.  lost: files of which NOTHING verified -- a band-sealed file with a failing
    channel in every band position (concealed all the same: its coarse records are as likely the cause), or a version-1 sealed file whose
    frame CRC fails (it cannot be localised: its pixels are left as decoded).  unverified: the unsealed files.  bands_total: {file: 3 n}
    for the band-sealed files; n_files: B."""

    FIELDS = ('concealed', 'rows', 'lost', 'unverified', 'bands_total', 'n_files')

    def __init__(self, concealed, rows, lost, unverified, bands_total, n_files):
        self.concealed, self.rows, self.lost, self.unverified = concealed, rows, list(lost), list(unverified)
        self.bands_total, self.n_files = bands_total, int(n_files)

    def as_dict(self):
        return {f: getattr(self, f) for f in self.FIELDS}

    def __eq__(self, other):
        return isinstance(other, SalvageInfo) and self.as_dict() == other.as_dict()

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def __repr__(self):
        return 'SalvageInfo({})'.format(', '.join('{}={!r}'.format(f, getattr(self, f)) for f in self.FIELDS))

    def line(self):
        """One line for people (l3c.py dec --salvage)."""
        tag = (lambda i: 'file {}: '.format(i)) if self.n_files > 1 else (lambda i: '')
        said = []
        for i in sorted(set(self.concealed) | set(self.lost)):
            if i in self.concealed:
                where = 'rows [{}, {})'.format(*self.rows[i]) if self.rows.get(i) else 'the padding rows'
                what = '{} concealed ({} of {} bands)'.format(where, len(self.concealed[i]), self.bands_total[i])
                what += (': LOST, no band position verified, every pixel is an estimate' if i in self.lost else ', every other row verified')
            else:
                what = 'LOST, the frame CRC fails and the seal has no band table to locate the damage: pixels as decoded, none verified'
            said.append(tag(i) + what)
        tail = '; not sealed: file(s) {}'.format(self.unverified) if self.unverified and self.n_files > 1 else ''
        if not said:
            return 'not sealed: nothing to verify' if len(self.unverified) == self.n_files else 'seal: ok' + tail
        return 'salvaged: ' + '; '.join(said) + tail


class RepairInfo(object):
    """What Bitcoding.decode_repair returned for B files.  repaired: {file: [(channel, band), ...]} the band payloads of the finest record
    that were rebuilt from the file's parity and whose band position then verified in all three channels: those pixels are the encoder's,
    bit for bit.  rows: {file: (y0, y1) or None} their hull in rows of the UNPADDED image (band_rows).  salvage: the SalvageInfo of what
    was left after the repair -- decode_salvage's own when nothing was repairable.  files: per file the healed file's bytes (the rebuilt
    payloads spliced in at their framing offsets; the same length, parity section, table and seal), None where nothing was repaired.
    rounds: the repair rounds that ran (0: no parity was uploaded, no XOR kernel launched).
    head: per file what heal_head did before the decode -- None for a file without an 'L3CH' section, else a HeadInfo -- (None: built by a
    caller that ran no heal_head); a file whose head was fixed is in `files` as well."""

    def __init__(self, repaired, rows, salvage, files, rounds=0, head=None):
        self.repaired, self.rows, self.salvage, self.files, self.rounds = repaired, rows, salvage, list(files), int(rounds)
        self.head = None if head is None else list(head)

    def __repr__(self):
        return 'RepairInfo(repaired={!r}, rows={!r}, rounds={}, healed files={}, salvage={!r})'.format(
            self.repaired, self.rows, self.rounds, [i for i, f in enumerate(self.files) if f is not None], self.salvage)

    def line(self):
        """One line for people (l3c.py dec --repair)."""
        if not self.repaired:
            return self.salvage.line()
        tag = (lambda i: 'file {}: '.format(i)) if self.salvage.n_files > 1 else (lambda i: '')
        said = []
        for i in sorted(self.repaired):
            where = 'rows [{}, {})'.format(*self.rows[i]) if self.rows.get(i) else 'the padding rows'
            k = len(self.repaired[i])
            said.append('{}{} restored ({} payload{})'.format(tag(i), where, k, '' if k == 1 else 's'))
        rest = self.salvage.line()
        if self.salvage.concealed or self.salvage.lost:
            return 'repaired: ' + '; '.join(said) + '; ' + rest
        tail = rest[len('seal: ok'):] if rest.startswith('seal: ok') else ''        # (the unsealed files of a mixed batch)
        return 'repaired: ' + '; '.join(said) + ', every row verified' + tail


def _padding_bytes(body):
    at = 6 if is_banded(body) else 0
    if len(body) < at + 8:
        raise ValueError('invalid file: seal on a file too short for its padding fields')
    return bytes(body[at:at + 8])


def is_sealed(data):
    """Whether the file ends with a seal of either version: at least 28 bytes, 'L3CS' 24 bytes before the end and the scale separator in
    front of it (every unsealed file of either format ends with that separator, and so does a band table).  A damaged seal still counts:
    split_seal raises for it."""
    return len(data) >= SEAL_BYTES + 4 and bytes(data[-24:-20]) == SEAL_SIGNATURE and bytes(data[-28:-24]) == _MAGIC_VALUE_SEP


_CRC_POLY = 0xEDB88320
_X8_TABLES = {}


def _x8_tables(nbytes):
    """ "Times x^(8 nbytes) mod P" as four 256-entry tables, one per byte of the other factor (CRC registers are reflected: bit 31 is
    x^0): a x^(8 nbytes) = t[0][a & 255] ^ t[1][a >> 8 & 255] ^ t[2][a >> 16 & 255] ^ t[3][a >> 24].  The arithmetic of csrc/crc_spans.h
    (mulmod, powmod); kept per length: the files of a call share two."""
    t = _X8_TABLES.get(nbytes)
    if t is not None:
        return t

    def mul(a, b):
        p = 0
        for i in range(31, -1, -1):
            if (a >> i) & 1:
                p ^= b
            b = (b >> 1) ^ (_CRC_POLY if b & 1 else 0)
        return p
    r, base, e = 0x80000000, 0x00800000, int(nbytes)          # 1, x^8
    while e:
        if e & 1:
            r = mul(r, base)
        base = mul(base, base)
        e >>= 1
    row = [0] * 32                                            # row[i]: what bit i of the other factor adds -- bit i is x^(31 - i)
    for i in range(31, -1, -1):
        row[i] = r
        r = (r >> 1) ^ (_CRC_POLY if r & 1 else 0)
    t = []
    for byte in range(4):
        tab = [0]
        for bit in range(8):
            tab += [v ^ row[8 * byte + bit] for v in tab]
        t.append(tab)
    if len(_X8_TABLES) >= 64:
        _X8_TABLES.clear()
    _X8_TABLES[nbytes] = t
    return t


def combine_band_crcs(crcs, L, HW):
    """zlib.crc32 of a planar frame [3][HW] from the CRCs of its bands, crcs (3, n) with n = ceil(HW / L): the frame is the concatenation
    of the bands in (channel, band) order, and crc(A | B) = crc(A) x^(8 |B|) + crc(B) over GF(2) (zlib's crc32_combine)."""
    crcs = np.asarray(crcs).astype(np.int64) & 0xffffffff
    n = n_bands(HW, L)
    if crcs.shape != (3, n):
        raise ValueError('combine_band_crcs: {} band CRCs for 3 x {} bands'.format(crcs.shape, n))
    words = crcs.tolist()
    (f0, f1, f2, f3), (l0, l1, l2, l3) = _x8_tables(int(L)), _x8_tables(int(HW - (n - 1) * L))
    a = 0
    for c in range(3):
        row = words[c]
        for j in range(n - 1):
            a = f0[a & 255] ^ f1[a >> 8 & 255] ^ f2[a >> 16 & 255] ^ f3[a >> 24] ^ row[j]
        a = l0[a & 255] ^ l1[a >> 8 & 255] ^ l2[a >> 16 & 255] ^ l3[a >> 24] ^ row[n - 1]
    return a


def _finest_header(body):
    """(C, H, W, L) of the last scale record of a banded file, walked by the length fields alone (csrc/seal.h: finest_record); None where
    the records do not end exactly with the data.  The parsers above do the full job later; this is what a seal's table is checked against."""
    found = _finest_record(body)
    return None if found is None else found[0]


def _finest_record(body):
    """_finest_header's walk -> ((C, H, W, L), the position of the record's first length field), or None."""
    end, p, found = len(body), 14, None
    if end < 14 or not is_banded(body):
        return None
    unpack = struct.unpack_from
    while p < end:
        if end - p < 9:
            return None
        C, H, W, L = unpack('<BHHI', body, p)
        p += 9
        if C == 0 or H * W == 0 or L == 0 or L % 64:
            return None
        n = n_bands(H * W, L)
        if n > MAX_BANDS:
            return None
        first = p
        for _ in range(C * n):
            if end - p < 4:
                return None
            p += 4 + unpack('<I', body, p)[0]
        if end - p < 4 or bytes(body[p:p + 4]) != _MAGIC_VALUE_SEP:
            return None
        p += 4
        found = ((C, H, W, L), first)
    return found


def parity_groups(n, G):
    """m = ceil(n / G): the parity streams per channel for n bands in groups of G; ValueError unless 1 <= G <= n."""
    n, G = int(n), int(G)
    if not 1 <= G <= n:
        raise ValueError('parity: the group size must be in 1..n = {}, got {}'.format(n, G))
    return -(-n // G)


def band_parity(payloads, G):
    """The parity payloads of ONE channel (the reference the kernels are tested against): payloads, the n band payloads of the channel
    (bytes-like, any lengths), in groups of G -> the m = ceil(n / G) parity payloads as bytes; group g is the XOR of the bands
    { j : j % m == g }, each zero-extended to the longest of them: rs_parity's row 0."""
    return [rows[0] for rows in rs_parity(payloads, G, 1)]


def parity_section_bytes(plens, R=1):
    """S of a parity section whose payload lengths are plens ((3, m)); R > 1: of the 'L3CQ' section with R rows per group."""
    plens = np.asarray(plens, dtype=np.int64).reshape(3, -1)
    return _SECTION_KINDS[_section_signature(R)] + 12 * plens.shape[1] + int(R) * int(plens.sum()) + 8


# ---- GF(2^8), polynomial 0x11D, alpha = 0x02: the arithmetic of the 'L3CQ' section (R parity rows per group; csrc/parity.hip on the device) ----

MAX_PARITY_STREAMS = 4
MAX_RS_GROUP = 255                  # the points alpha^k of a group's members must be distinct


def _gf_tables():
    exp, log, v = np.zeros(510, dtype=np.uint8), np.zeros(256, dtype=np.int64), 1
    for i in range(255):
        exp[i] = exp[i + 255] = v
        log[v] = i
        v <<= 1
        if v & 0x100:
            v ^= 0x11D
    return exp, log


_GF_EXP, _GF_LOG = _gf_tables()


def gf_mul(a, b):
    """a b in GF(2^8) mod 0x11D; a, b ints or uint8 arrays (broadcast)."""
    if np.isscalar(a) and np.isscalar(b):
        return 0 if a == 0 or b == 0 else int(_GF_EXP[_GF_LOG[a] + _GF_LOG[b]])
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    return np.where((a == 0) | (b == 0), np.uint8(0), _GF_EXP[_GF_LOG[a] + _GF_LOG[b]]).astype(np.uint8)


def gf_pow_alpha(e):
    """alpha^e, e >= 0."""
    return int(_GF_EXP[int(e) % 255])


def gf_inv(a):
    if a == 0:
        raise ZeroDivisionError('gf_inv(0)')
    return int(_GF_EXP[255 - _GF_LOG[a]])


def check_parity_streams(R, G, n):
    """R, the parity rows per group, for n bands in groups of G; ValueError unless R in 1..4 and, for R > 1, min(G, n) <= 255."""
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= R <= MAX_PARITY_STREAMS:
        raise ValueError('parity_streams must be in 1..{}, got {!r}'.format(MAX_PARITY_STREAMS, R))
    if R > 1 and min(int(G), int(n)) > MAX_RS_GROUP:
        raise ValueError('parity_streams > 1 needs groups of at most {} bands (distinct points in GF(2^8)), got min(G, n) = {}'.format(
            MAX_RS_GROUP, min(int(G), int(n))))
    return int(R)


def rs_parity(payloads, G, R):
    """The R parity rows per group of ONE channel (the reference the kernels are tested against): payloads, the n band payloads of the
    channel, in groups of G -> [m][R] bytes; row r of group g is the XOR over its members k (band g + k m) of alpha^(k r) d_k, each d_k
    zero-extended to the longest member.  Row 0 is band_parity's payload."""
    n = len(payloads)
    m = parity_groups(n, G)
    R = check_parity_streams(R, G, n)
    res = []
    for g in range(m):
        members = [np.frombuffer(bytes(p), dtype=np.uint8) for p in payloads[g::m]]
        rows = [np.zeros(max(len(a) for a in members), dtype=np.uint8) for _ in range(R)]
        for k, a in enumerate(members):
            for r in range(R):
                rows[r][:len(a)] ^= gf_mul(a, np.uint8(gf_pow_alpha(k * r)))
        res.append([row.tobytes() for row in rows])
    return res


def rs_repair_coefficients(erased_ks, present_ks, r0=0):
    """The erased members of a group from the parity rows r0 .. r0 + t - 1 (t = len(erased_ks)) and the present members: member k has
    the point x_k = alpha^k, row r = XOR_k x_k^r d_k, so  sum_e x_e^r d_e = P_r ^ sum_p x_p^r d_p  for the t rows; the t x t matrix
    (x_e^(r0 + i)) is a diagonal times a Vandermonde matrix and is inverted here.
    -> per erased member (in erased_ks' order) a pair (row coefficients [t], member coefficients [len(present_ks)]):
    d_e = XOR_i rows[i] P_(r0 + i)  ^  XOR_p members[p] d_p."""
    erased, present, t = [int(k) for k in erased_ks], [int(k) for k in present_ks], len(erased_ks)
    if t < 1 or len(set(erased)) != t or set(erased) & set(present) or any(not 0 <= k < MAX_RS_GROUP for k in erased + present):
        raise ValueError('rs_repair_coefficients: distinct members in 0..254, got erased {} and present {}'.format(erased, present))
    # Gauss-Jordan on [A | I], A[i][e] = x_e^(r0 + i)
    A = [[gf_pow_alpha(k * (r0 + i)) for k in erased] + [int(i == c) for c in range(t)] for i in range(t)]
    for col in range(t):
        piv = next((i for i in range(col, t) if A[i][col]), None)
        if piv is None:
            raise ValueError('rs_repair_coefficients: singular system for erased {} and rows {}..{}'.format(erased, r0, r0 + t - 1))
        A[col], A[piv] = A[piv], A[col]
        inv = gf_inv(A[col][col])
        A[col] = [gf_mul(inv, v) for v in A[col]]
        for i in range(t):
            if i != col and A[i][col]:
                f = A[i][col]
                A[i] = [v ^ gf_mul(f, w) for v, w in zip(A[i], A[col])]
    res = []
    for e in range(t):
        rows = A[e][t:]                                               # row e of the inverse: the weight of P_(r0 + i) in d_e
        members = []
        for k in present:
            w = 0
            for i in range(t):
                w ^= gf_mul(rows[i], gf_pow_alpha(k * (r0 + i)))
            members.append(w)
        res.append((rows, members))
    return res


def _band_lengths_of_finest(body, first, C, n):
    """The (C, n) length fields of the record whose first length field lies at `first` (as _finest_record found it)."""
    lens, p = np.zeros((C, n), dtype=np.int64), first
    for c in range(C):
        for j in range(n):
            lens[c, j], = struct.unpack_from('<I', body, p)
            p += 4 + int(lens[c, j])
    return lens


def head_from_body(body, G, R):
    """What make_seal(head=...) takes, from the numpy references: per head record of the banded file `body` (every record but the
    finest, coarsest first) a pair (crc (C, n) uint32: zlib.crc32 of every band payload, rows[c][g][r]: rs_parity(payloads of channel c,
    min(G, n), R))."""
    import zlib
    p, res = parse_banded(body), []
    for (C, H, W, L), off, nb in list(zip(p.scales, p.offset, p.nbytes))[:-1]:
        n = off.shape[1]
        payloads = [[bytes(body[int(off[c, j]):int(off[c, j] + nb[c, j])]) for j in range(n)] for c in range(C)]
        crc = np.array([[zlib.crc32(q) & 0xffffffff for q in row] for row in payloads], dtype=np.uint32).reshape(C, n)
        res.append((crc, [rs_parity(row, min(int(G), n), R) for row in payloads]))
    return res


def _head_part(body, G, R, head, framing=None):
    """The HEAD PART of an 'L3CH' section for the banded file `body`: the framing copy and head_crc from the body itself, the payload CRCs
    and rows from `head` (head_from_body's shape).  framing: (scales, nbytes) as parse_banded(body) has them, from a caller that holds them
    already (the encoder: walking the length fields of a file is a millisecond per thousand bands in Python)."""
    import zlib
    p = parse_banded(body) if framing is None else ParsedFraming(None, list(framing[0]), None, [np.asarray(nb, dtype=np.int64) for nb in framing[1]])
    if len(head) != len(p.scales) - 1:
        raise ValueError('make_seal: head needs one (crc, rows) pair per record but the finest, {} for {} records'.format(len(head), len(p.scales)))
    if len(p.scales) > MAX_HEAD_RECORDS:
        raise ValueError('make_seal: a head section holds at most {} records'.format(MAX_HEAD_RECORDS))
    meta, at = [struct.pack('<HH', len(p.scales), 0), bytes(body[:14])], 14
    for k, (header, nb) in enumerate(zip(p.scales, p.nbytes)):
        if k == len(p.scales) - 1:
            P0 = at
        meta += [struct.pack('<BHHI', *header), nb.astype('<u4').tobytes()]
        at += 9 + 4 * nb.size + int(nb.sum()) + 4
    if at != len(body):
        raise ValueError('make_seal: the framing given for the head adds up to {} bytes, the body has {}'.format(at, len(body)))
    meta.append(struct.pack('<I', zlib.crc32(memoryview(body)[:P0]) & 0xffffffff))
    rows_out = []
    for (C, H, W, L), nb, (crc, rows) in zip(p.scales, p.nbytes, head):
        n = nb.shape[1]
        Gk = min(int(G), n)
        m = parity_groups(n, Gk)
        crc = np.ascontiguousarray(np.asarray(crc).astype(np.int64) & 0xffffffff, dtype='<u4')
        if crc.shape != (C, n) or len(rows) != C or any(len(row) != m for row in rows) or \
                any(len(q) != R or len({len(r) for r in q}) != 1 for row in rows for q in row):
            raise ValueError('make_seal: head needs ({}, {}) payload CRCs and {} x {} x {} rows of one length per group for a record of {} x {} bands'
                             .format(C, n, C, m, R, C, n))
        hplen = np.array([[len(q[0]) for q in row] for row in rows], dtype='<u4')
        meta += [crc.tobytes(), struct.pack('<HH', Gk, m), hplen.tobytes()]
        rows_out += [bytes(r) for row in rows for q in row for r in q]
    meta = b''.join(meta)
    return meta + b''.join(rows_out) + struct.pack('<I', zlib.crc32(meta) & 0xffffffff)


def make_seal(body, generation, frame_crc, model_id=0, band_crcs=None, band_len=None, parity=None, head=None, head_framing=None):
    """The seal bytes for the unsealed file `body` (its padding fields go into the check word): 24 bytes, or with band_crcs ((3, n) words)
    and band_len (the finest record's) the band table and the version-2 seal, seal_bands_bytes(n) bytes.
    parity = (G, payloads) on top of a band seal, payloads[c][g] the parity payload of group g of channel c (band_parity per channel): the
    parity section in front of the table and the version-3 seal.  payloads[c][g] a LIST of R payloads of one length (rs_parity per channel):
    the 'L3CQ' section for R = 2..4; a list of one is written as the 'L3CP' section of its payload.
    head (needs parity): per head record of `body` (every record but the finest, coarsest first) a pair (crc (C, n) words of its band
    payloads, rows[c][g][r] = rs_parity(payloads of channel c, min(G, n), R)) -- head_from_body's shape: the 'L3CH' section, for every R in
    1..4; its framing copy and head_crc are taken from `body` (head_framing: the (scales, nbytes) of parse_banded(body), where the caller
    holds them already)."""
    import zlib
    table, section, checked = b'', b'', b''
    if head is not None and parity is None:
        raise ValueError('make_seal: head needs parity (the head rows use its G and R)')
    if parity is not None:
        if band_crcs is None:
            raise ValueError('make_seal: parity needs a band seal (band_crcs and band_len)')
        G, rows = parity
        n = np.asarray(band_crcs).reshape(3, -1).shape[1]
        m = parity_groups(n, G)
        if len(rows) != 3 or any(len(row) != m for row in rows):
            raise ValueError('make_seal: parity needs 3 x {} payloads for {} bands in groups of {}'.format(m, n, G))
        listed = isinstance(rows[0][0], (list, tuple))                             # rows[c][g]: a payload, or the list of R row payloads
        R = check_parity_streams(len(rows[0][0]) if listed else 1, G, n)
        if listed and any(not isinstance(p, (list, tuple)) or len(p) != R or len({len(q) for q in p}) != 1 for row in rows for p in row):
            raise ValueError('make_seal: parity needs {} row payloads of one length in every group'.format(R))
        rows = [[[bytes(q) for q in (p if listed else [p])] for p in row] for row in rows]                # [c][g][r]
        fields = (int(G), m) if R == 1 and head is None else (int(G), m, R, 0)
        front = (_section_signature(R) if head is None else HEAD_SIGNATURE) + struct.pack('<{}H'.format(len(fields)), *fields) + \
            b''.join(struct.pack('<I', len(p[0])) for row in rows for p in row)
        payload = b''.join(q for row in rows for p in row for q in p)
        if head is not None:
            payload += _head_part(body, int(G), R, head, head_framing)
        S = len(front) + len(payload) + 8
        if S >= 1 << 32:
            raise ValueError('make_seal: parity section of {} bytes'.format(S))
        tail = struct.pack('<I', S) + _MAGIC_VALUE_SEP
        section, checked = front + payload + tail, front + tail
    if band_crcs is not None:
        crcs = np.ascontiguousarray(np.asarray(band_crcs).astype(np.int64) & 0xffffffff, dtype='<u4').reshape(3, -1)
        n = crcs.shape[1]
        if not 1 <= n <= MAX_BANDS or band_len is None or int(band_len) <= 0:
            raise ValueError('make_seal: a band seal needs 1..{} bands per channel and their length, got {} and {}'.format(MAX_BANDS, n, band_len))
        if not is_banded(body):
            raise ValueError('make_seal: a band seal needs a banded file')
        T = 20 + 12 * n
        table = TABLE_SIGNATURE + struct.pack('<HHI', n, 0, int(band_len)) + crcs.tobytes() + struct.pack('<I', T) + _MAGIC_VALUE_SEP
    version = SEAL_VERSION_PARITY if section else SEAL_VERSION_BANDS if table else SEAL_VERSION
    seal20 = SEAL_SIGNATURE + struct.pack('<BBHIQ', version, 0, generation, frame_crc & 0xffffffff, model_id)
    return section + table + seal20 + struct.pack('<I', zlib.crc32(_padding_bytes(body) + checked + table + seal20) & 0xffffffff)


class _Tail(object):
    """What lies behind a sealed file's body, located from the file's end WITHOUT walking the body: the 24 seal bytes `s` and their
    fields, the band table (`table`, n), the parity section (section_at, S, signature, G, m, R, fields_at, plen) and `end`, where the body
    ends.  checked: the section bytes under the seal's check word."""


def _tail(data, heal=False):
    """The tail of a SEALED file (is_sealed) -> _Tail; raises what split_seal raises for a tail whose structure is broken.  The check
    word, the flags and everything that needs the body's records are split_seal's.  heal (heal_head): the file's signature and the
    separator the section starts behind -- the finest record's -- are not asked for: they are among the things heal_head restores."""
    t = _Tail()
    t.end, t.s = len(data) - SEAL_BYTES, bytes(data[-SEAL_BYTES:])
    t.version, t.flags, t.generation, t.frame_crc, t.model_id, t.check = struct.unpack('<BBHIQI', t.s[4:])
    if t.version not in (SEAL_VERSION, SEAL_VERSION_BANDS, SEAL_VERSION_PARITY):
        raise ValueError('invalid file: seal of an unknown version')
    t.table, t.checked, t.section_at, t.m, t.n, t.signature = b'', b'', None, 0, 0, None
    version, end = t.version, t.end
    if version != SEAL_VERSION:
        if not (heal or is_banded(data)):
            raise ValueError('invalid file: seal of an unknown version for a legacy file (version {}, needs a banded file)'.format(
                '2, the band seal' if version == SEAL_VERSION_BANDS else '3, the parity seal'))
        if end < 20 + 12 + 4:
            raise ValueError('invalid file: seal of an unknown version: {} needs a band table, and the file is too short for one'.format(version))
        T, = struct.unpack('<I', bytes(data[end - 8:end - 4]))
        n = (T - 20) // 12
        if T < 20 or (T - 20) % 12 or not 1 <= n <= MAX_BANDS:
            raise ValueError('invalid file: seal of an unknown version: {} needs a band table, and its length field is not 20 + 12 n with '
                             '1 <= n <= 1024'.format(version))
        if T > end - 14 - 4 or bytes(data[end - T - 4:end - T]) != _MAGIC_VALUE_SEP:
            raise ValueError("invalid file: seal band table does not start behind the file's last scale separator")
        t.table, end, t.n = bytes(data[end - T:end]), end - T, n
        if t.table[:4] != TABLE_SIGNATURE:
            raise ValueError("invalid file: seal band table without its 'L3CT' signature")
        if t.table[6:8] != b'\0\0':
            raise ValueError('invalid file: seal band table with a non-zero reserved field')
    if version == SEAL_VERSION_PARITY:
        S, = struct.unpack('<I', bytes(data[end - 8:end - 4]))           # (the separator at [end - 4, end) is the one the table starts behind)
        if S < parity_section_bytes([0, 0, 0]) or S > end - 14 - 4 or not (heal or bytes(data[end - S - 4:end - S]) == _MAGIC_VALUE_SEP):
            raise ValueError("invalid file: seal parity section does not start behind the file's last scale separator")
        section_at, end = end - S, end - S
        signature = bytes(data[section_at:section_at + 4])
        if signature not in _SECTION_KINDS:
            raise ValueError("invalid file: seal parity section without its 'L3CP' signature")
        G, m = struct.unpack('<HH', bytes(data[section_at + 4:section_at + 8]))
        fields_at, rs, hd, R = _SECTION_KINDS[signature], signature != PARITY_SIGNATURE, signature == HEAD_SIGNATURE, 1
        if m < 1 or fields_at + 8 + 12 * m > S:
            raise ValueError('invalid file: seal parity section is too short for its {} x 3 length fields'.format(m))
        if rs:
            R, reserved = struct.unpack('<HH', bytes(data[section_at + 8:section_at + 12]))
            if hd and not 1 <= R <= MAX_PARITY_STREAMS:
                raise ValueError("invalid file: seal parity section states {} parity streams, an 'L3CH' section holds 1..4".format(R))
            if not hd and not 2 <= R <= MAX_PARITY_STREAMS:
                raise ValueError("invalid file: seal parity section states {} parity streams, an 'L3CQ' section holds 2..4".format(R))
            if reserved:
                raise ValueError('invalid file: seal parity section with a non-zero reserved field')
        plen = np.frombuffer(bytes(data[section_at + fields_at:section_at + fields_at + 12 * m]), dtype='<u4').astype(np.int64).reshape(3, m)
        if hd and S < parity_section_bytes(plen, R):
            raise ValueError('invalid file: seal parity section length is less than 20 + 12 m + R times the sum of its payload lengths')
        if not hd and S != parity_section_bytes(plen, R):
            raise ValueError('invalid file: seal parity section length is not 20 + 12 m + R times the sum of its payload lengths' if rs else
                             'invalid file: seal parity section length is not 16 + 12 m + the sum of its payload lengths')
        t.checked = bytes(data[section_at:section_at + fields_at + 12 * m]) + bytes(data[section_at + S - 8:section_at + S])
        t.section_at, t.S, t.signature, t.G, t.m, t.R, t.fields_at, t.plen = section_at, S, signature, G, m, R, fields_at, plen
        t.head_at = section_at + fields_at + 12 * m + R * int(plen.sum())                   # A: the head part is file bytes [head_at, head_end)
        t.head_end = section_at + S - 8
    t.end = end
    return t


class HeadPart(object):
    """The head part of an 'L3CH' section whose head_check holds (Seal.head), as _parse_head read it.  records: every scale record's
    (C, H, W, L), coarsest first, the finest included; nbytes[k]: its (C, n_k) int64 length fields; file_header: the copy of body[0:14];
    head_crc; for every head record k (all but the finest) crcs[k] (C, n_k) uint32, groups[k] = (G_k, m_k), hplen[k] (C, m_k) int64 and
    rows[k][c][g][r], views of the file.  reserved, meta_bytes, size: what _check_head checks."""

    def positions(self, k):
        """Where record k lies in the body by the COPY's lengths -> (header position, (C, n) length field positions, the separator's)."""
        at = 14 + sum(9 + 4 * nb.size + int(nb.sum()) + 4 for nb in self.nbytes[:k])
        nb = self.nbytes[k]
        flat = nb.reshape(-1)
        fields = at + 9 + 4 * np.arange(flat.shape[0], dtype=np.int64) + np.cumsum(flat) - flat
        return at, fields.reshape(nb.shape), at + 9 + 4 * nb.size + int(nb.sum())


def _parse_head(hp, R):
    """The head part `hp` (a bytes-like view of section bytes [A, S - 8)) of a section with R rows per group -> HeadPart, or None where it
    cannot be walked -- a count or a header no writer produces, a field past its end -- or its head_check does not hold: damaged."""
    import zlib
    end, pos = len(hp) - 4, 4 + 14
    if pos > end:
        return None
    h = HeadPart()
    n_records, h.reserved = struct.unpack('<HH', bytes(hp[:4]))
    if not 1 <= n_records <= MAX_HEAD_RECORDS:
        return None
    h.file_header, h.records, h.nbytes = bytes(hp[4:18]), [], []
    for _ in range(n_records):
        if pos + 9 > end:
            return None
        C, H, W, L = struct.unpack('<BHHI', bytes(hp[pos:pos + 9]))
        if C == 0 or H * W == 0 or L == 0 or L % 64 or n_bands(H * W, L) > MAX_BANDS:
            return None
        n = n_bands(H * W, L)
        pos += 9
        if 4 * C * n > end - pos:
            return None
        h.records.append((C, H, W, L))
        h.nbytes.append(np.frombuffer(bytes(hp[pos:pos + 4 * C * n]), dtype='<u4').astype(np.int64).reshape(C, n))
        pos += 4 * C * n
    h.head_crc, = struct.unpack('<I', bytes(hp[pos:pos + 4]))
    pos += 4
    h.crcs, h.groups, h.hplen = [], [], []
    for (C, H, W, L), nb in zip(h.records[:-1], h.nbytes[:-1]):
        n = nb.shape[1]
        if 4 * C * n + 4 > end - pos:
            return None
        h.crcs.append(np.frombuffer(bytes(hp[pos:pos + 4 * C * n]), dtype='<u4').reshape(C, n))
        pos += 4 * C * n
        Gk, m = struct.unpack('<HH', bytes(hp[pos:pos + 4]))
        pos += 4
        if not 1 <= m <= n or 4 * C * m > end - pos:
            return None
        h.groups.append((Gk, m))
        h.hplen.append(np.frombuffer(bytes(hp[pos:pos + 4 * C * m]), dtype='<u4').astype(np.int64).reshape(C, m))
        pos += 4 * C * m
    if pos > end or zlib.crc32(bytes(hp[:pos])) & 0xffffffff != struct.unpack('<I', bytes(hp[end:end + 4]))[0]:
        return None
    h.meta_bytes, h.size = pos, len(hp)
    h.rows, view = [], memoryview(hp)
    if pos + R * sum(int(p.sum()) for p in h.hplen) == end:             # (else _check_head refuses the file)
        for (C, _, _, _), (_, m), hplen in zip(h.records, h.groups, h.hplen):
            rec = []
            for c in range(C):
                rec.append([])
                for g in range(m):
                    k = int(hplen[c, g])
                    rec[c].append([view[pos + r * k:pos + (r + 1) * k] for r in range(R)])
                    pos += R * k
            h.rows.append(rec)
    return h


def _check_head(h, body_bytes, G, R, n, L):
    """A head part whose head_check holds against itself, the band table (n, L) and the body's size: ValueError('invalid file: seal head
    ...') where they contradict one another (csrc/seal.h: check_head, the same checks in the same order)."""
    if h.reserved:
        raise ValueError('invalid file: seal head with a non-zero reserved field')
    if len(h.records) < 2:
        raise ValueError('invalid file: seal head states {} scale record(s)'.format(len(h.records)))
    if h.meta_bytes + R * sum(int(p.sum()) for p in h.hplen) + 4 != h.size:
        raise ValueError('invalid file: seal head length is not the one its fields add up to')
    C, H, W, Lf = h.records[-1]
    if C != 3 or n_bands(H * W, Lf) != n or Lf != L:
        raise ValueError('invalid file: seal head copy of the finest record does not match the band table')
    if 14 + sum(9 + 4 * nb.size + int(nb.sum()) + 4 for nb in h.nbytes) != body_bytes:
        raise ValueError('invalid file: seal head copy adds up to another body length')
    for nb, (Gk, m), hplen in zip(h.nbytes, h.groups, h.hplen):
        nk = nb.shape[1]
        if Gk != min(G, nk) or m != -(-nk // Gk):
            raise ValueError('invalid file: seal head states a group size or count that is not min(G, n) and ceil(n / G)')
        if any(int(hplen[c, g]) != int(nb[c, g::m].max()) for c in range(nb.shape[0]) for g in range(m)):
            raise ValueError("invalid file: seal head states a payload length that is not its longest member's")


def split_seal(data, view=False, head=None):
    """-> (body, Seal or None): the file without its seal (and band table), as the parsers above expect it.
    ValueError('invalid file: seal ...') for a recognised seal with an unknown version, non-zero flags or a wrong check word, and for a band
    seal whose table is not where its length field says, lacks its signature, has a non-zero reserved field, sits on a legacy file, states
    another n or L than the finest record's header, or whose frame CRC is not the combination of its band CRCs: never silently treated as
    absent.  view=True: the body of a sealed file is a memoryview of `data`, not a copy (the decoders: a copy of every file is a
    millisecond per 10 MB on the host, more than the hash costs on the device); everything above reads either.
    An 'L3CH' section (head parity) reads as the 'L3CQ' section it contains, R = 1 included; Seal.head is its head part, or None with
    Seal.head_damaged where that part is damaged -- never an error.  A head part that is intact but contradicts itself, the table or the body's
    size is ValueError('invalid file: seal head ...').  head: the HeadPart heal_head has read and checked in this very file (HeadInfo.part):
    it is taken as it is, not read and checked a second time."""
    import zlib
    if not is_sealed(data):
        return data, None
    t = _tail(data)
    s, table, end, n, section_at, generation, frame_crc, model_id = t.s, t.table, t.end, t.n, t.section_at, t.generation, t.frame_crc, t.model_id
    if t.flags:
        raise ValueError('invalid file: seal with non-zero flags')
    body = (memoryview(data) if view else data)[:end]
    if t.check != zlib.crc32(_padding_bytes(body) + t.checked + table + s[:20]) & 0xffffffff:
        raise ValueError('invalid file: seal check word does not match (damaged seal or padding fields)')
    if not table:
        return body, Seal(generation, frame_crc, model_id)
    n_stated, _, L = struct.unpack('<HHI', table[4:12])
    if n_stated != n:
        raise ValueError('invalid file: seal band table states another band count than its length')
    finest, first = _finest_record(body) or (None, None)
    if finest is None or finest[3] != L or n_bands(finest[1] * finest[2], L) != n:
        raise ValueError("invalid file: seal band table does not match the bands of the file's finest scale record")
    crcs = np.frombuffer(table[12:12 + 12 * n], dtype='<u4').reshape(3, n)
    if combine_band_crcs(crcs, L, finest[1] * finest[2]) != frame_crc:
        raise ValueError('invalid file: seal frame CRC is not the combination of its band CRCs')
    if section_at is None:
        return body, Seal(generation, frame_crc, model_id, L, crcs)
    G, m, R, plen, fields_at = t.G, t.m, t.R, t.plen, t.fields_at
    if finest[0] != 3 or not 1 <= G <= n or m != -(-n // G):
        raise ValueError("invalid file: seal parity section does not match the bands of the file's finest scale record")
    if R > 1 and G > MAX_RS_GROUP:
        raise ValueError('invalid file: seal parity section with more than one stream over groups of more than 255 bands')
    lens = _band_lengths_of_finest(body, first, 3, n)
    if any(int(plen[c, g]) != int(lens[c, g::m].max()) for c in range(3) for g in range(m)):
        raise ValueError("invalid file: seal parity section states a payload length that is not its longest member's")
    view, at, rows = memoryview(data), section_at + fields_at + 12 * m, []
    for c in range(3):
        rows.append([])
        for g in range(m):
            k = int(plen[c, g])
            rows[c].append([view[at + r * k:at + (r + 1) * k] for r in range(R)])
            at += R * k
    is_head = t.signature == HEAD_SIGNATURE
    if not is_head:
        head = None
    elif head is None:
        head = _parse_head(view[t.head_at:t.head_end], R)
        if head is not None:
            _check_head(head, end, G, R, n, L)
    return body, Seal(generation, frame_crc, model_id, L, crcs, G, rows, R, head=head, head_damaged=is_head and head is None)


class HeadInfo(object):
    """What heal_head did to one file with an 'L3CH' section.  framing_fixed: the framing fields rewritten from the section's copy (the
    file header's first 6 bytes, each of the 4 padding fields, each record header, length field and separator count as one field),
    framing: the same by kind; repaired, failed: [(record, channel, band)] the payloads of the coarser records (record 0: the coarsest) that
    did not hash to their CRC and were / were not rebuilt from the head rows; section_damaged: the head part itself is damaged (its
    head_check fails): nothing was checked, nothing done.  part: the HeadPart as heal_head read and checked it (None where damaged), for
    the split_seal that follows."""

    KINDS = ('file header', 'padding field', 'record header', 'length field', 'separator')

    def __init__(self, framing=None, repaired=(), failed=(), section_damaged=False, part=None):
        self.part = part
        self.framing = dict(framing or {})
        self.framing_fixed = sum(self.framing.values())
        self.repaired, self.failed, self.section_damaged = list(repaired), list(failed), bool(section_damaged)

    def __bool__(self):
        return bool(self.framing_fixed or self.repaired or self.failed or self.section_damaged)

    __nonzero__ = __bool__

    def __repr__(self):
        return 'HeadInfo(framing_fixed={}, repaired={!r}, failed={!r}, section_damaged={})'.format(
            self.framing_fixed, self.repaired, self.failed, self.section_damaged)

    def line(self):
        """One line for people (l3c.py dec --repair), e.g. 'head: 2 length fields and 1 coarse payload restored'."""
        if self.section_damaged:
            return 'head: the head section is damaged, nothing of the head could be checked'
        plural = lambda k, what: '{} {}{}'.format(k, what, '' if k == 1 else 's')                    # noqa: E731
        done = [plural(self.framing[kind], kind) for kind in self.KINDS if self.framing.get(kind)]
        if self.repaired:
            done.append(plural(len(self.repaired), 'coarse payload'))
        said = ', '.join(done[:-1]) + (' and ' if len(done) > 1 else '') + done[-1] + ' restored' if done else ''
        if self.failed:
            said += ('; ' if said else '') + plural(len(self.failed), 'coarse payload') + ' NOT restored (record, channel, band) {}'.format(self.failed[:6])
        return 'head: ' + (said or 'ok')


def heal_head(data):
    """The pre-pass of Bitcoding.decode_repair: -> (data', HeadInfo or None).  None: the file has no 'L3CH' section (or its seal is damaged
    where the check word covers it: split_seal then raises as ever).  The tail is found from the file's END and the body is never walked by
    its own length fields: every position comes from the section's framing copy.
    Fast path: head_crc matches body[0:P0) and the finest record's header, length fields and separator equal the copy -> `data` itself,
    nothing copied, no payload hashed.  Slow path: every framing byte that differs from the copy is rewritten (file header, padding
    fields, record headers, length fields, separators), then every payload of the coarser records is hashed against its CRC; the failures
    of a group (record, c, g) are its erasures: t = 1..R of them are rebuilt from the head rows r0 .. r0 + t - 1 and the present members
    (rs_repair_coefficients), r0 = 0 first, later windows while a rebuilt payload still fails its CRC -- the CRC is the arbiter.  data' is
    then a new bytes object of the same length, section, table and seal.  Band payloads of the finest record are not touched: they are
    decode_repair's.  A file whose length changed, or whose table, seal or checked section header is damaged, is not healed."""
    import zlib
    if not is_sealed(data):
        return data, None
    try:
        t = _tail(data, heal=True)
    except ValueError:
        return data, None                                     # (split_seal raises the same error to the caller)
    if t.signature != HEAD_SIGNATURE:
        return data, None
    R = t.R
    h = _parse_head(memoryview(data)[t.head_at:t.head_end], R)
    if h is None:
        return data, HeadInfo(section_damaged=True)
    # the seal's check word with the COPY's padding fields: a failure is damage to the table, the seal or the section's checked header
    if t.flags or t.check != zlib.crc32(h.file_header[6:14] + t.checked + t.table + t.s[:20]) & 0xffffffff:
        return data, None
    n_stated, _, L = struct.unpack('<HHI', t.table[4:12])
    if n_stated != t.n or not 1 <= t.G <= t.n or t.m != -(-t.n // t.G):
        return data, None                                     # (a table or section that split_seal refuses)
    _check_head(h, t.end, t.G, R, t.n, L)
    K = len(h.records) - 1
    P0, fields0, sep0 = h.positions(K)
    arr = np.frombuffer(data, dtype=np.uint8)
    want = h.nbytes[K].astype('<u4').reshape(-1).view(np.uint8).reshape(-1, 4)
    if zlib.crc32(memoryview(data)[:P0]) & 0xffffffff == h.head_crc and bytes(data[P0:P0 + 9]) == struct.pack('<BHHI', *h.records[K]) and \
            bytes(data[sep0:sep0 + 4]) == _MAGIC_VALUE_SEP and np.array_equal(arr[fields0.reshape(-1, 1) + np.arange(4)], want):
        return data, HeadInfo(part=h)
    buf, framing = bytearray(data), {}

    def restore(kind, at, good):
        if buf[at:at + len(good)] != good:
            buf[at:at + len(good)] = good
            framing[kind] = framing.get(kind, 0) + 1
    restore('file header', 0, h.file_header[:6])
    for i in range(4):
        restore('padding field', 6 + 2 * i, h.file_header[6 + 2 * i:8 + 2 * i])
    where = []
    for k in range(K + 1):
        at, fields, sep = h.positions(k)
        restore('record header', at, struct.pack('<BHHI', *h.records[k]))
        for f, nb in zip(fields.reshape(-1).tolist(), h.nbytes[k].reshape(-1).tolist()):
            restore('length field', f, struct.pack('<I', nb))
        restore('separator', sep, _MAGIC_VALUE_SEP)
        where.append(fields + 4)
    repaired, failed, mv = [], [], memoryview(buf)
    for k in range(K):
        C, n = h.nbytes[k].shape
        m = h.groups[k][1]
        payload = lambda c, j: mv[int(where[k][c, j]):int(where[k][c, j] + h.nbytes[k][c, j])]      # noqa: E731
        for c in range(C):
            bad = [j for j in range(n) if zlib.crc32(payload(c, j)) & 0xffffffff != int(h.crcs[k][c, j])]
            for g in sorted({j % m for j in bad}):
                erased = [j // m for j in bad if j % m == g]
                members, size, fixed = list(range(g, n, m)), int(h.hplen[k][c, g]), None
                for r0 in range(R - len(erased) + 1):                    # (no window at all for more than R erasures)
                    fixed = _rebuild_members(erased, members, m, r0, size, h.rows[k][c][g], payload, c, h.nbytes[k][c], h.crcs[k][c])
                    if fixed is not None:
                        break
                if fixed is None:
                    failed += [(k, c, g + e * m) for e in erased]
                    continue
                for e, got in zip(erased, fixed):
                    j = g + e * m
                    buf[int(where[k][c, j]):int(where[k][c, j]) + len(got)] = got
                    repaired.append((k, c, j))
    del mv
    return bytes(buf), HeadInfo(framing, repaired, failed, part=h)


def _rebuild_members(erased, members, m, r0, size, rows, payload, c, nbytes, crcs):
    """The erased members (indices k: band members[k]) of one group from its rows r0 .. r0 + t - 1 and its present members, on the host
    -> the rebuilt payloads in erased's order, or None when one of them does not hash to its CRC.  size: the rows' length."""
    import zlib
    present = [k for k in range(len(members)) if k not in erased]

    def extended(p):
        a = np.zeros(size, dtype=np.uint8)
        a[:len(p)] = np.frombuffer(p, dtype=np.uint8)
        return a
    have, parity, res = [extended(payload(c, members[k])) for k in present], [extended(rows[r0 + i]) for i in range(len(erased))], []
    for e, (row_coefs, member_coefs) in zip(erased, rs_repair_coefficients(erased, present, r0)):
        d = np.zeros(size, dtype=np.uint8)
        for a, w in list(zip(parity, row_coefs)) + list(zip(have, member_coefs)):
            if w:
                d ^= gf_mul(a, np.uint8(w))
        got = d[:int(nbytes[members[e]])].tobytes()
        if zlib.crc32(got) & 0xffffffff != int(crcs[members[e]]):
            return None
        res.append(got)
    return res


def band_rows(j, L, frame_hw, padding):
    """Rows [y0, y1) of the UNPADDED image that bands j (an int or a sequence) of length L of an H x W frame touch: their hull, or None when
    they lie in the padding rows alone.  padding: (left, right, top, bottom)."""
    H, W = frame_hw
    js = [int(j)] if np.isscalar(j) else [int(v) for v in j]
    top, bottom = int(padding[2]), int(padding[3])
    r0 = min(js) * L // W
    r1 = -(-min((max(js) + 1) * L, H * W) // W)
    y0, y1 = max(r0 - top, 0), min(r1 - top, H - top - bottom)
    return (y0, y1) if y0 < y1 else None


def failing_bands(seals, words, frame_hw, paddings, first_band=0, frame_words=None):
    """After the decode: the band CRCs of the decoded pixels against the tables, WITHOUT raising (decode_salvage; check_band_crcs raises on
    the same findings).  seals: per file a Seal or None; words[i]: the (3, m) CRC words of bands first_band .. first_band + m - 1 of
    decoded frame i (a full decode: all n; a region decode: the bands it decoded), ignored for files without a band seal; frame_hw: the
    padded (H, W); paddings: per file (left, right, top, bottom).  frame_words: the frame CRCs of the decoded frames, compared with the
    version-1 seals of the same call (None: those are not checked here).
    -> (failed, bands, rows): the files that failed, in call order; bands = {file: [(channel, band), ...]} and rows = {file: (y0, y1) or
    None} for the band-sealed ones among them (SealError.bands, .rows)."""
    failed, bands, rows = [], {}, {}
    words = (np.asarray(words).astype(np.int64) & 0xffffffff).astype(np.uint32)      # int32 or uint32 words, all files at once
    for i, s in enumerate(seals):
        if s is None:
            continue
        if s.band_crcs is None:
            if frame_words is not None and (int(frame_words[i]) & 0xffffffff) != s.frame_crc:
                failed.append(i)
            continue
        got = words[i]
        want = s.band_crcs[:, first_band:first_band + got.shape[1]]
        if got.shape != want.shape:
            raise ValueError('check_band_crcs: file {}: {} words for bands {}.. of a 3 x {} table'.format(i, got.shape, first_band, s.band_crcs.shape[1]))
        if np.array_equal(got, want):
            continue
        bad = [(int(c), int(first_band + j)) for c, j in zip(*np.nonzero(got != want))]
        if bad:
            failed.append(i)
            bands[i] = bad
            rows[i] = band_rows(sorted({j for _, j in bad}), s.band_len, frame_hw, paddings[i])
    return failed, bands, rows


def check_band_crcs(seals, words, frame_hw, paddings, first_band=0, frame_words=None):
    """failing_bands, raising: SealError('pixels') names the first failing file, lists all, and carries .bands and .rows for the
    band-sealed ones."""
    failed, bands, rows = failing_bands(seals, words, frame_hw, paddings, first_band, frame_words)
    if failed:
        i = failed[0]
        if i in bands:
            where = 'rows [{}, {})'.format(*rows[i]) if rows[i] else 'the padding rows'
            msg = ('file {} decoded to pixels that do not hash to its band CRCs in {} band(s) (channel, band) {}: {} of the image are damaged (a '
                   'damaged payload, or not the checkpoint that wrote it); every other row is verified'.format(
                       i, len(bands[i]), bands[i][:6] + (['...'] if len(bands[i]) > 6 else []), where))
        else:
            msg = ('file {} decoded to pixels whose CRC-32 {:08x} is not the sealed {:08x}: damaged payload, or not the checkpoint that wrote '
                   'it'.format(i, int(frame_words[i]) & 0xffffffff, seals[i].frame_crc))
        raise SealError('pixels', i, msg, failed, bands or None, rows or None)


def check_seals(seals, generation, model_id):
    """What a decoder checks BEFORE it decodes: every seal's generation, then its model id where both sides state one.  seals: per file a
    Seal or None; model_id: a callable (the id is only computed when a seal asks for it) or an int."""
    for i, s in enumerate(seals):
        if s is not None and s.generation != generation:
            raise SealError('generation', i, 'file {} was written by bitstream generation {}, this decoder is generation {}: it would decode '
                            'to wrong pixels'.format(i, s.generation, generation))
    for i, s in enumerate(seals):
        if s is not None and s.model_id:
            mine = model_id() if callable(model_id) else model_id
            if mine and mine != s.model_id:
                raise SealError('model', i, 'file {} was written with checkpoint {:016x}, this decoder holds {:016x}: it would decode to wrong '
                                'pixels'.format(i, s.model_id, mine))


def check_frame_crcs(seals, crcs):
    """After the decode: crcs[i] (the CRC-32 of decoded frame i) against seal i.  The error names the first failing file and lists all."""
    failed = [i for i, s in enumerate(seals) if s is not None and (int(crcs[i]) & 0xffffffff) != s.frame_crc]
    if failed:
        i = failed[0]
        raise SealError('pixels', i, 'file {} decoded to pixels whose CRC-32 {:08x} is not the sealed {:08x}: damaged payload, or not the '
                        'checkpoint that wrote it'.format(i, int(crcs[i]) & 0xffffffff, seals[i].frame_crc), failed)
