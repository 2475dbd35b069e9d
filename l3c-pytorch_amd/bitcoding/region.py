"""Region decode, the host side (no torch, no library call): which bands, symbols and convolution rows a ROW WINDOW of a frame needs.

Only the finest scale record of a file is windowed (Bitcoding.decode_region); it is ~95 % of the bytes.  Its P is a local function of z1 and
the coarser decoder's features: in exact arithmetic a row of P needs `halo_rows` rows of them on either side, none at a true image border.
A file decodes only where P is reproduced BIT FOR BIT, and that asks for more: the window is cut where every kept value keeps its place in
the kernels' tilings -- its first row is a multiple of GRANULE full-resolution rows (the Winograd kernel's 16 x 16 tiles on the sub-grids of
the dilation-4 branch: 64 rows; 32 at half resolution), its last row another one or the frame's end -- and the decoder stage runs on an
APRON beyond the window's cut edges, because a Winograd tile's rounding depends on all of its input rows (apron_rows).

All rows here are FRAME rows: rows of the padded image a file holds, full resolution."""
from collections import namedtuple

import numpy as np

GRANULE = 64

RegionPlan = namedtuple('RegionPlan', ['bands', 'sym_rows', 'conv_rows', 'valid_rows', 'hw', 'pix0', 'length'])
RegionPlan.__doc__ = """What rows [y0, y1) of an H x W frame need of its finest record:
  bands       (j0, j1)   the bands that hold a pixel of the rows
  sym_rows    (p0, p1)   rows the range decoder produces symbols in: from the first band's first pixel to the last needed one
  conv_rows   (c0, c1)   rows the convolutions run on (the window "image"): sym_rows + halo, widened to the granule, clipped to the frame
  valid_rows  (v0, v1)   rows of the window whose P equals the full frame's: conv_rows less the halo at every cut edge
  hw                     pixels of the window image, (c1 - c0) W
  pix0, length           int64 arrays, one row per band: the entry's first pixel inside the window image, and its symbols"""


def halo_rows(config_ms):
    """Full-resolution rows of z1 / F1 context a row of the RGB scale's P needs on either side: the 2 num_blocks + 1 body convs and the `up`
    conv of the decoder at half resolution (a row each, two full-resolution rows), then the dilation-4 branch of the classifier (four)."""
    return 2 * (2 * int(config_ms.dec.num_blocks) + 2) + 4


def apron_rows(config_ms, granule=GRANULE):
    """Full-resolution rows the DECODER stage of the windowed step (MultiscaleNetwork.get_P_rows) runs on beyond every cut edge of the
    conv rows, so that its output is the frame's BIT FOR BIT on the conv rows themselves.  The halo above is what a row needs in exact
    arithmetic.  The Winograd kernel computes every 4 x 4 output tile from a 6 x 6 input tile, and every one of the 36 inputs takes part in
    the rounding of every output: a row that differs anywhere in a tile's input changes the last bits of all four rows of the tile.  A
    difference therefore spreads FOUR rows per 3x3 layer, not one: 4 (2 num_blocks + 2) half-resolution rows through the decoder (72 for
    cr.cf), rounded up to the granule (96, 192 full-resolution rows).  Measured, not only derived: with the 18-row halo alone the first
    layer whose kept rows differ is the eleventh (tests/test_gpu_region.py).  The classifier's three branches then spread 4, 8 and 16
    full-resolution rows (a tile of the dilation-d sub-grid is 4 d rows), which the 40-row halo covers."""
    half = 4 * (2 * int(config_ms.dec.num_blocks) + 2)
    return 2 * (-(-half // (granule // 2)) * (granule // 2))


def decoder_rows(H, conv_rows, apron):
    """Rows [a0, a1) (full resolution, even) the decoder stage runs on for conv rows (c0, c1) of a frame of H rows: the apron beyond every
    cut edge, clipped to the frame."""
    c0, c1 = conv_rows
    return max(0, c0 - apron), min(int(H), c1 + apron)


def parse_box(box, padding, frame_hw):
    """A box (y0, y1) or (y0, y1, x0, x1) in the coordinates of the UNPADDED image -> ((y0, y1), (x0, x1)) in frame coordinates.
    padding: the file's (left, right, top, bottom); ValueError for an empty box or one that leaves the image."""
    left, right, top, bottom = padding
    H, W = frame_hw[0] - top - bottom, frame_hw[1] - left - right
    try:
        box = tuple(int(v) for v in box)
    except (TypeError, ValueError):
        raise ValueError('box must be (y0, y1) or (y0, y1, x0, x1), got {!r}'.format(box))
    if len(box) not in (2, 4):
        raise ValueError('box must be (y0, y1) or (y0, y1, x0, x1), got {!r}'.format(box))
    y0, y1 = box[:2]
    x0, x1 = box[2:] if len(box) == 4 else (0, W)
    if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
        raise ValueError('box rows [{}, {}) x columns [{}, {}) is empty or not inside the {}x{} image'.format(y0, y1, x0, x1, H, W))
    return (top + y0, top + y1), (left + x0, left + x1)


def shared_padding(paddings):
    """The one padding tuple of a batch; ValueError when the files disagree (a box means different frame rows in each of them then)."""
    first = tuple(int(v) for v in paddings[0])
    for p in paddings[1:]:
        if tuple(int(v) for v in p) != first:
            raise ValueError('decode_region needs files of one padding tuple, got {} and {}'.format(first, tuple(int(v) for v in p)))
    return first


def region_plan(H, W, L, rows, halo, granule=GRANULE, cut=True):
    """The plan for rows = (y0, y1), 0 <= y0 < y1 <= H, of ONE H x W frame whose finest record has bands of L symbols (L = H W: a legacy
    file, one band).  cut: the last band's entry ends with the last pixel of row y1 - 1 (the range decoder stops there); False: it is
    decoded whole."""
    H, W, L, halo, G = int(H), int(W), int(L), int(halo), int(granule)
    y0, y1 = (int(v) for v in rows)
    if not (H > 0 and W > 0 and L > 0 and halo >= 0 and G > 0):
        raise ValueError('bad frame: H={}, W={}, L={}, halo={}, granule={}'.format(H, W, L, halo, G))
    if not 0 <= y0 < y1 <= H:
        raise ValueError('rows [{}, {}) are empty or not inside the {} frame rows'.format(y0, y1, H))
    HW = H * W
    j0, j1 = (y0 * W) // L, -(-(y1 * W) // L)
    p0 = (j0 * L) // W
    p1 = y1 if cut else -(-min(j1 * L, HW) // W)
    c0 = max(0, (p0 - halo) // G * G)
    c1 = min(H, -(-(p1 + halo) // G) * G)
    v0 = 0 if c0 == 0 else c0 + halo
    v1 = H if c1 == H else c1 - halo
    assert v0 <= p0 and p1 <= v1, (v0, p0, p1, v1)
    j = np.arange(j0, j1, dtype=np.int64)
    end = np.minimum((j + 1) * L, HW)
    if cut:
        end = np.minimum(end, p1 * W)
    return RegionPlan((j0, j1), (p0, p1), (c0, c1), (v0, v1), (c1 - c0) * W, j * L - c0 * W, end - j * L)


def entry_table(plan, B):
    """(pixbase, hw, pix0, length) of ops.decode_rgb_entries for B frames of one plan, their window images back to back: B (j1 - j0) entries in
    the order (image, band)."""
    n = plan.pix0.shape[0]
    return (np.repeat(np.arange(B, dtype=np.int64), n) * plan.hw, np.full(B * n, plan.hw, dtype=np.int64), np.tile(plan.pix0, B),
            np.tile(plan.length, B))


class RegionInfo(object):
    """What Bitcoding.decode_region did for a box.  bands / sym_rows / conv_rows / valid_rows: the plan (frame rows); decoder_rows: the rows
    the decoder stage of the windowed step ran on (conv_rows plus the apron; at half resolution); n_bands, frame_rows: the
    record's bands per channel and the frame's rows; streams_used / streams_total and bytes_used / bytes_total: the band streams of the finest
    record the range decoder read, and their payload bytes, of all the record holds (summed over the batch; the coarser records are decoded
    whole and are not counted); verified: the seal fields that were checked ('generation', 'model'), empty for unsealed files or verify=False;
    ('bands' too where the decoded bands were hashed); pixel_crc_checked: True when every sealed file of the call is BAND-SEALED and the
    bands the call decoded hashed to their table words (Bitcoding.decode_region, verify=True); False otherwise -- a version-1 seal's CRC
    covers the whole frame."""

    FIELDS = ('box', 'bands', 'n_bands', 'sym_rows', 'conv_rows', 'valid_rows', 'decoder_rows', 'frame_rows', 'streams_used', 'streams_total', 'bytes_used',
              'bytes_total', 'sealed', 'verified', 'pixel_crc_checked')

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw[f])

    def as_dict(self):
        return {f: getattr(self, f) for f in self.FIELDS}

    def __repr__(self):
        return 'RegionInfo({})'.format(', '.join('{}={!r}'.format(f, getattr(self, f)) for f in self.FIELDS))

    def line(self):
        """One line for people (l3c.py dec --region)."""
        if self.sealed and self.pixel_crc_checked:
            seal = 'band-sealed: generation and model checked, the CRCs of bands {}..{} of every channel checked: every decoded pixel is verified'.format(
                self.bands[0], self.bands[1] - 1)
        else:
            seal = ('sealed: {} checked, pixel CRC not checked (it covers the whole frame)'.format(
                ' and '.join(v for v in self.verified if v != 'bands') or 'nothing') if self.sealed else 'not sealed')
        return ('region rows [{}, {}) x columns [{}, {}): bands {}..{} of {}, symbol rows {}..{}, conv rows {}..{} and decoder rows {}..{} '
                'of {}, {} of {} streams, {} of {} payload bytes of the finest record; {}'.format(
                    self.box[0], self.box[1], self.box[2], self.box[3], self.bands[0], self.bands[1] - 1, self.n_bands, self.sym_rows[0],
                    self.sym_rows[1] - 1, self.conv_rows[0], self.conv_rows[1] - 1, self.decoder_rows[0], self.decoder_rows[1] - 1,
                    self.frame_rows, self.streams_used, self.streams_total, self.bytes_used, self.bytes_total, seal))
