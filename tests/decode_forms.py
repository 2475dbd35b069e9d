"""The shapes of the decoder's NON-RECTANGULAR launches, named in one place (as tests/ref64.py names the value regimes of the head), and
seeded builders of their inputs.  No GPU: tests/test_decode_forms_cases.py checks that every edge listed below is really in these
tables; tests/test_gpu_table_forms.py and tests/test_gpu_decode_forms.py run the kernels over them.

Three launch forms (include/l3c_hip.h):
  grouped   l3c_dmll_cdf_table_parts: up to 8 parts (channel, pixel range) of ONE rectangular batch in one launch;
  ragged    l3c_dmll_cdf_table_ragged / l3c_ac_decode_chunks with the r_* fields: per image (or ENTRY) its own pixbase, size, range and
            table offset;
  entries   l3c_decode_rgb_entries: every entry cut into the same NUMBER of chunks, the trailing chunks of a short entry empty.

Everything ragged is laid out as the C ABI wants it: P (total_pix, Kp) with image i's pixels from pixel pixbase[i] on, the symbols as
int16 (C * total_pix,) with image i's C planes of hw[i] symbols from element C * pixbase[i] on.  A rectangular batch is the special
case pixbase[i] = i * HW, so one data model serves the four RGB pipelines.
"""
import numpy as np

from tests import ref64

K = 10
TABLE_PIX = 32          # csrc/dmll_kernels.hip: kTablePix, pixels per block of the table kernel
BLOCK = 64              # symbols per store block of the decoders: chunk boundaries lie on multiples of it
WIN_LP = 65             # entries of a window row (csrc/dmll_core.h: kWinLp)
WIN_BAD = 0x40000000    # statistics word: more than 1/64 of the chunk missed -> full rows
SENTINEL = -7           # guard symbols (not -1: the decoders' own marker for a stream that left the fast path)
RANGE_LENGTHS = (1, TABLE_PIX - 1, TABLE_PIX, TABLE_PIX + 1, 2 * TABLE_PIX, 3 * TABLE_PIX - 1)


def lp_of(rgb):
    return ref64.alphabet(rgb)[2] + 1


class EntryCase(object):
    """Images (hw, pixbase) inside a buffer of total_pix pixels and entries (image, pix0, len) over them.
    kinds: per image how the RGB builder fills it -- ('near', far ranges) or ('coupled', ())."""

    def __init__(self, name, hw, pixbase, total_pix, entries, kinds=None):
        self.name = name
        self.hw = np.asarray(hw, dtype=np.int64)
        self.pixbase = np.asarray(pixbase, dtype=np.int64)
        self.total_pix = int(total_pix)
        self.entries = [tuple(int(v) for v in e) for e in entries]
        self.kinds = kinds

    @property
    def S(self):
        return len(self.entries)

    def table(self):
        """-> (pixbase, hw, pix0, len) int64 arrays of S: the entry table of ops.decode_z_entries / ops.decode_rgb_entries."""
        img = np.array([e[0] for e in self.entries], dtype=np.int64)
        return (self.pixbase[img], self.hw[img], np.array([e[1] for e in self.entries], dtype=np.int64),
                np.array([e[2] for e in self.entries], dtype=np.int64))

    def plane(self, C, image, c):
        """First element of plane c of `image` in the ragged symbol buffer."""
        return int(C * self.pixbase[image] + c * self.hw[image])

    def masks(self, C):
        """-> (inside an image, covered by an entry): bool (C * total_pix,) over the ragged symbol buffer."""
        inside = np.zeros(C * self.total_pix, dtype=bool)
        covered = np.zeros(C * self.total_pix, dtype=bool)
        for i in range(len(self.hw)):
            inside[self.plane(C, i, 0):self.plane(C, i, 0) + C * int(self.hw[i])] = True
        for (i, p0, n) in self.entries:
            for c in range(C):
                covered[self.plane(C, i, c) + p0:self.plane(C, i, c) + p0 + n] = True
        return inside, covered

    def where(self, C, element):
        """Element of the ragged symbol buffer -> (image, channel, pixel) or 'guard'."""
        for i in range(len(self.hw)):
            a = self.plane(C, i, 0)
            if a <= element < a + C * int(self.hw[i]):
                return (i, int((element - a) // self.hw[i]), int((element - a) % self.hw[i]))
        return 'guard'


def _whole(hw):
    return [(i, 0, int(n)) for i, n in enumerate(hw)]


def _bands(B, HW, L):
    return [(b, j * L, min(L, HW - j * L)) for b in range(B) for j in range(-(-HW // L))]


NEAR, FAR = ('near', ()), ('near', ((0, 1 << 30),))
COUPLED = ('coupled', ())

# `lengths`: every range length around kTablePix; an image of ONE pixel; three bands of image 2 (one listed FIRST: not pixel order;
# its pixels [65, 97) stay uncovered); image 4 covered from pixel 2 on; guard pixels before, between and behind the images.
LENGTHS = EntryCase('lengths', hw=[1, 95, 161, 64, 33], pixbase=[3, 10, 110, 280, 350], total_pix=390,
                    entries=[(2, 97, 64), (0, 0, 1), (1, 0, 95), (2, 0, 32), (2, 32, 33), (3, 0, 64), (4, 2, 31)],
                    kinds=[FAR, COUPLED, ('near', ((32, 65),)), NEAR, COUPLED])
# `mixed`: lengths 1, 64, 200 and 2048 -- with 4 chunks the first two end with chunk 0 (three EMPTY chunks), the others fill every
# chunk, 200 = 64 + 64 + 64 + 8.  Two bands of image 0, the later one listed first; pixels [0, 64) and [2176, 2240) of it uncovered.
# The long band is `near`, the short one `far`; image 2 couples G and B to the decoded channels.
MIXED = EntryCase('mixed', hw=[2240, 1, 264], pixbase=[5, 2250, 2260], total_pix=2530,
                  entries=[(1, 0, 1), (0, 2112, 64), (2, 64, 200), (0, 64, 2048)],
                  kinds=[('near', ((2112, 2176),)), FAR, COUPLED])
MIXED_CHUNKS = 4
# the four RGB pipelines
RECT = EntryCase('rect', hw=[2240] * 3, pixbase=[0, 2240, 4480], total_pix=6720, entries=_whole([2240] * 3), kinds=[NEAR, FAR, COUPLED])
RAGGED = EntryCase('ragged', hw=[197, 700, 2240], pixbase=[0, 197, 897], total_pix=3137, entries=_whole([197, 700, 2240]),
                   kinds=[FAR, NEAR, COUPLED])
BAND_LEN = 256
BANDED = EntryCase('banded', hw=[1000] * 2, pixbase=[0, 1000], total_pix=2000, entries=_bands(2, 1000, BAND_LEN),
                   kinds=[('near', ((256, 512),)), COUPLED])
ENTRY_CASES = {c.name: c for c in (LENGTHS, MIXED, RECT, RAGGED, BANDED)}
Z_ENTRY_CASES = ('lengths', 'mixed')          # ops.decode_z_entries
Z_CHANNELS = (1, 5, 8)


def rect_bounds(HW, chunks):
    """[(pix0, npix)] tiling HW in `chunks` chunks on store-block boundaries (the planner's rule, bitcoding.py)."""
    step = -(-(-(-HW // chunks)) // BLOCK) * BLOCK
    return [(p0, min(step, HW - p0)) for p0 in range(0, HW, step)]


def banded_plan(HW, L, chunks):
    """csrc/decode_pipeline.hip BandPlan: band j steps in len_j / chunks rounded down to 64, the last chunk takes the rest.
    -> (start relative to the band, npix), int64 (chunks, n_bands)."""
    n = -(-HW // L)
    length = np.array([min(L, HW - j * L) for j in range(n)], dtype=np.int64)
    step = length // chunks // BLOCK * BLOCK
    k = np.arange(chunks, dtype=np.int64)[:, None]
    return k * step, np.where(k + 1 < chunks, step, length - k * step)


# name -> (ops entry point, case, plan parameters)
RGB_PIPELINES = {
    'rect': ('decode_rgb', RECT, dict(chunks=3)),
    'ragged': ('decode_rgb_ragged', RAGGED, dict(n_regular=3, probe=0)),
    'ragged-probes': ('decode_rgb_ragged', RAGGED, dict(n_regular=1, probe=64)),
    'banded-1': ('decode_rgb_banded', BANDED, dict(band_len=BAND_LEN, chunks=1)),
    'banded-3': ('decode_rgb_banded', BANDED, dict(band_len=BAND_LEN, chunks=3)),
    'entries': ('decode_rgb_entries', MIXED, dict(chunks=MIXED_CHUNKS)),
}
ENTRIES_SLICE_LIMIT = 2     # ops.decode_rgb_entries(limit=...): the four `mixed` entries in two calls


def stream_chunks(name):
    """The chunks every STREAM of an RGB pipeline case is decoded in: (start relative to the stream's first symbol, npix), int64
    (n_chunks, S), from the rule of its entry point."""
    from l3c_pytorch_amd import ops
    entry_point, case, kw = RGB_PIPELINES[name]
    if entry_point == 'decode_rgb':
        b = np.array(rect_bounds(int(case.hw[0]), kw['chunks']), dtype=np.int64)
        return np.repeat(b[:, :1], case.S, axis=1), np.repeat(b[:, 1:], case.S, axis=1)
    if entry_point == 'decode_rgb_ragged':
        return ops.ragged_rgb_plan([int(v) for v in case.hw], kw['n_regular'], kw['probe'])
    if entry_point == 'decode_rgb_banded':
        start, npix = banded_plan(int(case.hw[0]), kw['band_len'], kw['chunks'])
        return np.tile(start, (1, len(case.hw))), np.tile(npix, (1, len(case.hw)))
    start, npix, _, _ = ops.rgb_entries_plan(case.table()[3], kw['chunks'])
    return start, npix


# ---- table launches -------------------------------------------------------------------------------------------------------------------

TABLE_HW = (5, 19)          # 95 pixels: three blocks of the table kernel, the last one a pixel short
TABLE_B = 3
# grouped: name -> (rgb, C, regime, [(c, pix0, npix)])
GROUPED_CASES = {
    'rgb-3-parts': (True, 3, 'benign', [(0, 0, 95), (1, 31, 33), (2, 63, 32)]),
    'z-5-parts': (False, 5, 'sharp', [(0, 0, 1), (1, 5, 31), (2, 1, 64), (3, 0, 95), (4, 62, 33)]),
    'z-8-parts': (False, 8, 'benign', [(0, 0, 32), (1, 94, 1), (2, 32, 33), (3, 0, 95), (4, 31, 64), (5, 64, 31), (6, 63, 32), (7, 40, 2)]),
    'rgb-1-part': (True, 3, 'lambda', [(1, 7, 33)]),
}
# per part the statistics of the TABLE_B images (window rows per image, RGB): 0 and 3 = window rows, -1 and bit 30 = full rows
WINDOW_STATS = ([0, -1, 95 | WIN_BAD], [-1, 3, 0], [5 | WIN_BAD, 0, -1])


class RaggedTableCase(object):
    """One ragged table launch: the batch (pixbase, hw per image -- or per ENTRY, as ops.decode_z_entries uses the form) and per part its
    channel and every image's (pix0, npix)."""

    def __init__(self, name, pixbase, hw, total_pix, parts):
        self.name, self.total_pix = name, int(total_pix)
        self.pixbase, self.hw = np.asarray(pixbase, dtype=np.int64), np.asarray(hw, dtype=np.int64)
        self.parts = [(int(c), np.asarray(r, dtype=np.int64).reshape(-1, 2)) for c, r in parts]

    def table_off(self, Lp, gaps):
        """-> (per part the BYTE offsets of every image's rows, per part the table's size in entries).  packed: image b's rows right
        behind image b - 1's; gaps: 5 entries in front of the first slot and 7 behind every slot (offsets that are no multiple of 4 bytes)."""
        offs, sizes = [], []
        for _, r in self.parts:
            size = r[:, 1] * Lp + (7 if gaps else 0)
            start = np.cumsum(size) - size + (5 if gaps else 0)
            offs.append(start * 2)
            sizes.append(int(size.sum()) + (5 if gaps else 0))
        return offs, sizes


def _entry_ranges(case):
    _, _, pix0, length = case.table()
    return np.stack([pix0, length], axis=1)


def ragged_table_case(name, C):
    """`lengths-entries`: the batch is the ENTRY table of `lengths` (bands of one image are rows of the batch with the same pixbase), every
    channel a part over the same ranges.  `lengths-parts`: the batch is the IMAGES of `lengths`, three parts of different lengths over
    different ranges, each with npix = 0 for one image."""
    if name == 'lengths-entries':
        pixbase, hw, _, _ = LENGTHS.table()
        return RaggedTableCase(name, pixbase, hw, LENGTHS.total_pix, [(c, _entry_ranges(LENGTHS)) for c in range(min(C, 8))])
    assert name == 'lengths-parts'
    ranges = ([(0, 1), (0, 95), (97, 64), (0, 0), (2, 31)],
              [(0, 1), (10, 32), (0, 33), (0, 64), (5, 0)],
              [(0, 0), (94, 1), (64, 97), (63, 1), (0, 33)])
    return RaggedTableCase(name, LENGTHS.pixbase, LENGTHS.hw, LENGTHS.total_pix, list(zip((0, C - 2, C - 1), ranges)))


RAGGED_TABLE_CASES = ('lengths-entries', 'lengths-parts')


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------------


def near_P(rng, n):
    """The near-40 construction of tests/test_gpu_window.py, pixel-major (n, 120): logits N(0,1), means U(38, 42), log sigma U(0, 1.5),
    lambda = -30 (sigmoid ~ 0: no coupling, G and B stay near 40 too)."""
    CK = 3 * K
    P = rng.randn(n, 4 * CK).astype(np.float32)
    P[:, CK:2 * CK] = rng.uniform(38., 42., size=(n, CK))
    P[:, 2 * CK:3 * CK] = rng.uniform(0., 1.5, size=(n, CK))
    P[:, 3 * CK:] = -30.0
    return P


def rgb_inputs(case, seed=0):
    """-> P (total_pix, 120) fp32 with NaN in the guard pixels, sym int16 (3 * total_pix,) with SENTINEL in the guards.
    ('near', far): near_P; symbols 40 +- 10 (never outside their window), 200 .. 255 in the `far` pixel ranges (outside it EVERY time).
    ('coupled', ()): ref64's `lambda` regime -- saturated and half-open lambda couplings, symbols near a component's mean, every 16th
    uniformly random -- so a symbol outside its window is evaluated with real G <- R and B <- R, G couplings."""
    rng = np.random.RandomState(1000 + seed)
    P = np.full((case.total_pix, 12 * K), np.nan, dtype=np.float32)
    sym = np.full(3 * case.total_pix, SENTINEL, dtype=np.int16)
    for i, (kind, far) in enumerate(case.kinds):
        hw, pb = int(case.hw[i]), int(case.pixbase[i])
        if kind == 'near':
            Pi = near_P(rng, hw)
            s = rng.randint(30, 51, size=(3, hw)).astype(np.int16)
            for a, e in far:
                e = min(e, hw)
                s[:, a:e] = rng.randint(200, 256, size=(3, e - a))
        else:
            Pc, sc, _, _ = ref64.head_case('lambda', True, 1, hw, B=1, K=K)
            Pi, s = Pc[0, :, 0, :].T, sc[0, :, 0, :]
        P[pb:pb + hw] = Pi
        sym[3 * pb:3 * pb + 3 * hw] = s.reshape(-1)
    return P, sym


def z_inputs(case, C, seed=0):
    """Bottleneck inputs, image i in ref64 regime i (cycling): -> P (total_pix, 3 C K) fp32 (NaN guards), sym int16 (C * total_pix,)
    (SENTINEL guards; symbols where the mixture has its mass, every 16th uniformly random)."""
    P = np.full((case.total_pix, 3 * C * K), np.nan, dtype=np.float32)
    sym = np.full(C * case.total_pix, SENTINEL, dtype=np.int16)
    regimes = ref64.regimes(False)
    for i in range(len(case.hw)):
        hw, pb = int(case.hw[i]), int(case.pixbase[i])
        rng = np.random.RandomState(2000 + 100 * seed + 10 * C + i)
        Pi = ref64.make_P(regimes[i % len(regimes)], False, 1, 1, hw, C, K, rng)
        s = ref64.near_sym(Pi, False, C, K, rng)
        P[pb:pb + hw] = Pi[0, :, 0, :].T
        sym[C * pb:C * pb + C * hw] = s.reshape(-1)
    return P, sym


def table_inputs(regime, rgb, C, B=TABLE_B, HW=TABLE_HW):
    """A rectangular batch for the grouped launches: -> P (B, H, W, Kp) fp32 pixel-major, sym int16 (B, C, H, W)."""
    H, W = HW
    rng = np.random.RandomState(3000 + 100 * ref64.REGIMES.index(regime) + 10 * C + int(rgb))
    P = ref64.make_P(regime, rgb, B, H, W, C, K, rng)
    return np.ascontiguousarray(P.transpose(0, 2, 3, 1)), ref64.near_sym(P, rgb, C, K, rng)


def ragged_table_inputs(rcase, rgb, C):
    """Inputs of a ragged table launch over the images of `lengths` (rcase shares its pixbase / hw / total_pix)."""
    return rgb_inputs(LENGTHS, 7) if rgb else z_inputs(LENGTHS, C, 7)
