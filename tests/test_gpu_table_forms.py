"""-m gpu: the GROUPED and RAGGED launches of cdf_table_from_P_kernel (csrc/dmll_kernels.hip; l3c_dmll_cdf_table_parts,
l3c_dmll_cdf_table_ragged) bit for bit against the single-part launch of the same kernel, which tests/test_gpu_head_regimes.py ties to
fp64: every row of every (part, image) equals `ops.dmll_cdf_table` on that image ALONE (B = 1, its own P slice and symbols) over exactly
that range, with the same window statistic; every table lives in a buffer of seeded random int16 with slack on both sides, and whatever
lies outside the rows a launch owes is unchanged afterwards; the monotonicity flag is raised for the part that holds the violating row
and for no other.  Shapes and inputs: tests/decode_forms.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import decode_forms as df, ref64  # noqa: E402

K = df.K
SLACK = 37         # entries in front of every table: an odd count, the rows are 2-byte aligned and no more


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i64(a):
    return torch.tensor(np.asarray(a, dtype=np.int64), dtype=torch.int64, device='cuda')


def _i32(a):
    return torch.tensor(np.asarray(a, dtype=np.int64).astype(np.int32), dtype=torch.int32, device='cuda')


def _uses_window(stat):
    return stat is not None and 0 <= stat < df.WIN_BAD


class Buffer(object):
    """A table inside seeded random int16: SLACK entries in front, `behind` entries behind.  `expected` starts as a copy; the test writes
    into it what the launch owes and compares the whole buffer."""

    def __init__(self, size, seed, behind=SLACK):
        rng = np.random.RandomState(seed)
        self.size = int(size)
        self.buf = _dev(rng.randint(-32768, 32768, size=SLACK + self.size + behind).astype(np.int16))
        self.expected = self.buf.clone()
        self.ptr = self.buf.data_ptr() + 2 * SLACK
        self.slots = []                       # (first entry, end, label) of what the launch may write

    def owe(self, first, rows, label):
        """The launch owes `rows` (int16 tensor) from entry `first` of the table on."""
        rows = rows.reshape(-1)
        assert 0 <= first and first + rows.numel() <= self.size, label
        self.expected[SLACK + first:SLACK + first + rows.numel()] = rows
        self.slots.append((first, first + rows.numel(), label))

    def check(self, what):
        if torch.equal(self.buf, self.expected):
            return
        bad = torch.nonzero(self.buf != self.expected).reshape(-1)
        e = int(bad[0]) - SLACK
        where = [(label, (e - a) // label[-1], (e - a) % label[-1]) for a, b, label in self.slots if a <= e < b]
        pytest.fail('{}: {} entries differ, the first at table entry {} (buffer size {}): {} -- got {}, want {}'.format(
            what, bad.numel(), e, self.size, where[0] if where else 'OUTSIDE every row the launch owes',
            int(self.buf[e + SLACK]) & 0xFFFF, int(self.expected[e + SLACK]) & 0xFFFF))


def _reference(Pd, symd, td, C, rgb, c, p0, n, stat=None):
    """The single-part launch on ONE image: Pd (hw, Kp), symd (C, hw) or None.  -> what the launch writes: n full rows, or n window rows
    (65 entries each) when the statistic says so."""
    from l3c_pytorch_amd import ops
    hw = Pd.shape[0]
    ws = _i32([stat]) if stat is not None else None
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    tab = ops.dmll_cdf_table(Pd.reshape(1, 1, hw, -1), symd.reshape(1, C, 1, hw) if rgb else None, td, C, K, rgb, c, p0, n, flag, window_stats=ws)
    rows = tab.reshape(-1)
    return rows[:n * df.WIN_LP] if _uses_window(stat) else rows


def _launch_grouped(Pd, symd, td, B, HW, C, rgb, parts):
    """parts: [(c, pix0, npix, table pointer, flag pointer or None, stats pointer or None)]"""
    from l3c_pytorch_amd import _lib
    arr = (_lib.TablePart * len(parts))(*[_lib.TablePart(*p) for p in parts])
    _lib.call('l3c_dmll_cdf_table_parts', _lib.ptr(Pd, torch.float32), _lib.ptr(symd, torch.int16) if rgb else None, _lib.ptr(td, torch.float32),
              B, HW, C, K, int(rgb), td.shape[0], arr, len(parts), _lib.stream())


def _launch_ragged(Pd, symd, td, C, rgb, pixbase, hw, parts):
    """pixbase, hw: int64 device tensors of the batch; parts: [(c, pix0 tensor, npix tensor, table_off tensor, longest, table pointer,
    flag pointer or None, stats pointer or None)]"""
    from l3c_pytorch_amd import _lib
    batch = _lib.RaggedBatch(hw.numel(), int(hw.max()), pixbase.data_ptr(), hw.data_ptr())
    tparts = (_lib.TablePart * len(parts))()
    rparts = (_lib.RaggedPart * len(parts))()
    for i, (c, p0, n, off, longest, table, flag, stats) in enumerate(parts):
        tparts[i] = _lib.TablePart(c, 0, longest, table, flag, stats)
        rparts[i] = _lib.RaggedPart(p0.data_ptr(), n.data_ptr(), off.data_ptr())
    _lib.call('l3c_dmll_cdf_table_ragged', _lib.ptr(Pd, torch.float32), _lib.ptr(symd, torch.int16) if rgb else None, _lib.ptr(td, torch.float32),
              ctypes.byref(batch), C, K, int(rgb), td.shape[0], tparts, rparts, len(parts), _lib.stream())


# ---- grouped ---------------------------------------------------------------------------------------------------------------------


def _grouped(name, stats_of_part):
    rgb, C, regime, parts = df.GROUPED_CASES[name]
    P, sym = df.table_inputs(regime, rgb, C)
    B, H, W, _ = P.shape
    HW, Lp = H * W, df.lp_of(rgb)
    Pd, symd, td = _dev(P), _dev(sym), _dev(ref64.targets32(rgb))
    flags = torch.zeros(len(parts), dtype=torch.int32, device='cuda')
    bufs, launch, keep = [], [], []
    for i, (c, p0, n) in enumerate(parts):
        stats = stats_of_part(i)
        buf = Buffer(B * n * Lp, 100 * i + len(parts))
        for b in range(B):
            stat = None if stats is None else stats[b]
            rows = _reference(Pd[b].reshape(HW, -1), symd[b].reshape(C, HW), td, C, rgb, c, p0, n, stat)
            buf.owe(b * n * Lp, rows, ('part', i, 'image', b, 'row/entry of', df.WIN_LP if _uses_window(stat) else Lp))
        sd = _i32(stats) if stats is not None else None
        keep.append(sd)
        bufs.append(buf)
        launch.append((c, p0, n, buf.ptr, flags[i:i + 1].data_ptr(), sd.data_ptr() if sd is not None else None))
    _launch_grouped(Pd, symd, td, B, HW, C, rgb, launch)
    torch.cuda.synchronize()
    for i, buf in enumerate(bufs):
        buf.check('{} part {} {}'.format(name, i, parts[i]))
    return flags.cpu().numpy(), bufs


@pytest.mark.parametrize('name', sorted(df.GROUPED_CASES))
def test_grouped_launch_equals_the_single_part_launch(name):
    flags, _ = _grouped(name, lambda i: None)
    assert not flags.any()        # (these regimes give increasing rows; tests/test_gpu_head_regimes.py shows the flag violating ones)


def test_grouped_launch_window_rows_per_image_and_part():
    """RGB, three parts, every part its own statistics over the three images: a windowed image's slot starts with its npix * 65 window
    entries and keeps the rest of its npix * 257 entries untouched; a full-row image's entry 256 carries the window offset."""
    _, bufs = _grouped('rgb-3-parts', lambda i: df.WINDOW_STATS[i])
    parts = df.GROUPED_CASES['rgb-3-parts'][3]
    for i, buf in enumerate(bufs):     # what was compared is what the docstring says: shorter window slots, untouched remainders
        n = parts[i][2]
        for b, stat in enumerate(df.WINDOW_STATS[i]):
            a, e, _ = buf.slots[b]
            assert a == b * n * 257 and e - a == n * (65 if _uses_window(stat) else 257)
        w = [b for b, s in enumerate(df.WINDOW_STATS[i]) if not _uses_window(s)][0]
        offsets = ref64.as_u16(buf.buf[SLACK + w * n * 257:SLACK + (w + 1) * n * 257]).reshape(n, 257)[:, 256]
        assert offsets.max() <= 192 and (n < 8 or len(np.unique(offsets)) > 1)


# ---- ragged ----------------------------------------------------------------------------------------------------------------------


def _ragged(name, rgb, C, gaps, stats_of_part=lambda i: None):
    rcase = df.ragged_table_case(name, C)
    P, sym = df.ragged_table_inputs(rcase, rgb, C)
    Lp = df.lp_of(rgb)
    Pd, symd, td = _dev(P), _dev(sym), _dev(ref64.targets32(rgb))
    pixbase, hw = _i64(rcase.pixbase), _i64(rcase.hw)
    offs, sizes = rcase.table_off(Lp, gaps)
    flags = torch.zeros(len(rcase.parts), dtype=torch.int32, device='cuda')
    bufs, launch, keep = [], [], []
    for i, (c, ranges) in enumerate(rcase.parts):
        stats = stats_of_part(i)
        # slack behind the table as large as the table: a kernel that took the BYTE offsets for entry offsets would still write inside
        # this buffer, where the comparison finds it
        buf = Buffer(sizes[i], 200 * i + C, behind=sizes[i] + SLACK)
        for b, (p0, n) in enumerate(ranges.tolist()):
            if n == 0:
                continue              # nothing for this image: its (empty) slot owes nothing
            pb, h = int(rcase.pixbase[b]), int(rcase.hw[b])
            stat = None if stats is None else stats[b]
            rows = _reference(Pd[pb:pb + h], symd[C * pb:C * pb + C * h].reshape(C, h), td, C, rgb, c, p0, n, stat)
            buf.owe(int(offs[i][b]) // 2, rows, ('part', i, 'image', b, 'row/entry of', df.WIN_LP if _uses_window(stat) else Lp))
        sd = _i32(stats) if stats is not None else None
        t = (_i64(ranges[:, 0]), _i64(ranges[:, 1]), _i64(offs[i]), sd)
        keep.append(t)
        bufs.append(buf)
        launch.append((c, t[0], t[1], t[2], int(ranges[:, 1].max()), buf.ptr, flags[i:i + 1].data_ptr(), sd.data_ptr() if sd is not None else None))
    _launch_ragged(Pd, symd, td, C, rgb, pixbase, hw, launch)
    torch.cuda.synchronize()
    for i, buf in enumerate(bufs):
        buf.check('{} rgb={} C={} gaps={} part {}'.format(name, rgb, C, gaps, i))
    return flags.cpu().numpy()


@pytest.mark.parametrize('gaps', [False, True], ids=['packed', 'gaps'])
@pytest.mark.parametrize('rgb,C', [(True, 3), (False, 5), (False, 8)], ids=['rgb', 'z5', 'z8'])
@pytest.mark.parametrize('name', df.RAGGED_TABLE_CASES)
def test_ragged_launch_equals_the_single_part_launch(name, rgb, C, gaps):
    """Every (part, image) range of the case tables -- lengths 1 .. 97 around the 32-pixel block, a one-pixel image, bands of one image as
    rows of the batch, guard pixels (NaN in P) between the images, npix = 0 for one image of a part -- with the tables packed and with
    gaps between the slots."""
    flags = _ragged(name, rgb, C, gaps)
    assert not flags.any()


@pytest.mark.parametrize('name', df.RAGGED_TABLE_CASES)
def test_ragged_launch_window_rows_per_image_and_part(name):
    n_img = len(df.ragged_table_case(name, 3).hw)
    base = [0, -1, 40 | df.WIN_BAD, 0, 7, -1, 0, df.WIN_BAD]
    _ragged(name, True, 3, True, lambda i: (base[i:] + base[:i])[:n_img])


# ---- the flag is the part's own -----------------------------------------------------------------------------------------------------

NPIX, LIVE = 45, 20          # one row of 45 pixels per image; the live pixel


def _flag_inputs(cA):
    """tests/test_gpu_head_regimes.py, test_monotonicity_flag_one_violating_row_among_saturated_rows: `offrange` rows at the log sigma
    clamp are saturated (constant + l whatever the bin edges), ONE `wide` pixel is live -- here only in channel cA of image 1, so that
    every other part may cover the same pixel and stay saturated."""
    Pw, sym, C, _ = ref64.head_case('wide', True, 1, NPIX)
    P = ref64.head_case('offrange', True, 1, NPIX)[0].copy()
    v = P.reshape(2, 4, C, K, 1, NPIX)
    v[:, 2] = -9.0
    v[1, :, cA, :, 0, LIVE] = Pw.reshape(2, 4, C, K, 1, NPIX)[1, :, cA, :, 0, LIVE]
    return np.ascontiguousarray(P.transpose(0, 2, 3, 1)), sym


def _swapped(t, l):
    t = t.copy()
    t[l], t[l + 1] = t[l + 1], t[l]
    return t


@pytest.mark.parametrize('window', [False, True], ids=['full-rows', 'window-rows'])
@pytest.mark.parametrize('form', ['grouped', 'ragged'])
def test_the_flag_is_raised_for_the_part_with_the_violating_row_only(form, window):
    """Part A (each of R, G, B in turn) covers the live pixel with the LAST row of its range, the other two parts cover it too but see
    saturated rows there: A's flag and no other.  With A's range one pixel shorter -- the live pixel just outside -- no flag at all."""
    from l3c_pytorch_amd import ops
    t = ref64.targets32(True)
    for cA in range(3):
        P, sym = _flag_inputs(cA)
        Pd, symd = _dev(P), _dev(sym)
        stats = _i32([0, 0]) if window else None
        # the pair of bin edges to swap: inside the live pixel's window (its offset from an undisturbed launch), odd and even alike
        w0 = int(ref64.as_u16(ops.dmll_cdf_table(Pd, symd, _dev(t), 3, K, True, cA, LIVE, 1, None, window_stats=_i32([0, 0])))[1].reshape(-1)[64])
        td = _dev(_swapped(t, w0 + 20 + cA))
        for inside in (True, False):
            rangeA = (LIVE - 4, 5) if inside else (LIVE - 4, 4)
            ranges = [(0, NPIX), (LIVE, 9), (LIVE - 1, 3)]
            ranges[cA] = rangeA
            flags = torch.zeros(3, dtype=torch.int32, device='cuda')
            Lp = 257
            row_len = 65 if window else Lp
            if form == 'grouped':
                tabs = [torch.empty(2 * n * Lp, dtype=torch.int16, device='cuda') for _, n in ranges]
                _launch_grouped(Pd, symd, td, 2, NPIX, 3, True,
                                [(c, p0, n, tabs[c].data_ptr(), flags[c:c + 1].data_ptr(), stats.data_ptr() if window else None)
                                 for c, (p0, n) in enumerate(ranges)])
                slot1 = [n * Lp for _, n in ranges]                   # image 1's slot in every part's table
            else:
                # image 0 of part A gets a range of its own, so the live pixel lies inside ONE image's range of part A
                first = [(3, 10) if c == cA else r for c, r in enumerate(ranges)]
                # (twice the rows: a kernel that took the byte offsets for entry offsets would still write inside the tensor)
                tabs = [torch.empty(2 * (first[c][1] + ranges[c][1]) * Lp, dtype=torch.int16, device='cuda') for c in range(3)]
                slot1 = [n * Lp for _, n in first]
                keep = [(_i64([first[c][0], ranges[c][0]]), _i64([first[c][1], ranges[c][1]]), _i64([0, slot1[c] * 2])) for c in range(3)]
                _launch_ragged(Pd.reshape(2 * NPIX, -1), symd.reshape(-1), td, 3, True, _i64([0, NPIX]), _i64([NPIX, NPIX]),
                               [(c, keep[c][0], keep[c][1], keep[c][2], max(first[c][1], ranges[c][1]), tabs[c].data_ptr(),
                                 flags[c:c + 1].data_ptr(), stats.data_ptr() if window else None) for c in range(3)])
            torch.cuda.synchronize()
            got = flags.cpu().numpy().tolist()
            want = [int(inside and c == cA) for c in range(3)]
            print(form, 'window' if window else 'full', 'A =', cA, 'inside' if inside else 'outside', 'flags', got)
            assert got == want, (form, window, cA, inside, got)
            # the inputs do what they are built for: A's row of the live pixel violates, the others' rows of the same pixel do not
            for c, (p0, n) in enumerate(ranges):
                if not p0 <= LIVE < p0 + n:
                    assert c == cA and not inside
                    continue
                at = slot1[c] + (LIVE - p0) * row_len
                row = ref64.as_u16(tabs[c][at:at + row_len])
                bad = ~(np.diff(row[:row_len - 1]) > 0)
                assert int(bad.sum()) == int(c == cA), (form, window, cA, inside, c)
