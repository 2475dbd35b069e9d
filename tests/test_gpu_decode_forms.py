"""-m gpu: the RAGGED and ENTRIES forms of the range decoders (csrc/ac_kernels.hip: stream_view(), r_final, empty chunks) and the four
host pipelines that drive them together with the grouped / ragged table launches (csrc/decode_pipeline.hip: l3c_decode_rgb, _ragged,
_banded, _entries), on the shapes of tests/decode_forms.py.

The streams are built WITHOUT the code under test, once per entry and channel: the rows of the entry's range from the single-part table
launch on its image alone (true symbols for the coupling) -> ops.intervals_from_table -> ops.ac_encode; tests/test_gpu_head_regimes.py,
test_gpu_coder.py and test_gpu_coder_underflow.py tie these three to fp64 and to the oracle.  A decode must give back the encoded symbols
at every covered position and leave every other element of the symbol buffer -- guard gaps, the uncovered pixels of a partly covered
image -- as it was."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import decode_forms as df, ref64  # noqa: E402

K = df.K
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _encode_entries(Pd, symd, td, case, C, rgb):
    """-> payloads[c][e]: entry e's channel c, coded from the single-part table of its image alone over exactly its range."""
    from l3c_pytorch_amd import ops
    Lp = td.shape[0]
    pending = []
    for e, (i, p0, n) in enumerate(case.entries):
        pb, hw = int(case.pixbase[i]), int(case.hw[i])
        Pi = Pd[pb:pb + hw].reshape(1, 1, hw, -1)
        si = symd[C * pb:C * pb + C * hw].reshape(1, C, 1, hw)
        for c in range(C):
            tab = ops.dmll_cdf_table(Pi, si if rgb else None, td, C, K, rgb, c, p0, n)
            iv = ops.intervals_from_table(tab.reshape(n, Lp), si[0, c, 0, p0:p0 + n].reshape(1, n).contiguous(), 1, n)
            pending.append((c, e) + ops.ac_encode(iv, 1, n))
    payloads = [[None] * case.S for _ in range(C)]
    for c, e, out, nbytes in pending:
        payloads[c][e] = out[0, :int(nbytes[0])].cpu().numpy().tobytes()
    return payloads


class Inputs(object):
    """Everything a decode of `case` needs, built once per (case, alphabet, C): device P and bin edges, the true symbols, the packed
    streams (channel-major: stream (c, e) at index c * S + e) and the symbol buffer before / after a correct decode."""

    def __init__(self, case, rgb, C):
        from l3c_pytorch_amd import ops
        self.case, self.rgb, self.C = case, rgb, C
        P, sym = df.rgb_inputs(case) if rgb else df.z_inputs(case, C)
        self.P, self.targets = _dev(P), _dev(ref64.targets32(rgb))
        payloads = _encode_entries(self.P, _dev(sym), self.targets, case, C, rgb)
        flat = [payloads[c][e] for c in range(C) for e in range(case.S)]
        self.buf, self.offs, self.lens = ops.pack_streams(flat)
        self.offs_host = self.offs.cpu().numpy().reshape(C, case.S)
        self.lens_host = self.lens.cpu().numpy().reshape(C, case.S)
        inside, covered = case.masks(C)
        # RGB: the pipelines want the images zeroed, the guards hold the sentinel; bottleneck: the buffer is never read, all sentinel
        self.before = np.where(inside, 0, df.SENTINEL).astype(np.int16) if rgb else np.full(sym.shape, df.SENTINEL, dtype=np.int16)
        self.after = np.where(covered, sym, self.before)
        assert (self.after[inside & ~covered] == self.before[inside & ~covered]).all() and (sym[covered] >= 0).all()

    def fresh(self):
        return _dev(self.before)

    def check(self, got, what):
        got = got.cpu().numpy()
        if np.array_equal(got, self.after):
            return
        bad = np.nonzero(got != self.after)[0]
        first = int(bad[0])
        where = self.case.where(self.C, first)
        entry = None
        if where != 'guard':
            entry = [e for e, (i, p0, n) in enumerate(self.case.entries) if i == where[0] and p0 <= where[2] < p0 + n]
        pytest.fail('{}: {} symbols differ; the first at element {} = (image, channel, pixel) {}, entry {}: got {}, want {}'.format(
            what, bad.size, first, where, entry[0] if entry else 'NONE (uncovered)', int(got[first]), int(self.after[first])))


def _inputs(case, rgb, C):
    key = (case.name, rgb, C)
    if key not in _CACHE:
        _CACHE[key] = Inputs(case, rgb, C)
    return _CACHE[key]


# ---- bottleneck entries: ragged table launch + ragged decoder launch -----------------------------------------------------------------


@pytest.mark.parametrize('C', df.Z_CHANNELS)
@pytest.mark.parametrize('name', df.Z_ENTRY_CASES)
def test_bottleneck_entries_decode_what_was_encoded_and_touch_nothing_else(name, C):
    from l3c_pytorch_amd import ops
    case = df.ENTRY_CASES[name]
    inp = _inputs(case, False, C)
    sym = inp.fresh()
    pixbase, hw, pix0, length = case.table()
    hold = ops.decode_z_entries(inp.P, inp.targets, sym, inp.buf, inp.offs, inp.lens, pixbase, hw, pix0, length, case.total_pix, C, K)
    torch.cuda.synchronize()
    inp.check(sym, 'decode_z_entries {} C={}'.format(name, C))
    assert int(hold[2].item()) == 0


def test_an_empty_chunk_only_carries_the_state_record():
    """The ragged decoder launch with r_npix = 0 for one stream (a short entry beside a long one): no symbol, the stream's state record
    copied from state_in to state_out -- shown by an empty chunk in the MIDDLE of stream 0, which the next chunk resumes from."""
    from l3c_pytorch_amd import _lib, ops
    case = df.EntryCase('states', hw=[96, 160], pixbase=[2, 102], total_pix=270, entries=[(0, 0, 96), (1, 0, 160)])
    chunks = [[(0, 64), (0, 64)], [(64, 0), (64, 64)], [(64, 32), (128, 32)]]
    inp = _inputs(case, False, 1)
    Lp = inp.targets.shape[0]
    sym = inp.fresh()
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    nbytes = 2 * _lib.load().l3c_ac_decode_state_bytes()
    states = [torch.full((nbytes,), fill, dtype=torch.uint8, device='cuda') for fill in (0xA5, 0x5A)]
    pixbase, hw = _dev(case.pixbase), _dev(case.hw)
    for j, ranges in enumerate(chunks):
        rows = [ops.dmll_cdf_table(inp.P[int(case.pixbase[i]):int(case.pixbase[i] + case.hw[i])].reshape(1, 1, int(case.hw[i]), -1), None,
                                   inp.targets, 1, K, False, 0, p0, n).reshape(-1) for i, (p0, n) in enumerate(ranges) if n]
        table = torch.cat(rows)
        p0_d, n_d = _dev(np.array([r[0] for r in ranges], dtype=np.int64)), _dev(np.array([r[1] for r in ranges], dtype=np.int64))
        off_d = _dev(np.array([0, ranges[0][1] * Lp * 2], dtype=np.int64))
        part = _lib.AcDecodePart(_lib.ptr(table), Lp, _lib.ptr(inp.buf, torch.uint8), _lib.ptr(inp.offs, torch.int64),
                                 _lib.ptr(inp.lens, torch.int32), 2, max(n for _, n in ranges), _lib.ptr(flag, torch.int32),
                                 _lib.ptr(states[(j + 1) & 1]) if j else None, _lib.ptr(states[j & 1]), int(j == len(chunks) - 1),
                                 _lib.ptr(sym, torch.int16), 0, 0)
        part.r_npix, part.r_table_off, part.r_pixbase, part.r_hw, part.r_pix0 = (t.data_ptr() for t in (n_d, off_d, pixbase, hw, p0_d))
        part.r_C, part.r_c, part.r_table_bytes = 1, 0, table.numel() * 2
        _lib.call('l3c_ac_decode_chunks', (_lib.AcDecodePart * 1)(part), 1, _lib.stream())
        torch.cuda.synchronize()
        if j == 1:
            half = nbytes // 2
            before, carried = states[0].cpu().numpy(), states[1].cpu().numpy()
            print('state record of the stream with the empty chunk: in', before[:16].tolist(), 'out', carried[:16].tolist())
            assert np.array_equal(carried[:half], before[:half]), 'the empty chunk did not carry stream 0\'s state record on'
            assert not (carried[:16] == 0x5A).all() and not np.array_equal(carried[half:], before[half:])   # (stream 1 moved on)
    inp.check(sym, 'ragged l3c_ac_decode_chunks with an empty chunk')
    assert int(flag.item()) == 0


# ---- the four RGB pipelines -------------------------------------------------------------------------------------------------------------


class _TorchWithFilledWorkspaces(object):
    """`torch` as l3c_pytorch_amd.ops sees it during a pipeline call, with device byte buffers from torch.empty -- the workspaces the ops
    wrappers allocate -- pre-filled with 0xA5: whatever a pipeline needs initialised, it must initialise itself."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*args, **kw):
        t = torch.empty(*args, **kw)
        if t.dtype == torch.uint8 and t.is_cuda:
            t.fill_(0xA5)
        return t


@pytest.fixture
def filled_workspaces(monkeypatch):
    from l3c_pytorch_amd import ops
    monkeypatch.setattr(ops, 'torch', _TorchWithFilledWorkspaces())


@pytest.fixture(scope='module')
def side_stream():
    return torch.cuda.Stream()


def _run_pipeline(name, inp, sym, lag, mode, side, limit=None):
    """-> whatever the ops wrapper returns (workspaces: kept alive by the caller until the device is done)."""
    from l3c_pytorch_amd import ops
    entry_point, case, kw = df.RGB_PIPELINES[name]
    P, t = inp.P, inp.targets
    B, HW = len(case.hw), int(case.hw[0])
    if entry_point == 'decode_rgb':
        return ops.decode_rgb(P.reshape(B, 1, HW, -1), t, sym.reshape(B, 3, 1, HW), inp.buf, inp.offs, inp.lens,
                              df.rect_bounds(HW, kw['chunks']), K, lag, mode, side)
    if entry_point == 'decode_rgb_ragged':
        pix0, npix = df.stream_chunks(name)
        return ops.decode_rgb_ragged(P, t, sym, inp.buf, inp.offs, inp.lens, [int(v) for v in case.hw], pix0, npix, K, lag, mode, side)
    if entry_point == 'decode_rgb_banded':
        return ops.decode_rgb_banded(P.reshape(B, 1, HW, -1), t, sym.reshape(B, 3, 1, HW), inp.buf, inp.offs, inp.lens, kw['band_len'],
                                     kw['chunks'], K, lag, mode, side)
    pixbase, hw, pix0, length = case.table()
    return ops.decode_rgb_entries(P, t, sym, inp.buf, inp.offs_host, inp.lens_host, pixbase, hw, pix0, length, kw['chunks'], K, lag, mode,
                                  side, **({'limit': limit} if limit else {}))


@pytest.mark.parametrize('mode', [0, 1, 2], ids=['full-rows', 'auto', 'window-rows'])
@pytest.mark.parametrize('lag', [1, 2])
@pytest.mark.parametrize('name', sorted(df.RGB_PIPELINES))
def test_rgb_pipeline_decodes_what_was_encoded_and_touches_nothing_else(name, lag, mode, side_stream, filled_workspaces):
    """Every entry point x (lag 1 | lag 2 on a side stream) x window mode, on a batch that mixes a `near` stream (never outside its
    window), a `far` one (outside it every time: the decoder evaluates the full row itself, with the ragged re-basing of P / sym / HW /
    pix0) and a coupled image."""
    from l3c_pytorch_amd import ops
    entry_point, case, kw = df.RGB_PIPELINES[name]
    inp = _inputs(case, True, 3)
    sym = inp.fresh()
    hold = _run_pipeline(name, inp, sym, lag, mode, side_stream)
    torch.cuda.synchronize()
    inp.check(sym, '{} lag {} window mode {}'.format(name, lag, mode))
    if entry_point == 'decode_rgb' and mode == 1:
        # the statistics view, as test_gpu_window.py asserts for the single-part form: image 0 (`near`) never misses, image 1 (`far`)
        # misses on every symbol of every chunk: its count, and bit 30 = too many for window rows
        stats = hold[1].cpu().numpy()
        npix = np.array([n for _, n in df.rect_bounds(int(case.hw[0]), kw['chunks'])])
        print('window statistics (channel, slot, image):', stats.tolist())
        assert stats.shape == (3, len(npix) + 2, 3) and (stats[:, :2] == -1).all()
        assert (stats[:, 2:, 0] == 0).all()
        assert (stats[:, 2:, 1] == (npix | df.WIN_BAD)[None, :]).all()
    if entry_point == 'decode_rgb_entries':
        _check_entries_plan(case, kw['chunks'], hold, ops.ENTRIES_MAX)


def _check_entries_plan(case, n_chunks, hold, limit):
    """The plan the call wrote on the device == ops.rgb_entries_plan, slice by slice, each entry's final chunk included."""
    from l3c_pytorch_amd import ops
    pixbase, hw, pix0, length = case.table()
    slices = ops.entry_slices(case.S, limit)
    assert len(hold) == len(slices)
    for (a, e), (ws, _, _, _) in zip(slices, hold):
        start, npix, final, table_off = ops.rgb_entries_plan(length[a:e], n_chunks)
        d_pixbase, d_hw, d_pix0, d_npix, d_off, d_final = ops.rgb_entries_device_plan(ws, e - a, n_chunks)
        assert np.array_equal(d_pixbase, pixbase[a:e]) and np.array_equal(d_hw, hw[a:e]), (a, e)
        assert np.array_equal(d_pix0, pix0[a:e][None, :] + start), (a, e, d_pix0.tolist())
        assert np.array_equal(d_npix, npix) and np.array_equal(d_off, table_off), (a, e, d_npix.tolist(), d_off.tolist())
        assert np.array_equal(d_final, final), (a, e, d_final.tolist(), final.tolist())


def test_rgb_entries_in_two_slices(side_stream, filled_workspaces):
    """`limit` below the number of entries: the four `mixed` entries go through l3c_decode_rgb_entries two by two, the second call
    beside the symbols the first one left."""
    case = df.MIXED
    inp = _inputs(case, True, 3)
    sym = inp.fresh()
    hold = _run_pipeline('entries', inp, sym, 2, 1, side_stream, limit=df.ENTRIES_SLICE_LIMIT)
    torch.cuda.synchronize()
    inp.check(sym, 'entries in slices of {}'.format(df.ENTRIES_SLICE_LIMIT))
    _check_entries_plan(case, df.MIXED_CHUNKS, hold, df.ENTRIES_SLICE_LIMIT)
