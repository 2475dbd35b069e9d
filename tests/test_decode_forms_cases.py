"""The case tables of tests/decode_forms.py really hold the edges they claim (so that a later edit cannot drop one unnoticed), and every
RGB pipeline case meets its entry point's preconditions.  No GPU: pure numpy plus the host-only workspace functions of the library."""
import ctypes

import numpy as np
import pytest

from tests import decode_forms as df


def _all_range_lengths():
    lengths = set()
    for case in df.ENTRY_CASES.values():
        lengths.update(e[2] for e in case.entries)
    for _, _, _, parts in df.GROUPED_CASES.values():
        lengths.update(n for _, _, n in parts)
    for name in df.RAGGED_TABLE_CASES:
        for _, r in df.ragged_table_case(name, 3).parts:
            lengths.update(int(n) for n in r[:, 1])
    return lengths


def test_range_lengths_around_the_table_block():
    assert df.RANGE_LENGTHS == (1, 31, 32, 33, 64, 95)
    assert set(df.RANGE_LENGTHS) <= _all_range_lengths()
    assert set(df.RANGE_LENGTHS) <= set(e[2] for e in df.LENGTHS.entries)          # all of them in ONE entry table
    for name, (rgb, C, _, parts) in df.GROUPED_CASES.items():
        H, W = df.TABLE_HW
        assert 1 <= len(parts) <= 8 and len(parts) <= max(C, 1), name
        for c, p0, n in parts:
            assert 0 <= c < C and p0 >= 0 and n > 0 and p0 + n <= H * W, (name, c, p0, n)
    assert (H * W) % df.TABLE_PIX and H * W > 2 * df.TABLE_PIX                     # several blocks, the last one ragged
    assert sorted(len(p[3]) for p in df.GROUPED_CASES.values()) == [1, 3, 5, 8]
    assert [(p[0], p[1]) for p in df.GROUPED_CASES.values()].count((True, 3)) == 2
    assert any(C == 8 and len(parts) == 8 for _, C, _, parts in df.GROUPED_CASES.values())
    assert any(not rgb and C == 5 and len(parts) == 5 for rgb, C, _, parts in df.GROUPED_CASES.values())


def test_parts_of_different_lengths_over_different_ranges():
    rgb3 = df.GROUPED_CASES['rgb-3-parts'][3]
    assert [c for c, _, _ in rgb3] == [0, 1, 2]
    assert len({n for _, _, n in rgb3}) == 3 and len({p0 for _, p0, _ in rgb3}) == 3
    for name in ('z-5-parts', 'z-8-parts'):
        assert len({n for _, _, n in df.GROUPED_CASES[name][3]}) > 3
    r = df.ragged_table_case('lengths-parts', 3)
    assert len({int(q[:, 1].max()) for _, q in r.parts}) == len(r.parts)             # every part's longest range differs
    assert len(df.WINDOW_STATS) == 3 and all(len(s) == df.TABLE_B for s in df.WINDOW_STATS)
    assert len({tuple(s) for s in df.WINDOW_STATS}) == 3                               # differently per part
    for s in df.WINDOW_STATS:      # every part mixes window rows (0 <= v < 2^30) with full rows; every image is windowed in some part
        kinds = [0 <= v < df.WIN_BAD for v in s]
        assert any(kinds) and not all(kinds)
    assert all(any(0 <= s[b] < df.WIN_BAD for s in df.WINDOW_STATS) for b in range(df.TABLE_B))
    assert any(v & df.WIN_BAD and v > 0 for s in df.WINDOW_STATS for v in s) and any(v == -1 for s in df.WINDOW_STATS for v in s)
    assert any(0 < v < df.WIN_BAD for s in df.WINDOW_STATS for v in s)


def test_a_part_with_an_empty_range_for_one_image():
    r = df.ragged_table_case('lengths-parts', 5)
    assert [c for c, _ in r.parts] == [0, 3, 4]
    for _, q in r.parts:
        assert (q[:, 1] == 0).sum() == 1 and (q[:, 1] > 0).sum() == len(r.hw) - 1
        assert (q[:, 0] >= 0).all() and (q[:, 0] + q[:, 1] <= r.hw).all()
    assert len({int(np.argmin(q[:, 1])) for _, q in r.parts}) == len(r.parts)         # a different image each time
    for gaps in (False, True):
        offs, sizes = r.table_off(257, gaps)
        for (c, q), o, size in zip(r.parts, offs, sizes):
            slots = sorted((int(a) // 2, int(a) // 2 + int(n) * 257) for a, n in zip(o, q[:, 1]))
            assert (o % 2 == 0).all() and slots[-1][1] <= size
            assert all(a[1] <= b[0] for a, b in zip(slots, slots[1:]))                # slots do not overlap
            assert gaps == any(a[1] < b[0] for a, b in zip(slots, slots[1:]) if a[0] < a[1])
            assert int(o[0]) == (10 if gaps else 0)
    e = df.ragged_table_case('lengths-entries', 8)
    assert len(e.parts) == 8 and len(e.hw) == df.LENGTHS.S


@pytest.mark.parametrize('name', sorted(df.ENTRY_CASES))
def test_entries_lie_inside_their_images(name):
    case = df.ENTRY_CASES[name]
    assert len(case.hw) <= 8 and case.S <= 8 and case.hw.max() <= 2240
    ends = case.pixbase + case.hw
    assert (case.pixbase >= 0).all() and (ends[:-1] <= case.pixbase[1:]).all() and ends[-1] <= case.total_pix
    pixbase, hw, pix0, length = case.table()
    assert (pix0 >= 0).all() and (length > 0).all() and (pix0 + length <= hw).all()
    inside, covered = case.masks(3)
    assert not (covered & ~inside).any()
    for i in range(len(case.hw)):          # the entries of an image do not overlap
        spans = sorted((p0, p0 + n) for (j, p0, n) in case.entries if j == i)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (name, i)
    assert covered.sum() == 3 * sum(e[2] for e in case.entries)
    assert len(case.kinds) == len(case.hw)
    last = len(case.hw) - 1
    assert case.where(3, case.plane(3, last, 2)) == (last, 2, 0) and case.where(3, 3 * case.total_pix - 1) in ('guard', (last, 2, int(case.hw[last]) - 1))


def test_entry_table_edges():
    L, M = df.LENGTHS, df.MIXED
    for case in (L, M):
        assert (case.hw == 1).any()                                                   # an image of one pixel
        assert case.pixbase[0] > 0 and ((case.pixbase + case.hw)[:-1] < case.pixbase[1:]).all()    # guard pixels in front of and between
        assert case.pixbase[-1] + case.hw[-1] < case.total_pix                                        # ... and behind the images
        images = [e[0] for e in case.entries]
        assert len(images) > len(set(images))                                                         # bands of the same image
        pixbase, _, pix0, _ = case.table()
        assert (np.diff(pixbase + pix0) < 0).any()                                                    # not in pixel order
        inside, covered = case.masks(3)
        assert (inside & ~covered).any() and (~inside).any()                                          # partly covered images, guards
    assert sum(1 for e in L.entries if e[0] == 2) == 3
    for case in (df.RECT, df.RAGGED, df.BANDED):           # the pipelines that take whole images: packed, every pixel covered
        inside, covered = case.masks(3)
        assert inside.all() and covered.all()
    assert [int(v) for v in df.RAGGED.hw] == [197, 700, 2240] and (df.RECT.hw == 2240).all() and len(df.RECT.hw) == 3
    assert (df.BANDED.hw == 1000).all() and len(df.BANDED.hw) == 2 and df.BAND_LEN == 256 and df.BANDED.S == 8
    for case in df.ENTRY_CASES.values():     # every RGB batch mixes a near stream with a far one and has a coupled image
        kinds = case.kinds
        assert any(k == 'coupled' for k, _ in kinds)
        assert any(k == 'near' and far for k, far in kinds) and any(k == 'near' and (not far or far[0][1] < 1 << 30) for k, far in kinds)


def test_mixed_entries_have_empty_trailing_chunks_beside_full_ones():
    from l3c_pytorch_amd import ops
    lens = df.MIXED.table()[3]
    assert sorted(lens.tolist()) == [1, 64, 200, 2048] and df.MIXED_CHUNKS == 4
    start, npix, final, table_off = ops.rgb_entries_plan(lens, df.MIXED_CHUNKS)
    assert (npix.sum(axis=0) == lens).all()
    empty = (npix == 0)
    assert empty[1:, lens <= 64].all() and not empty[0].any()                          # the short entries: chunk 0 only
    assert not empty[:, lens >= 200].any()                                             # the others fill every chunk
    assert final.tolist() == [0 if n <= 64 else 3 for n in lens]
    assert npix[3, list(lens).index(200)] == 8                                         # a last chunk that is no multiple of 64
    assert len(ops.entry_slices(df.MIXED.S, df.ENTRIES_SLICE_LIMIT)) == 2


@pytest.mark.parametrize('name', sorted(df.RGB_PIPELINES))
def test_pipeline_preconditions(name):
    """include/l3c_hip.h: chunk boundaries on multiples of 64 (relative to the stream's first symbol), chunks tile the stream, a band
    holds 64 symbols per chunk, and the host-only workspace functions accept the shape."""
    from l3c_pytorch_amd import _lib, ops
    lib = _lib.load()
    entry_point, case, kw = df.RGB_PIPELINES[name]
    start, npix = df.stream_chunks(name)
    lens = case.table()[3]
    n_chunks, S = npix.shape
    assert S == case.S and (npix.sum(axis=0) == lens).all()
    assert (start % df.BLOCK == 0)[npix > 0].all()
    for s in range(S):
        live = npix[:, s] > 0
        assert live[0] and not (np.diff(live.astype(int)) > 0).any()                   # empty chunks only trail
        assert (start[live, s] == np.cumsum(npix[:, s])[live] - npix[live, s]).all()
    if entry_point != 'decode_rgb_entries':
        assert (npix > 0).all()
    if entry_point == 'decode_rgb':
        assert n_chunks == kw['chunks'] == 3
        ws = lib.l3c_decode_rgb_workspace_bytes(S, int(npix.max()), n_chunks, 2)
        assert 0 <= lib.l3c_decode_rgb_stats_offset(S, int(npix.max()), n_chunks, 2) < ws
    elif entry_point == 'decode_rgb_ragged':
        assert n_chunks == kw['n_regular'] + (2 if kw['probe'] else 0)
        assert not kw['probe'] or (npix[:2] == kw['probe']).all()
        ws = lib.l3c_decode_rgb_ragged_workspace_bytes(S, int(npix.sum(axis=1).max()), n_chunks, 2)
    elif entry_point == 'decode_rgb_banded':
        assert n_chunks == kw['chunks'] and (n_chunks == 1 or lens.min() >= df.BLOCK * n_chunks)
        assert kw['band_len'] % df.BLOCK == 0
        ws = lib.l3c_decode_rgb_banded_workspace_bytes(len(case.hw), int(case.hw[0]), kw['band_len'], n_chunks, 2)
    else:
        assert n_chunks == kw['chunks']
        ws = lib.l3c_decode_rgb_entries_workspace_bytes(S, np.ascontiguousarray(lens).ctypes.data_as(ctypes.POINTER(_lib.c_i64)), n_chunks, 2)
        assert ws == ops.rgb_entries_workspace_bytes(lens, n_chunks, 2)
    assert ws >= 0
    if name in ('ragged', 'ragged-probes', 'banded-3', 'entries'):
        assert (npix[-1] % df.BLOCK != 0).any()                                        # a last chunk that is no multiple of 64


def test_builders_are_seeded_and_put_the_symbols_where_they_claim():
    for case in (df.MIXED, df.LENGTHS):
        P, sym = df.rgb_inputs(case)
        P2, sym2 = df.rgb_inputs(case)
        assert np.array_equal(sym, sym2) and np.array_equal(P, P2, equal_nan=True)
        inside, _ = case.masks(3)
        assert (sym[~inside] == df.SENTINEL).all() and (sym[inside] >= 0).all() and (sym[inside] <= 255).all()
        assert np.isnan(P).all(axis=1).sum() == case.total_pix - case.hw.sum() and not np.isnan(P).any(axis=1)[case.pixbase[0]]
        for i, (kind, far) in enumerate(case.kinds):
            if kind != 'near':
                continue
            hw = int(case.hw[i])
            is_far = np.zeros(hw, dtype=bool)
            for a, e in far:
                is_far[a:min(e, hw)] = True
            planes = sym[case.plane(3, i, 0):case.plane(3, i, 0) + 3 * hw].reshape(3, hw)
            assert (np.abs(planes[:, ~is_far] - 40) <= 10).all() and (planes[:, is_far] >= 200).all()
            Pi = P[case.pixbase[i]:case.pixbase[i] + hw]
            assert (Pi[:, 90:] == -30).all() and (np.abs(Pi[:, 30:60] - 40) <= 2).all()
    for C in df.Z_CHANNELS:
        P, sym = df.z_inputs(df.LENGTHS, C)
        inside, _ = df.LENGTHS.masks(C)
        assert P.shape == (df.LENGTHS.total_pix, 3 * C * df.K)
        assert (sym[~inside] == df.SENTINEL).all() and (sym[inside] >= 0).all() and (sym[inside] <= 24).all()
    P, sym = df.table_inputs('benign', False, 8)
    assert P.shape == (df.TABLE_B, 5, 19, 3 * 8 * df.K) and sym.shape == (df.TABLE_B, 8, 5, 19)
