"""The host half of the native repair, checked without a GPU: l3c_repair_coefficients beside container.rs_repair_coefficients, the round
blobs of l3c_repair_round_plan (csrc/repair_plan.h) beside a restatement of Bitcoding._repair's selection (tests/repair_reference.py) on band
words fabricated from real sections (container.make_seal), l3c_decode_batch_banded_streams_offset / l3c_decode_plan_banded_stream, and the
argument checks of every new entry (each made before anything is launched: fake, well-aligned pointers stand in for device memory).  The
planner also runs stand-alone under the address and undefined-behaviour sanitizers (tests/cabi/repair_plan_check_main.cpp)."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd import _lib, ops
from l3c_pytorch_amd.bitcoding import container
from l3c_pytorch_amd.native_codec import REPAIR_GROUP_DTYPE, ROUND_MAGIC, parse_plan_banded, parse_round
from tests.repair_reference import select_groups
from tests.test_native_banded_abi import INVALID, _cfg, _err, _model, _plan_rc, _shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x100000
H, W, K = 64, 96, 16                      # 6144 pixels: n = 16 bands of L = 384
GEN, MODEL = 7, 0x1122334455667788


def sealed_file(cfg, seed, G=4, R=2, parity=True):
    """A banded file of random payloads with a band table of random words and, with `parity`, the section container.make_seal writes for
    its finest record -> (file, body bytes, the (3, n) table words)."""
    rng = np.random.RandomState(seed)
    shapes = _shapes(cfg, H, W, K)
    payloads = []
    for C, h, w, L in shapes:
        n = container.n_bands(h * w, L)
        payloads.append([[rng.randint(0, 256, int(rng.randint(0, 48))).astype(np.uint8).tobytes() for _ in range(n)] for _ in range(C)])
    body = container.write_file((0, 0, 0, 0), shapes, payloads, True)
    _, h, w, L = shapes[-1]
    n = container.n_bands(h * w, L)
    crcs = rng.randint(0, 2 ** 32, (3, n)).astype(np.uint32)
    rows = None
    if parity:
        rows = [container.rs_parity(payloads[-1][c], G, R) for c in range(3)]
        if R == 1:
            rows = [[p[0] for p in row] for row in rows]
    tail = container.make_seal(body, GEN, container.combine_band_crcs(crcs, L, h * w), MODEL, crcs, L, parity=(G, rows) if parity else None)
    return body + tail, len(body), crcs


class Batch(object):
    """B sealed files, the plan blob of their bodies, their seals, and their sections laid out in a `rows` buffer as NativeCodec does."""

    def __init__(self, specs):
        self.cfg = _cfg()
        made = [sealed_file(self.cfg, 11 + i, **spec) for i, spec in enumerate(specs)]
        self.files, self.bodies = [f for f, _, _ in made], [f[:b] for f, b, _ in made]
        self.words = np.stack([c for _, _, c in made]).copy()                           # (B, 3, n): every band verifies
        self.seals = [container.split_seal(f)[1] for f in self.files]
        rc, msg, blob, _, _, _ = _plan_rc(self.cfg, self.bodies)
        assert rc == 0, msg
        self.plan = np.frombuffer(blob, dtype=np.int64).copy()
        self.parsed = parse_plan_banded(blob)
        self.B, self.n = len(specs), self.words.shape[2]
        self.section_at, parts, at = np.full(self.B, -1, dtype=np.int64), [], 0
        for i, (f, b, _) in enumerate(made):
            if self.seals[i].parity is not None:
                self.section_at[i] = at
                parts.append(f[b:])
                at += (len(f) - b + 15) // 16 * 16
                parts.append(b'\xEE' * (at - sum(len(p) for p in parts)))
        self.rows = np.frombuffer(b''.join(parts), dtype=np.uint8)
        self.tried = np.zeros(0, dtype=REPAIR_GROUP_DTYPE)

    def stream(self, i, c, j):
        first = self.parsed['records'][-1][5]
        s = first + (c * self.B + i) * self.n + j
        return int(self.parsed['dst_offset'][s]), int(self.parsed['nbytes'][s])

    def plan_round(self, words=None, section_at=None, cap=None, files=None, plan=None):
        lib = _lib.load()
        plan = self.plan if plan is None else plan
        n_cap = lib.l3c_repair_round_plan_bytes(ctypes.byref(self.cfg), self.plan.ctypes.data)
        assert n_cap > 0, _err()
        n_cap = n_cap if cap is None else cap
        blob = np.zeros(max(n_cap, 8) // 8, dtype=np.int64)
        bufs = [np.frombuffer(f, dtype=np.uint8) for f in (self.files if files is None else files)]
        ptrs = (ctypes.c_void_p * self.B)(*[b.ctypes.data for b in bufs])
        sizes = np.asarray([b.size for b in bufs], dtype=np.int64)
        words = np.ascontiguousarray(self.words if words is None else words, dtype=np.uint32)
        section_at = np.ascontiguousarray(self.section_at if section_at is None else section_at, dtype=np.int64)
        n_groups = ctypes.c_int64(-5)
        rc = lib.l3c_repair_round_plan(ctypes.byref(self.cfg), plan.ctypes.data, ptrs, sizes.ctypes.data, words.ctypes.data, section_at.ctypes.data,
                                       self.tried.ctypes.data if len(self.tried) else None, len(self.tried), blob.ctypes.data, n_cap,
                                       ctypes.byref(n_groups))
        return rc, blob, n_groups.value

    def round(self, words):
        """One planned round beside the reference -> the parsed blob; the groups join `tried` as the caller's would."""
        rc, blob, n_groups = self.plan_round(words)
        assert rc == 0, _err()
        r = parse_round(blob.tobytes())
        tried = {(int(g['file']), int(g['c']), int(g['g']), tuple(int(j) for j in g['bands'][:g['t']]), int(g['r0'])) for g in self.tried}
        want = select_groups(self.seals, words.view(np.int32), (H, W), [(0, 0, 0, 0)] * self.B, tried)
        got = [(int(g['file']), int(g['c']), int(g['g']), tuple(int(j) for j in g['bands'][:g['t']]), int(g['r0'])) for g in r['groups']]
        assert got == want and n_groups == len(want) == r['n_groups'] and r['magic'] == ROUND_MAGIC and r['bytes'] <= blob.nbytes
        assert all((g['bands'][g['t']:] == 0).all() for g in r['groups'])
        self.check_tables(r, want)
        self.tried = np.concatenate([self.tried, r['groups']])
        return r, want

    def check_tables(self, r, groups):
        """Everything that follows from the groups: the l3c_band_rebuild tables against container.rs_repair_coefficients and the section's
        own bytes, the positions, their entries, streams and CRC spans against numpy."""
        n, B, L, HW = self.n, self.B, r['L'], r['HW']
        assert (r['B'], r['n'], HW) == (B, n, H * W) and r['dst_bytes'] == self.parsed['dst_bytes']
        k = 0
        for q, (i, c, g, js, r0) in enumerate(groups):
            s = self.seals[i]
            m, R, t = s.parity_groups, s.parity_streams, len(js)
            assert tuple(r['files'][i]) == (m, R)
            present = [o for o in range(g, n, m) if o not in js]
            rb = r['rebuild'][q]
            assert (rb['first_src'], rb['n_rows'], rb['n_members'], rb['t'], rb['reserved']) == (k, t, len(present), t, 0)
            solved = [([1], [1] * len(present))] if R == 1 else container.rs_repair_coefficients([(j - g) // m for j in js], [(o - g) // m for o in present], r0)
            for e, (row_w, member_w) in enumerate(solved):
                assert list(r['coef'][k:k + t, e]) == list(row_w) and list(r['coef'][k + t:k + t + len(present), e]) == list(member_w), (q, e)
                assert (int(rb['out'][e]['offset']), int(rb['out'][e]['bytes'])) == self.stream(i, c, js[e])
            assert (r['coef'][k:k + t + len(present), t:] == 0).all() and (rb['out'][t:]['bytes'] == 0).all()
            for u in range(t):                                              # the row spans: the section's own bytes, where the caller put them
                at, nb = int(r['src'][k + u]['offset']), int(r['src'][k + u]['bytes'])
                assert self.rows[at:at + nb].tobytes() == bytes(s.rows(c, g)[r0 + u]), (q, u)
            assert [(int(a), int(b)) for a, b in r['src'][k + t:k + t + len(present)]] == [self.stream(i, c, o) for o in present]
            k += t + len(present)
        assert k == r['n_src']
        spots = sorted({(i, j) for i, _, _, js, _ in groups for j in js})
        assert [tuple(p) for p in r['pos']] == spots and r['S'] == len(spots)
        if not spots:
            return
        e_i, e_j = np.asarray([i for i, _ in spots]), np.asarray([j for _, j in spots])
        length = np.minimum(L, HW - e_j * L)
        assert (r['entries'] == np.stack([e_i * HW, np.full(len(spots), HW), e_j * L, length])).all()
        assert r['n_chunks'] == max(1, min(8, int(length.min()) // 64)) and r['lag'] == (2 if len(spots) >= 16 else 1)
        for c in range(3):
            assert [(int(a), int(b)) for a, b in zip(r['in_offsets'][c], r['in_nbytes'][c])] == [self.stream(i, c, j) for i, j in spots]
            assert (r['crc'][c]['offset'] == (e_i * 3 + c) * HW + e_j * L).all() and (r['crc'][c]['bytes'] == length).all()


def damaged(batch, bad):
    """The batch's table words with the words of the (file, channel, band) in `bad` changed."""
    words = batch.words.copy()
    for i, c, j in bad:
        words[i, c, j] ^= 0x5A5A5A5A
    return words


# ---- coefficients -------------------------------------------------------------------------------------------------------------------


def test_coefficients_equal_rs_repair_coefficients_for_every_erasure_set_and_window():
    lib = _lib.load()
    G, checked = 8, 0
    for t in range(1, 5):
        for erased in itertools.combinations(range(G), t):
            present = [k for k in range(G) if k not in erased]
            for r0 in range(4 - t + 1):
                e, p = np.asarray(erased, dtype=np.int32), np.asarray(present, dtype=np.int32)
                rows, members = np.zeros((t, t), dtype=np.uint8), np.zeros((t, len(present)), dtype=np.uint8)
                assert lib.l3c_repair_coefficients(e.ctypes.data, t, r0, p.ctypes.data, len(present), rows.ctypes.data, members.ctypes.data) == 0, _err()
                want = container.rs_repair_coefficients(erased, present, r0)
                assert [list(r) for r in rows] == [list(w[0]) for w in want] and [list(m) for m in members] == [list(w[1]) for w in want], (erased, r0)
                checked += 1
    assert checked == 8 * 4 + 28 * 3 + 56 * 2 + 70
    one, out = np.asarray([3], dtype=np.int32), np.zeros(16, dtype=np.uint8)
    co = lib.l3c_repair_coefficients
    assert co(None, 1, 0, None, 0, out.ctypes.data, None) == INVALID and 'null pointer' in _err()
    for t, r0 in ((0, 0), (5, 0), (1, 4), (1, -1)):
        assert co(one.ctypes.data, t, r0, None, 0, out.ctypes.data, None) == INVALID and 't must be' in _err(), (t, r0)
    assert co(np.asarray([255], dtype=np.int32).ctypes.data, 1, 0, None, 0, out.ctypes.data, None) == INVALID and '0..254' in _err()
    assert co(np.asarray([3, 3], dtype=np.int32).ctypes.data, 2, 0, None, 0, out.ctypes.data, None) == INVALID and 'singular' in _err()
    assert co(one.ctypes.data, 1, 0, one.ctypes.data, 1, out.ctypes.data, out.ctypes.data) == INVALID and 'not both' in _err()


# ---- round plans --------------------------------------------------------------------------------------------------------------------


def test_one_erasure_per_channel_of_a_file_of_one_row():
    b = Batch([dict(G=4, R=1)])
    r, groups = b.round(damaged(b, [(0, 0, 1), (0, 1, 6), (0, 2, 11)]))
    assert groups == [(0, 0, 1, (1,), 0), (0, 1, 2, (6,), 0), (0, 2, 3, (11,), 0)] and (r['coef'][:, 0] == 1).all()


def test_two_erasures_of_one_group_and_one_more_than_the_rows():
    b = Batch([dict(G=4, R=2)])
    r, groups = b.round(damaged(b, [(0, 0, 1), (0, 0, 5)]))
    assert groups == [(0, 0, 1, (1, 5), 0)] and r['rebuild'][0]['n_rows'] == 2 and r['rebuild'][0]['n_members'] == 2
    b = Batch([dict(G=4, R=2)])
    r, groups = b.round(damaged(b, [(0, 0, 1), (0, 0, 5), (0, 0, 9)]))       # R + 1 erasures: nothing to try
    assert groups == [] and r['n_src'] == 0 and r['S'] == 0


def test_a_failing_member_that_is_no_erasure_of_the_group_keeps_the_group_out():
    b = Batch([dict(G=4, R=2)])
    # band 5 fails at channels 0 and 1: its erasure is channel 0; band 1 fails at channel 1 alone, and its group (1, 1) holds the failing band 5
    r, groups = b.round(damaged(b, [(0, 1, 1), (0, 0, 5), (0, 1, 5)]))
    assert groups == [(0, 0, 1, (5,), 0)]


def test_two_channels_of_one_position_take_two_rounds():
    b = Batch([dict(G=4, R=2)])
    words = damaged(b, [(0, 0, 3), (0, 1, 3)])
    r, groups = b.round(words)
    assert groups == [(0, 0, 3, (3,), 0)]
    words[0, 0, 3] = b.words[0, 0, 3]                                        # the round verified channel 0
    r, groups = b.round(words)
    assert groups == [(0, 1, 3, (3,), 0)]
    words[0, 1, 3] = b.words[0, 1, 3]
    assert b.round(words)[1] == []


def test_a_tried_window_moves_on_and_then_nothing_is_left():
    b = Batch([dict(G=4, R=2)])
    words = damaged(b, [(0, 2, 2)])
    assert b.round(words)[1] == [(0, 2, 2, (2,), 0)]
    assert b.round(words)[1] == [(0, 2, 2, (2,), 1)]                        # the position still fails: the other row
    assert b.round(words)[1] == []
    b = Batch([dict(G=4, R=4)])
    words = damaged(b, [(0, 1, 0), (0, 1, 4), (0, 1, 12)])
    assert [g[4] for _ in range(3) for g in b.round(words)[1]] == [0, 1]    # t = 3 of R = 4: two windows


def test_a_mixed_batch_takes_the_files_of_one_row_first():
    b = Batch([dict(G=4, R=2), dict(G=8, R=1), dict(G=16, R=3), dict(G=4, R=1)])
    r, groups = b.round(damaged(b, [(0, 0, 0), (1, 2, 9), (2, 1, 15), (2, 0, 7), (3, 0, 4), (0, 2, 13)]))
    assert [g[0] for g in groups] == [1, 3, 0, 0, 2, 2]
    assert len(groups) == 6 and r['S'] == 6


def test_a_file_without_parity_and_a_section_that_was_not_uploaded():
    b = Batch([dict(parity=False), dict(G=4, R=2)])
    assert b.section_at[0] == -1
    r, groups = b.round(damaged(b, [(0, 0, 3), (0, 1, 8)]))                  # band-sealed only: nothing to rebuild from
    assert groups == [] and tuple(r['files'][0]) == (0, 0) and tuple(r['files'][1]) == (4, 2)
    words = damaged(b, [(1, 0, 3)])
    rc, _, _ = b.plan_round(words, section_at=[-1, -1])
    assert rc == INVALID and 'section_at' in _err() and 'file 1' in _err()
    assert b.round(words)[1] == [(1, 0, 3, (3,), 0)]


def test_sixteen_positions_decode_on_two_streams():
    b = Batch([dict(G=1, R=1)])                                              # every band a group of its own
    r, groups = b.round(damaged(b, [(0, j % 3, j) for j in range(16)]))
    assert len(groups) == 16 and r['lag'] == 2 and r['n_chunks'] == 6


# ---- refusals -----------------------------------------------------------------------------------------------------------------------


def test_round_planner_refusals():
    lib = _lib.load()
    b = Batch([dict(G=4, R=2)])
    words = damaged(b, [(0, 0, 1)])
    assert lib.l3c_repair_round_plan_bytes(None, b.plan.ctypes.data) < 0
    assert lib.l3c_repair_round_plan_bytes(ctypes.byref(b.cfg), None) == INVALID
    bad = b.plan.copy()
    bad[0] ^= 1
    assert lib.l3c_repair_round_plan_bytes(ctypes.byref(b.cfg), bad.ctypes.data) == INVALID and 'magic' in _err()
    assert b.plan_round(words, plan=bad)[0] == INVALID and 'magic' in _err()
    assert b.plan_round(words, cap=64)[0] == INVALID and 'round_bytes too small' in _err()
    rc, blob, _ = b.plan_round(words)
    assert rc == 0
    exact = int(blob[1])
    assert b.plan_round(words, cap=exact)[0] == 0 and b.plan_round(words, cap=exact - 16)[0] == INVALID and 'round_bytes too small' in _err()
    # a file that is not the plan's: another band count; a damaged seal
    other = sealed_file(b.cfg, 99)[0]
    assert b.plan_round(words, files=[other[:-1] + bytes([other[-1] ^ 1])])[0] == INVALID and 'check word' in _err()
    n_groups = ctypes.c_int64()
    args = [ctypes.byref(b.cfg), b.plan.ctypes.data, (ctypes.c_void_p * 1)(FAKE), FAKE, FAKE, FAKE, None, 0, blob.ctypes.data, blob.nbytes, ctypes.byref(n_groups)]
    for at in (1, 2, 3, 4, 5, 8, 10):
        a = list(args)
        a[at] = None
        assert lib.l3c_repair_round_plan(*a) == INVALID and 'null pointer' in _err(), at
    a = list(args)
    a[7] = -1
    assert lib.l3c_repair_round_plan(*a) == INVALID
    # the accessor of a round blob
    g, ng, p, s = ctypes.POINTER(_lib.RepairGroup)(), ctypes.c_int64(), ctypes.POINTER(ctypes.c_int32)(), ctypes.c_int64()
    refs = (ctypes.byref(g), ctypes.byref(ng), ctypes.byref(p), ctypes.byref(s))
    assert lib.l3c_repair_round_groups(blob.ctypes.data, *refs) == 0 and ng.value == 1 and s.value == 1 and (g[0].file, g[0].c, g[0].bands[0]) == (0, 0, 1)
    assert (p[0], p[1]) == (0, 1)
    assert lib.l3c_repair_round_groups(None, *refs) == INVALID and lib.l3c_repair_round_groups(b.plan.ctypes.data, *refs) == INVALID and 'magic' in _err()
    broken = blob.copy()
    broken[22] += 16                                                         # groups_off
    assert lib.l3c_repair_round_groups(broken.ctypes.data, *refs) == INVALID and 'inconsistent' in _err()


def test_streams_offset_and_the_stream_accessor():
    lib = _lib.load()
    b = Batch([dict(G=4, R=2), dict(G=4, R=2)])
    cfg, plan = ctypes.byref(b.cfg), b.plan.ctypes.data
    off = lib.l3c_decode_batch_banded_streams_offset(cfg, plan)
    assert off >= 0 and off % 256 == 0
    assert off + 240 + b.parsed['dst_bytes'] <= lib.l3c_decode_batch_banded_workspace_bytes(cfg, plan)
    assert off + b.parsed['dst_bytes'] <= lib.l3c_decode_batch_banded_p_offset(cfg, plan)
    assert lib.l3c_decode_batch_banded_streams_offset(cfg, None) == INVALID and lib.l3c_decode_batch_banded_streams_offset(None, plan) < 0
    src, dst, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_uint32()
    out = (ctypes.byref(src), ctypes.byref(dst), ctypes.byref(nb))
    get = lib.l3c_decode_plan_banded_stream
    for k, rec in enumerate(b.parsed['records']):
        for index in (0, rec[6] // 2, rec[6] - 1):
            assert get(plan, k, index, *out) == 0, _err()
            s = rec[5] + index
            assert (src.value, dst.value, nb.value) == (int(b.parsed['src_offset'][s]), int(b.parsed['dst_offset'][s]), int(b.parsed['nbytes'][s]))
        assert get(plan, k, rec[6], *out) == INVALID and 'stream' in _err() and get(plan, k, -1, *out) == INVALID
    assert get(plan, len(b.parsed['records']), 0, *out) == INVALID and 'record' in _err() and get(plan, -1, 0, *out) == INVALID
    assert get(None, 0, 0, *out) == INVALID and get(plan, 0, 0, None, out[1], out[2]) == INVALID and 'null pointer' in _err()
    bad = b.plan.copy()
    bad[0] ^= 1
    assert get(bad.ctypes.data, 0, 0, *out) == INVALID and 'magic' in _err()
    bad = b.plan.copy()
    bad[2] += 1                                                              # B: the layout no longer follows
    assert get(bad.ctypes.data, 0, 0, *out) == INVALID and 'inconsistent' in _err()
    bad = b.plan.copy()
    s = b.parsed['records'][-1][5]
    bad[b.plan[22] // 8 + s] = b.parsed['dst_bytes']                         # dst_off: a slot behind the stream area
    assert get(bad.ctypes.data, len(b.parsed['records']) - 1, 0, *out) == INVALID and 'outside the stream buffer' in _err()
    assert lib.l3c_abi_version() == 4                                        # symbols were added, nothing existing changed


def _rebuild(src, coefs, groups, rows=FAKE, rows_bytes=4096, members=FAKE + (1 << 20), members_bytes=8192, dev=(FAKE + 8, FAKE + 4, FAKE + 16),
             host=(True, True, True), n_groups=None, n_src=None):
    t_src = np.zeros(len(src), dtype=ops.SPAN_DTYPE)
    for k, s in enumerate(src):
        t_src[k] = s
    coef = np.zeros((max(len(src), 1), 4), dtype=np.uint8)
    coef[:len(coefs)] = coefs
    t_g = np.zeros(len(groups), dtype=ops.REBUILD_GROUP_DTYPE)
    for q, (first, n_rows, n_members, t, outs) in enumerate(groups):
        t_g[q]['first_src'], t_g[q]['n_rows'], t_g[q]['n_members'], t_g[q]['t'] = first, n_rows, n_members, t
        for e, o in enumerate(outs):
            t_g[q]['out'][e] = o
    return _lib.load().l3c_band_rebuild(rows, rows_bytes, members, members_bytes, t_src.ctypes.data if host[0] else None, dev[0],
                                        coef.ctypes.data if host[1] else None, dev[1], len(src) if n_src is None else n_src,
                                        t_g.ctypes.data if host[2] else None, dev[2], len(groups) if n_groups is None else n_groups, None)


def test_band_rebuild_argument_checks_precede_any_device_call():
    assert ops.REBUILD_GROUP_DTYPE.itemsize == ctypes.sizeof(_lib.RebuildGroup) == 88 and REPAIR_GROUP_DTYPE.itemsize == ctypes.sizeof(_lib.RepairGroup) == 36
    src = [(5, 100), (107, 100), (0, 90), (128, 100)]                        # two rows at odd offsets, two members
    coefs = [(1, 2, 0, 0), (3, 4, 0, 0), (5, 6, 0, 0), (7, 8, 0, 0)]
    groups = [(0, 2, 2, 2, [(1024, 100), (2048, 77)])]
    # nothing to do is success, whatever the pointers
    assert _rebuild(src, coefs, groups, n_groups=0, rows=None, members=None, dev=(None, None, None), host=(False, False, False)) == 0
    assert _rebuild(src, coefs, groups, n_groups=-1) == INVALID and 'n_groups' in _err()
    assert _rebuild(src, coefs, groups, n_groups=65536) == INVALID
    for host in ((False, True, True), (True, False, True), (True, True, False)):
        assert _rebuild(src, coefs, groups, host=host) == INVALID and 'null pointer' in _err(), host
    for kw in (dict(rows=None), dict(members=None), dict(dev=(None, FAKE, FAKE)), dict(dev=(FAKE, None, FAKE)), dict(dev=(FAKE, FAKE, None))):
        assert _rebuild(src, coefs, groups, **kw) == INVALID and 'null pointer' in _err(), kw
    for kw in (dict(rows=FAKE + 2), dict(members=FAKE + (1 << 20) + 1), dict(dev=(FAKE, FAKE + 2, FAKE))):
        assert _rebuild(src, coefs, groups, **kw) == INVALID and '4-byte aligned' in _err(), kw
    for dev in ((FAKE + 4, FAKE, FAKE), (FAKE, FAKE, FAKE + 4)):
        assert _rebuild(src, coefs, groups, dev=dev) == INVALID and '8-byte aligned' in _err(), dev
    assert _rebuild(src, coefs, groups, members=FAKE + 2048) == INVALID and 'overlap rows' in _err()
    assert _rebuild(src, coefs, groups, rows_bytes=-1) == INVALID and _rebuild(src, coefs, groups, n_src=-1) == INVALID
    # every field of a group
    for g, needle in (((0, 0, 2, 2, groups[0][4]), 'n_rows'), ((0, 5, 2, 2, groups[0][4]), 'n_rows'), ((0, 2, -1, 2, groups[0][4]), 'n_members'),
                      ((0, 2, 2, 0, groups[0][4]), 't must be'), ((0, 2, 2, 5, groups[0][4]), 't must be'), ((-1, 2, 2, 2, groups[0][4]), 'exceed n_src'),
                      ((1, 2, 2, 2, groups[0][4]), 'exceed n_src'), ((2 ** 62, 2, 2, 2, groups[0][4]), 'exceed n_src')):
        assert _rebuild(src, coefs, [g]) == INVALID and needle in _err() and 'group 0' in _err(), (g, _err())
    # a row may lie anywhere inside rows_bytes and end with it; a member follows l3c_u8_xor_spans' rules
    for row, needle in (((-1, 5), 'negative'), ((0, -1), 'negative'), ((4000, 97), 'exceeds rows_bytes'), ((1, 2 ** 63 - 2), 'overflows')):
        assert _rebuild([row] + src[1:], coefs, groups) == INVALID and needle in _err() and 'source 0' in _err(), (row, _err())
    for member, needle in (((2, 90), 'multiple of 4'), ((-4, 90), 'negative'), ((8100, 93), 'exceeds members_bytes'), ((4, 2 ** 63 - 5), 'overflows')):
        assert _rebuild(src[:2] + [member] + src[3:], coefs, groups) == INVALID and needle in _err() and 'source 2' in _err(), (member, _err())
    for out, needle in (((-4, 5), 'negative'), ((0, -1), 'negative'), ((1026, 5), 'multiple of 4'), ((8184, 5), 'exceeds members_bytes'),
                        ((8192, 0), 'exceeds members_bytes'), ((4, 2 ** 63 - 2), 'overflows')):
        assert _rebuild(src, coefs, [(0, 2, 2, 2, [(1024, 100), out])]) == INVALID and needle in _err() and 'group 0' in _err(), (out, _err())
    # an output slot may overlap nothing the call reads or writes: a member of its own group, of another group, another slot; touching is fine
    two = [(0, 1, 1, 1, [(1024, 100)]), (0, 1, 1, 1, [(4096, 100)])]
    for outs, group in (([(88, 10)], 0), ([(224, 4)], 0), ([(1024, 100), (1124, 4)], 0)):
        assert _rebuild(src, coefs, [(0, 2, 2, len(outs), outs)]) == INVALID and 'overlap' in _err() and 'group {}'.format(group) in _err(), (outs, _err())
    assert _rebuild([(5, 100), (0, 90)], coefs[:2], [two[0], (0, 1, 1, 1, [(1120, 8)])]) == INVALID and 'overlap' in _err() and 'group 1' in _err()
    assert _rebuild([(5, 100), (0, 90), (9, 50), (2048, 64)], coefs, [(0, 1, 1, 1, [(2100, 4)]), (2, 1, 1, 1, [(4096, 4)])]) == INVALID and 'overlap' in _err()
    # (touching slots and sources pass the table check: the refusal that follows is the null device pointer)
    assert _rebuild(src, coefs, [(0, 2, 2, 2, [(92, 32), (228, 4)])], dev=(None, FAKE, FAKE)) == INVALID and 'null pointer' in _err()


def _round_desc(b, blob, **kw):
    lib = _lib.load()
    model = _model(b.cfg)
    ws = lib.l3c_decode_batch_banded_workspace_bytes(ctypes.byref(b.cfg), b.plan.ctypes.data)
    rws = lib.l3c_decode_repair_round_workspace_bytes(ctypes.byref(b.cfg), b.plan.ctypes.data, blob.ctypes.data)
    d = _lib.DecodeRepairRoundDesc(ctypes.pointer(model), b.plan.ctypes.data, blob.ctypes.data, FAKE, int(blob[1]), FAKE + (1 << 20), b.rows.size,
                                   FAKE + (2 << 20), ws, FAKE + (3 << 20), FAKE + (4 << 20), FAKE + (5 << 20), FAKE + (6 << 20), max(rws, 0))
    for k, v in kw.items():
        setattr(d, k, v)
    return d, model


def test_repair_round_argument_checks_precede_any_device_call():
    lib = _lib.load()
    b = Batch([dict(G=4, R=2)])
    rc, blob, _ = b.plan_round(damaged(b, [(0, 0, 1), (0, 0, 5), (0, 2, 6)]))
    assert rc == 0
    run = lambda **kw: lib.l3c_decode_repair_round(ctypes.byref(_round_desc(b, blob, **kw)[0]), FAKE, None)      # noqa: E731
    assert lib.l3c_decode_repair_round(None, FAKE, None) == INVALID and 'null descriptor' in _err()
    for name in ('round', 'rows', 'workspace', 'sym', 'pixels', 'crc_out', 'round_workspace', 'plan_host', 'round_host'):
        assert run(**{name: None}) == INVALID and 'null pointer' in _err(), name
    for name in ('round', 'workspace', 'sym', 'pixels', 'crc_out', 'round_workspace'):
        assert run(**{name: FAKE + 8}) == INVALID and '16-byte aligned' in _err(), name
    assert run(rows=FAKE + 2) == INVALID and '4-byte aligned' in _err()
    assert run(workspace_bytes=1024) == INVALID and 'workspace_bytes too small' in _err()
    assert run(round_workspace_bytes=16) == INVALID and 'round_workspace_bytes too small' in _err()
    assert run(round_bytes=int(blob[1]) - 8) == INVALID and 'round_bytes too small' in _err()
    assert run(rows_bytes=10) == INVALID and 'exceeds rows_bytes' in _err()                  # the row spans: l3c_band_rebuild's own check
    r = parse_round(blob.tobytes())
    # every word that follows from the groups is made again and compared; a group that does not fit its file is refused by name
    # (but the row spans, words 0 .. 3 of the source table here: those are bounded by rows_bytes above)
    for word in (9, int(blob[23]) // 8, int(blob[24]) // 8 + 4, int(blob[25]) // 8, int(blob[26]) // 8, int(blob[27]) // 8 + 2, int(blob[28]) // 8, int(blob[30]) // 8 + 1):
        bad = blob.copy()
        bad[word] ^= 4
        d, model = _round_desc(b, bad)
        assert lib.l3c_decode_repair_round(ctypes.byref(d), FAKE, None) == INVALID and 'not what its groups' in _err(), word
        assert lib.l3c_decode_repair_round_workspace_bytes(ctypes.byref(b.cfg), b.plan.ctypes.data, bad.ctypes.data) > 0     # (sizes read the header alone)
    for word, needle in ((0, 'magic'), (2, 'inconsistent header'), (6, 'inconsistent header'), (12, 'another plan')):
        bad = blob.copy()
        bad[word] ^= 1
        d, model = _round_desc(b, bad)
        assert lib.l3c_decode_repair_round(ctypes.byref(d), FAKE, None) == INVALID and needle in _err(), (word, _err())
        assert lib.l3c_decode_repair_round_workspace_bytes(ctypes.byref(b.cfg), b.plan.ctypes.data, bad.ctypes.data) == INVALID
    g_at = int(blob[22]) // 4
    for field, value, needle in ((0, 1, 'names no channel'), (1, 3, 'names no channel'), (2, 4, 'does not fit'), (3, 3, 'does not fit'), (4, 1, 'does not fit'),
                                 (5, 2, 'ascend'), (6, 1, 'ascend'), (7, 1, 'unused bands')):
        bad = blob.copy()
        bad.view(np.int32)[g_at + field] = value                             # group 0: (0, 0, 1, t = 2, r0 = 0, bands 1, 5)
        d, model = _round_desc(b, bad)
        assert lib.l3c_decode_repair_round(ctypes.byref(d), FAKE, None) == INVALID and needle in _err() and 'group 0' in _err(), (field, _err())
    assert r['n_groups'] == 2 and r['S'] == 3
    # a round with nothing left to try enqueues nothing
    rc, empty, n_groups = b.plan_round(b.words)
    assert rc == 0 and n_groups == 0
    d, model = _round_desc(b, empty)
    assert lib.l3c_decode_repair_round(ctypes.byref(d), FAKE, None) == 0


def test_round_planner_survives_broken_files_and_blobs_under_the_sanitizers(tmp_path):
    """tests/cabi/repair_plan_check_main.cpp: repair_plan.h and seal.h alone, built with the address and undefined-behaviour sanitizers and
    run as a child process -- a good file of every section kind, truncated files, bit-flipped sections, short and bit-flipped blobs."""
    exe = tmp_path / 'repair_plan_check'
    subprocess.run(['c++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'cabi', 'repair_plan_check_main.cpp'), '-o', str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4 and all(line.startswith('repair_plan_check: ') for line in lines), r.stdout
    assert lines[0].endswith('rounds planned and checked') and int(lines[0].split()[1]) >= 100
