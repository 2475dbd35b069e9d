"""-m gpu: the five kernels of csrc/container.hip -- container_write_kernel, banded_positions_kernel, container_write_banded_kernel,
band_intervals_kernel, container_read_kernel -- byte by byte against host references, on synthetic inputs chosen for their edges: payload
rows of random bytes with chosen lengths (no coder, no network runs).  The references are bitcoding.container.write_file for both file
formats and a few lines of numpy for the stream cutter and the interval re-lay."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = [0, 1, 2, 3, 4, 5, 7, 8, 9]
LENGTHS = SMALL + list(range(255, 261)) + list(range(1021, 1031)) + [5003]
GUARD = 64


def _draw_lengths(rng, count, p_small=0.5):
    """`count` stream lengths from LENGTHS, the short ones (shorter than a head, no body, one body dword) drawn more often"""
    small = rng.choice(SMALL, size=count)
    any_ = rng.choice(LENGTHS, size=count)
    return np.where(rng.random_sample(count) < p_small, small, any_).astype(np.int64)


def _rows(rng, lengths, random_tail=False):
    """coder output rows for streams of `lengths` bytes: (rows uint8 (S, stride), payload bytes per stream); the row stride a multiple of
    4 larger than the longest stream, the bytes beyond a stream's length 0xAB, or random ones with random_tail"""
    S = len(lengths)
    stride = (int(max(lengths)) + 4) // 4 * 4
    assert stride % 4 == 0 and stride > max(lengths)
    data = rng.randint(0, 256, size=(S, stride)).astype(np.uint8)
    payloads = [data[i, :n].tobytes() for i, n in enumerate(lengths)]
    if not random_tail:
        for i, n in enumerate(lengths):
            data[i, n:] = 0xAB
    return data, payloads


def _copy_classes(dst_pos, n):
    """what copy_payload (csrc/container.hip) does with a payload of n bytes that lands at byte dst_pos of an aligned buffer:
    (destination alignment, head bytes, body class 0 / 1 / 2 = many dwords, tail bytes)"""
    a = dst_pos & 3
    h = min((4 - a) & 3, n)
    body = (n - h) // 4
    return a, h, min(body, 2), n - h - 4 * body


# ---- l3c_container_write ----------------------------------------------------------------------------------------------------------

SHAPES = [1, 65535, 7, 300, 2, 65535, 1, 40]        # H / W of the scale records: both ends of u16 among them
PADDINGS = [0, 65535, 1, 255, 256, 65535, 0, 12]


@functools.lru_cache(maxsize=None)
def _write_plans():
    """Every case of the legacy writer test, built on the host: n_scales in {1, 4, 8} x B in {1, 3} x three rotations of C in {1, 3, 5}.
    -> list of dicts(n_scales, B, scales [(C, H, W)], padding [B][4], lengths [k] (B, C), sizes (B,), offsets (B,))"""
    from l3c_pytorch_amd.bitcoding import container
    plans = []
    for n_scales in (1, 4, 8):
        for B in (1, 3):
            for rot in range(3):
                rng = np.random.RandomState(1000 * n_scales + 10 * B + rot)
                scales = [((1, 3, 5)[(rot + k) % 3], SHAPES[(k + rot) % 8], SHAPES[(k + 3 * rot + 1) % 8]) for k in range(n_scales)]
                lengths = [_draw_lengths(rng, B * C).reshape(B, C) for C, _, _ in scales]
                padding = [[PADDINGS[(4 * b + i + rot) % 8] for i in range(4)] for b in range(B)]
                sizes = np.asarray([container.framing_bytes(scales, False) + sum(int(n[b].sum()) for n in lengths) for b in range(B)], dtype=np.int64)
                plans.append(dict(n_scales=n_scales, B=B, scales=scales, padding=padding, lengths=lengths, sizes=sizes,
                                  offsets=np.cumsum(sizes) - sizes, seed=int(rng.randint(1 << 30))))
    return plans


def _legacy_payload_positions(plan):
    """(position inside the destination buffer, length) of every payload of a plan: the files lie back to back"""
    res = []
    for b in range(plan['B']):
        p = int(plan['offsets'][b]) + 8
        for (C, _, _), n in zip(plan['scales'], plan['lengths']):
            p += 5
            for c in range(C):
                res.append((p + 4, int(n[b, c])))
                p += 4 + int(n[b, c])
            p += 4
        assert p == plan['offsets'][b] + plan['sizes'][b]
    return res


def _assert_copy_coverage(positions):
    """every destination alignment 0..3 meets every head length it can have (a stream shorter than its head included), a body of 0, 1 and
    many dwords, and every tail length"""
    seen = {_copy_classes(p, n) for p, n in positions}
    for a in range(4):
        for h in range(((4 - a) & 3) + 1):
            assert any(s[0] == a and s[1] == h for s in seen), ('alignment x head', a, h)
        for body in range(3):
            assert any(s[0] == a and s[2] == body for s in seen), ('alignment x body', a, body)
        for tail in range(4):
            assert any(s[0] == a and s[3] == tail for s in seen), ('alignment x tail', a, tail)
    assert any(n == 0 for _, n in positions) and any(n == 5003 for _, n in positions)


def test_legacy_writer_cases_cover_every_alignment_head_and_body():
    """host only: the coverage the cases below rely on, over all of them; also the parameter grid the cases are meant to span"""
    plans = _write_plans()
    _assert_copy_coverage([q for p in plans for q in _legacy_payload_positions(p)])
    assert {p['n_scales'] for p in plans} == {1, 4, 8} and {p['B'] for p in plans} == {1, 3}
    assert {s[0] for p in plans for s in p['scales']} == {1, 3, 5}
    dims = {d for p in plans for s in p['scales'] for d in s[1:]}
    pads = {v for p in plans for row in p['padding'] for v in row}
    assert {1, 65535} <= dims and {0, 65535} <= pads


@pytest.mark.parametrize('case', range(18))
def test_container_write_vs_host_writer(case):
    """l3c_container_write, called the way EncodedBatch._write_container does, against bitcoding.container.write_file: the files byte for
    byte, the guard bytes behind them untouched, the lengths read back by parse_containers.  Rows beyond their nbytes hold 0xAB, the
    destination 0xCD."""
    from l3c_pytorch_amd import _lib, ops
    from l3c_pytorch_amd.bitcoding import container
    plans = _write_plans()
    assert len(plans) == 18
    _assert_copy_coverage([q for p in plans for q in _legacy_payload_positions(p)])          # on the host, before anything is launched
    plan = plans[case]
    B, scales = plan['B'], plan['scales']
    rng = np.random.RandomState(plan['seed'])
    keep, payloads = [], []
    arr = (_lib.ContainerScale * len(scales))()
    for k, ((C, H, W), n) in enumerate(zip(scales, plan['lengths'])):
        rows, pl = _rows(rng, n.reshape(-1))
        out, nbytes = torch.from_numpy(rows).cuda(), torch.from_numpy(n.reshape(-1).astype(np.int32)).cuda()
        keep.append((out, nbytes, rows))
        payloads.append([[pl[b * C + c] for c in range(C)] for b in range(B)])
        arr[k] = _lib.ContainerScale(ops.ptr(out, torch.uint8), ops.ptr(nbytes, torch.int32), out.shape[1], C, H, W)
    files = [container.write_file(plan['padding'][b], scales, [p[b] for p in payloads], False) for b in range(B)]
    assert [len(f) for f in files] == list(plan['sizes'])
    total = int(plan['sizes'].sum())
    dst = torch.full((total + GUARD,), 0xCD, dtype=torch.uint8, device='cuda')
    pads = torch.from_numpy(np.asarray(plan['padding'], dtype=np.uint16).reshape(B, 4).view(np.int16)).cuda()
    offsets = torch.from_numpy(plan['offsets']).cuda()
    ops.call('l3c_container_write', arr, len(scales), B, ops.ptr(pads), ops.ptr(offsets, torch.int64), ops.ptr(dst), ops.stream())
    got = dst.cpu().numpy()
    want = np.frombuffer(b''.join(files) + bytes([0xCD]) * GUARD, dtype=np.uint8)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, 'first differing byte {} of {} (got {:#x}, want {:#x}); {} differ'.format(bad[0], total, got[bad[0]], want[bad[0]], bad.size)
    for b in range(B):          # the length fields, walked by hand (parse_containers refuses a file of one scale record)
        f, p = got[plan['offsets'][b]:plan['offsets'][b] + plan['sizes'][b]].tobytes(), 8
        for (C, _, _), n in zip(scales, plan['lengths']):
            p += 5
            for c in range(C):
                assert int.from_bytes(f[p:p + 4], 'little') == n[b, c]
                p += 4 + int(n[b, c])
            p += 4
        assert p == len(f)
    if len(scales) >= 2:
        parsed = container.parse_containers([got[o:o + s].tobytes() for o, s in zip(plan['offsets'], plan['sizes'])])
        assert parsed.scales == scales and [tuple(p) for p in parsed.padding] == [tuple(p) for p in plan['padding']]
        for k, n in enumerate(plan['lengths']):
            assert np.array_equal(parsed.nbytes[k], n)
    # the source rows are only read
    for out, _, rows in keep:
        assert np.array_equal(out.cpu().numpy(), rows)


# ---- l3c_container_write_banded ---------------------------------------------------------------------------------------------------

BANDED_SCALES = [(5, 8, 8, 64),          # one band: no full group, out_full NULL
                 (5, 10, 10, 64),        # two bands
                 (3, 95, 202, 64),       # H W = 64 * 300 - 10: 300 bands, 900 streams -- four rounds of the 256-wide scan
                 (1, 256, 256, 64)]      # the limit of 1024 bands per channel


def _banded_positions(scales, lengths, b, carry=True):
    """position inside file b of every length field, in file order (the format's, include/l3c_hip.h); carry False: what a scan in rounds
    of 256 streams gives when it drops the carry between its rounds -- only to show on the host that this input would expose that"""
    v = np.concatenate([4 + n[b].reshape(-1) for n in lengths])
    k = np.concatenate([np.full(n[b].size, i) for i, n in enumerate(lengths)])
    excl = np.cumsum(v) - v
    if not carry:
        i = np.arange(v.size)
        excl = excl - excl[i // 256 * 256]
    return 14 + 13 * k + 9 + excl


def test_container_write_banded_vs_host_writer():
    """l3c_container_write_banded (banded_positions_kernel: a scan of the length fields 256 at a time with a carry;
    container_write_banded_kernel) against write_file(..., banded=True) for B = 2 images with different lengths: files byte for byte, guard
    bytes untouched, every file read back by parse_banded.  Rows beyond their nbytes hold random garbage."""
    from l3c_pytorch_amd import _lib, ops
    from l3c_pytorch_amd.bitcoding import container
    from l3c_pytorch_amd.bitcoding.container import n_bands
    B, scales = 2, BANDED_SCALES
    rng = np.random.RandomState(77)
    nb = [n_bands(H * W, L) for _, H, W, L in scales]
    assert nb == [1, 2, 300, 1024] and 95 * 202 == 64 * 300 - 10
    lengths = [_draw_lengths(rng, B * C * n, p_small=0.8).reshape(B, C, n) for (C, _, _, _), n in zip(scales, nb)]
    spi = sum(C * n for (C, _, _, _), n in zip(scales, nb))
    # host-side preconditions: more than 256 streams per image, lengths that differ between the images and inside a scan round, and a
    # position that a missing carry would change
    assert spi > 4 * 256
    assert all(len(set(n[b].reshape(-1).tolist())) > 8 for n in lengths[2:] for b in range(B))
    assert not np.array_equal(lengths[2][0], lengths[2][1])
    for b in range(B):
        with_c, without = _banded_positions(scales, lengths, b), _banded_positions(scales, lengths, b, carry=False)
        assert (with_c[256:] != without[256:]).all() and np.array_equal(with_c[:256], without[:256])

    keep, payloads = [], []
    arr = (_lib.BandedScale * len(scales))()
    for k, ((C, H, W, L), n, ln) in enumerate(zip(scales, nb, lengths)):
        rows_l, pl_l = _rows(rng, ln[:, :, n - 1].reshape(-1), random_tail=True)
        out_l, nb_l = torch.from_numpy(rows_l).cuda(), torch.from_numpy(ln[:, :, n - 1].reshape(-1).astype(np.int32)).cuda()
        out_f = nb_f = pl_f = None
        if n > 1:
            rows_f, pl_f = _rows(rng, ln[:, :, :n - 1].reshape(-1), random_tail=True)
            out_f, nb_f = torch.from_numpy(rows_f).cuda(), torch.from_numpy(ln[:, :, :n - 1].reshape(-1).astype(np.int32)).cuda()
        keep.append((out_l, nb_l, out_f, nb_f))
        payloads.append([[[pl_f[(b * C + c) * (n - 1) + j] for j in range(n - 1)] + [pl_l[b * C + c]] for c in range(C)] for b in range(B)])
        arr[k] = _lib.BandedScale(ops.ptr(out_f, torch.uint8), ops.ptr(nb_f, torch.int32), out_f.shape[1] if out_f is not None else 0,
                                  ops.ptr(out_l, torch.uint8), ops.ptr(nb_l, torch.int32), out_l.shape[1], C, H, W, L)
    padding = [(0, 65535, 3, 4), (65535, 0, 1, 2)]
    files = [container.write_file(padding[b], scales, [p[b] for p in payloads], True) for b in range(B)]
    sizes = np.asarray([len(f) for f in files], dtype=np.int64)
    assert list(sizes) == [container.framing_bytes(scales, True) + sum(int(n[b].sum()) for n in lengths) for b in range(B)]
    offs = np.cumsum(sizes) - sizes
    total = int(sizes.sum())
    dst = torch.full((total + GUARD,), 0xCD, dtype=torch.uint8, device='cuda')
    n_ws = _lib.load().l3c_container_write_banded_workspace_bytes(arr, len(arr), B)
    assert n_ws == B * spi * 8
    ws = torch.full((n_ws + GUARD,), 0xCD, dtype=torch.uint8, device='cuda')
    pads = torch.from_numpy(np.asarray(padding, dtype=np.uint16).view(np.int16)).cuda()
    offsets = torch.from_numpy(offs).cuda()
    ops.call('l3c_container_write_banded', arr, len(arr), B, ops.ptr(pads), ops.ptr(offsets, torch.int64), ops.ptr(dst), ops.ptr(ws), n_ws,
             ops.stream())
    assert (ws.cpu().numpy()[n_ws:] == 0xCD).all(), 'write behind the workspace'
    got = dst.cpu().numpy()
    want = np.frombuffer(b''.join(files) + bytes([0xCD]) * GUARD, dtype=np.uint8)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, 'first differing byte {} of {} (got {:#x}, want {:#x}); {} differ'.format(bad[0], total, got[bad[0]], want[bad[0]], bad.size)
    for b in range(B):
        parsed = container.parse_banded(got[offs[b]:offs[b] + sizes[b]].tobytes())
        assert parsed.scales == scales and tuple(parsed.padding) == padding[b]
        for k, n in enumerate(lengths):
            assert np.array_equal(parsed.nbytes[k], n[b])


# ---- l3c_ac_band_intervals --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('S,N,L', [(5, 1000, 128),      # last band 104 symbols: a ragged last block
                                   (1, 64, 64),         # one band: full_out NULL
                                   (3, 4096, 64),
                                   (2, 130, 128),       # last band 2 symbols
                                   (7, 8192, 1024)])
def test_band_intervals_vs_numpy_gather(S, N, L):
    """ops.band_intervals (band_intervals_kernel) on random words against a gather by the layout of include/l3c_hip.h --
    word(s, t, r) = iv[(((t / 64) S + s) 2 + r) 64 + t % 64]; full band (s, j) is stream s (n - 1) + j of the first group, the last bands
    are the second -- for every word of every 64-symbol run the kernel writes (it copies whole runs: a ragged last block's unused words
    included).  The source is not modified."""
    from l3c_pytorch_amd import _lib, ops
    lib = _lib.load()
    words = lib.l3c_interval_words(S, N)
    blocks = -(-N // 64)
    assert words == blocks * S * 128
    rng = np.random.RandomState(S * 100000 + N + L)
    src = rng.randint(-2 ** 31, 2 ** 31, size=words, dtype=np.int64).astype(np.int32)
    iv = torch.from_numpy(src).cuda()
    groups = ops.band_intervals(iv, S, N, L)
    n, Lb = -(-N // L), L // 64
    last = N - (n - 1) * L
    run = src.reshape(blocks, S, 128)                      # [64-symbol block][stream][role, symbol]
    if n > 1:
        (full, full_streams, full_sym), groups = groups[0], groups[1:]
        assert (full_streams, full_sym) == (S * (n - 1), L) and full.numel() == lib.l3c_interval_words(S * (n - 1), L)
        want = np.empty((Lb, S * (n - 1), 128), dtype=np.int32)
        for s in range(S):
            for j in range(n - 1):
                want[:, s * (n - 1) + j] = run[j * Lb:(j + 1) * Lb, s]
        assert np.array_equal(full.cpu().numpy().reshape(want.shape), want)
    (tail, tail_streams, tail_sym), = groups
    assert (tail_streams, tail_sym) == (S, last) and tail.numel() == lib.l3c_interval_words(S, last)
    want = run[(n - 1) * Lb:].copy()                       # ((last + 63) / 64 blocks, S, 128)
    assert want.shape[0] == -(-last // 64)
    assert np.array_equal(tail.cpu().numpy().reshape(want.shape), want)
    assert np.array_equal(iv.cpu().numpy(), src)


# ---- l3c_container_read -----------------------------------------------------------------------------------------------------------

READ_LENGTHS = [0, 1, 2, 3, 4, 5, 8, 9] + list(range(16375, 16391)) + [40001]


def _read_case(lengths, aligns, gaps, rng):
    """A source buffer (0xEE, length a multiple of 4, ending with the last payload) with the payloads at positions of the given alignments,
    and the destination layout of bitcoding/upload.py -- (n + 3) / 4 * 4 + 4 bytes per stream -- with `gaps` bytes (multiples of 4) left
    free in front of each stream.  -> (source, src_off, dst_off, expected destination over 0xCD)"""
    src_off, dst_off, pos, dpos = [], [], 0, 0
    for n, a, g in zip(lengths, aligns, gaps):
        pos += (a - pos) % 4
        src_off.append(pos)
        pos += n
        dpos += g
        dst_off.append(dpos)
        dpos += (n + 3) // 4 * 4 + 4
    src = np.full((pos + 3) // 4 * 4, 0xEE, dtype=np.uint8)
    want = np.full(dpos + GUARD, 0xCD, dtype=np.uint8)
    for n, s, d in zip(lengths, src_off, dst_off):
        src[s:s + n] = rng.randint(0, 256, size=n)
        want[d:d + n] = src[s:s + n]
        want[d + n:d + (n + 3) // 4 * 4 + 4] = 0
    return src, np.asarray(src_off, dtype=np.int64), np.asarray(dst_off, dtype=np.int64), want


def _run_read(lengths, src, src_off, dst_off, want):
    from l3c_pytorch_amd import ops
    files = torch.from_numpy(src).cuda()
    dst = torch.full((want.size,), 0xCD, dtype=torch.uint8, device='cuda')
    ops.container_read(files, torch.from_numpy(src_off).cuda(), torch.from_numpy(dst_off).cuda(),
                       torch.from_numpy(np.asarray(lengths, dtype=np.int32)).cuda(), int(max(lengths)), dst)
    got = dst.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    if bad.size:
        s = int(np.searchsorted(dst_off, bad[0], side='right')) - 1
        raise AssertionError('destination byte {} (stream {}: {} bytes from source byte {}, at {}) is {:#x}, want {:#x}; {} bytes differ'.format(
            bad[0], s, lengths[s], src_off[s], dst_off[s], got[bad[0]], want[bad[0]], bad.size))
    assert np.array_equal(files.cpu().numpy(), src)


def test_container_read_every_alignment_and_slice_boundary():
    """l3c_container_read through ops.container_read: every length of READ_LENGTHS at every source alignment 0..3.  16377..16380 bytes pad
    to exactly one 4096-dword slice, 16381..16384 to one dword more, 40001 takes three slices.  Expected: the payload, zeros to the end of
    its padded length, 0xCD everywhere else -- the gaps left between some streams and the guard bytes at the end included."""
    rng = np.random.RandomState(5)
    lengths = [n for n in READ_LENGTHS for _ in range(4)]
    aligns = [a for _ in READ_LENGTHS for a in range(4)]
    order = rng.permutation(len(lengths))
    lengths, aligns = [lengths[i] for i in order], [aligns[i] for i in order]
    # ends on the aligned end of the source buffer, and starts misaligned: the word behind its last one would lie behind the buffer
    lengths.append(16383)
    aligns.append(1)
    gaps = [(0, 0, 4, 12)[i % 4] for i in range(len(lengths))]
    src, src_off, dst_off, want = _read_case(lengths, aligns, gaps, rng)
    # on the host, before anything is launched
    assert src.size % 4 == 0 and src_off[-1] + lengths[-1] == src.size
    assert {(int(o) & 3, n) for o, n in zip(src_off, lengths)} >= {(a, n) for a in range(4) for n in READ_LENGTHS}
    padded_words = {(n + 3) // 4 + 1 for n in lengths}
    assert {1, 2, 4095, 4096, 4097, 4098} <= padded_words and max(padded_words) > 2 * 4096
    assert (np.diff(dst_off) > (np.asarray(lengths[:-1]) + 3) // 4 * 4 + 4).any()
    _run_read(lengths, src, src_off, dst_off, want)


def test_container_read_more_streams_than_one_launch_takes():
    """65 535 + 3 streams of 0..9 bytes, back to back in the source: ops.container_read cuts them into launches of at most 65 535"""
    from l3c_pytorch_amd import ops
    rng = np.random.RandomState(6)
    S = ops.CONTAINER_READ_MAX_STREAMS + 3
    assert S == 65538
    lengths = rng.randint(0, 10, size=S)
    lengths[-3:] = (9, 0, 7)                              # the second launch: a full stream, an empty one, a misaligned one
    src_off = np.cumsum(lengths) - lengths
    padded = (lengths + 3) // 4 * 4 + 4
    dst_off = np.cumsum(padded) - padded
    src = np.full((int(lengths.sum()) + 3) // 4 * 4, 0xEE, dtype=np.uint8)
    src[:int(lengths.sum())] = rng.randint(0, 256, size=int(lengths.sum()))
    assert {(int(o) & 3, int(n)) for o, n in zip(src_off, lengths)} >= {(a, n) for a in range(4) for n in range(10)}
    want = np.full(int(padded.sum()) + GUARD, 0xCD, dtype=np.uint8)
    want[:int(padded.sum())] = 0
    idx = np.repeat(dst_off - src_off, lengths) + np.arange(int(lengths.sum()))    # destination position of every payload byte
    want[idx] = src[:int(lengths.sum())]
    _run_read([int(n) for n in lengths], src, src_off.astype(np.int64), dst_off.astype(np.int64), want)
