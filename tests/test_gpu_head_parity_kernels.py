"""-m gpu: the two kernels behind the head part of an 'L3CH' section -- l3c_head_parity (ops.head_parity) against container.rs_parity and
l3c_band_payload_crc32 (ops.band_payload_crc32) against zlib.crc32 -- on synthetic l3c_banded_scale buffers: 1 to 3 records per call,
C in {1, 5}, n in {1, 2, 7}, B in {1, 3}, G in {1, 4, 255 (clipped to n)}, R in {1, 2, 4}; payload lengths 0, 1, 3, 4, 5, 15, 16, 17, 4095,
4096, 4097 and the full stride; coder strides that are multiples of 4 but not of 16; garbage behind every length inside its slot; an
overrun member; guard bytes in front of and behind every output."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd import ops  # noqa: E402
from l3c_pytorch_amd.bitcoding import container  # noqa: E402

STRIDE_FULL, STRIDE_LAST = 4100, 20                      # multiples of 4, not of 16
LENS = [0, 1, 3, 4, 5, 15, 16, 17, 4095, 4096, 4097, STRIDE_FULL]
GUARD, FILL = 64, 0xAB
OVERRUN = -1                                             # L3C_AC_OVERRUN as int32

# (records [(C, n)], B, G, R, the overrun member (record, b, c, j) or None): every value the module's docstring names, each case two launches
CASES = [
    ([(5, 7)], 1, 4, 2, None),
    ([(1, 1)], 1, 1, 1, None),
    ([(1, 2), (5, 7)], 3, 255, 4, None),
    ([(5, 1), (1, 7), (5, 2)], 3, 4, 1, None),
    ([(5, 7), (1, 2)], 1, 1, 4, None),
    ([(5, 7), (5, 2), (1, 1)], 3, 4, 2, (0, 2, 3, 5)),
    ([(1, 7)], 3, 255, 2, (0, 1, 0, 6)),
]
_CACHE = {}


def _record(rng, B, C, n, first_len):
    """One record of n bands per channel: the two coder groups filled with garbage, every payload's length from LENS in turn (the last
    band's from those that fit its shorter stride) -> ((C, H, W, L, groups), host payloads [b][c][j])."""
    groups, hosts = [], []
    for rows, stride in ([(B * C * (n - 1), STRIDE_FULL)] if n > 1 else []) + [(B * C, STRIDE_LAST)]:
        out = torch.from_numpy(rng.randint(0, 256, size=(rows, stride), dtype=np.uint8))
        fits = [v for v in LENS if v <= stride]
        nb = np.array([fits[(first_len + 5 * i) % len(fits)] for i in range(rows)], dtype=np.int32)
        groups.append((out.cuda(), torch.from_numpy(nb).cuda()))
        hosts.append((out.numpy(), nb))

    def payload(b, c, j):
        out, nb = hosts[0] if j + 1 < n else hosts[-1]
        i = (b * C + c) * (n - 1) + j if j + 1 < n else b * C + c
        return out[i, :nb[i]].tobytes()
    return (C, 8, 8 * n, 64, groups), [[[payload(b, c, j) for j in range(n)] for c in range(C)] for b in range(B)]


def _case(i):
    """The records of CASES[i] on the device and their payloads on the host, built once and shared by the two tests."""
    if i not in _CACHE:
        shapes, B, G, R, overrun = CASES[i]
        rng = np.random.RandomState(i)
        built = [_record(rng, B, C, n, 3 * k + i) for k, (C, n) in enumerate(shapes)]
        if overrun is not None:
            k, b, c, j = overrun
            C, n = shapes[k]
            full = j + 1 < n
            built[k][0][4][0 if full else -1][1][(b * C + c) * (n - 1) + j if full else b * C + c] = OVERRUN
        _CACHE[i] = ([s for s, _ in built], [p for _, p in built])
    return _CACHE[i]


def _guarded(n, dtype):
    """A tensor of n elements between two guards, all FILL bytes -> (the whole, the view the kernel writes)."""
    per = torch.empty(0, dtype=dtype).element_size()
    whole = torch.full(((2 * GUARD + n * per),), FILL, dtype=torch.uint8, device='cuda')
    return whole, whole[GUARD:GUARD + n * per].view(dtype)


@pytest.mark.parametrize('i', range(len(CASES)))
def test_head_parity_is_rs_parity_of_every_record(i):
    shapes, B, G, R, overrun = CASES[i]
    scales, payloads = _case(i)
    layout, offsets, stride, total, first = ops.head_parity_layout(B, scales, G, R)
    assert stride % 16 == 0 and stride >= STRIDE_LAST and [s[:2] for s in layout] == shapes
    whole_p, parity = _guarded(total, torch.uint8)
    whole_n, nbytes = _guarded(first[-1], torch.int32)
    assert ops.head_parity(B, scales, G, R, out=(parity, nbytes))[0] is parity
    torch.cuda.synchronize()
    for whole, size in ((whole_p, total), (whole_n, 4 * first[-1])):
        host = whole.cpu().numpy()
        assert (host[:GUARD] == FILL).all() and (host[GUARD + size:] == FILL).all()
    got, lens = parity.cpu().numpy(), nbytes.cpu().numpy()
    marked = 0
    for k, ((C, n, m), off, f) in enumerate(zip(layout, offsets, first)):
        Gk = min(G, n)
        assert m == -(-n // Gk)
        slots = got[off:off + B * C * m * R * stride].reshape(B, C, m, R, stride)
        lk = lens[f:f + B * C * m].reshape(B, C, m)
        for b in range(B):
            for c in range(C):
                hit = overrun is not None and overrun[:3] == (k, b, c)
                want = container.rs_parity(payloads[k][b][c], Gk, R)
                for g in range(m):
                    if hit and overrun[3] % m == g:                     # the group is marked and none of its slots is written
                        assert lk[b, c, g] == OVERRUN and (slots[b, c, g] == FILL).all()
                        marked += 1
                        continue
                    size = len(want[g][0])
                    assert lk[b, c, g] == size == max(len(p) for p in payloads[k][b][c][g::m])
                    end4 = (size + 3) // 4 * 4
                    for r in range(R):
                        assert slots[b, c, g, r, :size].tobytes() == want[g][r], (k, b, c, g, r)
                        assert (slots[b, c, g, r, size:end4] == 0).all() and (slots[b, c, g, r, end4:] == FILL).all(), (k, b, c, g, r)
    assert marked == (overrun is not None)


@pytest.mark.parametrize('i', range(len(CASES)))
def test_band_payload_crc32_is_zlib_on_every_payload(i):
    shapes, B, G, R, overrun = CASES[i]
    scales, payloads = _case(i)
    total = sum(B * C * n for C, n in shapes)
    whole, out = _guarded(total, torch.int32)
    assert ops.band_payload_crc32(B, scales, out=out) is out
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + 4 * total:] == FILL).all()
    got, at = out.cpu().numpy().view(np.uint32), 0
    for k, (C, n) in enumerate(shapes):
        want = np.array([[[zlib.crc32(p) for p in ch] for ch in img] for img in payloads[k]], dtype=np.uint32)
        if overrun is not None and overrun[0] == k:
            want[overrun[1:]] = 0                                       # an overrun band gives 0 (its file is refused anyway)
        assert np.array_equal(got[at:at + B * C * n].reshape(B, C, n), want), k
        at += B * C * n
    assert at == total


def test_the_lengths_cover_every_value_and_the_empty_payload_hashes_to_zero():
    seen = set()
    for i in range(len(CASES)):
        for rec in _case(i)[1]:
            seen |= {len(p) for img in rec for ch in img for p in ch}
    assert seen >= set(LENS), sorted(set(LENS) - seen)
    assert zlib.crc32(b'') == 0


def test_the_crc_words_do_not_depend_on_how_the_records_are_split_over_calls():
    """Three records in one call against one call per record: another grid, another place of every payload in it, the same words."""
    shapes, B, _, _, _ = CASES[3]
    scales, _ = _case(3)
    together = ops.band_payload_crc32(B, scales).cpu().numpy()
    apart = np.concatenate([ops.band_payload_crc32(B, [s]).cpu().numpy() for s in scales])
    assert np.array_equal(together, apart)
