"""-m gpu: the two parity kernels (csrc/parity.hip: l3c_band_parity, l3c_u8_xor_spans) byte for byte against container.band_parity and
numpy's XOR, on synthetic coder outputs whose slots hold garbage behind every stream's length (the coder's do), with guard bytes behind
every output slot.  Milliseconds each: n = 16 bands per channel, rows of about 4 KiB."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd import ops  # noqa: E402
from l3c_pytorch_amd.bitcoding import container  # noqa: E402

LENS = [0, 1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 4097, 64]
N, H, W, L = 16, 32, 32, 64              # 16 bands of 64 symbols per channel
GUARD = 0xA5
_CASES = {}


def coder_output(B, stride_full, stride_last, seed, overrun=None, N=N):
    """Synthetic coder output of the finest record of B images, random bytes everywhere (behind the lengths too), lengths from LENS.
    Stream (b, c) = (0, 0): the longest member of group 0 at G = 3 (bands 0, 6, 12) comes first, of group 1 (1, 7, 13) last, of group 2
    (2, 8, 14) in the middle, 4097 bytes beside 64.  overrun: a (b, c, j) that reports L3C_AC_OVERRUN.  N: another band count than 16 (then
    without the three arranged groups).
    -> (groups on the device, lens (B, 3, N), payloads[b][c][j] bytes)."""
    key = (B, stride_full, stride_last, seed, overrun, N)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.RandomState(seed)
    lens = np.asarray([[[LENS[(5 * j + 3 * c + 7 * b + seed) % len(LENS)] for j in range(N)] for c in range(3)] for b in range(B)], dtype=np.int64)
    if N == 16:
        lens[0, 0, [0, 6, 12]] = (4097, 64, 5)
        lens[0, 0, [1, 7, 13]] = (64, 5, 4097)
        lens[0, 0, [2, 8, 14]] = (64, 4097, 255)
    full = rng.randint(0, 256, (B * 3 * (N - 1), stride_full)).astype(np.uint8)
    last = rng.randint(0, 256, (B * 3, stride_last)).astype(np.uint8)
    payloads = [[[(full[(b * 3 + c) * (N - 1) + j, :lens[b, c, j]] if j + 1 < N else last[b * 3 + c, :lens[b, c, j]]).tobytes() for j in range(N)]
                 for c in range(3)] for b in range(B)]
    reported = lens.copy()
    if overrun is not None:
        reported[overrun] = -1
    nb_full = reported[:, :, :N - 1].reshape(-1).astype(np.int32)
    nb_last = reported[:, :, N - 1].reshape(-1).astype(np.int32)
    groups = [(torch.from_numpy(full).cuda(), torch.from_numpy(nb_full).cuda()), (torch.from_numpy(last).cuda(), torch.from_numpy(nb_last).cuda())]
    _CASES[key] = (groups, lens, payloads)
    return _CASES[key]


def run_band_parity(groups, B, G, stride, n=N, hw=(H, W)):
    m = container.parity_groups(n, G)
    parity = torch.full((B, 3, m, stride), GUARD, dtype=torch.uint8, device='cuda')
    nbytes = torch.full((B, 3, m), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    ops.band_parity(B, hw[0], hw[1], L, groups, G, out=(parity, nbytes))
    torch.cuda.synchronize()
    return parity.cpu().numpy(), nbytes.cpu().numpy()


def check_band_parity(parity, nbytes, payloads, G, skip=()):
    B, _, m, stride = parity.shape
    for b in range(B):
        for c in range(3):
            want = container.band_parity(payloads[b][c], G)
            for g in range(m):
                slot = parity[b, c, g]
                if (b, c, g) in skip:
                    assert nbytes[b, c, g] == -1 and (slot == GUARD).all(), (b, c, g)
                    continue
                k = len(want[g])
                assert nbytes[b, c, g] == k, (b, c, g, nbytes[b, c, g], k)
                assert slot[:k].tobytes() == want[g], (b, c, g, k)
                k4 = (k + 3) // 4 * 4
                assert (slot[k:k4] == 0).all(), (b, c, g)                  # the members count as zero-extended: no garbage of theirs
                assert (slot[k4:] == GUARD).all(), (b, c, g, k)            # the rest of the slot is the caller's


@pytest.mark.parametrize('G', [1, 3, 4, 16])
@pytest.mark.parametrize('stride_full,stride_last,stride', [(4100, 4104, 4112), (4112, 4128, 4144)])      # rows at stride % 16 == 4 / 8 and == 0
def test_band_parity_matches_the_reference(G, stride_full, stride_last, stride):
    B = 2
    groups, lens, payloads = coder_output(B, stride_full, stride_last, 1)
    parity, nbytes = run_band_parity(groups, B, G, stride)
    assert parity.shape[2] == {1: 16, 3: 6, 4: 4, 16: 1}[G]
    check_band_parity(parity, nbytes, payloads, G)
    if G == 3:                                                          # the groups of (0, 0): longest first, last, in the middle
        assert list(nbytes[0, 0, :3]) == [4097, 4097, 4097]


@pytest.mark.parametrize('G', [12, 9])
def test_band_parity_of_more_members_than_one_batch(G):
    """A 32 x 24 plane, n = 12 bands.  G = 12: one group of 12 members, more than the eight the kernel takes at a time: a whole batch and a
    partly filled one; G = 9: m = 2 groups of 6."""
    groups, lens, payloads = coder_output(2, 4100, 4104, 5, N=12)
    parity, nbytes = run_band_parity(groups, 2, G, 4112, n=12, hw=(32, 24))
    assert parity.shape[2] == {12: 1, 9: 2}[G]
    check_band_parity(parity, nbytes, payloads, G)


def test_band_parity_of_one_image_and_of_one_band():
    groups, lens, payloads = coder_output(1, 4100, 4104, 2)
    parity, nbytes = run_band_parity(groups, 1, 3, 4112)
    check_band_parity(parity, nbytes, payloads, 3)
    # n == 1: no full-band group, every band its own parity (a copy, cut at its length)
    last = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (3, 136)).astype(np.uint8)).cuda()
    nb = torch.tensor([17, 0, 130], dtype=torch.int32, device='cuda')
    parity = torch.full((1, 3, 1, 144), GUARD, dtype=torch.uint8, device='cuda')
    nbytes = torch.zeros((1, 3, 1), dtype=torch.int32, device='cuda')
    ops.band_parity(1, 8, 8, 64, [(last, nb)], 1, out=(parity, nbytes))
    got, host = parity.cpu().numpy(), last.cpu().numpy()
    assert nbytes.view(-1).tolist() == [17, 0, 130]
    for c, k in enumerate((17, 0, 130)):
        assert (got[0, c, 0, :k] == host[c, :k]).all() and (got[0, c, 0, k:(k + 3) // 4 * 4] == 0).all() and (got[0, c, 0, (k + 3) // 4 * 4:] == GUARD).all()


def test_an_overrun_member_marks_its_group_and_is_not_read():
    B, G = 2, 4
    at = (1, 2, 5)                                                      # band 5 of B of image 1: group 5 % 4 = 1
    groups, lens, payloads = coder_output(B, 4100, 4104, 4, overrun=at)
    parity, nbytes = run_band_parity(groups, B, G, 4112)
    check_band_parity(parity, nbytes, payloads, G, skip={(1, 2, 1)})
    assert (nbytes == -1).sum() == 1


def run_xor(data, spans, first, slots, out_bytes):
    out = torch.full((out_bytes,), GUARD, dtype=torch.uint8, device='cuda')
    ops.u8_xor_spans(data, [o for o, _ in spans], [k for _, k in spans], first, out, [o for o, _ in slots], [k for _, k in slots])
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_xor(got, host, spans, first, slots):
    written = np.zeros(got.shape[0], dtype=bool)
    for g, (at, k) in enumerate(slots):
        want = np.zeros(k, dtype=np.uint8)
        for o, nb in spans[first[g]:first[g + 1]]:
            use = min(nb, k)
            want[:use] ^= host[o:o + use]
        end = (k + 3) // 4 * 4 + 4
        assert (got[at:at + k] == want).all(), (g, k)
        assert (got[at + k:at + end] == 0).all(), (g, k)                 # the zero tail the range decoders read
        written[at:at + end] = True
    assert (got[~written] == GUARD).all()                                # between and behind the slots: untouched


@pytest.mark.parametrize('shift', [0, 4])                               # sources and slots 16-byte aligned, or only 4
def test_xor_spans_matches_numpy(shift):
    rng = np.random.RandomState(7 + shift)
    host = rng.randint(0, 256, 96 * 1024).astype(np.uint8)
    data = torch.from_numpy(host).cuda()
    spans, first, slots, at, out_at = [], [0], [], 0, 16
    plan = [LENS[:5], LENS[5:9], [4097, 64, 5], [64, 5, 4097], [64, 4097, 255], [257], [0], [], [256, 256, 256, 256, 256, 256, 17], [4097] * 16]
    for g, members in enumerate(plan):
        for k in members:
            at = (at + 15) // 16 * 16 + shift
            spans.append((at, k))
            at += (k + 3) // 4 * 4
        first.append(len(spans))
        k = max(members) if members else 0
        if g == 8:
            k = 100                                                     # shorter than its members: they are cut
        if g == 1:
            k = 300                                                     # longer than its members: zero-extended
        out_at = (out_at + 15) // 16 * 16 + shift
        slots.append((out_at, k))
        out_at += (k + 3) // 4 * 4 + 4 + 32                             # a guard gap behind every slot
    assert at <= host.shape[0]
    got = run_xor(data, spans, first, slots, out_at + 64)
    check_xor(got, host, spans, first, slots)
    # a span may end with the buffer, a slot with `out`: nothing behind them is touched
    tail = host.shape[0] - 4096
    got = run_xor(data, [(tail, 4096), (tail + 4, 4092)], [0, 2], [(0, 4096)], 4096 + 4)
    check_xor(got, host, [(tail, 4096), (tail + 4, 4092)], [0, 2], [(0, 4096)])
    # no groups: nothing is launched
    out = torch.full((64,), GUARD, dtype=torch.uint8, device='cuda')
    ops.u8_xor_spans(data, [], [], [0], out, [], [])
    assert (out == GUARD).all()


@pytest.mark.parametrize('G', [3, 16])
def test_a_deleted_member_comes_back_from_the_parity(G):
    """l3c_u8_xor_spans of the parity from l3c_band_parity with the remaining members returns the deleted member's bytes, zero tail in place."""
    B = 2
    groups, lens, payloads = coder_output(B, 4100, 4104, 1)
    (full, _), (last, _) = groups
    m = container.parity_groups(N, G)
    stride = 4112
    parity = torch.full((B, 3, m, stride), GUARD, dtype=torch.uint8, device='cuda')
    nbytes = torch.zeros((B, 3, m), dtype=torch.int32, device='cuda')
    ops.band_parity(B, H, W, L, groups, G, out=(parity, nbytes))
    plen = nbytes.cpu().numpy()
    data = torch.cat([full.view(-1), last.view(-1), parity.view(-1)])
    last_at, parity_at = full.numel(), full.numel() + last.numel()

    def where(b, c, j):
        s = b * 3 + c
        return (s * (N - 1) + j) * 4100 if j + 1 < N else last_at + s * 4104
    spans, first, slots, deleted, out_at = [], [0], [], [], 0
    for b in range(B):
        for c in range(3):
            for g in range(m):
                gone = g + m * ((b + c) % len(range(g, N, m)))                          # another member in every (b, c)
                spans.append((parity_at + ((b * 3 + c) * m + g) * stride, int(plen[b, c, g])))
                spans += [(where(b, c, j), int(lens[b, c, j])) for j in range(g, N, m) if j != gone]
                first.append(len(spans))
                slots.append((out_at, int(lens[b, c, gone])))
                deleted.append(payloads[b][c][gone])
                out_at += (int(lens[b, c, gone]) + 3) // 4 * 4 + 4 + 12
    got = run_xor(data, spans, first, slots, out_at)
    for (at, k), want in zip(slots, deleted):
        assert got[at:at + k].tobytes() == want and (got[at + k:at + (k + 3) // 4 * 4 + 4] == 0).all()
        assert (got[at + (k + 3) // 4 * 4 + 4:at + (k + 3) // 4 * 4 + 16] == GUARD).all()
