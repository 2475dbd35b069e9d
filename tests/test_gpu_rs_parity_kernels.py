"""-m gpu: the two GF(2^8) kernels (csrc/parity.hip: l3c_band_parity_rs, l3c_u8_gf_spans) byte for byte against container.rs_parity and a
numpy table multiply, on the synthetic coder outputs of tests/test_gpu_parity_kernels.py (garbage behind every stream's length, guard bytes
around every output slot).  Milliseconds each: n = 16 bands per channel, rows of about 4 KiB."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd import ops  # noqa: E402
from l3c_pytorch_amd.bitcoding import container  # noqa: E402
from tests.test_gpu_parity_kernels import GUARD, H, L, LENS, N, W, check_xor, coder_output, run_band_parity, run_xor  # noqa: E402

TIMES = np.stack([container.gf_mul(np.arange(256, dtype=np.uint8), np.uint8(c)) for c in range(256)])       # TIMES[c][a] = c a


def run_band_parity_rs(groups, B, G, R, stride, n=N, hw=(H, W)):
    m = container.parity_groups(n, G)
    parity = torch.full((B, 3, m, R, stride), GUARD, dtype=torch.uint8, device='cuda')
    nbytes = torch.full((B, 3, m), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    ops.band_parity_rs(B, hw[0], hw[1], L, groups, G, R, out=(parity, nbytes))
    torch.cuda.synchronize()
    return parity.cpu().numpy(), nbytes.cpu().numpy()


def check_band_parity_rs(parity, nbytes, payloads, G, R, skip=()):
    B, _, m, _, stride = parity.shape
    for b in range(B):
        for c in range(3):
            want = container.rs_parity(payloads[b][c], G, R)
            for g in range(m):
                if (b, c, g) in skip:
                    assert nbytes[b, c, g] == -1 and (parity[b, c, g] == GUARD).all(), (b, c, g)
                    continue
                k = len(want[g][0])
                assert nbytes[b, c, g] == k, (b, c, g, nbytes[b, c, g], k)
                k4 = (k + 3) // 4 * 4
                for r in range(R):
                    slot = parity[b, c, g, r]
                    assert slot[:k].tobytes() == want[g][r], (b, c, g, r, k)
                    assert (slot[k:k4] == 0).all(), (b, c, g, r)               # the members count as zero-extended: no garbage of theirs
                    assert (slot[k4:] == GUARD).all(), (b, c, g, r, k)         # the rest of the slot is the caller's


@pytest.mark.parametrize('R', [2, 4])
@pytest.mark.parametrize('G', [1, 3, 4, 16])
@pytest.mark.parametrize('stride_full,stride_last,stride', [(4100, 4104, 4112), (4112, 4128, 4144)])      # rows at stride % 16 == 4 / 8 and == 0
def test_band_parity_rs_matches_the_reference(G, R, stride_full, stride_last, stride):
    B = 2
    groups, lens, payloads = coder_output(B, stride_full, stride_last, 1)
    parity, nbytes = run_band_parity_rs(groups, B, G, R, stride)
    assert parity.shape[2] == {1: 16, 3: 6, 4: 4, 16: 1}[G]
    check_band_parity_rs(parity, nbytes, payloads, G, R)
    if G == 3:                                                          # the groups of (0, 0): longest first, last, in the middle
        assert list(nbytes[0, 0, :3]) == [4097, 4097, 4097]
    # row 0 is ops.band_parity's slot, the lengths are its lengths
    xor, xor_nbytes = run_band_parity(groups, B, G, stride)
    assert (parity[:, :, :, 0] == xor).all() and (nbytes == xor_nbytes).all()


@pytest.mark.parametrize('R', [1, 3])
def test_band_parity_rs_of_one_and_three_rows(R):
    groups, lens, payloads = coder_output(2, 4100, 4104, 1)
    parity, nbytes = run_band_parity_rs(groups, 2, 4, R, 4112)
    check_band_parity_rs(parity, nbytes, payloads, 4, R)


@pytest.mark.parametrize('R', [2, 4])
@pytest.mark.parametrize('G', [12, 9])
def test_band_parity_rs_of_more_members_than_one_batch(G, R):
    """The case of tests/test_gpu_parity_kernels.py (n = 12 bands: a group of 12 members, a batch of eight and four on top; two groups of 6),
    where Horner's rule has to run through the empty members above the last one."""
    groups, lens, payloads = coder_output(2, 4100, 4104, 5, N=12)
    parity, nbytes = run_band_parity_rs(groups, 2, G, R, 4112, n=12, hw=(32, 24))
    assert parity.shape[2] == {12: 1, 9: 2}[G]
    check_band_parity_rs(parity, nbytes, payloads, G, R)


def test_band_parity_rs_of_one_band():
    # n == 1: no full-band group, every band its own group of one member: every row is a copy, cut at its length
    last = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (3, 136)).astype(np.uint8)).cuda()
    nb = torch.tensor([17, 0, 130], dtype=torch.int32, device='cuda')
    parity = torch.full((1, 3, 1, 4, 144), GUARD, dtype=torch.uint8, device='cuda')
    nbytes = torch.zeros((1, 3, 1), dtype=torch.int32, device='cuda')
    ops.band_parity_rs(1, 8, 8, 64, [(last, nb)], 1, 4, out=(parity, nbytes))
    got, host = parity.cpu().numpy(), last.cpu().numpy()
    assert nbytes.view(-1).tolist() == [17, 0, 130]
    for c, k in enumerate((17, 0, 130)):
        k4 = (k + 3) // 4 * 4
        for r in range(4):
            assert (got[0, c, 0, r, :k] == host[c, :k]).all() and (got[0, c, 0, r, k:k4] == 0).all() and (got[0, c, 0, r, k4:] == GUARD).all()


def test_an_overrun_member_marks_its_group_and_none_of_its_slots_is_written():
    B, G, R = 2, 4, 4
    at = (1, 2, 5)                                                      # band 5 of B of image 1: group 5 % 4 = 1
    groups, lens, payloads = coder_output(B, 4100, 4104, 4, overrun=at)
    parity, nbytes = run_band_parity_rs(groups, B, G, R, 4112)
    check_band_parity_rs(parity, nbytes, payloads, G, R, skip={(1, 2, 1)})
    assert (nbytes == -1).sum() == 1


def run_gf(data, spans, coefs, first, slots, out_bytes):
    out = torch.full((out_bytes,), GUARD, dtype=torch.uint8, device='cuda')
    ops.u8_gf_spans(data, [o for o, _ in spans], [k for _, k in spans], coefs, first, out, [o for o, _ in slots], [k for _, k in slots])
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_gf(got, host, spans, coefs, first, slots):
    written = np.zeros(got.shape[0], dtype=bool)
    for g, (at, k) in enumerate(slots):
        want = np.zeros(k, dtype=np.uint8)
        for (o, nb), c in zip(spans[first[g]:first[g + 1]], coefs[first[g]:first[g + 1]]):
            use = min(nb, k)
            want[:use] ^= TIMES[c][host[o:o + use]]
        end = (k + 3) // 4 * 4 + 4
        assert (got[at:at + k] == want).all(), (g, k)
        assert (got[at + k:at + end] == 0).all(), (g, k)                 # the zero tail the range decoders read
        written[at:at + end] = True
    assert (got[~written] == GUARD).all()                                # between and behind the slots: untouched


def _plan(shift):
    """The spans, groups and slots of tests/test_gpu_parity_kernels.py::test_xor_spans_matches_numpy."""
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
    return spans, first, slots, at, out_at


@pytest.mark.parametrize('shift', [0, 4])                               # sources and slots 16-byte aligned, or only 4
def test_gf_spans_matches_numpy(shift):
    rng = np.random.RandomState(7 + shift)
    host = rng.randint(0, 256, 96 * 1024).astype(np.uint8)
    data = torch.from_numpy(host).cuda()
    spans, first, slots, at, out_at = _plan(shift)                      # empty groups and one-member groups among them
    assert at <= host.shape[0]
    special = [0, 1, 2, 0x80, 0xFF, 0x1D, 0x8E]
    coefs = [special[k % len(special)] if k % 3 else int(rng.randint(0, 256)) for k in range(len(spans))]
    coefs[first[5]] = 0xFF                                              # the one-member group: a scaled copy
    got = run_gf(data, spans, coefs, first, slots, out_at + 64)
    check_gf(got, host, spans, coefs, first, slots)
    # every coefficient 1: l3c_u8_xor_spans' bytes, guard bytes included
    ones = [1] * len(spans)
    got = run_gf(data, spans, ones, first, slots, out_at + 64)
    check_xor(got, host, spans, first, slots)
    assert (got == run_xor(data, spans, first, slots, out_at + 64)).all()
    # every coefficient 0: zeros, and a span that may not be read at all is not
    got = run_gf(data, spans, [0] * len(spans), first, slots, out_at + 64)
    check_gf(got, host, spans, [0] * len(spans), first, slots)
    # a span may end with the buffer, a slot with `out`: nothing behind them is touched
    tail = host.shape[0] - 4096
    got = run_gf(data, [(tail, 4096), (tail + 4, 4092)], [2, 0x80], [0, 2], [(0, 4096)], 4096 + 4)
    check_gf(got, host, [(tail, 4096), (tail + 4, 4092)], [2, 0x80], [0, 2], [(0, 4096)])
    # no groups: nothing is launched
    out = torch.full((64,), GUARD, dtype=torch.uint8, device='cuda')
    ops.u8_gf_spans(data, [], [], [], [0], out, [], [])
    assert (out == GUARD).all()
    with pytest.raises(ValueError, match='one coefficient'):
        ops.u8_gf_spans(data, [0], [4], [256], [0, 1], out, [0], [4])
    with pytest.raises(ValueError, match='one coefficient'):
        ops.u8_gf_spans(data, [0], [4], [], [0, 1], out, [0], [4])


@pytest.mark.parametrize('G,R,t', [(4, 2, 2), (4, 4, 2), (16, 4, 4), (3, 2, 1), (16, 2, 2)])
def test_deleted_members_come_back_from_the_rows(G, R, t):
    """t members of every group deleted: l3c_u8_gf_spans of the rows r0 .. r0 + t - 1 from l3c_band_parity_rs and the remaining members, with
    container.rs_repair_coefficients' weights, returns the deleted members' bytes, zero tail in place -- for r0 = 0 and for the last window."""
    B = 2
    groups, lens, payloads = coder_output(B, 4100, 4104, 1)
    (full, _), (last, _) = groups
    m = container.parity_groups(N, G)
    stride = 4112
    parity = torch.full((B, 3, m, R, stride), GUARD, dtype=torch.uint8, device='cuda')
    nbytes = torch.zeros((B, 3, m), dtype=torch.int32, device='cuda')
    ops.band_parity_rs(B, H, W, L, groups, G, R, out=(parity, nbytes))
    plen = nbytes.cpu().numpy()
    data = torch.cat([full.view(-1), last.view(-1), parity.view(-1)])
    last_at, parity_at = full.numel(), full.numel() + last.numel()

    def where(b, c, j):
        s = b * 3 + c
        return (s * (N - 1) + j) * 4100 if j + 1 < N else last_at + s * 4104
    for r0 in sorted({0, R - t}):
        spans, coefs, first, slots, deleted, out_at = [], [], [0], [], [], 0
        for b in range(B):
            for c in range(3):
                for g in range(m):
                    count = len(range(g, N, m))
                    gone = sorted({(b + c + 5 * i) % count for i in range(t)})             # other members in every (b, c)
                    present = [k for k in range(count) if k not in gone]
                    rows_at = [(parity_at + (((b * 3 + c) * m + g) * R + r) * stride, int(plen[b, c, g])) for r in range(r0, r0 + len(gone))]
                    solved = container.rs_repair_coefficients(gone, present, r0)
                    for e, (rows, weights) in zip(gone, solved):
                        spans += rows_at + [(where(b, c, g + k * m), int(lens[b, c, g + k * m])) for k in present]
                        coefs += list(rows) + list(weights)
                        first.append(len(spans))
                        j = g + e * m
                        slots.append((out_at, int(lens[b, c, j])))
                        deleted.append(payloads[b][c][j])
                        out_at += (int(lens[b, c, j]) + 3) // 4 * 4 + 4 + 12
        got = run_gf(data, spans, coefs, first, slots, out_at)
        for (at, k), want in zip(slots, deleted):
            assert got[at:at + k].tobytes() == want and (got[at + k:at + (k + 3) // 4 * 4 + 4] == 0).all(), (r0, at, k)
            assert (got[at + (k + 3) // 4 * 4 + 4:at + (k + 3) // 4 * 4 + 16] == GUARD).all()
