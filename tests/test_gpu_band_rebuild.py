"""-m gpu: l3c_band_rebuild (csrc/parity.hip) byte for byte against numpy GF(2^8) arithmetic (container.gf_mul), and against l3c_u8_gf_spans
where both can run.  One launch covers the grid: row sources at every byte alignment, output lengths around the 4096-byte tile, t = 1..4
outputs of unequal length, 0 .. 17 members (the fold takes eight at a time), coefficients 0 and 1 among random ones, a random pattern
everywhere outside the slots that must come back unchanged, and a row span that ends with rows_bytes.  Milliseconds each."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd import ops  # noqa: E402
from l3c_pytorch_amd.bitcoding import container  # noqa: E402

TIMES = np.stack([container.gf_mul(np.arange(256, dtype=np.uint8), np.uint8(c)) for c in range(256)])       # TIMES[c][a] = c a
LENGTHS = [0, 1, 3, 4, 15, 16, 17, 4095, 4096, 4097, 8193]
MEMBERS = [0, 1, 8, 9, 17]


def slot_bytes(k):
    return (k + 3) // 4 * 4 + 4


class Case(object):
    """Tables of one l3c_band_rebuild call, built group by group: the rows back to back at arbitrary offsets, the members and the slots in
    one buffer with gaps between them."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.src, self.coefs, self.groups, self.row_at, self.mem_at = [], [], [], 0, 16

    def add(self, out_lengths, n_rows, n_members, align, coef=None, slot_shift=0):
        rng, first, longest = self.rng, len(self.src), max(out_lengths)
        for k in range(n_rows + n_members):
            # lengths around the longest output: shorter (zero-extended), equal, longer (cut); an empty source now and then
            nb = int(max(0, longest + rng.choice([-9, -1, 0, 0, 1, 7, 40]))) if rng.randint(0, 9) else 0
            if k < n_rows:
                at = self.row_at + (align - self.row_at) % 4
                self.row_at = at + nb
            else:
                at = (self.mem_at + 15) // 16 * 16 + 4 * int(rng.randint(0, 4))
                self.mem_at = at + (nb + 3) // 4 * 4
            self.src.append((at, nb))
            c = [int(v) for v in rng.randint(0, 256, 4)]
            for e in range(4):
                if rng.randint(0, 4) == 0:
                    c[e] = int(rng.randint(0, 2))                    # 0 and 1 among them
            if rng.randint(0, 7) == 0:
                c = [0, 0, 0, 0]                                        # a source that may not be read at all
            self.coefs.append(c if coef is None else coef)
        outs = []
        for nb in out_lengths:
            at = (self.mem_at + 15) // 16 * 16 + slot_shift
            outs.append((at, nb))
            self.mem_at = at + slot_bytes(nb) + 12                      # a guard gap behind every slot
        self.groups.append((first, n_rows, n_members, outs))

    def run(self, rows_tail=0):
        """-> (the members buffer as it was, as it is, the rows); rows_bytes is the end of the last row span + rows_tail."""
        rows = self.rng.randint(0, 256, self.row_at + rows_tail).astype(np.uint8)
        before = self.rng.randint(0, 256, self.mem_at + 64).astype(np.uint8)
        members = torch.from_numpy(before).cuda()
        ops.band_rebuild(torch.from_numpy(rows).cuda(), members, [a for a, _ in self.src], [n for _, n in self.src], self.coefs, self.groups)
        torch.cuda.synchronize()
        return before, members.cpu().numpy(), rows

    def check(self, before, after, rows):
        written = np.zeros(after.shape[0], dtype=bool)
        for q, (first, n_rows, n_members, outs) in enumerate(self.groups):
            for e, (at, k) in enumerate(outs):
                want = np.zeros(k, dtype=np.uint8)
                for s in range(first, first + n_rows + n_members):
                    o, nb = self.src[s]
                    use = min(nb, k)
                    data = rows if s < first + n_rows else before
                    want[:use] ^= TIMES[self.coefs[s][e]][data[o:o + use]]
                assert (after[at:at + k] == want).all(), (q, e, k, n_rows, n_members)
                assert (after[at + k:at + slot_bytes(k)] == 0).all(), (q, e, k)        # the zero tail the range decoders read
                written[at:at + slot_bytes(k)] = True
        assert (after[~written] == before[~written]).all()                             # the sources, the gaps, the tail: untouched


def grid(seed, slot_shift):
    case, i = Case(seed), 0
    for longest in LENGTHS:
        for t in (1, 2, 3, 4):
            for n_members in MEMBERS:
                others = [longest // 2, max(longest - 5, 0), longest + 3 if longest < 4096 else longest - 1]
                case.add([longest] + others[:t - 1], 1 + i % 4, n_members, i % 4, slot_shift=slot_shift)
                i += 1
    return case


@pytest.mark.parametrize('slot_shift', [0, 4])                       # members and slots 16-byte aligned, or only 4
def test_band_rebuild_matches_numpy_over_the_grid(slot_shift):
    case = grid(3 + slot_shift, slot_shift)
    assert len(case.groups) == len(LENGTHS) * 4 * len(MEMBERS)
    row_offsets = [case.src[s][0] for first, n_rows, _, _ in case.groups for s in range(first, first + n_rows) if case.src[s][1]]
    assert {a % 4 for a in row_offsets} == {0, 1, 2, 3}
    before, after, rows = case.run()                                 # the last row span ends with rows_bytes
    case.check(before, after, rows)


def test_rows_at_every_alignment_with_every_tail_length():
    """One group per (alignment, length % 4, rows_bytes - end): a row's first and last dword hold bytes that are not the row's."""
    for tail in (0, 1, 2, 3):
        case = Case(40 + tail)
        for align in range(4):
            for nb in (1, 2, 3, 4, 5, 6, 7, 8, 21, 4093, 4094, 4096, 4099):
                case.add([nb], 2, 1, align, coef=[1, 1, 1, 1])
        before, after, rows = case.run(rows_tail=tail)
        case.check(before, after, rows)


def test_coefficient_one_everywhere_is_the_xor_and_zero_everywhere_is_zeros():
    for coef in ([1, 1, 1, 1], [0, 0, 0, 0], [2, 0x80, 0xFF, 0x1D]):
        case = Case(7)
        for n_members in (0, 3, 8, 11):
            case.add([4097, 100, 4096, 31], 4, n_members, 3, coef=coef)
        before, after, rows = case.run()
        case.check(before, after, rows)


def test_aligned_inputs_give_the_bytes_of_t_gf_spans_groups():
    """On 4-byte aligned rows the existing kernel can run: t output groups of l3c_u8_gf_spans over the same spans, the same bytes."""
    case = Case(11)
    for t, n_members in ((1, 5), (2, 9), (4, 17), (3, 0)):
        case.add([4097, 2000, 4096, 17][:t], t, n_members, 0)
    before, after, rows = case.run(rows_tail=(-case.row_at) % 4)
    case.check(before, after, rows)
    data = torch.from_numpy(np.concatenate([rows, before])).cuda()      # one buffer for the old kernel: the rows, then the members
    shift = rows.shape[0]
    assert shift % 4 == 0
    offs, lens, coefs, first, slots = [], [], [], [0], []
    for g, (k0, n_rows, n_members, outs) in enumerate(case.groups):
        for e, (at, nb) in enumerate(outs):
            for s in range(k0, k0 + n_rows + n_members):
                offs.append(case.src[s][0] + (0 if s < k0 + n_rows else shift))
                lens.append(case.src[s][1])
                coefs.append(case.coefs[s][e])
            first.append(len(offs))
            slots.append((at, nb))
    out = torch.from_numpy(before.copy()).cuda()
    ops.u8_gf_spans(data, offs, lens, coefs, first, out, [a for a, _ in slots], [n for _, n in slots])
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == after).all()


def test_no_groups_launch_nothing_and_bad_tables_are_refused():
    from l3c_pytorch_amd import _lib
    rows, members = torch.zeros(64, dtype=torch.uint8, device='cuda'), torch.full((256,), 0xA5, dtype=torch.uint8, device='cuda')
    assert ops.band_rebuild(rows, members, [], [], [], []) is members and (members == 0xA5).all()
    with pytest.raises(_lib.L3CError, match='overlap'):
        ops.band_rebuild(rows, members, [1, 0], [9, 16], [[1, 0, 0, 0]] * 2, [(0, 1, 1, [(8, 4)])])
    with pytest.raises(ValueError, match='four coefficients'):
        ops.band_rebuild(rows, members, [1, 0], [9, 16], [[1, 0, 0, 256]] * 2, [(0, 1, 1, [(64, 4)])])
    with pytest.raises(ValueError, match='outputs'):
        ops.band_rebuild(rows, members, [1, 0], [9, 16], [[1, 0, 0, 0]] * 2, [(0, 1, 1, [])])
    torch.cuda.synchronize()
    assert (members == 0xA5).all()
