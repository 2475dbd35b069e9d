"""-m gpu: NativeCodec.decode_repair beside Bitcoding.decode_repair -- the same pixels and the same RepairInfo -- on every damage case of
tests/test_gpu_repair.py, tests/test_gpu_rs_repair.py and tests/test_gpu_head_repair.py (320x88, K = 16: L = 1792, n = 16 bands per channel,
G = 4), and the round call on its own against zlib.crc32 of the input's bands.  The native path rebuilds inside l3c_decode_repair_round
(ONE l3c_band_rebuild per round): no l3c_u8_gf_spans / l3c_u8_xor_spans call is made from Python."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd import _lib  # noqa: E402
from l3c_pytorch_amd.bitcoding import container  # noqa: E402
from l3c_pytorch_amd.native_codec import parse_round  # noqa: E402
from tests.test_gpu_band_seal import native  # noqa: E402
from tests.test_gpu_head_repair import coder, files as head_files, hurt  # noqa: E402
from tests.test_gpu_repair import damaged as damaged_p, parity_bitcoding, with_parity  # noqa: E402
from tests.test_gpu_rs_repair import K, L, N, damaged, rs_bitcoding, with_rs  # noqa: E402
from tests.test_gpu_salvage import NamedCalls  # noqa: E402


def head_key(heads):
    return None if heads is None else [None if h is None else (h.framing, list(h.repaired), list(h.failed), h.section_damaged) for h in heads]


def both(files, bc, monkeypatch=None):
    """decode_repair through both codecs: the same pixels, paddings and info -> (pixels, info of the native codec, its library calls)."""
    a, pa, ia = bc.decode_repair(files)
    calls = NamedCalls(monkeypatch) if monkeypatch is not None else None
    b, pb, ib = native(K).decode_repair(files)
    assert a.dtype == b.dtype == torch.uint8 and torch.equal(a, b)
    assert [tuple(p) for p in pa] == [tuple(p) for p in pb]
    assert ia.repaired == ib.repaired and ia.rows == ib.rows and ia.rounds == ib.rounds and ia.salvage == ib.salvage, (ia, ib)
    assert ia.files == ib.files and head_key(ia.head) == head_key(ib.head)
    assert ia.line() == ib.line()
    names = calls.names if calls is not None else None
    if names is not None:
        assert names.count('l3c_decode_repair_round') == ib.rounds
        assert not {'l3c_u8_gf_spans', 'l3c_u8_xor_spans', 'l3c_decode_rgb_entries', 'l3c_u8_crc32_spans'} & set(names)
    return b, ib, names


def repaired(info, want, rounds=None):
    """A repairing case: a silently skipped repair cannot pass."""
    assert info.rounds >= 1 and info.repaired and info.repaired == want, info
    assert rounds is None or info.rounds == rounds
    assert info.salvage.concealed == {} and info.salvage.lost == []


@pytest.mark.parametrize('c', [0, 1, 2])
def test_one_payload_of_an_l3cp_file(c, monkeypatch):
    x, v3, _ = with_parity(1, 320, 88)
    got, info, names = both([damaged_p(v3[0], [(c, 3)])], parity_bitcoding(), monkeypatch)
    repaired(info, {0: [(c, 3)]}, 1)
    assert torch.equal(got, x) and info.files[0] == v3[0] and info.rows == {0: (61, 82)} and 'l3c_dmll_conceal' not in names


def test_two_erasures_of_one_group_at_two_rows(monkeypatch):
    x, q = with_rs()
    got, info, _ = both([damaged(q[0], [(0, 3), (0, 7)])], rs_bitcoding(), monkeypatch)
    repaired(info, {0: [(0, 3), (0, 7)]}, 1)
    assert torch.equal(got, x) and info.files[0] == q[0]
    got, info, _ = both([damaged(q[0], [(0, 3), (0, 4)])], rs_bitcoding())          # adjacent bands: two groups, one round
    repaired(info, {0: [(0, 3), (0, 4)]}, 1)


def test_four_erasures_of_one_group_of_sixteen_at_four_rows(monkeypatch):
    x, four = with_rs(4, 64)
    streams = [(0, 3), (0, 7), (0, 8), (0, 11)]
    got, info, _ = both([damaged(four[0], streams)], rs_bitcoding(4, 64), monkeypatch)
    repaired(info, {0: streams}, 1)
    assert torch.equal(got, x) and info.files[0] == four[0]


def test_one_erasure_more_than_rows_is_concealed(monkeypatch):
    x, q = with_rs()
    got, info, names = both([damaged(q[0], [(0, 3), (0, 7), (0, 11)])], rs_bitcoding(), monkeypatch)
    assert info.repaired == {} and info.rounds == 0 and info.files == [None] and {j for _, j in info.salvage.concealed[0]} == {3, 7, 11}
    assert 'l3c_dmll_conceal' in names


def test_a_damaged_row_takes_the_second_window(monkeypatch):
    x, q = with_rs()
    got, info, _ = both([damaged(q[0], [(0, 3)], rows=[(0, 3, 0)])], rs_bitcoding(), monkeypatch)
    repaired(info, {0: [(0, 3)]}, 2)
    assert torch.equal(got, x) and info.files[0] == damaged(q[0], rows=[(0, 3, 0)])
    # both rows complemented: two windows tried, then concealed
    got, info, _ = both([damaged(q[0], [(0, 3)], rows=[(0, 3, 0), (0, 3, 1)])], rs_bitcoding())
    assert info.repaired == {} and info.rounds == 2 and {j for _, j in info.salvage.concealed[0]} == {3}


def test_two_channels_of_one_position_take_two_rounds(monkeypatch):
    x, q = with_rs()
    got, info, _ = both([damaged(q[0], [(0, 5), (2, 5), (0, 9)])], rs_bitcoding(), monkeypatch)
    repaired(info, {0: [(0, 5), (0, 9), (2, 5)]}, 2)
    assert torch.equal(got, x) and info.files[0] == q[0]


def test_a_batch_of_an_l3cp_and_an_l3cq_file(monkeypatch):
    x, q = with_rs()
    _, v3, _ = with_parity(1, 320, 88)
    got, info, _ = both([damaged_p(v3[0], [(1, 6)]), damaged(q[0], [(0, 3), (0, 7)])], rs_bitcoding(), monkeypatch)
    repaired(info, {0: [(1, 6)], 1: [(0, 3), (0, 7)]}, 1)
    assert torch.equal(got[0:1], x) and torch.equal(got[1:2], x) and info.files == [v3[0], q[0]]


def test_a_batch_of_padded_images_one_damaged(monkeypatch):
    x, v3, padding = with_parity(2, 317, 83)
    got, info, _ = both([v3[0], damaged_p(v3[1], [(1, 0), (2, 15)])], parity_bitcoding(), monkeypatch)
    repaired(info, {1: [(1, 0), (2, 15)]})
    left, right, top, bottom = padding
    assert torch.equal(got[:, :, top:320 - bottom, left:88 - right], x) and info.files == [None, v3[1]] and info.rows == {1: (0, 317)}


def test_a_coarse_payload_healed_on_the_host_and_a_finest_band_on_the_device(monkeypatch):
    x, vh = head_files()
    got, info, _ = both([hurt(vh[0], [], [(2, 4, 2), (3, 0, 7)])], coder(), monkeypatch)
    repaired(info, {0: [(0, 7)]}, 1)
    assert torch.equal(got, x) and info.files[0] == vh[0] and info.head[0].repaired == [(2, 4, 2)]
    got, info, _ = both([hurt(vh[0], [], [(1, 3, 5)])], coder())                      # the head alone: no round, the file healed
    assert torch.equal(got, x) and info.rounds == 0 and info.files[0] == vh[0] and info.repaired == {}


def test_an_intact_file_makes_the_calls_of_decode_salvage(monkeypatch):
    x, q = with_rs()
    nat = native(K)
    nat.decode_salvage(q)
    calls = NamedCalls(monkeypatch)
    want, _, salvage = nat.decode_salvage(q)
    names, calls.names = calls.names, []
    got, _, info = nat.decode_repair(q)
    assert calls.names == names and 'l3c_u8_crc32_bands' in names and 'l3c_decode_repair_round' not in names
    assert torch.equal(got, x) and torch.equal(got, want)
    assert info.repaired == {} and info.rows == {} and info.files == [None] and info.rounds == 0 and info.salvage == salvage and info.line() == 'seal: ok'
    # a band-sealed file without parity and an unsealed file: decode_salvage
    from tests.test_gpu_region import encoded
    from tests.test_gpu_repair import damaged_like_v2
    _, v2, _ = encoded(K, 1, 320, 88, seal='bands')
    bad = damaged_like_v2(v2[0], 0, 3)
    both([bad], rs_bitcoding())
    both(encoded(K, 1, 320, 88)[1], rs_bitcoding())


def test_the_round_call_on_a_blob_planned_by_hand():
    """The pieces decode_repair is made of, one by one: the decode with its workspace kept, band words written by hand (the table's, but for
    the two damaged bands), l3c_repair_round_plan, ONE l3c_decode_repair_round -- its CRC words are zlib.crc32 of the INPUT's bands, and the
    rebuilt payloads lie in the stream area where l3c_decode_plan_banded_stream says."""
    lib = _lib.load()
    x, q = with_rs()
    nat = native(K)
    bad = damaged(q[0], [(0, 3), (0, 7)])
    body, seal = nat._split_seal(bad)
    kept = {'plan': None}
    pixels, pads = nat._decode_bodies([body], None, None, kept)
    words = seal.band_crcs.copy().reshape(1, 3, N)
    frame = x.cpu().numpy().reshape(3, -1)
    assert all(zlib.crc32(frame[c, j * L:(j + 1) * L].tobytes()) == int(words[0, c, j]) for c in range(3) for j in range(N))
    words[0, 0, 3] ^= 1
    words[0, 0, 7] ^= 1
    file = np.frombuffer(bad, dtype=np.uint8)
    rows = torch.from_numpy(np.concatenate([np.zeros(3, dtype=np.uint8), file[len(body):]])).cuda()      # the section at an odd place of `rows`
    section_at = np.asarray([3], dtype=np.int64)
    plan = kept['plan']
    cap = lib.l3c_repair_round_plan_bytes(nat._cfg_ref, plan.ctypes.data)
    blob, n_groups = np.zeros(cap // 8, dtype=np.int64), ctypes.c_int64()
    ptrs, sizes = (ctypes.c_void_p * 1)(file.ctypes.data), np.asarray([file.size], dtype=np.int64)
    assert lib.l3c_repair_round_plan(nat._cfg_ref, plan.ctypes.data, ptrs, sizes.ctypes.data, words.ctypes.data, section_at.ctypes.data, None, 0,
                                     blob.ctypes.data, cap, ctypes.byref(n_groups)) == 0 and n_groups.value == 1
    r = parse_round(blob.tobytes())
    assert [tuple(p) for p in r['pos']] == [(0, 3), (0, 7)] and r['S'] == 2 and int(r['src'][0]['offset']) % 4 != 0
    blob_d = torch.from_numpy(blob[:r['bytes'] // 8]).cuda()
    ws, sym = kept['ws'], kept['sym']
    rws = torch.empty(lib.l3c_decode_repair_round_workspace_bytes(nat._cfg_ref, plan.ctypes.data, blob.ctypes.data), dtype=torch.uint8, device='cuda')
    again = torch.zeros(6, dtype=torch.int32, device='cuda')
    d = _lib.DecodeRepairRoundDesc(ctypes.pointer(nat.model), plan.ctypes.data, blob.ctypes.data, blob_d.data_ptr(), r['bytes'], rows.data_ptr(), rows.numel(),
                                   ws.data_ptr(), ws.numel(), sym.data_ptr(), pixels.data_ptr(), again.data_ptr(), rws.data_ptr(), rws.numel())
    _lib.call('l3c_decode_repair_round', ctypes.byref(d), torch.cuda.current_stream().cuda_stream, None)
    got = again.cpu().numpy().view(np.uint32).reshape(3, 2)
    for c in range(3):
        for e, j in enumerate((3, 7)):
            assert int(got[c, e]) == zlib.crc32(frame[c, j * L:(j + 1) * L].tobytes()), (c, j)
    assert torch.equal(pixels, x)
    # the rebuilt payloads, in the decoders' form, where the plan puts them
    parsed = container.parse_banded(container.split_seal(q[0])[0])
    area = (ws.data_ptr() + 255) // 256 * 256 - ws.data_ptr() + lib.l3c_decode_batch_banded_streams_offset(nat._cfg_ref, plan.ctypes.data)
    for j in (3, 7):
        src, dst, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_uint32()
        assert lib.l3c_decode_plan_banded_stream(plan.ctypes.data, nat.cfg.num_scales, j, ctypes.byref(src), ctypes.byref(dst), ctypes.byref(nb)) == 0
        a, k = int(parsed.offset[-1][0, j]), int(parsed.nbytes[-1][0, j])
        assert (src.value, nb.value) == (a, k)
        slot = ws[area + dst.value:area + dst.value + (k + 3) // 4 * 4 + 4].cpu().numpy()
        assert slot[:k].tobytes() == q[0][a:a + k] and (slot[k:] == 0).all()
