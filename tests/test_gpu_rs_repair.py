"""-m gpu: R parity streams per group -- Bitcoding(bands=K, seal='bands', parity=G, parity_streams=R) writes the 'L3CQ' section of seal version
3, Bitcoding.decode_repair rebuilds up to R damaged bands per group bit for bit; `l3c.py enc --parity G --parity-streams R / dec --repair`.

The frames are those of tests/test_gpu_repair.py: 320x88 at K = 16 -- L = 1792, n = 16 bands per channel --, G = 4 (m = 4 groups per channel,
band j in group j % 4) and R = 2.  The damage is a complemented payload of chosen (channel, band) streams, or of a (channel, group, row) of
the section."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd.bitcoding import container  # noqa: E402
from l3c_pytorch_amd.helpers import dataset_codec, synthetic  # noqa: E402
from tests.test_gpu_band_seal import native  # noqa: E402
from tests.test_gpu_region import bitcoding, blueprint, encoded, images  # noqa: E402
from tests.test_gpu_repair import damaged as damaged_p, damaged_like_v2, with_parity  # noqa: E402
from tests.test_gpu_salvage import NamedCalls  # noqa: E402

K, L, N, G, R = 16, 1792, 16, 4, 2
_CACHE = {}


def rs_bitcoding(streams=R, parity=G):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    if (streams, parity) not in _CACHE:
        _CACHE[streams, parity] = Bitcoding(blueprint(), bands=K, seal='bands', parity=parity, parity_streams=streams)
    return _CACHE[streams, parity]


def with_rs(streams=R, parity=G):
    """(the 320x88 image on the GPU, its 'L3CQ' file), encoded once per (R, G)."""
    key = ('files', streams, parity)
    if key not in _CACHE:
        x, _, _ = encoded(K, 1, 320, 88, seal='bands')
        _CACHE[key] = (x, rs_bitcoding(streams, parity).encode_batch(images(1, 320, 88).cuda()).to_bytes([(0, 0, 0, 0)]))
    return _CACHE[key]


def damaged(data, streams=(), rows=()):
    """The 'L3CQ' file with the payloads of the (channel, band) `streams` of its finest record complemented, and the (channel, group, row)
    payloads `rows` of its section: a walk over the framing and over the section's length fields, (c, g, r) order."""
    body, seal = container.split_seal(data)
    parsed = container.parse_banded(body)
    offset, nbytes = parsed.offset[-1], parsed.nbytes[-1]
    out = np.frombuffer(data, dtype=np.uint8).copy()
    for c, j in streams:
        a, n = int(offset[c, j]), int(nbytes[c, j])
        assert n > 16
        out[a:a + n] ^= 0xFF
    m = seal.parity_groups
    assert data[len(body):len(body) + 4] == b'L3CQ'
    at = len(body) + 12 + 12 * m
    for c in range(3):
        for g in range(m):
            for r in range(seal.parity_streams):
                n = len(seal.parity[c][g][r])
                if (c, g, r) in rows:
                    assert n > 16
                    out[at:at + n] ^= 0xFF
                at += n
    return out.tobytes()


def repair(files, bc=None):
    got, pads, info = (bc or rs_bitcoding()).decode_repair(files)
    assert got.dtype == torch.uint8
    return got, [tuple(p) for p in pads], info


def test_the_file_is_the_band_sealed_file_with_the_section_inserted():
    x, q = with_rs()
    _, v2, _ = encoded(K, 1, 320, 88, seal='bands')
    body, seal = container.split_seal(q[0])
    body2, seal2 = container.split_seal(v2[0])
    assert body == body2 and q[0][:len(body)] == v2[0][:len(body)] and q[0][len(body):len(body) + 4] == b'L3CQ' and q[0][-20] == 3
    assert (seal.generation, seal.frame_crc, seal.model_id, seal.band_len) == (seal2.generation, seal2.frame_crc, seal2.model_id, seal2.band_len)
    assert (seal.band_crcs == seal2.band_crcs).all() and (seal.parity_group, seal.parity_groups, seal.parity_streams) == (G, 4, R)
    # the rows are the reference's on the body's own band payloads
    parsed = container.parse_banded(body)
    for c in range(3):
        bands = [bytes(body[int(parsed.offset[-1][c, j]):int(parsed.offset[-1][c, j] + parsed.nbytes[-1][c, j])]) for j in range(N)]
        assert [[bytes(p) for p in rows] for rows in seal.parity[c]] == container.rs_parity(bands, G, R)
    S = container.parity_section_bytes([[len(p[0]) for p in row] for row in seal.parity], R)
    assert len(q[0]) == len(v2[0]) + S and q[0][len(body) + S:-20] == v2[0][len(body):-20]
    # the host-assembled form writes the same file
    frames = images(1, 320, 88)
    assert rs_bitcoding().encode_batch(frames.cuda()).to_bytes_host_assembled([(0, 0, 0, 0)]) == q
    # parity_streams = 1: every byte is today's 'L3CP' file
    _, v3, _ = with_parity(1, 320, 88)
    assert rs_bitcoding(1).encode_batch(frames.cuda()).to_bytes([(0, 0, 0, 0)]) == v3 and v3[0][len(body):len(body) + 4] == b'L3CP'
    # four rows; a group size beyond n is n: one group per channel of 16 members
    four = rs_bitcoding(4, 64).encode_batch(frames.cuda()).to_bytes([(0, 0, 0, 0)])
    s = container.split_seal(four[0])[1]
    assert (s.parity_group, s.parity_groups, s.parity_streams) == (N, 1, 4)
    for c in range(3):
        bands = [bytes(body[int(parsed.offset[-1][c, j]):int(parsed.offset[-1][c, j] + parsed.nbytes[-1][c, j])]) for j in range(N)]
        assert [[bytes(p) for p in rows] for rows in s.parity[c]] == container.rs_parity(bands, N, 4)


def test_an_intact_file_makes_the_calls_of_decode_salvage(monkeypatch):
    x, q = with_rs()
    bc = rs_bitcoding()
    bc.decode_salvage(q)                                    # (what the first decode of a process packs and caches is not part of the comparison)
    calls = NamedCalls(monkeypatch)
    want, _, salvage = bc.decode_salvage(q)
    names, calls.names = calls.names, []
    got, pads, info = repair(q)
    assert calls.names == names and 'l3c_u8_gf_spans' not in calls.names and 'l3c_u8_xor_spans' not in calls.names
    assert 'l3c_u8_crc32_bands' in calls.names
    assert torch.equal(got, x) and torch.equal(got, want) and torch.equal(got, bc.decode_batch(q, out_dtype=torch.uint8)[0])
    assert info.repaired == {} and info.rows == {} and info.files == [None] and info.rounds == 0 and info.salvage == salvage
    assert info.line() == 'seal: ok'


def test_two_erasures_in_one_group_come_back_exact(monkeypatch):
    x, q = with_rs()
    bad = damaged(q[0], [(0, 3), (0, 7)])                    # 3 % 4 == 7 % 4: what one XOR stream can only conceal
    with pytest.raises(container.SealError):
        rs_bitcoding().decode_batch([bad])
    calls = NamedCalls(monkeypatch)
    got, _, info = repair([bad])
    assert torch.equal(got, x)
    assert info.repaired == {0: [(0, 3), (0, 7)]} and info.files[0] == q[0] and info.rounds == 1
    assert info.salvage.concealed == {} and info.salvage.lost == []
    assert info.rows == {0: (61, 163)}
    assert info.line() == 'repaired: rows [61, 163) restored (2 payloads), every row verified'
    assert calls.names.count('l3c_u8_gf_spans') == 1 and calls.names.count('l3c_decode_rgb_entries') == 1
    assert 'l3c_u8_xor_spans' not in calls.names and 'l3c_dmll_conceal' not in calls.names
    # one erasure too, in every channel, and adjacent bands in different groups
    for streams in ([(1, 3)], [(2, 3)], [(0, 3), (0, 4)]):
        got, _, info = repair([damaged(q[0], streams)])
        assert torch.equal(got, x) and info.repaired == {0: streams} and info.files[0] == q[0] and info.rounds == 1, streams


def test_three_erasures_in_one_group_are_concealed():
    x, q = with_rs()
    bad = damaged(q[0], [(0, 3), (0, 7), (0, 11)])
    got, _, info = repair([bad])
    want, _, salvage = rs_bitcoding().decode_salvage([bad])
    assert torch.equal(got, want) and info.salvage == salvage and info.repaired == {} and info.files == [None] and info.rounds == 0
    assert {j for _, j in salvage.concealed[0]} == {3, 7, 11}
    assert info.line() == salvage.line()
    # four rows over one group of 16 bring back four, in one round
    x, four = with_rs(4, 64)
    streams = [(0, 3), (0, 7), (0, 8), (0, 11)]
    got, _, info = repair([damaged(four[0], streams)], rs_bitcoding(4, 64))
    assert torch.equal(got, x) and info.repaired == {0: streams} and info.files[0] == four[0] and info.rounds == 1


def test_a_damaged_parity_row(monkeypatch):
    x, q = with_rs()
    # one erasure and row 0 of its group complemented: row 0 alone rebuilds a payload that fails, row 1 alone heals it
    bad = damaged(q[0], [(0, 3)], rows=[(0, 3, 0)])
    calls = NamedCalls(monkeypatch)
    got, _, info = repair([bad])
    assert torch.equal(got, x) and info.repaired == {0: [(0, 3)]} and info.rounds == 2
    assert info.files[0] == damaged(q[0], rows=[(0, 3, 0)])                          # the healed file: the section unchanged
    assert info.salvage.concealed == {} and calls.names.count('l3c_u8_gf_spans') == 2
    # row 1 complemented instead: the first window does it
    got, _, info = repair([damaged(q[0], [(0, 3)], rows=[(0, 3, 1)])])
    assert torch.equal(got, x) and info.repaired == {0: [(0, 3)]} and info.rounds == 1
    # two erasures need both rows: with one complemented they are concealed, never "repaired"
    bad = damaged(q[0], [(0, 3), (0, 7)], rows=[(0, 3, 1)])
    got, _, info = repair([bad])
    assert info.repaired == {} and info.files == [None] and info.rounds == 1
    assert {j for _, j in info.salvage.concealed[0]} == {3, 7}
    want, _, salvage = rs_bitcoding().decode_salvage([bad])
    assert info.salvage == salvage and torch.equal(got, want)
    # both rows complemented beside one erasure: two windows tried, then concealed
    got, _, info = repair([damaged(q[0], [(0, 3)], rows=[(0, 3, 0), (0, 3, 1)])])
    assert info.repaired == {} and info.rounds == 2 and {j for _, j in info.salvage.concealed[0]} == {3}
    # with an intact body a damaged row is not noticed: exact pixels, nothing reported
    got, _, info = repair([damaged(q[0], rows=[(0, 3, 0), (2, 0, 1)])])
    assert torch.equal(got, x) and info.repaired == {} and info.rounds == 0 and info.line() == 'seal: ok'


def test_two_channels_of_one_position_take_two_rounds():
    x, q = with_rs()
    bad = damaged(q[0], [(0, 5), (2, 5), (0, 9)])            # R of bands 5 and 9 in one round; B of band 5 shows once R is back
    got, _, info = repair([bad])
    assert torch.equal(got, x) and info.repaired == {0: [(0, 5), (0, 9), (2, 5)]} and info.files[0] == q[0] and info.rounds == 2


def test_a_batch_of_an_l3cp_and_an_l3cq_file(monkeypatch):
    x, q = with_rs()
    _, v3, _ = with_parity(1, 320, 88)
    files = [damaged_p(v3[0], [(1, 6)]), damaged(q[0], [(0, 3), (0, 7)])]
    calls = NamedCalls(monkeypatch)
    got, _, info = repair(files)
    assert torch.equal(got[0:1], x) and torch.equal(got[1:2], x)
    assert info.repaired == {0: [(1, 6)], 1: [(0, 3), (0, 7)]} and info.files == [v3[0], q[0]] and info.rounds == 1
    assert calls.names.count('l3c_u8_xor_spans') == 1 and calls.names.count('l3c_u8_gf_spans') == 1
    assert calls.names.count('l3c_decode_rgb_entries') == 1
    # the 'L3CP' file of the pair still cannot heal two erasures of a group
    got, _, info = repair([damaged_p(v3[0], [(0, 3), (0, 7)]), damaged(q[0], [(0, 3), (0, 7)])])
    assert info.repaired == {1: [(0, 3), (0, 7)]} and {j for _, j in info.salvage.concealed[0]} == {3, 7} and torch.equal(got[1:2], x)


def test_every_other_reader_reads_the_band_sealed_file_it_contains():
    x, q = with_rs()
    _, v2, _ = encoded(K, 1, 320, 88, seal='bands')
    bc = bitcoding(K)                                        # a decoder that was never told about parity
    for f in (q, [damaged(q[0], rows=[(0, 3, 0), (1, 1, 1)])]):       # intact, and with damaged parity rows: exact pixels
        assert torch.equal(bc.decode_batch(f, out_dtype=torch.uint8)[0], x)
        a, _, ia = bc.decode_salvage(f)
        b, _, ib = bc.decode_salvage(v2)
        assert torch.equal(a, b) and ia == ib
        assert torch.equal(native(K).decode_batch(f)[0].to(torch.uint8), x)
        na, _, nia = native(K).decode_salvage(f)
        assert torch.equal(na, x) and nia == ia
        back = dataset_codec.decode_set(bc, {0: f[0]}, [0], sealed=True, banded=True)
        assert torch.equal(back[0].cuda(), x[0])
        assert dataset_codec.verify_set(bc, {0: f[0]}, [0], banded=True) == dataset_codec.verify_set(bc, {0: v2[0]}, [0], banded=True)
        got, info = bc.decode_region(f, (100, 140))
        assert torch.equal(got, x[:, :, 100:140]) and info.pixel_crc_checked
    # damage is located as in the band-sealed file, by both codecs
    bad3, bad2 = damaged(q[0], [(0, 3)]), damaged_like_v2(v2[0], 0, 3)
    for codec in (bc, native(K)):
        with pytest.raises(container.SealError) as e3:
            codec.decode_batch([bad3])
        with pytest.raises(container.SealError) as e2:
            codec.decode_batch([bad2])
        assert e3.value.bands == e2.value.bands and e3.value.rows == e2.value.rows == {0: (61, 82)}
        a, _, ia = codec.decode_salvage([bad3])
        b, _, ib = codec.decode_salvage([bad2])
        assert torch.equal(a, b) and ia == ib


def test_l3c_cli_enc_parity_streams_dec_repair(synthetic_l3c, tmp_path, capsys):
    """`enc --bands 16 --seal-bands --parity 4 --parity-streams 2`, then `dec --repair --write-repaired` on a file with two damaged bands of one
    group: the picture is the input, the line names the rows, the healed file is the original."""
    import importlib.util
    import os
    from PIL import Image
    cfg, sd = synthetic_l3c
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exp = tmp_path / 'logs' / '0306_0001 cr oi' / 'ckpts'
    exp.mkdir(parents=True)
    torch.save({'net': sd}, str(exp / 'ckpt_0000000001.pt'))
    img = synthetic.make_image(320, 88, 23, 'natural')
    src, out, png, healed = str(tmp_path / 'in.png'), str(tmp_path / 'out.l3c'), str(tmp_path / 'dec.png'), str(tmp_path / 'healed.l3c')
    Image.fromarray(img.permute(1, 2, 0).numpy()).save(src)
    spec = importlib.util.spec_from_file_location('l3c_cli', os.path.join(root, 'l3c.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    args = [str(tmp_path / 'logs'), '0306_0001']
    assert cli.main(args + ['enc', '--bands', '16', '--seal-bands', '--parity', '4', '--parity-streams', '2', src, out]) == 0
    capsys.readouterr()
    data = open(out, 'rb').read()
    seal = container.split_seal(data)[1]
    assert data[-20] == 3 and (seal.parity_group, seal.parity_streams) == (4, 2)
    assert cli.main(args + ['dec', '--repair', out, png]) == 0
    assert 'seal: ok' in capsys.readouterr().out
    assert cli.main(args + ['dec', out, png]) == 0                                   # the plain decode reads it too
    capsys.readouterr()
    with open(out, 'wb') as f:
        f.write(damaged(data, [(0, 3), (0, 7)]))
    assert cli.main(args + ['dec', '--repair', '--write-repaired', healed, out, png]) == 0
    said = capsys.readouterr().out
    assert 'repaired: rows [61, 163) restored (2 payloads), every row verified' in said and 'Repaired file' in said
    assert torch.equal(torch.from_numpy(np.array(Image.open(png))).permute(2, 0, 1), img)
    assert open(healed, 'rb').read() == data
    assert cli.main(args + ['dec', out, png]) == 1                                   # without the flag: as ever
    assert 'DecodeError: seal:' in capsys.readouterr().out
    with pytest.raises(ValueError, match='parity_streams > 1 needs parity'):
        cli.main(args + ['enc', '--bands', '16', '--seal-bands', '--parity-streams', '2', '-f', src, out])
