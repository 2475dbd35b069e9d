"""-m gpu: parity bands -- Bitcoding(bands=K, seal='bands', parity=G) writes seal version 3, Bitcoding.decode_repair rebuilds the damaged
bands of the finest record bit for bit and says which (container.RepairInfo); `l3c.py enc --parity / dec --repair`.

Frames are 320x88 at K = 16 -- L = 1792, n = 16 bands per channel -- and 317x83 images centre-padded to that frame; G = 4, so m = 4 groups
per channel and band j lies in group j % 4.  The damage is a complemented payload of chosen (channel, band) streams, or of a parity stream."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd.bitcoding import container  # noqa: E402
from l3c_pytorch_amd.helpers import dataset_codec, pad, synthetic  # noqa: E402
from tests.test_gpu_band_seal import native  # noqa: E402
from tests.test_gpu_region import bitcoding, blueprint, encoded, images  # noqa: E402
from tests.test_gpu_salvage import NamedCalls  # noqa: E402

K, L, N, G = 16, 1792, 16, 4
_CACHE = {}


def parity_bitcoding(parity=G):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    if parity not in _CACHE:
        _CACHE[parity] = Bitcoding(blueprint(), bands=K, seal='bands', parity=parity)
    return _CACHE[parity]


def with_parity(B, H, W, parity=G):
    """(images on the GPU, their version-3 files, the padding tuple), encoded once per case: the images and frames of tests.test_gpu_region."""
    key = ('files', B, H, W, parity)
    if key not in _CACHE:
        x, _, padding = encoded(K, B, H, W, seal='bands')
        frames = images(B, H, W)
        if any(padding):
            frames, _ = pad.pad(frames.long(), fac=parity_bitcoding().padding_factor(), mode=blueprint().get_padding_mode())
        _CACHE[key] = (x, parity_bitcoding(parity).encode_batch(frames.cuda()).to_bytes([padding] * B), padding)
    return _CACHE[key]


def damaged(data, streams=(), parity=()):
    """The file with the payloads of the (channel, band) `streams` of its finest record complemented, and the parity payloads of the
    (channel, group) pairs `parity`: a walk over the framing and the parity section's length fields."""
    body, seal = container.split_seal(data)
    parsed = container.parse_banded(body)
    offset, nbytes = parsed.offset[-1], parsed.nbytes[-1]
    out = np.frombuffer(data, dtype=np.uint8).copy()
    for c, j in streams:
        a, n = int(offset[c, j]), int(nbytes[c, j])
        assert n > 16
        out[a:a + n] ^= 0xFF
    m = seal.parity_groups
    at = len(body) + 8 + 12 * m
    for c in range(3):
        for g in range(m):
            n = len(seal.parity[c][g])
            if (c, g) in parity:
                assert n > 16
                out[at:at + n] ^= 0xFF
            at += n
    return out.tobytes()


def repair(files):
    got, pads, info = parity_bitcoding().decode_repair(files)
    assert got.dtype == torch.uint8
    return got, [tuple(p) for p in pads], info


def test_the_file_is_the_band_sealed_file_with_the_section_inserted():
    x, v3, _ = with_parity(1, 320, 88)
    _, v2, _ = encoded(K, 1, 320, 88, seal='bands')
    body, seal = container.split_seal(v3[0])
    body2, seal2 = container.split_seal(v2[0])
    assert body == body2 and v3[0][:len(body)] == v2[0][:len(body)]
    assert (seal.generation, seal.frame_crc, seal.model_id, seal.band_len) == (seal2.generation, seal2.frame_crc, seal2.model_id, seal2.band_len)
    assert (seal.band_crcs == seal2.band_crcs).all() and seal.parity_group == G and seal.parity_groups == 4 and seal2.parity is None
    # the parity payloads are the reference's on the body's own band payloads
    parsed = container.parse_banded(body)
    for c in range(3):
        bands = [bytes(body[int(parsed.offset[-1][c, j]):int(parsed.offset[-1][c, j] + parsed.nbytes[-1][c, j])]) for j in range(N)]
        assert [bytes(p) for p in seal.parity[c]] == container.band_parity(bands, G)
    S = container.parity_section_bytes([[len(p) for p in row] for row in seal.parity])
    assert len(v3[0]) == len(v2[0]) + S and v3[0][len(body) + S:-20] == v2[0][len(body):-20]
    # the host-assembled form writes the same file
    frames = images(1, 320, 88)
    assert parity_bitcoding().encode_batch(frames.cuda()).to_bytes_host_assembled([(0, 0, 0, 0)]) == v3
    # parity = 0: every byte is today's
    assert parity_bitcoding(0).encode_batch(frames.cuda()).to_bytes([(0, 0, 0, 0)]) == v2
    # a group size beyond n is n: one parity stream per channel
    big = parity_bitcoding(64).encode_batch(frames.cuda()).to_bytes([(0, 0, 0, 0)])
    s = container.split_seal(big[0])[1]
    assert s.parity_group == N and s.parity_groups == 1


def test_an_intact_file_makes_the_calls_of_decode_salvage(monkeypatch):
    x, v3, _ = with_parity(1, 320, 88)
    bc = parity_bitcoding()
    bc.decode_salvage(v3)                                   # (what the first decode of a process packs and caches is not part of the comparison)
    calls = NamedCalls(monkeypatch)
    want, _, salvage = bc.decode_salvage(v3)
    names, calls.names = calls.names, []
    got, pads, info = repair(v3)
    assert calls.names == names and 'l3c_u8_xor_spans' not in calls.names and 'l3c_u8_crc32_bands' in calls.names
    assert torch.equal(got, x) and torch.equal(got, want) and torch.equal(got, bc.decode_batch(v3, out_dtype=torch.uint8)[0])
    assert info.repaired == {} and info.rows == {} and info.files == [None] and info.rounds == 0 and info.salvage == salvage
    assert info.line() == 'seal: ok'
    # a file without parity and an unsealed file: decode_salvage
    _, v2, _ = encoded(K, 1, 320, 88, seal='bands')
    _, plain, _ = encoded(K, 1, 320, 88)
    damaged_v2 = damaged_like_v2(v2[0], 0, 3)
    got, _, info = repair([damaged_v2])
    want, _, salvage = bc.decode_salvage([damaged_v2])
    assert torch.equal(got, want) and info.salvage == salvage and info.repaired == {} and info.files == [None] and info.rounds == 0
    got, _, info = repair(plain)
    assert torch.equal(got, x) and info.salvage.unverified == [0] and info.repaired == {}


@pytest.mark.parametrize('c', [0, 1, 2])
def test_one_damaged_payload_is_restored(c, monkeypatch):
    x, v3, _ = with_parity(1, 320, 88)
    bad = damaged(v3[0], [(c, 3)])
    with pytest.raises(container.SealError):
        parity_bitcoding().decode_batch([bad])
    calls = NamedCalls(monkeypatch)
    got, _, info = repair([bad])
    assert torch.equal(got, x)
    assert info.repaired == {0: [(c, 3)]} and info.rows == {0: (61, 82)} and info.files[0] == v3[0] and info.rounds == 1
    assert info.salvage.concealed == {} and info.salvage.lost == []
    assert info.line() == 'repaired: rows [61, 82) restored (1 payload), every row verified'
    assert calls.names.count('l3c_u8_xor_spans') == 1 and calls.names.count('l3c_decode_rgb_entries') == 1 and 'l3c_dmll_conceal' not in calls.names
    assert parity_bitcoding().decode_repair([bad], out_dtype=torch.int64)[0].dtype == torch.int64


def test_two_channels_of_two_positions_in_one_group_index():
    x, v3, _ = with_parity(1, 320, 88)
    bad = damaged(v3[0], [(0, 5), (1, 9)])                   # both in group 1, different channels: different parity streams
    got, _, info = repair([bad])
    assert torch.equal(got, x) and info.repaired == {0: [(0, 5), (1, 9)]} and info.files[0] == v3[0]
    # recorded: two rounds.  G of band 5 does not verify while R of band 5 is damaged (G's means depend on the decoded R), so the group of
    # G of band 9 -- bands 1, 5, 9, 13 of G -- has a member that fails in the first round; R of band 5 comes back first, G of band 9 second
    assert info.rounds == 2, info.rounds
    assert info.rows == {0: (101, 204)}
    assert info.line() == 'repaired: rows [101, 204) restored (2 payloads), every row verified'


def test_two_channels_of_one_position_take_two_rounds():
    x, v3, _ = with_parity(1, 320, 88)
    bad = damaged(v3[0], [(0, 5), (2, 5)])                   # the erasure of position 5 is R; B shows once R is back
    got, _, info = repair([bad])
    assert torch.equal(got, x) and info.repaired == {0: [(0, 5), (2, 5)]} and info.files[0] == v3[0] and info.rounds == 2


def test_adjacent_bands_lie_in_different_groups():
    x, v3, _ = with_parity(1, 320, 88)
    bad = damaged(v3[0], [(0, 3), (0, 4)])
    got, _, info = repair([bad])
    assert torch.equal(got, x) and info.repaired == {0: [(0, 3), (0, 4)]} and info.files[0] == v3[0] and info.rounds == 1


def test_two_erasures_in_one_group_are_concealed():
    x, v3, _ = with_parity(1, 320, 88)
    bad = damaged(v3[0], [(0, 3), (0, 7)])                   # 3 % 4 == 7 % 4
    got, _, info = repair([bad])
    want, _, salvage = parity_bitcoding().decode_salvage([bad])
    assert torch.equal(got, want) and info.salvage == salvage and info.repaired == {} and info.files == [None] and info.rounds == 0
    assert {j for _, j in salvage.concealed[0]} == {3, 7}
    assert info.line() == salvage.line()


def test_a_damaged_parity_payload():
    x, v3, _ = with_parity(1, 320, 88)
    # with an intact body: the pixels are exact and nothing is reported, through every reader
    bad = damaged(v3[0], parity=[(0, 3), (2, 0)])
    got, _, info = repair([bad])
    assert torch.equal(got, x) and info.repaired == {} and info.salvage.concealed == {} and info.rounds == 0 and info.line() == 'seal: ok'
    assert torch.equal(parity_bitcoding().decode_batch([bad], out_dtype=torch.uint8)[0], x)
    # together with its group's band: the rebuilt payload does not verify -- concealed, not "repaired"
    bad = damaged(v3[0], [(0, 3)], parity=[(0, 3)])
    got, _, info = repair([bad])
    assert info.repaired == {} and info.files == [None] and info.rounds == 1
    assert {j for _, j in info.salvage.concealed[0]} == {3} and (0, 3) in info.salvage.concealed[0]
    assert info.salvage.rows == {0: (61, 82)} and info.line().startswith('salvaged: rows [61, 82) concealed')
    flat, want = got.reshape(3, -1), x.reshape(3, -1)
    assert torch.equal(flat[:, :3 * L], want[:, :3 * L]) and torch.equal(flat[:, 4 * L:], want[:, 4 * L:])
    want_pixels, _, salvage = parity_bitcoding().decode_salvage([bad])
    assert info.salvage == salvage and torch.equal(got, want_pixels)


def test_a_batch_of_padded_images_one_damaged():
    x, v3, padding = with_parity(2, 317, 83)
    files = [v3[0], damaged(v3[1], [(1, 0), (2, 15)])]
    got, pads, info = repair(files)
    assert pads == [padding] * 2
    left, right, top, bottom = padding
    assert torch.equal(got[:, :, top:320 - bottom, left:88 - right], x)
    assert info.repaired == {1: [(1, 0), (2, 15)]} and info.files == [None, v3[1]]
    assert info.rows == {1: (0, 317)} and info.line() == 'repaired: file 1: rows [0, 317) restored (2 payloads), every row verified'


def test_every_other_reader_reads_the_band_sealed_file_it_contains():
    x, v3, _ = with_parity(1, 320, 88)
    _, v2, _ = encoded(K, 1, 320, 88, seal='bands')
    bc = bitcoding(K)                                        # a decoder that was never told about parity
    assert torch.equal(bc.decode_batch(v3, out_dtype=torch.uint8)[0], x)
    a, _, ia = bc.decode_salvage(v3)
    b, _, ib = bc.decode_salvage(v2)
    assert torch.equal(a, b) and ia == ib
    assert torch.equal(native(K).decode_batch(v3)[0], native(K).decode_batch(v2)[0]) and torch.equal(native(K).decode_batch(v3)[0].to(torch.uint8), x)
    na, _, nia = native(K).decode_salvage(v3)
    assert torch.equal(na, x) and nia == ia
    back = dataset_codec.decode_set(bc, {0: v3[0]}, [0], sealed=True, banded=True)
    assert torch.equal(back[0].cuda(), x[0])
    got, info = bc.decode_region(v3, (100, 140))
    assert torch.equal(got, x[:, :, 100:140]) and info.pixel_crc_checked
    # damage is located as in the band-sealed file, by both codecs
    bad3, bad2 = damaged(v3[0], [(0, 3)]), damaged_like_v2(v2[0], 0, 3)
    for codec in (bc, native(K)):
        with pytest.raises(container.SealError) as e3:
            codec.decode_batch([bad3])
        with pytest.raises(container.SealError) as e2:
            codec.decode_batch([bad2])
        assert e3.value.bands == e2.value.bands and e3.value.rows == e2.value.rows == {0: (61, 82)}


def damaged_like_v2(data, c, j):
    from tests.test_gpu_band_seal import complemented
    return complemented(data, [j], [c])


def test_l3c_cli_enc_parity_dec_repair(synthetic_l3c, tmp_path, capsys):
    """`enc --bands 16 --seal-bands --parity 4`, then `dec --repair` on the intact file (`seal: ok`) and on a damaged one: the picture is
    the input, the line names the rows, --write-repaired writes the original file; `dec` without the flag still refuses the damaged file."""
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
    assert cli.main(args + ['enc', '--bands', '16', '--seal-bands', '--parity', '4', src, out]) == 0
    assert 'parity over groups of 4' in capsys.readouterr().out
    data = open(out, 'rb').read()
    assert data[-20] == 3 and container.split_seal(data)[1].parity_group == 4
    assert cli.main(args + ['dec', '--repair', out, png]) == 0
    assert 'seal: ok' in capsys.readouterr().out
    assert cli.main(args + ['dec', out, png]) == 0                                   # the plain decode reads it too
    capsys.readouterr()
    with open(out, 'wb') as f:
        f.write(damaged(data, [(0, 3)]))
    assert cli.main(args + ['dec', '--repair', '--write-repaired', healed, out, png]) == 0
    said = capsys.readouterr().out
    assert 'repaired: rows [61, 82) restored (1 payload), every row verified' in said and 'Repaired file' in said
    assert torch.equal(torch.from_numpy(np.array(Image.open(png))).permute(2, 0, 1), img)
    assert open(healed, 'rb').read() == data
    assert cli.main(args + ['dec', out, png]) == 1                                   # without the flag: as ever
    assert 'DecodeError: seal:' in capsys.readouterr().out
    assert cli.main(args + ['dec', '--repair', '--region', '0:10', out, png]) == 1
    assert '--region' in capsys.readouterr().out
    assert cli.main(args + ['dec', '--write-repaired', healed, out, png]) == 1
    assert '--write-repaired needs --repair' in capsys.readouterr().out
    with pytest.raises(ValueError, match='--parity needs'):
        cli.main(args + ['enc', '--bands', '16', '--parity', '4', '-f', src, out])
