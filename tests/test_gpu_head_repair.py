"""-m gpu: head parity -- Bitcoding(bands=K, seal='bands', parity=G, parity_streams=R, parity_head=True) writes the 'L3CH' section, and
Bitcoding.decode_repair heals the HEAD of a damaged file (container.heal_head: framing fields and payloads of the coarser records) before it
rebuilds bands of the finest record.

The 320x88 frames of tests/test_gpu_repair.py at K = 16, G = 4, R = 2: the records are 40x11, 80x22, 160x44 (5 channels) and 320x88 with
n = 7, 14, 16, 16 bands per channel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd.bitcoding import container  # noqa: E402
from l3c_pytorch_amd.helpers import dataset_codec, synthetic  # noqa: E402
from tests.test_gpu_band_seal import native  # noqa: E402
from tests.test_gpu_region import bitcoding, blueprint, images  # noqa: E402
from tests.test_gpu_salvage import NamedCalls  # noqa: E402

K, G, R = 16, 4, 2
BANDS = [7, 14, 16, 16]
_CACHE = {}


def coder(head=True, streams=R):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    if (head, streams) not in _CACHE:
        _CACHE[head, streams] = Bitcoding(blueprint(), bands=K, seal='bands', parity=G, parity_streams=streams, parity_head=head)
    return _CACHE[head, streams]


def files(head=True, streams=R):
    """(the image on the GPU, its file), encoded once per kind."""
    key = ('file', head, streams)
    if key not in _CACHE:
        x = images(1, 320, 88)
        _CACHE[key] = (x.cuda(), coder(head, streams).encode_batch(x.cuda()).to_bytes([(0, 0, 0, 0)]))
    return _CACHE[key]


def hurt(data, fields=(), payloads=()):
    """The file with one bit flipped in the length fields of the (record, channel, band) triples `fields` and the payloads of `payloads`
    complemented; record 3 is the finest.  Positions from the intact file's framing."""
    parsed = container.parse_banded(container.split_seal(data)[0])
    out = np.frombuffer(data, dtype=np.uint8).copy()
    for k, c, j in fields:
        out[int(parsed.offset[k][c, j]) - 4] ^= 0x10
    for k, c, j in payloads:
        a, n = int(parsed.offset[k][c, j]), int(parsed.nbytes[k][c, j])
        assert n > 8, (k, c, j, n)
        out[a:a + n] ^= 0xFF
    return out.tobytes()


def test_the_file_is_the_L3CQ_file_with_the_head_part_inserted():
    x, vh = files()
    _, vq = files(head=False)
    body, seal = container.split_seal(vh[0])
    body_q, seal_q = container.split_seal(vq[0])
    assert body == body_q and seal == seal_q and seal.head is not None and seal_q.head is None and not seal.head_damaged
    parsed = container.parse_banded(body)
    assert [nb.shape for nb in parsed.nbytes] == [(5, 7), (5, 14), (5, 16), (3, 16)]
    t, tq = container._tail(vh[0]), container._tail(vq[0])
    assert vh[0][t.section_at:t.section_at + 4] == b'L3CH' and vq[0][tq.section_at:tq.section_at + 4] == b'L3CQ'
    head_bytes = t.head_end - t.head_at
    assert len(vh[0]) == len(vq[0]) + head_bytes and t.S == tq.S + head_bytes
    assert vh[0][t.section_at + 4:t.head_at] == vq[0][tq.section_at + 4:tq.section_at + tq.S - 8]          # G, m, R, plen, the finest rows
    assert vh[0][t.section_at + t.S:-4] == vq[0][tq.section_at + tq.S:-4]                                  # the table and seal bytes 0..19
    # the CRC words and rows are the references' on the body's own payloads, and so is the whole tail
    ref = container.head_from_body(body, G, R)
    for k, (crc, rows) in enumerate(ref):
        assert np.array_equal(seal.head.crcs[k], crc) and seal.head.groups[k] == (4, -(-BANDS[k] // 4))
        assert [[[bytes(q) for q in grp] for grp in ch] for ch in seal.head.rows[k]] == rows
    rows = [[[bytes(q) for q in seal.rows(c, g)] for g in range(4)] for c in range(3)]
    assert vh[0][len(body):] == container.make_seal(body, seal.generation, seal.frame_crc, seal.model_id, seal.band_crcs, seal.band_len,
                                                    parity=(G, rows), head=ref)
    # the host-assembled form writes the same file
    assert coder().encode_batch(x).to_bytes_host_assembled([(0, 0, 0, 0)]) == vh
    # one row per group: 'L3CH' all the same, around the 'L3CP' file's row
    _, v1 = files(streams=1)
    _, vp = files(head=False, streams=1)
    t1, tp = container._tail(v1[0]), container._tail(vp[0])
    assert v1[0][t1.section_at:t1.section_at + 4] == b'L3CH' and vp[0][tp.section_at:tp.section_at + 4] == b'L3CP'
    assert v1[0][t1.section_at + 12:t1.head_at] == vp[0][tp.section_at + 8:tp.section_at + tp.S - 8]
    assert container.split_seal(v1[0])[1] == container.split_seal(vp[0])[1]


def test_without_the_flag_the_bytes_and_the_library_calls_are_the_L3CQ_encoders(monkeypatch):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    x, vq = files(head=False)
    plain = Bitcoding(blueprint(), bands=K, seal='bands', parity=G, parity_streams=R)        # the constructor as it was called before
    calls = NamedCalls(monkeypatch)
    assert plain.encode_batch(x).to_bytes([(0, 0, 0, 0)]) == vq
    before, calls.names = calls.names, []
    assert coder(head=False).encode_batch(x).to_bytes([(0, 0, 0, 0)]) == vq
    without, calls.names = calls.names, []
    coder().encode_batch(x).to_bytes([(0, 0, 0, 0)])
    assert without == before and 'l3c_head_parity' not in before and 'l3c_band_payload_crc32' not in before
    at = before.index('l3c_band_parity_rs') + 1                  # the two new calls sit behind the finest record's parity, nothing else moves
    assert calls.names == before[:at] + ['l3c_band_payload_crc32', 'l3c_head_parity'] + before[at:]
    _, vp = files(head=False, streams=1)
    assert Bitcoding(blueprint(), bands=K, seal='bands', parity=G).encode_batch(x).to_bytes([(0, 0, 0, 0)]) == vp


def test_more_coarser_records_than_one_launch_takes_are_refused_before_anything_is_coded(monkeypatch):
    from l3c_pytorch_amd import ops
    x, _ = files()
    monkeypatch.setattr(ops, 'HEAD_MAX_RECORDS', 2)              # this model writes 3 records in front of the finest
    calls = NamedCalls(monkeypatch)
    with pytest.raises(ValueError, match='parity_head needs 1..2 scale records in front of the finest .* this model writes 4 record'):
        coder().encode_batch(x)
    assert not {'l3c_ac_band_intervals', 'l3c_ac_encode_groups', 'l3c_head_parity', 'l3c_band_payload_crc32'} & set(calls.names)
    coder(head=False).encode_batch(x)                            # without the flag there is no such limit


def test_an_intact_file_makes_the_calls_of_the_L3CQ_file(monkeypatch):
    x, vh = files()
    _, vq = files(head=False)
    bc = coder()
    bc.decode_repair(vq)
    calls = NamedCalls(monkeypatch)
    want, _, info_q = bc.decode_repair(vq)
    names, calls.names = calls.names, []
    got, _, info = bc.decode_repair(vh)
    assert calls.names == names and torch.equal(got, x) and torch.equal(want, x)
    assert info_q.head == [None] and len(info.head) == 1 and not info.head[0] and info.head[0].line() == 'head: ok'
    assert info.files == [None] and info.repaired == {} and info.rounds == 0 and info.line() == 'seal: ok'


@pytest.mark.parametrize('what', ['a finest length field', 'a coarse length field', 'a payload of the 80x22 record',
                                  'two payloads of one group of the 160x44 record', 'a coarse payload and a finest band of another group'])
def test_head_damage_is_healed_and_every_pixel_comes_back(what):
    x, vh = files()
    fields, payloads = {'a finest length field': ([(3, 1, 6)], []), 'a coarse length field': ([(1, 2, 9)], []),
                        'a payload of the 80x22 record': ([], [(1, 3, 5)]),
                        'two payloads of one group of the 160x44 record': ([], [(2, 0, 1), (2, 0, 5)]),
                        'a coarse payload and a finest band of another group': ([], [(2, 4, 2), (3, 0, 7)])}[what]
    bad = hurt(vh[0], fields, payloads)
    with pytest.raises(ValueError) as e:                         # today: an invalid file, or pixels that do not verify
        coder().decode_batch([bad])
    assert 'invalid file' in str(e.value) or (isinstance(e.value, container.SealError) and e.value.reason == 'pixels'), str(e.value)
    if fields:
        assert 'invalid file' in str(e.value)
    got, _, info = coder().decode_repair([bad])
    assert torch.equal(got, x), what
    head = info.head[0]
    coarse = [p for p in payloads if p[0] < 3]
    assert head.framing == ({'length field': len(fields)} if fields else {}) and head.framing_fixed == len(fields)
    assert head.repaired == coarse and head.failed == [] and not head.section_damaged
    finest = [(c, j) for k, c, j in payloads if k == 3]
    assert info.repaired == ({0: finest} if finest else {}) and info.salvage.concealed == {} and info.salvage.lost == []
    assert info.files[0] == vh[0]                                # healed: the original file, head fixes and rebuilt bands spliced in
    assert torch.equal(coder().decode_batch(info.files, out_dtype=torch.uint8)[0], x)
    want = {'a finest length field': 'head: 1 length field restored', 'a coarse length field': 'head: 1 length field restored',
            'a payload of the 80x22 record': 'head: 1 coarse payload restored',
            'two payloads of one group of the 160x44 record': 'head: 2 coarse payloads restored',
            'a coarse payload and a finest band of another group': 'head: 1 coarse payload restored'}[what]
    assert head.line() == want
    assert info.line() == ('repaired: rows [142, 163) restored (1 payload), every row verified' if finest else 'seal: ok')


def test_three_payloads_of_one_group_are_beyond_two_rows():
    x, vh = files()
    lost = [(2, 0, 1), (2, 0, 5), (2, 0, 9)]
    bad = hurt(vh[0], payloads=lost + [(1, 0, 0)])
    got, _, info = coder().decode_repair([bad])
    head = info.head[0]
    assert head.failed == lost and head.repaired == [(1, 0, 0)]
    # what is left is today's salvage of the file with that damage
    left = hurt(vh[0], payloads=lost)
    assert info.files[0] == left
    want, _, salvage = coder().decode_salvage([left])
    assert torch.equal(got, want) and info.salvage == salvage and info.repaired == {}
    assert salvage.lost == [0] or salvage.concealed, 'a wrong coarse record must show in the pixels'


def test_every_other_reader_reads_the_band_sealed_file_it_contains():
    x, vh = files()
    _, vq = files(head=False)
    bc = bitcoding(K)                                            # a decoder that was never told about parity
    assert torch.equal(bc.decode_batch(vh, out_dtype=torch.uint8)[0], x)
    got, info = bc.decode_region(vh, (100, 140))
    assert torch.equal(got, x[:, :, 100:140]) and info.pixel_crc_checked
    back = dataset_codec.decode_set(bc, {0: vh[0]}, [0], sealed=True, banded=True)
    assert torch.equal(back[0].cuda(), x[0])
    assert torch.equal(native(K).decode_batch(vh)[0], native(K).decode_batch(vq)[0]) and torch.equal(native(K).decode_batch(vh)[0].to(torch.uint8), x)
    a, _, ia = native(K).decode_salvage(vh)
    b, _, ib = native(K).decode_salvage(vq)
    assert torch.equal(a, x) and torch.equal(a, b) and ia == ib
    # a damaged head part: the file still reads, through both codecs, and decode_repair says that the section is damaged
    t = container._tail(vh[0])
    bad = vh[0][:t.head_at + 40] + bytes([vh[0][t.head_at + 40] ^ 1]) + vh[0][t.head_at + 41:]
    assert torch.equal(bc.decode_batch([bad], out_dtype=torch.uint8)[0], x) and torch.equal(native(K).decode_batch([bad])[0].to(torch.uint8), x)
    got, _, info = coder().decode_repair([bad])
    assert torch.equal(got, x) and info.head[0].section_damaged and info.files == [None]


def test_l3c_cli_enc_parity_head_dec_repair(synthetic_l3c, tmp_path, capsys):
    """`enc --bands 16 --seal-bands --parity 4 --parity-streams 2 --parity-head`, then `dec --repair` on a file with a flipped length field:
    the head line comes in front of the repair line, the picture is the input, --write-repaired writes the original file."""
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
    assert cli.main(args + ['enc', '--bands', '16', '--seal-bands', '--parity', '4', '--parity-streams', '2', '--parity-head', src, out]) == 0
    capsys.readouterr()
    data = open(out, 'rb').read()
    assert container.split_seal(data)[1].head is not None
    with open(out, 'wb') as f:
        f.write(hurt(data, fields=[(2, 1, 3)]))
    with pytest.raises(ValueError, match='invalid file'):            # without the flag: as ever
        cli.main(args + ['dec', out, png])
    capsys.readouterr()
    assert cli.main(args + ['dec', '--repair', '--write-repaired', healed, out, png]) == 0
    said = capsys.readouterr().out
    assert 'head: 1 length field restored\nseal: ok' in said and 'Repaired file' in said
    assert torch.equal(torch.from_numpy(np.array(Image.open(png))).permute(2, 0, 1), img)
    assert open(healed, 'rb').read() == data
    with pytest.raises(ValueError, match='--parity-head needs --parity'):
        cli.main(args + ['enc', '--bands', '16', '--seal-bands', '--parity-head', '-f', src, out])
