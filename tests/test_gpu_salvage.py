"""-m gpu: salvage decode -- Bitcoding.decode_salvage and NativeCodec.decode_salvage conceal the damaged bands of a band-sealed file, return
every verified pixel exact and say which is which (container.SalvageInfo); `l3c.py dec --salvage`.

Frames are 320x88 at K = 16 -- bands of L = 1792 symbols, 20.4 rows -- and 317x83 images centre-padded to that frame.  The damage is the one
tests/test_gpu_band_seal.py applies: complemented band payloads of the finest record.  Every case runs through both codecs, which must agree
in pixels and in info."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd.bitcoding import container  # noqa: E402
from l3c_pytorch_amd.bitcoding.container import SealError  # noqa: E402
from l3c_pytorch_amd.helpers import synthetic  # noqa: E402
from tests.test_gpu_band_seal import complemented, native  # noqa: E402
from tests.test_gpu_region import Calls, bitcoding, crop, encoded, images  # noqa: E402,F401

K, L = 16, 1792


class NamedCalls(Calls):
    """Calls, and the names of the library calls it counted."""

    def __init__(self, monkeypatch):
        from l3c_pytorch_amd import _lib, ops
        Calls.__init__(self, monkeypatch)
        self.names = []
        counting = _lib.call

        def naming(name, *args):
            self.names.append(name)
            return counting(name, *args)
        for mod in (_lib, ops):
            monkeypatch.setattr(mod, 'call', naming)


def salvage_both(files):
    """decode_salvage through both codecs: the same pixels, paddings and info -> (pixels, paddings, info)."""
    a, pa, ia = bitcoding(K).decode_salvage(files)
    b, pb, ib = native(K).decode_salvage(files)
    assert a.dtype == b.dtype == torch.uint8 and torch.equal(a, b)
    assert [tuple(p) for p in pa] == [tuple(p) for p in pb]
    assert ia == ib, (ia, ib)
    return a, [tuple(p) for p in pa], ia


def planes(t):
    """(B, 3, H, W) -> (B, 3, HW)."""
    return t.reshape(t.shape[0], 3, -1)


def test_an_intact_batch_is_decode_batch_and_launches_no_conceal(monkeypatch):
    x, sealed, _ = encoded(K, 1, 320, 88, seal='bands')
    calls = NamedCalls(monkeypatch)
    got, pads, info = salvage_both(sealed)
    assert torch.equal(got, x) and pads == [(0, 0, 0, 0)]
    assert info.concealed == {} and info.rows == {} and info.lost == [] and info.unverified == []
    assert info.line() == 'seal: ok'
    assert calls.n == len(calls.names) > 0 and 'l3c_dmll_conceal' not in calls.names
    assert 'l3c_u8_crc32_bands' in calls.names                                     # ... and it WAS verified
    assert torch.equal(bitcoding(K).decode_batch(sealed, out_dtype=torch.uint8)[0], got)
    # unsealed files: nothing to verify, and the info says so
    _, plain, _ = encoded(K, 1, 320, 88)
    got, _, info = salvage_both(plain)
    assert torch.equal(got, x) and info.unverified == [0] and info.concealed == {} and info.lost == []
    # out_dtype
    assert bitcoding(K).decode_salvage(sealed, out_dtype=torch.int64)[0].dtype == torch.int64


def test_a_damaged_band_takes_the_preview_estimate_and_the_rest_is_exact(monkeypatch):
    x, sealed, _ = encoded(K, 1, 320, 88, seal='bands')
    bad = complemented(sealed[0], [3])
    calls = NamedCalls(monkeypatch)
    got, _, info = salvage_both([bad])
    assert calls.names.count('l3c_dmll_conceal') == 2                              # one per codec
    g, want = planes(got), planes(x)
    assert torch.equal(g[:, :, :3 * L], want[:, :, :3 * L]) and torch.equal(g[:, :, 4 * L:], want[:, :, 4 * L:])
    bc = bitcoding(K)
    total = bc.n_predicted_scales() + 1
    preview, _ = bc.decode_preview([bad], records=total - 1)                       # the same get_P, hence the same P, through l3c_dmll_mean
    assert torch.equal(g[:, :, 3 * L:4 * L], planes(preview)[:, :, 3 * L:4 * L])
    assert not torch.equal(g[:, :, 3 * L:4 * L], want[:, :, 3 * L:4 * L])
    assert info.concealed == {0: [(0, 3), (1, 3), (2, 3)]} and info.rows == {0: (61, 82)}
    assert info.lost == [] and info.unverified == []
    assert info.line() == 'salvaged: rows [61, 82) concealed (3 of 48 bands), every other row verified'


def test_a_channel_that_verified_is_kept_and_conditions_the_others():
    x, sealed, _ = encoded(K, 1, 320, 88, seal='bands')
    bad = complemented(sealed[0], [3], [1])                                        # band 3's stream of G only
    got, _, info = salvage_both([bad])
    assert torch.equal(got[:, 0], x[:, 0])                                         # R verified everywhere: kept
    for codec in (bitcoding(K), native(K)):
        with pytest.raises(SealError) as e:
            codec.decode_batch([bad])
        assert e.value.reason == 'pixels' and info.concealed[0] == e.value.bands[0] and info.rows == e.value.rows
    assert (1, 3) in info.concealed[0] and (0, 3) not in info.concealed[0] and {j for _, j in info.concealed[0]} == {3}
    raw = bitcoding(K).decode_batch([bad], out_dtype=torch.int64, verify=False)[0]
    g = planes(got.long())
    assert not torch.equal(g[:, 1, 3 * L:4 * L], planes(raw)[:, 1, 3 * L:4 * L])
    assert int(g.min()) >= 0 and int(g.max()) <= 255
    keep = torch.ones(3, 320 * 88, dtype=torch.bool)
    for c, j in info.concealed[0]:
        keep[c, j * L:(j + 1) * L] = False
    assert torch.equal(planes(got)[0][keep.cuda()], planes(x)[0][keep.cuda()])    # every pixel outside the concealed bands is the input


def test_a_batch_of_padded_images_one_damaged():
    x, sealed, padding = encoded(K, 2, 317, 83, seal='bands')
    files = [sealed[0], complemented(sealed[1], [0], [2])]
    got, pads, info = salvage_both(files)
    assert pads == [padding] * 2
    left, right, top, bottom = padding
    inner = got[:, :, top:320 - bottom, left:88 - right]
    assert torch.equal(inner[0], x[0])
    assert torch.equal(got[0], bitcoding(K).decode_batch(sealed, out_dtype=torch.uint8)[0][0])
    assert info.concealed == {1: [(2, 0)]} and info.rows == {1: (0, 21 - padding[2])} and info.lost == []
    assert torch.equal(inner[1, :2], x[1, :2]) and torch.equal(inner[1, :, 21 - top:], x[1, :, 21 - top:])
    assert info.line().startswith('salvaged: file 1: rows [0, {})'.format(21 - top))


def test_a_file_with_no_verified_band_position_is_lost():
    x, sealed, _ = encoded(K, 1, 320, 88, seal='bands')
    bad = complemented(sealed[0], list(range(16)))                                 # all 16 band positions
    got, _, info = salvage_both([bad])
    assert info.lost == [0] and {j for _, j in info.concealed[0]} == set(range(16)) and info.rows == {0: (0, 320)}
    preview, _ = bitcoding(K).decode_preview([bad], records=bitcoding(K).n_predicted_scales())
    assert torch.equal(got, preview)                                               # concealed all the same: the whole frame is the estimate
    assert 'LOST' in info.line()
    assert got.shape == x.shape


def test_a_damaged_version_1_file_is_lost_and_its_neighbour_unaffected():
    x, sealed, _ = encoded(K, 1, 320, 88, seal='bands')
    _, v1, _ = encoded(K, 1, 320, 88, seal=True)
    _, plain, _ = encoded(K, 1, 320, 88)
    bad_v1 = complemented(v1[0], [2])
    files = [bad_v1, sealed[0], plain[0], complemented(sealed[0], [5], [0])]
    got, _, info = salvage_both(files)
    assert info.lost == [0] and info.unverified == [2] and list(info.concealed) == [3] and {j for _, j in info.concealed[3]} == {5}
    assert torch.equal(got[1], x[0]) and torch.equal(got[2], x[0])
    raw = bitcoding(K).decode_batch([bad_v1], out_dtype=torch.uint8, verify=False)[0]
    assert torch.equal(got[0], raw[0])                                             # left as decoded
    assert 'file 0: LOST' in info.line() and 'not sealed: file(s) [2]' in info.line()
    # a batch of version-1 and unsealed files alone: no band table anywhere
    got, _, info = salvage_both([bad_v1, v1[0], plain[0]])
    assert info.lost == [0] and info.unverified == [2] and info.concealed == {} and torch.equal(got[1], x[0])


def test_decode_batch_still_raises_and_the_pre_decode_checks_still_do():
    _, sealed, _ = encoded(K, 1, 320, 88, seal='bands')
    bad = complemented(sealed[0], [3])
    for codec in (bitcoding(K), native(K)):
        with pytest.raises(SealError) as e:
            codec.decode_batch([bad])
        assert e.value.reason == 'pixels' and e.value.index == 0 and e.value.failed == [0]
        assert e.value.bands == {0: [(0, 3), (1, 3), (2, 3)]} and e.value.rows == {0: (61, 82)}
    # another generation is not damage: raised before anything is decoded, by both
    body, seal = container.split_seal(sealed[0])
    other = body + container.make_seal(body, seal.generation + 1, seal.frame_crc, seal.model_id, seal.band_crcs, seal.band_len)
    for codec in (bitcoding(K), native(K)):
        with pytest.raises(SealError) as e:
            codec.decode_salvage([other])
        assert e.value.reason == 'generation'
    # a legacy file among banded ones is refused as decode_batch refuses it
    _, legacy, _ = encoded(0, 1, 320, 88)
    for codec in (bitcoding(K), native(K)):
        with pytest.raises(ValueError):
            codec.decode_salvage([sealed[0], legacy[0]])


def test_l3c_cli_dec_salvage(synthetic_l3c, tmp_path, capsys):
    """`dec --salvage` on a damaged band-sealed file writes the picture -- the undamaged rows are the input -- and prints the rows; on an
    intact file it prints `seal: ok`; `dec` without the flag still refuses the damaged file."""
    import importlib.util
    import os
    from PIL import Image
    cfg, sd = synthetic_l3c
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exp = tmp_path / 'logs' / '0306_0001 cr oi' / 'ckpts'
    exp.mkdir(parents=True)
    torch.save({'net': sd}, str(exp / 'ckpt_0000000001.pt'))
    img = synthetic.make_image(320, 88, 23, 'natural')
    src, out, png = str(tmp_path / 'in.png'), str(tmp_path / 'out.l3c'), str(tmp_path / 'dec.png')
    Image.fromarray(img.permute(1, 2, 0).numpy()).save(src)
    spec = importlib.util.spec_from_file_location('l3c_cli', os.path.join(root, 'l3c.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    args = [str(tmp_path / 'logs'), '0306_0001']
    assert cli.main(args + ['enc', '--bands', '16', '--seal-bands', src, out]) == 0
    capsys.readouterr()
    assert cli.main(args + ['dec', '--salvage', out, png]) == 0
    assert 'seal: ok' in capsys.readouterr().out
    assert torch.equal(torch.from_numpy(np.array(Image.open(png))).permute(2, 0, 1), img)
    data = open(out, 'rb').read()
    with open(out, 'wb') as f:
        f.write(complemented(data, [3]))
    assert cli.main(args + ['dec', '--salvage', out, png]) == 0
    said = capsys.readouterr().out
    assert 'salvaged: rows [61, 82) concealed (3 of 48 bands), every other row verified' in said
    back = torch.from_numpy(np.array(Image.open(png))).permute(2, 0, 1)
    assert back.shape == img.shape and torch.equal(back[:, :61], img[:, :61]) and torch.equal(back[:, 82:], img[:, 82:])
    assert not torch.equal(back[:, 61:82], img[:, 61:82])
    assert cli.main(args + ['dec', out, png]) == 1                                 # without the flag: as ever
    assert 'DecodeError: seal:' in capsys.readouterr().out
    assert cli.main(args + ['dec', '--salvage', '--region', '0:10', out, png]) == 1
    assert '--region' in capsys.readouterr().out
