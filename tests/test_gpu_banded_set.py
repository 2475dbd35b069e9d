"""-m gpu: set decoding of BANDED `.l3c` files -- `decode_set(..., banded=True)` / `Bitcoding.decode_many(..., banded=True)`: every band of
every image of a ragged group is a stream of its own (l3c_decode_rgb_entries, ops.decode_z_entries).  A mixed set -- an 8x8 image (one
band), a 40x104 one (a 64-symbol last band at K = 64), one above 1 MPix, shapes that repeat, shapes that need padding -- must come back bit
exact, with the symbols of every scale that `decode_batch` gives file by file, whatever the row form, the group budget or the slice size."""
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.golden import make_hip_bitstream as gen  # noqa: E402

# (H, W) of the images: 26 images, 22 distinct padded shapes
SIZES = [(8, 8), (40, 104), (1024, 1032), (24, 40), (64, 96), (64, 96), (70, 90), (120, 200), (256, 384), (512, 768), (200, 328), (96, 64),
         (48, 48), (33, 77), (128, 128), (128, 128), (160, 96), (16, 248), (248, 16), (300, 212), (88, 136), (40, 104), (72, 72), (56, 200),
         (384, 256), (8, 8)]
_BP, _SETS = {}, {}


def blueprint(cfg):
    if cfg not in _BP:
        _BP[cfg] = gen.blueprint(cfg, True)
    return _BP[cfg]


def image_set(cfg='cr'):
    from l3c_pytorch_amd.helpers import synthetic
    sizes = SIZES if cfg == 'cr' else [(8, 8), (40, 104), (32, 48), (96, 64), (70, 90), (32, 48), (160, 112)]
    return {i: synthetic.make_image(h, w, 300 + i, 'natural') for i, (h, w) in enumerate(sizes)}


def coded_set(cfg, K, recurse=0):
    """-> (blueprint, images, files) of the set written with Bitcoding(bands=K) (K = 0: legacy files); cached."""
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.helpers import dataset_codec
    key = (cfg, K, recurse)
    if key not in _SETS:
        bp, imgs = blueprint(cfg), image_set(cfg)
        bc = Bitcoding(bp, bands=K, auto_recurse=recurse)
        files, _, _ = dataset_codec.encode_set(bc, imgs, list(imgs), max_batch=16, fac=bc.padding_factor())
        _SETS[key] = (bp, imgs, files)
    return _SETS[key]


class Spy(object):
    """Counts the calls of the group decode and records what the entries RGB decode was given and returned."""

    def __init__(self, monkeypatch):
        from l3c_pytorch_amd import ops
        from l3c_pytorch_amd.bitcoding.set_decode import SetDecoder
        self.groups, self.rgb = [], []
        group, rgb = SetDecoder.decode_group, ops.decode_rgb_entries

        def spy_group(dec, grp, *a, **kw):
            self.groups.append((len(grp), kw.get('banded', False)))
            return group(dec, grp, *a, **kw)

        def spy_rgb(P, targets, sym, buf, offs, lens, pixbase, hw, pix0, length, n_chunks, *a, **kw):
            keep = rgb(P, targets, sym, buf, offs, lens, pixbase, hw, pix0, length, n_chunks, *a, **kw)
            self.rgb.append({'pixbase': pixbase, 'hw': hw, 'pix0': pix0, 'len': length, 'chunks': n_chunks, 'limit': kw.get('limit'), 'keep': keep})
            return keep
        monkeypatch.setattr(SetDecoder, 'decode_group', spy_group)
        monkeypatch.setattr(ops, 'decode_rgb_entries', spy_rgb)


def assert_round_trip(back, imgs):
    assert sorted(back) == sorted(imgs)
    for i in imgs:
        assert back[i].shape == imgs[i].shape and torch.equal(back[i].cpu(), imgs[i]), (i, tuple(imgs[i].shape))


@pytest.mark.parametrize('K', [4, 64])
def test_mixed_set_round_trips_and_the_device_plan_is_the_planners(K, monkeypatch):
    from l3c_pytorch_amd import ops
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding, is_banded
    from l3c_pytorch_amd.helpers import dataset_codec
    bp, imgs, files = coded_set('cr', K)
    assert len(imgs) >= 24 and all(is_banded(f) for f in files.values())
    spy = Spy(monkeypatch)
    bc = Bitcoding(bp)
    back = dataset_codec.decode_set(bc, files, list(imgs), banded=True)
    torch.cuda.synchronize()
    assert_round_trip(back, imgs)
    assert spy.groups and all(b for _, b in spy.groups) and len(spy.rgb) == len(spy.groups)       # the band-aware group decode did the work
    # the plan the library's kernel wrote into the workspace is the pure function's (tests/test_banded_set_plan.py checks that one)
    for call in spy.rgb:
        S, n = len(call['len']), call['chunks']
        assert S >= len(imgs) and len(call['keep']) == 1
        pixbase, hw, pix0, npix_dev, off_dev, final = ops.rgb_entries_device_plan(call['keep'][0][0], S, n)
        start, npix, fin, off = ops.rgb_entries_plan(call['len'], n)
        assert (pixbase == call['pixbase']).all() and (hw == call['hw']).all()
        assert (pix0 == call['pix0'][None] + start).all()
        assert (npix_dev == npix).all() and (off_dev == off).all() and (final == fin).all()
        assert (npix == 0).any() and n > 1                                   # short bands really had empty chunks beside the long ones
        print('K', K, 'entries', S, 'chunks', n, 'empty chunks', int((npix == 0).sum()), 'of', npix.size)


def _scale_symbols(bp, batches, banded_set, window='auto', **attrs):
    """Every entry's symbols of every scale record (coarse -> fine, the decoder's bottleneck inputs recorded through sym_to_bn, then the
    pixels): through decode_many as a set, or batch by batch through decode_batch."""
    from l3c_pytorch_amd import ops
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    seen, orig = [], ops.sym_to_bn

    def spy(sym, *a):
        seen.append(sym.clone().cpu())
        return orig(sym, *a)
    bc = Bitcoding(bp, rgb_window=window)
    for k, v in attrs.items():
        setattr(bc.set_decoder, k, v)
    ops.sym_to_bn = spy
    try:
        if banded_set:
            res = bc.decode_many(batches, out_dtype=torch.int16, banded=True)
            torch.cuda.synchronize()
            E, n = len(batches), len(seen) // len(batches)
            assert len(seen) == E * n                                        # one group: scale-major over the entries
            return [[seen[k * E + g] for k in range(n)] + [res[g][0].cpu()] for g in range(E)]
        out = []
        for files in batches:
            del seen[:]
            dec, _ = bc.decode_batch(files, out_dtype=torch.int16)
            out.append(list(seen) + [dec.cpu()])
        return out
    finally:
        ops.sym_to_bn = orig


@pytest.mark.parametrize('K', [4, 64])
def test_every_scales_symbols_are_decode_batchs_whatever_the_row_form(K):
    from l3c_pytorch_amd.helpers import dataset_codec
    bp, imgs, files = coded_set('cr', K)
    chunks, _ = dataset_codec.plan_decode_set(files, list(imgs), 16)
    batches = [[files[i] for i in c] for c in chunks]
    want = _scale_symbols(bp, batches, False)
    for window in ('always', 'never', 'auto'):
        got = _scale_symbols(bp, batches, True, window)
        assert len(got) == len(want)
        for g, (a, b) in enumerate(zip(got, want)):
            assert len(a) == len(b) == 4
            for k, (x, y) in enumerate(zip(a, b)):
                assert x.shape == y.shape and torch.equal(x, y), (window, chunks[g], k)


def test_rgb_shared_set_with_recursion(monkeypatch):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.helpers import dataset_codec
    for K in (4, 64):
        bp, imgs, files = coded_set('cr_rgb_shared', K, recurse=3)
        spy = Spy(monkeypatch)
        for window in ('auto', 'always', 'never'):
            back = dataset_codec.decode_set(Bitcoding(bp, auto_recurse=3, rgb_window=window), files, list(imgs), banded=True)
            assert_round_trip(back, imgs)
        assert spy.groups and len(spy.rgb) == 4 * len(spy.groups)           # the model's scale and three recursions: four RGB scales per group
        monkeypatch.undo()


def test_small_budgets_split_into_groups_and_slices(monkeypatch):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.helpers import dataset_codec
    bp, imgs, files = coded_set('cr', 64)
    spy = Spy(monkeypatch)
    bc = Bitcoding(bp)
    bc.set_decoder.RAGGED_GROUP_PIXELS = 300 * 1000          # the set is 2.4 MPix: several groups
    bc.set_decoder.ENTRY_LIMIT = 50               # and every ragged call in slices of at most 50 bands
    back = dataset_codec.decode_set(bc, files, list(imgs), banded=True)
    assert_round_trip(back, imgs)
    assert len(spy.groups) >= 3
    assert all(c['limit'] == 50 for c in spy.rgb) and any(len(c['keep']) > 1 for c in spy.rgb)
    for c in spy.rgb:
        assert len(c['keep']) == -(-len(c['len']) // 50)
    bc2 = Bitcoding(bp)
    bc2.set_decoder.RAGGED_GROUP = 3              # groups cut by the image count
    assert_round_trip(dataset_codec.decode_set(bc2, files, list(imgs), banded=True), imgs)


def test_without_the_flag_banded_files_are_still_refused():
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.helpers import dataset_codec
    bp, imgs, files = coded_set('cr', 4)
    bc = Bitcoding(bp)
    order = list(imgs)[:6]
    with pytest.raises(ValueError, match='legacy .l3c files only: a banded file'):
        bc.decode_many([[files[i]] for i in order])
    with pytest.raises(ValueError, match='legacy .l3c files only: a banded file'):
        bc.decode_many([[files[i]] for i in order], banded=False)
    with pytest.raises(ValueError, match='legacy .l3c files only: a banded file'):
        dataset_codec.decode_set(bc, files, order)
    assert_round_trip(dataset_codec.decode_set(bc, files, order, banded=True), {i: imgs[i] for i in order})


def test_a_set_that_mixes_legacy_and_banded_files(monkeypatch):
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding
    from l3c_pytorch_amd.helpers import dataset_codec
    bp, imgs, legacy = coded_set('cr', 0)
    _, _, banded4 = coded_set('cr', 4)
    _, _, banded64 = coded_set('cr', 64)
    files = {i: (legacy, banded4, banded64)[i % 3][i] for i in imgs}
    spy = Spy(monkeypatch)
    back = dataset_codec.decode_set(Bitcoding(bp), files, list(imgs), banded=True)
    assert_round_trip(back, imgs)
    assert sorted({b for _, b in spy.groups}) == [False, True]               # format-pure groups, one kind each
    # the legacy set alone goes the way it always went, flag or not
    assert_round_trip(dataset_codec.decode_set(Bitcoding(bp), legacy, list(imgs), banded=True), imgs)
    assert_round_trip(dataset_codec.decode_set(Bitcoding(bp), legacy, list(imgs)), imgs)


def test_malformed_banded_files_raise_from_the_set_path_and_the_coder_goes_on():
    from l3c_pytorch_amd.bitcoding.bitcoding import Bitcoding, parse_banded
    from l3c_pytorch_amd.helpers import dataset_codec
    bp, imgs, files = coded_set('cr', 4)
    _, _, other = coded_set('cr_rgb_shared', 4, recurse=3)
    bc = Bitcoding(bp)
    order = [3, 4, 5, 6, 7, 8]
    victim = files[7]                                                        # 120x200: alone in its batch
    p = parse_banded(victim)
    h1 = int(p.offset[1][0, 0]) - 4 - 9                                      # the second record's header
    C, H, W, L = p.scales[1]
    assert struct.unpack_from('<BHHI', victim, h1) == (C, H, W, L) and L > 64
    bad = {
        'a shape the network does not predict': victim[:h1] + struct.pack('<BHH', C, H + 1, W) + victim[h1 + 5:],
        'another channel count': victim[:h1] + struct.pack('<B', 3) + victim[h1 + 1:],
        'another band length': victim[:h1 + 5] + struct.pack('<I', 64) + victim[h1 + 9:],        # 24 bands instead of 4
        'coarsest scale of another size': victim[:14] + struct.pack('<BHH', p.scales[0][0], 2, 2) + victim[19:],
        'truncated in the last record': victim[:-100],
        'truncated in the first record': victim[:40],
        'a file of the other model': other[2],
        'version': victim[:4] + b'\x02' + victim[5:],
    }
    for what, f in bad.items():
        broken = dict(files)
        broken[7] = f
        try:
            dataset_codec.decode_set(bc, broken, order, banded=True)
        except ValueError:
            pass
        else:
            pytest.fail('no ValueError for a file with ' + what)
        torch.cuda.synchronize()
    # a batch whose files disagree: equal padded shape, another band count (the planner keeps them apart; decode_many is told otherwise)
    _, _, files64 = coded_set('cr', 64)
    with pytest.raises(ValueError, match='band length'):
        bc.decode_many([[files[4], files64[5]], [files[3]]], banded=True)
    with pytest.raises(ValueError, match='mixes'):
        bc.decode_many([[files[4], coded_set('cr', 0)[2][5]], [files[3]]], banded=True)
    # the same Bitcoding then decodes a good set
    assert_round_trip(dataset_codec.decode_set(bc, files, list(imgs), banded=True), imgs)
