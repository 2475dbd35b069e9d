"""-m gpu: pictures as they come (include/l3c_hip.h: l3c_u8_gather / l3c_u8_scatter, l3c_encode_images / l3c_decode_images;
native_codec.NativeCodec.encode_images / decode_images).

The two kernels against numpy, byte for byte: a view's address array  offset + y row_stride + x pix_stride + c chan_stride  IS the
definition, so the expected frame is np.pad(..., 'constant') of what lies at those addresses and the expected scatter is an assignment
through them into a buffer prefilled with 0xA5.  Frames of every vector width the kernels pick (Wp % 16 == 0, % 8 == 0, % 4 == 0), images
narrower than one thread's run, packed pixels at every alignment, more than one block, and one frame large enough for the grid-stride loop.  Then the codec on a batch of
differently sized HWC images against Bitcoding on the zero-padded batch, both formats, both directions, every layout."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from l3c_pytorch_amd.helpers import pad  # noqa: E402
from tests.test_gpu_native_banded import bitcoding, codec  # noqa: E402

FILL = 0xA5
VARIANTS = ('planar', 'pitch', 'rgb_odd', 'rgbx', 'bgr')
#          1x1 -> 8x8, 8x8 (no padding), 5x13 -> 8x16, 9x17 -> 16x24, the widths around one and two 16-pixel runs, two multi-block frames
SIZES = [(1, 1), (8, 8), (5, 13), (9, 17), (3, 15), (3, 16), (2, 17), (3, 31), (4, 33), (33, 120), (70, 130)]


def _view(variant, h, w, at):
    """(offset, row_stride, chan_stride, pix_stride), bytes the image occupies from `at` on (gaps included)."""
    if variant == 'planar':
        return (at, w, h * w, 1), 3 * h * w
    if variant == 'pitch':                                # planar with row pitch w + 5
        return (at, w + 5, h * (w + 5), 1), 3 * h * (w + 5)
    if variant == 'rgb_odd':                              # RGB at an odd base offset with a pitch that is no multiple of 4
        pitch = 3 * w + (1 if (3 * w + 1) % 4 else 2)
        at += 1 - at % 2
        return (at, pitch, 1, 3), h * pitch
    if variant == 'rgbx':
        return (at, 4 * w, 1, 4), 4 * h * w
    if variant == 'bgr':                                  # B G R in memory: the view starts at the R byte and walks down
        return (at + 2, 3 * w, -1, 3), 3 * h * w
    raise ValueError(variant)


def _addresses(entry):
    offset, rs, cs, ps, h, w = (int(v) for v in entry.tolist()[:6])
    c, y, x = np.meshgrid(np.arange(3), np.arange(h), np.arange(w), indexing='ij')
    return offset + y * rs + x * ps + c * cs


class Batch(object):
    """Images of `sizes` in `variants`, back to back (3 stray bytes between them) in one buffer of random bytes; centre padding to `fac`
    unless frame = (Hp, Wp, [(top, left)]) places them by hand."""

    def __init__(self, sizes, variants, seed, fac=8, frame=None):
        from l3c_pytorch_amd.native_codec import IMAGE_DTYPE
        rng = np.random.RandomState(seed)
        self.pixels = [rng.randint(0, 256, (3, h, w)).astype(np.uint8) for h, w in sizes]
        self.table = np.zeros(len(sizes), dtype=IMAGE_DTYPE)
        at, self.pads = 0, []
        for k, ((h, w), v) in enumerate(zip(sizes, variants)):
            if frame is None:
                p = pad.padding_for(h, w, fac)
                Hp, Wp = h + p[2] + p[3], w + p[0] + p[1]
            else:
                Hp, Wp, (top, left) = frame[0], frame[1], frame[2][k]
                p = (left, Wp - left - w, top, Hp - top - h)
            assert k == 0 or (Hp, Wp) == (self.Hp, self.Wp), 'the images of a batch share a frame'
            self.Hp, self.Wp = Hp, Wp
            self.pads.append(p)
            (offset, rs, cs, ps), n = _view(v, h, w, at)
            self.table[k] = (offset, rs, cs, ps, h, w, p[2], p[0])
            at = max(at, offset) + n + 3
        self.nbytes = at
        self.buffer = rng.randint(0, 256, at).astype(np.uint8)
        for k, px in enumerate(self.pixels):
            a = _addresses(self.table[k])
            assert a.min() >= 0 and a.max() < at
            self.buffer[a] = px
        self.frames = np.stack([np.pad(px, ((0, 0), (p[2], p[3]), (p[0], p[1])), 'constant') for px, p in zip(self.pixels, self.pads)])

    def gather(self, shift=0):
        """shift: the strided buffer starts `shift` bytes into its allocation (an unaligned base pointer)."""
        from l3c_pytorch_amd import _lib
        B = len(self.table)
        src = torch.from_numpy(np.concatenate([np.zeros(shift, dtype=np.uint8), self.buffer])).cuda()
        tab = torch.from_numpy(self.table.view(np.uint8)).cuda()
        dst = torch.full((B, 3, self.Hp, self.Wp), FILL, dtype=torch.uint8, device='cuda')
        pads = torch.full((B, 4), -1, dtype=torch.int16, device='cuda')
        _lib.call('l3c_u8_gather', src.data_ptr() + shift, self.nbytes, self.table.ctypes.data, tab.data_ptr(), B, self.Hp, self.Wp, dst.data_ptr(),
                  pads.data_ptr(), _lib.stream())
        return dst, pads.cpu().numpy().view(np.uint16)

    def scatter(self, frames, shift=0):
        from l3c_pytorch_amd import _lib
        tab = torch.from_numpy(self.table.view(np.uint8)).cuda()
        dst = torch.full((shift + self.nbytes,), FILL, dtype=torch.uint8, device='cuda')
        _lib.call('l3c_u8_scatter', frames.data_ptr(), len(self.table), self.Hp, self.Wp, dst.data_ptr() + shift, self.nbytes, self.table.ctypes.data,
                  tab.data_ptr(), _lib.stream())
        got = dst.cpu().numpy()
        assert (got[:shift] == FILL).all()
        return got[shift:]

    def check(self, shift=0):
        frames, pads = self.gather(shift)
        assert np.array_equal(frames.cpu().numpy(), self.frames)                          # the whole frame: picture and zeros
        assert [tuple(int(v) for v in p) for p in pads] == [tuple(p) for p in self.pads]
        want = np.full(self.nbytes, FILL, dtype=np.uint8)
        for k, px in enumerate(self.pixels):
            want[_addresses(self.table[k])] = px
        # scatter from frames whose padding is NOT zero: nothing of it may reach the destination
        noisy = np.random.RandomState(1).randint(0, 256, self.frames.shape).astype(np.uint8)
        for k, (px, p) in enumerate(zip(self.pixels, self.pads)):
            noisy[k, :, p[2]:p[2] + px.shape[1], p[0]:p[0] + px.shape[2]] = px
        got = self.scatter(torch.from_numpy(noisy).cuda(), shift)
        assert np.array_equal(got, want)                                                  # the crop where the views are, 0xA5 everywhere else
        back = self.scatter(frames, shift)                                                # scatter(gather(x)) == x
        assert np.array_equal(back, want)


@pytest.mark.parametrize('variant', VARIANTS)
def test_kernels_against_numpy_every_size(variant):
    for k, (h, w) in enumerate(SIZES):
        b = Batch([(h, w)], [variant], 10 * k + 1)
        if (h, w) in ((1, 1), (5, 13), (9, 17)):
            assert (b.Hp, b.Wp) == {(1, 1): (8, 8), (5, 13): (8, 16), (9, 17): (16, 24)}[h, w]
        if (h, w) == (8, 8):
            assert b.pads == [(0, 0, 0, 0)]
        if variant == 'pitch':
            assert b.table['row_stride'][0] == w + 5
        if variant == 'rgb_odd':
            assert b.table['offset'][0] % 2 == 1 and b.table['row_stride'][0] % 4 != 0
        b.check()


def test_three_sizes_and_layouts_share_one_frame():
    b = Batch([(5, 13), (8, 16), (1, 9)], ['rgb_odd', 'planar', 'bgr'], 7)
    assert (b.Hp, b.Wp) == (8, 16) and b.pads == [pad.padding_for(5, 13, 8), (0, 0, 0, 0), pad.padding_for(1, 9, 8)]
    b.check()
    Batch([(5, 13), (8, 16), (1, 9), (3, 10), (8, 11)], ['rgbx', 'pitch', 'planar', 'rgb_odd', 'bgr'], 8).check()


@pytest.mark.parametrize('shift', [1, 2, 3])
def test_packed_pixels_at_every_alignment_and_at_the_ends_of_the_buffer(shift):
    """Packed pixels move as the aligned dwords AROUND a run: a buffer whose base pointer is itself unaligned, images that begin with the
    buffer's first byte and end with its last (no stray bytes behind: the run's last dwords would leave the buffer), rows of odd pitch."""
    for variants in (['bgr', 'rgb_odd', 'rgbx'], ['rgbx', 'bgr', 'bgr'], ['rgb_odd', 'rgbx', 'rgb_odd']):
        b = Batch([(8, 48), (7, 41), (3, 43)], variants, 30 + shift)
        assert (b.Hp, b.Wp) == (8, 48)
        b.nbytes = max(int(_addresses(e).max()) for e in b.table) + 1      # the last image's last byte is the buffer's
        b.buffer = b.buffer[:b.nbytes]
        b.check(shift)
    Batch([(9, 50), (16, 56)], ['bgr', 'rgb_odd'], 40 + shift).check(shift)          # Wp = 56: 8-byte frame accesses


def test_frames_of_dword_width_and_free_placement():
    """Wp % 8 == 4: the frames move as single dwords; (top, left) anywhere in the frame, one image flush with each edge."""
    for variant in VARIANTS:
        Batch([(5, 9), (6, 12), (1, 1)], [variant] * 3, 5, frame=(6, 12, [(1, 2), (0, 0), (5, 11)])).check()
    Batch([(7, 30)], ['planar'], 6, frame=(9, 36, [(2, 5)])).check()           # a planar row that starts dword aligned only in some rows


def test_grid_stride_loop():
    """2900 x 2900 at one dword per thread is more than 8192 blocks of 256: every thread takes a second turn.  One planar image, built
    without the address arrays (they would take longer than the kernels)."""
    from l3c_pytorch_amd import _lib
    from l3c_pytorch_amd.native_codec import IMAGE_DTYPE
    h, w, Hp, Wp, top, left = 2897, 2893, 2900, 2900, 1, 3
    assert Hp * (Wp // 4) > 8192 * 256 and Wp % 8 == 4
    g = torch.Generator().manual_seed(9)
    pixels = torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g)
    table = np.zeros(1, dtype=IMAGE_DTYPE)
    table[0] = (0, w, h * w, 1, h, w, top, left)
    n = pixels.numel()
    src, tab = pixels.reshape(-1).cuda(), torch.from_numpy(table.view(np.uint8)).cuda()
    frames = torch.full((1, 3, Hp, Wp), FILL, dtype=torch.uint8, device='cuda')
    _lib.call('l3c_u8_gather', src.data_ptr(), n, table.ctypes.data, tab.data_ptr(), 1, Hp, Wp, frames.data_ptr(), None, _lib.stream())
    want = torch.nn.functional.pad(pixels, (left, Wp - left - w, top, Hp - top - h), 'constant', 0)
    assert torch.equal(frames[0].cpu(), want)
    dst = torch.full((n + 5,), FILL, dtype=torch.uint8, device='cuda')
    _lib.call('l3c_u8_scatter', frames.data_ptr(), 1, Hp, Wp, dst.data_ptr(), n, table.ctypes.data, tab.data_ptr(), _lib.stream())
    assert torch.equal(dst[:n].cpu(), pixels.reshape(-1)) and (dst[n:] == FILL).all()


# ---- the codec -------------------------------------------------------------------------------------------------------------------

SHAPES = [(61, 93), (57, 90), (64, 96)]                   # all -> 64 x 96
_CASE = {}


def _chw(h, w, seed):
    """A smooth image with noise on top (uint8, host): something the calibrated model codes well below 16 bits per symbol."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    base = 128 + 90 * torch.sin(yy[None] / 9.0 + torch.arange(3).view(3, 1, 1)) * torch.cos(xx[None] / 13.0 + seed)
    return (base + torch.randint(-12, 13, (3, h, w), generator=g)).clamp(0, 255).to(torch.uint8)


def _as(layout, chw):
    """The (3,h,w) host tensor in `layout`, as a numpy array."""
    hwc = chw.permute(1, 2, 0).contiguous().numpy()
    if layout == 'chw':
        return chw.numpy()
    if layout == 'hwc':
        return hwc
    if layout == 'bgr':
        return np.ascontiguousarray(hwc[:, :, ::-1])
    return np.concatenate([hwc, np.zeros(hwc.shape[:2] + (1,), dtype=np.uint8)], axis=2)      # hwcx


def case(K):
    """(images (3,h,w), paddings, the zero-padded batch, the files of Bitcoding(bp[, bands=K]) on it), computed once and shared."""
    if K not in _CASE:
        imgs = [_chw(h, w, 3 + k) for k, (h, w) in enumerate(SHAPES)]
        pads = [pad.padding_for(h, w, 8) for h, w in SHAPES]
        x = torch.stack([torch.nn.functional.pad(im, p, 'constant', 0) for im, p in zip(imgs, pads)]).cuda()
        assert tuple(x.shape) == (3, 3, 64, 96)
        _CASE[K] = (imgs, pads, x, bitcoding(K).encode_batch(x).to_bytes(pads))
    return _CASE[K]


@pytest.mark.parametrize('K', [0, 4])
def test_encode_images_equals_bitcoding_on_the_padded_batch(K):
    imgs, pads, x, want = case(K)
    got = codec(K).encode_images([_as('hwc', im) for im in imgs], layout='hwc')
    assert [len(f) for f in got] == [len(f) for f in want]
    for k in range(3):
        assert got[k] == want[k], 'file {}'.format(k)
    assert codec(K).encode_images([torch.from_numpy(_as('bgr', im)) for im in imgs], layout='bgr') == want      # host tensors, another layout


@pytest.mark.parametrize('K', [0, 4])
@pytest.mark.parametrize('layout', ['chw', 'hwc', 'hwcx', 'bgr'])
def test_decode_images_returns_each_input_in_every_layout(K, layout):
    imgs, pads, x, want = case(K)
    out = codec(0).decode_images(want, layout=layout)          # the files Bitcoding wrote; decode reads either format
    assert len(out) == 3
    for im, t in zip(imgs, out):
        assert t.is_cuda and t.dtype == torch.uint8
        assert np.array_equal(t.cpu().numpy(), _as(layout, im))


@pytest.mark.parametrize('K', [0, 4])
def test_bitcoding_reads_what_encode_images_wrote(K):
    imgs, pads, x, want = case(K)
    files = codec(K).encode_images([_as('hwcx', im) for im in imgs], layout='hwcx')
    pixels, got_pads = bitcoding(K).decode_batch(files, out_dtype=torch.uint8)
    assert [tuple(p) for p in got_pads] == pads
    for k, im in enumerate(imgs):
        assert torch.equal(pad.undo_pad(pixels[k:k + 1], *got_pads[k])[0].cpu(), im)


def test_two_padded_shapes_and_both_formats_come_back_in_input_order():
    shapes = [(61, 93), (30, 40), (64, 96), (25, 33), (57, 90), (1, 1)]
    imgs = [_chw(h, w, 20 + k) for k, (h, w) in enumerate(shapes)]
    from l3c_pytorch_amd.helpers import dataset_codec
    legacy = codec(0).encode_images([im.numpy() for im in imgs], max_batch=2)
    assert [dataset_codec.file_padded_shape(f) for f in legacy] == [(64, 96), (32, 40), (64, 96), (32, 40), (64, 96), (8, 8)]
    banded = codec(4).encode_images(imgs)
    mix = [banded[k] if k % 2 else legacy[k] for k in range(len(imgs))]      # legacy and banded files in one call
    for files in (legacy, banded, mix):
        out = codec(0).decode_images(files, max_batch=2)
        assert [tuple(t.shape) for t in out] == [(3, h, w) for h, w in shapes]
        for im, t in zip(imgs, out):
            assert torch.equal(t.cpu(), im)


def test_device_entries_and_a_table_that_does_not_fit_the_plan():
    from l3c_pytorch_amd import _lib
    from l3c_pytorch_amd.native_codec import IMAGE_DTYPE, decode_plan, image_entry
    imgs, pads, x, want = case(0)
    c = codec(0)
    # pixels already on the GPU: planar images back to back
    src = torch.cat([im.reshape(-1) for im in imgs]).cuda()
    table, off = np.zeros(3, dtype=IMAGE_DTYPE), 0
    for k, (im, p) in enumerate(zip(imgs, pads)):
        table[k] = image_entry('chw', tuple(im.shape), off, p[2], p[0])
        off += im.numel()
    assert c.to_bytes(*c.encode_images_device(src, table, 64, 96)) == want
    blob, H, W, got_pads = decode_plan(c.cfg, want)
    assert (H, W) == (64, 96) and got_pads == pads
    sizes = [len(f) for f in want]
    files_dev = torch.zeros(sum(sizes) + 16, dtype=torch.uint8, device='cuda')
    files_dev[:sum(sizes)] = torch.from_numpy(np.frombuffer(b''.join(want), dtype=np.uint8).copy()).cuda()
    plan_dev = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    dst = torch.full((off,), FILL, dtype=torch.uint8, device='cuda')
    c.decode_images_device(files_dev, blob, plan_dev, dst, table)
    assert torch.equal(dst.cpu(), torch.cat([im.reshape(-1) for im in imgs]))
    # a table made for a 72 x 96 frame: refused before anything runs
    bad = table.copy()
    bad['h'][2], bad['top'][2] = 72, 0
    big = torch.full((off + 3 * 8 * 96,), FILL, dtype=torch.uint8, device='cuda')
    with pytest.raises(_lib.L3CError, match='image 2: top \\+ h'):
        c.decode_images_device(files_dev, blob, plan_dev, big, bad)
    bad = table.copy()
    bad['offset'][2] += 1                                  # one byte past the end of dst
    with pytest.raises(_lib.L3CError, match='image 2: the view ends behind'):
        c.decode_images_device(files_dev, blob, plan_dev, dst, bad)
    with pytest.raises(_lib.L3CError, match='image 2: the view ends behind'):
        c.encode_images_device(src, bad, 64, 96)
    torch.cuda.synchronize()
    assert (big == FILL).all()
