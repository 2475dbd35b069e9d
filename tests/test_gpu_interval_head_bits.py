"""-m gpu: the encoder's interval head (l3c_dmll_encode_intervals: the vector tile fill and the compile-time shapes of
csrc/dmll_kernels.hip) against its predecessor, which the TEST-ONLY library keeps with its text unchanged (csrc/xcheck_iv.hip,
l3c_xcheck_dmll_encode_intervals): every interval word equal bit for bit, the zero words of the pixels past HW in the last 64-block
included.  Both write into a larger buffer filled with 0xA5A5A5A5, and the margins on both sides must still hold it afterwards.

Shapes: (C, K, rgb) = (3, 10, true) and (5, 10, false) -- the two compile-time instantiations -- and (1, 3, false), which takes the
run-time kernel; B = 3; HW = 1, 63, 64, 65, 101 and 2 * 64 + 37.  With the 600-byte rows of the 150-channel tile every odd HW puts the
tiles of image 1 on an 8-byte boundary only (the 8-byte fill), an odd row count of the last tile ends the 16-byte fill in a single
half, and P as a view one float into a larger buffer forces the 4-byte fill.

Inputs (seeded): logits N(0, 3); mu uniform over [x_min - 40 bin, x_max + 40 bin]; log_sigma uniform over [-9, 3] (across the -7 clamp);
lambdas N(0, 2); symbols uniform with the first forced to 0 and the second to L - 1 (c_high = 0x10000).  Every case must reach all four
ranges of sigmoid_sat (a >= 16.7, a <= -89, the library path -89 < a <= -80, and the middle) and both edge symbols: this is asserted
on the CPU from the inputs in fp64, with the range limits drawn in by 0.5 so that no fp32 rounding of `a` can move a counted term out of
its range.  The seed of a case is the first of its sequence whose inputs do (at HW = 1 a draw has as few as 18 terms); the inputs alone
decide that, before anything runs on the GPU.

The decoder's table kernel takes the same fill: its rows for C = 5, HW = 101, B = 3 -- ranges that start on 8-byte boundaries -- give, through
l3c_ac_intervals_from_table, the predecessor's words as well."""
import numpy as np
import pytest
import torch

from oracle import cdf as ocdf

pytestmark = pytest.mark.gpu

MARGIN = 64                      # words on either side of an output
SENTINEL = 0xA5A5A5A5 - (1 << 32)   # as int32

SHAPES = [(3, 10, True), (5, 10, False), (1, 3, False)]
SIZES = [1, 63, 64, 65, 101, 2 * 64 + 37]
B = 3


def _spec(rgb):
    return (0.0, 255.0, 256) if rgb else (-1.0, 1.0, 25)


def _draw(seed, C, K, rgb, HW):
    x_min, x_max, L = _spec(rgb)
    bin_w = (x_max - x_min) / (L - 1)
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    CK = C * K
    Kp = (4 if rgb else 3) * CK
    P = torch.empty(B, 1, HW, Kp)
    P[..., :CK] = torch.randn(B, 1, HW, CK, generator=g) * 3
    P[..., CK:2 * CK] = torch.rand(B, 1, HW, CK, generator=g) * (x_max - x_min + 80 * bin_w) + (x_min - 40 * bin_w)
    P[..., 2 * CK:3 * CK] = torch.rand(B, 1, HW, CK, generator=g) * 12 - 9
    if rgb:
        P[..., 3 * CK:] = torch.randn(B, 1, HW, CK, generator=g) * 2
    sym = torch.randint(0, L, (B, C, 1, HW), generator=g).to(torch.int16)
    flat = sym.view(-1)
    flat[0] = 0
    flat[1] = L - 1
    return P, sym


def _covered(P, sym, targets, C, K, rgb):
    """fp64, from the inputs alone: do the sigmoid arguments (t - mu') exp(-max(log_sigma, -7)) of the two entries per symbol reach all
    four ranges of sigmoid_sat, and do both edge symbols occur?"""
    _, _, L = _spec(rgb)
    CK = C * K
    Pd = P.double()[:, 0]                                              # (B, HW, Kp)
    HW = Pd.shape[1]
    s = sym[:, :, 0].long()                                            # (B, C, HW)
    x = s.double()
    mu = Pd[..., CK:2 * CK].reshape(B, HW, C, K).permute(0, 2, 1, 3).clone()        # (B, C, HW, K)
    ls = Pd[..., 2 * CK:3 * CK].reshape(B, HW, C, K).permute(0, 2, 1, 3).clamp(min=-7.0)
    if rgb:
        lam = torch.sigmoid(Pd[..., 3 * CK:].reshape(B, HW, 3, K))     # [0]: G on R, [1]: B on R, [2]: B on G
        mu[:, 1] += lam[:, :, 0] * x[:, 0, :, None]
        mu[:, 2] += lam[:, :, 1] * x[:, 0, :, None] + lam[:, :, 2] * x[:, 1, :, None]
    t = targets.double()
    a = torch.stack([(t[s + d][..., None] - mu) * torch.exp(-ls) for d in (0, 1)])
    ranges = [(a >= 17.2).any(), (a <= -89.5).any(), ((a > -88.5) & (a <= -80.5)).any(), ((a > -79.5) & (a < 16.2)).any()]
    return all(bool(r) for r in ranges) and bool((s == 0).any()) and bool((s == L - 1).any())


def _case(C, K, rgb, HW):
    x_min, x_max, L = _spec(rgb)
    targets = ocdf.coding_targets(x_min, x_max, L)
    base = 100000 * C + 1000 * HW
    for seed in range(base, base + 1000):
        P, sym = _draw(seed, C, K, rgb, HW)
        if _covered(P, sym, targets, C, K, rgb):
            return P, sym, targets
    raise AssertionError('no draw in 1000 reaches the four sigmoid ranges and both edge symbols')


def _intervals(product, P, sym, targets, C, K, rgb):
    """-> (guarded buffer, the interval words inside it)"""
    from l3c_pytorch_amd import _lib, ops
    Bn, H, W, _ = P.shape
    n = _lib.load().l3c_interval_words(Bn * C, H * W)
    buf = torch.full((n + 2 * MARGIN,), SENTINEL, dtype=torch.int32, device='cuda')
    iv = buf[MARGIN:MARGIN + n]
    args = (ops.ptr(P, torch.float32), ops.ptr(sym, torch.int16), ops.ptr(targets, torch.float32), Bn, H * W, C, K, int(rgb),
            targets.shape[0], ops.ptr(iv), ops.stream())
    if product:
        _lib.call('l3c_dmll_encode_intervals', *args)
    else:
        _lib.call_xcheck('l3c_xcheck_dmll_encode_intervals', *args)
    return buf, iv


def _same_words(P, sym, targets, C, K, rgb, what):
    from l3c_pytorch_amd import ops
    HW = P.shape[1] * P.shape[2]
    got_buf, got = _intervals(True, P, sym, targets, C, K, rgb)
    want_buf, want = _intervals(False, P, sym, targets, C, K, rgb)
    for buf, who in ((got_buf, 'product'), (want_buf, 'predecessor')):
        assert bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[-MARGIN:] == SENTINEL).all()), '{} ({}): wrote outside its output'.format(what, who)
    assert torch.equal(got, want), '{}: {} of {} words differ'.format(what, int((got != want).sum()), got.numel())
    assert torch.equal(ops.dmll_encode_intervals(P, sym, targets, C, K, rgb), want), what + ' (ops.dmll_encode_intervals)'
    if HW % 64:                                                        # [t / 64][stream][role][64]: the pixels past HW
        tail = got.view(-1, B * C, 2, 64)[-1, :, :, HW % 64:]
        assert bool((tail == 0).all()), what + ': words past HW are not zero'
    return want


@pytest.mark.parametrize('HW', SIZES)
@pytest.mark.parametrize('C,K,rgb', SHAPES)
def test_interval_words_equal_predecessor(C, K, rgb, HW):
    P, sym, targets = _case(C, K, rgb, HW)
    P, sym, targets = P.cuda(), sym.cuda(), targets.cuda()
    assert P.data_ptr() % 16 == 0
    _same_words(P, sym, targets, C, K, rgb, 'C {} K {} rgb {} HW {}'.format(C, K, rgb, HW))


@pytest.mark.parametrize('C,K,rgb', SHAPES[:2])
def test_interval_words_equal_predecessor_P_off_alignment(C, K, rgb):
    """P starts 4 bytes into a larger buffer: no 16-byte and no 8-byte loads of it."""
    HW = 2 * 64 + 37
    P, sym, targets = _case(C, K, rgb, HW)
    store = torch.zeros(P.numel() + 1, device='cuda')
    store[1:] = P.reshape(-1).cuda()
    Pv = store[1:].view(P.shape)
    assert Pv.data_ptr() % 16 == 4 and Pv.is_contiguous()
    _same_words(Pv, sym.cuda(), targets.cuda(), C, K, rgb, 'C {} K {} rgb {} HW {} P off alignment'.format(C, K, rgb, HW))


def test_table_kernel_through_the_fill_gives_predecessor_intervals():
    """ops.dmll_cdf_table (cdf_table_from_P_kernel calls the same fill_tile; its 32-pixel tiles of image 1 start on 8-byte boundaries at HW =
    101) -> l3c_ac_intervals_from_table: the words of the predecessor's fused head.  And a range that starts at an odd pixel (every tile of
    images 0 and 2 on an 8-byte boundary) gives the same rows as the full range."""
    from l3c_pytorch_amd import ops
    C, K, rgb, HW = 5, 10, False, 101
    P, sym, targets = _case(C, K, rgb, HW)
    P, sym, targets = P.cuda(), sym.cuda(), targets.cuda()
    _, want = _intervals(False, P, sym, targets, C, K, rgb)
    tabs = [ops.dmll_cdf_table(P, None, targets, C, K, rgb, c, 0, HW) for c in range(C)]       # (B, HW, Lp) each
    rows = torch.stack(tabs, dim=1).reshape(B * C * HW, targets.shape[0])                      # stream order b * C + c
    got = ops.intervals_from_table(rows, sym.reshape(B * C, HW), B * C, HW)
    assert torch.equal(got, want), int((got != want).sum())
    part = ops.dmll_cdf_table(P, None, targets, C, K, rgb, 2, 33, HW - 33)
    assert torch.equal(part, tabs[2][:, 33:])
