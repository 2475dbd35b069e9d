"""l3c_dmll_conceal (include/l3c_hip.h, csrc/dmll_kernels.hip: dmll_conceal_kernel) on its own: the estimator of l3c_dmll_mean on pixel
spans of decoded RGB symbols, conditioned on the channels that are kept.

B = 2 images of HW = 209 pixels -- three full tiles of 64 and one of 17 --, K = 10, L = 256, random P (ref64.make_P, `benign`), the symbols
pre-filled with in-range random values between guard bytes.  With replace == 7 a span must hold the bits of l3c_dmll_mean; with a partial
mask the kept channels are untouched and the others follow the rule in fp64, evaluated from P and the symbols the call left behind.  The
one test that needs no GPU checks that the inputs themselves keep the fp64 rule's near-tie share below its cap."""
import numpy as np
import pytest
import torch

from tests import ref64

B, HW, K = 2, 209, 10
ALPHA = (0.0, 255.0, 256)
SEED = 20
NAN_PIXEL = (1, 140)                     # (image, pixel): its whole P record is NaN
NEAR, NEAR_CAP = 1e-3, 0.01              # distance from a rounding boundary, in symbols, inside which +-1 is allowed; the share it may cover
FULL = [(0, 0, 64, 7), (0, 128, 81, 7), (1, 64, 1, 7), (1, 128, 0, 7)]
MIXED = [(0, 0, 64, 1), (0, 64, 64, 6), (0, 128, 81, 5), (1, 0, 64, 2), (1, 64, 64, 3), (1, 128, 81, 4)]


def uniform(mask):
    return [(0, 0, 209, mask), (1, 64, 145, mask)]


RUNS = [uniform(m) for m in range(1, 7)] + [MIXED]


def inputs():
    """P (B, 12 K, 1, HW) fp32 with one NaN record, the symbols the buffer holds before a call (B, 3, 1, HW) int16."""
    rng = np.random.RandomState(SEED)
    P = ref64.make_P('benign', True, B, 1, HW, 3, K, rng)
    P[NAN_PIXEL[0], :, 0, NAN_PIXEL[1]] = np.nan
    return P, ref64.make_sym(True, B, 1, HW, 3, rng)


def replaced(spans):
    """-> bool (B, 3, 1, HW): the (image, channel, pixel) items the spans overwrite."""
    from l3c_pytorch_amd import ops
    r = np.zeros((B, 3, 1, HW), dtype=bool)
    for s in ops.conceal_spans(spans):          # the table the call is handed
        for c in range(3):
            if int(s['replace']) >> c & 1:
                r[int(s['image']), c, 0, int(s['pix0']):int(s['pix0'] + s['npix'])] = True
    return r


def scaled_mean64(P, sym, c):
    """The rule in fp64 for channel c, conditioned on the values of `sym`'s channels below c: the clamped mean in symbol units (a NaN record
    gives NaN)."""
    pi, mu, _ = ref64.params64(P, ref64.values_at(sym, ALPHA), True, 3, K, c)
    bw = (ALPHA[1] - ALPHA[0]) / (ALPHA[2] - 1)
    return (np.clip((pi * mu).sum(axis=1), ALPHA[0], ALPHA[1]) - ALPHA[0]) / bw


def near_boundary(t):
    with np.errstate(invalid='ignore'):
        return np.abs(t - np.floor(t) - 0.5) <= NEAR


def judge(P, before, after, spans):
    """`after` (what a call left of `before`) against the rule -> (items judged, items within NEAR of a rounding boundary)."""
    rep = replaced(spans)
    assert (after[~rep] == before[~rep]).all(), 'a kept symbol changed'
    nan = np.zeros((B, 1, HW), dtype=bool)
    nan[NAN_PIXEL[0], 0, NAN_PIXEL[1]] = True
    items = near_items = 0
    for c in range(3):
        with np.errstate(invalid='ignore'):
            t = scaled_mean64(P, after, c)
        sel = rep[:, c] & ~nan
        assert np.isfinite(t[sel]).all()
        want = np.clip(np.rint(t), 0, ALPHA[2] - 1)
        near = near_boundary(t)
        got = after[:, c].astype(np.float64)
        assert (got[sel & ~near] == want[sel & ~near]).all(), (c, np.argwhere(sel & ~near & (got != want))[:5])
        assert (np.abs(got[sel & near] - want[sel & near]) <= 1).all(), c
        assert (got[rep[:, c] & nan] == 0).all(), 'a NaN record snaps to x_min'
        items += int(sel.sum())
        near_items += int((sel & near).sum())
    return items, near_items


def test_the_inputs_keep_the_fp64_rule_inside_its_cap():
    """No GPU: the rule applied in fp64 alone, channel by channel on its own results, for every run of the partial-mask test.  The share of
    items whose fp64 mean lies within 1e-3 of a rounding boundary must be below 1 % (about 0.2 % for spread-out fractional parts); the
    seed is chosen so that it is."""
    P, before = inputs()
    items = near_items = 0
    for spans in RUNS:
        rep = replaced(spans)
        sym = before.copy()
        for c in range(3):
            with np.errstate(invalid='ignore'):
                t = scaled_mean64(P, sym, c)
            q = np.clip(np.rint(np.nan_to_num(t)), 0, ALPHA[2] - 1).astype(np.int16)
            sym[:, c][rep[:, c]] = q[rep[:, c]]
        n, m = judge(P, before, sym, spans)
        items, near_items = items + n, near_items + m
    assert items == (354 * 9 + 64 + 2 * 64 + 2 * 81 + 64 + 2 * 64 + 81) - (9 + 1)      # the NaN pixel: in every uniform run and in MIXED's last span
    assert near_items < NEAR_CAP * items, (near_items, items)
    assert before.min() == 0 and before.max() == 255


# ---- on the device ---------------------------------------------------------------------------------------------------------------------


def _device():
    from tests.test_gpu_head_shapes import _nhwc
    P, before = inputs()
    return P, before, _nhwc(P)


def _conceal(Pd, before, spans, n_spans=None):
    """One l3c_dmll_conceal call on a guarded copy of `before` -> (the symbols after it as numpy, guards intact?)."""
    from l3c_pytorch_amd import _lib, ops
    from tests.test_gpu_head_shapes import Guarded
    g = Guarded(before.shape, torch.int16)
    g.out.copy_(torch.from_numpy(before))
    table = ops.conceal_spans(spans)
    table_d = ops.upload_small(table.view(np.int64)) if len(table) else None
    n = len(table) if n_spans is None else n_spans
    _lib.call('l3c_dmll_conceal', ops.ptr(Pd, torch.float32), B, HW, K, ALPHA[0], ALPHA[1], ALPHA[2], table.ctypes.data if len(table) else None,
              ops.ptr(table_d) if len(table) else None, n, ops.ptr(g.out, torch.int16), ops.stream())
    torch.cuda.synchronize()
    return g.out.cpu().numpy(), g.intact()


@pytest.mark.gpu
def test_replace_7_is_l3c_dmll_mean_bit_for_bit():
    from l3c_pytorch_amd import ops
    P, before, Pd = _device()
    mean = ops.dmll_mean(Pd, 3, K, True, *ALPHA).cpu().numpy()
    after, intact = _conceal(Pd, before, FULL)
    rep = replaced(FULL)
    assert rep.sum() == 3 * (64 + 81 + 1)
    assert intact
    assert (after[rep] == mean[rep]).all()
    assert (after[~rep] == before[~rep]).all()
    # the same through the wrapper, the whole frame as spans: the whole of l3c_dmll_mean
    sym = torch.from_numpy(before).cuda()
    ops.dmll_conceal(Pd, sym, [(0, 0, HW, 7), (1, 0, HW, 7)], K, *ALPHA)
    assert torch.equal(sym.cpu(), torch.from_numpy(mean))
    assert mean[NAN_PIXEL[0], :, 0, NAN_PIXEL[1]].tolist() == [0, 0, 0]


@pytest.mark.gpu
def test_partial_masks_follow_the_rule_in_fp64():
    P, before, Pd = _device()
    items = near_items = 0
    for spans in RUNS:
        after, intact = _conceal(Pd, before, spans)
        assert intact
        n, m = judge(P, before, after, spans)
        items, near_items = items + n, near_items + m
    print('items {}, within {} of a rounding boundary {}'.format(items, NEAR, near_items))
    assert near_items < NEAR_CAP * items, (near_items, items)


@pytest.mark.gpu
def test_nothing_to_do_leaves_the_symbols_untouched():
    from l3c_pytorch_amd import ops
    P, before, Pd = _device()
    for spans, n in (([], None), (FULL, 0), ([(b, p0, npix, 0) for b, p0, npix, _ in FULL], None), ([(0, 64, 0, 7), (1, 192, 0, 5)], None)):
        after, intact = _conceal(Pd, before, spans, n)
        assert intact and (after == before).all()
    sym = torch.from_numpy(before).cuda()
    assert ops.dmll_conceal(Pd, sym, [], K, *ALPHA) is sym and torch.equal(sym.cpu(), torch.from_numpy(before))
