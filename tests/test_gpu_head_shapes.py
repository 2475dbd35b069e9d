"""-m gpu: the mixture-head kernels of csrc/dmll_kernels.hip at the (C, K, alphabet) the C ABI admits besides the two shipped heads
(ref64.HEAD_SHAPES: what each row is there for).  Every kernel takes C, K, rgb and the alphabet at run time; Kp = (4 | 3) C K decides the
form of the P tile's fill (16-byte pieces, 16-byte pieces placed as two halves, 8-byte halves, single floats), C the threads per block and
the turns of the compute loop, K how full the kMaxK register arrays are, Kp again whether the tile fits LDS.

Two kinds of check.  WITHOUT A TOLERANCE (every shape, W = 1, 63, 64, 65, 165 with B = 3, H = 1, so that at odd W the images 1 and 2 start off
16-byte alignment): the same P 0, 8 and 4 bytes past a 16-byte boundary gives the same bits from every kernel (the fill only moves data) and
nothing outside an output is written; the encoder's interval words are the decoder's table rows; window rows are slices of full rows; one
range-coded round trip.  A wrong row index in the fill moves one pixel's parameters into another pixel's slot -- encoder and decoder share the
fill, so a round trip cannot see that, the other forms of the fill and fp64 can.  AGAINST FP64 (every shape at W = 165): the rules of
tests/test_gpu_head_regimes.py and tests/test_gpu_preview.py, unchanged; tests/test_ref64.py runs the oracle through them on the same inputs.
Which fill form and which block size a case must take is asserted from its inputs alone, and that all of them occur."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dmll as odmll  # noqa: E402
from tests import ref64  # noqa: E402

B = 3
WIDTHS = (1, 63, 64, 65, 165)
W_MAX = 165
RANGES = ((0, 31), (0, 32), (1, 33), (3, 64))        # (pix0, npix) of the table kernel inside W = 165, besides the whole image
OFFSETS = (0, 8, 4)                                   # bytes past a 16-byte boundary
HEAD_PIX, TABLE_PIX, MAX_K = 64, 32, 16               # csrc/dmll_kernels.hip: kHeadPix, kTablePix, kMaxK
MARGIN, FILL = 256, 0xA5                              # bytes on either side of an output, and what they hold

SHAPES = [pytest.param(*s, id=ref64.shape_id(*s)) for s in ref64.HEAD_SHAPES]
SHAPE_SIZES = [pytest.param(*s, W, id='{}-W{}'.format(ref64.shape_id(*s), W)) for s in ref64.HEAD_SHAPES for W in WIDTHS]
SHAPE_REGIMES = [pytest.param(*s, regime, id='{}-{}'.format(ref64.shape_id(*s), regime))
                 for s in ref64.HEAD_SHAPES for regime in ref64.shape_regimes(s[2])]


def _kp(C, K, rgb):
    return (4 if rgb else 3) * C * K


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nhwc(P):
    return torch.from_numpy(P).permute(0, 2, 3, 1).contiguous().cuda()


def _at_offset(t, offset):
    """The same values, contiguous, `offset` bytes (a multiple of 4) past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[offset // 4:offset // 4 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == offset
    return out


def _ranges(W):
    return ((0, W),) + (RANGES if W == W_MAX else ())


# ---- which form of the fill, which block size: from the inputs alone ------------------------------------------------------------------


def _tile_div(Kp, max_pix):
    """tile_div_checked: (vec, q) of the vector fill, or (0, 0) where the host falls back to single floats -- odd Kp, or a reciprocal that is
    not exact for every piece index of a tile."""
    if Kp % 2:
        return 0, 0
    vec = 4 if Kp % 4 == 0 else 2
    q = Kp // vec
    magic = ((1 << 20) + q - 1) // q
    i = np.arange(max_pix * q, dtype=np.int64)
    if (i * magic > 0xffffffff).any() or ((i * magic) >> 20 != i // q).any():
        return 0, 0
    return vec, q


def _fill_form(Kp, max_pix, address):
    """fill_tile's choice for a tile whose first byte is at `address` (only its value mod 16 matters)."""
    vec, _ = _tile_div(Kp, max_pix)
    a = address % 16
    if vec == 4 and a == 0:
        return '16'
    if vec == 2 and a == 0:
        return 'half'
    if vec == 2 and a % 8 == 0:
        return '8'
    return '4'


def _tile_forms(Kp, max_pix, base, W, pix0, npix):
    """Every tile of a launch over pixels [pix0, pix0 + npix) of B images of W pixels, P at address `base`: {(form, rows of the tile)}."""
    return {(_fill_form(Kp, max_pix, base + 4 * Kp * (b * W + pix0 + off)), min(max_pix, npix - off))
            for b in range(B) for off in range(0, npix, max_pix)}


def _interval_threads(C, K, rgb):
    """l3c_dmll_encode_intervals: (the run-time kernel?, threads per block)."""
    compiled = (C, K, rgb) in ((3, 10, True), (5, 10, False))
    return not compiled, 320 if HEAD_PIX * C == 320 else 256


def test_the_cases_reach_every_fill_form_and_both_block_sizes():
    """From the parametrisation alone: every even Kp of the table takes the vector fill (the host's reciprocal is exact, no silent fall-back);
    all four forms occur at both tile heights; the half form meets a tile with an odd number of rows (its single trailing 8-byte load) and
    rows shorter than a piece's reach (q = 3: nearly every piece straddles two rows); the run-time interval kernel is launched with 320 and
    with 256 threads, with more than one turn of its compute loop, a partial last turn included; K = 1 and K = kMaxK occur."""
    forms = {HEAD_PIX: set(), TABLE_PIX: set()}
    half_odd = {HEAD_PIX: False, TABLE_PIX: False}
    threads, turns = set(), set()
    for C, K, rgb, alpha in ref64.HEAD_SHAPES:
        Kp = _kp(C, K, rgb)
        for max_pix in (HEAD_PIX, TABLE_PIX):
            assert _tile_div(Kp, max_pix) == ((0, 0) if Kp % 2 else (4, Kp // 4) if Kp % 4 == 0 else (2, Kp // 2)), (Kp, max_pix)
        rt, nt = _interval_threads(C, K, rgb)
        assert rt
        threads.add(nt)
        turns.add(HEAD_PIX * C / nt)
        for W in WIDTHS:
            for offset in OFFSETS:
                got = _tile_forms(Kp, HEAD_PIX, offset, W, 0, W)
                forms[HEAD_PIX] |= {f for f, _ in got}
                half_odd[HEAD_PIX] |= any(f == 'half' and n % 2 for f, n in got)
                for p0, n in _ranges(W):
                    got = _tile_forms(Kp, TABLE_PIX, offset, W, p0, n)
                    forms[TABLE_PIX] |= {f for f, _ in got}
                    half_odd[TABLE_PIX] |= any(f == 'half' and n % 2 for f, n in got)
    assert forms[HEAD_PIX] == forms[TABLE_PIX] == {'16', 'half', '8', '4'}, forms
    assert half_odd[HEAD_PIX] and half_odd[TABLE_PIX]
    assert threads == {256, 320} and {1.0, 1.75, 2.0} <= turns, (threads, turns)
    assert HEAD_PIX * (max(_kp(C, K, rgb) for C, K, rgb, _ in ref64.HEAD_SHAPES) + 1) * 4 == 64 * 1024          # the LDS limit, to the byte
    ks = {K for _, K, _, _ in ref64.HEAD_SHAPES}
    assert 1 in ks and MAX_K in ks
    assert 3 in {_tile_div(_kp(C, K, rgb), HEAD_PIX)[1] for C, K, rgb, _ in ref64.HEAD_SHAPES if _kp(C, K, rgb) % 4 == 2}


# ---- every kernel once, every output between sentinel margins ---------------------------------------------------------------------------


class Guarded(object):
    """An output of `shape` inside a byte buffer that holds FILL everywhere else (and, before the call, there as well)."""

    def __init__(self, shape, dtype):
        self.n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((self.n + 2 * MARGIN,), FILL, dtype=torch.uint8, device='cuda')
        self.out = self.buf[MARGIN:MARGIN + self.n].view(dtype).view(shape)
        assert self.out.is_contiguous() and self.out.data_ptr() == self.buf.data_ptr() + MARGIN

    def intact(self):
        return bool((self.buf[:MARGIN] == FILL).all()) and bool((self.buf[MARGIN + self.n:] == FILL).all())


def _inputs(C, K, rgb, alpha, regime, W):
    """-> P, sym (numpy) and, on the device: P (B, 1, W, Kp), sym, the values of sym, the bin edges, the two sets of uniforms."""
    P, sym = ref64.shape_case(C, K, rgb, alpha, regime, 1, W)
    rng = np.random.RandomState(W + 1000 * K)
    u_mix = rng.uniform(1e-5, 1 - 1e-5, size=(B, C, K, 1, W)).astype(np.float32)
    u_log = rng.uniform(1e-5, 1 - 1e-5, size=(B, C, 1, W)).astype(np.float32)
    return P, sym, u_mix, u_log, (_nhwc(P), _dev(sym), _dev(ref64.values_at(sym, alpha)), _dev(ref64.targets_of(alpha)), _dev(u_mix), _dev(u_log))


def _run_all(dev, C, K, rgb, alpha, W):
    """l3c_dmll_channel_params, l3c_dmll_cdf_table (every range of _ranges(W); RGB: window rows as well), l3c_dmll_encode_intervals,
    l3c_dmll_nll, l3c_dmll_sample and l3c_dmll_mean on P, each output a Guarded.  -> [(what, Guarded)]."""
    from l3c_pytorch_amd import _lib, ops
    Pd, symd, xd, td, umd, uld = dev
    assert tuple(Pd.shape) == (B, 1, W, _kp(C, K, rgb))
    Lp = td.shape[0]
    p, s = ops.ptr, ops.stream()
    sym_or_null = p(symd, torch.int16) if rgb else None
    out = []

    def new(what, shape, dtype):
        g = Guarded(shape, dtype)
        out.append((what, g))
        return g

    for c in range(C):
        pi, mu, ls = (new('params c{} {}'.format(c, n), (B, K, 1, W), torch.float32) for n in ('pi', 'mu', 'log_sigma'))
        _lib.call('l3c_dmll_channel_params', p(Pd, torch.float32), sym_or_null, B, W, C, K, int(rgb), c, p(pi.out), p(mu.out), p(ls.out), s)
        for p0, n in _ranges(W):
            for window in ((False, True) if rgb else (False,)):
                what = 'table c{} [{}, {}){}'.format(c, p0, p0 + n, ' window rows' if window else '')
                tab, flag = new(what, (B, n, Lp), torch.int16), new(what + ' flag', (1,), torch.int32)
                flag.out.zero_()
                stats = torch.zeros(B, dtype=torch.int32, device='cuda') if window else None
                _lib.call('l3c_dmll_cdf_table', p(Pd, torch.float32), sym_or_null, p(td, torch.float32), B, W, C, K, int(rgb), c, p0, n, Lp,
                          p(tab.out), p(flag.out), p(stats) if window else None, s)
    iv = new('intervals', (_lib.load().l3c_interval_words(B * C, W),), torch.int32)
    _lib.call('l3c_dmll_encode_intervals', p(Pd, torch.float32), p(symd, torch.int16), p(td, torch.float32), B, W, C, K, int(rgb), Lp, p(iv.out), s)
    nll = new('nll', (B, C, 1, W), torch.float32)
    _lib.call('l3c_dmll_nll', p(Pd, torch.float32), p(xd, torch.float32), B, W, C, K, int(rgb), alpha[0], alpha[1], alpha[2], p(nll.out), s)
    smp = new('sample', (B, C, 1, W), torch.float32)
    _lib.call('l3c_dmll_sample', p(Pd, torch.float32), p(umd, torch.float32), p(uld, torch.float32), B, W, C, K, int(rgb), p(smp.out), s)
    mean = new('mean', (B, C, 1, W), torch.int16)
    _lib.call('l3c_dmll_mean', p(Pd, torch.float32), B, W, C, K, int(rgb), alpha[0], alpha[1], alpha[2], p(mean.out), s)
    return out


@pytest.mark.parametrize('C,K,rgb,alpha,W', SHAPE_SIZES)
def test_alignment_changes_no_bit_and_nothing_is_written_outside(C, K, rgb, alpha, W):
    """Every kernel on P at 0, 8 and 4 bytes past a 16-byte boundary: the outputs -- and the FILL bytes around them -- are the same bytes, and
    the margins still hold FILL.  The three copies take different forms of the fill (asserted from Kp and the addresses: the aligned copy
    the widest form its Kp admits somewhere, the copy 4 bytes off single floats everywhere)."""
    Kp = _kp(C, K, rgb)
    for regime in ref64.shape_regimes(rgb):
        dev = _inputs(C, K, rgb, alpha, regime, W)[-1]
        runs, forms = [], []
        for offset in OFFSETS:
            Pv = _at_offset(dev[0], offset)
            assert torch.equal(Pv, dev[0])
            forms.append({f for f, _ in _tile_forms(Kp, HEAD_PIX, Pv.data_ptr(), W, 0, W)})
            runs.append(_run_all((Pv,) + dev[1:], C, K, rgb, alpha, W))
        assert ('16' if Kp % 4 == 0 else 'half' if Kp % 2 == 0 else '4') in forms[0], forms
        assert forms[1] == ({'4'} if Kp % 4 != 2 else {'8', 'half'} if W % 2 else {'8'}), forms
        assert forms[2] == {'4'}, forms
        for what, g in runs[0]:
            assert g.intact(), '{} {}: wrote outside its output'.format(regime, what)
        for offset, run in zip(OFFSETS[1:], runs[1:]):
            for (what, g0), (_, g) in zip(runs[0], run):
                assert torch.equal(g.buf, g0.buf), '{} {}: P {} bytes off alignment changes {} bytes'.format(
                    regime, what, offset, int((g.buf != g0.buf).sum()))


# ---- encoder and decoder -----------------------------------------------------------------------------------------------------------------


def _table(Pd, symd, td, C, K, rgb, c, p0, n, window_stats=None):
    """-> (rows (B, n, Lp) int16 on the device, the same as int64 numpy in 0 .. 65535, flag)."""
    from l3c_pytorch_amd import ops
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    tab = ops.dmll_cdf_table(Pd, symd if rgb else None, td, C, K, rgb, c, p0, n, flag, window_stats=window_stats)
    return tab, ref64.as_u16(tab), int(flag.item())


def _params(Pd, symd, C, K, rgb, c):
    from l3c_pytorch_amd import ops
    return ops.dmll_channel_params(Pd, symd if rgb else None, C, K, rgb, c)


def _unpack_intervals(iv, n_streams, n_sym):
    """include/l3c_hip.h: word(stream s, symbol t, role r) = iv[(((t / 64) * n_streams + s) * 2 + r) * 64 + t % 64]; role 0 = c_low,
    role 1 = 65536 - c_high.  -> c_low, c_high (n_streams, n_sym) int64."""
    iv = iv.cpu().numpy().view(np.uint32).astype(np.int64)
    t = np.arange(n_sym)[None, :]
    s = np.arange(n_streams)[:, None]
    base = (((t // 64) * n_streams + s) * 2) * 64 + t % 64
    return iv[base], 65536 - iv[base + 64]


@pytest.mark.parametrize('C,K,rgb,alpha,W', SHAPE_SIZES)
def test_interval_words_are_the_table_rows(C, K, rgb, alpha, W):
    """l3c_dmll_encode_intervals (64-pixel tiles; 320 or 256 threads, one to two turns) against l3c_ac_intervals_from_table on the rows of
    l3c_dmll_cdf_table (32-pixel tiles, 256 threads): every word of every channel equal, both edge symbols of the alphabet among the symbols,
    the words past W zero.  The sub-ranges are rows of the full table; the fused table is the two-kernel one (l3c_dmll_channel_params +
    l3c_cdf_table_mixture).  RGB: window rows are slices of the full rows, by the rule of tests/test_gpu_head_regimes.py."""
    from l3c_pytorch_amd import ops
    L = alpha[2]
    for regime in ref64.shape_regimes(rgb):
        P, sym, _, _, (Pd, symd, _, td, _, _) = _inputs(C, K, rgb, alpha, regime, W)
        Lp = td.shape[0]
        assert (sym == 0).any() and (sym == L - 1).any()
        iv = ops.dmll_encode_intervals(Pd, symd, td, C, K, rgb)
        fulls = []
        for c in range(C):
            what = (regime, c)
            tab, full, flag = _table(Pd, symd, td, C, K, rgb, c, 0, W)
            fulls.append(tab)
            assert flag == int(not ref64.rows_increasing(full).all()), what
            pi, mu, ls = _params(Pd, symd, C, K, rgb, c)
            two, _ = ops.cdf_table_mixture(td, pi, mu, ls)
            assert torch.equal(two.reshape(B, W, Lp), tab), what
            for p0, n in _ranges(W)[1:]:
                _, part, pflag = _table(Pd, symd, td, C, K, rgb, c, p0, n)
                assert np.array_equal(part, full[:, p0:p0 + n]), (what, p0, n)
                assert pflag == int(not ref64.rows_increasing(part).all()), (what, p0, n)
            if rgb:
                stats = torch.zeros(B, dtype=torch.int32, device='cuda')
                mean = (pi.cpu().numpy().astype(np.float64) * mu.cpu().numpy()).sum(axis=1).reshape(B, W)
                want_w0 = np.clip(np.floor(np.clip(mean, 0, 255)) - 31, 0, 192)
                for p0, n in _ranges(W):
                    _, mixed, wflag = _table(Pd, symd, td, C, K, True, c, p0, n, window_stats=stats)
                    wins = mixed.reshape(B, -1)[:, :n * 65].reshape(B, n, 65)
                    assert wflag == int(not (np.diff(wins[..., :64], axis=-1) > 0).all()), (what, p0, n)
                    w0 = wins[..., 64]
                    assert w0.min() >= 0 and w0.max() <= 192
                    assert np.abs(w0 - want_w0[:, p0:p0 + n]).max() <= 1, (what, p0, n)      # (the kernel sums pi_k mu_k sequentially in fp32)
                    rows = np.take_along_axis(full[:, p0:p0 + n], w0[..., None] + np.arange(64)[None, None, :], -1)
                    assert np.array_equal(wins[..., :64], rows), (what, p0, n)
                    if flag == 0:
                        assert wflag == 0
        rows = torch.stack(fulls, dim=1).reshape(B * C * W, Lp)                             # stream order b * C + c
        want = ops.intervals_from_table(rows, symd.reshape(B * C, W), B * C, W)
        assert torch.equal(iv, want), '{}: {} of {} words differ'.format(regime, int((iv != want).sum()), iv.numel())
        if W % 64:                                                                          # [t / 64][stream][role][64]: the pixels past W
            assert bool((iv.view(-1, B * C, 2, 64)[-1, :, :, W % 64:] == 0).all()), regime


@pytest.mark.parametrize('C,K,rgb,alpha', SHAPES)
def test_round_trip(C, K, rgb, alpha):
    """`benign` at W = 165: intervals -> l3c_ac_encode -> tables -> l3c_ac_decode gives the symbols back.  The rows must be strictly increasing
    (every term of the sum is a nondecreasing function of the bin edge, rounded additions keep that, the entry adds l) and flagged so.
    Lp = 260 is a refusal case: l3c_ac_decode takes Lp <= 257 and says so; the encoder's side and the table are still produced."""
    from l3c_pytorch_amd import _lib, ops
    W = W_MAX
    _, _, _, _, (Pd, symd, _, td, _, _) = _inputs(C, K, rgb, alpha, 'benign', W)
    Lp = td.shape[0]
    iv = ops.dmll_encode_intervals(Pd, symd, td, C, K, rgb)
    tabs = []
    for c in range(C):
        tab, full, flag = _table(Pd, symd, td, C, K, rgb, c, 0, W)
        assert flag == 0 and ref64.rows_increasing(full).all(), c
        tabs.append(tab)
    table_all = torch.stack(tabs, dim=1).reshape(B * C * W, Lp).contiguous()
    out, n = ops.ac_encode(iv, B * C, W)
    n, out = n.cpu().numpy(), out.cpu().numpy()
    assert (n > 0).all()
    buf, offs, lens = ops.pack_streams([out[i, :n[i]].tobytes() for i in range(B * C)])
    if Lp > 257:
        with pytest.raises(_lib.L3CError, match=r'Lp out of range \(2\.\.257\)'):
            ops.ac_decode(table_all, buf, offs, lens, B * C, W, True)
        return
    dec = ops.ac_decode(table_all, buf, offs, lens, B * C, W, True).reshape(B, C, 1, W)
    assert torch.equal(dec, symd)


# ---- against fp64 ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('C,K,rgb,alpha,regime', SHAPE_REGIMES)
def test_parameters_table_and_intervals_vs_fp64(C, K, rgb, alpha, regime):
    """W = 165, the rules of tests/test_gpu_head_regimes.py: log_sigma bit-equal to max(P, -7), |pi - pi64| <= PI_BOUND, the (coupled) mean
    within mu_bound64; every table entry and both entries of every interval through ref64.check_entries on the parameters the device
    computed, the two shares pooled over the channels and capped; c_high == 65536 exactly at the top symbol; rows that increase in fp64
    increase, and the flag says what the rows do."""
    from l3c_pytorch_amd import ops
    W, L = W_MAX, alpha[2]
    t = ref64.targets_of(alpha)
    Lp = t.shape[0]
    P, sym, _, _, (Pd, symd, _, td, _, _) = _inputs(C, K, rgb, alpha, regime, W)
    x = ref64.values_at(sym, alpha)
    c_low, c_high = _unpack_intervals(ops.dmll_encode_intervals(Pd, symd, td, C, K, rgb), B * C, W)
    c_low, c_high = c_low.reshape(B, C, W), c_high.reshape(B, C, W)
    tables, intervals = ref64.EntryStats(), ref64.EntryStats()
    worst_pi = worst_mu = 0.0
    for c in range(C):
        what = '{} {} c{}'.format(ref64.shape_id(C, K, rgb, alpha), regime, c)
        pi, mu, ls = [v.cpu().numpy() for v in _params(Pd, symd, C, K, rgb, c)]
        pi64, mu64, ls64 = ref64.params64(P, x, rgb, C, K, c)
        want_ls = np.maximum(P.reshape(B, -1, C, K, 1, W)[:, 2, c], np.float32(-7))
        assert ls.tobytes() == want_ls.tobytes() and (ls.astype(np.float64) == ls64).all(), what
        e_pi = np.abs(pi - pi64).max() / ref64.PI_BOUND
        r_mu = (np.abs(mu - mu64) / np.maximum(ref64.mu_bound64(P, x, rgb, C, K, c), 1e-300)).max()
        worst_pi, worst_mu = max(worst_pi, e_pi), max(worst_mu, r_mu)
        assert e_pi <= 1, (what, e_pi)
        assert r_mu <= 1, (what, r_mu)
        assert np.abs(pi.sum(axis=1) - 1).max() < 1e-5
        _, full, flag = _table(Pd, symd, td, C, K, rgb, c, 0, W)
        ref64.check_entries(full.reshape(B, 1, W, Lp), pi, mu, ls, t, what=what, stats=tables)
        e64 = ref64.entries64(ref64.cdf64(pi, mu, ls, t), Lp)
        inc64 = ref64.rows_increasing(e64).reshape(B, W)
        assert ref64.rows_increasing(full)[inc64].all(), what
        assert flag == int(not ref64.rows_increasing(full).all()), (what, flag)
        s = sym[:, c].astype(np.int64)
        top = (s == L - 1).reshape(B, W)
        assert (c_high[:, c][top] == 65536).all() and (c_high[:, c][~top] < 65536).all(), what
        assert (c_low[:, c] >= 0).all() and (c_low[:, c] < 65536).all()
        got = np.stack([c_low[:, c], c_high[:, c]], axis=-1).reshape(B, 1, W, 2)
        got[..., 1] = np.where(top.reshape(B, 1, W), e64[..., L], got[..., 1])     # entry L is never read (the top symbol's c_high is 2^16)
        ref64.check_entries(got, pi, mu, ls, t, index=np.stack([s, s + 1], axis=-1), what=what + ' intervals', stats=intervals)
    print('SHAPE {} {}: |pi - pi64| / PI_BOUND <= {:.3f}, |mu - mu64| / bound <= {:.3f}; table: {}; intervals: {}'.format(
        ref64.shape_id(C, K, rgb, alpha), regime, worst_pi, worst_mu, tables, intervals))
    tables.assert_caps((C, K, rgb, alpha, regime, 'table'))
    intervals.assert_caps((C, K, rgb, alpha, regime, 'intervals'))


@pytest.mark.parametrize('C,K,rgb,alpha', SHAPES)
def test_nll_sample_and_mean_vs_fp64(C, K, rgb, alpha):
    """W = 165.  l3c_dmll_nll against the oracle's fp32 NLL within ref64.nll_tolerance (the slack term above 1e-3 on < 2 %), -log 1e-12 where
    every component sits at the mass clamp; l3c_dmll_sample against the oracle on the same draws by the rule of
    test_sample_kernel_at_ragged_tiles; l3c_dmll_mean by ref64.mean_rule64, the excused share of the shape capped at 2 %."""
    from l3c_pytorch_amd import ops
    W = W_MAX
    spec = odmll.Spec(rgb, alpha[0], alpha[1], alpha[2])
    name = ref64.shape_id(C, K, rgb, alpha)
    n_mean = n_excused = 0
    for regime in ref64.shape_regimes(rgb):
        P, sym, u_mix, u_log, (Pd, symd, xd, td, umd, uld) = _inputs(C, K, rgb, alpha, regime, W)
        x = ref64.values_at(sym, alpha)
        got = ops.dmll_nll(Pd, xd, C, K, rgb, alpha[0], alpha[1], alpha[2]).cpu().numpy()
        ref32 = odmll.nll(spec, torch.from_numpy(x), torch.from_numpy(P)).numpy()
        r64, clamped = ref64.nll64(P, x, rgb, C, K, return_clamped=True, alpha=alpha)
        tol, share = ref64.nll_tolerance(ref32, r64)
        err = np.abs(got.astype(np.float64) - ref32)
        print('SHAPE {} {}: nll max error / tolerance = {:.3f}, slack term above 1e-3 on {:.3%}, at the clamp {}'.format(
            name, regime, (err / tol).max(), share, int(clamped.sum())))
        assert np.isfinite(got).all()
        assert (err <= tol).all(), (regime, (err / tol).max())
        assert share < ref64.NLL_SLACK_SHARE, (regime, share)
        if clamped.any():
            assert np.abs(got[clamped] + np.log(1e-12)).max() < 1e-4

        smp = ops.dmll_sample(Pd, umd, uld, C, K, rgb).cpu()
        want = odmll.sample(spec, torch.from_numpy(P), C, torch.from_numpy(u_mix), torch.from_numpy(u_log))
        assert smp.shape == want.shape == (B, C, 1, W)
        bad = ((smp - want).abs() > 2e-3).float().mean().item()
        assert bad < 1e-3, (regime, bad)
        if rgb:
            assert smp.min() >= 0 and smp.max() <= 255

        if regime in ref64.mean_regimes(rgb, K):
            mean = ops.dmll_mean(Pd, C, K, rgb, alpha[0], alpha[1], alpha[2]).cpu().numpy().astype(np.int64)
            assert mean.shape == (B, C, 1, W) and mean.min() >= 0 and mean.max() <= alpha[2] - 1
            for c in range(C):
                want_sym, excused = ref64.mean_rule64(P, mean, rgb, C, K, alpha, c)
                wrong = (mean[:, c] != want_sym) & ~excused
                assert not wrong.any(), (regime, c, int(wrong.sum()), mean[:, c][wrong][:4], want_sym[wrong][:4])
                n_mean, n_excused = n_mean + excused.size, n_excused + int(excused.sum())
    print('SHAPE {}: mean excused {:.3%} of {}'.format(name, n_excused / n_mean, n_mean))
    assert n_excused <= ref64.MEAN_EXCUSED_CAP * n_mean, (n_excused, n_mean)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------

REFUSAL_W = 5
LDS = 'Kp too large for the LDS tile'
K_RANGE = r'K out of range \(1\.\.16\)'
BAD_SHAPE = 'bad shape'
LAMBDA = 'lambda coupling is only defined for C == 3'
LP_RANGE = r'Lp out of range \(2\.\.260\)'
WINDOW = r'window rows are defined for the 256-symbol alphabet \(Lp == 257\)'

# (call, C, K, rgb, Lp, window rows, the message)
REFUSALS = (
    [(call, C, K, False, 26, False, LDS) for call in ('intervals', 'nll', 'sample', 'mean') for C, K in ((8, 16), (43, 2))]   # Kp 384; 258: the first above 255
    + [('table', 11, 12, False, 26, False, LDS)]
    + [(call, 5, 17, False, 26, False, K_RANGE) for call in ('table', 'two_kernel_table', 'nll', 'sample', 'mean')]
    + [('intervals', 5, 17, False, 26, False, 'K out of range')]
    + [(call, 5, 0, False, 26, False, K_RANGE) for call in ('table', 'two_kernel_table', 'nll', 'sample', 'mean')]
    + [(call, 5, 0, False, 26, False, BAD_SHAPE) for call in ('intervals', 'params')]
    + [(call, C, 4, True, 257, False, LAMBDA) for call in ('params', 'table', 'intervals', 'nll', 'sample', 'mean') for C in (1, 5)]
    + [(call, 5, 4, False, Lp, False, LP_RANGE) for call in ('table', 'two_kernel_table') for Lp in (261, 1)]
    + [('table', 3, 4, True, 256, True, WINDOW), ('table', 5, 4, False, 26, True, WINDOW)]
)


@pytest.mark.parametrize('call,C,K,rgb,Lp,window,message', [pytest.param(*r, id='{}-C{}K{}{}Lp{}{}'.format(
    r[0], r[1], r[2], 'rgb' if r[3] else 'z', r[4], 'w' if r[5] else '')) for r in REFUSALS])
def test_refusals(call, C, K, rgb, Lp, window, message):
    """What the ABI does not take returns L3C_ERR_INVALID_ARG with its message and launches nothing: the output still holds FILL in every
    byte.  (Every buffer has the size the refused shape would need.)"""
    from l3c_pytorch_amd import _lib, ops
    lib = _lib.load()
    W, Kp = REFUSAL_W, max(_kp(C, K, rgb), 1)
    p, s = ops.ptr, ops.stream()
    Pd = torch.zeros(B, 1, W, Kp, device='cuda')
    symd = torch.zeros(B, C, 1, W, dtype=torch.int16, device='cuda')
    xd = torch.zeros(B, C, 1, W, device='cuda')
    td = torch.linspace(-1, 1, max(Lp, 1), device='cuda')
    um = torch.full((B, C, max(K, 1), 1, W), 0.5, device='cuda')
    par = torch.zeros(3, B, max(K, 1), 1, W, device='cuda')
    stats = torch.zeros(B, dtype=torch.int32, device='cuda')
    if call == 'params':
        g = Guarded((3, B, max(K, 1), 1, W), torch.float32)
        rc = lib.l3c_dmll_channel_params(p(Pd), p(symd), B, W, C, K, int(rgb), 0, p(g.out[0]), p(g.out[1]), p(g.out[2]), s)
    elif call == 'table':
        g = Guarded((B, W, max(Lp, 1)), torch.int16)
        rc = lib.l3c_dmll_cdf_table(p(Pd), p(symd), p(td), B, W, C, K, int(rgb), 0, 0, W, Lp, p(g.out), None, p(stats) if window else None, s)
    elif call == 'two_kernel_table':
        g = Guarded((B, W, max(Lp, 1)), torch.int16)
        rc = lib.l3c_cdf_table_mixture(p(td), p(par[0]), p(par[1]), p(par[2]), B, W, K, Lp, p(g.out), None, s)
    elif call == 'intervals':
        g = Guarded((lib.l3c_interval_words(B * C, W),), torch.int32)
        rc = lib.l3c_dmll_encode_intervals(p(Pd), p(symd), p(td), B, W, C, K, int(rgb), Lp, p(g.out), s)
    elif call == 'nll':
        g = Guarded((B, C, 1, W), torch.float32)
        rc = lib.l3c_dmll_nll(p(Pd), p(xd), B, W, C, K, int(rgb), -1.0, 1.0, 25, p(g.out), s)
    elif call == 'sample':
        g = Guarded((B, C, 1, W), torch.float32)
        rc = lib.l3c_dmll_sample(p(Pd), p(um), p(xd), B, W, C, K, int(rgb), p(g.out), s)
    else:
        assert call == 'mean'
        g = Guarded((B, C, 1, W), torch.int16)
        rc = lib.l3c_dmll_mean(p(Pd), B, W, C, K, int(rgb), -1.0, 1.0, 25, p(g.out), s)
    error = lib.l3c_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -1 and re.search(message, error), (rc, error)                     # include/l3c_hip.h: L3C_ERR_INVALID_ARG
    assert bool((g.buf == FILL).all()), 'a refused call wrote to its output'

