"""-m gpu: the logistic-mixture head kernels (csrc/dmll_kernels.hip, csrc/dmll_core.h) against the plain fp64 references of
tests/ref64.py, in the value regimes where such kernels go wrong: the -7 clamp, means on bin edges, very wide and far-off components,
one-hot and flat softmax, saturated lambda coupling, the 1e-12 clamp of the NLL -- and the in-register monotonicity check shown rows
that violate it.  A lossless round trip cannot notice a wrong table (encoder and decoder share the device functions); these can.
tests/test_ref64.py runs the oracle through the same rules on the same inputs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cdf as ocdf, dmll as odmll  # noqa: E402
from tests import ref64  # noqa: E402

CASES = [pytest.param(regime, rgb, id='{}-{}'.format(regime, 'rgb' if rgb else 'z'))
         for rgb in (True, False) for regime in ref64.regimes(rgb)]
B = 2


def _name(rgb):
    return 'rgb' if rgb else 'z'


def _spec(rgb):
    return odmll.RGB if rgb else odmll.z_spec()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nhwc(P):
    return torch.from_numpy(P).permute(0, 2, 3, 1).contiguous().cuda()


def _misaligned(t):
    """The same values, contiguous, 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def _case(regime, rgb, H, W, **kw):
    P, sym, C, K = ref64.head_case(regime, rgb, H, W, **kw)
    return P, sym, C, K, _nhwc(P), _dev(sym), _dev(ref64.targets32(rgb))


def _params(Pd, symd, C, K, rgb, c):
    from l3c_pytorch_amd import ops
    return [v.cpu().numpy() for v in ops.dmll_channel_params(Pd, symd if rgb else None, C, K, rgb, c)]


def _table(Pd, symd, td, C, K, rgb, c, p0, n, window_stats=None):
    """-> (rows (B, n, Lp) int64 in 0 .. 65535, flag)."""
    from l3c_pytorch_amd import ops
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    tab = ops.dmll_cdf_table(Pd, symd if rgb else None, td, C, K, rgb, c, p0, n, flag, window_stats=window_stats)
    return ref64.as_u16(tab), int(flag.item())


def _unpack_intervals(iv, n_streams, n_sym):
    """include/l3c_hip.h: word(stream s, symbol t, role r) = iv[(((t / 64) * n_streams + s) * 2 + r) * 64 + t % 64]; role 0 = c_low,
    role 1 = 65536 - c_high.  -> c_low, c_high (n_streams, n_sym) int64."""
    iv = iv.cpu().numpy().view(np.uint32).astype(np.int64)
    t = np.arange(n_sym)[None, :]
    s = np.arange(n_streams)[:, None]
    base = (((t // 64) * n_streams + s) * 2) * 64 + t % 64
    return iv[base], 65536 - iv[base + 64]


# ---- 1. parameters ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('regime,rgb', CASES)
def test_channel_params_vs_fp64(regime, rgb):
    """l3c_dmll_channel_params against fp64 from P: log_sigma bit-equal to max(P, -7); |pi - pi64| <= 8 * 2^-24; the (coupled) mean within
    4 * 2^-24 * (|mu| + |sigmoid(lam) x0| + |sigmoid(lam) x1|), elementwise."""
    for (H, W) in ref64.SHAPES:
        P, sym, C, K, Pd, symd, _ = _case(regime, rgb, H, W)
        x = ref64.values_of(sym, rgb)
        for c in range(C):
            pi, mu, ls = _params(Pd, symd, C, K, rgb, c)
            pi64, mu64, ls64 = ref64.params64(P, x, rgb, C, K, c)
            want_ls = np.maximum(P.reshape(B, -1, C, K, H, W)[:, 2, c], np.float32(-7))
            assert ls.tobytes() == want_ls.tobytes(), (H, W, c)
            assert (ls.astype(np.float64) == ls64).all()
            e_pi = np.abs(pi - pi64).max()
            r_mu = (np.abs(mu - mu64) / np.maximum(ref64.mu_bound64(P, x, rgb, C, K, c), 1e-300)).max()
            print('{} {} {}x{} c{}: max |pi - pi64| = {:.2f} * 2^-24, max |mu - mu64| / bound = {:.3f}'.format(
                _name(rgb), regime, H, W, c, e_pi / ref64.U32, r_mu))
            assert e_pi <= ref64.PI_BOUND, (H, W, c, e_pi / ref64.U32)
            assert r_mu <= 1, (H, W, c, r_mu)
            assert np.abs(pi.sum(axis=1) - 1).max() < 1e-5


# ---- 2. table ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('regime,rgb', CASES)
def test_table_vs_fp64_on_its_own_parameters(regime, rgb):
    """l3c_dmll_cdf_table, every channel, the full range and the sub-ranges (7, 50) and (HW - 33, 33): every entry through
    ref64.check_entries on the parameters the device computed (test_channel_params_vs_fp64 ties those to P); rows strictly increasing
    over [0, Lp-2] and flag 0 wherever the fp64 rows are; a sub-range equals the full table's rows.  Channel 0 (no coupling) also against
    the oracle's table from the oracle's parameters: difference <= 1 on < 1 % of the entries.  (For c > 0 the figure is printed only:
    an ulp of the coupled mean times e^7.)  The two shares per channel at 12x20, pooled over the channels at the small shapes."""
    t = ref64.targets32(rgb)
    Lp = t.shape[0]
    for (H, W) in ref64.SHAPES:
        P, sym, C, K, Pd, symd, td = _case(regime, rgb, H, W)
        HW = H * W
        pooled = ref64.EntryStats()
        for c in range(C):
            what = '{} {} {}x{} c{}'.format(_name(rgb), regime, H, W, c)
            pi, mu, ls = _params(Pd, symd, C, K, rgb, c)
            full, flag = _table(Pd, symd, td, C, K, rgb, c, 0, HW)
            s = ref64.check_entries(full.reshape(B, H, W, Lp), pi, mu, ls, t, what=what, stats=pooled)
            if HW >= 240:
                s.assert_caps(what)
            inc64 = ref64.rows_increasing(ref64.entries64(ref64.cdf64(pi, mu, ls, t), Lp)).reshape(B, HW)
            assert ref64.rows_increasing(full)[inc64].all(), what
            assert flag == int(not ref64.rows_increasing(full).all()), (what, flag)
            if inc64.all():
                assert flag == 0, what
            for p0, n in [(7, 50), (HW - 33, 33)]:
                if p0 < 0 or p0 + n > HW:
                    continue
                part, pflag = _table(Pd, symd, td, C, K, rgb, c, p0, n)
                assert np.array_equal(part[..., :-1], full[:, p0:p0 + n, :-1]), (what, p0, n)
                sub = [v.reshape(B, K, HW)[:, :, p0:p0 + n].reshape(B, K, 1, n) for v in (pi, mu, ls)]
                ref64.check_entries(part.reshape(B, 1, n, Lp), *sub, t, what='{} rows [{}, {})'.format(what, p0, p0 + n))
                assert pflag == int(not ref64.rows_increasing(part).all()), (what, p0, n)
            # the oracle's table from the oracle's own parameters
            x = torch.from_numpy(ref64.values_of(sym, rgb))
            o = odmll.params_for_channel(_spec(rgb), torch.from_numpy(P), c, C, x)
            otab = ref64.as_u16(ocdf.mixture_cdf_table(o[0], torch.from_numpy(t), o[1], o[2])).reshape(B, HW, Lp)
            d = (full - otab) & 0xFFFF
            d = np.minimum(d, 65536 - d)
            print('{}: against the oracle end to end: max |difference| {}, differing {:.3%}'.format(what, int(d.max()), (d != 0).mean()))
            if c == 0:
                assert d.max() <= 1, (what, int(d.max()))
                if HW >= 240:
                    assert (d != 0).mean() < ref64.MISMATCH_CAP, (what, (d != 0).mean())
        pooled.assert_caps((regime, rgb, H, W))


@pytest.mark.parametrize('Lp,K', [(3, 2), (5, 4)])
def test_exact_ties_go_to_the_even_entry(Lp, K):
    """cdf_quantise rounds half to EVEN (rintf, as torch.round in the reference).  ref64.tie_case: rows whose scaled CDF is exactly
    k + 0.5 in fp32 and in fp64, for even and for odd k (tests/test_ref64.py asserts that of the inputs, and that the oracle's table is the
    fp64 one) -- every entry of the fused table, of the two-kernel table and of the encoder's intervals must EQUAL the fp64 entries; the
    near-tie excuse of check_entries does not apply to a tie that is exact."""
    from l3c_pytorch_amd import ops
    P, t, tied = ref64.tie_case(Lp, K)
    n = P.shape[3]
    Pd, td = _nhwc(P), _dev(t)
    pi, mu, ls = ops.dmll_channel_params(Pd, None, 1, K, False, 0)
    assert (pi.cpu().numpy() == 1.0 / K).all()
    want = ref64.entries64(ref64.cdf64(pi.cpu().numpy(), mu.cpu().numpy(), ls.cpu().numpy(), t), Lp)[0, 0]          # (n, Lp)
    fused, flag = _table(Pd, None, td, 1, K, False, 0, 0, n)
    assert np.array_equal(fused[0], want), (fused[0] - want)
    assert flag == int(not ref64.rows_increasing(want).all())
    two, _ = ops.cdf_table_mixture(td, pi, mu, ls)
    assert np.array_equal(ref64.as_u16(two)[0, 0], want)
    for s in range(Lp - 1):
        sym = torch.full((1, 1, 1, n), s, dtype=torch.int16, device='cuda')
        c_low, c_high = _unpack_intervals(ops.dmll_encode_intervals(Pd, sym, td, 1, K, False), 1, n)
        assert np.array_equal(c_low[0], want[:, s]), s
        assert np.array_equal(c_high[0], want[:, s + 1] if s < Lp - 2 else np.full(n, 65536)), s


# ---- 3. intervals -----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('regime,rgb', CASES)
def test_fused_intervals_vs_fp64_and_table(regime, rgb):
    """l3c_dmll_encode_intervals: c_low and c_high through the same rule at entries sym and sym + 1; c_high == 65536 exactly at the top
    symbol; bit-equal to the table of l3c_dmll_cdf_table; and where every row is strictly increasing the stream coded from them decodes
    losslessly through that table.  The two shares are taken over the whole case (four shapes, every channel)."""
    from l3c_pytorch_amd import ops
    t = ref64.targets32(rgb)
    Lp = t.shape[0]
    L = Lp - 1
    pooled = ref64.EntryStats()
    for (H, W) in ref64.SHAPES:
        P, sym, C, K, Pd, symd, td = _case(regime, rgb, H, W)
        HW = H * W
        assert (sym == 0).any() and (sym == L - 1).any()
        iv = ops.dmll_encode_intervals(Pd, symd, td, C, K, rgb)
        c_low, c_high = _unpack_intervals(iv, B * C, HW)
        c_low, c_high = c_low.reshape(B, C, HW), c_high.reshape(B, C, HW)
        tabs, monotone = [], True
        for c in range(C):
            what = '{} {} {}x{} c{} intervals'.format(_name(rgb), regime, H, W, c)
            pi, mu, ls = _params(Pd, symd, C, K, rgb, c)
            s = sym[:, c].astype(np.int64)
            top = (s == L - 1).reshape(B, HW)
            assert (c_high[:, c][top] == 65536).all() and (c_high[:, c][~top] < 65536).all(), what
            assert (c_low[:, c] >= 0).all() and (c_low[:, c] < 65536).all()
            idx = np.stack([s, s + 1], axis=-1)
            got = np.stack([c_low[:, c], c_high[:, c]], axis=-1).reshape(B, H, W, 2)
            # entry L is never read (the top symbol's c_high is 2^16): compare it with itself
            w_top = ref64.entries64(ref64.cdf64(pi, mu, ls, t), Lp)[..., L]
            got[..., 1] = np.where(top.reshape(B, H, W), w_top, got[..., 1])
            ref64.check_entries(got, pi, mu, ls, t, index=idx, what=what, stats=pooled)
            full, flag = _table(Pd, symd, td, C, K, rgb, c, 0, HW)
            monotone = monotone and flag == 0
            assert np.array_equal(c_low[:, c], np.take_along_axis(full, s.reshape(B, HW, 1), -1)[..., 0]), what
            hi = np.where(top, 65536, np.take_along_axis(full, np.minimum(s + 1, L).reshape(B, HW, 1), -1)[..., 0])
            assert np.array_equal(c_high[:, c], hi), what
            tabs.append(full)
        print('{} {} {}x{}: every row strictly increasing: {}'.format(_name(rgb), regime, H, W, monotone))
        if monotone:
            table_all = _dev(np.stack(tabs, axis=1).reshape(B * C * HW, Lp).astype(np.uint16).view(np.int16))
            out, n = ops.ac_encode(iv, B * C, HW)
            n, out = n.cpu().numpy(), out.cpu().numpy()
            buf, offs, lens = ops.pack_streams([out[i, :n[i]].tobytes() for i in range(B * C)])
            dec = ops.ac_decode(table_all, buf, offs, lens, B * C, HW, True).reshape(B, C, H, W)
            assert torch.equal(dec, symd), (regime, rgb, H, W)
    print('{} {} intervals pooled: {}'.format(_name(rgb), regime, pooled))
    pooled.assert_caps((regime, rgb))


# ---- 4. window rows ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('regime', ref64.regimes(True))
def test_window_rows_are_slices_of_the_full_rows(regime):
    """RGB, window_stats zeros (every image on window rows): entries 0 .. 63 are the slice [w0, w0 + 64) of the full row, entry 64 is w0, the
    window sits around the mixture's mean; `offrange` pins w0 to 0 or 192."""
    for (H, W) in ref64.SHAPES:
        P, sym, C, K, Pd, symd, td = _case(regime, True, H, W)
        HW = H * W
        stats = torch.zeros(B, dtype=torch.int32, device='cuda')
        for c in range(C):
            full, flag = _table(Pd, symd, td, C, K, True, c, 0, HW)
            mixed, wflag = _table(Pd, symd, td, C, K, True, c, 0, HW, window_stats=stats)
            pi, mu, _ = _params(Pd, symd, C, K, True, c)
            mean = (pi.astype(np.float64) * mu).sum(axis=1).reshape(B, HW)
            want_w0 = np.clip(np.floor(np.clip(mean, 0, 255)) - 31, 0, 192)
            wins = mixed.reshape(B, -1)[:, :HW * 65].reshape(B, HW, 65)
            assert wflag == int(not (np.diff(wins[..., :64], axis=-1) > 0).all())
            for b in range(B):
                win = wins[b]
                w0 = win[:, 64]
                assert w0.min() >= 0 and w0.max() <= 192
                assert np.abs(w0 - want_w0[b]).max() <= 1, (regime, H, W, c)         # (the kernel sums pi_k mu_k sequentially in fp32)
                if regime == 'offrange':
                    assert np.isin(w0, (0, 192)).all()
                assert np.array_equal(win[:, :64], np.take_along_axis(full[b], w0[:, None] + np.arange(64)[None, :], -1)), (regime, H, W, c, b)
            if flag == 0:
                assert wflag == 0


# ---- 5. negative log-likelihood ---------------------------------------------------------------------------------------------------


def _nll_case(regime, rgb, far_every):
    """-> (elements, elements whose slack term exceeds 1e-3, elements at the mass clamp)."""
    from l3c_pytorch_amd import ops
    x_min, x_max, L = ref64.alphabet(rgb)
    n = big = hit = 0
    for (H, W) in ref64.SHAPES:
        P, sym, C, K, Pd, _, _ = _case(regime, rgb, H, W, far_every=far_every)
        x = ref64.values_of(sym, rgb)
        got = ops.dmll_nll(Pd, _dev(x), C, K, rgb, x_min, x_max, L).cpu().numpy()
        ref32 = odmll.nll(_spec(rgb), torch.from_numpy(x), torch.from_numpy(P)).numpy()
        r64, clamped = ref64.nll64(P, x, rgb, C, K, return_clamped=True)
        tol, share = ref64.nll_tolerance(ref32, r64)
        err = np.abs(got.astype(np.float64) - ref32)
        print('{} {} {}x{}: max |nll - oracle| = {:.3g}, max error / tolerance = {:.3f}, slack term above 1e-3 on {:.3%}, at the clamp {}'.format(
            _name(rgb), regime, H, W, err.max(), (err / tol).max(), share, int(clamped.sum())))
        assert np.isfinite(got).all()
        assert (err <= tol).all(), (regime, rgb, H, W, (err / tol).max())
        if clamped.any():
            assert np.abs(got[clamped] + np.log(1e-12)).max() < 1e-4
        n, big, hit = n + got.size, big + share * got.size, hit + int(clamped.sum())
    assert big < ref64.NLL_SLACK_SHARE * n, (regime, rgb, big / n)
    return n, big, hit


@pytest.mark.parametrize('regime,rgb', CASES)
def test_nll_vs_oracle_with_the_references_own_conditioning(regime, rgb):
    """l3c_dmll_nll against the oracle's fp32 NLL, per element within 2e-5 + 2e-5 |ref| + 4 |oracle fp32 - fp64| (the project's tolerance plus
    the reference's own fp32 conditioning); the last term exceeds 1e-3 on < 2 % of the case (tests/test_ref64.py shows it with the oracle
    alone).  Symbols where the mixture has its mass, every 16th pixel anywhere, 0 and L-1 included (the two edge branches)."""
    _nll_case(regime, rgb, 16)


@pytest.mark.parametrize('rgb', [True, False])
def test_nll_hits_the_mass_clamp_in_sharp(rgb):
    """`sharp` with uniformly random symbols: x far from every mean, every component at the 1e-12 clamp: -log(1e-12) = 27.631 nats."""
    n, _, hit = _nll_case('sharp', rgb, 1)
    assert hit > 0.25 * n, (hit, n)


# ---- 6. misaligned P --------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('regime,rgb', [('benign', True), ('sharp', True), ('lambda', True), ('benign', False)])
def test_misaligned_P_gives_the_same_bits(regime, rgb):
    """fill_tile's 16-byte path needs Kp % 4 == 0 and an aligned source; the same P 4 bytes off a 16-byte boundary takes the scalar path (on
    the RGB scale's Kp = 120 no other input reaches it): table, window rows and intervals bit-equal to the aligned run."""
    from l3c_pytorch_amd import ops
    for (H, W) in ref64.SHAPES:
        P, sym, C, K, Pd, symd, td = _case(regime, rgb, H, W)
        HW = H * W
        Pm = _misaligned(Pd)
        assert Pd.data_ptr() % 16 == 0 and torch.equal(Pm, Pd)
        assert torch.equal(ops.dmll_encode_intervals(Pm, symd, td, C, K, rgb), ops.dmll_encode_intervals(Pd, symd, td, C, K, rgb))
        stats = torch.zeros(B, dtype=torch.int32, device='cuda')
        for c in range(C):
            for p0, n in [(0, HW), (7, 50)]:
                if p0 + n > HW:
                    continue
                a, fa = _table(Pd, symd, td, C, K, rgb, c, p0, n)
                m, fm = _table(Pm, symd, td, C, K, rgb, c, p0, n)
                assert np.array_equal(a[..., :-1], m[..., :-1]) and fa == fm, (regime, rgb, H, W, c, p0)
                if rgb:
                    a, fa = _table(Pd, symd, td, C, K, rgb, c, p0, n, window_stats=stats)
                    m, fm = _table(Pm, symd, td, C, K, rgb, c, p0, n, window_stats=stats)
                    assert np.array_equal(a.reshape(B, -1)[:, :n * 65], m.reshape(B, -1)[:, :n * 65]) and fa == fm


# ---- 7. the monotonicity flag -----------------------------------------------------------------------------------------------------

SWAPS = {True: (0, 1, 2, 62, 63, 64, 126, 127, 128, 191, 254, 255), False: (0, 1, 12, 23, 24)}


def _swapped(t, l):
    t = t.copy()
    t[l], t[l + 1] = t[l + 1], t[l]
    return t


@pytest.mark.parametrize('npix', ref64.MONO_NPIX)
@pytest.mark.parametrize('rgb', [True, False])
def test_monotonicity_flag_sees_a_swapped_pair_of_bin_edges(rgb, npix):
    """The in-register check of cdf_table_from_P_kernel (in-thread pair, next-lane pair, the hand-over between 128-entry runs) shown rows
    that violate it: the `wide` mixture (every bin holds > 8 counts, tests/test_ref64.py) evaluated at bin edges with entries l and l + 1
    swapped (`targets` is a caller-supplied array).  The flag must equal a numpy check of the produced rows over [0, Lp-2] and
    l3c_cdf_check_monotone on the same table; l = Lp - 2 swaps only the never-read last entry and must leave it 0.  Nothing is decoded."""
    from l3c_pytorch_amd import ops
    t = ref64.targets32(rgb)
    Lp = t.shape[0]
    P, sym, C, K, Pd, symd, _ = _case('wide', rgb, 1, npix)
    for c in range(C):
        for l in SWAPS[rgb] + (None,):
            ts = t if l is None else _swapped(t, l)
            flag = torch.zeros(1, dtype=torch.int32, device='cuda')
            tab = ops.dmll_cdf_table(Pd, symd if rgb else None, _dev(ts), C, K, rgb, c, 0, npix, flag)
            rows = ref64.as_u16(tab)
            bad = ~(np.diff(rows[..., :-1], axis=-1) > 0)
            want = int(bad.any())
            assert want == int(l is not None and l <= Lp - 3), (rgb, npix, c, l)              # the inputs do what they are built for
            if want:
                assert (np.nonzero(bad)[-1] == l).all()                                        # and only at the swapped pair
            assert int(flag.item()) == want, (rgb, npix, c, l, int(flag.item()))
            assert ops.table_is_monotone(tab.reshape(-1, Lp)) == (not want), (rgb, npix, c, l)


@pytest.mark.parametrize('rgb,npix,rows', [(True, 45, (0, 1, 2, 31, 33, 44)), (True, 32, (1, 31)), (False, 45, (0, 3, 4, 5, 44)), (False, 5, (4,))])
def test_monotonicity_flag_one_violating_row_among_saturated_rows(rgb, npix, rows):
    """As above with ONE `wide` row among `offrange` rows at the log_sigma clamp (saturated: their entries are a constant + l whatever the bin edges, so a swap
    cannot disturb them): the pair (l, l + 1) of row p sits at entry p * Lp + l of the block -- an even entry is checked inside a thread,
    an odd one against the next lane, entry 127 mod 128 through the hand-over between runs -- so a guard that is wrong in one of the three
    places cannot hide behind a row that another place catches.  (RGB row 1, l = 254: entry 511, the hand-over at its l <= Lp - 3 limit.)"""
    from l3c_pytorch_amd import ops
    t = ref64.targets32(rgb)
    Lp = t.shape[0]
    Pw, sym, C, K = ref64.head_case('wide', rgb, 1, npix)
    Po = ref64.head_case('offrange', rgb, 1, npix)[0]
    Po.reshape(B, -1, C, K, 1, npix)[:, 2] = -9.0      # at the clamp: sigma = e^-7, every edge is thousands of sigma from every mean
    symd = _dev(sym)
    for p in rows:
        P = Po.copy()
        P[:, :, :, p] = Pw[:, :, :, p]
        Pd = _nhwc(P)
        for c in range(C):
            for l in SWAPS[rgb]:
                flag = torch.zeros(1, dtype=torch.int32, device='cuda')
                tab = ops.dmll_cdf_table(Pd, symd if rgb else None, _dev(_swapped(t, l)), C, K, rgb, c, 0, npix, flag)
                bad = ~(np.diff(ref64.as_u16(tab)[..., :-1], axis=-1) > 0)
                want = int(l <= Lp - 3)
                assert int(bad.any()) == want and bad.sum() == want * B, (rgb, npix, p, c, l)
                if want:
                    assert (np.nonzero(bad)[1] == p).all() and (np.nonzero(bad)[2] == l).all()
                assert int(flag.item()) == want, (rgb, npix, p, c, l, int(flag.item()))
                assert ops.table_is_monotone(tab.reshape(-1, Lp)) == (not want)


@pytest.mark.parametrize('npix', ref64.MONO_NPIX)
def test_monotonicity_flag_of_window_rows(npix):
    """The window-row variant (8 lanes per pixel, 8 entries per lane): the flag against a numpy check of the 64 entries of every window,
    with the swapped pair inside some windows and outside others."""
    from l3c_pytorch_amd import ops
    t = ref64.targets32(True)
    P, sym, C, K, Pd, symd, _ = _case('wide', True, 1, npix)
    stats = torch.zeros(B, dtype=torch.int32, device='cuda')
    seen = set()
    for c in range(C):
        for l in SWAPS[True] + (None,):
            ts = t if l is None else _swapped(t, l)
            flag = torch.zeros(1, dtype=torch.int32, device='cuda')
            tab = ops.dmll_cdf_table(Pd, symd, _dev(ts), C, K, True, c, 0, npix, flag, window_stats=stats)
            win = ref64.as_u16(tab).reshape(B, -1)[:, :npix * 65].reshape(B, npix, 65)
            w0 = win[..., 64]
            bad = ~(np.diff(win[..., :64], axis=-1) > 0)
            if l is not None:
                inside = (w0 <= l) & (l + 1 <= w0 + 63)                  # both entries of the pair are in the window
                assert np.array_equal(bad.any(axis=-1), inside), (npix, c, l)
                seen.update(inside.reshape(-1).tolist())
            else:
                assert not bad.any()
            assert int(flag.item()) == int(bad.any()), (npix, c, l, int(flag.item()))
    if npix >= 5:
        assert seen == {True, False}


# ---- 8. sample --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('rgb', [True, False])
@pytest.mark.parametrize('HW', [1, 63, 65])
def test_sample_kernel_at_ragged_tiles(rgb, HW):
    """l3c_dmll_sample at HW 1, 63 and 65 (one pixel, a tile minus one, a tile plus one) with the tolerance rule of
    tests/test_gpu_head.py: within 2e-3 wherever both picked the same component; a Gumbel-max flip tolerated on < 0.1 % -- which at
    these sizes (at most 2 * 5 * 65 values) means on none."""
    from l3c_pytorch_amd import ops
    P, _, C, K = ref64.head_case('benign', rgb, 1, HW)
    rng = np.random.RandomState(HW)
    u_mix = rng.uniform(1e-5, 1 - 1e-5, size=(B, C, K, 1, HW)).astype(np.float32)
    u_log = rng.uniform(1e-5, 1 - 1e-5, size=(B, C, 1, HW)).astype(np.float32)
    got = ops.dmll_sample(_nhwc(P), _dev(u_mix), _dev(u_log), C, K, rgb).cpu()
    want = odmll.sample(_spec(rgb), torch.from_numpy(P), C, torch.from_numpy(u_mix), torch.from_numpy(u_log))
    assert got.shape == want.shape == (B, C, 1, HW)
    bad = ((got - want).abs() > 2e-3).float().mean().item()
    assert bad < 1e-3, bad
    if rgb:
        assert got.min() >= 0 and got.max() <= 255


# ---- 9. the network fixtures ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('name', ['net_32.npz', 'net_cal_32.npz', 'net_cal_64x96.npz'])
def test_fixture_P_parameters_and_table_vs_fp64(golden, name):
    """Steps 1 and 2 on the P tensors of the committed network fixtures (the reference's own network outputs): P0 with the image as
    symbols where the fixture's P0 covers the whole image, P1 with the symbols of bn1."""
    g = golden(name)
    cases = []
    if g['P0'].shape[2:] == g['img'].shape[2:]:
        cases.append((True, g['P0'], g['img'].astype(np.int16)))
    bw = np.float32(2 / 24)
    cases.append((False, g['P1'], np.rint((g['bn1'] + 1) / bw).astype(np.int16)))
    for rgb, P, sym in cases:
        P = np.ascontiguousarray(P, dtype=np.float32)
        Bf, _, H, W = P.shape
        C, K = (3, 10) if rgb else (5, 10)
        t = ref64.targets32(rgb)
        Lp = t.shape[0]
        Pd, symd, td = _nhwc(P), _dev(sym), _dev(t)
        x = ref64.values_of(sym, rgb)
        for c in range(C):
            what = '{} {} c{}'.format(name, _name(rgb), c)
            pi, mu, ls = _params(Pd, symd, C, K, rgb, c)
            pi64, mu64, ls64 = ref64.params64(P, x, rgb, C, K, c)
            assert (ls.astype(np.float64) == ls64).all(), what
            assert np.abs(pi - pi64).max() <= ref64.PI_BOUND, what
            assert (np.abs(mu - mu64) <= ref64.mu_bound64(P, x, rgb, C, K, c)).all(), what
            full, flag = _table(Pd, symd, td, C, K, rgb, c, 0, H * W)
            ref64.check_entries(full.reshape(Bf, H, W, Lp), pi, mu, ls, t, what=what).assert_caps(what)
            assert flag == int(not ref64.rows_increasing(full).all())
