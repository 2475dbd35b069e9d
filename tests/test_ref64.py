"""CPU: the ORACLE through the rules of tests/ref64.py, on the inputs the -m gpu files feed the HIP kernels (tests/test_gpu_head_regimes.py).
This is the proof that those inputs keep the reference itself inside the caps -- a kernel that misses a rule there misses something a
correct fp32 implementation meets."""
import numpy as np
import pytest
import torch

from oracle import cdf as ocdf, dmll as odmll
from tests import ref64

ALPHABETS = [pytest.param(True, id='rgb'), pytest.param(False, id='z')]
CASES = [pytest.param(regime, rgb, id='{}-{}'.format(regime, 'rgb' if rgb else 'z'))
         for rgb in (True, False) for regime in ref64.regimes(rgb)]


def _spec(rgb):
    return odmll.RGB if rgb else odmll.z_spec()


def _oracle_params(P, sym, rgb, C, c):
    x = torch.from_numpy(ref64.values_of(sym, rgb))
    return [v.numpy() for v in odmll.params_for_channel(_spec(rgb), torch.from_numpy(P), c, C, x)]


@pytest.mark.parametrize('regime,rgb', CASES)
def test_oracle_parameters_and_table_meet_the_fp64_rule(regime, rgb):
    """Stage (a): the oracle's fp32 parameters against fp64 from P; stage (b): its uint16 table against fp64 on its own parameters.
    The two shares per channel at 12x20, pooled over the channels at the small shapes."""
    t = ref64.targets32(rgb)
    for (H, W) in ref64.SHAPES:
        P, sym, C, K = ref64.head_case(regime, rgb, H, W)
        x = ref64.values_of(sym, rgb)
        pooled = ref64.EntryStats()
        for c in range(C):
            pi, mu, ls = _oracle_params(P, sym, rgb, C, c)
            pi64, mu64, ls64 = ref64.params64(P, x, rgb, C, K, c)
            assert (ls.astype(np.float64) == ls64).all()
            assert (np.abs(pi - pi64) <= ref64.PI_BOUND).all(), np.abs(pi - pi64).max() / ref64.U32
            assert (np.abs(mu - mu64) <= ref64.mu_bound64(P, x, rgb, C, K, c)).all()
            table = ocdf.mixture_cdf_table(*(torch.from_numpy(v) for v in (pi, t, mu, ls))).numpy()
            what = '{} {} {}x{} c{}'.format('rgb' if rgb else 'z', regime, H, W, c)
            s = ref64.check_entries(table, pi, mu, ls, t, what=what, stats=pooled)
            inc64 = ref64.rows_increasing(ref64.entries64(ref64.cdf64(pi, mu, ls, t), t.shape[0]))
            print('   rows strictly increasing in fp64: {:.1%}'.format(inc64.mean()))
            assert ref64.rows_increasing(ref64.as_u16(table))[inc64].all(), what
            if H * W >= 240:
                s.assert_caps(what)
        pooled.assert_caps((regime, rgb, H, W))


@pytest.mark.parametrize('rgb', ALPHABETS)
def test_wide_gives_every_bin_eight_counts(rgb):
    """The monotonicity tests swap two adjacent bin edges of a `wide` row and expect exactly that pair of entries to come out
    non-increasing: every bin must hold well over one count of mass.  Asserted: at least 8 / 65280 in fp64, every bin of every row."""
    t = ref64.targets32(rgb)
    for (H, W) in ref64.SHAPES + tuple((1, n) for n in ref64.MONO_NPIX):
        P, sym, C, K = ref64.head_case('wide', rgb, H, W)
        for c in range(C):
            pi, mu, ls = _oracle_params(P, sym, rgb, C, c)
            mass = ref64.bin_mass64(pi, mu, ls, t).min()
            assert mass >= 8 / 65280, (H, W, c, mass * 65280)


@pytest.mark.parametrize('rgb', ALPHABETS)
def test_offrange_saturates_and_wraps(rgb):
    """Means below the range: the CDF is 1 at the last edge, entry Lp-1 = 65536 - (Lp-1) + (Lp-1) wraps to 0; above: the CDF is 0 and the
    entries are 0 .. Lp-1.  Both kinds of row occur, in every channel, and entries 0 .. Lp-2 stay strictly increasing.  On the RGB scale
    (1.2 spans are 41 of the widest sigma) both kinds are saturated at every edge; on the bottleneck scales (5 to 6 sigma) only nearly."""
    t = ref64.targets32(rgb)
    Lp = t.shape[0]
    P, sym, C, K = ref64.head_case('offrange', rgb, 12, 20)
    for c in range(C):
        e = ref64.entries64(ref64.cdf64(*_oracle_params(P, sym, rgb, C, c), t), Lp)
        wrapped = e[..., Lp - 1] == 0
        assert 0.2 < wrapped.mean() < 0.8, wrapped.mean()
        if rgb:
            assert (e[wrapped] == (65536 - (Lp - 1) + np.arange(Lp)) % 65536).all()
            assert (e[~wrapped] == np.arange(Lp)).all()
        assert ref64.rows_increasing(e).all()


@pytest.mark.parametrize('regime,rgb', CASES)
def test_oracle_nll_meets_its_own_tolerance_rule(regime, rgb):
    """tests/test_gpu_head_regimes.py compares the NLL kernel with the oracle's fp32 NLL within 2e-5 + 2e-5 |ref| + 4 |oracle fp32 - fp64|.
    The last term is the reference's own conditioning (1 - sigmoid differences in the upper tail of a component lose all relative
    precision in fp32); it must stay the exception: above 1e-3 on less than 2 % of the elements of the case (the four shapes pooled).
    The symbols sit where the mixture has its mass, every 16th pixel anywhere."""
    n = big = 0
    for (H, W) in ref64.SHAPES:
        P, sym, C, K = ref64.head_case(regime, rgb, H, W)
        x = ref64.values_of(sym, rgb)
        ref32 = odmll.nll(_spec(rgb), torch.from_numpy(x), torch.from_numpy(P)).numpy()
        tol, share = ref64.nll_tolerance(ref32, ref64.nll64(P, x, rgb, C, K))
        n, big = n + ref32.size, big + share * ref32.size
        assert np.isfinite(ref32).all()
    print('{} {}: slack term above 1e-3 on {:.3%} of {} elements'.format('rgb' if rgb else 'z', regime, big / n, n))
    assert big < ref64.NLL_SLACK_SHARE * n, big / n


@pytest.mark.parametrize('rgb', ALPHABETS)
def test_sharp_with_far_symbols_hits_the_mass_clamp(rgb):
    """`sharp` with uniformly random symbols: most elements have every component at the 1e-12 clamp of the bin's mass (NLL = -log 1e-12 =
    27.6 nats), in fp64 and in the oracle alike, and the tolerance rule still holds."""
    n = big = hit = 0
    for (H, W) in ref64.SHAPES:
        P, sym, C, K = ref64.head_case('sharp', rgb, H, W, far_every=1)
        x = ref64.values_of(sym, rgb)
        ref32 = odmll.nll(_spec(rgb), torch.from_numpy(x), torch.from_numpy(P)).numpy()
        r64, clamped = ref64.nll64(P, x, rgb, C, K, return_clamped=True)
        tol, share = ref64.nll_tolerance(ref32, r64)
        assert (np.abs(ref32 - r64) <= tol).all()
        assert np.allclose(ref32[clamped], -np.log(1e-12), atol=1e-4)
        n, big, hit = n + ref32.size, big + share * ref32.size, hit + int(clamped.sum())
    assert hit > 0.25 * n, (hit, n)
    assert big < ref64.NLL_SLACK_SHARE * n, big / n


@pytest.mark.parametrize('Lp,K', [(3, 2), (5, 4)])
def test_exact_ties_go_to_the_even_entry_in_the_oracle(Lp, K):
    """ref64.tie_case: the scaled CDF is exactly k + 0.5, for even and for odd k; the reference rounds half to even (torch.round), and so
    does the fp64 statement -- entry for entry the same table."""
    P, t, tied = ref64.tie_case(Lp, K)
    pi, mu, ls = [v.numpy() for v in odmll.params_for_channel(odmll.Spec(False, -1, 1, Lp - 1), torch.from_numpy(P), 0, 1)]
    scaled = ref64.cdf64(pi, mu, ls, t)[0, 0] * (65536 - (Lp - 1))
    at_tie = np.take_along_axis(scaled, tied[:, None], -1)[:, 0]
    assert (at_tie - np.floor(at_tie) == 0.5).all()
    assert (np.floor(at_tie) % 2 == 0).any() and (np.floor(at_tie) % 2 == 1).any()
    want = ref64.entries64(ref64.cdf64(pi, mu, ls, t), Lp)
    assert ((np.take_along_axis(want[0, 0], tied[:, None], -1)[:, 0] - tied) % 2 == 0).all()
    table = ocdf.mixture_cdf_table(*(torch.from_numpy(v) for v in (pi, t, mu, ls)))
    assert np.array_equal(ref64.as_u16(table), want)


# ---- the heads of tests/test_gpu_head_shapes.py: every (C, K, alphabet) of ref64.HEAD_SHAPES ---------------------------------------

SHAPE_W = 165          # B = 3, H = 1: the size at which the -m gpu file checks every shape against fp64
SHAPE_CASES = [pytest.param(C, K, rgb, alpha, regime, id='{}-{}'.format(ref64.shape_id(C, K, rgb, alpha), regime))
               for (C, K, rgb, alpha) in ref64.HEAD_SHAPES for regime in ref64.shape_regimes(rgb)]


def test_shape_builders_leave_the_shipped_cases_alone():
    """head_case draws what it drew before the alphabet was threaded through (make_P with and without `alpha` on the shipped alphabets), and
    the shape table is the one the kernels' forms were chosen for: Kp of every row."""
    for rgb in (True, False):
        for regime in ref64.shape_regimes(rgb):
            P, sym, C, K = ref64.head_case(regime, rgb, 5, 13)
            rng = np.random.RandomState(10000 * ref64.REGIMES.index(regime) + 100 * 5 + 13 + (5000 if rgb else 0))
            P2 = ref64.make_P(regime, rgb, 2, 5, 13, C, K, rng, alpha=ref64.alphabet(rgb))
            assert P.tobytes() == P2.tobytes()
            assert np.array_equal(sym, ref64.near_sym(P2, rgb, C, K, rng, alpha=ref64.alphabet(rgb)))
        assert np.array_equal(ref64.targets32(rgb), ref64.targets_of(ref64.alphabet(rgb)))
    assert [(4 if rgb else 3) * C * K for C, K, rgb, _ in ref64.HEAD_SHAPES] == [12, 60, 192, 3, 6, 18, 42, 45, 60, 240, 126, 240, 255]
    assert [a[2] + 1 for _, _, _, a in ref64.HEAD_SHAPES] == [257, 257, 257, 3, 26, 8, 65, 26, 26, 260, 26, 26, 26]


@pytest.mark.parametrize('C,K,rgb,alpha,regime', SHAPE_CASES)
def test_oracle_meets_the_rules_at_every_head_shape(C, K, rgb, alpha, regime):
    """The oracle on the inputs of tests/test_gpu_head_shapes.py, through the rules that file applies to the kernels: parameters within
    PI_BOUND / mu_bound64 / the exact clamp; its table through check_entries on its own parameters, the two shares pooled over the channels
    of the case and inside the caps; rows that increase in fp64 increase; the NLL inside nll_tolerance with the slack term above 1e-3 on
    < 2 %; both edge symbols occur."""
    spec = odmll.Spec(rgb, alpha[0], alpha[1], alpha[2])
    t = ref64.targets_of(alpha)
    Lp = t.shape[0]
    P, sym = ref64.shape_case(C, K, rgb, alpha, regime, 1, SHAPE_W)
    assert P.shape == (3, (4 if rgb else 3) * C * K, 1, SHAPE_W) and sym.min() == 0 and sym.max() == alpha[2] - 1
    x = ref64.values_at(sym, alpha)
    assert np.array_equal(x, spec.to_bn(torch.from_numpy(sym)).numpy())
    pooled, intervals = ref64.EntryStats(), ref64.EntryStats()
    worst_pi = worst_mu = 0.0
    for c in range(C):
        pi, mu, ls = [v.numpy() for v in odmll.params_for_channel(spec, torch.from_numpy(P), c, C, torch.from_numpy(x))]
        pi64, mu64, ls64 = ref64.params64(P, x, rgb, C, K, c)
        assert (ls.astype(np.float64) == ls64).all()
        worst_pi = max(worst_pi, np.abs(pi - pi64).max() / ref64.PI_BOUND)
        worst_mu = max(worst_mu, (np.abs(mu - mu64) / np.maximum(ref64.mu_bound64(P, x, rgb, C, K, c), 1e-300)).max())
        table = ocdf.mixture_cdf_table(*(torch.from_numpy(v) for v in (pi, t, mu, ls))).numpy()
        what = '{} {} c{}'.format(ref64.shape_id(C, K, rgb, alpha), regime, c)
        ref64.check_entries(table, pi, mu, ls, t, what=what, stats=pooled)
        inc64 = ref64.rows_increasing(ref64.entries64(ref64.cdf64(pi, mu, ls, t), Lp))
        assert ref64.rows_increasing(ref64.as_u16(table))[inc64].all(), what
        # the two entries per symbol an encoder reads: where the mixture has its mass, few of them saturated
        idx = np.stack([sym[:, c], sym[:, c] + 1], axis=-1).astype(np.int64)
        ref64.check_entries(np.take_along_axis(ref64.as_u16(table), idx, -1), pi, mu, ls, t, index=idx, what=what + ' intervals', stats=intervals)
    print('   |pi - pi64| / PI_BOUND <= {:.3f}, |mu - mu64| / bound <= {:.3f}; table: {}; intervals: {}'.format(worst_pi, worst_mu, pooled, intervals))
    assert worst_pi <= 1 and worst_mu <= 1, (worst_pi, worst_mu)
    pooled.assert_caps((C, K, rgb, alpha, regime, 'table'))
    intervals.assert_caps((C, K, rgb, alpha, regime, 'intervals'))
    ref32 = odmll.nll(spec, torch.from_numpy(x), torch.from_numpy(P)).numpy()
    tol, share = ref64.nll_tolerance(ref32, ref64.nll64(P, x, rgb, C, K, alpha=alpha))
    print('   nll: slack term above 1e-3 on {:.3%} of {} elements'.format(share, ref32.size))
    assert np.isfinite(ref32).all() and share < ref64.NLL_SLACK_SHARE, share


def _mean32(spec, P, C):
    """The mixture's mean as symbols in fp32 torch, channel by channel on its own estimates (what l3c_dmll_mean computes)."""
    Pt = torch.from_numpy(P)
    B, _, H, W = P.shape
    sym = torch.zeros(B, C, H, W, dtype=torch.long)
    for c in range(C):
        pi, mu, _ = odmll.params_for_channel(spec, Pt, c, C, spec.to_bn(sym))
        sym[:, c] = spec.to_sym((pi * mu).sum(dim=1))
    return sym.numpy()


@pytest.mark.parametrize('C,K,rgb,alpha', [pytest.param(*s, id=ref64.shape_id(*s)) for s in ref64.HEAD_SHAPES])
def test_fp32_mean_meets_the_excuse_rule_at_every_head_shape(C, K, rgb, alpha):
    """ref64.mean_rule64 on a plain fp32 statement of the estimator: no symbol differs from fp64's outside the excused pixels, and those
    stay below 2 % of the shape's (pixel, channel) items (regimes pooled)."""
    spec = odmll.Spec(rgb, alpha[0], alpha[1], alpha[2])
    n = n_excused = 0
    for regime in ref64.mean_regimes(rgb, K):
        P, _ = ref64.shape_case(C, K, rgb, alpha, regime, 1, SHAPE_W)
        got = _mean32(spec, P, C)
        for c in range(C):
            want, excused = ref64.mean_rule64(P, got, rgb, C, K, alpha, c)
            assert not ((got[:, c] != want) & ~excused).any(), (regime, c)
            n, n_excused = n + excused.size, n_excused + int(excused.sum())
    print('   mean: excused {:.3%} of {}'.format(n_excused / n, n))
    assert n_excused <= ref64.MEAN_EXCUSED_CAP * n, (n_excused, n)


def test_quantise_argmin_is_the_oracles_quantiser():
    from oracle import net as onet
    rng = np.random.RandomState(0)
    for L in (2, 25, 256):
        levels = np.linspace(-1, 1, L).astype(np.float32)
        x = rng.uniform(-1.3, 1.3, size=(2, 3, 5, 7)).astype(np.float32)
        x[0, 0, 0, :L - 1][:7] = ((levels[:-1] + levels[1:]) / 2)[:7]          # ties between adjacent levels
        sym, q = ref64.quantise_argmin(x, levels)
        q_ref, sym_ref = onet.quantise(torch.from_numpy(x), torch.from_numpy(levels))
        assert (sym == sym_ref.numpy()).all() and (q == q_ref.numpy()).all()


def test_conv_references_against_torch_double():
    import torch.nn.functional as F
    rng = np.random.RandomState(1)
    img = rng.randint(0, 256, size=(2, 3, 9, 11)).astype(np.float32)
    w1, b1, w2, b2 = rng.randn(3, 3), rng.randn(3), rng.randn(3, 3) / 100, rng.randn(3)
    w3, b3 = rng.randn(16, 3, 3, 3), rng.randn(16)
    d = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))   # noqa: E731
    z = F.conv2d(F.conv2d(d(img), d(w1).reshape(3, 3, 1, 1), d(b1)), d(w2).reshape(3, 3, 1, 1), d(b2))
    out = F.conv2d(z, d(w3), d(b3), padding=1)
    z64, ez, out64, eo = ref64.rgb_head64(img, w1, b1, w2, b2, w3, b3)
    assert np.allclose(z64, z.numpy(), rtol=1e-12, atol=1e-12) and np.allclose(out64, out.numpy(), rtol=1e-12, atol=1e-10)
    assert (ez > 0).all() and (eo > 0).all()
    x, w, b = rng.randn(2, 5, 4, 6), rng.randn(16, 5), rng.randn(16)
    val, bound = ref64.conv1x1_64(x, w, b)
    assert np.allclose(val, F.conv2d(d(x), d(w).reshape(16, 5, 1, 1), d(b)).numpy(), rtol=1e-12, atol=1e-12)
    fuse = rng.randn(2, 16, 4, 6)
    val2, bound2 = ref64.dec_head64(x, w, b, fuse)
    assert np.allclose(val2, val + fuse) and (bound2 > 0).all() and (bound > 0).all()
