"""Plain fp64 references (numpy) of the logistic-mixture head and of the thin conv kernels, and the value regimes they are
checked in.  No GPU, no fixtures: tests/test_ref64.py runs the oracle through the same rules on the CPU, the -m gpu files
(tests/test_gpu_head_regimes.py, tests/test_gpu_small_kernels.py) run the HIP kernels through them.

Layout of P (N, Kp, H, W): channel = p * (C * K) + c * K + k, p in {0: logit, 1: mu, 2: log sigma, 3: lambda (RGB only)}.

WHY THE TABLE REFERENCE HAS TWO STAGES.  For G and B the coupled mean mu + sigmoid(lam) * x carries one fp32 ulp at ~300 (3e-5);
a component at log_sigma = -7 multiplies that by e^7, so two correct fp32 implementations that differ in the last bit of an expf
differ by tens of table counts (the oracle's own fp32 table is up to 30 counts from an fp64-from-P table in `sharp` and `peaked`).
So (a) the PARAMETERS are checked against fp64 from P (`params64`, `mu_bound64`), and (b) the TABLE against fp64 evaluated on the
implementation's own fp32 parameters (`cdf64`, `entries64`, `check_entries`).
"""
import numpy as np
import torch

from oracle import cdf as ocdf

LOG_SCALES_MIN = -7.0
U32 = 2.0 ** -24            # unit roundoff of fp32
REGIMES = ('benign', 'sharp', 'wide', 'offrange', 'peaked', 'flat', 'lambda')      # `lambda`: RGB only
LAMBDAS = (-90.0, -30.0, 0.0, 17.0, 30.0)
EXCUSED_CAP, MISMATCH_CAP = 0.15, 0.01


def alphabet(rgb):
    """-> (x_min, x_max, L) of the RGB scale / the bottleneck scales."""
    return (0.0, 255.0, 256) if rgb else (-1.0, 1.0, 25)


def regimes(rgb):
    return [r for r in REGIMES if rgb or r != 'lambda']


def targets_of(alpha):
    """The Lp fp32 bin edges the coder evaluates the CDF at (the oracle's), as numpy; alpha = (x_min, x_max, L)."""
    x_min, x_max, L = alpha
    return ocdf.coding_targets(x_min, x_max, L).numpy()


def values_at(sym, alpha):
    """Symbols -> the fp32 values the head is conditioned on / scores (Spec.to_bn: two rounded fp32 operations); alpha = (x_min, x_max, L)."""
    x_min, x_max, L = alpha
    bw = np.float32((x_max - x_min) / (L - 1))
    return (sym.astype(np.float32) * bw + np.float32(x_min)).astype(np.float32)


def targets32(rgb):
    """`targets_of` on the alphabet of the RGB scale / the bottleneck scales."""
    return targets_of(alphabet(rgb))


def values_of(sym, rgb):
    """`values_at` on the alphabet of the RGB scale / the bottleneck scales."""
    return values_at(sym, alphabet(rgb))


# ---- value regimes -----------------------------------------------------------------------------------------------------------


def make_P(regime, rgb, B, H, W, C, K, rng, alpha=None):
    """-> P (B, Kp, H, W) fp32.  alpha: (x_min, x_max, L) of a head that is not one of the two shipped ones (`benign`, `sharp`, `lambda` only):
    on a bottleneck-style head `benign` then draws mu from the range widened by a tenth of its span on either side and log_sigma from
    U(-9, -1 + log(bin width / (2 / 24))) -- sigma up to 4.4 bins, as on the shipped alphabet, where both are the figures below.
      benign    logits N(0,1); mu U(-20, 280) | U(-1.2, 1.2); log_sigma U(-9, 2) | U(-9, -1); lambda N(0,1)
      sharp     log_sigma U(-12, -6) (mostly at the -7 clamp); means on multiples of half a bin width: the bin edges themselves (the
                coder's fp32 targets: sigmoid(0) = .5 exactly) and the bin centres
      wide      log_sigma U(2, 8) | U(-1, 4).  RGB: a component at log_sigma = 8 puts at most 65280 / (4 e^8) = 5.5 counts into a bin, so
                component 0 is an anchor (mean U(0, 255) with lambda -30: no coupling; log_sigma U(4.5, 6.5): at least 23 counts per bin
                within 255 of its mean; logit 4: more than a third of the weight): every bin of every row then holds more than 8 counts
      offrange  per (pixel, channel) every mean 1.2 .. 12 spans below x_min or 1 .. 12 spans above x_max (G and B start 2 spans further
                below: the lambda coupling adds up to 2 spans): saturated rows, entry Lp-1 wraps to 0 on the `below` side
      peaked    logits * 40 (a one-hot softmax)
      flat      all K logits of a (pixel, channel) equal
      lambda    lambdas drawn from {-90, -30, 0, 17, 30} (sigmoid saturated to 0 and to 1)                               RGB only"""
    if regime not in regimes(rgb):
        raise ValueError('regime {!r} is not defined for rgb={}'.format(regime, rgb))
    if alpha is not None and tuple(alpha) != alphabet(rgb) and (rgb or regime not in ('benign', 'sharp')):
        raise ValueError('regime {!r} is not defined for the alphabet {} (rgb={})'.format(regime, alpha, rgb))
    x_min, x_max, L = alphabet(rgb) if alpha is None else alpha
    span = x_max - x_min
    shape = (B, C, K, H, W)
    logit = rng.randn(*shape)
    if rgb:
        mu = rng.uniform(-20, 280, size=shape)
        ls = rng.uniform(-9, 2, size=shape)
    elif (x_min, x_max, L) == alphabet(False):
        mu = rng.uniform(-1.2, 1.2, size=shape)
        ls = rng.uniform(-9, -1, size=shape)
    else:
        mu = rng.uniform(x_min - 0.1 * span, x_max + 0.1 * span, size=shape)
        ls = rng.uniform(-9, -1 + np.log(span / (L - 1) / (2 / 24)), size=shape)
    lam = rng.randn(*shape)
    if regime == 'sharp':
        ls = rng.uniform(-12, -6, size=shape)
        t = targets_of((x_min, x_max, L)).astype(np.float64)
        grid = np.sort(np.concatenate([t, x_min + np.arange(L) * (span / (L - 1))]))        # edges and centres
        mu = grid[rng.randint(0, grid.size, size=shape)]
    elif regime == 'wide':
        ls = rng.uniform(2, 8, size=shape) if rgb else rng.uniform(-1, 4, size=shape)
        if rgb:
            ls[:, :, 0] = rng.uniform(4.5, 6.5, size=ls[:, :, 0].shape)
            logit[:, :, 0] = 4.0
            mu[:, :, 0] = rng.uniform(0, 255, size=mu[:, :, 0].shape)
            lam[:, :, 0] = -30.0
    elif regime == 'offrange':
        below = rng.randint(0, 2, size=(B, C, 1, H, W)).astype(bool)
        extra = (np.arange(C) > 0).reshape(1, C, 1, 1, 1) * (2.0 if rgb else 0.0)
        lo = x_min - span * (1.2 + extra + rng.uniform(0, 1, size=shape) * (12 - 1.2 - extra))
        hi = x_max + span * rng.uniform(1, 12, size=shape)
        mu = np.where(below, lo, hi)
    elif regime == 'peaked':
        logit = logit * 40
    elif regime == 'flat':
        logit = np.broadcast_to(rng.randn(B, C, 1, H, W), shape)
    elif regime == 'lambda':
        lam = np.asarray(LAMBDAS)[rng.randint(0, len(LAMBDAS), size=shape)]
    parts = [logit, mu, ls] + ([lam] if rgb else [])
    return np.stack(parts, axis=1).reshape(B, len(parts) * C * K, H, W).astype(np.float32)


def make_sym(rgb, B, H, W, C, rng, alpha=None):
    """int16 symbols (B, C, H, W) with 0 and L-1 at some pixels of every channel (the first and the last pixel of image 0)."""
    L = (alphabet(rgb) if alpha is None else alpha)[2]
    sym = rng.randint(0, L, size=(B, C, H, W)).astype(np.int16)
    flat = sym.reshape(B, C, H * W)
    flat[0, :, 0] = L - 1
    flat[B - 1, :, H * W - 1] = 0
    return sym


def near_sym(P, rgb, C, K, rng, far_every=16, alpha=None):
    """Symbols where the mixture has its mass: channel by channel the value nearest to the (coupled, fp64) mean of a randomly picked
    component (picked with the mixture's own weights), clipped to the alphabet (`offrange`: the edge symbols).  Every `far_every`-th pixel keeps a uniformly random symbol (0:
    none); in every channel the first pixel of image 0 gets L-1 and the last pixel of the last image gets 0."""
    alpha = alphabet(rgb) if alpha is None else alpha
    x_min, x_max, L = alpha
    B, _, H, W = P.shape
    bw = (x_max - x_min) / (L - 1)
    sym = rng.randint(0, L, size=(B, C, H, W)).astype(np.int16)
    far = np.zeros(H * W, dtype=bool)
    if far_every:
        far[far_every - 1::far_every] = True
    far = far.reshape(1, H, W)
    for c in range(C):
        pi, mu, _ = params64(P, values_at(sym, alpha), rgb, C, K, c)
        k = (rng.uniform(size=(B, 1, H, W)) > np.cumsum(pi, axis=1)).sum(axis=1, keepdims=True).clip(0, K - 1)   # k ~ pi
        near = np.clip(np.rint((np.take_along_axis(mu, k, 1)[:, 0] - x_min) / bw), 0, L - 1).astype(np.int16)
        sym[:, c] = np.where(far, sym[:, c], near)
        flat = sym.reshape(B, C, H * W)
        flat[0, c, 0] = L - 1
        flat[B - 1, c, H * W - 1] = 0
    return sym


MONO_NPIX = (1, 5, 32, 45)                         # rows per launch of the monotonicity-flag tests (H = 1)
SHAPES = ((12, 20), (1, 1), (5, 13), (8, 8))      # HW % 32 and HW % 64 ragged, HW < 32


def head_case(regime, rgb, H, W, B=2, K=10, far_every=16):
    """The inputs of one (regime, alphabet, shape) case, the same on the CPU and on the GPU side: P (B, Kp, H, W) fp32, sym int16, C, K."""
    C = 3 if rgb else 5
    rng = np.random.RandomState(10000 * REGIMES.index(regime) + 100 * H + W + (5000 if rgb else 0))
    P = make_P(regime, rgb, B, H, W, C, K, rng)
    return P, near_sym(P, rgb, C, K, rng, far_every), C, K


# The heads of tests/test_gpu_head_shapes.py: (C, K, rgb, alphabet), each there for what its Kp = (4 | 3) C K and its C do in
# csrc/dmll_kernels.hip (the fill form of the P tile: Kp % 4 and q = Kp / 4 | Kp / 2; the threads per block: 320 iff C == 5; the turns of the
# compute loop: 64 C items; the kMaxK register arrays: K = 1 and K = 16; the LDS limit of the 64-pixel tile: 64 (Kp + 1) floats in 64 KiB, Kp <= 255).  The last row
# is the one tile that fills the limit to the byte.
HEAD_SHAPES = (
    (3, 1, True, (0.0, 255.0, 256)),      # Kp 12: K = 1; 16-byte fill at q = 3; window rows
    (3, 5, True, (0.0, 255.0, 256)),      # Kp 60: 16-byte fill at q = 15
    (3, 16, True, (0.0, 255.0, 256)),     # Kp 192: K = kMaxK with coupling; the largest RGB tile; the mean kernel's extra LDS
    (1, 1, False, (-1.0, 1.0, 2)),        # Kp 3: the smallest of everything; odd Kp
    (1, 2, False, (-1.0, 1.0, 25)),       # Kp 6: half fill at q = 3, nearly every piece straddles rows
    (3, 2, False, (-1.0, 1.0, 7)),        # Kp 18: half fill at q = 9
    (2, 7, False, (-2.0, 3.0, 64)),       # Kp 42: half fill at q = 21; an asymmetric range
    (5, 3, False, (-1.0, 1.0, 25)),       # Kp 45: 320 threads with the 4-byte fill
    (5, 4, False, (-1.0, 1.0, 25)),       # Kp 60: 320 threads on the run-time interval kernel, 16-byte fill
    (5, 16, False, (-1.0, 1.0, 259)),     # Kp 240: 320 threads; K = kMaxK; the largest tile of an even Kp; Lp = 260
    (7, 6, False, (-1.0, 1.0, 25)),       # Kp 126: half fill at q = 63; 448 items: 1.75 turns on 256 threads
    (8, 10, False, (-1.0, 1.0, 25)),      # Kp 240: 512 items: two full turns
    (17, 5, False, (-1.0, 1.0, 25)),      # Kp 255: the largest tile the limit admits, 65 536 bytes exactly; 1088 items: 4.25 turns
)
SHAPE_REGIMES = ('benign', 'sharp', 'lambda')      # `lambda`: the RGB shapes only


def shape_regimes(rgb):
    return [r for r in SHAPE_REGIMES if rgb or r != 'lambda']


def mean_regimes(rgb, K):
    """The regimes l3c_dmll_mean is judged in at a head shape: all of shape_regimes, except `sharp` at K = 1 -- with a single component the
    mean IS that component's mu, which `sharp` puts on bin edges: an exact rounding tie at a fifth to a half of the pixels, each of them
    excused by the rule (the cap on the excused share is about inputs; with K > 1 the weighted sum leaves the grid)."""
    return [r for r in shape_regimes(rgb) if not (K == 1 and r == 'sharp')]


def shape_id(C, K, rgb, alpha):
    return 'C{}K{}{}L{}'.format(C, K, 'rgb' if rgb else 'z', alpha[2])


def shape_case(C, K, rgb, alpha, regime, H, W, B=3, far_every=16):
    """`head_case` for any head: the inputs of one (shape, alphabet, regime, size) case, the same on the CPU and on the GPU side:
    P (B, Kp, H, W) fp32, sym int16 (B, C, H, W)."""
    if regime not in shape_regimes(rgb):
        raise ValueError('regime {!r} is not one of the shape cases (rgb={})'.format(regime, rgb))
    rng = np.random.RandomState(1000003 * REGIMES.index(regime) + 100019 * C + 5003 * K + 307 * alpha[2] + 100 * H + W + (5000 if rgb else 0))
    P = make_P(regime, rgb, B, H, W, C, K, rng, alpha=alpha)
    return P, near_sym(P, rgb, C, K, rng, far_every, alpha=alpha)


def tie_case(Lp, K):
    """Rows whose scaled CDF is EXACTLY k + 0.5 at one entry, in fp32 and in fp64 alike: a bottleneck-style head (no coupling) with C = 1
    and K equal logits (pi = 1 / K exactly, K a power of two); n components far below every bin edge (sigmoid = 1), one exactly ON edge j
    (sigmoid(0) = .5), the others far above (0) -- the CDF at edge j is (n + .5) / K, and with Lp = 1 + K the scale 65536 - K makes
    (n + .5) / K * scale = (2 n + 1) * (32768 / K - .5): a tie, to an even k for odd n and to an odd k for even n (Lp 3, K 2:
    16383.5 and 49150.5; Lp 5, K 4: 8191.5, 24574.5, 40957.5, 57340.5).  One pixel per (n, j), j = 1 .. Lp - 2.
    -> P (1, 3 K, 1, n_pix) fp32, targets (Lp,) fp32, the tied entry of every pixel (n_pix,)."""
    assert Lp == K + 1 and K & (K - 1) == 0
    t = np.linspace(-1.5, 1.5, Lp).astype(np.float32)
    cases = [(n, j) for n in range(K) for j in range(1, Lp - 1)]
    P = np.zeros((1, 3, 1, K, 1, len(cases)), dtype=np.float32)
    P[:, 2] = -9.0
    for i, (n, j) in enumerate(cases):
        P[0, 1, 0, :, 0, i] = [-1000.0] * n + [t[j]] + [1000.0] * (K - n - 1)
    return P.reshape(1, 3 * K, 1, len(cases)), t, np.array([j for _, j in cases])


# ---- the head in fp64 --------------------------------------------------------------------------------------------------------


def sigmoid64(a):
    return 0.5 * (1.0 + np.tanh(np.asarray(a, dtype=np.float64) / 2.0))


def _split(P, rgb, C):
    B, Kp, H, W = P.shape
    n = 4 if rgb else 3
    K = Kp // (n * C)
    return P.astype(np.float64).reshape(B, n, C, K, H, W), K


def _coupling64(l, x, rgb, c):
    """The two coupling terms sigmoid(lam) * x of channel c, (B, K, H, W) each (zeros where the channel has none)."""
    zero = np.zeros_like(l[:, 1, c])
    if not (rgb and c > 0):
        return zero, zero
    x = x.astype(np.float64)
    if c == 1:
        return sigmoid64(l[:, 3, 0]) * x[:, 0:1], zero
    return sigmoid64(l[:, 3, 1]) * x[:, 0:1], sigmoid64(l[:, 3, 2]) * x[:, 1:2]


def params64(P, x, rgb, C, K, c):
    """fp32 P (B, Kp, H, W), x (B, C, H, W) values of the coded channels -> fp64 pi, mu', log_sigma, each (B, K, H, W)."""
    l, K_ = _split(P, rgb, C)
    assert K_ == K
    logit = l[:, 0, c]
    e = np.exp(logit - logit.max(axis=1, keepdims=True))
    a, b = _coupling64(l, x, rgb, c)
    return e / e.sum(axis=1, keepdims=True), l[:, 1, c] + a + b, np.maximum(l[:, 2, c], LOG_SCALES_MIN)


def mu_bound64(P, x, rgb, C, K, c):
    """Bound on |fp32 mu' - fp64 mu'|: mu + (a + b) with a, b = sigmoid(lam) * x -- two additions, a product and a sigmoid (an expf, an
    addition and a division, each within an ulp) per term: 4 * 2^-24 * (|mu| + |a| + |b|), elementwise."""
    l, _ = _split(P, rgb, C)
    a, b = _coupling64(l, x, rgb, c)
    return 4 * U32 * (np.abs(l[:, 1, c]) + np.abs(a) + np.abs(b))


PI_BOUND = 8 * U32          # absolute: pi <= 1; K expf and a K-term sum in the denominator, one division


def cdf64(pi32, mu32, ls32, targets):
    """The mixture CDF in fp64 ON fp32 PARAMETERS (B, K, H, W) at the fp32 bin edges -> (B, H, W, Lp)."""
    pi, mu, ls = (np.asarray(v, dtype=np.float64)[..., None] for v in (pi32, mu32, ls32))
    t = np.asarray(targets, dtype=np.float64)
    return (pi * sigmoid64((t - mu) * np.exp(-ls))).sum(axis=1)


def entries64(cdf, Lp):
    """(rint(cdf * (65536 - (Lp - 1))) + l) & 0xFFFF, int64; cdf (..., Lp)."""
    assert cdf.shape[-1] == Lp
    return (np.rint(cdf * (65536 - (Lp - 1))).astype(np.int64) + np.arange(Lp)) & 0xFFFF


def as_u16(table):
    """int16 / uint16 table (numpy or torch) -> int64 numpy in 0 .. 65535."""
    if isinstance(table, torch.Tensor):
        table = table.cpu().numpy()
    return table.astype(np.int64) & 0xFFFF


def rows_increasing(entries):
    """Per row: strictly increasing over entries 0 .. Lp-2 (the last entry is never read: the top symbol's upper bound is 2^16)."""
    return (np.diff(entries[..., :-1], axis=-1) > 0).all(axis=-1)


class EntryStats(object):
    """Counts of one or more `check_entries` calls; `assert_caps` applies the two shares to the pooled counts."""

    def __init__(self):
        self.n = self.excused = self.mismatch = 0
        self.dev = 0.0

    def add(self, n, excused, mismatch, dev):
        self.n += n
        self.excused += excused
        self.mismatch += mismatch
        self.dev = max(self.dev, dev)
        return self

    def __str__(self):
        return 'dev {:.4f} counts, excused {:.3%}, mismatching {:.3%} of {} entries'.format(
            self.dev, self.excused / max(self.n, 1), self.mismatch / max(self.n, 1), self.n)

    def assert_caps(self, what):
        assert self.excused < EXCUSED_CAP * self.n, (what, 'excused share', self.excused, self.n)
        assert self.mismatch < MISMATCH_CAP * self.n, (what, 'mismatching share', self.mismatch, self.n)


def check_entries(got, pi32, mu32, ls32, targets, index=None, what='', stats=None):
    """The acceptance rule for uint16 table entries.  got: (B, H, W, Lp) entries (any integer type, taken mod 2^16), or with `index`
    (B, H, W, n) int: the entries index[..., j] of every row, got (B, H, W, n).
      dev    = max |oracle fp32 CDF - fp64 CDF| * scale over the case: the rounding deviation of the REFERENCE's fp32 statement on the same
               fp32 parameters, computed here on the CPU -- never from `got`
      delta  = 4 * dev  (the device's expf and division differ from the CPU's in the last bits; K terms are summed)
      an entry must EQUAL entries64 wherever the fp64 scaled value is further than delta from a half-integer, elsewhere it may differ by 1
      (mod 2^16).  Asserts that per entry; the two shares (excused < 15 %, differing at all < 1 %) are statistics: they are added to
      `stats` and asserted by EntryStats.assert_caps on a sample large enough to carry them."""
    t = np.asarray(targets, dtype=np.float32)
    Lp = t.shape[0]
    scale = float(65536 - (Lp - 1))
    c64 = cdf64(pi32, mu32, ls32, t)
    c32 = ocdf.mixture_cdf_float(*(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for v in (pi32, t, mu32, ls32)))
    dev = float(np.abs(c32.numpy().astype(np.float64) - c64).max() * scale)
    delta = 4 * dev
    scaled = c64 * scale
    want = entries64(c64, Lp)
    near_tie = np.abs(np.abs(scaled - np.floor(scaled)) - 0.5) <= delta
    got = as_u16(got)
    if index is not None:
        want, near_tie = np.take_along_axis(want, index, -1), np.take_along_axis(near_tie, index, -1)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = (got - want) & 0xFFFF
    diff = np.minimum(diff, 65536 - diff)
    unexcused = (diff != 0) & ~near_tie
    s = EntryStats().add(diff.size, int(near_tie.sum()), int((diff != 0).sum()), dev)
    print('{}: {}, max |difference| {}'.format(what, s, int(diff.max())))
    assert delta < 0.25, (what, 'the reference itself is ill-conditioned here', dev)
    assert not unexcused.any(), (what, 'entries differ where fp64 is not near a tie', int(unexcused.sum()), int(diff[unexcused].max()))
    assert diff.max() <= 1, (what, int(diff.max()))
    if stats is not None:
        stats.add(s.n, s.excused, s.mismatch, s.dev)
    return s


def bin_mass64(pi32, mu32, ls32, targets):
    """fp64 probability mass of every bin, (B, H, W, Lp - 1)."""
    return np.diff(cdf64(pi32, mu32, ls32, targets), axis=-1)


# ---- negative log-likelihood -------------------------------------------------------------------------------------------------


def _softplus64(a):
    return np.logaddexp(0.0, a)


def nll64(P, x, rgb, C, K, return_clamped=False, alpha=None):
    """forward() of the reference's loss in fp64 from fp32 P (B, Kp, H, W) and fp32 values x (B, C, H, W) -> (B, C, H, W) nats
    [, mask: every component of the element sits at the 1e-12 clamp of the bin's mass].  alpha: (x_min, x_max, L) of a head that is not one of
    the two shipped ones."""
    x_min, x_max, L = alphabet(rgb) if alpha is None else alpha
    half = (x_max - x_min) / (L - 1) / 2
    l, K_ = _split(P, rgb, C)
    assert K_ == K
    logit, mu, ls = l[:, 0], l[:, 1], np.maximum(l[:, 2], LOG_SCALES_MIN)
    x = x.astype(np.float64)[:, :, None]
    if rgb:
        lam = sigmoid64(l[:, 3])
        mu = np.stack((mu[:, 0], mu[:, 1] + lam[:, 0] * x[:, 0], mu[:, 2] + lam[:, 1] * x[:, 0] + lam[:, 2] * x[:, 1]), axis=1)
    centered = x - mu
    inv = np.exp(-ls)
    plus_in, min_in = inv * (centered + half), inv * (centered - half)
    mass = sigmoid64(plus_in) - sigmoid64(min_in)
    clamped = mass < 1e-12
    lp = np.log(np.maximum(mass, 1e-12))
    upper = np.float32(x_max - 0.001).astype(np.float64)
    lower = np.float32(x_min + 0.001).astype(np.float64)
    is_top, is_bottom = np.broadcast_to(x > upper, lp.shape), np.broadcast_to(x < lower, lp.shape)
    lp = np.where(is_top, -_softplus64(min_in), lp)
    lp = np.where(is_bottom, plus_in - _softplus64(plus_in), lp)
    log_pi = logit - logit.max(axis=2, keepdims=True)
    log_pi = log_pi - np.log(np.exp(log_pi).sum(axis=2, keepdims=True))
    s = lp + log_pi
    m = s.max(axis=2, keepdims=True)
    out = -(np.log(np.exp(s - m).sum(axis=2)) + m[:, :, 0])
    if return_clamped:
        return out, (clamped & ~is_top & ~is_bottom).all(axis=2)
    return out


NLL_SLACK_CAP, NLL_SLACK_SHARE = 1e-3, 0.02


def nll_tolerance(ref32, ref64):
    """Per element: the project's tolerance (2e-5 absolute + 2e-5 relative) plus 4 x the reference's own fp32 conditioning
    |oracle fp32 - fp64| (it matters where two sigmoids near 1 are subtracted).  -> (tolerance, share of elements whose slack term
    exceeds 1e-3: must stay below 2 % of the case)."""
    slack = 4 * np.abs(ref32.astype(np.float64) - ref64)
    return 2e-5 + 2e-5 * np.abs(ref32) + slack, float((slack > NLL_SLACK_CAP).mean())


# ---- the mixture's mean as symbols -------------------------------------------------------------------------------------------------

MEAN_EXCUSED_CAP = 0.02


def mean_rule64(P, got, rgb, C, K, alpha, c):
    """The rule of tests/test_gpu_preview.py::test_mean_kernel_against_fp64 for channel c of the symbols `got` (B, C, H, W) an implementation
    of l3c_dmll_mean returned: fp64 from P, conditioned on `got`'s own earlier channels.  -> (want, excused), (B, H, W) each: a pixel is
    excused iff fp64's scaled mean t is within bound / bw + 1e-6 of a rounding tie, with
        bound = sum_k (PI_BOUND + 16 u pi_k) (|mu_k| + |a_k| + |b_k|)         a, b: the two coupling terms, u = 2^-24;
    everywhere else the symbol must EQUAL want = clip(rint(t), 0, L-1).  The excused share is capped (MEAN_EXCUSED_CAP), not tolerated."""
    x_min, x_max, L = alpha
    bw = (x_max - x_min) / (L - 1)
    x = values_at(np.asarray(got), alpha)
    l, _ = _split(P, rgb, C)
    pi, mu, _ = params64(P, x, rgb, C, K, c)
    a, b = _coupling64(l, x, rgb, c)
    t = (np.clip((pi * mu).sum(axis=1), x_min, x_max) - x_min) / bw
    bound = ((PI_BOUND + 16 * U32 * pi) * (np.abs(l[:, 1, c]) + np.abs(a) + np.abs(b))).sum(axis=1)
    excused = np.abs(np.abs(t - np.floor(t)) - 0.5) <= bound / bw + 1e-6
    return np.clip(np.rint(t), 0, L - 1).astype(np.int64), excused


# ---- the thin convolutions ---------------------------------------------------------------------------------------------------


def conv1x1_64(x, w, b):
    """x (B, Cin, H, W), w (Cout, Cin), b (Cout,) -> fp64 value and the bound (Cin + 1) * 2^-24 * (sum |x w| + |b|): a chain of Cin fused
    multiply-adds and the bias addition, Cin + 1 roundings."""
    x, w, b = (np.asarray(v, dtype=np.float64) for v in (x, w, b))
    val = np.einsum('bihw,oi->bohw', x, w) + b.reshape(1, -1, 1, 1)
    mag = np.einsum('bihw,oi->bohw', np.abs(x), np.abs(w)) + np.abs(b).reshape(1, -1, 1, 1)
    return val, (w.shape[1] + 1) * U32 * mag


def dec_head64(bn_q, w, b, fuse):
    """1x1 conv C -> Cf (+ fuse (B, Cf, H, W) or None): C fused multiply-adds, the bias, the fuse addition."""
    val, _ = conv1x1_64(bn_q, w, b)
    mag = np.einsum('bihw,oi->bohw', np.abs(np.asarray(bn_q, dtype=np.float64)), np.abs(np.asarray(w, dtype=np.float64)))
    mag = mag + np.abs(np.asarray(b, dtype=np.float64)).reshape(1, -1, 1, 1)
    n = w.shape[1] + 1
    if fuse is not None:
        val, mag, n = val + fuse.astype(np.float64), mag + np.abs(fuse.astype(np.float64)), n + 1
    return val, n * U32 * mag


def _meanshift64(v, err, w, b):
    """3 -> 3 pointwise map ((v0 w0 + v1 w1) + v2 w2) + b with separately rounded products: a term passes through its product and up to
    three additions: 4 roundings; plus the input's own error through |w|."""
    w, b = np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64)
    val = np.einsum('bihw,oi->bohw', v, w) + b.reshape(1, 3, 1, 1)
    mag = np.einsum('bihw,oi->bohw', np.abs(v), np.abs(w)) + np.abs(b).reshape(1, 3, 1, 1)
    return val, np.einsum('bihw,oi->bohw', err, np.abs(w)) + 4 * U32 * mag


def _conv3x3_same(x, w):
    """x (B, Cin, H, W) fp64, w (Cout, Cin, 3, 3) fp64, zero padding 1 -> (B, Cout, H, W)."""
    B, Cin, H, W = x.shape
    xp = np.zeros((B, Cin, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((B, w.shape[0], H, W))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum('bihw,oi->bohw', xp[:, :, ky:ky + H, kx:kx + W], w[:, :, ky, kx])
    return out


def rgb_head64(img, w1, b1, w2, b2, w3, b3):
    """sub_rgb_mean -> MeanShift -> conv3x3 3 -> Cf (zero padding of the SHIFTED image).  -> shifted, its bound, out, its bound
    (27 fused multiply-adds and the bias: 28 roundings, plus the shifted image's error through |w3|)."""
    img = np.asarray(img, dtype=np.float64)
    u, eu = _meanshift64(img, np.zeros_like(img), np.reshape(w1, (3, 3)), b1)
    z, ez = _meanshift64(u, eu, np.reshape(w2, (3, 3)), b2)
    w3, b3 = np.asarray(w3, dtype=np.float64), np.asarray(b3, dtype=np.float64)
    out = _conv3x3_same(z, w3) + b3.reshape(1, -1, 1, 1)
    mag = _conv3x3_same(np.abs(z), np.abs(w3)) + np.abs(b3).reshape(1, -1, 1, 1)
    return z, ez, out, _conv3x3_same(ez, np.abs(w3)) + 28 * U32 * mag


def quantise_argmin(x32, levels32):
    """The reference's hard quantiser on fp32 values: argmin_l (x - level_l)^2 with the subtraction and the square each rounded to fp32,
    first minimum on ties (torch.min).  x32 (...,) fp32 -> (symbols int64, levels[symbols] fp32)."""
    x32, levels32 = np.asarray(x32, dtype=np.float32), np.asarray(levels32, dtype=np.float32)
    best = np.zeros(x32.shape, dtype=np.int64)
    dbest = np.square(x32 - levels32[0], dtype=np.float32)
    for l in range(1, levels32.shape[0]):
        d = np.square(x32 - levels32[l], dtype=np.float32)
        better = d < dbest
        best[better] = l
        dbest = np.where(better, d, dbest)
    return best, levels32[best]
