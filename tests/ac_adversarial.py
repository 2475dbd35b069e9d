"""Streams that drive the range coder where random data never goes (TEST INFRASTRUCTURE): long runs of underflow ("pending")
bits, resolved at chosen symbol positions with a chosen number of emitted bits.

`build(plan, Lp, seed)` follows the coder state with tests/ac_trace.step and picks, symbol by symbol, a strictly increasing table row
and a symbol of the kind the plan asks for.  The split of the current interval that lands on 2^31 is
c0 = ((2^31 - low) << 16) // span; the coded interval [c0 - j, c0 + 1 + j) keeps 2^31 inside for any jitter j, and the jitter sets
how many underflow bits the symbol adds.  A segment that cannot be had within its candidate budget raises Infeasible.

`CASES` names the streams the suite runs (see each function's docstring); `case(name, Lp)` builds one, checks from
ac_trace.describe that it reaches what it is meant to reach (AssertionError otherwise) and caches it for the session."""
import functools
import itertools
from collections import namedtuple

import numpy as np

from tests import ac_trace as T

LPS = (3, 26, 257)
N_CASE = 1300               # 5 whole pack steps and a ragged sixth: the 4-step record ring of ac_pack_body reloads
_BUDGET = 4000              # candidate intervals tried per symbol


class Infeasible(Exception):
    pass


class _Misaligned(Exception):
    """The stream is what the case wants except for where its bits fall in the 32-bit words: the case tries its next seed."""


class _Gen:
    def __init__(self, Lp, seed):
        self.Lp, self.top = Lp, Lp - 2
        self.rng = np.random.RandomState(seed)
        self.low, self.high, self.pending = 0, 0xFFFFFFFF, 0
        self.rows, self.syms = [], []

    # ---- placing an interval (c_lo, c_hi) in a strictly increasing row ---------------------------------------------------------
    def _places(self, c_lo, c_hi):
        """symbols x that can carry [c_lo, c_hi): x entries below c_lo, top - 1 - x entries above c_hi up to 65535."""
        if not 0 <= c_lo < c_hi <= 0x10000:
            return None
        if c_hi == 0x10000:
            return (self.top, self.top) if c_lo >= self.top else None
        a, b = max(0, self.top - 1 - (65535 - c_hi)), min(c_lo, self.top - 1)
        return (a, b) if a <= b else None

    def _increasing(self, k, a, b):
        """k strictly increasing values in [a, b)."""
        return np.sort(self.rng.randint(0, b - a - k + 1, size=k)) + np.arange(k) + a

    def _commit(self, c_lo, c_hi):
        a, b = self._places(c_lo, c_hi)
        want = (0, self.top, int(self.rng.randint(a, b + 1)), b, a)[len(self.syms) % 5]   # symbol 0, the top one, interior ones
        x = min(max(want, a), b)
        row = np.zeros(self.Lp, dtype=np.int64)
        row[:x] = self._increasing(x, 0, c_lo)
        row[x] = c_lo
        if x < self.top:
            row[x + 1] = c_hi
            row[x + 2:self.top + 1] = self._increasing(self.top - 1 - x, c_hi + 1, 65536)
        # entry Lp - 1 is never read (the top symbol's c_high is the constant 2^16): the wrapped 0 of a real table, or anything above
        last = int(row[self.top])
        row[self.top + 1] = 0 if last == 65535 or len(self.syms) % 2 else self.rng.randint(last + 1, 65536)
        lo1, n, m, self.low, self.high = T.step(self.low, self.high, c_lo, c_hi)
        self.pending = m if n else self.pending + m
        self.rows.append(row)
        self.syms.append(x)
        return n, m

    def _pick(self, candidates, ok, what):
        tried = 0
        for c_lo, c_hi in candidates:
            tried += 1
            if tried > _BUDGET:
                break
            c_lo, c_hi = int(c_lo), int(c_hi)
            if self._places(c_lo, c_hi) is None:
                continue
            lo1, n, m, low, high = T.step(self.low, self.high, c_lo, c_hi)
            if ok(n, m, low, high):
                return self._commit(c_lo, c_hi)
        raise Infeasible('{} at symbol {} (Lp {}, low {:#x}, high {:#x}, pending {}) after {} candidates'.format(
            what, len(self.syms), self.Lp, self.low, self.high, self.pending, tried - 1))

    # ---- candidate intervals ---------------------------------------------------------------------------------------------------
    def _span(self):
        return self.high - self.low + 1

    def _around(self, point, jitters):
        """intervals that keep `point` (inside [low, high]) inside: [c0 - ja, c0 + 1 + jb) around the split that lands on it"""
        c0 = ((point - self.low) << 16) // self._span()
        for ja, jb in jitters:
            yield max(0, c0 - ja), min(0x10000, c0 + 1 + jb)

    def _random_intervals(self, widths):
        for w in widths:
            w = int(min(max(w, 1), 0x10000))
            c_lo = int(self.rng.randint(0, 0x10000 - w + 1))
            yield c_lo, c_lo + w

    def _straddles(self, m_want):
        """n == 0 and m_want underflow bits: the farther of low', high' lies 2^(31 - m) .. 2^(32 - m) from 2^31"""
        unit = self._span() / 65536.0
        j0 = (1 << (31 - m_want)) / unit
        scales = (1.4, 1.1, 1.7, 1.25, 1.55, 1.0, 1.9, 0.9, 2.0)
        jit = []
        for s in scales:
            j = int(j0 * s)
            jit += [(j, j), (j, j // 2), (j // 2, j), (j, 0), (0, j), (j, int(self.rng.randint(0, j + 1)))]
        return self._around(T.TOP, jit)

    # ---- the kinds of a plan ---------------------------------------------------------------------------------------------------
    def random(self):
        r, rng = self.rng.randint(3), self.rng
        if r == 0:
            w = (65536.0 * rng.rand() ** 3 for _ in range(50))              # anything, narrow ones often
        elif r == 1:
            w = (65536.0 * (1.0 - 0.3 * rng.rand()) for _ in range(50))     # likely symbols
        else:
            w = (2.0 ** rng.uniform(0, 16) for _ in range(50))
        return self._pick(self._random_intervals(itertools.chain(w, [2000.0] * 200)), lambda n, m, lo, hi: True, 'random')

    def straddle(self, m_want=None):
        order = [m_want] if m_want else [int(v) for v in self.rng.permutation([1, 1, 2, 3, 5, 8, 10, 11, 12, 14])]
        for mw in order:
            try:
                return self._pick(self._straddles(mw), lambda n, m, lo, hi: n == 0 and m == mw, 'straddle')
            except Infeasible:
                if m_want:
                    raise
        return self._pick(self._around(T.TOP, [(j, j) for j in range(0, 3000, 7)]), lambda n, m, lo, hi: n == 0 and m > 0, 'straddle')

    def neutral(self):
        r, k = self.rng, self.top + 4
        cand = ((r.randint(0, k), 0x10000 - r.randint(0, k)) for _ in range(40))
        rest = [(0, 0x10000 - j) for j in range(self.top, self.top + 40)] + [(j, 0x10000) for j in range(self.top, self.top + 40)]
        return self._pick(itertools.chain(cand, rest), lambda n, m, lo, hi: n == 0 and m == 0, 'neutral')

    def quiet(self):
        if self.pending:
            raise Infeasible('quiet at symbol {} with pending {}'.format(len(self.syms), self.pending))
        return self.neutral()

    def settle(self):
        """n > 0 and m == 0: ends whatever run there was, owes nothing, and leaves an interval near the full range (so that a long
        hold of near-certain symbols can follow)."""
        w = (65536.0 * 2.0 ** -self.rng.uniform(0.5, 6) for _ in range(_BUDGET))
        return self._pick(self._random_intervals(w), lambda n, m, lo, hi: 0 < n <= 8 and m == 0 and self.pending + n <= T.SERIAL_THRESHOLD
                          and lo < (1 << 28) and hi >= (1 << 32) - (1 << 28), 'settle')

    def dense(self, ok=None):
        ok = ok or (lambda n, m: n >= 16)
        return self._pick(self._random_intervals([1] * _BUDGET), lambda n, m, lo, hi: ok(n, m), 'dense')

    def resolve(self, e):
        n_want = e - self.pending
        if not 1 <= n_want <= 16:
            raise Infeasible('resolve({}) at symbol {} with pending {}'.format(e, len(self.syms), self.pending))
        span, unit = self._span(), self._span() / 65536.0
        cand = []
        # around the odd multiples of 2^(31 - n) inside the interval: low' and high' agree above that bit and differ in it
        q = 1 << (31 - n_want)
        for p in range(self.low // (2 * q) * 2 * q + q, self.high, 2 * q):
            if self.low + span // 64 < p < self.high - span // 64:
                cand += list(self._around(p, [(j, j) for j in (0, 1, 3, 10, 40, 150, 600)]))
            if len(cand) > 200:
                break
        w = ((1 << (32 - n_want)) / unit * self.rng.uniform(0.2, 1.0) for _ in range(_BUDGET))
        self.rng.shuffle(cand)
        return self._pick(itertools.chain(cand, self._random_intervals(w)), lambda n, m, lo, hi: n == n_want, 'resolve({})'.format(e))

    def run(self, target, count):
        """`count` symbols with n == 0 that take pending to exactly `target`: straddles of varied m, near-certain holds between."""
        for left in range(count, 0, -1):
            need = target - self.pending
            if need < 0 or need > 14 * left:
                raise Infeasible('run to {} with pending {} and {} symbols left'.format(target, self.pending, left))
            avg = need / left
            if need == 0 or (need <= left - 1 and self.rng.rand() > avg):
                try:
                    self.neutral()
                    continue
                except Infeasible:
                    if need == 0:
                        raise
            # (the last bit is kept for the last symbol: a hold at the target is not always to be had, a hold below it can be a straddle)
            lo, hi = max(1, need - 12 * (left - 1)), min(need - 1 if left > 1 and need > 1 else need, 14)
            first = int(min(max(self.rng.choice([1, round(avg), round(2 * avg), 10 + self.rng.randint(5)]), lo), hi))
            for mw in sorted(range(lo, hi + 1), key=lambda v: abs(v - first)):
                try:
                    self.straddle(mw)
                    break
                except Infeasible:
                    pass
            else:
                raise Infeasible('run: no straddle with m in [{}, {}] at symbol {}'.format(lo, hi, len(self.syms)))
        if self.pending != target:
            raise Infeasible('run ended with pending {} instead of {}'.format(self.pending, target))

    def alternate(self, count):
        """straddles up to 14..16 pending bits, then a width-1 symbol that emits 29..32 bits; again and again.  (From a near-full
        interval a width-1 symbol is 2^16 - 1 wide and all but never inside one aligned 2^16 block: n is 14..17 here, not >= 16.)"""
        for _ in range(count):
            if self.pending < 14:
                # (a straddle from a near-full interval cannot add more than about 14 bits: from little, get there in two)
                for mw in [int(t) - self.pending for t in self.rng.permutation([16, 15, 14])] if self.pending >= 4 else (8, 7, 9, 6, 10):
                    try:
                        if 1 <= mw <= 14:
                            self.straddle(mw)
                            break
                    except Infeasible:
                        pass
                else:
                    raise Infeasible('alternate: no straddle from pending {}'.format(self.pending))
            else:
                p = self.pending
                self.dense(lambda n, m: 29 <= n + p <= T.SERIAL_THRESHOLD and m <= 4)


def build(plan, Lp, seed):
    """plan: list of (kind, count) with kind in random / straddle / neutral / quiet / dense / settle / alternate, ('run', target,
    count) and ('resolve', e)  ->  (tab uint16 (N, Lp), sym int16 (N,)).  Deterministic for a seed."""
    assert Lp in LPS, Lp
    g = _Gen(Lp, seed)
    for seg in plan:
        kind = seg[0]
        if kind == 'resolve':
            g.resolve(seg[1])
        elif kind == 'run':
            g.run(seg[1], seg[2])
        elif kind == 'alternate':
            g.alternate(seg[1])
        elif kind in ('random', 'straddle', 'neutral', 'quiet', 'dense', 'settle'):
            for _ in range(seg[1]):
                getattr(g, kind)()
        else:
            raise ValueError(kind)
    tab = np.stack(g.rows).astype(np.uint16)
    assert (np.diff(tab[:, :Lp - 1].astype(np.int64), axis=1) > 0).all()
    return tab, np.array(g.syms, dtype=np.int16)


def build_constant_row(N, periods):
    """One row [0, 32767, wrap] for every symbol: the symbol whose interval contains 2^31 (n == 0, the run grows by about a bit a
    symbol), and after periods[k] symbols of the k-th run the OTHER symbol, which resolves it."""
    row = np.array([0, 32767, 0], dtype=np.uint16)
    low, high = 0, 0xFFFFFFFF
    sym, k, since = [], 0, 0
    for _ in range(N):
        inside = [x for x in (0, 1) if T.step(low, high, *T.interval(row, x))[1] == 0]
        assert len(inside) == 1, inside
        x = inside[0]
        if since >= periods[k % len(periods)]:
            x, k, since = 1 - x, k + 1, -1
        since += 1
        low, high = T.step(low, high, *T.interval(row, x))[3:]
        sym.append(x)
    return row, np.array(sym, dtype=np.int16)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
Case = namedtuple('Case', 'name Lp tab sym trace desc marks')   # marks: symbol positions by name (resolvers, run starts)
S = T.PACK_STEP


def resolver_plan(items, N=N_CASE):
    """items: (R, e, L, n) in order: a settle at R - L - 1, a run of L symbols to pending e - n, the resolver at R; random elsewhere"""
    plan, pos = [], 0
    for R, e, L, n in items:
        gap = R - L - 1 - pos
        assert gap >= 0, (R, L, pos)
        plan += [('random', gap), ('settle', 1), ('run', e - n, L), ('resolve', e)]
        pos = R + 1
    return plan + [('random', N - pos)]


def _serial_steps(d):
    return [k for k, st in enumerate(d.steps) if st.serial]


def _check_run(tr, d, start, R):
    """a run that starts from nothing at `start` and is resolved at R"""
    assert d.pending_before[start] == 0 and (tr.n[start:R] == 0).all() and tr.n[R] > 0, (start, R)


def _threshold(e, p):
    def make(Lp, seed):
        """A resolver that emits exactly e bits at lane p of step 2: e == 32 stays on the parallel path in every step, e == 33 makes
        step 2 the stream's one serial step.  p == 0: the whole run is carried in (it fills step 1); 63 / 64: the run lies in
        wavefront 0 and the resolver is its last lane / lane 0 of wavefront 1; 255: the run lies in wavefront 3."""
        R = 2 * S + p
        L = {0: S, 63: 63, 64: 64, 255: 63}[p]
        tab, sym = build(resolver_plan([(R, e, L, 2)]), Lp, seed)
        tr = T.trace(tab, sym)
        d = T.describe(tr)
        _check_run(tr, d, R - L, R)
        assert d.e[R] == e and np.delete(d.e, R).max() <= T.SERIAL_THRESHOLD, (d.e[R], d.e.max())
        assert _serial_steps(d) == ([2] if e > T.SERIAL_THRESHOLD else []), _serial_steps(d)
        if p == 0:
            assert d.steps[2].pending == e - 2 and d.steps[1].pending == 0
        return tab, sym, tr, d, {'resolver': R, 'run_start': R - L}
    return make


def _serial_between(Lp, seed):
    """The run starts in wavefront 3 of step 1 and is resolved by symbol 10 of step 2 with e = 47: step 1 parallel, step 2 serial and
    entered with a partial word, step 3 parallel, entered with the partial word the serial path hands back, and emitting bits."""
    start, R = S + 200, 2 * S + 10
    tab, sym = build(resolver_plan([(R, 47, R - start, 3)]), Lp, seed)
    tr = T.trace(tab, sym)
    d = T.describe(tr)
    _check_run(tr, d, start, R)
    assert 3 * 64 <= start - S < S and d.e[R] == 47 >= 40
    assert _serial_steps(d) == [2] and d.steps[3].bits > 0 and d.steps[2].pending > 0
    if d.steps[2].bit_off_mod32 == 0 or d.steps[3].bit_off_mod32 == 0:
        raise _Misaligned
    return tab, sym, tr, d, {'resolver': R, 'run_start': start}


def _long_run(Lp, seed):
    """650 symbols with n == 0 take pending to 398 across steps 1 and 2, which emit nothing; the resolver at 850 emits 400 bits
    (the k > 32 loop of put_with_pending, twelve times over); random symbols follow."""
    start, R = 200, 850
    tab, sym = build(resolver_plan([(R, 400, R - start, 2)]), Lp, seed)
    tr = T.trace(tab, sym)
    d = T.describe(tr)
    _check_run(tr, d, start, R)
    assert R - start >= 600 and d.e[R] == 400 and d.longest_run == 398
    assert d.steps[1].bits == 0 and d.steps[2].bits == 0 and d.steps[1].pending < d.steps[2].pending < d.steps[3].pending
    assert _serial_steps(d) == [3]
    if d.steps[3].bit_off_mod32 == 0 or d.steps[4].bit_off_mod32 == 0:
        raise _Misaligned
    return tab, sym, tr, d, {'resolver': R, 'run_start': start}


def _run_to_end(Lp, seed):
    """The stream ends inside a run: nothing emits from symbol 900 on, no step is serial, and the flush writes the 60 pending bits."""
    tab, sym = build([('random', 899), ('settle', 1), ('run', 60, N_CASE - 900)], Lp, seed)
    tr = T.trace(tab, sym)
    d = T.describe(tr)
    assert d.final_pending == 60 >= 33 and not _serial_steps(d) and d.steps[4].bits == 0 and d.steps[5].bits == 0
    assert (tr.n[900:] == 0).all() and d.pending_before[900] == 0
    if d.steps[4].bit_off_mod32 == 0:
        raise _Misaligned
    return tab, sym, tr, d, {'run_start': 900}


def _serial_last_step(Lp, seed):
    """The ragged last step is serial (a resolver with e = 40 at its symbol 10) and the stream ends in a new run: the flush starts
    from the serial path's pending and partial word."""
    R = 5 * S + 10
    plan = resolver_plan([(R, 40, 90, 2)])[:-1] + [('straddle', N_CASE - R - 1)]
    tab, sym = build(plan, Lp, seed)
    tr = T.trace(tab, sym)
    d = T.describe(tr)
    _check_run(tr, d, R - 90, R)
    assert _serial_steps(d) == [5] and d.final_pending >= 1 and d.e[R] == 40
    if (sum(st.bits for st in d.steps) & 31) == 0:
        raise _Misaligned
    return tab, sym, tr, d, {'resolver': R, 'run_start': R - 90}


def _quiet(Lp, seed):
    """Near-certain symbols from 301 to 1030 with nothing pending: steps 2 and 3 emit no bit at all while a partial word is carried."""
    tab, sym = build([('random', 300), ('settle', 1), ('quiet', 730), ('random', N_CASE - 1031)], Lp, seed)
    tr = T.trace(tab, sym)
    d = T.describe(tr)
    for k in (2, 3):
        assert d.steps[k].bits == 0 and d.steps[k].pending == 0, (k, d.steps[k])
    assert d.steps[4].pending == 0 and d.steps[4].bits > 0 and not _serial_steps(d)
    if d.steps[2].bit_off_mod32 == 0:
        raise _Misaligned
    return tab, sym, tr, d, {}


def _dense_straddle(Lp, seed):
    """Straddles to 14..16 pending bits and width-1 symbols in turn over steps 1 and 2 (and some of 0 and 3): e = 29..32 again and
    again, never more, so every step stays on the parallel path with its widest symbols; marks keeps the bits of every step."""
    tab, sym = build([('random', 199), ('settle', 1), ('alternate', 700), ('random', N_CASE - 900)], Lp, seed)
    tr = T.trace(tab, sym)
    d = T.describe(tr)
    big = (d.e >= 29) & (d.e <= T.SERIAL_THRESHOLD)
    assert not _serial_steps(d) and big[S:2 * S].sum() >= 40 and big[2 * S:3 * S].sum() >= 40, (big[S:2 * S].sum(), big[2 * S:3 * S].sum())
    assert (d.e == T.SERIAL_THRESHOLD).sum() >= 10
    return tab, sym, tr, d, {'bits_per_step': [st.bits for st in d.steps]}


def _many_serial(Lp, seed):
    """Serial steps 0, 1, 3 and 4 (e = 34, 64, 65, 47), parallel steps 2 and 5 between and after them."""
    items = [(200, 34, 99, 2), (300, 64, 59, 1), (900, 65, 150, 3), (1100, 47, 30, 4)]
    tab, sym = build(resolver_plan(items), Lp, seed)
    tr = T.trace(tab, sym)
    d = T.describe(tr)
    assert _serial_steps(d) == [0, 1, 3, 4] and [int(d.e[R]) for R, _, _, _ in items] == [34, 64, 65, 47]
    return tab, sym, tr, d, {'resolvers': [R for R, _, _, _ in items]}


# Every case at every Lp, except:
#   quiet at Lp 257 -- the likeliest symbol of a 257-entry row has probability 1 - 255 / 2^16, so 512 symbols cost at least 2.8 bits,
#   and two whole steps cannot go by without a bit emitted or pending.
_MAKERS = {}
for _e in (32, 33):
    for _p in (0, 63, 64, 255):
        _MAKERS['threshold_e{}_p{}'.format(_e, _p)] = _threshold(_e, _p)
_MAKERS.update(serial_between=_serial_between, long_run=_long_run, run_to_end=_run_to_end, serial_last_step=_serial_last_step,
               quiet=_quiet, dense_straddle=_dense_straddle, many_serial=_many_serial)
CASES = [(name, Lp) for Lp in LPS for name in _MAKERS if not (name == 'quiet' and Lp == 257)]
_SEEDS = 24                 # word alignments are 31 in 32 right: the seeds after the first are for the rest


@functools.lru_cache(maxsize=None)
def case(name, Lp):
    base = 1000 * (sorted(_MAKERS).index(name) + 1) + Lp
    for seed in range(base, base + _SEEDS):
        try:
            tab, sym, tr, d, marks = _MAKERS[name](Lp, seed)
        except _Misaligned:
            continue
        assert len(sym) == N_CASE and d.total_bits <= 16 * N_CASE       # the encoder's output slot holds 16 bits a symbol
        tab.setflags(write=False)
        sym.setflags(write=False)
        return Case(name, Lp, tab, sym, tr, d, marks)
    raise AssertionError('{} Lp {}: no seed gives the word alignment the case needs'.format(name, Lp))


@functools.lru_cache(maxsize=None)
def constant_row_case():
    """Case `constant_row` (Lp 3 only: the row is the case): 1 500 symbols of the row [0, 32767, wrap], runs resolved after 20 .. 150
    symbols.  The broadcast-row encode and ac_decode_const_row_kernel."""
    row, sym = build_constant_row(1500, (20, 70, 33, 150, 64, 100, 31, 32))
    tr = T.trace(row, sym)
    d = T.describe(tr)
    assert len(_serial_steps(d)) >= 1 and d.longest_run >= 64, (_serial_steps(d), d.longest_run)
    row.setflags(write=False)
    sym.setflags(write=False)
    return Case('constant_row', 3, row, sym, tr, d, {})


def all_cases():
    return [case(name, Lp) for name, Lp in CASES] + [constant_row_case()]


def summary_line(c):
    """what the case reaches, for the record: largest e, longest pending run, serial steps and bit_off & 31 where they hand over"""
    ser = _serial_steps(c.desc)
    hand = [(c.desc.steps[k].bit_off_mod32, c.desc.steps[k + 1].bit_off_mod32 if k + 1 < len(c.desc.steps) else
             (sum(st.bits for st in c.desc.steps) & 31)) for k in ser]
    return '{:22s} Lp {:3d}  max e {:3d}  longest run {:3d}  serial steps {}  bit_off&31 in/out {}'.format(
        c.name, c.Lp, int(c.desc.e.max()), c.desc.longest_run, ser, hand)
