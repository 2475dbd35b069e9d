"""The plain-integer coder (tests/ac_trace.py) against the oracle, and the adversarial streams (tests/ac_adversarial.py) against what
they claim to reach.  CPU only: the GPU tests of the same streams are in tests/test_gpu_coder_underflow.py."""
import numpy as np
import pytest

from oracle import ac
from tests import ac_adversarial as A
from tests import ac_trace as T

ALL = A.CASES + [('constant_row', 3)]


def _case(name, Lp):
    return A.constant_row_case() if name == 'constant_row' else A.case(name, Lp)


def _agrees(tab, sym):
    data = T.emit(T.trace(tab, sym))
    assert data == ac.encode(tab, sym)
    assert (ac.decode(tab, data, len(sym)) == np.asarray(sym)).all()


@pytest.mark.parametrize('name,Lp', ALL)
def test_case_meets_its_precondition_and_trace_equals_oracle(name, Lp):
    """Building the case asserts what it reaches (its docstring in ac_adversarial); then emit(trace) is the oracle's byte string and
    the oracle decodes it back."""
    c = _case(name, Lp)
    print(A.summary_line(c))
    assert c.Lp == Lp and c.tab.shape[-1] == Lp and 0 <= c.sym.min() and c.sym.max() <= Lp - 2
    data = T.emit(c.trace)
    assert data == ac.encode(c.tab, c.sym)
    assert (ac.decode(c.tab, data, len(c.sym)) == c.sym).all()


def test_cases_use_symbol_zero_the_top_symbol_and_interior_ones():
    for Lp in (26, 257):
        c = A.case('many_serial', Lp)
        assert (c.sym == 0).any() and (c.sym == Lp - 2).any() and ((c.sym > 0) & (c.sym < Lp - 2)).any()
    c = A.case('many_serial', 3)
    assert (c.sym == 0).any() and (c.sym == 1).any()


def test_generator_is_deterministic_and_raises_when_it_cannot():
    plan = [('random', 40), ('settle', 1), ('run', 20, 30), ('resolve', 23), ('straddle', 12), ('neutral', 5), ('random', 10)]
    for Lp in A.LPS:
        a, b = A.build(plan, Lp, 7), A.build(plan, Lp, 7)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
        d = T.describe(T.trace(*a))
        assert d.e[71] == 23 and d.pending_before[71] == 20 and (d.e[41:71] == 0).all()
        m = T.trace(*a).m[72:84]
        assert (T.trace(*a).n[72:89] == 0).all() and (m > 0).all() and (m == 1).any() and (m >= 10).any() and (T.trace(*a).m[84:89] == 0).all()
        _agrees(*a)
        tab, sym = A.build([('random', 20), ('dense', 30), ('random', 5)], Lp, 9)
        iv = [T.interval(tab[i], sym[i]) for i in range(20, 50)]
        assert all(hi - lo == 1 for lo, hi in iv) and (T.trace(tab, sym).n[20:50] >= 16).all()
        _agrees(tab, sym)
    with pytest.raises(A.Infeasible):
        A.build([('settle', 1), ('run', 5, 10), ('resolve', 40)], 3, 0)         # 40 - 5 common-prefix bits do not exist
    with pytest.raises(A.Infeasible):
        A.build([('settle', 1), ('straddle', 3), ('quiet', 1)], 26, 0)          # quiet means nothing pending
    with pytest.raises(A.Infeasible):
        A.build([('settle', 1), ('run', 200, 10)], 257, 0)                      # 20 underflow bits a symbol do not exist


def test_trace_equals_oracle_on_reference_kats(golden):
    g = golden('ac_kat.npz')
    names = sorted({k.split('/')[0] for k in g.files if k.endswith('/sym')})
    assert len(names) >= 8
    for name in names:
        tab, sym, ref = g[name + '/cdf'], g[name + '/sym'], g[name + '/bytes'].tobytes()
        assert T.emit(T.trace(tab, sym)) == ref, name
        _agrees(tab, sym)


def test_trace_equals_oracle_on_random_tables():
    from tests import gpu_util as gu
    rng = np.random.RandomState(11)
    for it in range(50):
        Lp = int(rng.choice([2, 3, 26, 130, 257]))
        N = int(rng.randint(1, 700))
        tab = gu.random_tables(rng, 1, N, Lp, shape=rng.choice([0.05, 0.3, 2.0]))[0]
        sym = gu.sample_symbols(rng, tab) if it % 2 else rng.randint(0, Lp - 1, size=N).astype(np.int16)
        _agrees(tab, sym)


def test_what_the_older_fixtures_reach(golden):
    """The figures the comments on `underflow_Lp3` (tests/golden/make_golden.py) and test_hostsim_degenerate_intervals quote: neither
    comes near the serial path of the bit-packing kernel."""
    g = golden('ac_kat.npz')
    d = T.describe(T.trace(g['underflow_Lp3/cdf'], g['underflow_Lp3/sym']))
    assert d.longest_run == 5 and d.e.max() == 6 and not any(st.serial for st in d.steps)
