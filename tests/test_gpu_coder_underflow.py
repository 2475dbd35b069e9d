"""-m gpu: the HIP range coder on the streams of tests/ac_adversarial.py -- pending runs in the hundreds, resolvers that emit 32, 33,
... 400 bits at chosen lanes of a pack step, streams that end inside a run.  These are the only inputs in the suite that take the
serial path of the encoder's bit-packing kernel (ac_pack_body: `sh.rare`) and its hand-over back to the parallel path (pending, bit
offset, partial word); tests/test_ac_adversarial.py proves on the CPU that every stream reaches what it claims.  The oracle is the
truth everywhere; integer work, everything exact."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ac as oracle_ac  # noqa: E402
from tests import ac_adversarial as A  # noqa: E402
from tests import ac_trace as T  # noqa: E402

N = A.N_CASE
S_PLAIN = 33                # one more than the 32 streams a wavefront of the encoder's phase 1 codes


@functools.lru_cache(maxsize=None)
def _stack(Lp):
    """every case of this Lp and random streams up to S_PLAIN, all N symbols long -> (names, tabs, syms, oracle bytes)"""
    from tests import gpu_util as gu
    cases = [A.case(name, lp) for name, lp in A.CASES if lp == Lp]
    rng = np.random.RandomState(Lp)
    n_rand = S_PLAIN - len(cases)
    rt = gu.random_tables(rng, n_rand, N, Lp, shape=0.3)
    rs = gu.sample_symbols(rng, rt)
    tabs = np.concatenate([np.stack([c.tab for c in cases]), rt])
    syms = np.concatenate([np.stack([c.sym for c in cases]), rs])
    names = [c.name for c in cases] + ['random{}'.format(i) for i in range(n_rand)]
    want = [oracle_ac.encode(tabs[s], syms[s]) for s in range(S_PLAIN)]
    return names, tabs, syms, want


def _first_difference(a, b):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return 'lengths {} / {}, first differing byte {}'.format(len(a), len(b), k)


@pytest.mark.parametrize('Lp', A.LPS)
def test_plain_launch_vs_oracle(Lp):
    from tests import gpu_util as gu
    names, tabs, syms, want = _stack(Lp)
    assert tabs.shape == (S_PLAIN, N, Lp)
    got = gu.hip_encode_streams(tabs, syms)
    bad = [(names[s], _first_difference(got[s], want[s])) for s in range(S_PLAIN) if got[s] != want[s]]
    assert not bad, bad


def test_grouped_launch_vs_oracle():
    """The same streams as groups of different (S, N, Lp) in ONE launch pair: every case of every Lp, the random streams, the constant
    row's stream as a table of equal rows, and prefixes of the Lp 26 streams that end inside step 4 (N = 1100: three serial steps of
    many_serial behind them, the long run resolved, another flush)."""
    from l3c_pytorch_amd import ops
    streams = []
    for Lp in A.LPS:
        names, tabs, syms, want = _stack(Lp)
        k = sum(1 for _, lp in A.CASES if lp == Lp)
        streams.append((tabs[:k], syms[:k], want[:k], names[:k]))
        streams.append((tabs[k:], syms[k:], want[k:], names[k:]))
    c = A.constant_row_case()
    streams.append((np.tile(c.tab, (1, len(c.sym), 1)), c.sym[None], [oracle_ac.encode(c.tab, c.sym)], [c.name]))
    names, tabs, syms, _ = _stack(26)
    pt, ps = np.ascontiguousarray(tabs[:15, :1100]), np.ascontiguousarray(syms[:15, :1100])
    streams.append((pt, ps, [oracle_ac.encode(pt[s], ps[s]) for s in range(15)], [n + '[:1100]' for n in names[:15]]))
    assert len({(t.shape[0], t.shape[1]) for t, _, _, _ in streams}) >= 5
    groups = []
    for t, s, _, _ in streams:
        Sg, Ng, Lp = t.shape
        tt = torch.from_numpy(np.ascontiguousarray(t).view(np.int16)).cuda().reshape(Sg * Ng, Lp)
        groups.append((ops.intervals_from_table(tt, torch.from_numpy(np.ascontiguousarray(s)).cuda(), Sg, Ng), Sg, Ng))
    res, _ = ops.ac_encode_groups(groups)
    bad = []
    for g, ((out, n), (t, _, want, names)) in enumerate(zip(res, streams)):
        n, out = n.cpu().numpy(), out.cpu().numpy()
        for s in range(len(want)):
            got = out[s, :n[s]].tobytes()
            if got != want[s]:
                bad.append((g, t.shape, names[s], _first_difference(got, want[s])))
    assert not bad, bad


@pytest.mark.parametrize('monotone', [True, False])
@pytest.mark.parametrize('Lp', A.LPS)
def test_decode_vs_oracle(Lp, monotone):
    """The oracle's bytes through the lean pass (monotone) and the ring pass: a decoder meets the run as `value` shifted 400 bits on
    in one symbol."""
    from tests import gpu_util as gu
    names, tabs, syms, want = _stack(Lp)
    dec = gu.hip_decode_streams(tabs, want, monotone)
    bad = [(names[s], int((dec[s] != syms[s]).sum()), int(np.argmax(dec[s] != syms[s]))) for s in range(S_PLAIN) if (dec[s] != syms[s]).any()]
    assert not bad, bad


@pytest.mark.parametrize('Lp', A.LPS)
def test_chunked_decode_cut_inside_runs_and_at_resolvers(Lp):
    """l3c_ac_decode_chunks with the cuts 512 and 576: directly before the 33-bit resolver of threshold_e33_p0 (512) and of
    threshold_e33_p64 (576), directly after that of threshold_e33_p63 (575), inside the run of serial_between (456 .. 522) and twice
    inside the long run (200 .. 850).  The carried state must be the one-shot decoder's."""
    from l3c_pytorch_amd import ops
    names = ['threshold_e33_p0', 'threshold_e33_p64', 'threshold_e33_p63', 'serial_between', 'long_run', 'many_serial']
    cs = [A.case(name, Lp) for name in names]
    cuts = (0, 512, 576, N)
    assert cs[0].marks['resolver'] == 512 and cs[1].marks['resolver'] == 576 and cs[2].marks['resolver'] + 1 == 576
    assert all(c.desc.e[c.marks['resolver']] == 33 for c in cs[:3])
    for c, inside in ((cs[3], (512,)), (cs[4], (512, 576))):
        assert all(c.marks['run_start'] < p < c.marks['resolver'] and c.desc.pending_before[p] > 0 for p in inside)
    assert all(p % 64 == 0 for p in cuts[:-1])
    Sn = len(cs)
    tabs, syms = np.stack([c.tab for c in cs]), np.stack([c.sym for c in cs])
    payloads = [oracle_ac.encode(c.tab, c.sym) for c in cs]
    buf, offs, lens = ops.pack_streams(payloads)
    for flag_value in (0, 1):
        out = torch.full((Sn, N + 7), -7, dtype=torch.int16, device='cuda')      # row stride != stream length
        flag = torch.full((1,), flag_value, dtype=torch.int32, device='cuda')
        states = [ops.ac_decode_state(Sn), ops.ac_decode_state(Sn)]
        for j in range(len(cuts) - 1):
            p0, n = cuts[j], cuts[j + 1] - cuts[j]
            chunk = torch.from_numpy(np.ascontiguousarray(tabs[:, p0:p0 + n]).view(np.int16)).cuda().reshape(Sn * n, Lp)
            ops.ac_decode_chunks([ops.ac_decode_part(chunk, buf, offs, lens, Sn, n, flag, states[(j + 1) & 1] if j else None,
                                                     states[j & 1], j == len(cuts) - 2, out, N + 7, p0)])
        got = out.cpu().numpy()
        assert (got[:, :N] == syms).all(), (flag_value, [(names[s], int((got[s, :N] != syms[s]).sum())) for s in range(Sn)])
        assert (got[:, N:] == -7).all()


@functools.lru_cache(maxsize=None)
def _constant_row_streams():
    c = A.constant_row_case()
    others = [A.build_constant_row(len(c.sym), p)[1] for p in ((40, 33, 34), (300, 5, 64))]
    return c.tab, np.stack([c.sym] + others)


def test_constant_row_broadcast():
    """One row for every symbol (row stride 0): the broadcast-row encode and ac_decode_const_row_kernel on runs of up to 300 bits."""
    from l3c_pytorch_amd import ops
    row, sym = _constant_row_streams()
    Sn, Nn = sym.shape
    want = [oracle_ac.encode(row, sym[s]) for s in range(Sn)]
    assert max(T.describe(T.trace(row, sym[s])).longest_run for s in range(Sn)) >= 300
    trow = torch.from_numpy(row.view(np.int16).copy()).cuda()
    iv = ops.intervals_from_table(trow, torch.from_numpy(sym.copy()).cuda(), Sn, Nn, broadcast_row=True)
    out, n = ops.ac_encode(iv, Sn, Nn)
    n, out = n.cpu().numpy(), out.cpu().numpy()
    for s in range(Sn):
        assert out[s, :n[s]].tobytes() == want[s], (s, _first_difference(out[s, :n[s]].tobytes(), want[s]))
    buf, offs, lens = ops.pack_streams(want)
    for monotone in (True, False):
        dec = ops.ac_decode(trow, buf, offs, lens, Sn, Nn, monotone, broadcast_row=True).cpu().numpy()
        assert (dec == sym).all(), (monotone, [int((dec[s] != sym[s]).sum()) for s in range(Sn)])


def test_raw_entry_point_keeps_a_bad_stream_inside_its_slot():
    """l3c_ac_encode itself (the torchac facade refuses such tables before it gets there): stream 2 of seven codes symbols whose
    intervals are empty or reversed (c_high <= c_low), which may ask for up to 31 bits a symbol.  Its length must come back as
    L3C_AC_OVERRUN (0xFFFFFFFF) or fit the slot; its neighbours -- both with a serial step of their own -- and the rows in front of and
    behind the seven slots must be untouched by it.  Stream 2 is never decoded."""
    from l3c_pytorch_amd import _lib, ops
    from tests import gpu_util as gu
    Sn, Nn, Lp = 7, 600, 3
    rng = np.random.RandomState(600)
    tabs = gu.random_tables(rng, Sn, Nn, Lp, shape=0.3)
    syms = gu.sample_symbols(rng, tabs)
    for s, seed in ((1, 1), (3, 3)):
        tabs[s], syms[s] = A.build(A.resolver_plan([(300, 47, 60, 2)], N=Nn), Lp, seed)
        assert [st.serial for st in T.describe(T.trace(tabs[s], syms[s])).steps] == [False, True, False]
    c = rng.randint(0, 65536, size=Nn)
    tabs[2, :, 0] = c                                              # symbol 0 is coded: [c, c) on even rows,
    tabs[2, :, 1] = np.where(np.arange(Nn) % 2, c // 2, c)         # [c, c / 2) on odd ones
    syms[2] = 0
    assert (tabs[2, :, 1] <= tabs[2, :, 0]).all()
    want = [oracle_ac.encode(tabs[s], syms[s]) for s in range(Sn) if s != 2]
    stride = _lib.load().l3c_ac_max_bytes(Nn)
    t = torch.from_numpy(np.ascontiguousarray(tabs).view(np.int16)).cuda().reshape(Sn * Nn, Lp)
    iv = ops.intervals_from_table(t, torch.from_numpy(syms).cuda(), Sn, Nn)
    slots = torch.full((Sn + 2, stride), 0xA5, dtype=torch.uint8, device='cuda')       # a guard row on either side
    nbytes = torch.empty(Sn, dtype=torch.int32, device='cuda')
    ws = torch.empty(_lib.load().l3c_ac_encode_workspace_bytes(Sn), dtype=torch.uint8, device='cuda')
    _lib.call('l3c_ac_encode', _lib.ptr(iv), Sn, Nn, _lib.ptr(slots[1:Sn + 1]), stride, _lib.ptr(nbytes), _lib.ptr(ws), _lib.stream())
    n = nbytes.cpu().numpy().view(np.uint32)
    out = slots.cpu().numpy()
    print('bad stream: nbytes {:#x}, stride {}'.format(int(n[2]), stride))
    assert (out[0] == 0xA5).all() and (out[Sn + 1] == 0xA5).all()
    assert n[2] == 0xFFFFFFFF or n[2] <= stride
    for s, w in zip([s for s in range(Sn) if s != 2], want):
        assert n[s] == len(w) and out[1 + s, :n[s]].tobytes() == w, (s, int(n[s]), len(w))
