"""The range coder's per-symbol state machine in plain Python integers (TEST INFRASTRUCTURE).

A third statement of the coder next to oracle/ac_oracle.c (bit-at-a-time loop) and csrc/ac_core.h (closed form): `step` mirrors
interval_update + renorm_counts of ac_core.h, `emit` writes the bits by the literal rule, and `describe` says what the encoder's
bit-packing kernel (ac_pack_body in csrc/ac_kernels.hip) meets on a stream: how many bits every symbol emits, which of its steps
take the serial path and what they are handed.  No ctypes, no compiled code: the tests pin it against the oracle."""
from collections import namedtuple

import numpy as np

# ac_pack_body codes kPackThreads = kPackWaves * 64 = 256 symbols per step ...
PACK_STEP = 256
# ... and sends a step through its serial path when some symbol of it emits more than 32 bits (`__any(e > 32u)`)
SERIAL_THRESHOLD = 32
WAVE = 64                       # symbols per wavefront of a step

_M32 = 0xFFFFFFFF
TOP = 1 << 31

Trace = namedtuple('Trace', 'low1 n m final_low')
Step = namedtuple('Step', 'serial bits bit_off_mod32 pending')
Description = namedtuple('Description', 'e pending_before steps final_pending longest_run total_bits')


def step(low, high, c_lo, c_hi):
    """One symbol from the resting state (low, high) -> (low', n, m, low, high): low' the lower bound right after the interval
    update, n the common-prefix bits of low'/high', m the underflow bits, then the renormalised state."""
    rng = (high - low) & _M32
    hi1 = (low - 1 + ((rng * c_hi + c_hi) >> 16)) & _M32
    lo1 = (low + ((rng * c_lo + c_lo) >> 16)) & _M32
    n = 32 - (lo1 ^ hi1).bit_length()
    if n >= 32:
        low, high = 0, _M32
    else:
        low = (lo1 << n) & _M32
        high = ((hi1 << n) | ((1 << n) - 1)) & _M32
    m = 32 - (~((low & ~high) << 1) & _M32).bit_length()
    if m:
        low = (low << m) & 0x7FFFFFFF
        high = ((high << m) | TOP | ((1 << m) - 1)) & _M32
    return lo1, n, m, low, high


def interval(row, x):
    """(c_low, c_high) of symbol x in a table row of Lp entries: the top symbol's c_high is the constant 2^16."""
    return int(row[x]), (0x10000 if x == len(row) - 2 else int(row[x + 1]))


def trace(tab, sym):
    """tab: (N, Lp) uint16 table, or one row (Lp,) shared by all symbols; sym: N symbols -> Trace(low1, n, m, final_low)."""
    tab = np.asarray(tab)
    if tab.dtype == np.int16:
        tab = tab.view(np.uint16)
    sym = np.asarray(sym).reshape(-1)
    N = len(sym)
    rows = tab.tolist()
    one_row = tab.ndim == 1
    low, high = 0, _M32
    low1, ns, ms = [0] * N, [0] * N, [0] * N
    for i, x in enumerate(sym.tolist()):
        c_lo, c_hi = interval(rows if one_row else rows[i], x)
        low1[i], ns[i], ms[i], low, high = step(low, high, c_lo, c_hi)
    return Trace(np.array(low1, dtype=np.uint32), np.array(ns, dtype=np.int64), np.array(ms, dtype=np.int64), low)


def emit(tr):
    """The byte string of a trace by the literal rule: a symbol with n > 0 writes the first of the top n bits of low', then the
    complement of it once per pending bit, then the other n - 1 bits, and leaves pending = m; one with n == 0 adds m to pending.
    The flush writes the quadrant bit of the final low with pending + 1 complements; zeros pad to a byte."""
    out = []
    pending = 0
    for lo1, n, m in zip(tr.low1.tolist(), tr.n.tolist(), tr.m.tolist()):
        if n:
            first = lo1 >> 31
            out.append('1' if first else '0')
            out.append(('0' if first else '1') * pending)
            if n > 1:
                out.append(format((lo1 >> (32 - n)) & ((1 << (n - 1)) - 1), '0{}b'.format(n - 1)))
            pending = m
        else:
            pending += m
    first = 0 if tr.final_low < 0x40000000 else 1
    out.append('1' if first else '0')
    out.append(('0' if first else '1') * (pending + 1))
    bits = ''.join(out)
    bits += '0' * (-len(bits) % 8)
    return int(bits, 2).to_bytes(len(bits) // 8, 'big')


def describe(tr):
    """What the bit-packing kernel meets: per symbol e (bits emitted: n + pending_before, 0 when n == 0) and pending_before; per
    step of PACK_STEP symbols Step(serial: any e > SERIAL_THRESHOLD, bits emitted, bit_off & 31 and pending at step entry)."""
    N = len(tr.n)
    e = np.zeros(N, dtype=np.int64)
    pb = np.zeros(N, dtype=np.int64)
    pending = 0
    longest = 0
    for i, (n, m) in enumerate(zip(tr.n.tolist(), tr.m.tolist())):
        pb[i] = pending
        if n:
            e[i] = n + pending
            pending = m
        else:
            pending += m
        longest = max(longest, pending)
    steps = []
    bit_off = 0
    for s0 in range(0, N, PACK_STEP):
        es = e[s0:s0 + PACK_STEP]
        steps.append(Step(bool((es > SERIAL_THRESHOLD).any()), int(es.sum()), bit_off & 31, int(pb[s0])))
        bit_off += int(es.sum())
    return Description(e, pb, steps, pending, longest, bit_off + pending + 2)
