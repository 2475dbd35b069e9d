"""Zero-length chunks and per-stream finality (csrc/ac_core.h: chunk_is_empty, chunk_no_advance, entry_step / entry_npix /
entry_final_chunk -- what the HIP decoders and l3c_decode_rgb_entries instantiate) on the host: a KAT stream decoded through a chunk sequence
with empty chunks in it and the final flag on its last non-empty chunk gives the symbols of the one-shot decode; the chunking rule is the
planner's (ops.rgb_entries_plan).

What is shared with the kernels is the RULE: which chunk is empty, which symbol does not advance the state, how an entry is cut.  What an
empty chunk then DOES -- hand the record on, write nothing -- is the simulator's own loop here and an early return of their own in the
kernels (ring_decode_body, lean_decode_body); the record checks below pin the simulator to the contract, they do not run the kernels' code.
The kernels' empty chunks are exercised on the GPU, in all three row forms (tests/test_gpu_banded_set.py: every RGB call of the mixed set
has empty chunks, and every scale's symbols must be decode_batch's)."""
import numpy as np

from tests.hostsim import ac_hostsim as hs
from tests.hostsim import chunk_hostsim as cs


def _names(g):
    return sorted({k.split('/')[0] for k in g.files if k.endswith('/sym')})


def _sequences(N, rng):
    """Chunk sequences for a stream of N symbols: (chunk lengths, index of the final chunk)."""
    lib = cs.get()
    for chunks in (1, 2, 3, 8, 33, 64):                          # the lock-step rule: trailing chunks empty when the stream is short
        lens = [lib.hostsim_entry_npix(N, chunks, k) for k in range(chunks)]
        yield lens, lib.hostsim_entry_final_chunk(N, chunks)
    for _ in range(6):                                           # arbitrary cuts with empty chunks INTERLEAVED (before, between, after)
        cuts = sorted(rng.randint(0, N + 1, size=rng.randint(0, 6)).tolist())
        lens = list(np.diff([0] + cuts + [N]))
        for pos in sorted(rng.randint(0, len(lens) + 1, size=rng.randint(1, 5)).tolist(), reverse=True):
            lens.insert(pos, 0)
        yield lens, max(k for k, n in enumerate(lens) if n > 0)


def test_chunk_sequences_with_empty_chunks_decode_the_kat_symbols(golden):
    g = golden('ac_kat.npz')
    rng = np.random.RandomState(3)
    n_seq = 0
    for n in _names(g):
        tab, sym, ref = g[n + '/cdf'], g[n + '/sym'], g[n + '/bytes'].tobytes()
        if tab.ndim != 2 or tab.shape[0] != len(sym):
            continue                                             # (a KAT that codes every symbol with one row: no per-symbol rows to cut)
        N = len(sym)
        want = hs.decode(tab, ref, N, True)
        assert (want == sym).all()
        for lens, final in _sequences(N, rng):
            assert sum(lens) == N and lens[final] > 0 and not any(lens[final + 1:])
            got, rec, written = cs.decode_chunks(tab, ref, lens, final)
            assert written == N and (got == want).all(), (n, lens, final)
            for k, ln in enumerate(lens):                        # the contract of an empty chunk: the record it was given, bit for bit
                if ln == 0 and k > 0:
                    assert (rec[k] == rec[k - 1]).all(), (n, lens, k)
            n_seq += 1
    assert n_seq >= 24


def test_the_final_flag_on_another_chunk_is_not_the_same_decode(golden):
    """The rule matters: with the flag one chunk early the symbol after that chunk's last is decoded from a state that never advanced."""
    g = golden('ac_kat.npz')
    differs = 0
    for n in _names(g):
        tab, sym, ref = g[n + '/cdf'], g[n + '/sym'], g[n + '/bytes'].tobytes()
        if tab.ndim != 2 or tab.shape[0] != len(sym) or len(sym) < 256:
            continue
        N = len(sym)
        lens = [N // 2, 0, N - N // 2, 0]
        good, _, _ = cs.decode_chunks(tab, ref, lens, 2)
        early, _, _ = cs.decode_chunks(tab, ref, lens, 0)
        assert (good == sym).all()
        assert (early[:N // 2] == sym[:N // 2]).all()
        differs += int((early != sym).any())
    assert differs >= 1


def test_chunking_rule_is_the_planners():
    from l3c_pytorch_amd import ops
    lib = cs.get()
    lens = np.asarray([1, 63, 64, 65, 128, 4096, 4160, 16384, 1056768, 64 * 33 - 1], dtype=np.int64)
    for chunks in (1, 2, 7, 8, 34, 64, 256):
        start, npix, final, _ = ops.rgb_entries_plan(lens, chunks)
        for e, n in enumerate(lens):
            step = lib.hostsim_entry_step(int(n), chunks)
            assert step % 64 == 0 and step * chunks >= n and (step - 64) * chunks < n
            assert [lib.hostsim_entry_npix(int(n), chunks, k) for k in range(chunks)] == npix[:, e].tolist()
            assert lib.hostsim_entry_final_chunk(int(n), chunks) == final[e]
            assert all(start[k, e] == k * step for k in range(chunks) if npix[k, e] > 0)
