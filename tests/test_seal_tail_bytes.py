"""The bytes of every seal tail, pinned (no GPU): tests/golden/seal_tails.json holds small synthetic bodies and the tails this project wrote
behind them -- version 1 (on a legacy and on a banded body), version 2, version 3 'L3CP' with G = 2 and G = 5, 'L3CQ' with R = 2 and R = 4.
container.make_seal, split_seal -> make_seal, and the C writers behind l3c_seal_write / _write_bands / _write_parity / _write_parity_rs
must all give these bytes, and the two *_bytes functions their lengths: the Python reference and csrc/seal.h cannot drift together unseen.
`python tests/test_seal_tail_bytes.py` writes the fixture anew (only for a deliberate change of the format)."""
import ctypes
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path.insert(0, ROOT)

import l3c_pytorch_amd  # noqa: E402,F401
from l3c_pytorch_amd import _lib  # noqa: E402
from l3c_pytorch_amd.bitcoding import container  # noqa: E402

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'seal_tails.json')
H, W, L = 16, 20, 64                                   # the finest record: 320 pixels in n = 5 bands, C = 3


def _make_cases():
    """The fixture's content from this tree's container.py: two banded bodies (two and three records) and a legacy one."""
    rng = np.random.RandomState(20)
    n = container.n_bands(H * W, L)
    # [3][5] payload lengths: empty bands, unequal members inside the groups of G = 2 (m = 3: {0, 3}, {1, 4}, {2}) and of G = 5 (m = 1), and with
    # G = 2 two empty parity payloads in the last channel
    lens = [[0, 7, 3, 9, 2], [5, 0, 0, 1, 12], [0, 4, 0, 0, 0]]
    bodies = []
    for coarse in ([(1, 8, 10, 128)], [(1, 4, 5, 64), (2, 8, 10, 64)]):
        finest = [[rng.randint(0, 256, k).astype(np.uint8).tobytes() for k in row] for row in lens]
        payloads = [[[rng.randint(0, 256, 1 + j + c).astype(np.uint8).tobytes() for j in range(container.n_bands(h * w, l))] for c in range(C)]
                    for C, h, w, l in coarse]
        bodies.append((container.write_file((1, 2, 3, 4), coarse + [(3, H, W, L)], payloads + [finest], True), finest))
    legacy = container.write_file((0, 5, 0, 6), [(1, 4, 5), (3, 8, 10)], [[b'ab'], [b'', b'cde', b'f']], False)
    cases = [dict(name='legacy v1', body=legacy.hex(), generation=3, frame_crc=0xCAFEF00D, model_id=7, tail=container.make_seal(legacy, 3, 0xCAFEF00D, 7).hex())]
    for k, (body, finest) in enumerate(bodies):
        frame = rng.randint(0, 256, 3 * H * W).astype(np.uint8).tobytes()
        crcs = [[zlib.crc32(frame[c * H * W + j * L:c * H * W + min((j + 1) * L, H * W)]) for j in range(n)] for c in range(3)]
        base = dict(body=body.hex(), generation=3 + k, frame_crc=zlib.crc32(frame), model_id=0x1122334455667788 + k)
        cases.append(dict(base, name='body {} v1'.format(k), tail=container.make_seal(body, base['generation'], base['frame_crc'], base['model_id']).hex()))
        base.update(band_len=L, band_crcs=crcs)
        cases.append(dict(base, name='body {} v2'.format(k),
                          tail=container.make_seal(body, base['generation'], base['frame_crc'], base['model_id'], crcs, L).hex()))
        for G, R in ((2, 1), (5, 1), (2, 2), (5, 4)):
            rows = [container.rs_parity(ch, G, R) for ch in finest]              # [c][g][r]
            parity = [[p[0] for p in row] for row in rows] if R == 1 else rows
            tail = container.make_seal(body, base['generation'], base['frame_crc'], base['model_id'], crcs, L, parity=(G, parity))
            cases.append(dict(base, name='body {} v3 G={} R={}'.format(k, G, R), G=G, R=R, rows=[[[p.hex() for p in g] for g in row] for row in rows],
                              tail=tail.hex()))
    return cases


def _cases():
    with open(FIXTURE) as f:
        cases = json.load(f)
    for case in cases:
        case['body'], case['tail'] = bytes.fromhex(case['body']), bytes.fromhex(case['tail'])
        if 'band_crcs' in case:
            case['band_crcs'] = np.asarray(case['band_crcs'], dtype=np.uint32)
        if 'rows' in case:
            case['rows'] = [[[bytes.fromhex(p) for p in g] for g in row] for row in case['rows']]
    return cases


def _make_seal(case, parity=None):
    return container.make_seal(case['body'], case['generation'], case['frame_crc'], case['model_id'], case.get('band_crcs'), case.get('band_len'),
                               parity=parity)


def test_the_fixture_covers_every_kind_of_tail():
    cases = _cases()
    kinds = {(c['tail'][-20], c.get('G'), c.get('R')) for c in cases}
    assert kinds == {(1, None, None), (2, None, None), (3, 2, 1), (3, 5, 1), (3, 2, 2), (3, 5, 4)}
    assert {c['tail'][:4] for c in cases if 'rows' in c} == {b'L3CP', b'L3CQ'}
    assert any(not container.is_banded(c['body']) for c in cases)
    for c in cases:
        if 'rows' in c:
            lens = [[len(g[0]) for g in row] for row in c['rows']]
            assert c['band_crcs'].shape == (3, 5) and (0 in sum(lens, [])) == (c['G'] == 2) and len(set(sum(lens, []))) > 1, c['name']
    assert os.path.getsize(FIXTURE) < 32 * 1024


def test_make_seal_writes_the_fixture_bytes():
    for c in _cases():
        if 'rows' not in c:
            assert _make_seal(c) == c['tail'], c['name']
            continue
        if c['R'] == 1:                                    # 'L3CP': payloads, or lists of one payload
            assert _make_seal(c, (c['G'], [[g[0] for g in row] for row in c['rows']])) == c['tail'], c['name']
        assert _make_seal(c, (c['G'], c['rows'])) == c['tail'], c['name']


def test_split_seal_then_make_seal_is_a_round_trip():
    for c in _cases():
        for view in (False, True):
            body, seal = container.split_seal(c['body'] + c['tail'], view=view)
            assert bytes(body) == c['body'] and (seal.generation, seal.frame_crc, seal.model_id) == (c['generation'], c['frame_crc'], c['model_id']), c['name']
            parity = None if seal.parity is None else (seal.parity_group, seal.parity)
            assert seal.parity_streams == c.get('R') and seal.parity_group == c.get('G'), c['name']
            assert container.make_seal(bytes(body), seal.generation, seal.frame_crc, seal.model_id, seal.band_crcs, seal.band_len, parity=parity) == c['tail'], \
                c['name']
            if 'rows' in c:                                # the documented shapes of Seal.parity: payloads for R = 1, lists of R payloads above
                want = [[g[0] for g in row] for row in c['rows']] if c['R'] == 1 else c['rows']
                got = [[bytes(g) for g in row] for row in seal.parity] if c['R'] == 1 else [[[bytes(p) for p in g] for g in row] for row in seal.parity]
                assert got == want and seal.parity_groups == len(want[0]), c['name']


def test_the_c_writers_write_the_fixture_bytes_and_state_their_lengths():
    lib = _lib.load()
    for c in _cases():
        body, tail = c['body'], c['tail']
        seal = ctypes.byref(_lib.Seal(c['generation'], c['frame_crc'], c['model_id']))
        padding = body[6:14] if container.is_banded(body) else body[:8]
        out = ctypes.create_string_buffer(len(tail))

        def wrote(rc):
            got = out.raw
            ctypes.memset(out, 0xEE, len(tail))
            return rc == 0 and got == tail
        if 'band_crcs' not in c:
            assert len(tail) == 24 and wrote(lib.l3c_seal_write(seal, padding, out)), c['name']
            continue
        words, n = np.ascontiguousarray(c['band_crcs']), c['band_crcs'].shape[1]
        if 'rows' not in c:
            assert lib.l3c_seal_bands_bytes(n) == len(tail), c['name']
            assert wrote(lib.l3c_seal_write_bands(seal, padding, words.ctypes.data, n, c['band_len'], out)), c['name']
            continue
        G, R, rows = c['G'], c['R'], c['rows']
        m = len(rows[0])
        plen = np.asarray([len(g[0]) for row in rows for g in row], dtype=np.uint32)
        payloads = b''.join(p for row in rows for g in row for p in g)
        assert len(payloads) == R * int(plen.sum())
        assert lib.l3c_seal_parity_rs_bytes(n, m, R, len(payloads)) == len(tail), c['name']
        assert wrote(lib.l3c_seal_write_parity_rs(seal, padding, words.ctypes.data, n, c['band_len'], G, R, plen.ctypes.data, payloads, out)), c['name']
        if R == 1:
            assert lib.l3c_seal_parity_bytes(n, m, len(payloads)) == len(tail), c['name']
            assert wrote(lib.l3c_seal_write_parity(seal, padding, words.ctypes.data, n, c['band_len'], G, plen.ctypes.data, payloads, out)), c['name']


if __name__ == '__main__':
    with open(FIXTURE, 'w') as f:
        json.dump(_make_cases(), f, indent=0, sort_keys=True)
        f.write('\n')
    print('wrote', FIXTURE, os.path.getsize(FIXTURE), 'bytes')
