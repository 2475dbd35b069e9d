"""The planning half of Bitcoding._repair restated for tests/test_native_repair_abi.py (no GPU): which groups a round rebuilds and from
which window of rows (bitcoding/bitcoding.py: the selection loop of _repair), on seals read by container.split_seal."""
from l3c_pytorch_amd.bitcoding import container


def select_groups(seals, band_words, frame_hw, paddings, tried):
    """-> [(file, c, g, erased bands, r0)] in the order Bitcoding._repair takes them; `tried`: the set of the groups of all earlier rounds."""
    n = band_words.shape[2]
    _, failing, _ = container.failing_bands(seals, band_words, frame_hw, paddings)
    groups = []
    for i, bad in failing.items():
        if seals[i].parity is None:
            continue
        bad, m, R = set(bad), seals[i].parity_groups, seals[i].parity_streams
        erasures = {}
        for j in sorted({j for _, j in bad}):
            c = min(c for c, jj in bad if jj == j)
            erasures.setdefault((c, j % m), []).append(j)
        for (c, g), js in sorted(erasures.items()):
            if len(js) > R or any((c, o) in bad for o in range(g, n, m) if o not in js):
                continue
            r0 = next((r for r in range(R - len(js) + 1) if (i, c, g, tuple(js), r) not in tried), None)
            if r0 is not None:
                groups.append((i, c, g, tuple(js), r0))
    groups.sort(key=lambda group: seals[group[0]].parity_streams > 1)
    return groups
