"""Region decode, the host side (no GPU): region_plan against a brute-force walk over the pixels, the halo against the fp64 oracle network,
and the box / padding errors."""
import random

import numpy as np
import pytest
import torch

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd.bitcoding import region
from l3c_pytorch_amd.bitcoding.container import band_len, n_bands
from l3c_pytorch_amd.helpers import synthetic
from oracle import net as onet

HALO = 40


def _cases(n=400):
    rnd = random.Random(16)
    out = [(320, 88, 16, (180, 200)), (320, 88, 0, (0, 40)), (328, 88, 64, (298, 328)), (8, 8, 1, (0, 8)), (64, 8, 64, (63, 64))]
    while len(out) < n:
        H, W = 8 * rnd.randint(1, 60), 8 * rnd.randint(1, 24)
        K = rnd.choice([0, 1, 2, 3, 4, 16, 64, 256, 1024])        # 0: a legacy file, L = H W
        y0 = rnd.randrange(H)
        y1 = rnd.choice([y0 + 1, H, rnd.randint(y0 + 1, H), min(H, y0 + rnd.randint(1, 70))])
        out.append((H, W, K, (y0, y1)))
    return out


@pytest.mark.parametrize('cut', [True, False], ids=['cut', 'whole_last_band'])
def test_region_plan_brute_force(cut):
    for H, W, K, (y0, y1) in _cases():
        HW = H * W
        L = band_len(HW, K) if K else HW
        plan = region.region_plan(H, W, L, (y0, y1), HALO, cut=cut)
        ctx = (H, W, K, L, (y0, y1), plan)
        (j0, j1), (p0, p1), (c0, c1), (v0, v1) = plan.bands, plan.sym_rows, plan.conv_rows, plan.valid_rows
        # the bands are those that hold a pixel of the rows, found pixel by pixel
        band_of = np.arange(y0 * W, y1 * W) // L
        assert (j0, j1) == (int(band_of.min()), int(band_of.max()) + 1), ctx
        assert 0 <= j0 < j1 <= n_bands(HW, L), ctx
        # every entry starts at a band start; every pixel of the rows lies in exactly one entry
        assert plan.hw == (c1 - c0) * W and len(plan.pix0) == len(plan.length) == j1 - j0, ctx
        cover = np.zeros(HW, dtype=np.int32)
        for j, a, n in zip(range(j0, j1), plan.pix0, plan.length):
            first = int(a) + c0 * W
            assert first == j * L and n > 0, ctx
            assert 0 <= a and a + n <= plan.hw, ctx                                   # inside the window image
            assert first + n <= min((j + 1) * L, HW), ctx                              # inside its band
            cover[first:first + n] += 1
        assert (cover[y0 * W:y1 * W] == 1).all() and cover.max() == 1, ctx
        # the symbol rows are the smallest rows that hold every entry's pixels
        decoded = np.flatnonzero(cover)
        assert p0 == decoded[0] // W and (p0, p1) == (j0 * L // W, y1 if cut else -(-min(j1 * L, HW) // W)), ctx
        if cut:
            assert decoded[-1] == y1 * W - 1, ctx                                      # the decoder stops with the rows' last pixel
        else:
            assert decoded[-1] == min(j1 * L, HW) - 1 and p1 == decoded[-1] // W + 1, ctx
        # the conv rows: a multiple of the granule or an image border, and valid rows that hold the symbol rows
        assert 0 <= c0 < c1 <= H and (c0 % 64 == 0) and (c1 % 64 == 0 or c1 == H), ctx
        assert (v0, v1) == (0 if c0 == 0 else c0 + HALO, H if c1 == H else c1 - HALO), ctx
        assert v0 <= p0 <= y0 and y1 <= p1 <= v1, ctx
        # ... and no wider than the granule asks for
        assert c0 == 0 or p0 - HALO - c0 < 64, ctx
        assert c1 == H or c1 - (p1 + HALO) < 64, ctx
        pixbase, hw, pix0, length = region.entry_table(plan, 3)
        assert pixbase.tolist() == [b * plan.hw for b in range(3) for _ in range(j1 - j0)] and (hw == plan.hw).all(), ctx
        assert pix0.tolist() == plan.pix0.tolist() * 3 and length.tolist() == plan.length.tolist() * 3, ctx


def test_region_plan_the_named_cases():
    L = band_len(320 * 88, 16)
    assert L == 1792
    plan = region.region_plan(320, 88, L, (180, 200), HALO)             # band 8 starts in row 162: 122 rounds down to 64
    assert plan.bands == (8, 10) and plan.sym_rows == (162, 200) and plan.conv_rows == (64, 256) and plan.valid_rows == (104, 216)
    plan = region.region_plan(320, 88, L, (190, 210), HALO)             # band 9 starts in row 183
    assert plan.bands == (9, 11) and plan.sym_rows == (183, 210) and plan.conv_rows == (128, 256) and plan.valid_rows == (168, 216)
    assert plan.pix0.tolist() == [9 * L - 128 * 88, 10 * L - 128 * 88] and plan.length.tolist() == [L, 210 * 88 - 10 * L]
    legacy = region.region_plan(320, 88, 320 * 88, (0, 40), HALO)
    assert legacy.bands == (0, 1) and legacy.conv_rows == (0, 128) and legacy.valid_rows == (0, 88) and legacy.length.tolist() == [40 * 88]
    whole = region.region_plan(328, 88, band_len(328 * 88, 64), (0, 328), HALO)
    assert whole.conv_rows == whole.valid_rows == whole.sym_rows == (0, 328) and int(whole.length.sum()) == 328 * 88


@pytest.mark.parametrize('rows', [(5, 5), (7, 3), (-1, 4), (0, 321), (320, 321)])
def test_region_plan_refuses_bad_rows(rows):
    with pytest.raises(ValueError):
        region.region_plan(320, 88, 1792, rows, HALO)


def test_halo_rows_of_the_config(synthetic_l3c_cal):
    cfg, _ = synthetic_l3c_cal
    assert region.halo_rows(cfg) == HALO == 2 * (2 * onet.L3C_HYPER.dec_blocks + 2) + 4


def test_apron_of_the_decoder_stage(synthetic_l3c_cal):
    """Four rows per 3x3 layer of the decoder (a Winograd tile), 18 layers, at half resolution, up to the granule: 192 frame rows."""
    cfg, _ = synthetic_l3c_cal
    assert region.apron_rows(cfg) == 192 and region.apron_rows(cfg) % region.GRANULE == 0
    assert region.apron_rows(cfg) // 2 >= 4 * (2 * cfg.dec.num_blocks + 2)
    assert region.decoder_rows(320, (128, 256), 192) == (0, 320)
    assert region.decoder_rows(2048, (960, 1152), 192) == (768, 1344)
    assert region.decoder_rows(712, (640, 712), 192) == (448, 712) and region.decoder_rows(712, (0, 128), 192) == (0, 320)


def test_halo_against_the_oracle(synthetic_l3c_cal):
    """fp64 oracle network, calibrated checkpoint, a 320x88 image: P of scale 0 from z1 and F1 cropped to a row window equals the full
    frame's within 1e-9 exactly on the window's valid rows -- the next row on either cut side does not (the same criterion: it is off by
    more than 1e-9; with this checkpoint by 4e-9 .. 7e-9, the corner taps of 18 convolutions in a row, and by 1e-6 five rows further out)."""
    _, sd = synthetic_l3c_cal
    sd = {k: v.double() for k, v in sd.items()}
    H, W = 320, 88
    with torch.no_grad():
        out = onet.forward(synthetic.make_image(H, W, 3, 'natural').double().unsqueeze(0), sd)
        full = out.P[0]
        for (c0, c1), (v0, v1), rows in (((128, 256), (168, 216), (170, 214)), ((0, 128), (0, 88), (10, 80)), ((192, 320), (232, 320), (240, 320))):
            plan = region.region_plan(H, W, band_len(H * W, 64), rows, HALO)
            assert plan.conv_rows == (c0, c1) and plan.valid_rows == (v0, v1)
            P, _ = onet.get_P(0, out.bn[1][:, :, c0 // 2:c1 // 2], out.F_dec[1][:, :, c0 // 2:c1 // 2], sd)
            diff = (P - full[:, :, c0:c1]).abs().amax(dim=(0, 1, 3))                   # per row of the window
            assert float(diff[v0 - c0:v1 - c0].max()) <= 1e-9, ((c0, c1), float(diff[v0 - c0:v1 - c0].max()))
            if c0:
                assert float(diff[v0 - c0 - 1]) > 1e-9, ((c0, c1), 'row above', float(diff[v0 - c0 - 1]))
            if c1 < H:
                assert float(diff[v1 - c0]) > 1e-9, ((c0, c1), 'row below', float(diff[v1 - c0]))


# ---- errors ------------------------------------------------------------------------------------------------------------------------

PAD = (2, 3, 1, 2)          # left, right, top, bottom: a 317x83 image centre-padded to 320x88


def test_parse_box_maps_into_the_frame():
    assert region.parse_box((0, 317), PAD, (320, 88)) == ((1, 318), (2, 85))
    assert region.parse_box((180, 200, 10, 11), PAD, (320, 88)) == ((181, 201), (12, 13))
    assert region.parse_box([5, 6], (0, 0, 0, 0), (320, 88)) == ((5, 6), (0, 88))


@pytest.mark.parametrize('box', [(5, 5), (9, 4), (0, 10, 7, 7), (0, 10, 9, 3),               # empty
                                 (-1, 4), (0, 318), (317, 318), (0, 10, -1, 5), (0, 10, 0, 84), (0, 10, 83, 84),   # outside the image
                                 (1, 2, 3), (1,), 'rows', None])
def test_parse_box_refuses(box):
    with pytest.raises(ValueError):
        region.parse_box(box, PAD, (320, 88))


def test_unequal_paddings_are_refused():
    assert region.shared_padding([PAD, list(PAD), np.asarray(PAD)]) == PAD
    with pytest.raises(ValueError):
        region.shared_padding([PAD, (3, 2, 1, 2)])
