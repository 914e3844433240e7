"""tests/pixel_ref.py against a scalar restatement of code8 (vcm_ts_amd/csrc/roi_common.h): (int) rintf(255.0f * v) after
fminf(fmaxf(v, 0), 1).  The scalar form takes the float32 product from float64 -- 255 * v has at most 32 significant bits,
so the float64 product is exact and the cast to float32 rounds once, as the device's multiply does -- and Python's round()
is round-half-to-even, as rintf is."""
import math

import numpy as np

from tests import pixel_ref as P

F32 = np.float32


def scalar_code(v):
    v = float(F32(v))
    if math.isnan(v) or v < 0.0:  # fmaxf(NaN, 0) is 0
        v = 0.0
    v = min(v, 1.0)
    return int(round(float(F32(255.0 * v))))


def test_code_on_the_exact_codes_and_around_every_midpoint():
    exact = np.arange(256, dtype=F32) / F32(255.0)
    assert np.array_equal(P.code(exact), np.arange(256)) and P.code(exact).dtype == np.int64
    assert [scalar_code(v) for v in exact] == list(range(256))
    mid = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(F32)
    below, above = np.nextafter(mid, F32(-1)), np.nextafter(mid, F32(2))
    for values in (mid, below, above):
        assert values.dtype == F32 and P.code(values).tolist() == [scalar_code(v) for v in values]
    # monotone across every midpoint, between the two neighbouring codes; where the float32 product is exactly k + 0.5
    # (one ulp of v is less than one of 255 v near the top) the even code wins
    k = np.arange(255)
    assert (k <= P.code(below)).all() and (P.code(below) <= P.code(mid)).all() and (P.code(mid) <= P.code(above)).all()
    assert (P.code(above) <= k + 1).all() and (P.code(above) - P.code(below)).sum() >= 250
    ties = [v for v in np.concatenate([mid, below, above]) if float(F32(255.0 * float(v))) % 1.0 == 0.5]
    assert ties and all(P.code(v) % 2 == 0 for v in ties)


def test_code_outside_the_range_and_of_a_nan():
    inf, nan = F32(np.inf), F32(np.nan)
    values = np.array([-0.0, -1e-30, -1.0, -3e38, -inf, nan, 1.0, 1.0 + 2.0 ** -23, 2.0, 3e38, inf], dtype=F32)
    want = [0, 0, 0, 0, 0, 0, 255, 255, 255, 255, 255]
    assert P.code(values).tolist() == want == [scalar_code(v) for v in values]
    assert P.code(values.reshape(1, 11)).shape == (1, 11) and int(P.code(F32(0.5))) == 128  # 127.5: the even neighbour


def test_luma_and_grid():
    pic = np.array([0.0, 1.0, 0.5, 0.25], dtype=F32).reshape(1, 2, 2).repeat(3, axis=0)
    k = P.code(pic[0])
    assert np.array_equal(P.luma(pic), k) and np.array_equal(P.luma_of_codes(k, k, k), k)  # 54 + 183 + 19 == 256
    assert int(P.luma_of_codes(255, 0, 0)) == 54 and int(P.luma_of_codes(0, 255, 0)) == 182 and int(P.luma_of_codes(0, 0, 255)) == 19
    assert P.grid(1, 1) == (4, 4) and P.grid(64, 65) == (4, 8) and P.grid(1080, 1920) == (68, 120)
