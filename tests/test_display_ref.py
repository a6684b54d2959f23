"""tests/display_ref.py, the numpy restatement of DESIGN.md section 26, against what it
must reduce to: image.to_display at the defaults, hand-picked bins, monotone curves,
and the fixed exposure case on the committed C1 image (no GPU needed)."""
import os

import numpy as np
import pytest

import display_ref as D
from pnraytracing_amd import image

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c1_oracle_image.npz")


@pytest.fixture(scope="module")
def c1():
    return np.load(GOLDEN)["image"]


def test_defaults_are_to_display_plus_alpha(c1):
    got = D.display_ref(c1)
    assert got.dtype == np.uint8 and got.shape == c1.shape
    assert np.array_equal(got[..., :3], image.to_display(c1))
    assert np.all(got[..., 3] == 255)
    # bottom_first only flips the rows
    assert np.array_equal(D.display_ref(c1, bottom_first=True), got[::-1])


def test_nan_negative_and_huge_inputs():
    img = np.zeros((1, 6, 4), F)
    img[0, :, 0] = [np.nan, -1.0, -0.0, np.inf, 1e30, 0.5]
    for tone in D.TONES:
        for transfer in D.TRANSFERS:
            q = D.display_ref(img, tone, transfer)[0, :, 0]
            assert list(q[:3]) == [0, 0, 0], (tone, transfer)
            assert list(q[3:5]) == [255, 255], (tone, transfer)
            assert 0 < q[5] < 255


def test_hand_picked_bins():
    y = np.array([1.0, 2.0 ** -16, 1e-30, 2.0 ** 16, 1e30, 0.0, -1.0, np.nan, np.inf, -np.inf, -0.0], F)
    counted, b = D.luma_bins(y)
    assert list(counted) == [True] * 5 + [False] * 6
    assert list(b[:5]) == [256, 0, 0, 511, 511]
    # 16 bins per octave: the bin's lower edge is 2^((b - 256) / 16) up to the mantissa's four bits
    for k in range(-16, 16):
        assert D.luma_bins(np.array([2.0 ** k], F))[1][0] == 256 + 16 * k
    assert D.luma_bins(np.array([1.0625, np.nextafter(F(1.0625), F(0))], F))[1].tolist() == [257, 256]
    # the histogram of an image counts what luma_bins counts
    img = np.zeros((1, len(y), 4), F)
    img[0, :, 1] = y / F(0.7152)
    h = D.histogram_ref(img)
    assert h["n_pixels"] == len(y) and h["n_counted"] == 5 == int(h["bins"].sum())


@pytest.mark.parametrize("transfer", D.TRANSFERS)
@pytest.mark.parametrize("tone", D.TONES)
def test_curves_are_monotone_and_map_zero_to_zero(tone, transfer):
    ramp = np.concatenate([np.linspace(0, 2, 4097), np.geomspace(2, 70000, 1024)]).astype(F)
    img = np.zeros((1, len(ramp), 4), F)
    img[0, :, :3] = ramp[:, None]
    q = D.display_ref(img, tone, transfer)[0, :, 0].astype(int)
    assert q[0] == 0 and q[-1] == 255
    assert np.all(np.diff(q) >= 0)
    u = D.transfer_curve(np.minimum(D.tone_curve(ramp, tone), F(1)), transfer)
    assert u[0] == 0 and np.all(np.diff(u) >= 0) and u.max() <= 1


def test_fixed_exposure_case_on_c1(c1):
    h = D.histogram_ref(c1)
    assert (h["n_pixels"], h["n_counted"]) == (65536, 65209)
    assert D.exposure_mean_bin(h, 50, 950) == 227
    e = D.exposure_ref(h, 50, 950, 0.18)
    assert e.dtype == F and e == F(0.6322508)
    # shards' histograms add up to the whole
    parts = [D.histogram_ref(c1, rows=[y for y in range(256) if (y // 8) % 3 == s]) for s in range(3)]
    assert sum(p["n_pixels"] for p in parts) == h["n_pixels"]
    assert np.array_equal(sum(p["bins"] for p in parts), h["bins"])


def test_exposure_edge_cases():
    empty = {"n_pixels": 10, "n_counted": 0, "bins": np.zeros(D.LUMA_BINS, np.int64)}
    assert D.exposure_ref(empty) == F(1)

    def one(b, n=100):
        bins = np.zeros(D.LUMA_BINS, np.int64)
        bins[b] = n
        return {"n_pixels": n, "n_counted": n, "bins": bins}
    assert D.exposure_ref(one(256), key=1.0) == F(1)                 # luminance 1 stays
    assert D.exposure_ref(one(0), key=1.0) == F(2.0 ** 16)           # k = 256
    assert D.exposure_ref(one(511), key=1.0) == F(F(2.0 ** -16) * D.T16[1])   # k = -255: e = -16, j = 1
    assert D.exposure_ref(one(240), key=0.18) == F(F(0.18) * F(2))
