"""write_exr(..., layers=...) / read_exr_layers: the guide images and the denoised
preview as extra float channels of the accumulation image's EXR file."""
import numpy as np
import pytest

from pnraytracing_amd import image as I

F = np.float32


def _images(h=7, w=5, seed=3):
    rng = np.random.default_rng(seed)
    beauty = rng.random((h, w, 4)).astype(F)
    layers = {"albedo": rng.random((h, w, 4)).astype(F),
              "normal": rng.normal(0, 1, (h, w, 4)).astype(F),
              "position": (rng.normal(0, 100, (h, w, 4))).astype(F),
              "denoised": rng.random((h, w, 3)).astype(F)}
    layers["normal"][0, 0] = (np.float32("-0.0"), np.float32("inf"), 1e-45, -1.0)     # bits survive, not just values
    return beauty, layers


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_layers_round_trip_bit_for_bit(tmp_path):
    beauty, layers = _images()
    p = str(tmp_path / "a.exr")
    I.write_exr(p, beauty, layers=layers)
    got = I.read_exr_layers(p)
    assert sorted(got) == sorted(layers)
    for name, img in layers.items():
        assert got[name].shape == img.shape, name
        assert np.array_equal(_bits(got[name]), _bits(img)), name


def test_read_exr_of_a_layered_file_returns_the_beauty_image(tmp_path):
    beauty, layers = _images()
    p = str(tmp_path / "a.exr")
    I.write_exr(p, beauty, layers=layers)
    got = I.read_exr(p)
    assert got.shape == beauty.shape
    assert np.array_equal(_bits(got), _bits(beauty))


def test_default_call_writes_the_same_bytes(tmp_path):
    beauty, _ = _images()
    a, b, c = (str(tmp_path / n) for n in ("a.exr", "b.exr", "c.exr"))
    I.write_exr(a, beauty)
    I.write_exr(b, beauty, layers=None)
    I.write_exr(c, beauty, layers={})
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    assert I.read_exr_layers(a) == {}
    # the file without layers, byte for byte as the format lays it out: a 4-channel
    # chlist (A, B, G, R), one chunk of 8 + 4 * 4 * w bytes per scanline
    raw = open(a, "rb").read()
    h, w = beauty.shape[:2]
    assert raw.count(b"\0" + b"\x02\0\0\0" + b"\0\0\0\0" + b"\x01\0\0\0\x01\0\0\0") == 4
    assert raw.endswith(np.ascontiguousarray(beauty[0, :, 0], "<f4").tobytes())     # bottom row last, R last


def test_three_channel_beauty_with_layers(tmp_path):
    beauty, layers = _images()
    p = str(tmp_path / "a.exr")
    I.write_exr(p, beauty[..., :3], layers={"denoised": layers["denoised"]})
    assert np.array_equal(_bits(I.read_exr(p)), _bits(beauty[..., :3]))
    assert np.array_equal(_bits(I.read_exr_layers(p)["denoised"]), _bits(layers["denoised"]))


@pytest.mark.parametrize("name,img", [("a.b", np.zeros((7, 5, 3), F)), ("", np.zeros((7, 5, 3), F)),
                                      ("x" * 30, np.zeros((7, 5, 3), F)), ("ok", np.zeros((7, 6, 3), F)),
                                      ("ok", np.zeros((7, 5, 2), F))])
def test_bad_layers_are_refused(tmp_path, name, img):
    beauty, _ = _images()
    with pytest.raises(ValueError):
        I.write_exr(str(tmp_path / "a.exr"), beauty, layers={name: img})
