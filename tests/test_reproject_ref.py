"""Self-checks of tests/reproject_ref.py on the CPU: guide images
of two cameras from the oracle's closest hits, the accumulation and moments of the anchor
colours through the adaptive sequence (frame counts 2..5); and the replay table the GPU
tests compare the library's statistics with (no GPU needed)."""
import numpy as np
import pytest

import moments_ref as R
import reproject_common as C
import reproject_ref as RP
from guides_common import SHAPES, bits

F, U = np.float32, np.uint32
W, H = C.W, C.H

# The largest |colour_out - colour_in| of an identity reprojection over the three scenes
# and shapes, as measured on the restatement: 5.19e-6 (c3 at 67x45; colours up to 1).  The
# projection lands a few ulps off the pixel's integer coordinates (|a|, |b| <= 1.3e-5), so
# up to three more taps enter with weights of that size.  Asserted at four times that.
IDENTITY_MEASURED = 5.19e-6
IDENTITY_BOUND = 4 * IDENTITY_MEASURED


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", C.SCENES)
def test_identity(name, shape):
    w, h = shape
    acc, mom = C.state(name, w, h)
    out, mo, st, nv = C.replay(name, "identity", w, h)
    pa, na = C.oracle_guides(name, "identity", w, h)
    hit = pa[..., 3] == 1
    n = R.frames_of(mom)
    assert n.min() >= 2 and n.max() <= 5
    if (w, h) == (W, H):
        assert set(np.unique(n)) == {2, 3, 4, 5}
    # every hit pixel is reprojected, every miss zeroed
    assert (nv[hit] >= 1).all() and (nv[~hit] == -1).all()
    assert C.stats_tuple(st)[:3] == (int(hit.sum()), 0, int((~hit).sum()))
    assert not bits(out[~hit]).any() and not bits(mo[~hit]).any()
    # n' = min(n of the valid taps, cap)
    _, valid, _, index = RP.tap_table(acc, mom, pa, na, pa, na, C.camera_a(name, w, h), w, h)
    tap_n = np.where(valid, n.reshape(-1)[index], U(0xFFFFFFFF)).min(axis=-1)
    n1 = R.frames_of(mo)
    assert np.array_equal(n1[hit], np.minimum(tap_n, U(32))[hit])
    own = index == (np.arange(h * w).reshape(h, w))[..., None]
    assert (valid & own).any(axis=-1)[hit].all(), "the pixel's own tap is among the valid ones"
    assert (n1[hit] <= n[hit]).all()
    assert st["sum_frames"] == int(n1.astype(np.int64).sum()) and st["max_frames"] == int(n1.max())
    # the colour, within the measured bound
    diff = np.abs(out[..., :3].astype(np.float64) - acc[..., :3])[hit]
    worst = float(diff.max()) if diff.size else 0.0
    print(name, shape, "identity: max |colour difference|", worst, "valid taps", np.unique(nv, return_counts=True))
    assert worst <= IDENTITY_BOUND
    assert (out[hit][:, 3] == 1).all()


def test_identity_bound_is_the_measured_one():
    worst = 0.0
    for name in C.SCENES:
        for w, h in SHAPES:
            acc, _ = C.state(name, w, h)
            out, _, _, nv = C.replay(name, "identity", w, h)
            d = np.abs(out[..., :3].astype(np.float64) - acc[..., :3])[nv >= 0]
            worst = max(worst, float(d.max()) if d.size else 0.0)
    print("identity: max |colour difference| over all scenes and shapes:", worst)
    assert 0.5 * IDENTITY_MEASURED <= worst <= 1.01 * IDENTITY_MEASURED


@pytest.mark.parametrize("name", C.SCENES)
def test_zero_camera_disoccludes_every_hit(name):
    acc, mom = C.state(name, W, H)
    pa, na = C.oracle_guides(name, "identity", W, H)
    hit = pa[..., 3] == 1
    with np.errstate(all="raise"):                   # nothing raises, whatever the caller's error state
        out, mo, st = RP.reproject(acc, mom, pa, na, pa, na, np.zeros((4, 3), F), W, H)
    assert C.stats_tuple(st) == (0, int(hit.sum()), int((~hit).sum()), 0, 0)
    assert not bits(out).any() and not bits(mo).any()


@pytest.mark.parametrize("move", ["identity", "rotate"])
def test_max_history_caps_the_count(move):
    acc, mom = C.state("c3", W, H)
    free = C.replay("c3", move)
    capped = C.replay("c3", move, params=(("max_history", 3),))
    n_free, n_cap = R.frames_of(free[1]), R.frames_of(capped[1])
    assert (n_free > 3).sum() >= 30 and n_free.max() == 5
    assert np.array_equal(n_cap, np.minimum(n_free, U(3))) and capped[2]["max_frames"] == 3
    assert capped[2]["sum_frames"] == int(n_cap.astype(np.int64).sum()) < free[2]["sum_frames"]
    # the colour and the mean do not depend on the cap; M2 is the same variance at the capped count
    assert np.array_equal(bits(capped[0]), bits(free[0]))
    assert np.array_equal(bits(capped[1][..., 0]), bits(free[1][..., 0]))
    k = n_free > 3
    var_free = free[1][..., 1][k] / (n_free[k] - 1).astype(F)
    var_cap = capped[1][..., 1][k] / F(2)
    assert np.allclose(var_cap, var_free, rtol=1e-6, atol=0)
    assert C.stats_tuple(capped[2])[:3] == C.stats_tuple(free[2])[:3]


def test_parameters_reject_taps():
    base = C.replay("c3", "translate")[2]
    strict = C.replay("c3", "translate", params=(("position_tolerance", 0.002),))[2]
    loose = C.replay("c3", "translate", params=(("normal_min", -1.0), ("position_tolerance", 0.5)))[2]
    assert strict["n_reprojected"] < base["n_reprojected"] < loose["n_reprojected"]
    for st in (base, strict, loose):
        assert st["n_reprojected"] + st["n_disoccluded"] + st["n_missed"] == W * H


# ---- the replay table ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,move", sorted(C.REPLAY))
def test_replay_table(name, move):
    st = C.replay(name, move)[2]
    print(name, move, C.stats_tuple(st))
    assert C.stats_tuple(st) == C.REPLAY[(name, move)]
    assert st["n_reprojected"] + st["n_disoccluded"] + st["n_missed"] == st["n_pixels"] == W * H
    if move == "away":
        assert st["n_reprojected"] == 0 and st["n_disoccluded"] > 0


def test_replay_covers_every_class():
    """From the replay, not from the GPU: an input for which this fails is a test error."""
    assert sorted(C.REPLAY) == sorted((n, m) for n in C.SCENES for m in C.MOVES)
    four = some = none = missed = 0
    for name in C.SCENES:
        for move in ("rotate", "translate", "zoom"):
            nv = C.replay(name, move)[3]
            four += int((nv == 4).sum())
            some += int(((nv >= 1) & (nv <= 3)).sum())
            none += int((nv == 0).sum())
            if name == "c2wide":
                missed += int((nv == -1).sum())
    print("four valid taps", four, "one to three", some, "disoccluded", none, "missed (c2wide)", missed)
    assert min(four, some, none, missed) >= 30, (four, some, none, missed)
