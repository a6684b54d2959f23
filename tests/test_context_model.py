"""tests/context_model.py and tests/sequence_ops.py checked on the CPU: the model lands on
the recorded results of the suite's hand-written sequences, every edit the generated
sequences make is visible in the next frame (so a stale cache cannot hide), the committed
seeds cover what they are meant to cover, and the generator is deterministic."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import place_ref as P
import refit_common as C
import refit_ref as RF
import reproject_common as RC
import sequence_ops as Q
import test_gpu_place as GP
import test_gpu_refit as GR
from context_model import ModelTracer
from guides_common import bits
from pnraytracing_amd import host as H

EDITS = ("materials", "vertices", "place", "environment", "texture", "camera", "resize", "depth")
PRIMARY_EDITS = ("materials", "vertices", "place", "environment", "camera")      # what a kept primary record would carry


def same(got, want, what):
    d = Q.difference(np.asarray(got), np.asarray(want))
    assert d is None, f"{what}: {d}"


# ---- 1 the hand-written sequences ----------------------------------------------------------------
def adaptive_state(name, w, h):
    """reproject_common.run_state on the model."""
    m = ModelTracer()
    RC.run_state(m, name, w, h)
    return m


@pytest.mark.parametrize("shape", [(RC.W, RC.H), (8, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", RC.SCENES)
def test_adaptive_replay_state(name, shape):
    m = adaptive_state(name, *shape)
    acc, mom = RC.state(name, *shape)
    same(m.read_accum(), acc, "accumulation")
    same(m.read_moments(), mom, "moments")


@pytest.mark.parametrize("name", RC.SCENES)
def test_reproject_replay_and_recorded_statistics(name):
    start = adaptive_state(name, RC.W, RC.H)
    for move in RC.MOVES:
        m = copy.deepcopy(start)
        m.set_frame(RC.W, RC.H, RC.camera_b(name, move, RC.W, RC.H), 4)
        st = m.reproject(RC.camera_a(name, RC.W, RC.H))
        acc, mom, ref_st, _ = RC.replay(name, move)
        assert RC.stats_tuple(st) == RC.stats_tuple(ref_st) == RC.REPLAY[(name, move)], (name, move)
        same(m.read_accum(), acc, f"{move}: accumulation")
        same(m.read_moments(), mom, f"{move}: moments")
        m.denoise()                          # the guide images are the new camera's on return
        g = m.read_aov("position")
        same(g, RC.oracle_guides(name, move, RC.W, RC.H)[0], f"{move}: position guide")


@pytest.mark.parametrize("how", ["update_vertices", "place_models"])
@pytest.mark.parametrize("name", ["C1", "C2", "C4"])
def test_refit_and_place_sequences(name, how):
    """tests/test_gpu_refit.py's and test_gpu_place.py's sequence: two still frames, the edit, the depth-1
    redraw, three still frames -- against the oracle of host.refit_packed's scene, refit_ref and place_ref."""
    cfg = C.scene(name)
    first, rec = C.edit(name)
    new = GR.edited(cfg, first, rec).packed
    redraw, final = GR.oracle_sequence(name)
    cam = GR.camera(name).uniforms()
    m = ModelTracer()
    m.load(cfg)
    m.set_frame(C.W, C.Hh, cam, 4)
    if how == "place_models":
        _, mesh, own, matrix = GP.model(name)
        mid = m.define_model(first, H.model_records(mesh))
    for f in range(2):
        m.render(f, 1)
    if how == "update_vertices":
        m.update_vertices(first, rec, *((new.lights, new.lights_sum_area) if name == "C1" else ()))
    else:
        m.place_models([(mid, matrix)], relight=name == "C1")
        same(m.read_vertices(first, len(rec)), P.place_ref(H.model_records(mesh), matrix), "records vs place_ref")
    same(m.read_vertices(first, len(rec)), P.words8(rec), "records vs host.model_vertices")
    m.set_frame(C.W, C.Hh, cam, 1)
    m.render(0, 1)
    same(m.read_accum(), redraw, "the redraw frame")
    m.set_frame(C.W, C.Hh, cam, 4)
    for f in range(3):
        m.render(f, 1)
    same(m.read_accum(), final, "the still frames after the edit")
    boxes = m.read_bvh_boxes(cfg.packed.nodes)
    same(boxes, new.nodes, "boxes vs pnrt_bvh_refit_cpu")
    same(boxes, RF.refit_ref(new.vertices, new.triangles, cfg.packed.nodes), "boxes vs refit_ref")


# ---- 2 every edit is visible -----------------------------------------------------------------------
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_every_edit_is_visible(seed):
    """The next frame with and without each edit, same frame number, oracle only: at least 5 % of the pixels
    differ, and for the edits a primary record would carry the first-hit image differs as well."""
    w = Q.world_of(seed)
    m = ModelTracer()
    w.start(m, Q.starts_with_moments(seed))
    n_edits = 0
    for k, op in enumerate(Q.sequence(seed)):
        without = copy.deepcopy(m) if op.role in EDITS else None
        Q.apply(op, m, w, [])
        if without is None:
            continue
        n_edits += 1
        what = f"seed {seed} op {k} {op!r}"
        if op.role == "resize":
            assert (m.width, m.height) != (without.width, without.height), what
            continue
        a, b = m.colors(5, 1)[0], without.colors(5, 1)[0]
        differ = np.any(bits(a) != bits(b), axis=-1)
        assert differ.mean() >= 0.05, f"{what}: {differ.sum()} of {differ.size} pixels differ"
        if op.role in PRIMARY_EDITS:
            first = np.any(m.first_hit_image() != without.first_hit_image(), axis=-1)
            assert first.any(), f"{what}: the first-hit image does not change"
            # ... and where it changes, the frame does
            assert (first & differ.reshape(-1)).any(), f"{what}: no pixel whose first hit changed changes colour"
    assert n_edits >= 3


# ---- 3 coverage of the committed seeds ---------------------------------------------------------------
def refused(r):
    return isinstance(r, tuple) and len(r) == 2 and r[0] == "refused"


def test_coverage_of_the_committed_seeds():
    assert 12 <= len(Q.SEEDS) <= 16
    kinds, pairs, lent, stale = {}, set(), 0, set()
    sizes, lamps = set(), 0
    for seed in Q.SEEDS:
        ops = Q.sequence(seed)
        run, _ = Q.model_run(seed)
        assert 30 <= len(ops) <= 50
        lamps += len(Q.world_of(seed).cfg.packed.lights) > 8
        cp = Q.checkpoints(seed, len(ops))
        gaps = np.diff((-1,) + cp)
        assert cp[-1] == len(ops) - 1 and all(8 <= g <= 12 for g in gaps[:-1]) and 1 <= gaps[-1] <= 12
        for k, op in enumerate(ops):
            kinds[op.kind] = kinds.get(op.kind, 0) + 1
            if op.kind in ("render", "render_shards", "render_rays"):
                assert 1 <= op.args[1] <= 4
            if op.kind == "resize":
                sizes.add(op.args[0])
            if op.role in Q.INVALIDATORS and not refused(run[k][0]):
                for j in range(k + 1, len(ops)):
                    if ops[j].role in Q.CONSUMERS and not refused(run[j][0]):
                        pairs.add((op.role, ops[j].role))
                    if ops[j].kind in Q.READ_BACKS:
                        break
            if op.kind == "render_guides" and k and ops[k - 1].kind == "render" and not refused(run[k - 1][0]):
                lent += 1                    # (a whole-image render of the camera still set: its records are lent)
            if op.role == "denoise" and refused(run[k][0]) and k >= 2 and ops[k - 1].role in Q.INVALIDATORS \
                    and ops[k - 2].kind == "render_guides":
                stale.add(ops[k - 1].role)
    rare = {k: n for k, n in kinds.items() if n < 3}
    assert not rare, f"op kinds that occur fewer than three times: {rare}"
    assert set(Q.FILLERS) <= set(kinds) and set(Q.COUNTS_AS) <= set(kinds)
    missing = [(i, c) for i in Q.INVALIDATORS for c in Q.CONSUMERS if (i, c) not in pairs]
    assert not missing, f"(invalidator, consumer) pairs without a read-back in between that never occur: {missing}"
    assert lent >= 2
    assert len(stale) >= 3, stale
    assert sizes == {0, 1, 2} and lamps >= 1


def test_the_model_refuses_what_the_contract_refuses():
    """The refusals the sequences meet, by kind: each at least once over the committed seeds."""
    seen = set()
    for seed in Q.SEEDS:
        for op, (r, _) in zip(Q.sequence(seed), Q.model_run(seed)[0]):
            if refused(r):
                assert r[1] == -3
                seen.add(op.kind)
    assert {"denoise", "render", "render_adaptive", "render_rays"} <= seen, seen


# ---- 4 determinism ---------------------------------------------------------------------------------
def test_the_generator_is_deterministic_across_processes():
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import sequence_ops as Q; "
            "print(repr([Q.sequence(s) for s in Q.SEEDS]))") % (here, os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle"))
    out = [subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True,
                          env=dict(os.environ, PYTHONHASHSEED=str(k))).stdout.strip() for k in (1, 2)]
    assert out[0] == out[1] == repr([Q.sequence(s) for s in Q.SEEDS])
