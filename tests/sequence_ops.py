"""TEST INFRASTRUCTURE shared by tests/test_context_model.py and tests/test_gpu_sequences.py:
the one scene of the call-sequence tests, the seeded generator of call sequences, and
``apply``, which runs one op on a ``PathTracer`` or on a ``context_model.ModelTracer``.

The scene is a Cornell box seen through a 100-degree lens (camera rays miss around the box
and show the environment), with an emissive panel in front of the back wall that every camera sees at every size,
and a textured, placeable ball of 384 triangles on the floor; the floor carries
the same texture, so that a texture upload changes more than the ball's pixels.  Every
fourth seed adds lamps_common's emissive soup: a light list of 14 entries.

An op is a kind and plain arguments -- indices into the palettes below, never arrays -- so
that a sequence prints the same in every process.  Every palette is chosen so that two
different entries give different pixels: an emission has a component below 1 (the colour
is clamped to [0, 1], and an emission of 60 looks like one of 20), the ball's poses and the
cameras move what is in view, the environments differ where the camera rays miss."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import lamps_common
from guides_common import camera_rays
from pnraytracing_amd import host as H
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import KERNEL_V1, TRAVERSE_EXACT, TRAVERSE_ZCULL, PnrtError

F = np.float32
SEEDS = tuple(range(14))
SIZES = ((40, 30), (33, 17), (8, 8))
CAMERAS = (((0, 2.8, 5.5), (0, 2.8, 0), 100.0), ((1.0, 3.3, 5.0), (0, 2.4, 0), 100.0), ((-1.2, 2.2, 4.8), (0.3, 2.9, 0), 90.0))
BALL_POSES = ([H.translate(0.2, 1.2, -0.3), H.scale(1.1)],
              [H.translate(-0.9, 1.4, 0.4), H.rotate(30.0, 0, 1, 0), H.scale(1.0)],
              [H.translate(0.8, 1.6, -0.8), H.rotate(-40.0, 1, 0, 0), H.scale(1.2, 0.9, 1.1)],
              [H.translate(0.0, 1.1, 0.8), H.scale(0.9)])
LIGHT_POSES = ([H.translate(0, 3.9, -2.7), H.rotate(90.0, 1, 0, 0), H.scale(0.05)],
               [H.translate(0.5, 3.7, -2.6), H.rotate(90.0, 1, 0, 0), H.scale(0.04)],
               [H.translate(-0.4, 4.0, -2.65), H.rotate(90.0, 1, 0, 0), H.scale(0.055)])
EMISSIONS = ((60.0, 60.0, 60.0), (0.9, 30.0, 0.4), (20.0, 0.5, 0.7), (0.3, 0.6, 45.0))
CEILINGS = ((0.73, 0.73, 0.73), (0.2, 0.5, 0.8), (0.8, 0.3, 0.2))
MODES = (TRAVERSE_ZCULL, TRAVERSE_EXACT)
CEILING_MATERIAL, LIGHT_MATERIAL = 5, 6
N_LAMPS = 12

INVALIDATORS = ("materials", "vertices", "place", "environment", "texture", "camera", "resize", "mode", "depth")
CONSUMERS = ("render", "render_rays", "render_adaptive", "render_guides", "denoise", "reproject", "query_rays")
READ_BACKS = ("read_aov", "read_denoised", "read_display", "luma_histogram", "convergence", "read_error", "read_moments",
              "query_rays", "read_vertices", "read_bvh_boxes")
# kind -> the invalidator / consumer it counts as
COUNTS_AS = {"vertices_lights": "vertices", "place_relight": "place", "environment_build": "environment",
             "render_shards": "render", "render_rays_adaptive": "render_adaptive", "denoise_variance": "denoise"}


@dataclasses.dataclass(frozen=True)
class Op:
    kind: str
    args: tuple = ()

    def __repr__(self):
        return f"{self.kind}{self.args!r}"

    @property
    def role(self):
        return COUNTS_AS.get(self.kind, self.kind)


class World:
    """The scene and everything an op's indices stand for."""

    def __init__(self, lamps: bool):
        wall = H.Material(baseColor=(0.65, 0.65, 0.65))
        self.ball = H.mesh_displaced_sphere(16, 12, 1.0, (0.0, 0.0, 0.0), 0.08, 0xC0FFEE)
        self.quad = H.mesh_quad(27.5)
        sb = H.SceneBuilder()
        sb.add_model(self.ball, BALL_POSES[0], H.Material(baseColor=(0.8, 0.8, 0.8), roughness=0.4, specular=0.5), "ball",
                     texture_ids=[0])
        q = self.quad
        sb.add_model(q, [H.scale(0.1)], wall, "floor", texture_ids=[0])
        sb.add_model(q, [H.translate(0, 2.75, -2.75), H.rotate(90.0, 1, 0, 0), H.scale(0.1)], wall, "front_wall")
        sb.add_model(q, [H.translate(2.75, 2.75, 0), H.rotate(90.0, 0, 0, 1), H.scale(0.1)], wall.copy(baseColor=(0.12, 0.45, 0.15)),
                     "right_wall")
        sb.add_model(q, [H.translate(-2.75, 2.75, 0.0), H.rotate(-90.0, 0, 0, 1), H.scale(0.1)],
                     wall.copy(baseColor=(0.65, 0.05, 0.05)), "left_wall")
        sb.add_model(q, [H.translate(0, 5.54, 0), H.rotate(180.0, 0, 0, 1), H.scale(0.1)], wall.copy(baseColor=CEILINGS[0]), "ceiling")
        sb.add_model(q, LIGHT_POSES[0], wall.copy(baseColor=CEILINGS[0], emssive=EMISSIONS[0]), "light")
        if lamps:
            sb.add_model(lamps_common.soup(N_LAMPS, 1, (0, 3, 0)), [H.scale(1.0)], lamps_common.LAMP, "lamps")
        packed = sb.build()
        self.ball_first, self.n_ball = 0, len(self.ball.positions)
        self.light_first = self.n_ball + 5 * 6
        assert len(packed.lights) == 2 + (N_LAMPS if lamps else 0)
        self.textures = [S.checker_texture(37, 19, 3, 7), S.checker_texture(24, 24, 3, 11), S.checker_texture(50, 13, 3, 5)]
        self.textures[1] = (255 - self.textures[1][0],) + self.textures[1][1:]
        envs = [H.synthetic_hdr(64, 32, s) for s in (1, 2, 3)]
        envs[1] = np.ascontiguousarray(envs[1][::-1, ::-1] * F(0.5))
        self.envs = [None, (envs[0], H.hdr_table(envs[0])), (envs[1], H.hdr_table(envs[1]))]
        self.env_build = np.ascontiguousarray(np.roll(envs[2], 17, axis=1))
        w, h = SIZES[0]
        self.cfg = S.SceneConfig("sequences" + ("+lamps" if lamps else ""), packed, self.camera(0, w, h), w, h, 1, max_depth=4,
                                 env_rgb=self.envs[1][0], env_table=self.envs[1][1], textures=[self.textures[0]])
        self.materials = packed.materials.copy()

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def camera(idx: int, w: int, h: int):
        eye, center, fov = CAMERAS[idx]
        cam = H.camera_update(eye, center, (0, 1, 0), fov, F(w) / F(h))
        cam.setflags(write=False)
        return cam

    @functools.lru_cache(maxsize=None)
    def ball_records(self, pose: int):
        return H.model_vertices(self.ball, BALL_POSES[pose])

    @functools.lru_cache(maxsize=None)
    def light_edit(self, pose: int):
        """(records, lights) of the light quad under LIGHT_POSES[pose]: the list's areas depend on no other edit."""
        rec = H.model_vertices(self.quad, LIGHT_POSES[pose])
        return rec, H.refit_packed(self.cfg.packed, self.light_first, rec).lights

    def material_records(self, emission: int, ceiling: int):
        rec = self.materials[CEILING_MATERIAL:LIGHT_MATERIAL + 1].copy()
        rec[0, 3:6] = CEILINGS[ceiling]
        rec[1, 0:3] = EMISSIONS[emission]
        return rec

    def start(self, t, moments: bool):
        """Every sequence starts here: the scene, the two models, and the moments for the seeds that use them."""
        t.load(self.cfg)
        assert t.define_model(self.ball_first, H.model_records(self.ball)) == 0
        assert t.define_model(self.light_first, H.model_records(self.quad)) == 1
        if moments:
            t.enable_moments(True)


@functools.lru_cache(maxsize=None)
def world(lamps: bool) -> World:
    return World(lamps)


def world_of(seed: int) -> World:
    return world(seed % 4 == 3)


def apply(op: Op, t, w: World, keep: list):
    """Run `op` on `t`; -> what the call returns (None for most), or ("refused", code).  `keep` holds what must
    outlive the call (ray buffers in flight)."""
    k, a = op.kind, op.args
    try:
        if k in ("render", "render_shards"):
            return t.render(*a)
        if k == "render_rays":
            rays = t.make_rays("pinhole", w.camera(a[2], t.width, t.height))
            keep.append(rays)
            return t.render_rays(a[0], a[1], rays, 0)
        if k == "render_adaptive":
            return t.render_adaptive(*a)
        if k == "render_rays_adaptive":
            rays = t.make_rays("pinhole", w.camera(a[2], t.width, t.height))
            keep.append(rays)
            return t.render_rays_adaptive(a[0], a[1], rays, 0, a[3], a[4])
        if k == "materials":
            return t.update_materials(CEILING_MATERIAL, w.material_records(*a))
        if k == "vertices":
            return t.update_vertices(w.ball_first, w.ball_records(a[0]))
        if k == "vertices_lights":
            rec, lights = w.light_edit(a[0])
            return t.update_vertices(w.light_first, rec, lights)
        if k == "place":
            return t.place_models([(0, H.model_matrix(BALL_POSES[a[0]]))])
        if k == "place_relight":
            return t.place_models([(1, H.model_matrix(LIGHT_POSES[a[0]]))], relight=True)
        if k == "environment":
            return t.upload_env(*(w.envs[a[0]] or (None, None)))
        if k == "environment_build":
            return t.upload_env_build(w.env_build)
        if k == "texture":
            return t.upload_texture(0, *w.textures[a[0]])
        if k in ("mode", "v1"):
            return t.set_options(a[0])
        if k in ("camera", "resize", "depth"):
            size, cam, depth = a
            return t.set_frame(*SIZES[size], w.camera(cam, *SIZES[size]), depth)
        if k == "reset_accum":
            return t.reset_accum()
        if k == "enable_moments":
            return t.enable_moments(a[0])
        if k == "reproject":
            return t.reproject(w.camera(a[0], t.width, t.height))
        if k == "render_guides":
            return t.render_guides()
        if k == "read_aov":
            return t.read_aov(a[0])
        if k == "denoise":
            return t.denoise(levels=a[0])
        if k == "denoise_variance":
            return t.denoise_variance(levels=a[0])
        if k == "display":
            return t.display(source=a[0], tone=a[1], transfer=a[2], exposure=a[3], bottom_first=a[4])
        if k == "luma_histogram":
            return t.luma_histogram(a[0], *a[1:])
        if k == "convergence":
            return t.convergence(*a)
        if k == "query_rays":
            cfg = dataclasses.replace(w.cfg, camera=w.camera(a[1], t.width, t.height), width=t.width, height=t.height)
            return t.query_rays(camera_rays(cfg), any_hit=a[0])[:, :13]
        if k == "read_vertices":
            return t.read_vertices(0, len(w.cfg.packed.vertices))
        if k == "read_bvh_boxes":
            return t.read_bvh_boxes(w.cfg.packed.nodes)
        return getattr(t, k)(*a)             # read_denoised, read_display, read_error, read_moments
    except PnrtError as e:
        if getattr(e, "code", None) not in (-1, -3):     # PNRT_E_ARG, PNRT_E_STATE; a HIP or trace error is no refusal
            raise
        return ("refused", e.code)


# ---- the generator ------------------------------------------------------------------------------
PAIRS = tuple((i, c) for c in CONSUMERS for i in INVALIDATORS)
FILLERS = ("display", "read_display", "luma_histogram", "convergence", "read_error", "read_moments", "read_aov", "read_denoised",
           "read_vertices", "read_bvh_boxes", "denoise_variance", "render_rays_adaptive", "render_shards", "reset_accum",
           "enable_moments", "v1", "environment_build", "vertices_lights", "place_relight", "query_rays", "render_guides",
           "denoise", "render_rays", "reproject", "texture", "materials", "resize", "depth")


class _Gen:
    def __init__(self, seed: int):
        self.rng = np.random.default_rng(seed)
        self.seed = seed
        self.ops = []
        self.size = self.cam = 0
        self.depth = 4
        self.mode, self.v1 = TRAVERSE_ZCULL, False
        self.moments = starts_with_moments(seed)
        self.ever, self.cover = self.moments, self.moments
        self.ball = self.light = self.emission = self.ceiling = self.texture = 0
        self.env = 1
        self.frame = 0

    def pick(self, n: int, other_than=None) -> int:
        choices = [k for k in range(n) if k != other_than]
        return int(choices[int(self.rng.integers(len(choices)))])

    def emit(self, kind, *args):
        self.ops.append(Op(kind, tuple(args)))

    # -- state the consumers need
    def want_wavefront(self):
        if self.v1:
            self.v1 = False
            self.emit("v1", self.mode)

    def want_moments(self):
        self.want_wavefront()
        if not self.moments:
            self.moments = self.ever = True
            self.emit("enable_moments", True)
        if not self.cover:
            self.emit("reset_accum")
            self.cover, self.frame = True, 0
        if self.frame == 0:
            self.render(2)

    def render(self, n=None, kind="render"):
        n = int(self.rng.integers(1, 5)) if n is None else n
        if self.v1 and self.moments and kind != "render":
            self.want_wavefront()
        if kind == "render":
            self.emit("render", self.frame, n)
        elif kind == "render_shards":
            for shard in (1, 0):
                self.emit("render_shards", self.frame, n, 4, 2, shard)
        elif kind == "render_rays":
            self.want_wavefront()
            self.emit("render_rays", self.frame, n, self.cam)
        if not (self.v1 and self.moments):   # (refused: nothing rendered)
            if not self.moments:
                self.cover = False
            self.frame += n

    def after_edit(self):
        """Frame numbers after an edit: mostly continue, sometimes a redraw, sometimes frame 0 over the old image."""
        r = int(self.rng.integers(6))
        if r == 0:
            self.emit("reset_accum")
            self.frame = 0
            self.cover = self.cover or self.ever
        elif r == 1:
            self.frame = 0

    # -- the invalidators
    def invalidate(self, what: str):
        if self.depth == 0 and what != "depth":      # at depth 0 a frame shows emission and environment only
            self.invalidate("depth")
        if what == "materials":
            self.emission, self.ceiling = self.pick(len(EMISSIONS), self.emission), self.pick(len(CEILINGS))
            self.emit("materials", self.emission, self.ceiling)
        elif what == "vertices":
            self.ball = self.pick(len(BALL_POSES), self.ball)
            self.emit("vertices", self.ball)
        elif what == "vertices_lights":
            self.light = self.pick(len(LIGHT_POSES), self.light)
            self.emit("vertices_lights", self.light)
        elif what == "place":
            self.ball = self.pick(len(BALL_POSES), self.ball)
            self.emit("place", self.ball)
        elif what == "place_relight":
            self.light = self.pick(len(LIGHT_POSES), self.light)
            self.emit("place_relight", self.light)
        elif what == "environment":
            self.env = self.pick(3, self.env)
            self.emit("environment", self.env)
        elif what == "environment_build":
            if self.env == 3:
                self.invalidate("environment")
            self.env = 3
            self.emit("environment_build")
        elif what == "texture":
            self.texture = self.pick(3, self.texture)
            self.emit("texture", self.texture)
        elif what == "camera":
            self.cam = self.pick(len(CAMERAS), self.cam)
            self.emit("camera", self.size, self.cam, self.depth)
        elif what == "depth":
            self.depth = self.pick(5, self.depth)
            self.emit("depth", self.size, self.cam, self.depth)
        elif what == "resize":
            self.size = self.pick(len(SIZES), self.size)
            self.emit("resize", self.size, self.cam, self.depth)
            self.frame = 0 if self.rng.integers(4) else self.frame     # a zeroed image: mostly from frame 0
            self.cover = self.cover or self.ever
        elif what == "mode":
            self.mode = MODES[1 - MODES.index(self.mode)]
            self.emit("mode", self.mode | (KERNEL_V1 if self.v1 else 0))
        else:
            raise KeyError(what)

    # -- the consumers
    def consume(self, what: str, inv: str, cam_before: int):
        if what in ("render", "render_rays"):
            if inv != "resize":
                self.after_edit()
            self.render(kind=what)
        elif what == "render_adaptive":
            if self.frame == 0:
                self.frame = 1               # (the image may be zeroed: every pixel is unmeasured and takes the frame whole)
            n = int(self.rng.integers(1, 4))
            self.emit("render_adaptive", self.frame, n, (0.05, 0.3, 0.0)[int(self.rng.integers(3))], int(self.rng.integers(2, 6)))
            self.frame += n
        elif what == "render_guides":
            self.emit("render_guides")
        elif what == "denoise":
            self.emit("denoise", int(self.rng.integers(1, 6)))       # refused: the guides are stale (not after "depth")
            self.emit("render_guides")
            self.emit("denoise", int(self.rng.integers(1, 6)))
        elif what == "reproject":
            self.emit("reproject", cam_before)
        elif what == "query_rays":
            self.emit("query_rays", bool(self.rng.integers(2)), self.cam)

    def pair(self, inv: str, con: str):
        if con in ("render_adaptive", "reproject"):
            self.want_moments()
        if con in ("render_rays",):
            self.want_wavefront()
        if con == "denoise":
            self.emit("render_guides")
        cam_before = self.cam
        self.invalidate(inv)
        self.consume(con, inv, cam_before)

    def filler(self, kind: str):
        r = self.rng
        if kind == "display":
            self.emit("display", ("accum", "denoised")[int(r.integers(2))], ("clamp", "reinhard", "aces")[int(r.integers(3))],
                      ("linear", "srgb")[int(r.integers(2))], (1.0, 0.5, 2.5)[int(r.integers(3))], bool(r.integers(2)))
        elif kind == "luma_histogram":
            self.emit("luma_histogram", ("accum", "denoised")[int(r.integers(2))], 3, 2, int(r.integers(2)))
        elif kind == "convergence":
            self.emit("convergence", 0.1, 2, 3, int(r.integers(3)))
        elif kind == "read_aov":
            self.emit("read_aov", ("position", "normal", "albedo")[int(r.integers(3))])
        elif kind in ("read_display", "read_error", "read_moments", "read_denoised", "read_vertices", "read_bvh_boxes", "render_guides"):
            self.emit(kind)
        elif kind in ("denoise", "denoise_variance"):
            self.emit(kind, int(r.integers(1, 6)))
        elif kind == "render_rays_adaptive":
            self.want_moments()
            n = int(r.integers(1, 4))
            self.emit("render_rays_adaptive", max(self.frame, 1), n, self.cam, 0.0, 0xFFFFFFFF)
            self.frame = max(self.frame, 1) + n
        elif kind in ("render_shards", "render_rays"):
            self.render(kind=kind)
        elif kind == "reset_accum":
            self.emit("reset_accum")
            self.frame = 0
            self.cover = self.cover or self.ever
        elif kind == "enable_moments":
            self.moments = not self.moments
            if self.moments and not self.ever:
                self.ever = self.cover = True
            self.emit("enable_moments", self.moments)
            self.render()
        elif kind == "v1":                   # the one-kernel path: a render (refused while the moments are on), the two
            self.v1 = True                   # refusals, and back
            self.emit("v1", self.mode | KERNEL_V1)
            self.render()
            self.emit("render_adaptive", max(self.frame, 1), 1, 0.1, 2)
            self.emit("render_rays", self.frame, 1, self.cam)
            self.want_wavefront()
        elif kind == "query_rays":
            self.emit("query_rays", bool(r.integers(2)), self.cam)
        elif kind == "reproject":
            self.want_moments()
            cam_before = self.cam
            self.invalidate("camera")
            self.emit("reproject", cam_before)
        else:
            self.invalidate(kind)
            self.render()


@functools.lru_cache(maxsize=None)
def sequence(seed: int) -> tuple:
    """The op list of a seed: 30 to 50 ops.  Steered: the (invalidator, consumer) pairs are dealt out over
    SEEDS, each seed renders guides straight after a render once, and the filler kinds rotate with the seed."""
    g = _Gen(seed)
    g.render(2)
    g.emit("render_guides")                  # straight after a render of the same camera: lent records ...
    g.render(1)                              # ... with the pipe's next call queued behind them
    pairs = [p for k, p in enumerate(PAIRS) if k % len(SEEDS) == seed % len(SEEDS)]
    order = g.rng.permutation(len(pairs))
    at = (seed * 5) % len(FILLERS)
    for k in order:
        g.pair(*pairs[int(k)])
        for _ in range(2):
            if len(g.ops) < 44:
                g.filler(FILLERS[at % len(FILLERS)])
                at += 1
    while len(g.ops) < 30:
        g.filler(FILLERS[at % len(FILLERS)])
        at += 1
    assert 30 <= len(g.ops) <= 50, (seed, len(g.ops))
    return tuple(g.ops)


def starts_with_moments(seed: int) -> bool:
    """Every third seed starts without the moments."""
    return seed % 3 != 2


def checkpoints(seed: int, n_ops: int) -> tuple:
    """The op indices after which the pipelined variant reads the images back: every 8 to 12 ops, and the last."""
    step = 8 + seed % 5
    return tuple(sorted(set(range(step - 1, n_ops, step)) | {n_ops - 1}))


# ---- what a checkpoint compares --------------------------------------------------------------------
def readable(model) -> tuple:
    """The names of the images the model says a context can hand out now."""
    names = ["accum"]
    if model.moments_ever:
        names.append("moments")
    if model.guides is not None and model.guides["position"].shape[:2] == (model.height, model.width):
        names += ["position", "normal", "albedo"]
    for name, img in (("denoised", model.denoised), ("display", model.disp)):
        if img is not None and img.shape[:2] == (model.height, model.width):
            names.append(name)
    return tuple(names)


READERS = {"accum": "read_accum", "moments": "read_moments", "denoised": "read_denoised", "display": "read_display"}


def snapshot(t, names) -> dict:
    """The images `names` of a PathTracer or a ModelTracer."""
    return {n: getattr(t, READERS[n])() if n in READERS else t.read_aov(n) for n in names}


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def difference(got, want):
    """None when equal, else a description: results are None, ("refused", code), dicts or arrays."""
    if isinstance(want, dict) and isinstance(got, dict):
        for key in want:
            if key not in got:
                return f"no field {key}"
            d = difference(got[key], want[key])
            if d:
                return f"{key}: {d}"
        return None
    if isinstance(want, np.ndarray) and isinstance(got, np.ndarray):
        if got.shape != want.shape:
            return f"shape {got.shape}, expected {want.shape}"
        bad = np.argwhere(words(got) != words(want))
        if len(bad):
            where = bad if bad.shape[1] < 3 else np.unique(bad[:, :2], axis=0)
            return f"{len(where)} differ, first (row, column ...) {where[:4].tolist()}"
        return None
    if isinstance(want, np.ndarray) or isinstance(got, np.ndarray) or got != want:
        return f"{got!r}, expected {want!r}"
    return None


@functools.lru_cache(maxsize=None)
def model_run(seed: int):
    """The model's replay of a seed, computed once: ([(what op k returned, the images after op k)], the model)."""
    from context_model import ModelTracer
    w = world_of(seed)
    m = ModelTracer()
    w.start(m, starts_with_moments(seed))
    out = []
    for op in sequence(seed):
        r = apply(op, m, w, [])
        out.append((r, snapshot(m, readable(m))))
    return tuple(out), m
