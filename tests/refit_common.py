"""TEST INFRASTRUCTURE shared by tests/test_refit_*.py and tests/test_gpu_refit*.py: the
three small scenes and the geometry edits made to them -- a model's vertex records under
a new matrix, through the host library's own ModelOutput code (host.model_vertices)."""
import functools

from pnraytracing_amd import host as H
from pnraytracing_amd import scenes as S

W, Hh = 48, 32


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "C1":
        return S.cornell_c1(W, Hh, spp=1)
    if name == "C2":
        return S.bunny_c2(W, Hh, spp=1, nu=24, nv=12, env=True)
    if name == "C4":
        return S.teapot_c4(W, Hh, spp=1)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def edit(name):
    """(first vertex, (n, 15) records): C2's bunny translated (its model is added first,
    main.cpp:207-208), C4's teapot rotated about y (added first), C1's ceiling light (added
    last) scaled up and lowered -- its two triangles change area."""
    if name == "C2":
        mesh = H.mesh_displaced_sphere(24, 12, S.BUNNY_RADIUS, S.BUNNY_CENTER, 0.12, 0x5EED)
        return 0, H.model_vertices(mesh, [H.translate(0.9, 0.3, -1.6), H.scale(8)])
    if name == "C4":
        return 0, H.model_vertices(H.mesh_teapot(), [H.rotate(40.0, 0, 1, 0), H.scale(0.2)])
    if name == "C1":
        rec = H.model_vertices(H.mesh_quad(27.5), [H.translate(0, 5.0, 0), H.rotate(180.0, 0, 0, 1), H.scale(0.035)])
        return len(scene("C1").packed.vertices) - len(rec), rec
    raise KeyError(name)


def same_model_unmoved(name):
    """The edit's range holds the model the edit moves: under the scene's own matrix
    model_vertices gives back the packed records bit for bit."""
    if name == "C2":
        mesh = H.mesh_displaced_sphere(24, 12, S.BUNNY_RADIUS, S.BUNNY_CENTER, 0.12, 0x5EED)
        return 0, H.model_vertices(mesh, [H.translate(0, 0, -2), H.scale(8)])
    if name == "C4":
        return 0, H.model_vertices(H.mesh_teapot(), [H.scale(0.2)])
    rec = H.model_vertices(H.mesh_quad(27.5), [H.translate(0, 5.54, 0), H.rotate(180.0, 0, 0, 1), H.scale(0.02)])
    return len(scene("C1").packed.vertices) - len(rec), rec
