"""Frames that carry the trigonometric branches no other render reaches
through every kernel (needs an MI355X).

The host's go_tan beyond Pi/4 (fov above 90), its go_sin / go_cos in every
octant and in the large-argument reduction (constant fuzziness up to 5e8), and
the device's go_trig in the surface VM and in the fuzz offset of a closure
material (a surface function of u * 720 degrees and u * 8 radians). Every
frame: bytes and all counters equal the oracle's on the generic and on the
specialised context; the camera's rays, traced by the radiance kernel and
averaged, give the same bytes; closest-hit queries on the primary rays equal
tests/query_ref.py. Each test first counts, from the oracle's side, the pixels
whose primary ray lands where the test is about.
"""
import functools
from dataclasses import replace

import numpy as np
import pytest

import go_raytracer_amd as rt
from go_raytracer_amd import gml
import camera_ref
import oracle_bind
import query_ref as Q

abi = rt.abi
S = rt.scene
pytestmark = pytest.mark.gpu

RB = abi.RADIANCE_DTYPE.itemsize
FOVS = [1.0, 30.0, 89.999, 90.0, 90.001, 120.0, 135.0, 150.0, 179.0, 179.999]
# every octant of sin.go's reduction (0.3 .. 6.0 are octants 0 .. 7), the
# second turn, and the three-part reduction with a large multiple of Pi/4
FUZZ_LINEAR = [0.3, 1.2, 2.8, 4.4, 6.0, 100.0]
FUZZ_BVH = [0.8, 2.0, 3.6, 5.2, 7.0, 12345.678, 5e8]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = rt.RenderContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def spec_ctx():
    c = rt.RenderContext(0, specialize=True)
    yield c
    c.close()


# ---- the scenes ---------------------------------------------------------------

def fov_scene(fov):
    a = rt.configs.c3(48, 32)
    return replace(a, fov=fov, depth=4)


def fuzz_scene(fuzz, width, height, spheres=None):
    """Reflective spheres, one material each, over a reflective plane."""
    n = spheres or len(fuzz)
    objs = []
    for i in range(n):
        m = S.material((0.9 - 0.05 * i, 0.3 + 0.05 * i, 0.4), 0.6, fuzz[i % len(fuzz)], 0.0, 0.0, 0.8, 0.5, 20.0)
        row, col = divmod(i, 4)
        objs.append(S.Sphere(m).translate(-2.4 + 1.6 * col + 0.4 * row, -0.45 + 1.0 * row, 4.5 + 1.2 * row).uscale(0.55))
    objs.append(S.Plane(S.material((0.7, 0.7, 0.7), 0.4, fuzz[0], 0.0, 0.0, 1.0, 0.2, 5.0)).translate(0.0, -1.0, 0.0))
    lights = [S.PointLight((4.0, 5.0, 0.0), (0.7, 0.7, 0.7)), S.PointLight((-5.0, 6.0, 8.0), (0.5, 0.5, 0.5))]
    return S.RenderArgs(ambient=(0.1, 0.1, 0.1), lights=lights, scene=S.Union(tuple(objs)), depth=3, fov=80.0,
                        width=width, height=height, bg_start=(0.0, 0.0, 0.0), bg_end=(0.5, 0.7, 1.0))


CLOSURE_TRIG = """
{ /v /u /face
  u 720.0 mulf sin 0.5 mulf 0.5 addf
  v 720.0 mulf cos 0.5 mulf 0.5 addf
  0.6 point
  0.5  u 8.0 mulf  0.0 0.0  0.8 0.4 12.0 material } /s
s sphere -1.5 0.1 4.2 translate
s cylinder 0.3 -1.0 4.6 translate 30.0 rotatex 0.7 1.4 0.7 scale union
s cube 1.3 -0.9 3.4 translate 25.0 rotatey 15.0 rotatex union
s plane 0.0 -1.0 0.0 translate union /sc
0.2 0.2 0.2 point
[ -3.0 4.0 0.0 point 0.8 0.8 0.8 point pointlight  4.0 5.0 6.0 point 0.5 0.5 0.5 point pointlight ]
sc 3 90.0 64 48 "trig.ppm" render
"""


@functools.lru_cache(maxsize=None)
def packed(name):
    if name.startswith("fov"):
        return S.convert(fov_scene(float(name[3:])))
    if name == "fuzz_linear":
        return S.convert(fuzz_scene(FUZZ_LINEAR, 72, 48))
    if name == "fuzz_bvh":
        return S.convert(fuzz_scene(FUZZ_BVH, 72, 48, spheres=12))
    assert name == "closure"
    rendered, _ = gml.run_text(CLOSURE_TRIG)
    return S.convert(rendered[0][0])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(oracle frame, oracle counters, reference camera rays, oracle table of
    each pixel's first sample): computed once, shared, never modified."""
    p = packed(name)
    assert p.width <= 96 and p.height <= 64 and p.scene.depth <= 4
    img, st = oracle_bind.render_rows(p)
    rays = camera_ref.rays(p)
    first = rays[:, :, 0].reshape(-1)
    return img, st.as_dict(), rays, Q.Table(p, first["origin"], first["dir"])


def primary_hits(name, want):
    """Pixels whose first sample's primary ray lands on: "any" object, one with
    a constant material of fuzziness > 0 ("fuzzy"), one with a surface program
    ("closure")."""
    p = packed(name)
    T = reference(name)[3]
    n = 0
    for r, i in enumerate(T.winners()):
        if i < 0:
            continue
        o = p.scene.objects[int(i)]
        face = int(T.f[r, i])
        if o.kind == abi.RT_CSG:
            o = p.scene.csg_leaves[o.csg_first + (face >> 4)]
            face &= 7
        m = o.material[face]
        if want == "any" or (want == "closure" and m < 0) or \
                (want == "fuzzy" and m >= 0 and p.scene.materials[m].fuzziness > 0):
            n += 1
    return n


# ---- the checks ---------------------------------------------------------------

def render(c, p):
    c.set_scene(p)
    c.read_stats(reset=True)
    img = c.render()
    return img, c.read_stats(reset=True).as_dict()


def assert_same(img, ref, what):
    if not np.array_equal(img, ref):
        bad = np.argwhere((img != ref).any(axis=-1))
        y, x = bad[0]
        raise AssertionError("%s: %d pixels differ; first at (x=%d,y=%d) gpu=%s oracle=%s"
                             % (what, len(bad), x, y, img[y, x], ref[y, x]))


def check_every_kernel(ctx, spec_ctx, name):
    import torch
    p = packed(name)
    ref, ost, want_rays, table = reference(name)
    # the render kernels, generic and specialised
    for c, which in ((ctx, "generic"), (spec_ctx, "specialised")):
        img, st = render(c, p)
        assert_same(img, ref, "%s, %s" % (name, which))
        assert st == ost, (name, which)
    # the camera's rays (device trigonometry plays no part for the pinhole; the view's extent is the host's go_tan)
    H, W = p.height, p.width
    ctx.set_scene(p)
    rays = torch.empty(H * W * 4 * abi.RAY_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    out = torch.empty(H * W * 4 * RB, dtype=torch.uint8, device="cuda:0")
    ctx.camera_rays_async(0, H, rays)
    ctx.query_radiance_async(rays, out)
    img = ctx.image_from_radiance(out, 4)
    torch.cuda.synchronize()
    got_rays = rays.cpu().numpy().view(abi.RAY_DTYPE).reshape(H, W, 4)
    assert got_rays.tobytes() == want_rays.tobytes(), "%s: camera rays differ from tests/camera_ref.py" % name
    # the radiance kernel on those rays
    assert_same(img.cpu().numpy(), ref, "%s, camera rays -> radiance -> image" % name)
    rad = out.cpu().numpy().view(abi.RADIANCE_DTYPE)
    assert int(rad["rays"].sum()) == ost["primary_rays"] + ost["secondary_rays"], name
    # the query kernel on each pixel's first ray
    first = got_rays[:, :, 0].reshape(-1)
    got = ctx.closest_hits(first["origin"], first["dir"])
    bad = Q.fields_equal(got, table.closest())
    assert not bad, "%s: closest-hit fields %s differ" % (name, bad)


@pytest.mark.parametrize("fov", FOVS)
def test_fov_from_narrow_to_almost_flat(ctx, spec_ctx, fov):
    """c3 at 48x32: fov / 2 on both sides of Pi/4 (the host go_tan's -1 / y
    branch above it) up to the last degree before the tangent's pole."""
    name = "fov%r" % fov
    p = packed(name)
    assert p.scene.fov == fov
    assert primary_hits(name, "any") > 0
    ctx.set_scene(p)
    assert ctx.camera_rays().tobytes() == reference(name)[2].tobytes()  # camera_ref: ==, no tolerance
    check_every_kernel(ctx, spec_ctx, name)


@pytest.mark.parametrize("name", ["fuzz_linear", "fuzz_bvh"])
def test_constant_fuzz_in_every_octant(ctx, spec_ctx, name):
    """The host evaluates cos(fuzz) and sin(fuzz) at rt_set_scene: 13 values over
    the eight octants, a second turn and the large-argument reduction, in a
    scene below the linear / BVH switch and one above it."""
    p = packed(name)
    fuzzy = {m.fuzziness for m in p.scene.materials[:p.scene.num_materials]}
    assert fuzzy == set(FUZZ_LINEAR if name == "fuzz_linear" else FUZZ_BVH)
    assert primary_hits(name, "fuzzy") >= 200
    ctx.set_scene(p)
    assert bool(ctx.scene_info() & abi.RT_INFO_BVH) == (name == "fuzz_bvh")
    check_every_kernel(ctx, spec_ctx, name)


def test_fuzz_octants_are_all_eight():
    from gomath_inputs import octant
    assert {octant(f) for f in FUZZ_LINEAR + FUZZ_BVH} == set(range(8))
    assert len(FUZZ_LINEAR + FUZZ_BVH) == 13 and max(FUZZ_BVH) * 1.2732395447351628 > 2.0 ** 29


def test_fuzziness_beyond_the_restated_range_is_rejected(ctx):
    p = S.convert(fuzz_scene([float(1 << 29)], 16, 12))
    with pytest.raises(rt.render.RenderError) as e:
        ctx.set_scene(p)
    assert "(%d)" % abi.RT_E_INVALID in str(e.value)
    # the context stays usable
    ctx.set_scene(packed("fuzz_linear"))
    assert_same(ctx.render(), reference("fuzz_linear")[0], "after the rejected scene")


def test_closure_trig_in_the_vm_and_the_fuzz_offset(ctx, spec_ctx):
    """A sphere, a cylinder, a cube and a plane share one surface function:
    sin(720 u) and cos(720 v) degrees in the colour (two turns: every octant,
    in the VM), fuzziness 8 u radians (every octant, in the device's fuzz
    offset); on the plane u and v are world coordinates, hundreds of turns."""
    p = packed("closure")
    assert p.scene.num_programs >= 1 and (p.width, p.height) == (64, 48)
    assert primary_hits("closure", "closure") >= 500
    kinds = {p.scene.objects[int(i)].kind for i in reference("closure")[3].winners() if i >= 0}
    assert kinds == {abi.RT_SPHERE, abi.RT_CYLINDER, abi.RT_CUBE, abi.RT_PLANE}
    assert reference("closure")[1]["surface_errors"] == 0
    check_every_kernel(ctx, spec_ctx, "closure")
