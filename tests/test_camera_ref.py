"""tests/camera_ref.py against trace_ref and the oracle (CPU-only): with the
zero camera it restates the reference's camera, and its posed basis for the
reference's pose is the identity. This pins the reference the camera-render
tests compare the device with."""
import numpy as np

import go_raytracer_amd as rt
import camera_ref as CR
import oracle_bind
import trace_ref as T

abi = rt.abi


def field_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in abi.RAY_DTYPE.names)


def test_zero_camera_rays_equal_trace_ref_and_average_to_the_oracle_frame():
    p = T.packed("c3")  # 24 x 16
    want = T.camera_rays(p, 0, 16)
    got = CR.rays(p)
    assert got.shape == (16, 24, 4) and field_equal(got, want) and got.tobytes() == want.tobytes()
    assert field_equal(CR.rays(p, abi.rt_camera(), 5, 11), want[5:11])
    flat = got.reshape(-1)
    rad = T.trace_many(p, flat["origin"], flat["dir"], 0).reshape(got.shape)
    img, mean = CR.resolve(rad)
    ref, _ = oracle_bind.render_rows(p)
    assert np.array_equal(img, ref)
    assert np.array_equal(img, T.image(rad))
    assert mean.shape == (16, 24, 3) and len(np.unique(mean)) > 50


def test_sample_count_changes_the_draws_as_the_header_says():
    p = T.packed("c3")
    four = CR.rays(p)
    cam = abi.rt_camera()
    cam.samples = 2
    two = CR.rays(p, cam)
    assert two.shape == (16, 24, 2)
    # row 0 of a strip: sample s reads draws 2s, 2s + 1 whatever S is; row 1 starts at S * D
    assert field_equal(two[0], four[0, :, :2])
    assert not np.array_equal(two[1]["origin"], four[1, :, :2]["origin"])
    assert np.array_equal(two[1, :, 0]["origin"][:, 0], four[0, :, 2]["origin"][:, 0])  # the x jitter of draw 4


def test_reference_pose_is_the_identity():
    r, w, f = CR.basis((0.0, 0.0, -1.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    assert (r, w, f) == ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    p = T.packed("c3")
    cam = abi.rt_camera()
    cam.samples = 3
    plain = CR.rays(p, cam)
    cam.flags = abi.RT_CAMERA_POSED
    cam.eye[:] = [0.0, 0.0, -1.0]
    cam.look_at[:] = [0.0, 0.0, 0.0]
    cam.up[:] = [0.0, 1.0, 0.0]
    posed = CR.rays(p, cam)
    assert plain.shape == (16, 24, 3) and field_equal(posed, plain)
    # an oblique pose moves every origin and keeps the directions' lengths near 1
    cam.eye[:] = [3.0, 2.0, -4.0]
    cam.up[:] = [0.2, 1.0, 0.1]
    obl = CR.rays(p, cam)
    assert (obl["origin"] != plain["origin"]).any(axis=-1).all()
    assert np.allclose(np.linalg.norm(obl["dir"], axis=-1), 1.0, atol=1e-12)
