"""Reference for the camera renders (include/rt_abi.h rt_camera,
rt_camera_rays_async, rt_render_camera_async): the header's "Camera renders"
semantics restated in Python floats -- test infrastructure.

Python floats are IEEE doubles with one rounding per operation and every
expression below keeps the header's order, so rays() and resolve() can be
compared with `==`. The PCG stream and Go's Sin / Cos / Tan come from the
oracle (oracle_pcg_float64, oracle_go_*); the vector helpers, the scene's view
and the quantisation are trace_ref's. Nothing here calls the library under
test: a camera is read from an abi.rt_camera record (None: all zeros).
"""
import ctypes as C
import math

import numpy as np

import go_raytracer_amd as rt
import oracle_bind
import trace_ref as T

abi = rt.abi
DEG = 0.017453292519943295
EYE = (0.0, 0.0, -1.0)


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def basis(eye, look_at, up):
    """(r, w, f) of a posed camera: right, up, forward."""
    f = T.v_norm(T.v_sub(look_at, eye))
    r = T.v_norm(cross(up, f))
    w = cross(f, r)
    return r, w, f


def frame(packed, cam):
    """(W, H, samples, draws per sample) of `cam` on `packed`."""
    cam = abi.rt_camera() if cam is None else cam
    sc = T.scene_of(packed)
    W = int(cam.width) or sc.width
    H = int(cam.height) or sc.height
    return W, H, int(cam.samples) or 4, 4 if cam.model == abi.RT_CAMERA_THINLENS else 2


def _sin(deg):
    return oracle_bind.lib().oracle_go_sin(DEG * deg)


def _cos(deg):
    return oracle_bind.lib().oracle_go_cos(DEG * deg)


def rays(packed, cam=None, y0=0, y1=None):
    """The camera's rays for rows [y0, y1): abi.RAY_DTYPE array [rows, W, samples]."""
    lib = oracle_bind.lib()
    cam = abi.rt_camera() if cam is None else cam
    sc = T.scene_of(packed)
    W, H, S, D = frame(packed, cam)
    if y1 is None:
        y1 = H
    model = int(cam.model)
    if model == abi.RT_CAMERA_ORTHO:
        vw = float(cam.extent)
    elif model != abi.RT_CAMERA_EQUIRECT and cam.fov > 0.0:
        fovr = float(cam.fov) * math.pi / 180.0
        vw = 2.0 / lib.oracle_go_tan(fovr / 2.0)
    else:
        vw = sc.vw
    vh = vw * (float(H) / float(W))
    posed = bool(cam.flags & abi.RT_CAMERA_POSED)
    if posed:
        eye = tuple(cam.eye[:])
        r, w, f = basis(eye, tuple(cam.look_at[:]), tuple(cam.up[:]))
    out = np.zeros((y1 - y0, W, S), dtype=abi.RAY_DTYPE)
    out["tmax"] = np.inf
    out["exclude"] = -1
    per_row = S * D
    draws = (C.c_double * (20 * per_row))()
    for x in range(W):
        for ymin in range(y0 // 20 * 20, y1, 20):
            lib.oracle_pcg_float64(0xDEAD ^ x, 0xBEEF ^ ymin, 20 * per_row, draws)
            for y in range(max(ymin, y0), min(ymin + 20, H, y1)):
                for s in range(S):
                    at = (y - ymin) * per_row + s * D
                    dx = draws[at] - 0.5
                    dy = draws[at + 1] - 0.5
                    su = (float(x) + dx) / float(W - 1)
                    sv = (float(y) + dy) / float(H - 1)
                    if model == abi.RT_CAMERA_EQUIRECT:
                        th = (su - 0.5) * 360.0
                        ph = (0.5 - sv) * 180.0
                        st, ct, sp, cp = _sin(th), _cos(th), _sin(ph), _cos(ph)
                        o = EYE
                        d = (st * cp, sp, ct * cp)
                    else:
                        u = su * vw - vw / 2.0
                        v = sv * vh - vh / 2.0
                        o = (u, -v, 0.0)
                        if model == abi.RT_CAMERA_ORTHO:
                            d = (0.0, 0.0, 1.0)
                        else:
                            d = T.v_norm(T.v_sub(o, EYE))
                            if model == abi.RT_CAMERA_THINLENS:
                                P = T.v_add(EYE, T.v_scale(d, T._div(float(cam.focus), d[2])))
                                rho = (float(cam.aperture) / 2.0) * math.sqrt(draws[at + 2])
                                al = 360.0 * draws[at + 3]
                                L = T.v_add(EYE, (rho * _cos(al), rho * _sin(al), 0.0))
                                o = L
                                d = T.v_norm(T.v_sub(P, L))
                    if posed:
                        pz = o[2] + 1.0
                        o = tuple(eye[k] + o[0] * r[k] + o[1] * w[k] + pz * f[k] for k in range(3))
                        d = tuple(d[0] * r[k] + d[1] * w[k] + d[2] * f[k] for k in range(3))
                    out[y - y0, x, s]["origin"] = o
                    out[y - y0, x, s]["dir"] = d
    return out


def resolve(rad):
    """(bytes, mean) of [rows, W, S] radiance records: the samples added in
    order, ((c0 + c1) + c2) + ..., scaled by 1.0 / S, quantised
    (trace_ref.image for any sample count, the mean kept)."""
    rows, W, S = rad.shape
    img = np.zeros((rows, W, 4), dtype=np.uint8)
    img[..., 3] = 255
    mean = np.zeros((rows, W, 3), dtype=np.float64)
    inv = 1.0 / S
    for y in range(rows):
        for x in range(W):
            total = tuple(float(c) for c in rad[y, x, 0]["color"])
            for k in range(1, S):
                total = T.v_add(total, tuple(float(c) for c in rad[y, x, k]["color"]))
            c = T.v_scale(total, inv)
            mean[y, x] = c
            img[y, x, :3] = [T.quantise(c[0]), T.quantise(c[1]), T.quantise(c[2])]
    return img, mean
