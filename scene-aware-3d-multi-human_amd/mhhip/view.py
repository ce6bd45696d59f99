"""Free-viewpoint render of a fit: the fitted meshes and the coloured scene point cloud from ANY camera, or a camera path
with one view per frame, in one z-buffer on the device (``mh_view_project`` / ``_clear`` / ``_raster`` / ``_splat`` /
``_resolve``, csrc/mh_view.hip).  The side or top view is where depth, scale and contact errors show: people stand ON the
scene, do not float above it and keep their distances in depth.  Replaces the reference's interactive Open3D window
(mhmocap/visualization.py) on a headless device.  Read-only: buffers of its own, nothing of an engine's state is written.

Cameras are ``(R, t)`` with ``x_view = R x + t`` and the fit's own convention: x right, y down, z forward."""
import ctypes

import numpy as np
import torch

from . import _lib, raster
from ._lib import check, ptr

VIEW_OUTPUTS = ('image', 'depth', 'label', 'face', 'coverage')
MAX_VIEWS = 64          # views per mh_view_project call
SCENE_LABEL = -2


# ---- cameras (plain numpy) ----------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0, -1, 0)):
    """Camera at ``eye`` looking at ``target``: (R (3,3), t (3)) float64 with x_view = R x + t.  The rows of R are the
    camera's axes in the fit's convention -- x right, y DOWN, z forward -- so ``up`` (a world direction, default the world's
    -y) points to the top of the image and the target lies on the optical axis: R target + t = (0, 0, distance)."""
    eye, target, up = (np.asarray(a, np.float64).reshape(3) for a in (eye, target, up))
    z = target - eye
    d = np.linalg.norm(z)
    if not d > 0:
        raise ValueError('look_at: eye and target coincide')
    z = z / d
    x = np.cross(z, up)                  # right = forward x up: a right-handed frame with y down
    if np.linalg.norm(x) < 1e-9:         # looking along `up`: the world's z (or x) stands in for it
        x = np.cross(z, (0.0, 0.0, 1.0) if abs(z[2]) < 0.9 else (1.0, 0.0, 0.0))
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ eye


def orbit(center, radius, elevation_deg, azimuth_deg):
    """Cameras on a sphere of ``radius`` around ``center``, looking at it: azimuth 0, elevation 0 is the fit camera's side
    (the camera at center - radius z, looking along +z); the azimuth turns about the world's vertical (y) axis, a positive
    elevation raises the camera (towards -y).  Scalars give (R (3,3), t (3)); arrays (broadcast) give ((T,3,3), (T,3))."""
    center = np.asarray(center, np.float64).reshape(3)
    el, az = np.broadcast_arrays(np.radians(np.asarray(elevation_deg, np.float64)), np.radians(np.asarray(azimuth_deg, np.float64)))
    single = el.ndim == 0
    Rs, ts = [], []
    for e, a in zip(el.reshape(-1), az.reshape(-1)):
        eye = center + float(radius) * np.asarray([-np.sin(a) * np.cos(e), -np.sin(e), -np.cos(a) * np.cos(e)])
        R, t = look_at(eye, center)
        Rs.append(R)
        ts.append(t)
    return (Rs[0], ts[0]) if single else (np.stack(Rs), np.stack(ts))


def top_down(center, height):
    """Camera ``height`` above ``center`` (towards -y) looking straight down; the fit camera's forward (+z) is the top of the image."""
    center = np.asarray(center, np.float64).reshape(3)
    return look_at(center - np.asarray([0.0, float(height), 0.0]), center, up=(0, 0, 1))


def cloud_from_depth(depth, mask, cam_K, rgb=None, splat=1.0):
    """The coloured point cloud of a scene depth map under the camera it belongs to: the masked pixels (row-major) with a
    finite positive depth, unprojected with pixel centres at +0.5 -> (points (P,3) f32, colours (P,3) u8, extent (P) f32,
    pixel index (P) int64).  ``rgb`` (H,W,3) u8, None: mid-grey.  extent = splat * depth / fx: a depth pixel keeps its metric
    footprint in another view."""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    K = np.asarray(cam_K, np.float32).reshape(3, 3)
    keep = (np.asarray(mask).reshape(H, W) != 0) & np.isfinite(depth) & (depth > 0)
    pix = np.flatnonzero(keep.reshape(-1))
    d = depth.reshape(-1)[pix]
    u = (pix % W).astype(np.float32) + np.float32(0.5)
    v = (pix // W).astype(np.float32) + np.float32(0.5)
    pts = np.stack([(u - K[0, 2]) / K[0, 0] * d, (v - K[1, 2]) / K[1, 1] * d, d], axis=1).astype(np.float32)
    col = np.full((len(pix), 3), 128, np.uint8) if rgb is None else np.asarray(rgb).reshape(H * W, 3)[pix].astype(np.uint8)
    return pts, col, (np.float32(splat) * d / K[0, 0]).astype(np.float32), pix


def _views(view, T):
    R, t = view
    R, t = np.asarray(R, np.float32), np.asarray(t, np.float32)
    if R.shape == (3, 3) and t.shape == (3,):
        R, t = np.broadcast_to(R, (T, 3, 3)), np.broadcast_to(t, (T, 3))
    if R.shape != (T, 3, 3) or t.shape != (T, 3):
        raise ValueError('view must be (R (3,3), t (3)) or ((T,3,3), (T,3)) with T = %d, got %s and %s' % (T, R.shape, t.shape))
    return np.ascontiguousarray(R), np.ascontiguousarray(t)


def render_view(model, verts, view, K, image_size, cloud=None, cloud_rgb=None, cloud_size_m=None, palette=None, light=(0, 0, 1),
                ambient=0.3, background=(255, 255, 255), near=0.1, max_half=3, outputs=None, chunk=32, timings=None):
    """verts (T,N,V,3) on the device, in the space the views are given in (the fit camera's) -> dict of device tensors:

    image (T,H,W,3) u8: a person's pixel is 255 * palette * shade, a scene pixel has its point's colour, an empty one
    ``background`` | depth (T,H,W) f32 in metres along the view's axis, a multiple of 2^-12 (-1 = empty) | label (T,H,W) i32:
    person, -2 = scene, -1 = empty | face (T,H,W) i32: face of the person / point of the cloud / -1 | coverage (T,N+1) i32:
    pixels of every person, then of the scene.  ``outputs``: the names wanted (default all five; ``'keys'`` may be asked for
    as well: the z-buffer (T,H,W), the bits of the uint64 keys in an int64 tensor); only those are allocated and returned.

    ``view``: (R (3,3), t (3)) for every frame or ((T,3,3), (T,3)), one view per frame; ``K`` 3x3 and ``image_size`` (W,H)
    of the VIEW (W, H <= 4096).  ``cloud`` (P,3) with ``cloud_rgb`` (P,3) u8 (None: mid-grey) and ``cloud_size_m`` (P)
    extents in metres (None: single pixels): a point covers a square of up to 2 ``max_half`` + 1 pixels.  ``palette`` (N,3)
    in [0,1], default ``raster.default_palette``; shade = ambient + (1 - ambient) max(0, -n.light) as in
    ``raster.render_scene``, ``light`` in VIEW space: the default (0,0,1) is a head-light.  Everything in front of ``near``
    metres is dropped; faces are not clipped: a face with a vertex in front of ``near`` disappears as a whole.

    After the float32 projection everything is integer arithmetic and one 64-bit atomic minimum per covered pixel: the same
    bits on every launch (conventions: csrc/mh_view.hip).  At most ``chunk`` (<= 64) frames at a time, so memory beyond the
    outputs does not grow with T.  ``timings``: a dict to which the milliseconds of project, raster, splat and resolve
    are ADDED (the call then waits for the device)."""
    W, H = int(image_size[0]), int(image_size[1])
    if verts.dim() != 4 or verts.shape[-1] != 3:
        raise ValueError('verts must be (T,N,V,3), got %s' % (tuple(verts.shape),))
    T, N, V = int(verts.shape[0]), int(verts.shape[1]), int(verts.shape[2])
    allowed = VIEW_OUTPUTS + ('keys',)
    names = VIEW_OUTPUTS if outputs is None else tuple(outputs)
    bad = [k for k in names if k not in allowed]
    if bad or not names:
        raise ValueError('outputs must name some of %s, got %r' % (', '.join(allowed), outputs))
    if N > 32:
        raise ValueError('at most 32 people per frame, got %d' % N)
    if not (0 < W <= 4096 and 0 < H <= 4096):
        raise ValueError('image_size must be within 4096 x 4096, got %r' % (image_size,))
    if not 0 <= int(max_half) <= 8:
        raise ValueError('max_half must be in [0, 8], got %r' % (max_half,))
    R, t = _views(view, T)
    chunk = max(1, min(int(chunk), T, MAX_VIEWS))
    dev = verts.device
    L = _lib.lib()
    Kh = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
    Kp = Kh.ctypes.data_as(_lib.c_float_p)
    fq = int(np.rint(np.float64(Kh[0]) * 64))
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)
    with torch.cuda.device(dev), torch.no_grad():
        st = _lib.stream_ptr(dev)
        verts = verts.contiguous().float()
        faces = torch.as_tensor(np.ascontiguousarray(np.asarray(model.faces).astype(np.int32))).to(dev)
        F = int(faces.shape[0])
        pal = raster.default_palette(N) if palette is None else np.ascontiguousarray(np.asarray(palette, np.float32))
        if pal.shape != (N, 3):
            raise ValueError('palette must be (N,3) = (%d,3), got %s' % (N, pal.shape))
        pal = torch.as_tensor(pal).to(dev)
        lgt = np.ascontiguousarray(np.asarray(light, np.float32).reshape(3))
        bg = np.ascontiguousarray(np.asarray(background, np.uint8).reshape(3))
        bgp = bg.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        P = 0
        if cloud is not None:
            cloud = torch.as_tensor(cloud).to(dev).float().contiguous().view(-1, 3)
            P = int(cloud.shape[0])
        if P:
            rgb = torch.full((P, 3), 128, dtype=torch.uint8, device=dev) if cloud_rgb is None else \
                torch.as_tensor(cloud_rgb).to(dev).contiguous().view(P, 3)
            if rgb.dtype != torch.uint8:
                raise ValueError('cloud_rgb must be uint8, got %s' % rgb.dtype)
            size_q = None
            if cloud_size_m is not None:
                sz = torch.as_tensor(cloud_size_m).to(dev).double().view(P)
                size_q = torch.round(sz * 4096).clamp(0, 2 ** 31 - 1).to(torch.int32).contiguous()
            pq = torch.empty(chunk, P, 3, dtype=torch.int32, device=dev)
        shapes = dict(image=((T, H, W, 3), torch.uint8), depth=((T, H, W), torch.float32), label=((T, H, W), torch.int32),
                      face=((T, H, W), torch.int32), coverage=((T, N + 1), torch.int32), keys=((T, H, W), torch.int64))
        out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in names}
        keys = out['keys'] if 'keys' in out else torch.empty(chunk, H, W, dtype=torch.int64, device=dev)
        vq = torch.empty(chunk * N, V, 3, dtype=torch.int32, device=dev)
        resolve = [k for k in names if k != 'keys']
        ms = dict(project=0.0, raster=0.0, splat=0.0, resolve=0.0)
        marks = []

        def stage(name, fn):
            if timings is None:
                return fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            marks.append((name, a, b))

        for t0 in range(0, T, chunk):
            tc = min(chunk, T - t0)
            v = verts[t0:t0 + tc]
            Rc, tcam = np.ascontiguousarray(R[t0:t0 + tc]), np.ascontiguousarray(t[t0:t0 + tc])
            kc = keys[t0:t0 + tc] if 'keys' in out else keys[:tc]

            def project():
                # rows of a frame's N bodies share the frame's view: N V entries per view
                check(L.mh_view_project(N * V, 1, tc, ptr(v), fp(Rc), fp(tcam), Kp, float(near), ptr(vq), st))
                if P:
                    check(L.mh_view_project(P, 0, tc, ptr(cloud), fp(Rc), fp(tcam), Kp, float(near), ptr(pq), st))
            stage('project', project)
            check(L.mh_view_clear(tc, H, W, ptr(kc), st))
            stage('raster', lambda: check(L.mh_view_raster(tc, N, V, F, H, W, ptr(vq), ptr(faces), ptr(kc), st)))
            if P:
                stage('splat', lambda: check(L.mh_view_splat(tc, P, H, W, ptr(pq), ptr(size_q), fq, int(max_half), ptr(kc), st)))
            if resolve:
                vv = None
                if 'image' in out:     # the shading's normals: the vertices in view space (a rotation: plain tensor algebra)
                    Rd, td = torch.as_tensor(Rc).to(dev), torch.as_tensor(tcam).to(dev)
                    vv = (torch.einsum('tij,tnvj->tnvi', Rd, v) + td.view(tc, 1, 1, 3)).contiguous()
                o = lambda k: ptr(out[k][t0:t0 + tc]) if k in out else None
                stage('resolve', lambda: check(L.mh_view_resolve(
                    tc, N, V, F, H, W, ptr(kc), ptr(vv), ptr(faces), ptr(rgb) if P else None, ptr(pal), fp(lgt), float(ambient), bgp,
                    o('image'), o('depth'), o('label'), o('face'), o('coverage'), st)))
        if timings is not None:
            torch.cuda.synchronize(dev)
            for name, a, b in marks:
                ms[name] += a.elapsed_time(b)
            for name in ms:
                timings[name] = timings.get(name, 0.0) + ms[name]
    return out
