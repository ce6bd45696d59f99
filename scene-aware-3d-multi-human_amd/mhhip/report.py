"""The fit in numbers: per frame and per person, computed on the device (``mh_fit_report_pixels``, ``mh_fit_report_verts``
and kernels the cycle already has).  Read-only: buffers of its own, nothing of an engine's state is written."""
import numpy as np
import torch

from . import _lib, raster
from ._lib import check, ptr

COLUMNS = ('reproj_px', 'reproj_max_px', 'joints_used', 'mask_rendered', 'mask_seg', 'mask_inter', 'mask_iou', 'depth_bias_m',
           'depth_abs_m', 'behind_scene_px', 'pen_verts', 'pen_max_m', 'contact_dy_m', 'foot_slide_m')


def fit_report(model, verts, cam_K, image_size, bits=None, disp=None, min_z=None, max_z=None, scene_depth=None, scene_mask=None,
               scene_points=None, joints=None, pose2d=None, cam_dist_coef=None, joint_confidence_thr=0.5, verts_prev=None,
               has_prev=None, margin=0.05, depth_offset=0.2, chunk=32):
    """verts (T,N,V,3) on the device, camera space -> dict of (T,N) device tensors, the columns of ``COLUMNS``:

    reproj_px, reproj_max_px, joints_used -- ``joints`` (T,N,J,3) projected with ``cam_K`` / ``cam_dist_coef`` against
      ``pose2d`` (T,N,J,3) = x, y, confidence: mean and largest pixel distance over the joints with confidence >=
      ``joint_confidence_thr`` and their number; NaN, NaN, 0 for a body without such a joint (and without joints / pose2d);
    mask_rendered, mask_seg, mask_inter, mask_iou -- pixels the body owns in the composite of ``raster.render_scene``, pixels
      of its instance mask (``bits`` (T,H,W) int32 of ``mh_pack_masks``), pixels with both, inter / (rendered + seg - inter)
      (NaN when the union is empty); -1 / NaN without ``bits``;
    depth_bias_m, depth_abs_m -- mean d and mean |d| over the intersection, d = rendered depth + ``depth_offset`` - target
      depth 1 / (disp (1/min_z - 1/max_z) + 1/max_z) (``disp`` (T,H,W), ``min_z``, ``max_z`` (T)); NaN when the intersection is
      empty or without ``disp``;
    behind_scene_px -- pixels the body owns where ``scene_mask`` (H,W) is set and its depth > ``scene_depth`` + ``margin``;
    pen_verts, pen_max_m -- vertices (hidden ones included) inside the scene: z - scene_depth[pixel] > margin, and the largest
      such difference (0 if none); the three are -1, -1, NaN without a scene;
    contact_dy_m -- (mean of the 32 scene points nearest to the lowest vertex).y - that vertex.y (``scene_points`` (M,3));
      NaN without them;
    foot_slide_m -- || lowest vertex - the same vertex in ``verts_prev`` (T,N,V,3) ||; ``verts_prev`` None: the rows are
      consecutive frames, row t - 1 is the previous frame of row t; NaN where ``has_prev`` (T) is false (default: row 0).

    At most ``chunk`` frames are rendered at a time: memory beyond the inputs and outputs does not grow with T."""
    W, H = int(image_size[0]), int(image_size[1])
    if verts.dim() != 4 or verts.shape[-1] != 3:
        raise ValueError('verts must be (T,N,V,3), got %s' % (tuple(verts.shape),))
    T, N, V = int(verts.shape[0]), int(verts.shape[1]), int(verts.shape[2])
    if N > 32:
        raise ValueError('at most 32 people per frame, got %d' % N)
    if disp is not None and (bits is None or min_z is None or max_z is None):
        raise ValueError('disp needs bits, min_z and max_z')
    if (scene_depth is None) != (scene_mask is None):
        raise ValueError('scene_depth and scene_mask come together')
    chunk = max(1, min(int(chunk), T))
    dev = verts.device
    L = _lib.lib()
    f32 = lambda a, *s: torch.as_tensor(a, dtype=torch.float32).to(dev).contiguous().view(*s)
    nan = lambda: torch.full((T, N), float('nan'), dtype=torch.float32, device=dev)
    neg = lambda: torch.full((T, N), -1, dtype=torch.int32, device=dev)
    out = {}
    with torch.cuda.device(dev), torch.no_grad():
        st = _lib.stream_ptr(dev)
        verts = verts.contiguous().float()
        K = np.ascontiguousarray(np.asarray(cam_K, np.float32).reshape(9))
        Kp = K.ctypes.data_as(_lib.c_float_p)
        have_scene = scene_depth is not None
        if have_scene:
            scene_depth = f32(scene_depth, H, W)
            scene_mask = (torch.as_tensor(scene_mask).to(dev).reshape(H, W) != 0).to(torch.uint8).contiguous()
        # ---- pixels: composite of the chunk's frames, then one pass over its pixels ---------------------------------------------
        counts = torch.zeros(T, N, 4, dtype=torch.int32, device=dev)
        dsum = torch.zeros(T, N, 2, dtype=torch.float32, device=dev)
        have_bits = bits is not None
        if have_bits:
            bits = torch.as_tensor(bits).to(dev).contiguous().view(T, H, W)
            assert bits.dtype == torch.int32, 'bits are the int32 words of mh_pack_masks'
        if disp is not None:
            disp, min_z, max_z = f32(disp, T, H, W), f32(min_z, T), f32(max_z, T)
        if have_bits or have_scene:
            no_bits = None if have_bits else torch.zeros(chunk, H, W, dtype=torch.int32, device=dev)
            for t0 in range(0, T, chunk):
                tc = min(chunk, T - t0)
                sl = slice(t0, t0 + tc)
                img = raster.render_scene(model, verts[sl], cam_K, (W, H), outputs=('person', 'depth'), chunk=chunk)
                check(L.mh_fit_report_pixels(tc, N, H, W, ptr(img['person']), ptr(img['depth']),
                                             ptr(bits[sl]) if have_bits else ptr(no_bits[:tc]),
                                             None if disp is None else ptr(disp[sl]), None if disp is None else ptr(min_z[sl]),
                                             None if disp is None else ptr(max_z[sl]), ptr(scene_depth) if have_scene else None,
                                             ptr(scene_mask) if have_scene else None, float(depth_offset), float(margin),
                                             ptr(counts[sl]), ptr(dsum[sl]), st))
                del img
        c = counts.to(torch.float32)
        if have_bits:
            out['mask_rendered'], out['mask_seg'], out['mask_inter'] = (counts[..., k].clone() for k in range(3))
            union = c[..., 0] + c[..., 1] - c[..., 2]
            out['mask_iou'] = torch.where(union > 0, c[..., 2] / union.clamp(min=1), nan())
        else:
            out['mask_rendered'], out['mask_seg'], out['mask_inter'], out['mask_iou'] = neg(), neg(), neg(), nan()
        if disp is not None:
            some = c[..., 2] > 0
            out['depth_bias_m'] = torch.where(some, dsum[..., 0] / c[..., 2].clamp(min=1), nan())
            out['depth_abs_m'] = torch.where(some, dsum[..., 1] / c[..., 2].clamp(min=1), nan())
        else:
            out['depth_bias_m'], out['depth_abs_m'] = nan(), nan()
        # ---- body against scene -------------------------------------------------------------------------------------------------
        if have_scene:
            out['behind_scene_px'] = counts[..., 3].clone()
            pen_n = torch.zeros(T, N, dtype=torch.int32, device=dev)
            pen_m = torch.zeros(T, N, dtype=torch.float32, device=dev)
            check(L.mh_fit_report_verts(T * N, V, H, W, Kp, ptr(verts), ptr(scene_depth), ptr(scene_mask), float(margin), ptr(pen_n),
                                        ptr(pen_m), st))
            out['pen_verts'], out['pen_max_m'] = pen_n, pen_m
        else:
            out['behind_scene_px'], out['pen_verts'], out['pen_max_m'] = neg(), neg(), nan()
        # ---- key-points ---------------------------------------------------------------------------------------------------------
        if joints is not None and pose2d is not None:
            J = int(joints.shape[-2])
            jt = joints.contiguous().float().view(1, T * N * J, 3)
            p2 = f32(pose2d, T, N, J, 3)
            uv = torch.empty(1, T * N * J, 2, dtype=torch.float32, device=dev)
            Kdev = torch.as_tensor(K.reshape(1, 3, 3)).to(dev)
            kd = None if cam_dist_coef is None else np.ascontiguousarray(np.asarray(cam_dist_coef, np.float32).reshape(5))
            check(L.mh_project_points(1, T * N * J, ptr(jt), ptr(Kdev), None if kd is None else kd.ctypes.data_as(_lib.c_float_p), 0,
                                      ptr(uv), st))
            dist = (uv.view(T, N, J, 2) - p2[..., :2]).pow(2).sum(-1).sqrt()
            use = p2[..., 2] >= float(np.float32(joint_confidence_thr))
            n = use.sum(-1)
            out['reproj_px'] = torch.where(n > 0, (dist * use).sum(-1) / n.clamp(min=1), nan())
            out['reproj_max_px'] = torch.where(n > 0, torch.where(use, dist, torch.zeros_like(dist)).amax(-1), nan())
            out['joints_used'] = n.to(torch.int32)
        else:
            out['reproj_px'], out['reproj_max_px'] = nan(), nan()
            out['joints_used'] = torch.zeros(T, N, dtype=torch.int32, device=dev)
        # ---- lowest vertex: contact offset and foot slide -----------------------------------------------------------------------
        low_idx = torch.zeros(T * N, dtype=torch.int32, device=dev)
        low_xyz = torch.zeros(T * N, 3, dtype=torch.float32, device=dev)
        check(L.mh_lowest_vertex(ptr(verts), T * N, V, ptr(low_idx), ptr(low_xyz), st))
        if scene_points is not None and int(scene_points.shape[0]) > 0:
            pts = scene_points.to(dev).contiguous().float().view(-1, 3)
            M = int(pts.shape[0])
            grid = torch.empty(L.mh_scene_grid_bytes(M), dtype=torch.uint8, device=dev)
            dy = torch.zeros(T * N, dtype=torch.float32, device=dev)
            check(L.mh_scene_grid_build(ptr(pts), M, ptr(grid), st))
            check(L.mh_contact_knn_grid(ptr(grid), M, ptr(low_xyz), T * N, 32, ptr(dy), st))
            out['contact_dy_m'] = dy.view(T, N)
        else:
            out['contact_dy_m'] = nan()
        body = torch.arange(T * N, device=dev)
        ok = torch.ones(T, dtype=torch.bool, device=dev)
        if verts_prev is None:
            body = (body - N).clamp(min=0)
            ok[0] = False
            src = verts
        else:
            src = verts_prev.contiguous().float()
            assert tuple(src.shape) == (T, N, V, 3), 'verts_prev must have the shape of verts'
        was = src.view(T * N * V, 3)[body * V + low_idx.long()].view(T, N, 3)
        if has_prev is not None:
            ok = torch.as_tensor(np.asarray(has_prev, bool)).to(dev)
        slide = (low_xyz.view(T, N, 3) - was).pow(2).sum(-1).sqrt()
        out['foot_slide_m'] = torch.where(ok.view(T, 1).expand(T, N), slide, nan())
    return out
