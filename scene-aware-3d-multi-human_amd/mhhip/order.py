"""Who stands in front of whom, against the instance masks: the depth-ordering term of the fit (``mh_order_term``) as
numbers per frame and per person.  Read-only: buffers and a rasteriser workspace of its own."""
import numpy as np
import torch

from . import _lib, raster
from ._lib import check, ptr


def order_terms(model, verts, cam_K, image_size, bits, ebits, gate=None, margin=0.05, delta=0.5, chunk=32):
    """verts (T,N,V,3) on the device, camera space; bits, ebits (T,H,W) int32: the raw and the twice-eroded instance-mask
    words (``mh_pack_masks``, ``mh_erode_bits``); gate (T,N) float or None: a body with gate 0 takes part in nothing
    -> dict of device tensors, for person n of frame t as the OWNER of a pixel (include/mhmocap_hip.h has the definition):

    order_px (T,N) i32: (pixel, other person) pairs where the other person -- absent there according to the raw mask --
    is not at least ``margin`` behind n | order_pairs (T,N,N) i32: the same by the other person, [t][n][other] |
    order_loss (T,N) f32: the term's value at coefficient 1, (1 / (H W)) sum of d^2 (linear beyond ``delta``).

    The selection pass runs like in ``raster.render_scene`` (loss coefficients 0, no gradients) over at most ``chunk``
    frames at a time on one workspace of its own, so memory beyond the outputs does not grow with T."""
    W, H = int(image_size[0]), int(image_size[1])
    if verts.dim() != 4 or verts.shape[-1] != 3:
        raise ValueError('verts must be (T,N,V,3), got %s' % (tuple(verts.shape),))
    T, N, V = int(verts.shape[0]), int(verts.shape[1]), int(verts.shape[2])
    if N > 32:
        raise ValueError('at most 32 people per frame, got %d' % N)
    chunk = max(1, min(int(chunk), T))
    dev = verts.device
    L = _lib.lib()
    with torch.cuda.device(dev), torch.no_grad():
        st = _lib.stream_ptr(dev)
        verts = verts.contiguous().float()
        words = []
        for name, w in (('bits', bits), ('ebits', ebits)):
            w = torch.as_tensor(w).to(dev).contiguous()
            if w.dtype != torch.int32 or tuple(w.shape) != (T, H, W):
                raise ValueError('%s must be (T,H,W) int32 = (%d,%d,%d), got %s %s' % (name, T, H, W, w.dtype, tuple(w.shape)))
            words.append(w)
        bits, ebits = words
        if gate is not None:
            gate = torch.as_tensor(gate, dtype=torch.float32).to(dev).contiguous().view(T, N)
        faces = torch.as_tensor(np.ascontiguousarray(np.asarray(model.faces).astype(np.int32))).to(dev)
        F = int(faces.shape[0])
        out = dict(order_px=torch.zeros(T, N, dtype=torch.int32, device=dev),
                   order_pairs=torch.zeros(T, N, N, dtype=torch.int32, device=dev),
                   order_loss=torch.zeros(T, N, dtype=torch.float32, device=dev))
        zeros = raster.selection_zeros((chunk, N, V, F, H, W), dev)
        K = np.ascontiguousarray(np.asarray(cam_K, np.float32).reshape(9))
        ws = torch.empty(L.mh_raster_workspace_bytes(chunk, N, V, F, H, W), dtype=torch.uint8, device=dev)
        for t0 in range(0, T, chunk):
            tc = min(chunk, T - t0)
            dims = (tc, N, V, F, H, W)
            sl = slice(t0, t0 + tc)
            v = verts[sl]
            raster.selection_pass(dims, K, v, faces, ws, st, zeros)
            check(L.mh_order_term(*dims, ptr(ws), ptr(bits[sl]), ptr(ebits[sl]), None if gate is None else ptr(gate[sl]),
                                  1.0, float(margin), float(delta), None, ptr(out['order_loss'][sl]), ptr(out['order_px'][sl]),
                                  ptr(out['order_pairs'][sl]), None, st))
    return out
