"""What the maps over bodies (``contact``, ``proximity``, ``inside``, ``surface``) share on the host: the faces of a model and the
tables made of them, kept on the model per device; the body parts; and the checks of the arguments they have in common.
Nothing here launches a kernel."""
import numpy as np
import torch

PART_NAMES = ('pelvis', 'left_hip', 'right_hip', 'spine1', 'left_knee', 'right_knee', 'spine2', 'left_ankle', 'right_ankle', 'spine3',
              'left_foot', 'right_foot', 'neck', 'left_collar', 'right_collar', 'head', 'left_shoulder', 'right_shoulder', 'left_elbow',
              'right_elbow', 'left_wrist', 'right_wrist', 'left_hand', 'right_hand')
MAX_RADIUS = 0.64           # MH_SCENE_NEAREST_MAX_CELLS (32) cells of the smallest grid cell (0.02 m)
MAX_PEOPLE = 32


def body_parts(model):
    """(V,) uint8: the joint with the largest skinning weight of every vertex, the first one on ties.  ``model``: a body model
    (``lbs_weights``), an SMPL data struct (``weights``), or the (V,J) weights themselves, J <= 32."""
    w = model
    for name in ('lbs_weights', 'weights'):
        if hasattr(w, name):
            w = getattr(w, name)
            break
    w = w.toarray() if hasattr(w, 'toarray') else w
    w = np.asarray(w.detach().cpu() if isinstance(w, torch.Tensor) else w)
    if w.ndim != 2 or w.shape[0] == 0 or not 1 <= w.shape[1] <= 32:
        raise ValueError('skinning weights must be (V,J) with 1 <= J <= 32, got %s' % (tuple(w.shape),))
    return np.argmax(w, axis=1).astype(np.uint8)          # numpy's argmax keeps the first of equal entries


def part_table(model, V, dev):
    """(``body_parts(model)`` on ``dev``, the number of parts): one part of ``PART_NAMES`` for each of the V vertices"""
    part = body_parts(model)
    if part.shape[0] != V:
        raise ValueError('the model has %d vertices, verts %d' % (part.shape[0], V))
    P = len(PART_NAMES)
    if int(part.max()) >= P:
        raise ValueError('the model has more than %d parts' % P)
    return torch.as_tensor(part).to(dev), P


def faces_of(model):
    """the faces of a body model (``faces``), of an SMPL data struct (``f``), or the array itself, on the host"""
    for name in ('faces', 'f'):
        if hasattr(model, name):
            return np.asarray(getattr(model, name))
    return np.asarray(model)


def vertex_faces(faces, V):
    """faces (F,3) integers, V -> (adj_start (V+1) int32, adj_face (A) int32): for vertex v the faces
    ``adj_face[adj_start[v]:adj_start[v+1]]`` that name it, in ascending face index, a face once per corner that names the
    vertex.  Corners that name a vertex outside [0, V) are left out (the kernel skips such a face altogether)."""
    faces = np.asarray(faces)
    if faces.ndim != 2 or faces.shape[1] != 3 or int(V) <= 0:
        raise ValueError('faces must be (F,3) and V positive, got %s and %r' % (tuple(faces.shape), V))
    V = int(V)
    corner = faces.astype(np.int64).reshape(-1)
    face = np.repeat(np.arange(faces.shape[0], dtype=np.int64), 3)
    keep = (corner >= 0) & (corner < V)
    corner, face = corner[keep], face[keep]
    order = np.argsort(corner, kind='stable')             # stable: the faces of a vertex stay in ascending order
    adj_start = np.zeros(V + 1, np.int32)
    adj_start[1:] = np.cumsum(np.bincount(corner, minlength=V))
    return adj_start, face[order].astype(np.int32)


def _tables(model, dev):
    """the tables of ``model`` on ``dev``, {'faces': int32 tensor, V: (adj_start, adj_face), ...}: built once per model and
    device where the model can keep them (``model._body_tables``)"""
    cache = getattr(model, '_body_tables', None)
    if cache is not None and str(dev) in cache:
        return cache[str(dev)]
    tabs = {'faces': torch.as_tensor(np.ascontiguousarray(faces_of(model), dtype=np.int32)).to(dev)}
    try:
        if cache is None:
            cache = model._body_tables = {}
        cache[str(dev)] = tabs
    except AttributeError:                                  # (an array of faces: nothing to keep them on)
        pass
    return tabs


def faces(model, dev):
    """(F,3) int32 on ``dev``, F > 0"""
    fc = _tables(model, dev)['faces']
    if fc.dim() != 2 or fc.shape[1] != 3 or fc.shape[0] == 0:
        raise ValueError('faces must be (F,3), got %s' % (tuple(fc.shape),))
    return fc


def adjacency(model, V, dev):
    """(faces (F,3), adj_start (V+1), adj_face (A)) int32 on ``dev``: ``vertex_faces`` of the model's faces, built at its
    first use"""
    tabs = _tables(model, dev)
    if V not in tabs:
        tabs[V] = tuple(torch.as_tensor(a).to(dev) for a in vertex_faces(faces_of(model), V))
    return (tabs['faces'],) + tabs[V]


def shape(verts):
    """(T, N, V) of verts (T,N,V,3), N <= MAX_PEOPLE"""
    if verts.dim() != 4 or verts.shape[-1] != 3 or 0 in verts.shape:
        raise ValueError('verts must be (T,N,V,3), got %s' % (tuple(verts.shape),))
    T, N, V = int(verts.shape[0]), int(verts.shape[1]), int(verts.shape[2])
    if N > MAX_PEOPLE:
        raise ValueError('at most %d people per frame, got %d' % (MAX_PEOPLE, N))
    return T, N, V


def batch_shape(verts, points):
    """(B, V, Q) of verts (B,V,3) and points (B,Q,3)"""
    if verts.dim() != 3 or verts.shape[-1] != 3 or 0 in verts.shape:
        raise ValueError('verts must be (V,3) or (B,V,3), got %s' % (tuple(verts.shape),))
    B, V = int(verts.shape[0]), int(verts.shape[1])
    if points.dim() != 3 or points.shape[-1] != 3 or 0 in points.shape or points.shape[0] != B:
        raise ValueError('points must be (Q,3) for verts (V,3) or (B,Q,3) for verts (B,V,3), got %s' % (tuple(points.shape),))
    return B, V, int(points.shape[1])


def live_mask(live, *dims):
    """``live`` of shape ``dims``, (T,N) or (B), as uint8 on the host, or None"""
    if live is None:
        return None
    lv = torch.as_tensor(live)
    if tuple(lv.shape) != dims:
        raise ValueError('live must be %s = (%s), got %s' % ('(T,N)' if len(dims) == 2 else '(B)', ','.join('%d' % d for d in dims),
                                                             tuple(lv.shape)))
    return (lv != 0).to(torch.uint8)


def cell_radius(radius):
    """a radius the grid kernels can walk: positive, at most MAX_RADIUS; as the float32 the kernel gets"""
    r = float(np.float32(radius))
    if not (np.isfinite(r) and 0.0 < r <= MAX_RADIUS):
        raise ValueError('radius must be positive and at most %.2f m (the kernel walks every cell within it), got %r' % (MAX_RADIUS, radius))
    return r


def any_radius(radius):
    """a positive radius, inf included; as the float32 the kernel gets"""
    r = float(np.float32(radius))
    if not r > 0.0:                                         # (NaN, zero, negative, -inf)
        raise ValueError('radius must be positive (inf is allowed), got %r' % (radius,))
    return r


def contact_within(contact, radius):
    """the contact threshold of a map, as the float32 the kernel gets: it cannot lie beyond the search radius"""
    contact = float(np.float32(contact))
    if not 0.0 <= contact <= radius:
        raise ValueError('contact must lie in [0, radius = %g]: beyond the radius no distance is known, got %g' % (radius, contact))
    return contact
