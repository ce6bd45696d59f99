"""Scenes, launches and the fixture of tests/test_raster_five_waves_gpu.py.

The selection kernel (csrc/mh_raster.hip, k_raster_strip) was put on a register diet and tried with ten waves per tile
workgroup instead of eight (RSB): which wave meets which face, and in which order the keys reach a pixel, follows the wave
count.  The 40 bytes per pixel must not.  The fixture pins that inside the tree: it was written by THIS script with the
library of the commit before the change (MHHIP_LIB=<that build> python tests/golden/make_five_waves.py, on the GPU), and the
test runs the same functions on the tree's library.

five_waves_parent.npz holds, per scene, the camera-space vertices handed to the selection pass (float32: the test does
not depend on any host's libm or BLAS), the windows and the keys; and the leaves after a three-cycle deterministic fit."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, 'five_waves_parent.npz')
EMPTY = np.uint64(0xffffffffffffffff)

# (name, W, H, T, N, seed, zlo, zhi): SMPL-sized bodies close to the camera -- windows of two tiles, the second one partial,
# a score of rounds per wave
KEY_SCENES = [('landscape', 96, 54, 1, 2, 11, 1.6, 2.0), ('portrait', 27, 48, 1, 1, 12, 0.9, 1.0)]
FIT = dict(T=6, N=2, W=64, H=36, batch=3, seed=77, cycles=3)


def faces_digest(faces):
    return hashlib.sha1(np.ascontiguousarray(np.asarray(faces).astype(np.int32)).tobytes()).hexdigest()


def posed_bodies(smpl_struct, smpl_regs, T, N, W, H, seed, zlo, zhi):
    """(T,N,V,3) float32 camera-space vertices of the suite's random scene (tests/test_raster_gpu.py::_scene, through the
    fuzz module that uses it), posed by the CPU oracle"""
    import torch
    import test_raster_fuzz_gpu as fz
    from oracle import lbs_oracle as lo
    sp, pT, _ = fz.tr._scene(T, N, W, H, seed, zlo, zhi)
    omodel = lo.BodyModel(smpl_struct, smpl_regs)
    with torch.no_grad():
        be = torch.tensor(sp['betas_gt'])[None].expand(T, N, 10).reshape(-1, 10)
        v = lo.smpl_forward(omodel, be, torch.tensor(sp['poses_gt']).view(-1, 72))['verts'].view(T, N, -1, 3)
        v = v + torch.tensor(pT).view(T, N, 1, 3)
    return np.ascontiguousarray(v.numpy().astype(np.float32))


class Selection(object):
    """the selection pass alone on given vertices and faces (mhhip.raster.selection_pass without the re-initialisation:
    a second launch on the same workspace meets the first one's face lists and keys)"""

    def __init__(self, verts, faces, W, H, fov=60.0, dev='cuda:0'):
        import torch
        from mhhip import _lib, synthetic
        from mhhip.raster import selection_zeros
        self.dev = torch.device(dev)
        self.verts = torch.as_tensor(np.ascontiguousarray(verts, np.float32)).to(self.dev)
        self.faces = torch.as_tensor(np.ascontiguousarray(np.asarray(faces).astype(np.int32))).to(self.dev)
        T, N, V = self.verts.shape[:3]
        self.dims = (int(T), int(N), int(V), int(self.faces.shape[0]), int(H), int(W))
        self.K = np.ascontiguousarray(synthetic.default_cam_K((W, H), fov).reshape(9))
        L = _lib.lib()
        self.ws = torch.empty(L.mh_raster_workspace_bytes(*self.dims), dtype=torch.uint8, device=self.dev)
        self.z = selection_zeros(self.dims, self.dev)
        _lib.check(L.mh_raster_workspace_init(*self.dims, _lib.ptr(self.ws), _lib.stream_ptr(self.dev)))

    def launch(self):
        """one selection launch -> (win (B,4) int32, keys (window pixels, 5) uint64 in body order)"""
        import ctypes
        import torch
        from mhhip import _lib
        from mhhip._lib import check, ptr
        L, z, st = _lib.lib(), self.z, _lib.stream_ptr(self.dev)
        check(L.mh_raster_terms_phase(*self.dims, self.K.ctypes.data_as(_lib.c_float_p), ptr(self.verts), ptr(self.faces),
                                      ptr(z['bits']), ptr(z['bits']), ptr(z['depths']), ptr(z['tz']), ptr(z['tz']), ptr(z['ones']),
                                      ptr(z['front']), ptr(z['zb']), ptr(z['ones']), ptr(z['zb']), 0.0, 0.0, 1e-3, None, None, None,
                                      ptr(z['dbody']), ptr(z['sbody']), ptr(self.ws), None, None, 1, st))
        torch.cuda.synchronize()
        T, N, _, _, H, W = self.dims
        B = T * N
        off = (ctypes.c_size_t * 3)()
        check(L.mh_raster_workspace_offsets(*self.dims, off))
        win = self.ws[off[0]:off[0] + B * 16].view(torch.int32).view(B, 4).cpu().numpy()
        first = self.ws[off[1]:off[1] + B * 8].view(torch.int64).cpu().numpy()
        npix = np.maximum(win[:, 2], 0).astype(np.int64) * np.maximum(win[:, 3], 0)
        if not int(npix.sum()):
            return win, np.zeros((0, 5), np.uint64)
        src = np.concatenate([first[b] + np.arange(npix[b], dtype=np.int64) for b in range(B)])
        raw = self.ws[off[2]:off[2] + B * H * W * 40].view(torch.int64).view(-1, 5)
        return win, raw[torch.as_tensor(src, device=self.dev)].cpu().numpy().view(np.uint64).reshape(-1, 5)


def fit_leaves(smpl_struct, smpl_regs, oracle_model, tmp_path):
    """the leaves after FIT['cycles'] cycles of a fit in deterministic mode, on the suite's small sequence
    (tests/test_raster_paths_gpu.py::_setup)"""
    import test_raster_paths_gpu as tp
    from mhhip.raster import set_deterministic
    f = FIT
    old = set_deterministic(True)
    try:
        opt, dl, _, _, _ = tp._setup(smpl_struct, smpl_regs, oracle_model, tmp_path, f['T'], f['N'], f['W'], f['H'], f['batch'], f['seed'], True)
        opt.fit(dl, num_iter=f['cycles'])
        e = opt.engine
        return {n: e.leaf(n).detach().cpu().numpy().copy() for n in ('poses_T', 'poses_smpl', 'betas', 'zmin_lin', 'zmax_lin', 'xscale')}
    finally:
        set_deterministic(old)


def main(out):
    import pathlib
    import tempfile
    for p in (ROOT, os.path.join(ROOT, 'scene-aware-3d-multi-human_amd'), os.path.join(ROOT, 'tests'), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    from mhhip import synthetic
    from oracle import lbs_oracle
    struct = synthetic.make_smpl_struct(1)
    regs = synthetic.make_extra_regressors(1, struct)
    faces = np.asarray(struct.f).astype(np.int32)
    d = dict(faces_sha1=np.array(faces_digest(faces)))
    for name, W, H, T, N, seed, zlo, zhi in KEY_SCENES:
        verts = posed_bodies(struct, regs, T, N, W, H, seed, zlo, zhi)
        win, keys = Selection(verts, faces, W, H).launch()
        assert int((keys[:, 0] != EMPTY).sum()) > 100, name
        d[name + '_verts'], d[name + '_win'], d[name + '_keys'] = verts, win, keys
    for n, v in fit_leaves(struct, regs, lbs_oracle.BodyModel(struct, regs), pathlib.Path(tempfile.mkdtemp())).items():
        d['fit_' + n] = v
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
