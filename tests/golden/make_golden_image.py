"""Golden fixture for the stand-alone image-space modules: the reference's own ``Erode2D`` / ``Dilate2D``
(morphology.py:6-41) at kernel sizes 1, 3, 5 and 7 on maps smaller and larger than the window, and its two loss builders
(losses.py:19-40) with the gradients of BOTH tensor arguments -- shared and per-person targets and masks, pixels below, at
and above the clamp, zero and negative ones, masks that are not binary, a broadcast second argument.
Only in the build container (the reference is loaded in place, as ``make_golden.py`` does); writes numbers only.

    python tests/golden/make_golden_image.py
"""
import importlib
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), 'scene-aware-3d-multi-human_amd'))
import golden_inputs as gi  # noqa: E402
import make_golden as mg  # noqa: E402


def main():
    assert os.path.isdir(mg.REF), 'reference not present: fixtures can only be regenerated in the build container'
    sys.argv = ['x']
    mg._install_stubs()
    mg._ref_package()
    losses = importlib.import_module('refmh.losses')
    morph = importlib.import_module('refmh.morphology')
    torch.set_num_threads(1)
    out = {}
    for (H, W), x in gi.image_morph_inputs().items():
        for k in gi.IMAGE_MORPH_KSIZES:
            out['erode_%dx%d_k%d' % (H, W, k)] = morph.Erode2D(kernel_size=k)(torch.tensor(x)).numpy()
            out['dilate_%dx%d_k%d' % (H, W, k)] = morph.Dilate2D(kernel_size=k)(torch.tensor(x)).numpy()
    for name, (pred, true, mask) in gi.image_depth_loss_cases().items():
        tp, tt = torch.tensor(pred, requires_grad=True), torch.tensor(true, requires_grad=True)
        l = losses.build_avg_depth_loss_fn()(tp, tt, torch.tensor(mask))
        l.backward()
        out['depth_%s' % name] = l.detach().numpy()
        out['depth_%s_gpred' % name] = tp.grad.numpy().copy()
        out['depth_%s_gtrue' % name] = tt.grad.numpy().copy()
    for name, (y1, y2, mask) in gi.image_mse_cases().items():
        t1, t2 = torch.tensor(y1, requires_grad=True), torch.tensor(y2, requires_grad=True)
        l = losses.build_masked_mse_loss_fn()(t1, t2, torch.tensor(mask))
        l.backward()
        out['mse_%s' % name] = l.detach().numpy()
        out['mse_%s_g1' % name] = t1.grad.numpy().copy()
        out['mse_%s_g2' % name] = t2.grad.numpy().copy()
    path = os.path.join(HERE, 'reference_image_cpu.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB,', len(out), 'arrays')


if __name__ == '__main__':
    main()
