"""Test infrastructure: the tile weight gradient of csrc/conv_bf16.hip in a process of its own.

``GANLAB_BF16_WGRAD_ROLL`` is read once per process, so ``conv_wgrad_bf16_kernel`` and ``wgrad_bf16_reduce_kernel`` only run in a
process started with it set to 0.  tests/test_gpu_bf16_kernels.py starts this file once, with the variable added to its own
environment, and compares what it writes: for every ``tile`` row of tests/bf16_forms.py (and every distribution the row runs
under) the weight gradient and the (symbol, workgroups) launches, and for the up / pooled rows what the library answers to the
fused geometry - no workspace and GANLAB_EUNSUPPORTED, after which ``ops.k_conv_wgrad`` takes its materialising path.

    python tests/bf16_tile_wgrad_worker.py <outputs.pt>
"""
import ctypes
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def run():
    assert os.environ.get('GANLAB_BF16_WGRAD_ROLL') == '0', 'start this worker with GANLAB_BF16_WGRAD_ROLL=0'
    import bf16_forms as B
    import x3_forms as X
    from gan_lab_amd import _lib, ops
    L = _lib.lib()
    out = {'rows': {}, 'fused': {}}
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    for name, f in B.ROWS.items():
        if not f.tile:
            continue
        g = f.geom(ops)
        if f.kind != 'plain':
            assert g.bf_fused is not None
            T = X.to_gpu(X.draw(f, 'randn'))
            gw, ws = torch.zeros(f.co, f.ci, 3, 3, device='cuda'), torch.zeros(1 << 20, device='cuda')
            c0 = _lib.launch_count()
            rc = L.ganlab_conv_wgrad_bf16(p(T.gy), p(T.x), p(gw), ctypes.byref(g.bf_fused), f.scale, p(ws), ws.numel() * 4, None)
            out['fused'][name] = dict(workspace=int(L.ganlab_conv_wgrad_bf16_workspace(ctypes.byref(g.bf_fused))), rc=int(rc),
                                      launched=_lib.launch_count() - c0)
        for dist in ('randn',) + (X.DISTS if f.dists else ()):
            (gw,), launches = B.run(ops, f, X.draw(f, dist))
            out['rows']['%s|%s' % (name, dist)] = dict(gw=gw, launches=launches)
    return out


if __name__ == '__main__':
    dst = sys.argv[1]
    torch.save(run(), dst + '.tmp')
    os.replace(dst + '.tmp', dst)
