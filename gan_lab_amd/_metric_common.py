"""What the set metrics' modules (swd, msssim, spectrum, prdc, frechet, kid, ppl) share word for word; ``prefix`` is the module's
name as its messages open with it.  The table of the metrics and the learners' side of them is validation.py."""
import os

import torch


def wanted(metrics, name):
    """Does ``metrics`` (a config's gen_metrics / disc_metrics, or None) list ``name``, in any letter case?"""
    return any(isinstance(m, str) and m.casefold() == name for m in (metrics or ()))


def device_gate(device, prefix):
    """(torch.device, host_only) of an evaluation object.  GANLAB_HOST_LOGIC_ONLY=1 (CPU tests of the host logic) lets one stand
    on a CPU device: feeds are checked and counted, nothing is computed."""
    dev = torch.device(device)
    host_only = dev.type != 'cuda' and os.environ.get('GANLAB_HOST_LOGIC_ONLY') == '1'
    if dev.type != 'cuda' and not host_only:
        raise TypeError(f'{prefix}: the metric runs on the GPU only (device={device!r}); the HIP path has no CPU fallback')
    return dev, host_only


def host_only_error(prefix):
    return RuntimeError(f'{prefix}: GANLAB_HOST_LOGIC_ONLY=1 checks the host logic only; the metric itself needs the GPU')


def check_rows(rows, dim, prefix):
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[1] != dim or rows.dtype != torch.float32:
        raise ValueError(f'{prefix}: a feed must be an (n, {dim}) float32 matrix, got '
                         f'{tuple(getattr(rows, "shape", ()))} {getattr(rows, "dtype", type(rows).__name__)}')
