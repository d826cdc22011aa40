"""The compute-dtype switch of the dense 3x3 convolutions, ``Geom`` (the interned description of one convolution) and the
launch observer that bench.py and tools/step_layers.py count executed FLOPs with.

Drives no kernel: ``Geom`` asks the library which fast paths take a geometry.  The conv launchers of ``gan_lab_amd.ops`` are the
users; re-exported by ``gan_lab_amd.ops``."""
import ctypes

from .. import _lib
from .._lib import ConvGeom


# ---- compute dtype of the dense 3x3 convolutions ---------------------------------------------------
# 'f32' (default): exact fp32 MFMA, the reference's arithmetic.  'bf16': BASELINE config #2 "bf16 compute /
# fp32 master" - eligible 3x3 layers multiply bf16-rounded operands on v_mfma_f32_16x16x32_bf16 with fp32
# accumulation (csrc/conv_bf16.hip); tensors in HBM, parameters, optimiser state and every other kernel stay fp32.
_COMPUTE = ['f32']


def set_compute_dtype(name):
    if name not in ('f32', 'bf16'):
        raise ValueError("compute dtype must be 'f32' or 'bf16'")
    _COMPUTE[0] = name


def get_compute_dtype():
    return _COMPUTE[0]


class compute_dtype(object):
    """with ops.compute_dtype('bf16'): ... - graphs BUILT inside keep their kernels for the backward."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self._prev = _COMPUTE[0]
        set_compute_dtype(self.name)

    def __exit__(self, *exc):
        _COMPUTE[0] = self._prev
        return False


class Geom:
    """Static description of one convolution (mirrors ganlab_conv_geom) + derived output size.
    ``up``: nearest 2x upsample folded in front; ``pool``: 2x2 average pool folded behind (stride-2
    fused kernels, csrc/conv_s2.hip).  ``s2`` tells whether the stride-2 fast path applies."""
    __slots__ = ('N', 'Cin', 'Hin', 'Win', 'Cout', 'ks', 'pad', 'up', 'pool', 'Ho', 'Wo', 's2', '_c', 'bf', 'bf_fused')

    _CACHE = {}

    def __new__(cls, N, Cin, Hin, Win, Cout, ks, pad, up=0, pool=0):
        # a training step builds the same few dozen geometries again and again; each costs two ctypes structures and
        # two library queries, so they are interned (instances are immutable after construction).  An instance enters
        # the cache only once its construction has SUCCEEDED: a rejected geometry raises on every attempt.
        key = (int(N), int(Cin), int(Hin), int(Win), int(Cout), int(ks), int(pad), int(bool(up)), int(bool(pool)),
               _COMPUTE[0])
        g = cls._CACHE.get(key)
        if g is None:
            g = object.__new__(cls)
            g._c = None
            g._build(*key[:9])
            if len(cls._CACHE) > 4096:
                cls._CACHE.clear()
            cls._CACHE[key] = g
        return g

    def __init__(self, N, Cin, Hin, Win, Cout, ks, pad, up=0, pool=0):
        pass            # built (and validated) in __new__

    def _build(self, N, Cin, Hin, Win, Cout, ks, pad, up, pool):
        if ks not in (1, 3):
            raise ValueError('conv kernels support ks in {1, 3}; a 4x4 valid conv runs as a linear')
        self.N, self.Cin, self.Hin, self.Win, self.Cout, self.ks, self.pad, self.up, self.pool = \
            int(N), int(Cin), int(Hin), int(Win), int(Cout), int(ks), int(pad), int(bool(up)), int(bool(pool))
        hv, wv = (2 * Hin, 2 * Win) if up else (Hin, Win)
        self.Ho, self.Wo = hv + 2 * pad - ks + 1, wv + 2 * pad - ks + 1
        if self.pool:
            self.Ho, self.Wo = self.Ho // 2, self.Wo // 2
        cg = ConvGeom(self.N, self.Cin, self.Hin, self.Win, self.Cout, self.ks, self.pad, self.up, self.pool)
        # bf16 compute mode (decided HERE, so a backward that runs outside the `compute_dtype` block still uses the
        # kernels its forward used).  ``bf``: the plain geometry at the resolution of the taps (what the weight-gradient
        # kernels take, on a materialised upsample of x or of the pooled layer's gy); ``bf_fused``: this geometry with
        # its up / pool flag - the forward and input-gradient kernels fold the resampling in
        self.bf = self.bf_fused = None
        if _COMPUTE[0] == 'bf16':
            v = ConvGeom(self.N, self.Cin, hv, wv, self.Cout, self.ks, self.pad, 0, 0)
            if _lib.lib().ganlab_conv_bf16_supported(ctypes.byref(v)):
                self.bf = v
                if (self.up or self.pool) and _lib.lib().ganlab_conv_bf16_supported(ctypes.byref(cg)):
                    self.bf_fused = cg
                elif self.pool:
                    self.bf = None
        self.s2 = bool(self.bf is None and (self.up or self.pool) and
                       _lib.lib().ganlab_conv_s2_supported(ctypes.byref(cg)))
        if self.pool and not self.s2 and self.bf_fused is None:
            raise ValueError('pool=1 geometry is not supported by the stride-2 kernels; compose conv + pool')
        self._c = cg

    def ref(self):
        return ctypes.byref(self._c)

    @property
    def in_shape(self):
        return (self.N, self.Cin, self.Hin, self.Win)

    @property
    def out_shape(self):
        return (self.N, self.Cout, self.Ho, self.Wo)


def pool_fusable(N, Cin, Hin, Win, Cout, ks, pad):
    """Whether conv(ks, pad) followed by AvgPool2d(2) can run as ONE stride-2 kernel."""
    if ks != 3 or pad != 1:
        return False
    if _COMPUTE[0] == 'bf16':
        v = ConvGeom(int(N), int(Cin), int(Hin), int(Win), int(Cout), 3, 1, 0, 1)
        if _lib.lib().ganlab_conv_bf16_supported(ctypes.byref(v)):
            return True         # the bf16 kernel sums the 2 x 2 outputs in its epilogue
    c = ConvGeom(int(N), int(Cin), int(Hin), int(Win), int(Cout), 3, 1, 0, 1)
    return bool(_lib.lib().ganlab_conv_s2_supported(ctypes.byref(c)))


# ---- launch observer (measurement only) -------------------------------------------------------------
# bench.py / tools/step_layers.py count the convolution FLOPs the step actually EXECUTES (stride-2 fused layers run
# 16 low-resolution taps instead of 4 x 9, the shared D(real) forward and the skipped weight gradients never launch)
# by registering a callable here; every conv launcher reports (kind, Geom) to it.  None = no overhead.
_OBSERVER = [None]


def set_launch_observer(fn):
    prev = _OBSERVER[0]
    _OBSERVER[0] = fn
    return prev


def conv_flops(g):
    """FLOPs one pass (forward, input gradient or weight gradient) over geometry ``g`` executes in this library."""
    if g.s2:
        lo_h, lo_w = (g.Hin, g.Win) if g.up else (g.Ho, g.Wo)
        return 2.0 * 16 * g.Cin * g.Cout * lo_h * lo_w * g.N
    if g.bf is not None:       # bf16 layers run all 9 taps at the taps' resolution, also with a folded upsample / pool
        return 2.0 * g.ks * g.ks * g.Cin * g.Cout * g.bf.Hin * g.bf.Win * g.N
    return 2.0 * g.ks * g.ks * g.Cin * g.Cout * g.Ho * g.Wo * g.N


def _note(kind, g):
    if _OBSERVER[0] is not None:
        _OBSERVER[0](kind, g)
