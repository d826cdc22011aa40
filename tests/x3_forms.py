"""One layer form of the split-product (3 x bf16) conv kernels, run three ways: on the split-product kernel, on the exact-fp32
kernel of the same entry point (``ops.set_x3(False)``) and in float64 on the CPU - with the operands drawn from the
distributions a training step feeds these kernels, not from ``randn`` alone.  Lifted from tests/test_gpu_x3.py, which runs the
same forms inline; tests/test_gpu_x3_operands.py is the user.

A form is a ``Form`` record: its geometry, the operands it needs, its GPU call and its float64 restatement.  ``draw`` makes the
operands of a form under one distribution (CPU, fp32, seeded), ``run_three_ways`` returns the three results and the kernel
symbols each GPU run launched.  Nothing here asserts a bar: that is the test's business."""
import collections
import contextlib
import ctypes
import zlib

import torch
import torch.nn.functional as F

TOL = 2e-4                  # the accuracy bar of the fp32 kernels (tests/test_gpu_ops.py, tests/test_gpu_x3.py)
WGRAD_FLOOR = 2.5e-7        # ATen's own weight-gradient error level (tools/op_error_probe.py; tests/test_gpu_x3.py)


@contextlib.contextmanager
def x3_at_any_size(ops):
    """The split-product kernels on these small cases too: no minimum tile count for the launch."""
    old_min, ops._X3_MIN_TILES = ops._X3_MIN_TILES, 1
    try:
        yield
    finally:
        ops._X3_MIN_TILES = old_min


def rms_rel(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return ((a - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def launched(ops):
    from gan_lab_amd import _lib
    return _lib.last_launch()[0] or ''


# ---- the forms --------------------------------------------------------------------------------------------------------------------
# kind: 'plain' (H x W in and out), 'up' (hl x wl in, 2hl x 2wl out), 'pool' (2hl x 2wl in, hl x wl out); role: which operand
# the kernel streams beside the weights - 'fwd' (the activation), 'dgrad' (gy), 'wgrad' (both, no weights)
class Form(object):
    def __init__(self, name, kind, role, shape, symbol, scale, needs, gpu, ref, outs=('y',), aff=False, tail=False):
        self.name, self.kind, self.role, self.shape, self.symbol, self.scale = name, kind, role, tuple(shape), symbol, scale
        self.needs, self.gpu, self.ref, self.outs, self.aff, self.tail = needs, gpu, ref, outs, aff, tail
        self.n, self.ci, self.co, h, w = self.shape
        self.hw_in = (2 * h, 2 * w) if kind == 'pool' else (h, w)
        self.hw_out = (2 * h, 2 * w) if kind == 'up' else (h, w)

    def at(self, shape):
        """the same form at another shape"""
        return Form(self.name, self.kind, self.role, shape, self.symbol, self.scale, self.needs, self.gpu, self.ref, self.outs,
                    self.aff, self.tail)

    def geom(self, ops):
        return ops.Geom(self.n, self.ci, self.hw_in[0], self.hw_in[1], self.co, 3, 1, up=int(self.kind == 'up'),
                        pool=int(self.kind == 'pool'))

    def x3_ok(self, ops, g):
        if self.role == 'wgrad':
            return ops.x3_wgrad_ok(g) if self.kind == 'plain' else ops.x3_s2_wgrad_ok(g)
        dgrad = self.role == 'dgrad'
        if self.symbol == 'conv_x3_fwd_kernel':
            return ops.x3_ok(g, dgrad)
        return ops.x3_s2_ok(g, dgrad) if self.symbol == 'conv_x3_up_kernel' else ops.x3_s2_down_ok(g, dgrad)

    def operand_shapes(self):
        n, ci, co, (hi, wi), (ho, wo) = self.n, self.ci, self.co, self.hw_in, self.hw_out
        return dict(x=(n, ci, hi, wi), gy=(n, co, ho, wo), wt=(co, ci, 3, 3), b=(co,), s=(n, ci), t=(n, ci), nz=(n, 1, ho, wo),
                    nw=(co,))


BIAS_SCALE, TAIL_BIAS_SCALE, SLOPE, EPS = 0.5, 0.7, 0.2, 1e-8


def _bias(v, k=BIAS_SCALE):
    return k * v.view(1, -1, 1, 1)


def _affine(T, n, ci):
    return T.x * T.s.view(n, ci, 1, 1) + T.t.view(n, ci, 1, 1)


def _up2(v):
    return F.interpolate(v, scale_factor=2, mode='nearest')


def _conv_ref(f, x, wt, scale=None):
    """the layer's linear part in the dtype of its arguments: conv, upsample + conv, conv + average pool"""
    if f.kind == 'up':
        x = _up2(x)
    y = F.conv2d(x, wt * (f.scale if scale is None else scale), None, padding=1)
    return F.avg_pool2d(y, 2) if f.kind == 'pool' else y


def _dgrad_ref(f, T):
    xd = torch.zeros(f.n, f.ci, *f.hw_in, dtype=T.gy.dtype, requires_grad=True)
    gx, = torch.autograd.grad(_conv_ref(f, xd, T.wt), xd, T.gy)
    return gx


def _wgrad_ref(f, T):
    wd = torch.zeros(f.co, f.ci, 3, 3, dtype=T.gy.dtype, requires_grad=True)
    gw, = torch.autograd.grad(_conv_ref(f, _affine(T, f.n, f.ci) if f.aff else T.x, wd, 1.0), wd, T.gy)
    return gw * f.scale


# GPU calls: (ops, form, geom, T, x3) -> tuple of outputs; T: the operands on the GPU.  `x3`: which of the two runs this is -
# only the layer tail, which picks its entry point itself, looks at it.
def _gpu_fwd(ops, f, g, T, x3):
    return ops.k_conv_fwd(T.x, T.wt, T.b, g, f.scale, BIAS_SCALE, ops.ACT_LRELU, SLOPE),


def _ref_fwd(f, T):
    return F.leaky_relu(_conv_ref(f, T.x, T.wt) + _bias(T.b), SLOPE),


def _gpu_dgrad(ops, f, g, T, x3):
    return ops.k_conv_dgrad(T.gy, T.wt, g, f.scale),


def _ref_dgrad(f, T):
    return _dgrad_ref(f, T),


def _gpu_dgrad_mask(ops, f, g, T, x3):
    return ops.k_conv_dgrad_mask(T.gy, T.wt, T.x, g, f.scale, SLOPE),


def _ref_dgrad_mask(f, T):
    return _dgrad_ref(f, T) * torch.where(T.x > 0, 1.0, SLOPE).to(T.gy.dtype),


def _gpu_fwd_aff(ops, f, g, T, x3):
    return ops.k_conv_fwd_aff(T.x, T.s, T.t, T.wt, g, f.scale),


def _ref_fwd_aff(f, T):
    return _conv_ref(f, _affine(T, f.n, f.ci), T.wt),


def _gpu_tail(ops, f, g, T, x3):
    """the whole layer: y = lrelu(conv(a*s + t) + noise_w * noise + bias) and the InstanceNorm statistics of y"""
    from gan_lab_amd import _lib
    L = _lib.lib()
    n, co, (h, w) = f.n, f.co, f.hw_out
    p = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None
    y = torch.empty(n, co, h, w, device='cuda')
    mean, rstd = torch.empty(n, co, device='cuda'), torch.empty(n, co, device='cuda')
    nz, nw = getattr(T, 'nz', None), getattr(T, 'nw', None)
    if x3:
        chunks = L.ganlab_conv_fwd_aff_tail_x3_chunks(g.ref())
        assert chunks == (h // 16) * (w // 16) * 4
        ws = torch.empty(n * co * chunks * 2, dtype=torch.float64, device='cuda')
        wp = ops._packed_x3(T.wt, ops.PACK_FWD, f.scale)
        _lib.check(L.ganlab_conv_fwd_aff_tail_x3(p(T.x), p(wp), p(T.s), p(T.t), p(T.b), p(nz), p(nw), p(y), p(mean), p(rstd), g.ref(),
                                                 TAIL_BIAS_SCALE, ops.ACT_LRELU, SLOPE, EPS, p(ws), ws.numel() * 8, None), 'tail x3')
    else:
        chunks = L.ganlab_conv_fwd_aff_tail_chunks(g.ref())
        assert chunks > 0
        ws = torch.empty(n * co * chunks * 2, dtype=torch.float64, device='cuda')
        wp = ops._packed(T.wt, ops.PACK_FWD, f.scale)
        _lib.check(L.ganlab_conv_fwd_aff_tail_f32(p(T.x), p(wp), p(T.s), p(T.t), p(T.b), p(nz), p(nw), p(y), p(mean), p(rstd), g.ref(),
                                                  TAIL_BIAS_SCALE, ops.ACT_LRELU, SLOPE, EPS, p(ws), ws.numel() * 8, None),
                   'tail exact')
    return y, mean, rstd


def _ref_tail(f, T):
    pre = _conv_ref(f, _affine(T, f.n, f.ci), T.wt) + _bias(T.b, TAIL_BIAS_SCALE)
    if hasattr(T, 'nz'):
        pre = pre + T.nw.view(1, -1, 1, 1) * T.nz
    y = F.leaky_relu(pre, SLOPE)
    return y, y.mean(dim=(2, 3)), 1.0 / torch.sqrt(y.var(dim=(2, 3), unbiased=False) + EPS)


def _gpu_wgrad(ops, f, g, T, x3):
    if f.aff:       # (at the shapes used here the exact-fp32 affine-on-load kernels take the geometry too)
        return ops.k_conv_wgrad_aff(T.gy, T.x, T.s, T.t, g, f.scale),
    return ops.k_conv_wgrad(T.gy, T.x, g, f.scale),


def _ref_wgrad(f, T):
    return _wgrad_ref(f, T),


def _forms():
    fwd, dg, wg = ('x', 'wt', 'b'), ('gy', 'wt'), ('x', 'gy')
    aff = ('x', 's', 't', 'wt')
    x3f, x3u, x3d = 'conv_x3_fwd_kernel', 'conv_x3_up_kernel', 'conv_x3_down_kernel'
    unit = lambda ci: 1.0 / (3 * ci ** 0.5)
    fs = [
        # N, Cin, Cout, H, W of the layer (up / pool: its low resolution); the shapes are cases of tests/test_gpu_x3.py
        Form('fwd', 'plain', 'fwd', (3, 128, 192, 32, 16), x3f, unit(128), fwd, _gpu_fwd, _ref_fwd),
        Form('dgrad', 'plain', 'dgrad', (3, 128, 192, 32, 16), x3f, unit(128), dg, _gpu_dgrad, _ref_dgrad),
        Form('dgrad_mask', 'plain', 'dgrad', (3, 128, 64, 32, 32), x3f, 0.03, dg + ('x',), _gpu_dgrad_mask, _ref_dgrad_mask),
        Form('fwd_aff', 'plain', 'fwd', (3, 128, 128, 32, 32), x3f, 0.02, aff, _gpu_fwd_aff, _ref_fwd_aff, aff=True),
        Form('fwd_aff_tail', 'plain', 'fwd', (3, 128, 128, 32, 32), x3f, 0.02, aff + ('b', 'nz', 'nw'), _gpu_tail, _ref_tail,
             outs=('y', 'mean', 'rstd'), aff=True, tail=True),
        Form('up_fwd', 'up', 'fwd', (3, 128, 64, 32, 16), x3u, unit(128), fwd, _gpu_fwd, _ref_fwd),
        Form('up_fwd_aff', 'up', 'fwd', (3, 128, 64, 32, 16), x3u, unit(128), aff, _gpu_fwd_aff, _ref_fwd_aff, aff=True),
        Form('pool_dgrad', 'pool', 'dgrad', (3, 64, 128, 32, 16), x3u, unit(64), dg, _gpu_dgrad, _ref_dgrad),
        Form('pool_fwd', 'pool', 'fwd', (3, 128, 256, 8, 32), x3d, unit(128), fwd, _gpu_fwd, _ref_fwd),
        Form('up_dgrad', 'up', 'dgrad', (3, 256, 128, 8, 32), x3d, unit(256), dg, _gpu_dgrad, _ref_dgrad),
        Form('wgrad', 'plain', 'wgrad', (3, 128, 64, 16, 64), 'x3w_reduce_kernel', 0.013, wg, _gpu_wgrad, _ref_wgrad),
        Form('wgrad_aff', 'plain', 'wgrad', (3, 128, 64, 16, 64), 'x3w_reduce_kernel', 0.013, wg + ('s', 't'), _gpu_wgrad,
             _ref_wgrad, aff=True),
        Form('s2_wgrad_pool', 'pool', 'wgrad', (3, 64, 128, 16, 64), 'x3sw_reduce_kernel', 0.017, wg, _gpu_wgrad, _ref_wgrad),
        Form('s2_wgrad_up', 'up', 'wgrad', (3, 128, 64, 16, 64), 'x3sw_reduce_kernel', 0.017, wg, _gpu_wgrad, _ref_wgrad),
        Form('s2_wgrad_up_aff', 'up', 'wgrad', (3, 128, 64, 16, 64), 'x3sw_reduce_kernel', 0.017, wg + ('s', 't'), _gpu_wgrad,
             _ref_wgrad, aff=True),
    ]
    return collections.OrderedDict((f.name, f) for f in fs)


FORMS = _forms()


# ---- the operand distributions ----------------------------------------------------------------------------------------------------
DISTS = ('one_signed', 'offset', 'mixed_exponents', 'sparse', 'tiny', 'huge')
# tiny / huge: the power of two on the streamed operand.  The weights take 2^(-+2) with it, so a forward or input-gradient
# result sits near 2^(-+62) = 2e-19 / 5e18, inside [1e-20, 1e20]; a weight gradient takes 2^(-+60) on x and 2^(+-40) on gy
# (result near 2^(-+20)).  The layer tail squares its result for the variance in fp32: 2^(-+40), so that y^2 stays a normal fp32.
EXP_STREAM, EXP_TAIL, EXP_WEIGHT, EXP_WGRAD_GY = 60, 40, 2, 40


def activation_operand(f):
    """The operand that takes the activation-like draw: x (a under the affine) - the conv's input in the forward forms and the
    weight gradients, the mask source in the masked input gradient.  The plain input gradients have no activation among their
    operands: there `offset` and `sparse`, which name only the activation, go to the operand the kernel streams through the same
    staging code, gy (they would otherwise repeat the randn case).  `one_signed` has a draw of its own for gy."""
    return 'x' if 'x' in f.needs else 'gy'


def _subnormals(shape, g):
    """fp32 subnormals +-k * 2^-149, k < 2^23"""
    k = torch.randint(1, 2 ** 23, shape, generator=g, dtype=torch.int32)
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return k.view(torch.float32) * sign


def _sparsify(v, g):
    v = v.clone()
    v[torch.rand(v.shape, generator=g) < 0.5] = 0.0
    v[:, 1] = 0.0                   # one whole channel
    if v.shape[2] > 5:
        v[:, :, 5, :] = 0.0         # one whole image row
    pick = (v != 0) & (torch.rand(v.shape, generator=g) < 0.01)
    v[pick] = _subnormals(v.shape, g)[pick]
    return v


def draw(f, dist, seed=0):
    """The operands of form ``f`` under distribution ``dist``: a namespace of CPU fp32 tensors (f.needs)."""
    assert dist in DISTS + ('randn',), dist
    # (a form of another table - tests/exact_forms.py - takes a stream of its own, from its name)
    index = list(FORMS).index(f.name) if f.name in FORMS else len(FORMS) + zlib.crc32(f.name.encode()) % 100003
    g = torch.Generator().manual_seed(20011 + 97 * index + 7 * (DISTS + ('randn',)).index(dist) + seed)
    shp = f.operand_shapes()
    rn = lambda k: torch.randn(*shp[k], generator=g)
    d = {k: (torch.rand(*shp[k], generator=g) + 0.5 if k == 's' else rn(k)) for k in f.needs}
    act = activation_operand(f)
    if dist == 'one_signed':
        if 'x' in d:
            d['x'] = F.leaky_relu(rn('x'), SLOPE) + 0.5
        if 'gy' in d:
            d['gy'] = rn('gy') * torch.where(rn('gy') > 0, 1.0, 0.2)
    elif dist == 'offset':
        d[act] = 100.0 + rn(act)
        if 't' in d:
            d['t'] = 100.0 + rn('t')
    elif dist == 'mixed_exponents':
        for k in ('x', 'gy', 'wt'):
            if k in d:
                d[k] = rn(k) * torch.pow(2.0, torch.randint(-12, 13, shp[k], generator=g).float())
    elif dist == 'sparse':
        d[act] = _sparsify(d[act], g)
    elif dist in ('tiny', 'huge'):
        sg = -1 if dist == 'tiny' else 1
        if f.role == 'wgrad':
            e = dict(x=sg * EXP_STREAM, t=sg * EXP_STREAM, gy=-sg * EXP_WGRAD_GY)
        else:
            es = sg * (EXP_TAIL if f.tail else EXP_STREAM)
            ew = sg * EXP_WEIGHT
            e = dict(x=es, t=es, gy=es, wt=ew, b=es + ew, nw=es + ew)
        for k, p in e.items():
            if k in d:
                d[k] = d[k] * 2.0 ** p
    return collections.namedtuple('Operands', sorted(d))(**d)


def tail_near_constant_operands(f, ratio=30.0):
    """The layer tail's operands with a bias that puts |mean| / std of every output plane near ``ratio``: the case in which
    E[y^2] - mean^2 cancels (tests/test_gpu_ops.py test_instnorm_near_constant_planes guards it in the pointwise kernels).
    The size of the bias comes from the float64 conv of the same operands; its sign and a 10 % spread are drawn."""
    T = draw(f, 'randn')
    Td = T._replace(**{k: getattr(T, k).double() for k in T._fields})
    pre = _conv_ref(f, _affine(Td, f.n, f.ci), Td.wt) + Td.nw.view(1, -1, 1, 1) * Td.nz
    std = pre.std(dim=(2, 3)).mean(dim=0)           # per channel: the noise weight sets it
    g = torch.Generator().manual_seed(77)
    sign = torch.where(torch.rand(f.co, generator=g) < 0.5, -1.0, 1.0)
    b = sign * (ratio * std / TAIL_BIAS_SCALE) * (1.0 + 0.1 * torch.randn(f.co, generator=g))
    return T._replace(b=b.float())


# ---- running a form ---------------------------------------------------------------------------------------------------------------
Result = collections.namedtuple('Result', 'names x3 exact f64 launched_x3 launched_exact symbol')


def to_gpu(T):
    return T._replace(**{k: getattr(T, k).cuda() for k in T._fields})


def to_f64(T):
    return T._replace(**{k: getattr(T, k).double() for k in T._fields})


def _launches(fn):
    """fn()'s results and the kernel symbols it launched through the library (oldest first)"""
    from gan_lab_amd import _lib
    c0 = _lib.launch_count()
    out = fn()
    torch.cuda.synchronize()
    return out, [k or '' for k, _ in _lib.launches_since(c0)]


def run_x3(ops, f, T):
    """(outputs, launched symbols) of the split-product run alone; T: the operands on the GPU"""
    g = f.geom(ops)
    with x3_at_any_size(ops):
        assert ops.x3_enabled() and f.x3_ok(ops, g), (f.name, f.shape)
        return _launches(lambda: tuple(v.clone() for v in f.gpu(ops, f, g, T, True)))


def run_exact(ops, f, T):
    g = f.geom(ops)
    prev = ops.set_x3(False)
    try:
        return _launches(lambda: tuple(v.clone() for v in f.gpu(ops, f, g, T, False)))
    finally:
        ops.set_x3(prev)


def run_three_ways(ops, f, T):
    """Form ``f`` on operands ``T`` (CPU fp32, from ``draw``): split-product kernel, exact-fp32 kernel, float64 on the CPU."""
    Tg = to_gpu(T)
    y3, l3 = run_x3(ops, f, Tg)
    sym = launched(ops)
    y1, l1 = run_exact(ops, f, Tg)
    yd = tuple(v.detach() for v in f.ref(f, to_f64(T)))
    return Result(f.outs, tuple(v.cpu() for v in y3), tuple(v.cpu() for v in y1), yd, l3, l1, sym)


def ran(symbol, launches):
    return any(symbol in k for k in launches)
