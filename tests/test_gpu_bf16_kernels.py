"""The bf16-compute convolution kernels by name against float64 (tests/bf16_forms.py: one row per kernel per edge).

The kernels round their operands to bf16 and multiply exactly, so every reference runs on the operands rounded by
``bf16_forms.rne_bf16`` (the weight as rne(w * scale)) and only the fp32 summation order separates it from the kernel.  Every row:
  * the launches contain the row's kernel symbol, and every (symbol, workgroups) pair of the row's restated plan in order;
  * EXACT yardstick, ``randn``: within tests/test_gpu_bf16.py's own bars of float64 - 2e-5 forward, 5e-5 gradients (max error
    over the tensor's maximum, ``util.assert_close``);
  * RATIO yardstick: the rms error against float64 is at most ``row.factor`` (2, exact_forms' factor) x that of fp32 ATen on the
    CPU on the same rounded operands; weight gradients: or x3_forms.WGRAD_FLOOR.
The rows marked ``dists`` - one per kernel instantiation, its most edge-laden geometry, the odd-RS and ragged split-K rows among
them - run again under every distribution of x3_forms.DISTS at the ratio yardstick and x3_forms.TOL.  One +inf, NaN or fp32
maximum (inf once rounded) must stay where linear algebra puts it.  ``pack_bf16_kernel`` is compared bit for bit.  The tile weight
gradient runs in a child process with GANLAB_BF16_WGRAD_ROLL=0 (tests/bf16_tile_wgrad_worker.py).  A HIP error, a child that
dies of a signal or one that runs into its time limit ends the session: nothing more is started on a device that has faulted.
Measured worst ratios per kernel instantiation: DESIGN.md section 4.0."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import bf16_forms as B
import x3_forms as X
from util import assert_close, rel_err
from x3_forms import TOL, WGRAD_FLOOR, rms_rel

pytestmark = pytest.mark.gpu

SEEN = set()                # normalised symbols of every launch the rows of this file made
WORKER_LIMIT = 300          # seconds: a python start, the library load and 11 small weight gradients take about 30


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from gan_lab_amd import ops as _ops, _lib
    _lib.lib()
    return _ops


def run_gpu(ops, f, T):
    """B.run; a HIP error ends the whole session - nothing more is started on a device that has faulted"""
    try:
        got, launches = B.run(ops, f, T)
    except RuntimeError as e:
        if 'HIP' in str(e) or 'hip' in str(e):
            pytest.exit(f'{f.name}: {e}', returncode=3)
        raise
    SEEN.update(k for k, _ in launches)
    return got, launches


def judge(name, dist, got, launches):
    """the bars of one run of row ``name``: ``got`` its outputs (CPU), ``launches`` what it launched"""
    f = B.ROWS[name]
    print(f'BF16 {name} {dist}: launched {launches}')
    assert any(B.norm(f.symbol) in k for k, _ in launches), (name, f.symbol, launches)
    assert B.plan_found(f.plan, launches), (name, f.plan, launches)
    R = B.round_operands(f, X.draw(f, dist))
    (y,), (yd,), (ya,) = got, f.ref(f, X.to_f64(R)), f.define(f, R)
    yd, ya, out = yd.detach(), ya.detach(), f.outs[0]
    assert ya.dtype == torch.float32 and torch.isfinite(yd).all(), (name, dist)
    if dist in ('tiny', 'huge'):       # (util.rel_err floors its denominator at 1e-30)
        assert 1e-20 <= yd.pow(2).mean().sqrt().item() <= 1e20 and yd.abs().max().item() <= 1e20, (name, dist)
    ek, ea = rms_rel(y, yd), rms_rel(ya, yd)
    print(f'BF16 {name} {dist} {out}: rms vs float64 kernel {ek:.3e} ATen {ea:.3e} ratio {ek / max(ea, 1e-300):.2f} | '
          f'max-rel vs float64 {rel_err(y, yd):.2e} | launched {f.symbol} grid {f.plan[0][1]}')
    assert torch.isfinite(y).all(), (name, dist)
    assert_close(y, yd, f.tol if dist == 'randn' else TOL, f'{name} {dist} {out} vs float64 on the rounded operands')
    bar = max(f.factor * ea, WGRAD_FLOOR) if f.role == 'wgrad' else f.factor * ea
    assert ek <= bar, (name, dist, ek, ea, f.factor)


def check_row(ops, name, dist):
    got, launches = run_gpu(ops, B.ROWS[name], X.draw(B.ROWS[name], dist))
    judge(name, dist, got, launches)


MAIN = [n for n, r in B.ROWS.items() if not r.tile]
TILE = [n for n, r in B.ROWS.items() if r.tile]


@pytest.mark.parametrize('name', MAIN)
def test_bf16_kernel_row(ops, name):
    check_row(ops, name, 'randn')


@pytest.mark.parametrize('dist', X.DISTS)
@pytest.mark.parametrize('name', [n for n in MAIN if B.ROWS[n].dists])
def test_bf16_kernel_on_training_like_operands(ops, name, dist):
    check_row(ops, name, dist)


# ---- non-finite values stay where linear algebra puts them ---------------------------------------------------------------------------
# One +inf, NaN or fp32 maximum - finite in fp32, inf once rounded to bf16 - in image 0 of the streamed operand (gy of an input
# gradient, else x), in the last row and column of a tile or strip.  The affected SET is where the float64 result on the rounded
# operands is non-finite; elsewhere the result is bit-equal to the clean run.
@pytest.mark.parametrize('value', [float('inf'), float('nan'), B.FP32_MAX], ids=['inf', 'nan', 'fp32max'])
@pytest.mark.parametrize('name,pixel', B.NONFINITE, ids=[c[0] for c in B.NONFINITE])
def test_bf16_non_finite_stays_where_linear_algebra_puts_it(ops, name, pixel, value):
    f = B.ROWS[name]
    clean = X.draw(f, 'randn')
    which = 'gy' if f.role == 'dgrad' else 'x'
    v = getattr(clean, which).clone()
    assert v.shape[0] >= 2 and v.shape[2] > pixel[0] and v.shape[3] > pixel[1]
    v[0, B.POISON_CHANNEL, pixel[0], pixel[1]] = value
    assert torch.isfinite(v).all() == (value == B.FP32_MAX)
    bad = clean._replace(**{which: v})
    ref, = f.ref(f, X.to_f64(B.round_operands(f, bad)))
    affected = ~torch.isfinite(ref)
    if f.role == 'wgrad':       # the rows of the poisoned input channel, and nothing else
        want = torch.zeros_like(affected)
        want[:, B.POISON_CHANNEL] = True
        assert torch.equal(affected, want)
    else:                       # a neighbourhood of the pixel in image 0, in every channel
        assert affected[0].any() and not affected[1:].any() and affected.sum().item() <= 64 * affected.shape[1]
    (y_clean,), l0 = run_gpu(ops, f, clean)
    (y_bad,), l1 = run_gpu(ops, f, bad)
    assert B.plan_found(f.plan, l0) and B.plan_found(f.plan, l1), (name, l0, l1)
    assert torch.isfinite(y_clean).all()
    got = ~torch.isfinite(y_bad)
    print(f'BF16 non-finite {name} {value}: reference non-finite at {int(affected.sum())} elements, kernel at {int(got.sum())}; '
          f'NaN among them {int(torch.isnan(y_bad).sum())} | launched {f.symbol}')
    assert torch.equal(got, affected), (int(got.sum()), int(affected.sum()), int((got ^ affected).sum()))
    assert torch.equal(y_bad[~affected], y_clean[~affected])


# ---- pack_bf16_kernel, bit for bit ---------------------------------------------------------------------------------------------------
def bf16_nan(bits):
    return ((bits & 0x7F80) == 0x7F80) & ((bits & 0x7F) != 0)


@pytest.mark.parametrize('scale', [1.0, B.f32(1.0 / 24.0)], ids=['scale1', 'scale24th'])
@pytest.mark.parametrize('name,mode,cout,cin', B.PACK_ROWS, ids=[c[0] for c in B.PACK_ROWS])
def test_bf16_pack_bit_for_bit(ops, name, mode, cout, cin, scale):
    """``_packed_bf16`` as int16 against the restated layout [chunk][tap][kg][CO][8] of rne_bf16(w * scale).  Planted in w: ties
    with an even and an odd low kept bit, both signs; fp32's maximum and the first value that rounds up to inf; subnormals; a NaN
    (compared as NaN).  At scale 1 the product is w itself and the planted values reach the rounding as they are."""
    from gan_lab_amd import _lib
    g = torch.Generator().manual_seed(11 + mode)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    plant = B.from_bits(torch.tensor([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001,        # ties and neighbours
                                    0x7F7FFFFF, 0x7F7F8000, 0xFF7F8000, 0x7F7F7FFF,                                  # overflow, and not
                                    0x00000001, 0x00008000, 0x00018000, 0x807FFFFF, 0x00400000,                      # subnormals
                                    0x7FC00000, 0x7F800001]))                                                        # NaN
    where = torch.randperm(w.numel(), generator=g)[:plant.numel()]
    w.view(-1)[where] = plant
    wg = w.cuda()
    c0 = _lib.launch_count()
    packed = ops._packed_bf16(wg, mode, scale)
    torch.cuda.synchronize()
    launches = [(B.norm(k or ''), n) for k, n in _lib.launches_since(c0)]
    SEEN.update(k for k, _ in launches)
    n = 9 * cout * cin
    print(f'BF16 {name} scale {scale}: launched {launches}')
    assert packed.dtype == torch.bfloat16 and packed.numel() == n
    assert any('pack_bf16_kernel' in k and grid == min(B.cdiv(n, 256), 4096) for k, grid in launches), launches
    got = packed.view(torch.int16).cpu().to(torch.int32) & 0xFFFF
    want = B.bf16_bits(B.pack_layout(B.rne_bf16(w * scale), mode)).reshape(-1).to(torch.int32) & 0xFFFF
    nan = bf16_nan(want)
    assert int(nan.sum()) == 2 and torch.equal(bf16_nan(got), nan)
    diff = (got != want) & ~nan
    assert not diff.any(), (int(diff.sum()), [(hex(a), hex(b)) for a, b in zip(got[diff][:8].tolist(), want[diff][:8].tolist())])
    if scale == 1.0:
        assert int((want == 0x7F80).sum()) == 2 and int((want == 0xFF80).sum()) == 1      # the overflows became inf


# ---- the tile weight gradient: a child process with GANLAB_BF16_WGRAD_ROLL=0 ---------------------------------------------------------
@pytest.fixture(scope='module')
def tile_run(ops, tmp_path_factory):
    dst = str(tmp_path_factory.mktemp('bf16_tile') / 'out.pt')
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'bf16_tile_wgrad_worker.py')
    env = dict(os.environ, GANLAB_BF16_WGRAD_ROLL='0')
    try:
        res = subprocess.run([sys.executable, worker, dst], env=env, capture_output=True, text=True, timeout=WORKER_LIMIT)
    except subprocess.TimeoutExpired:
        pytest.exit(f'the tile weight-gradient worker ran into its limit of {WORKER_LIMIT} s', returncode=3)
    if res.returncode < 0 or res.returncode in (134, 139):
        pytest.exit(f'the tile weight-gradient worker died ({res.returncode}):\n{res.stderr[-2000:]}', returncode=3)
    if res.returncode != 0 and ('HIP' in res.stderr or 'hip' in res.stderr):
        pytest.exit(f'the tile weight-gradient worker met a HIP error:\n{res.stderr[-2000:]}', returncode=3)
    assert res.returncode == 0, res.stderr[-4000:]
    out = torch.load(dst, weights_only=False)
    for rec in out['rows'].values():
        SEEN.update(k for k, _ in rec['launches'])
    return out


@pytest.mark.parametrize('name', TILE)
def test_bf16_tile_wgrad_row(tile_run, name):
    rec = tile_run['rows'][f'{name}|randn']
    judge(name, 'randn', (rec['gw'],), rec['launches'])
    assert not any('roll' in k for k, _ in rec['launches']), rec['launches']


@pytest.mark.parametrize('dist', X.DISTS)
@pytest.mark.parametrize('name', [n for n in TILE if B.ROWS[n].dists])
def test_bf16_tile_wgrad_on_training_like_operands(tile_run, name, dist):
    rec = tile_run['rows'][f'{name}|{dist}']
    judge(name, dist, (rec['gw'],), rec['launches'])


def test_bf16_tile_process_refuses_fused_geometries(tile_run):
    """with the rolling kernel off bf16_wgrad_ok refuses up and pool: no workspace, GANLAB_EUNSUPPORTED, nothing launched - and
    ops.k_conv_wgrad then ran the tile kernel at the taps' resolution (the rows above)"""
    assert sorted(tile_run['fused']) == ['tile_pool_other_path', 'tile_up_other_path']
    for name, rec in tile_run['fused'].items():
        assert rec == dict(workspace=0, rc=-4, launched=0), (name, rec)
        assert B.plan_found(B.ROWS[name].plan, tile_run['rows'][f'{name}|randn']['launches'])


# ---- argument checks that return codes without launching -----------------------------------------------------------------------------
def test_bf16_entry_points_check_workspace_and_geometry(ops):
    from gan_lab_amd import _lib
    L, G = _lib.lib(), _lib.ConvGeom
    EWORKSPACE, EUNSUPPORTED = -2, -4
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    z = lambda *s: torch.zeros(*s, device='cuda')
    n, ci, co, h, w = 1, 448, 64, 16, 16
    x, gy, b = z(n, ci, h, w), z(n, co, h, w), z(co)
    wt = z(co, ci, 3, 3)
    wf, wd = ops._packed_bf16(wt, B.PACK_FWD, 1.0), ops._packed_bf16(wt, B.PACK_DGRAD, 1.0)
    torch.cuda.synchronize()
    g = G(n, ci, h, w, co, 3, 1, 0, 0)
    assert L.ganlab_conv_bf16_splitk_plan(ctypes.byref(g), 0) == 3 == B.bf16_splitk_plan(n, ci, co, h, w)
    need = 3 * n * co * h * w * 4
    ws = z(need // 4)
    y = z(n, co, h, w)
    gyd, gxd, wdd = z(n, ci, h, w), z(n, co, h, w), ops._packed_bf16(z(ci, co, 3, 3), B.PACK_DGRAD, 1.0)
    torch.cuda.synchronize()
    c0 = _lib.launch_count()
    args =(p(x), p(wf), p(b), p(y), ctypes.byref(g), 0.5, ops.ACT_LRELU, 0.2)
    assert L.ganlab_conv_fwd_bf16_splitk(*args, p(ws), need - 1, None) == EWORKSPACE
    assert L.ganlab_conv_fwd_bf16_splitk(*args, None, need, None) == EWORKSPACE
    # the input gradient of the layer with the channels swapped contracts the 448 channels
    gd = G(n, co, h, w, ci, 3, 1, 0, 0)
    assert L.ganlab_conv_bf16_splitk_plan(ctypes.byref(gd), 1) == 3 and L.ganlab_conv_bf16_splitk_plan(ctypes.byref(gd), 0) == 1
    assert L.ganlab_conv_dgrad_bf16_splitk(p(gyd), p(wdd), p(gxd), ctypes.byref(gd), p(ws), need - 1, None) == EWORKSPACE
    # the weight gradient
    gw_geom = G(2, 64, 8, 32, 64, 3, 1, 0, 0)
    xw, gyw, gw = z(2, 64, 8, 32), z(2, 64, 8, 32), z(64, 64, 3, 3)
    nbytes = L.ganlab_conv_wgrad_bf16_workspace(ctypes.byref(gw_geom))
    assert nbytes == B.wr_plan(2, 64, 64, 8, 32)['flush'] * 64 * 64 * 9 * 4
    wsw = z(nbytes // 4)
    assert L.ganlab_conv_wgrad_bf16(p(gyw), p(xw), p(gw), ctypes.byref(gw_geom), 1.0, p(wsw), nbytes - 1, None) == EWORKSPACE
    # unsupported geometries: 32 input channels; a 16-wide map for the weight gradient
    g32 = G(2, 32, 8, 32, 64, 3, 1, 0, 0)
    assert not B.bf16_ok(2, 32, 64, 8, 32) and L.ganlab_conv_bf16_supported(ctypes.byref(g32)) == 0
    assert L.ganlab_conv_fwd_bf16(p(x), p(wf), p(b), p(y), ctypes.byref(g32), 0.5, ops.ACT_LRELU, 0.2, None) == EUNSUPPORTED
    assert L.ganlab_conv_fwd_bf16_splitk(p(x), p(wf), p(b), p(y), ctypes.byref(g32), 0.5, ops.ACT_LRELU, 0.2, p(ws), need, None) == EUNSUPPORTED
    assert L.ganlab_conv_dgrad_bf16(p(gy), p(wd), p(x), ctypes.byref(g32), None) == EUNSUPPORTED
    assert L.ganlab_conv_dgrad_bf16_splitk(p(gy), p(wd), p(x), ctypes.byref(g32), p(ws), need, None) == EUNSUPPORTED
    assert L.ganlab_conv_wgrad_bf16(p(gyw), p(xw), p(gw), ctypes.byref(g32), 1.0, p(wsw), nbytes, None) == EUNSUPPORTED
    g16 = G(2, 64, 16, 16, 64, 3, 1, 0, 0)
    assert not B.bf16_wgrad_ok(2, 64, 64, 16, 16) and L.ganlab_conv_wgrad_bf16_workspace(ctypes.byref(g16)) == 0
    assert L.ganlab_conv_wgrad_bf16(p(gyw), p(xw), p(gw), ctypes.byref(g16), 1.0, p(wsw), nbytes, None) == EUNSUPPORTED
    assert _lib.launch_count() == c0, 'a refused call launched a kernel'
    # and the byte that was missing is all that was wrong
    assert L.ganlab_conv_fwd_bf16_splitk(*args, p(ws), need, None) == 0
    assert L.ganlab_conv_wgrad_bf16(p(gyw), p(xw), p(gw), ctypes.byref(gw_geom), 1.0, p(wsw), nbytes, None) == 0
    torch.cuda.synchronize()
    assert _lib.launch_count() == c0 + 4


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
def test_bf16_every_instantiation_ran(ops, tile_run):
    """closes the file: every instantiation the launchers of conv_bf16.hip can reach was launched by a test above (run the whole
    file: a selection of its tests leaves instantiations out)"""
    missing = [want for want in B.INSTANTIATIONS if not any(B.norm(want) in k for k in SEEN)]
    print('BF16 launched:', sorted(k for k in SEEN if 'bf16' in k))
    assert not missing, missing
