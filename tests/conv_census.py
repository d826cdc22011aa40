"""A census of convolution dispatch: one row per branch of the routing in ``gan_lab_amd.ops`` (``conv_route``, the pack rows,
the sub-choices inside a family), each at the smallest shape that still decides its branch with ``ops._X3_MIN_TILES`` at its
default.  ``run`` sends a row through the public launcher twice and returns what the library launched, as (symbol, workgroups)
pairs: the first call's list shows the weight-pack kernel too, the second is the steady state (pack-cache hit).

tests/golden/conv_census.json holds both lists of every row as recorded from the commit BEFORE ``conv_route`` existed
(``python tests/conv_census.py OUT.json`` with that commit's ``gan_lab_amd`` first on ``PYTHONPATH``): the routing is pinned
against that record, not against the code that now states it.  Users: tests/test_gpu_conv_census.py (replay on the GPU),
tests/test_host_logic.py (``conv_route`` alone, on the CPU)."""
import json
import os
import sys

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_census.json')

# name, op, Geom arguments (N, Cin, Hin, Win, Cout, ks, pad, up, pool), compute dtype, form
# form: which launcher of ``op`` - 'plain'; 'mask' the masked input gradient; 'aff' the affine-on-load forward / weight
# gradient; 'tail' the one-pass modulated layer (``_ConvModTail``)
_P64 = (64, 64, 64, 64, 3, 1, 0, 0)             # 64 -> 64 3x3 at 64^2: 16 tiles per image
_UP64, _POOL64 = (64, 16, 16, 64, 3, 1, 1, 0), (64, 32, 32, 64, 3, 1, 0, 1)             # 4 transposed-form tiles per image
_UP128, _POOL128 = (128, 32, 32, 128, 3, 1, 1, 0), (128, 64, 64, 128, 3, 1, 0, 1)       # 8 strided-form tiles per image
_UP32, _POOL32 = (32, 32, 32, 32, 3, 1, 1, 0), (32, 64, 64, 32, 3, 1, 0, 1)             # thin stride-2 layers
_UP64W = (64, 8, 32, 64, 3, 1, 1, 0)            # 4 tiles per image again: the affine-on-load up kernels want rows of 32 pixels
ROWS = [
    # split-product plain: 128 tiles at N = 8, 112 at N = 7
    ('plain64_n8_fwd', 'fwd', (8,) + _P64, 'f32', 'plain'),
    ('plain64_n8_dgrad', 'dgrad', (8,) + _P64, 'f32', 'plain'),
    ('plain64_n8_dgrad_mask', 'dgrad', (8,) + _P64, 'f32', 'mask'),
    ('plain64_n7_fwd', 'fwd', (7,) + _P64, 'f32', 'plain'),
    ('plain64_n7_dgrad', 'dgrad', (7,) + _P64, 'f32', 'plain'),
    ('plain64_n7_dgrad_mask', 'dgrad', (7,) + _P64, 'f32', 'mask'),
    # split-product transposed: an up layer's forward, a pooled layer's input gradient - 128 tiles at N = 32
    ('up64_n32_fwd', 'fwd', (32,) + _UP64, 'f32', 'plain'),
    ('up64_n31_fwd', 'fwd', (31,) + _UP64, 'f32', 'plain'),
    ('pool64_n32_dgrad', 'dgrad', (32,) + _POOL64, 'f32', 'plain'),
    ('pool64_n31_dgrad', 'dgrad', (31,) + _POOL64, 'f32', 'plain'),
    # split-product strided: a pooled layer's forward, an up layer's input gradient - 128 tiles at N = 16
    ('pool128_n16_fwd', 'fwd', (16,) + _POOL128, 'f32', 'plain'),
    ('pool128_n15_fwd', 'fwd', (15,) + _POOL128, 'f32', 'plain'),
    ('up128_n16_dgrad', 'dgrad', (16,) + _UP128, 'f32', 'plain'),
    ('up128_n15_dgrad', 'dgrad', (15,) + _UP128, 'f32', 'plain'),
    # exact stride-2: thin layers
    ('up32_fwd', 'fwd', (4,) + _UP32, 'f32', 'plain'),
    ('up32_dgrad', 'dgrad', (4,) + _UP32, 'f32', 'plain'),
    ('pool32_fwd', 'fwd', (4,) + _POOL32, 'f32', 'plain'),
    ('pool32_dgrad', 'dgrad', (4,) + _POOL32, 'f32', 'plain'),
    # the long-contraction linear (at most 64 rows), and one row more
    ('linear8192_n8_fwd', 'fwd', (8, 8192, 1, 1, 512, 1, 0, 0, 0), 'f32', 'plain'),
    ('linear8192_n65_fwd', 'fwd', (65, 8192, 1, 1, 512, 1, 0, 0, 0), 'f32', 'plain'),
    # exact fp32 sub-choices: split-K, the streaming fromRGB / toRGB kernels
    ('splitk512_fwd', 'fwd', (4, 512, 4, 4, 512, 3, 1, 0, 0), 'f32', 'plain'),
    ('splitk512_dgrad', 'dgrad', (4, 512, 4, 4, 512, 3, 1, 0, 0), 'f32', 'plain'),
    ('fromrgb_fwd', 'fwd', (4, 3, 64, 64, 16, 1, 0, 0, 0), 'f32', 'plain'),
    ('fromrgb_dgrad', 'dgrad', (4, 3, 64, 64, 16, 1, 0, 0, 0), 'f32', 'plain'),
    ('torgb_fwd', 'fwd', (4, 16, 64, 64, 3, 1, 0, 0, 0), 'f32', 'plain'),
    ('torgb_dgrad', 'dgrad', (4, 16, 64, 64, 3, 1, 0, 0, 0), 'f32', 'plain'),
    # bf16 compute: plain, folded upsample, 16-wide maps
    ('bf16_plain_fwd', 'fwd', (8, 64, 32, 32, 64, 3, 1, 0, 0), 'bf16', 'plain'),
    ('bf16_plain_dgrad', 'dgrad', (8, 64, 32, 32, 64, 3, 1, 0, 0), 'bf16', 'plain'),
    ('bf16_plain_wgrad', 'wgrad', (8, 64, 32, 32, 64, 3, 1, 0, 0), 'bf16', 'plain'),
    ('bf16_up_fwd', 'fwd', (8, 64, 16, 16, 64, 3, 1, 1, 0), 'bf16', 'plain'),
    ('bf16_up_dgrad', 'dgrad', (8, 64, 16, 16, 64, 3, 1, 1, 0), 'bf16', 'plain'),
    ('bf16_up_wgrad', 'wgrad', (8, 64, 16, 16, 64, 3, 1, 1, 0), 'bf16', 'plain'),
    ('bf16_w16_fwd', 'fwd', (8, 128, 16, 16, 128, 3, 1, 0, 0), 'bf16', 'plain'),
    # weight gradients: exact rolling (thin, rows of 64 pixels), exact tile, split-product plain and stride-2, exact stride-2
    ('thin16_wgrad', 'wgrad', (4, 16, 64, 64, 16, 3, 1, 0, 0), 'f32', 'plain'),
    ('tile32_wgrad', 'wgrad', (4, 32, 16, 16, 32, 3, 1, 0, 0), 'f32', 'plain'),
    ('plain64_n8_wgrad', 'wgrad', (8,) + _P64, 'f32', 'plain'),
    ('up64_n32_wgrad', 'wgrad', (32,) + _UP64, 'f32', 'plain'),
    ('pool64_n32_wgrad', 'wgrad', (32,) + _POOL64, 'f32', 'plain'),
    ('up32_wgrad', 'wgrad', (4,) + _UP32, 'f32', 'plain'),
    ('pool32_wgrad', 'wgrad', (4,) + _POOL32, 'f32', 'plain'),
    # affine on load
    ('plain64_n8_fwd_aff', 'fwd', (8,) + _P64, 'f32', 'aff'),
    ('plain64_n7_fwd_aff', 'fwd', (7,) + _P64, 'f32', 'aff'),
    ('up64w_n32_fwd_aff', 'fwd', (32,) + _UP64W, 'f32', 'aff'),
    ('up64w_n31_fwd_aff', 'fwd', (31,) + _UP64W, 'f32', 'aff'),
    ('plain64_n8_wgrad_aff', 'wgrad', (8,) + _P64, 'f32', 'aff'),
    ('thin16_wgrad_aff', 'wgrad', (4, 16, 64, 64, 16, 3, 1, 0, 0), 'f32', 'aff'),
    ('up64w_n32_wgrad_aff', 'wgrad', (32,) + _UP64W, 'f32', 'aff'),
    ('up32_wgrad_aff', 'wgrad', (4,) + _UP32, 'f32', 'aff'),
    # the one-pass layer: thin rolling kernel, the tile kernels' TAIL epilogue, the split-product TAIL form
    ('thin16_tail', 'fwd', (4, 16, 64, 64, 16, 3, 1, 0, 0), 'f32', 'tail'),
    ('plain64_n7_tail', 'fwd', (7,) + _P64, 'f32', 'tail'),
    ('plain64_n8_tail', 'fwd', (8,) + _P64, 'f32', 'tail'),
]

# Which family a launch list shows: the first substring found in any of its symbols.  The split-product stride-2 weight gradient
# is one kernel for up and pooled layers; ``conv_route`` reports it under the form of the layer's forward.
SYMBOL_FAMILY = (
    ('bf16', 'bf16'),
    ('conv_x3_up_kernel', 'x3_up'),
    ('conv_x3_down_kernel', 'x3_down'),
    ('conv_x3_s2_wgrad_kernel', 'x3_up|x3_down'),
    ('conv_x3_', 'x3'),
    ('_s2_', 's2'),
)
FAMILIES = ('bf16', 'x3', 'x3_up', 'x3_down', 's2', 'linear', 'f32')
PACK_SYMBOL_ROW = {'pack_kernel': 'f32', 'pack_s2_kernel': 's2', 'pack_bf16_kernel': 'bf16', 'x3_pack_kernel': 'x3',
                   'x3_up_pack_kernel': 'x3_up', 'x3_down_pack_kernel': 'x3_down'}


def family_of(row, launches):
    """The family the recorded launches of ``row`` show.  Exact fp32 has no mark of its own: it is what carries none of the
    others'; the long-contraction linear is a FORWARD that ran the weight-gradient kernels."""
    symbols = [s for s, _ in launches]
    for mark, family in SYMBOL_FAMILY:
        if any(mark in s for s in symbols):
            if '|' in family:
                return 'x3_up' if row[2][7] else 'x3_down'
            return family
    return 'linear' if row[1] == 'fwd' and any('wgrad' in s for s in symbols) else 'f32'


def pack_rows_of(launches):
    """The pack rows whose single-weight kernels a first-call launch list shows."""
    rows = set()
    for s, _ in launches:
        hits = [k for k in PACK_SYMBOL_ROW if k in s]       # ('pack_kernel' is the tail of the split-product names: longest wins)
        if hits:
            rows.add(PACK_SYMBOL_ROW[max(hits, key=len)])
    return rows


def geom_of(ops, row):
    with ops.compute_dtype(row[3]):
        return ops.Geom(*row[2])


def admitted(ops, row, g):
    """Does the restricted launcher of ``row``'s form take its geometry?  (What its callers ask before they choose it.)"""
    import torch
    form, up = row[4], bool(g.up)
    w = torch.empty(g.Cout, g.Cin, g.ks, g.ks, device='meta')
    if form == 'mask':
        return ops.conv_dgrad_mask_ok(g)
    if form == 'aff':       # (the one-pass layer's backward sends its thin shapes to the affine-on-load weight gradient too)
        return ops.conv_aff_ok(g.in_shape, w, up) or (row[1] == 'wgrad' and not up and ops.mod_conv_shape_ok(g.in_shape, w))
    if form == 'tail':
        return ops.mod_conv_shape_ok(g.in_shape, w) or ops.conv_tail_shape_ok(g.in_shape, w)
    return True


def run(ops, row):
    """[first call's launches, second call's launches] of ``row``, each a list of (symbol, workgroups)."""
    import torch
    from gan_lab_amd import _lib
    name, op, _, _, form = row
    g = geom_of(ops, row)
    assert ops.x3_enabled() and ops.get_compute_dtype() == 'f32' and admitted(ops, row, g), name
    ones = lambda *shape: torch.ones(*shape, device='cuda')
    x, gy, w = ones(*g.in_shape), ones(*g.out_shape), ones(g.Cout, g.Cin, g.ks, g.ks)
    s_, t_, bias = ones(g.N, g.Cin), ones(g.N, g.Cin), ones(g.Cout)
    scale, slope = 0.01, 0.2
    call = {
        ('fwd', 'plain'): lambda: ops.k_conv_fwd(x, w, bias, g, scale, 1.0, ops.ACT_LRELU, slope),
        ('dgrad', 'plain'): lambda: ops.k_conv_dgrad(gy, w, g, scale),
        ('dgrad', 'mask'): lambda: ops.k_conv_dgrad_mask(gy, w, x, g, scale, slope),
        ('wgrad', 'plain'): lambda: ops.k_conv_wgrad(gy, x, g, scale),
        ('fwd', 'aff'): lambda: ops.k_conv_fwd_aff(x, s_, t_, w, g, scale),
        ('wgrad', 'aff'): lambda: ops.k_conv_wgrad_aff(gy, x, s_, t_, g, scale),
        ('fwd', 'tail'): lambda: ops._ConvModTail.apply(x, s_, t_, w, bias, None, None, None, scale, 1.0, ops.ACT_LRELU, slope,
                                                        1e-8),
    }[(op, form)]
    lists = []
    with torch.no_grad():
        for _ in range(2):
            c0 = _lib.launch_count()
            call()
            torch.cuda.synchronize()
            lists.append([list(p) for p in _lib.launches_since(c0)])
    return lists


def load():
    with open(FIXTURE) as f:
        return json.load(f)


if __name__ == '__main__':          # record: {row name: [first, second]}
    from gan_lab_amd import ops
    out = {row[0]: run(ops, row) for row in ROWS}
    with open(sys.argv[1], 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('recorded', len(out), 'rows from', os.path.dirname(ops.__file__))
