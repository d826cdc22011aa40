"""Host tests of how ``gan_lab_amd.ops`` is laid out: the facade keeps every name it had before the op families moved to
``gan_lab_amd/_ops/``, and no moved function reads a name that tests, bench.py or tools rebind on ``ops``."""
import ast
import importlib
import inspect
import os
import pkgutil
import sys
import types

import gan_lab_amd._ops
from gan_lab_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# Names assigned or monkeypatched on the ``ops`` module.  Regenerate with a search for  setattr(ops  and  ops\.\w+ =  over
# tests/, tools/ and bench.py (tools/flip_probe.py sets its three through a loop variable).
REBOUND = (
    'k_conv_fwd', 'k_conv_dgrad',                                                               # bench.py, tools/step_layers.py
    'k_conv_dgrad_rgb_sums', 'k_conv_wgrad_act', '_MASK_BITS',                                  # tests/test_gpu_ops.py
    '_X3_MIN_TILES',                                                                            # tests/test_gpu_x3.py, tools/op_error_probe.py
    '_PACK_CACHE', '_PACK_TABLES',                                                              # tests/test_host_logic.py
    'direct_param_grads', 'pack_generation',                                                    # tests/test_gpu_learner.py
    'diff_augment', 'ada_augment',                                                              # tests/test_gpu_diffaug.py, test_gpu_ada.py
    'k_conv_wgrad', 'k_conv_dgrad_mask', 'k_conv_dgrad_act', 'k_conv_fwd_mask', 'k_conv_fwd_aff', 'k_conv_wgrad_aff',
    'k_conv_fwd_blur_bits', 'k_conv_s2_fwd_blur_tail', 'k_conv_s2_dgrad_blur_act',              # tools/step_layers.py
    'conv2d', 'bias_act', 'linear',                                                             # tools/flip_probe.py
)

# one public name per family module (and the shared plumbing): ``ops.<name>`` is the defining module's object
SAMPLE = {
    'core': ('input_grad_only', 'no_grad_towards', 'direct_param_grads', '_take', 'arena_takes', '_p', '_st', '_c'),
    'geom': ('Geom', 'set_launch_observer', 'compute_dtype'),
    'pointwise': ('k_channel_sum', 'chan_affine', 'resample', 'tanh'),
    'norm': ('layer_norm', '_BatchNormTrain'),
    'loss': ('hinge_mean', 'mbstd_stat'),
    'attention': ('attention', 'k_dot', 'gated_residual'),
    'metrics': ('swd_down', 'prdc_knn', 'moments_accum', 'kid_rowsums', 'msssim_level', 'spectrum_feed'),
    'optim': ('SnTable', 'ortho_apply', 'adam_step', 'EwmaTable'),
    'augment': ('randn', 'diff_augment', 'ada_augment', 'AdaDraw'),
    'cond': ('randint', 'cond_batch_norm'),
    'hier': ('HierTable', 'hier_modulate', 'mod_batch_norm', 'class_projection'),
    'cr': ('cr_transform', 'cr_msd', 'cr_imsd'),
    'cond_loss': ('class_cross_entropy', 'class_contrastive'),
    'project': ('pyramid_mse', 'w_moments', 'project_step'),
}
ADDED = ('arena_takes',)        # sampled names the facade has gained since the golden list was taken


def _family_modules():
    names = sorted(m.name for m in pkgutil.iter_modules(gan_lab_amd._ops.__path__))
    return {n: importlib.import_module('gan_lab_amd._ops.' + n) for n in names}


def test_ops_surface_unchanged():
    """tests/golden/ops_surface.txt: every non-dunder key of ``vars(ops)`` of the last single-file ``ops.py`` (commit 4c84b4d)."""
    with open(os.path.join(GOLDEN, 'ops_surface.txt')) as f:
        listed = f.read().split()
    assert len(listed) == 391 and len(set(listed)) == 391
    missing = [n for n in listed if not hasattr(ops, n)]
    assert not missing, missing
    mods = _family_modules()
    assert sorted(mods) == sorted(SAMPLE)
    for mod, names in SAMPLE.items():
        for n in names:
            assert n in listed or n in ADDED, n
            assert getattr(ops, n) is getattr(mods[mod], n), (mod, n)
            assert getattr(mods[mod], n).__module__ == mods[mod].__name__, (mod, n)


def _code_objects(mod):
    """Every code object of a function, method or nested function / lambda / comprehension defined in ``mod``."""
    seen, todo = set(), []

    def push(obj):
        if isinstance(obj, (staticmethod, classmethod)):
            obj = obj.__func__
        if isinstance(obj, property):
            for f in (obj.fget, obj.fset, obj.fdel):
                push(f)
        elif isinstance(obj, types.FunctionType) and obj.__module__ == mod.__name__:
            todo.append(obj.__code__)
            push(getattr(obj, '__wrapped__', None))        # the body under @once_differentiable
        elif isinstance(obj, type) and obj.__module__ == mod.__name__ and obj not in seen:
            seen.add(obj)
            for v in vars(obj).values():
                push(v)

    for v in vars(mod).values():
        push(v)
    while todo:
        code = todo.pop()
        if code in seen:
            continue
        seen.add(code)
        yield code
        todo.extend(c for c in code.co_consts if isinstance(c, types.CodeType))


def test_rebound_names_stay_in_ops():
    """A rebinding of ``ops.<name>`` reaches only functions whose globals are ``ops.py``'s own, so no code under ``_ops/`` may
    read such a name; and no module there imports ``gan_lab_amd.ops`` (no cycle, no way round the rule)."""
    mods = _family_modules()
    for name, mod in mods.items():
        for code in _code_objects(mod):
            hit = sorted(set(code.co_names) & set(REBOUND))
            assert not hit, f'_ops/{name}.py: {code.co_name} (line {code.co_firstlineno}) reads {hit}'
        imported = [v for v in vars(mod).values() if isinstance(v, types.ModuleType)]
        assert ops not in imported and sys.modules['gan_lab_amd.ops'] not in imported, name
        assert not any(getattr(v, '__module__', None) == 'gan_lab_amd.ops' for v in vars(mod).values()), name
        for node in ast.walk(ast.parse(inspect.getsource(mod))):        # imports inside functions too
            if isinstance(node, ast.Import):
                targets = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                base = 'gan_lab_amd._ops'.rsplit('.', node.level - 1)[0] if node.level else ''
                source = '.'.join(p for p in (base, node.module) if p)
                targets = [source] + [source + '.' + a.name for a in node.names]
            else:
                continue
            assert 'gan_lab_amd.ops' not in targets, f'_ops/{name}.py line {node.lineno}'
    # the walk reaches a Function's backward under @staticmethod @once_differentiable ...
    assert any(c.co_name == 'backward' and '_want_param_grads' in c.co_names for c in _code_objects(mods['cond']))
    # ... reaches a ``_take`` caller outside ``ops.py`` (counted by ``arena_takes`` all the same: see the test below) ...
    assert any(c.co_name == 'k_channel_sum' and '_take' in c.co_names for c in _code_objects(mods['pointwise']))
    # ... and sees through a class, a staticmethod and a nested lambda
    probe = types.ModuleType('gan_lab_amd._ops._probe')

    class Fn(object):
        @staticmethod
        def forward(x):
            return (lambda: k_conv_fwd)()       # noqa: F821
    Fn.__module__ = Fn.forward.__module__ = probe.__name__
    probe.Fn = Fn
    assert any('k_conv_fwd' in c.co_names for c in _code_objects(probe))


def test_arena_takes_counts_where_take_hits_the_arena():
    """``ops.arena_takes()`` rises by one exactly when ``_take`` hands out an offered arena slot (the branch that marks the name
    taken), in whichever module the caller lives; a ``_take`` that allocates leaves it alone.  Host tensors: ``_sink`` / ``_take``
    read only ``.grad``, ``.device``, sizes and the arena's serial."""
    import torch

    def param(*shape):
        p = torch.nn.Parameter(torch.zeros(*shape))
        p.grad = torch.zeros(*shape)
        p._ganlab_arena = types.SimpleNamespace(serial=7)
        return p
    p, q, like = param(2, 3), param(4), torch.zeros(1)
    with ops.direct_param_grads(), torch.no_grad():
        start = ops.arena_takes()
        fresh = ops._take('gw', (2, 3), like)                       # nothing offered at all
        assert ops.arena_takes() == start and fresh.shape == (2, 3) and fresh._base is None
        ops._sink('gw', p)
        fresh = ops._take('gb', (2, 3), like)                       # something offered, under another name
        assert ops.arena_takes() == start and fresh._base is None and not ops._sunk('gb')
        out = ops._take('gw', (3, 2), like)                         # the offer: same element count
        assert ops.arena_takes() == start + 1
        assert out._base is p.grad and out.data_ptr() == p.grad.data_ptr() and out.shape == (3, 2)
        assert p._ganlab_written == 7 and ops._sunk('gw') and not ops._sunk('gw')
        ops._sink('gb', q)
        fresh = ops._take('gb', (5,), like)                         # offered, but 4 elements against 5
        assert ops.arena_takes() == start + 1 and fresh.shape == (5,) and fresh._base is None
        assert not ops._sunk('gb') and not hasattr(q, '_ganlab_written')
    assert ops.arena_takes() == start + 1 and ops.arena_takes is gan_lab_amd._ops.core.arena_takes
