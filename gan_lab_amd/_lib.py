"""ctypes binding of the C-ABI kernel library (include/ganlab_hip.h -> csrc/libganlab_hip.so).

The header is the only statement of the ABI: the compiler checks every definition in csrc/*.hip against it, and this
module parses it once at import into ``SIGNATURES`` (name -> (restype, argtypes)), the ``ctypes.Structure`` mirror of each
``typedef struct`` and ``DEFINES`` (the integer ``#define``s).  A new entry point is declared in the header and defined
in a .hip; nothing is restated here.  A declaration the parser does not understand raises at import, it is never skipped.

There is NO fallback: if the shared library is missing or a kernel returns an error code the call
raises.  PyTorch is used only for device memory, streams and autograd bookkeeping.
"""
import ctypes
import os
import re
import subprocess

# PyTorch bundles its own HIP runtime (torch/lib/libamdhip64.so).  It MUST be loaded before our
# library so that `libamdhip64.so.7` resolves to that same runtime: otherwise two runtimes coexist,
# torch's stream handles are foreign to ours and every launch fails.
import torch  # noqa: F401  (load order matters)

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
HEADER = os.path.join(_HERE, os.pardir, 'include', 'ganlab_hip.h')
# GANLAB_HIP_LIB: file name of an A/B build of the same library under csrc/ (make VARIANT=...); never a fallback
SO_PATH = os.path.join(CSRC, os.path.basename(os.environ.get('GANLAB_HIP_LIB', '') or 'libganlab_hip.so'))


class GanlabLibraryError(RuntimeError):
    pass


_SCALARS = {'int': ctypes.c_int, 'unsigned': ctypes.c_uint, 'long long': ctypes.c_longlong,
            'unsigned long long': ctypes.c_ulonglong, 'float': ctypes.c_float, 'double': ctypes.c_double,
            'size_t': ctypes.c_size_t, 'uint64_t': ctypes.c_uint64}
# the one struct the host passes by address; the job tables (ganlab_*_job, ganlab_pack_desc) are device copies
_HOST_STRUCT = 'ganlab_conv_geom'


def _bad(what, text):
    return GanlabLibraryError(f'include/ganlab_hip.h: {what}: {" ".join(text.split())!r}')


def _declarator(text, structs):
    """(ctypes type, name or None) of one ``[const] type[*] [name]``: a scalar of _SCALARS, or a pointer to one, to void,
    [unsigned] char or a struct of the header - every pointer is a c_void_p except char* and the host struct's."""
    words = [w for w in text.replace('*', ' * ').split() if w != 'const']
    if not re.fullmatch(r'[\w\s*]+', text) or words.count('*') > 1:
        raise _bad('not a declarator this binding understands', text)
    if '*' in words:
        base, name = ' '.join(words[:words.index('*')]), words[words.index('*') + 1:]
        if base == _HOST_STRUCT and base in structs:
            ctype = ctypes.POINTER(structs[base])
        elif base == 'char':
            ctype = ctypes.c_char_p
        elif base in _SCALARS or base in structs or base in ('void', 'unsigned char'):
            ctype = ctypes.c_void_p
        else:
            raise _bad(f'pointer to unknown type {base!r}', text)
    else:
        base, name = ' '.join(words), []
        if base not in _SCALARS:
            base, name = ' '.join(words[:-1]), words[-1:]
        if base not in _SCALARS:
            raise _bad(f'unknown type {base!r}', text)
        ctype = _SCALARS[base]
    if len(name) > 1:
        raise _bad('not a declarator this binding understands', text)
    return ctype, (name[0] if name else None)


def _struct(cname, body, structs):
    """ctypes.Structure mirror of ``typedef struct { body } ganlab_foo_bar;``, named FooBar, fields in header order."""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        first, *more = decl.split(',')              # `int a, b, c`: one type, several names
        ctype, name = _declarator(first, structs)
        if name is None or not all(re.fullmatch(r'\s*\w+\s*', m) for m in more):
            raise _bad(f'field of {cname}', decl)
        fields += [(n.strip(), ctype) for n in [name] + more]
    pyname = ''.join(part.capitalize() for part in cname.split('_')[1:])
    return type(pyname, (ctypes.Structure,), {'_fields_': fields, '__doc__': f'Mirror of `{cname}` (include/ganlab_hip.h).'})


def parse_header(text):
    """(signatures, structs, defines) of a C header in the style of include/ganlab_hip.h: {function: (restype, argtypes)},
    {typedef name: ctypes.Structure class} and {macro: int}.  Anything else left in the text raises GanlabLibraryError."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'#\s*ifdef\s+__cplusplus\b.*?#\s*endif', '', text, flags=re.S)      # extern "C" { ... }
    defines = {}
    for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*)$', text, flags=re.M):
        try:
            defines[name] = int(value.strip().strip('()'), 0)
        except ValueError:
            raise _bad('#define that is not an integer', f'{name} {value}') from None
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    structs = {}
    struct_re = re.compile(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', flags=re.S)
    for body, cname in struct_re.findall(text):
        structs[cname] = _struct(cname, body, structs)
    signatures = {}
    for decl in filter(None, (d.strip() for d in struct_re.sub('', text).split(';'))):
        m = re.fullmatch(r'(.+?)\b(\w+)\s*\((.+)\)', decl, flags=re.S)
        if not m:
            raise _bad('not a function prototype', decl)
        ret, name, args = m.groups()
        restype, stray = _declarator(ret, structs)
        if stray is not None:
            raise _bad('not a function prototype', decl)
        args = [] if args.strip() == 'void' else [_declarator(a, structs)[0] for a in args.split(',')]
        signatures[name] = (restype, args)
    return signatures, structs, defines


with open(HEADER) as _f:
    SIGNATURES, STRUCTS, DEFINES = parse_header(_f.read())

ConvGeom, PackDesc, SnJob, OrthoJob, HierJob, EwmaJob = (
    STRUCTS['ganlab_' + _n] for _n in ('conv_geom', 'pack_desc', 'sn_job', 'ortho_job', 'hier_job', 'ewma_job'))

ACT_NONE, ACT_LRELU = DEFINES['GANLAB_ACT_NONE'], DEFINES['GANLAB_ACT_LRELU']
PACK_FWD, PACK_DGRAD = DEFINES['GANLAB_PACK_FWD'], DEFINES['GANLAB_PACK_DGRAD']
SN_ROW_CHUNK, SN_COL_TILE, SN_ELEM_BLOCK = (DEFINES['GANLAB_SN_' + _n] for _n in ('ROW_CHUNK', 'COL_TILE', 'ELEM_BLOCK'))
ORTHO_TILE, ORTHO_QROWS, ORTHO_ROW, ORTHO_COL = (DEFINES['GANLAB_ORTHO_' + _n] for _n in ('TILE', 'QROWS', 'ROW', 'COL'))

_LIB = None


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    res = subprocess.run(['make', '-C', CSRC, '-j4'], capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
        print(res.stderr)
    if res.returncode != 0:
        raise GanlabLibraryError('building libganlab_hip.so failed:\n' + res.stderr[-4000:])
    return SO_PATH


def lib():
    """The loaded library; raises (never falls back) when it is missing."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise GanlabLibraryError(
                f'{SO_PATH} not found: the HIP kernel library is required (there is no CPU/PyTorch '
                f'fallback). Build it with `python -c "import __graft_entry__ as g; g.build()"` or '
                f'`make -C {CSRC}`.')
        handle = ctypes.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the .so does not export it
            fn.restype = res
            fn.argtypes = args
        for cname, mirror in STRUCTS.items():       # struct ganlab_x <-> int ganlab_x_size(void), as the library was compiled
            size = getattr(handle, cname + '_size')()
            if size != ctypes.sizeof(mirror):
                raise GanlabLibraryError(f'{mirror.__name__} mirror is {ctypes.sizeof(mirror)} bytes, the library\'s '
                                         f'{cname} {size}: header and binding disagree')
        _LIB = handle
    return _LIB


def last_launch():
    """(demangled kernel symbol, workgroups) of this thread's most recent launch through the library."""
    buf = ctypes.create_string_buffer(1024)
    grid = ctypes.c_uint(0)
    n = lib().ganlab_last_launch(buf, 1024, ctypes.byref(grid))
    return (buf.value.decode() if n > 0 else None), int(grid.value)


def launch_count():
    """Kernels this thread has launched through the library so far."""
    return int(lib().ganlab_launch_count())


def launches_since(count):
    """[(symbol, workgroups)] of this thread's launches after ``launch_count()`` returned ``count`` (oldest first; the
    library keeps the last 16)."""
    n = min(launch_count() - count, 16)
    out = []
    buf = ctypes.create_string_buffer(1024)
    grid = ctypes.c_uint(0)
    for back in range(n - 1, -1, -1):
        if lib().ganlab_launch_history(back, buf, 1024, ctypes.byref(grid)) > 0:
            out.append((buf.value.decode(), int(grid.value)))
    return out


_ERR = {DEFINES['GANLAB_' + _n]: f'GANLAB_{_n} ({_what})' for _n, _what in (
    ('EINVAL', 'bad argument'), ('EWORKSPACE', 'workspace too small'), ('ELAUNCH', 'kernel launch failed'),
    ('EUNSUPPORTED', 'geometry not handled'))}


def check(rc, what):
    if rc != 0:
        raise GanlabLibraryError(f'{what} failed: {_ERR.get(rc, rc)}')
