"""CPU tests of the ctypes binding derived from include/ganlab_hip.h (gan_lab_amd/_lib.py): the parser on literal header
snippets, what it refuses, that nothing the real header declares is dropped, and the struct mirrors' sizes against the library."""
import ctypes
import os
import re

import pytest

from gan_lab_amd import _lib

c_int, c_uint, c_ll, c_ull, c_f, c_d, c_sz, c_u64, c_p, c_cp = (
    ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_float, ctypes.c_double, ctypes.c_size_t,
    ctypes.c_uint64, ctypes.c_void_p, ctypes.c_char_p)

SNIPPET = """
/* a header in the style of ganlab_hip.h */
#ifndef SNIPPET_H
#define SNIPPET_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define GANLAB_OK 0
#define GANLAB_EINVAL (-1)   /* bad argument (null pointer; see *_supported) */
#define GANLAB_MASK 0x20     // hexadecimal
typedef struct {
  int N, Cin, Hin; /* physical input */
  int up;          /* 1: upsampled */
} ganlab_conv_geom;
typedef struct ganlab_toy_job {
  int a, b, c;
  const float* w; float* gw;
  long long blk0;
  float scale;
  void* dst;
} ganlab_toy_job;
int ganlab_abi_version(void);
/* wrapped over three lines */
int ganlab_wrapped_f32(const float* x, float* y,
                       const ganlab_conv_geom* g, float scale, int act,
                       void* workspace, size_t workspace_bytes, void* stream);
unsigned long long ganlab_launch_count(void);
size_t ganlab_workspace(const ganlab_conv_geom* g);
long long ganlab_pack(const float* w, void* out, long long n, double q, unsigned flags);
int ganlab_last_launch(char* name, int cap, unsigned* grid);
int ganlab_decode(const unsigned char* p, uint64_t seed, const ganlab_toy_job* jobs_device, long long* batches);
#ifdef __cplusplus
}
#endif
#endif /* SNIPPET_H */
"""


def test_parser_on_a_literal_header():
    sig, structs, defines = _lib.parse_header(SNIPPET)
    assert defines == {'GANLAB_OK': 0, 'GANLAB_EINVAL': -1, 'GANLAB_MASK': 32}
    assert list(structs) == ['ganlab_conv_geom', 'ganlab_toy_job']
    geom, job = structs['ganlab_conv_geom'], structs['ganlab_toy_job']
    assert issubclass(geom, ctypes.Structure) and (geom.__name__, job.__name__) == ('ConvGeom', 'ToyJob')
    assert geom._fields_ == [('N', c_int), ('Cin', c_int), ('Hin', c_int), ('up', c_int)]
    assert job._fields_ == [('a', c_int), ('b', c_int), ('c', c_int), ('w', c_p), ('gw', c_p), ('blk0', c_ll), ('scale', c_f),
                            ('dst', c_p)]
    g = geom(2, 3, 4, 1)                           # positional construction, as the callers do
    assert (g.N, g.Cin, g.Hin, g.up) == (2, 3, 4, 1)
    gp = ctypes.POINTER(geom)
    assert sig == {
        'ganlab_abi_version': (c_int, []),
        'ganlab_wrapped_f32': (c_int, [c_p, c_p, gp, c_f, c_int, c_p, c_sz, c_p]),
        'ganlab_launch_count': (c_ull, []),
        'ganlab_workspace': (c_sz, [gp]),
        'ganlab_pack': (c_ll, [c_p, c_p, c_ll, c_d, c_uint]),
        'ganlab_last_launch': (c_int, [c_cp, c_int, c_p]),
        'ganlab_decode': (c_int, [c_p, c_u64, c_p, c_p]),
    }
    assert list(sig) == ['ganlab_abi_version', 'ganlab_wrapped_f32', 'ganlab_launch_count', 'ganlab_workspace', 'ganlab_pack',
                         'ganlab_last_launch', 'ganlab_decode']


@pytest.mark.parametrize('text,offending', [
    ('int ganlab_a(short n);', 'short n'),                                          # scalar outside the table
    ('short ganlab_a(int n);', 'short'),
    ('int ganlab_a(const short* p, int n);', 'const short* p'),                     # pointer to a type outside the table
    ('int ganlab_a(const ganlab_missing* g);', 'const ganlab_missing* g'),          # struct the header does not define
    ('int ganlab_a(void (*cb)(int), int n);', 'void (*cb)(int)'),                   # function pointer
    ('int ganlab_a(float** rows);', 'float** rows'),
    ('int ganlab_a(int n, ...);', '...'),
    ('int ganlab_a();', 'ganlab_a()'),                                              # unprototyped
    ('int ganlab_a(int n) { return n; }', 'return n'),                              # not a declaration
    ('extern int ganlab_counter;', 'extern int ganlab_counter'),
    ('typedef struct { int a; short b; } ganlab_s;', 'short b'),                    # struct fields
    ('typedef struct { int a; float *p, *q; } ganlab_s;', 'float *p, *q'),
    ('typedef struct { int a; int; } ganlab_s;', 'int'),
    ('#define GANLAB_EPS 1e-8f\nint ganlab_a(void);', 'GANLAB_EPS 1e-8f'),
])
def test_parser_refuses_what_it_does_not_understand(text, offending):
    with pytest.raises(_lib.GanlabLibraryError) as e:
        _lib.parse_header(text)
    assert offending in str(e.value), str(e.value)


def _real_header():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, 'include', 'ganlab_hip.h')) as f:
        return re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)


def test_nothing_the_header_declares_is_dropped():
    src = _real_header()
    assert len(re.findall(r'ganlab_\w+\s*\(', src)) == len(_lib.SIGNATURES) > 0
    typedefs = re.findall(r'\}\s*(ganlab_\w+)\s*;', src)
    assert len(typedefs) == len(re.findall(r'typedef\s+struct', src)) == len(_lib.STRUCTS) > 0
    for cname in typedefs:
        assert issubclass(_lib.STRUCTS[cname], ctypes.Structure)
        assert _lib.SIGNATURES[cname + '_size'] == (c_int, [])
    assert (_lib.ConvGeom, _lib.PackDesc, _lib.SnJob, _lib.OrthoJob, _lib.HierJob, _lib.EwmaJob) == tuple(
        _lib.STRUCTS['ganlab_' + n] for n in ('conv_geom', 'pack_desc', 'sn_job', 'ortho_job', 'hier_job', 'ewma_job'))
    defined = re.findall(r'^\s*#\s*define\s+(GANLAB_\w+)[ \t]+\S', src, flags=re.M)
    assert sorted(defined) == sorted(_lib.DEFINES) and len(defined) == len(set(defined))


def test_struct_mirrors_match_the_library_sizes():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    L = _lib.lib()
    for cname, mirror in _lib.STRUCTS.items():
        assert ctypes.sizeof(mirror) == getattr(L, cname + '_size')(), cname
