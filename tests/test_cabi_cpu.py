"""The whole C ABI in one place: dfl_amd._native is computed from include/dfl_hip.h by dfl_amd/_cabi.py, so the reader is what
has to be right.  Its layout of every struct is held against a C compiler's sizeof / offsetof of the same header, what it cannot
read it has to refuse, and its prototypes are the header's.  No GPU: the compiled program is a host program of a few printf."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from dfl_amd import _cabi, _native as nat

HEADER = os.path.join(ROOT, 'include', 'dfl_hip.h')
STRUCTS, FIELDS = 55, 690            # the header's count when this test was written: a reader that finds fewer has skipped some


def _compiler():
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    for cc in ('cc', 'gcc', os.path.join(rocm, 'llvm', 'bin', 'clang'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang')):
        if shutil.which(cc):
            return shutil.which(cc)
    return None


def test_every_struct_has_the_layout_the_c_compiler_gives_it(tmp_path):
    cc = _compiler()
    if cc is None:
        pytest.skip('no host C compiler (cc, gcc or the clang of ROCm)')
    _, structs, _ = _cabi.load(HEADER)
    c_name = {v: k for k, v in _cabi.RENAME.items()}
    src = ['#include <stdio.h>', '#include "dfl_hip.h"', 'int main(void) {']
    for name, cls in structs.items():
        src.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            f = c_name.get(f, f)
            src.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, f, name, f, name, f))
    src += ['  return 0;', '}']
    (tmp_path / 'layout.c').write_text('\n'.join(src))
    exe = str(tmp_path / 'layout')
    subprocess.run([cc, '-I', os.path.dirname(HEADER), '-o', exe, str(tmp_path / 'layout.c')], check=True, timeout=120)
    said = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split('\n'):
        if line:
            said[line.split()[0]] = tuple(int(t) for t in line.split()[1:])
    n_fields, wrong = 0, []
    for name, cls in structs.items():
        if said[name] != (C.sizeof(cls),):
            wrong.append((name, said[name], C.sizeof(cls)))
        for f, _ in cls._fields_:
            n_fields += 1
            d = getattr(cls, f)
            if said['%s.%s' % (name, c_name.get(f, f))] != (d.offset, d.size):
                wrong.append((name, f, said['%s.%s' % (name, c_name.get(f, f))], (d.offset, d.size)))
    print('%d structs, %d fields, %d mismatches against %s' % (len(structs), n_fields, len(wrong), cc))
    assert not wrong, wrong
    assert len(structs) >= STRUCTS and n_fields >= FIELDS, (len(structs), n_fields)
    assert len(said) == len(structs) + n_fields
    # ... and those are the classes the binding publishes, under the CamelCase of the header's names
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert list(structs) == re.findall(r'\}\s*(dfl_\w+)\s*;', hdr.split('dfl_status;')[1].replace('} dfl_op_kind;', ''))
    for name, cls in structs.items():
        pub = getattr(nat, _cabi.camel(name))
        assert pub is nat._STRUCTS[name] and pub.__name__ == cls.__name__ and C.sizeof(pub) == C.sizeof(cls)
        assert [(f, getattr(pub, f).offset, getattr(pub, f).size) for f, _ in pub._fields_] == \
               [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_]


def test_constants_are_the_headers():
    consts, _, _ = _cabi.load(HEADER)
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    defines = re.findall(r'^#define (DFL_\w+) +(\d+)\s*$', hdr, flags=re.M)
    assert len(defines) >= 40
    for name, value in defines:
        assert consts[name] == int(value) == getattr(nat, name[4:]), name
    kinds = re.findall(r'(DFL_OP_\w+) = (\d+)', hdr)
    assert len(kinds) == 24 and [int(v) for _, v in kinds] == list(range(1, 25))
    for name, value in kinds:
        assert consts[name] == int(value) == getattr(nat, name[4:]), name
    assert consts['DFL_OK'] == 0 and consts['DFL_ERR_WORKSPACE'] == -4
    assert nat.BN_R == 8 and nat.MAX_SIDE_STREAMS == 2 and nat.HEAD_LARGE_NM == 48
    from dfl_amd.plan import UNetPlan
    assert UNetPlan.BN_R is nat.BN_R


GOOD = '''#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* dfl_stream_t;
#define DFL_N 3
#define DFL_M (2 * DFL_N + 1)   /* names an earlier constant */
typedef enum { DFL_A = 1, DFL_B, DFL_C = DFL_M << 1 } dfl_kind;
typedef struct { const float* a; const float* b; int32_t p, q[DFL_N][2]; double d; } dfl_inner;
typedef struct {
  dfl_inner in;
  const void* const* pp; uint64_t k[DFL_M / 2];
  float f;
} dfl_outer_args;
int64_t dfl_f(const dfl_outer_args* a, int32_t n, double x, dfl_stream_t s);
const char* dfl_g(void);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_reader_reads_every_form_the_header_uses():
    consts, structs, funcs = _cabi.parse(GOOD)
    assert consts == {'DFL_N': 3, 'DFL_M': 7, 'DFL_A': 1, 'DFL_B': 2, 'DFL_C': 14}
    inner, outer = structs['dfl_inner'], structs['dfl_outer_args']
    assert (inner.__name__, outer.__name__) == ('Inner', 'OuterArgs')
    assert inner._fields_ == [('a', C.c_void_p), ('b', C.c_void_p), ('p', C.c_int32), ('q', C.c_int32 * 2 * 3), ('d', C.c_double)]
    assert outer._fields_ == [('inp', inner), ('pp', C.c_void_p), ('k', C.c_uint64 * 3), ('f', C.c_float)]
    assert funcs == {'dfl_f': (C.c_int64, [C.c_void_p, C.c_int32, C.c_double, C.c_void_p]), 'dfl_g': (C.c_char_p, [])}


REFUSED = {
    'an unknown type': ('typedef struct { int32_t n; size_t bytes; } dfl_x;', 'size_t bytes'),
    'an unknown pointee': ('typedef struct { const half* p; } dfl_x;', 'half'),
    'a declarator it cannot read': ('typedef struct { int32_t n; int32_t (*fn)(int32_t); } dfl_x;', '(*fn)'),
    'a declaration without a type': ('typedef struct { int32_t n; m; } dfl_x;', ' m;'),
    'a bit-field': ('typedef struct { int32_t n;\n uint32_t flag : 1; } dfl_x;', 'flag : 1'),
    'a union': ('typedef union { int32_t i; float f; } dfl_x;', 'union'),
    'a union inside a struct': ('typedef struct { int32_t n; union { int32_t i; float f; } u; } dfl_x;', 'union'),
    'a nested anonymous struct': ('typedef struct { int32_t n;\n struct { int32_t i; float f; } s; } dfl_x;', 'struct { int32_t i'),
    'a tagged struct': ('typedef struct dfl_tag { int32_t n; } dfl_x;', 'dfl_tag'),
    'a define that is no integer': ('#define DFL_SCALE 1.5f', 'DFL_SCALE'),
    'a define that is a string': ('#define DFL_NAME "dfl"', 'DFL_NAME'),
    'a define of an unknown name': ('#define DFL_TWICE (2 * DFL_NOT_THERE)', 'DFL_TWICE'),
    'a function-like macro': ('#define DFL_MIN(a, b) ((a) < (b) ? (a) : (b))', 'DFL_MIN'),
    'an array bound that is no constant': ('typedef struct { float taps[n]; } dfl_x;', 'taps[n]'),
    'another preprocessor line': ('#pragma pack(1)', 'pragma'),
    'a conditional block': ('#if DFL_N > 2\n#define DFL_BIG 1\n#endif', '#if DFL_N'),
    'a struct by value in a prototype that is not declared': ('int dfl_f(dfl_nothing a);', 'dfl_nothing'),
    'an array parameter': ('int dfl_f(const float m[9]);', 'm[9]'),
    'a trailing comma in an enum': ('typedef enum { DFL_P = 1, } dfl_p;', 'DFL_P'),
    'a parameter without a type': ('int dfl_f(a);', 'dfl_f(a)'),
    'a global': ('extern int dfl_counter;', 'dfl_counter'),
    'void by value': ('typedef struct { void v; } dfl_x;', 'void v'),
}


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_reader_refuses(what):
    """Each text is the good header with one more line, which the reader must refuse -- by its line number and text --
    instead of passing over it."""
    extra, named = REFUSED[what]
    lines = GOOD.split('\n')
    at = lines.index('const char* dfl_g(void);') + 1
    text = '\n'.join(lines[:at] + extra.split('\n') + lines[at:])
    bad = [k for k, ln in enumerate(extra.split('\n')) if named in ln][0]
    with pytest.raises(_cabi.HeaderError) as e:
        _cabi.parse(text, 'x.h')
    assert str(e.value).startswith('x.h:%d: ' % (at + bad + 1)), str(e.value)
    assert named.strip() in str(e.value), str(e.value)


def test_python_keyword_field_is_renamed_in_place():
    assert _cabi.RENAME == {'in': 'inp'}
    names = [f for f, _ in nat.ResampleArgs._fields_]
    assert 'inp' in names and 'in' not in names
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = hdr[:hdr.index('} dfl_resample_args;')].rsplit('typedef struct {', 1)[1]
    first = re.search(r'(\w+)\s*;', body).group(1)
    assert first == 'in' and names[0] == 'inp' and nat.ResampleArgs.inp.offset == 0 and nat.ResampleArgs.inp.size == C.sizeof(C.c_void_p)
    assert nat.ResampleArgs.plan.offset == 16 and nat.ResampleArgs._fields_[2] == ('plan', nat.ResamplePlan)
    a = nat.ResampleArgs(inp=4096, out=8192)
    assert C.cast(C.addressof(a), C.POINTER(C.c_void_p))[0] == 4096


INT64 = ('dfl_loss_scratch_doubles', 'dfl_prep_scratch_doubles', 'dfl_augment_scratch_bytes', 'dfl_sim_scratch_doubles',
         'dfl_sim_patch_count', 'dfl_sim_patch_scratch_doubles')


def test_prototypes_are_the_headers_and_lib_sets_every_signature():
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r'\b(dfl_[a-z0-9_]+)\s*\(', hdr))                 # the expression of test_host_cpu.py
    _, _, funcs = _cabi.load(HEADER)
    assert set(funcs) == declared and len(funcs) >= 87
    assert nat.EXPORTS == list(funcs) == sorted(funcs, key=lambda f: re.search(r'\b%s\s*\(' % f, hdr).start())   # header order
    assert sorted(f for f, (res, _) in funcs.items() if res is C.c_int64) == sorted(INT64)
    assert [f for f, (res, _) in funcs.items() if res not in (C.c_int, C.c_int64)] == ['dfl_last_error']
    L = nat.lib()
    for f, (res, args) in funcs.items():
        fn = getattr(L, f)
        assert fn.restype is res and list(fn.argtypes) == args, f
    for f in INT64:
        assert getattr(L, f).restype is C.c_int64, f
    assert L.dfl_last_error.restype is C.c_char_p
    assert L.dfl_conv2d.argtypes == [C.c_void_p, C.c_void_p] and L.dfl_sizeof.argtypes == [C.c_int]
    assert L.dfl_adam_step.argtypes[4:8] == [C.c_int64, C.c_float, C.c_double, C.c_double]
    assert L.dfl_loss_scratch_doubles(2, 7, 14) > 0 and L.dfl_head_scratch_ld(32) % 4 == 0 and L.dfl_get_math_mode() >= 0
