"""CPU: the binding gen_adversarial_amd/_lib.py derives from include/ga_ops.h has the layout the C compiler gives the header —
sizeof of every descriptor and of ga_op, offsetof of every field, every GA_OP_* value — and its header parser refuses what it
does not know instead of guessing."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from gen_adversarial_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'ga_ops.h')


def _host_cc():
    """$CC, then cc, then the clang of the ROCm toolchain that builds the library"""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'))))      # csrc/Makefile: HIPCC
    for cand in (os.environ.get('CC'), 'cc', os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang')):
        path = cand and shutil.which(cand)
        if path:
            return path
    raise AssertionError('no host C compiler: neither $CC, cc nor the ROCm clang')


def _header_text():
    return re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)


def test_layout_matches_the_c_compiler(tmp_path):
    """a C program generated from the binding's class and field names prints what the compiler makes of the header"""
    expect, lines = {}, []

    def probe(key, expr):
        lines.append(f'    printf("{key} %ld\\n", (long)({expr}));')

    for ctype, cls in L._H.types.items():
        expect[f'sizeof {ctype}'] = C.sizeof(cls)
        probe(f'sizeof {ctype}', f'sizeof({ctype})')
        for name, _ in cls._fields_:
            expect[f'offsetof {ctype} {name}'] = getattr(cls, name).offset
            probe(f'offsetof {ctype} {name}', f'offsetof({ctype}, {name})')
    union = dict(L.Op._fields_)['u']
    for row in L._H.ops:
        expect[f'kind {row.kind}'] = row.value
        probe(f'kind {row.kind}', row.kind)
        expect[f'offsetof ga_op u.{row.member}'] = L.Op.u.offset + getattr(union, row.member).offset
        probe(f'offsetof ga_op u.{row.member}', f'offsetof(ga_op, u.{row.member})')
        expect[f'sizeof u.{row.member}'] = C.sizeof(row.cls)
        probe(f'sizeof u.{row.member}', f'sizeof(((ga_op*)0)->u.{row.member})')
    assert 'offsetof ga_op u' in expect and expect['sizeof ga_op'] == 288 and len(L._H.ops) == 30 and len(expect) > 500
    src = tmp_path / 'probe.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ga_ops.h"\nint main(void) {\n' + '\n'.join(lines) + '\n    return 0;\n}\n')
    exe = tmp_path / 'probe'
    subprocess.run([_host_cc(), '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.rsplit(' ', 1) for line in out.splitlines())}
    assert got.keys() == expect.keys()
    wrong = {k: (got[k], v) for k, v in expect.items() if got[k] != v}
    assert not wrong, f'(compiler, ctypes): {wrong}'


def test_typedefs_classes_and_the_op_list_cover_each_other():
    hdr = _header_text()
    typedefs = set(re.findall(r'\}\s*(ga_\w+)\s*;', hdr))
    assert typedefs == set(L._H.types) == set(L._CLASS_NAMES) and len(typedefs) == 31          # 30 descriptors + ga_op
    for ctype, cls in L._H.types.items():
        assert cls.__name__ == L._CLASS_NAMES[ctype] and getattr(L, cls.__name__) is cls
    classes = {v for v in vars(L).values() if isinstance(v, type) and issubclass(v, C.Structure)}
    assert classes == set(L._H.types.values())                                                 # every class comes from a typedef
    rows = re.findall(r'\bX\(\s*(GA_OP_\w+)\s*,\s*(\d+)\s*,\s*(\w+)\s*,\s*(ga_\w+)\s*,\s*(ga_\w+)\s*\)', hdr)
    assert len(rows) == 30 and sorted(int(r[1]) for r in rows) == list(range(1, 31))
    assert [(r.kind, r.value, r.member, r.cls, r.entry) for r in L._H.ops] == \
        [(k, int(v), m, L._H.types[d], e) for k, v, m, d, e in rows]
    assert {r[3] for r in rows} == typedefs - {'ga_op'}                                        # a descriptor that no op uses is a mistake
    assert len({r[2] for r in rows}) == 30 and len({r[0] for r in rows}) == 30
    for row in L._H.ops:
        assert getattr(L, row.kind) == row.value
        op = L.make_op(row.cls())
        assert op.kind == row.value and isinstance(getattr(op.u, row.member), row.cls)


def _parse(text, **names):
    return L.Header(text, names)


def test_parser_reads_the_forms_the_header_uses():
    h = _parse('''
        /* a comment with a ; a { and int fake; in it */
        #define GA_T_ONE 1
        #define GA_T_NEG   -3   /* trailing; comment */
        enum ga_t { GA_T_A = 0, GA_T_B = 4 /* not, = 5 */ };
        typedef struct ga_t_desc {
            const float* a[2][2];   /* float* hidden; */
            // int also_hidden;
            int N, H, W, C;
            float* planes[4]; unsigned x_bytes, y_bytes; long n; unsigned long m; float s;
            const void* w; void** out;
        } ga_t_desc;
        int ga_t(const ga_t_desc* d, void* stream);
        const char* ga_t_name(void);
        long ga_t_scalars(const float* x, float** y, long n, float a, unsigned b, int, void* stream);
    ''', ga_t_desc='TDesc')
    T = h.types['ga_t_desc']
    assert T.__name__ == 'TDesc' and [n for n, _ in T._fields_] == \
        ['a', 'N', 'H', 'W', 'C', 'planes', 'x_bytes', 'y_bytes', 'n', 'm', 's', 'w', 'out']
    f = dict(T._fields_)
    assert f['a']._length_ == 4 and f['a']._type_ is L.fp and f['planes']._length_ == 4
    assert all(f[n] is L.i32 for n in 'NHWC') and f['x_bytes'] is f['y_bytes'] is C.c_uint
    assert f['n'] is C.c_long and f['m'] is C.c_ulong and f['s'] is L.f32 and f['w'] is L.fp and f['out'] is L.fp
    assert h.consts == {'GA_T_ONE': 1, 'GA_T_NEG': -3, 'GA_T_A': 0, 'GA_T_B': 4}
    assert h.protos == {'ga_t': (C.c_int, [C.POINTER(T), C.c_void_p]), 'ga_t_name': (C.c_char_p, []),
                        'ga_t_scalars': (C.c_long, [C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_uint, C.c_int, C.c_void_p])}


def test_parser_reads_an_op_list():
    h = _parse('''
        typedef struct ga_a_desc { float* x; } ga_a_desc;
        typedef struct ga_b_desc { long n; int k; } ga_b_desc;
        #define GA_OP_LIST(X) \\
            X(GA_OP_A, 1, a, ga_a_desc, ga_a) \\
            X(GA_OP_B, 7, bb, ga_b_desc, ga_run_b)
        #define GA_OP_ENUM_(kind, value, member, desc, entry) kind = value,
        #define GA_OP_MEMBER_(kind, value, member, desc, entry) desc member;
        enum ga_op_kind { GA_OP_LIST(GA_OP_ENUM_) };
        typedef struct ga_op { int kind; int _pad; union { GA_OP_LIST(GA_OP_MEMBER_) } u; } ga_op;
        int ga_a(const ga_a_desc* d, void* stream);
        int ga_plan_run(const ga_op* ops, int n, void* stream, int* failed_index);
    ''', ga_a_desc='ADesc', ga_b_desc='BDesc', ga_op='Op')
    A, B, Op = (h.types[t] for t in ('ga_a_desc', 'ga_b_desc', 'ga_op'))
    assert h.ops == [('GA_OP_A', 1, 'a', A, 'ga_a'), ('GA_OP_B', 7, 'bb', B, 'ga_run_b')]
    assert h.consts == {'GA_OP_A': 1, 'GA_OP_B': 7}
    assert [n for n, _ in Op._fields_] == ['kind', '_pad', 'u'] and dict(Op._fields_)['u']._fields_ == [('a', A), ('bb', B)]
    assert C.sizeof(Op) == 24 and h.protos['ga_plan_run'][1] == [C.POINTER(Op), C.c_int, C.c_void_p, C.c_void_p]


@pytest.mark.parametrize('decl', [
    'double x;',                          # unknown base types
    'size_t n;',
    'int64_t n;',
    'ga_other_desc inner;',               # a struct the header did not define
    'int flags : 3;',                     # bit-field
    'int (*callback)(int);',              # function pointer
    'float* a, b;',                       # would make b a float
    'int a[2][2][2];',
    'int a[N];',
    'void v;',
    'char c;',
    'float*** p;',
    'struct { int a; } inner;',
    'int x = 3;',
])
def test_parser_refuses_other_members(decl):
    with pytest.raises(ImportError, match='not supported'):
        _parse('typedef struct ga_t_desc { int ok; %s } ga_t_desc;' % decl, ga_t_desc='TDesc')


@pytest.mark.parametrize('text', [
    'int ga_f(double x);',
    'int ga_f(const ga_missing_desc* d, void* stream);',
    'int ga_f(int (*cb)(int));',
    'double ga_f(void);',
    'int ga_f(int a[4]);',
    'typedef struct ga_t_desc { int a; } ga_u_desc;',             # tag and typedef differ
    'typedef struct ga_nameless_desc { int a; } ga_nameless_desc;',   # no Python name given
    'enum ga_e { GA_E_FIRST, GA_E_SECOND };',                     # values the parser would have to count
    'typedef int ga_int;',
    'static int ga_f(void);',
    'int ga_f(void) { return 0; }',
])
def test_parser_refuses_other_declarations(text):
    with pytest.raises(ImportError, match='not supported'):
        _parse(text, ga_t_desc='TDesc', ga_u_desc='UDesc')
