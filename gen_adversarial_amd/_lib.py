"""
ctypes binding of libga_ops.so, built at import from include/ga_ops.h: the descriptor classes, `Op`, the GA_* constants, the
kind <-> union member <-> class <-> entry point association (GA_OP_LIST) and every prototype are read out of the header, nothing
about the ABI is restated here except _CLASS_NAMES.  tests/test_abi_layout_cpu.py checks the resulting layouts against the C
compiler's.  The product path has NO fallback: if the library is missing or fails to load, importing this module raises.
"""
from __future__ import annotations

import collections
import ctypes as C
import math
import os
import re

# PyTorch-ROCm bundles its own libamdhip64.so.7; libga_ops.so needs the same SONAME.  Importing torch FIRST makes the
# dynamic loader bind our library to the HIP runtime torch already initialised (one runtime per process: streams and
# device pointers are shared).  Loading ours first would pull the system ROCm copy and leave two runtimes in the process
# ("no ROCm-capable device is detected" on the second one).
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('GA_OPS_LIB') or os.path.join(_HERE, 'libga_ops.so')   # GA_OPS_LIB: debug builds only (make trace)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'ga_ops.h')

fp = C.c_void_p     # device pointers travel as integers
i32 = C.c_int
f32 = C.c_float

# C typedef -> Python class: the one entry a new op needs on this side
_CLASS_NAMES = {
    'ga_conv_desc': 'ConvDesc', 'ga_dwconv5_desc': 'DwDesc', 'ga_rowchan_reduce_desc': 'ReduceDesc',
    'ga_se_excite_desc': 'SeExciteDesc', 'ga_se_apply_desc': 'SeApplyDesc', 'ga_bilinear_up2_bwd_desc': 'BilinearBwdDesc',
    'ga_sampler_desc': 'SamplerDesc', 'ga_dml_desc': 'DmlDesc', 'ga_maxpool2_desc': 'MaxpoolDesc', 'ga_image_io_desc': 'ImageIoDesc',
    'ga_axpby_desc': 'AxpbyDesc', 'ga_blur_desc': 'BlurDesc', 'ga_rep_sum_desc': 'RepSumDesc', 'ga_interleave2_desc': 'Interleave2Desc',
    'ga_maxpool3s2_desc': 'Maxpool3s2Desc', 'ga_avgpool_act_desc': 'AvgpoolActDesc', 'ga_gconv_desc': 'GconvDesc',
    'ga_prelu_desc': 'PreluDesc', 'ga_unary_desc': 'UnaryDesc', 'ga_modout_desc': 'ModoutDesc', 'ga_up2_blur_desc': 'Up2BlurDesc',
    'ga_pixelnorm_desc': 'PixelnormDesc', 'ga_latent_mix_desc': 'LatentMixDesc', 'ga_pool_denorm_desc': 'PoolDenormDesc',
    'ga_attn_desc': 'AttnDesc', 'ga_layernorm_desc': 'LayernormDesc', 'ga_resize2_crop_desc': 'Resize2CropDesc',
    'ga_dec_cell_desc': 'DecCellDesc', 'ga_dec_cell_halo_desc': 'DecCellHaloDesc', 'ga_avae_desc': 'AvaeDesc', 'ga_op': 'Op'}

# ---- the header parser: accepts the declaration forms ga_ops.h uses and raises ImportError on anything else, never guesses a type
_SCALARS = {'int': i32, 'float': f32, 'long': C.c_long, 'unsigned': C.c_uint, 'unsigned long': C.c_ulong}
_DECL = re.compile(r'\s*(?:const\s+)?(unsigned\s+long|unsigned|int|float|long|void|char|ga_\w+)\b\s*(\*{0,2})\s*(.*?)\s*', re.S)
_ITEM = re.compile(r'\s*(?:enum\s*\w*\s*\{([^{}]*)\}\s*;'                                                    # 1: enum body
                   r'|typedef\s+struct\s+(\w+)\s*\{((?:[^{}]|\{[^{}]*\})*)\}\s*(\w+)\s*;'                    # 2-4: struct
                   r'|([^;{}()]+?)\b(ga_\w+)\s*\(([^;{}()]*)\)\s*;)')                                         # 5-7: prototype
OpRow = collections.namedtuple('OpRow', 'kind value member cls entry')      # one GA_OP_LIST line


def _bad(text):
    raise ImportError(f'include/ga_ops.h: declaration form not supported by the binding: {" ".join(text.split())!r}')


def _decl(text):
    """'const float* x, y' -> ('float', '*', 'x, y')"""
    m = _DECL.fullmatch(text) or _bad(text)
    return ' '.join(m.group(1).split()), m.group(2), m.group(3)


class Header:
    """include/ga_ops.h as the binding needs it."""

    def __init__(self, src: str, names: dict):
        self.consts = {}    # every GA_* #define / enum constant -> int, the op kinds included
        self.types = {}     # C typedef -> ctypes class
        self.protos = {}    # function -> (restype, argtypes)
        self.ops = []       # GA_OP_LIST as OpRow's
        src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
        src = re.sub(r'//[^\n]*', ' ', src).replace('\\\n', ' ')
        src = re.sub(r'^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b', ' ', src, flags=re.S | re.M)
        self._rows = None
        for name, arg, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(\w+)(?:\((\w+)\))?[ \t]+(.*)$', src, flags=re.M):
            if name == 'GA_OP_LIST':
                row = r'\b%s\(\s*(\w+)\s*,\s*(\d+)\s*,\s*(\w+)\s*,\s*(\w+)\s*,\s*(\w+)\s*\)' % arg
                self._rows = re.findall(row, value)
                if re.sub(row, '', value).strip():
                    _bad(value)
            elif not arg and re.fullmatch(r'-?\d+', value.strip()):
                self.consts[name] = int(value)
        src = re.sub(r'^[ \t]*#.*$', ' ', src, flags=re.M)
        pos = 0
        while src[pos:].strip():
            m = _ITEM.match(src, pos) or _bad(src[pos:].split(';')[0])
            pos = m.end()
            enum, struct, body, alias, result, func, params = m.groups()
            if enum is not None:
                self._enum(enum)
            elif struct:
                if struct != alias:
                    _bad(m.group(0))
                if struct not in names:
                    _bad(f'typedef {struct}: no entry in _CLASS_NAMES')
                self.types[struct] = type(names[struct], (C.Structure,), {'_fields_': self._fields(body)})
            else:
                base, ptr, rest = _decl(result)
                if rest:
                    _bad(m.group(0))
                restype = C.c_char_p if (base, ptr) == ('char', '*') else self._value(result)
                params = [] if params.strip() == 'void' else params.split(',')
                self.protos[func] = (restype, [self._value(p) for p in params])
        self._op_list()

    def _enum(self, body):
        if re.fullmatch(r'\s*GA_OP_LIST\(\w+\)\s*', body):       # the kinds: taken from the list itself
            return
        for item in filter(str.strip, body.split(',')):
            m = re.fullmatch(r'\s*(\w+)\s*=\s*(-?\d+)\s*', item) or _bad('enum { %s }' % item)
            self.consts[m.group(1)] = int(m.group(2))

    def _op_list(self):
        if self._rows and not self.ops:
            for kind, value, member, desc, entry in self._rows:
                if desc not in self.types:
                    _bad(f'GA_OP_LIST: {desc} is not a struct typedef above the first use of the list')
                self.ops.append(OpRow(kind, int(value), member, self.types[desc], entry))
                self.consts[kind] = int(value)
        return self.ops

    def _fields(self, body):
        out = []
        for stmt in filter(str.strip, body.split(';')):
            m = re.fullmatch(r'\s*union\s*\{\s*GA_OP_LIST\(\w+\)\s*\}\s*(\w+)\s*', stmt)
            if m:
                out.append((m.group(1), type('OpUnion', (C.Union,), {'_fields_': [(o.member, o.cls) for o in self._op_list()]})))
                continue
            base, ptr, rest = _decl(stmt)
            names = rest.split(',')
            if ptr and len(names) > 1:      # 'float* a, b' makes b a float: not a form the header uses
                _bad(stmt)
            typ = fp if ptr else _SCALARS.get(base) or self.types.get(base) or _bad(stmt)
            for n in names:
                m = re.fullmatch(r'\s*(\w+)\s*((?:\[\d+\]){0,2})\s*', n) or _bad(stmt)
                dims = [int(d) for d in re.findall(r'\d+', m.group(2))]
                out.append((m.group(1), typ * math.prod(dims) if dims else typ))    # a[2][2] flattens to a[4]
        return out

    def _value(self, text):
        """ctypes type of a parameter or a result"""
        base, ptr, name = _decl(text)
        if not re.fullmatch(r'\w*', name) or base.startswith('ga_') and (base not in self.types or ptr != '*'):
            _bad(text)
        if base.startswith('ga_'):
            return C.POINTER(self.types[base])
        return C.c_void_p if ptr else _SCALARS.get(base) or _bad(text)


_H = Header(open(HEADER_PATH).read(), _CLASS_NAMES)
globals().update(_H.consts)                                          # GA_OK, GA_E_*, GA_ACT_*, GA_CONV_*, GA_AVAE_*, GA_OP_*, ...
globals().update({c.__name__: c for c in _H.types.values()})         # ConvDesc, ..., Op
Op = _H.types['ga_op']
ABI_VERSION = _H.consts['GA_ABI_VERSION']   # descriptor layouts + entry points; _load() refuses a library built from another header
ERRORS = {v: k for k, v in _H.consts.items() if k == 'GA_OK' or k.startswith('GA_E_')}
EXPORTS = list(_H.protos)
_OP_OF = {o.cls: o for o in _H.ops}
# descriptor class -> its own entry point, where the header declares one as (const desc*, void* stream)
_DIRECT = {o.cls: o.entry for o in _H.ops if _H.protos.get(o.entry) == (C.c_int, [C.POINTER(o.cls), C.c_void_p])}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                          f'or `make -C gen_adversarial_amd/csrc` — there is no CPU fallback on the product path')
    lib = C.CDLL(LIB_PATH)
    if lib.ga_abi_version() != ABI_VERSION:
        raise ImportError(f'ABI mismatch: {LIB_PATH} reports GA_ABI_VERSION {lib.ga_abi_version()}, include/ga_ops.h says '
                          f'{ABI_VERSION}: rebuild with `make -C gen_adversarial_amd/csrc`')
    for name, (restype, argtypes) in _H.protos.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
    if lib.ga_sizeof_op() != C.sizeof(Op):
        raise ImportError(f'ABI mismatch: library ga_op is {lib.ga_sizeof_op()} bytes, binding is {C.sizeof(Op)}')
    return lib


lib = _load()


class GaError(RuntimeError):
    pass


def check(rc: int, what: str = ''):
    if rc != 0:
        extra = f' ({lib.ga_last_hip_error().decode()})' if ERRORS.get(rc) == 'GA_E_LAUNCH' else ''
        raise GaError(f'{what}: {ERRORS.get(rc, rc)}{extra}')


def make_op(desc) -> Op:
    row = _OP_OF[type(desc)]
    op = Op()
    op.kind = row.value
    setattr(op.u, row.member, desc)
    return op


def run(desc, stream: int = 0):
    """Launch one op: through its own C entry point where it has one, else (axpby, rep_sum, pixelnorm) as a one-op plan."""
    name = _DIRECT.get(type(desc))
    if name:
        check(getattr(lib, name)(C.byref(desc), stream), name)
    else:
        check(lib.ga_plan_run(C.byref(make_op(desc)), 1, stream, None), _OP_OF[type(desc)].kind)


class Plan:
    """A flat list of ops replayed by one ga_plan_run call."""

    def __init__(self):
        self.descs = []
        self.names = []
        self._arr = None

    def add(self, desc, name: str = ''):
        self.descs.append(desc)
        self.names.append(name)
        self._arr = None

    def finalize(self):
        arr = (Op * len(self.descs))()
        for i, d in enumerate(self.descs):
            arr[i] = make_op(d)
        self._arr = arr
        return self

    def __len__(self):
        return len(self.descs)

    def run(self, stream: int = 0, start: int = 0, end: int = None):
        """Replay ops[start:end) with one C call."""
        if self._arr is None:
            self.finalize()
        end = len(self.descs) if end is None else end
        if end <= start:
            return
        failed = C.c_int(-1)
        first = C.cast(C.byref(self._arr, start * C.sizeof(Op)), C.POINTER(Op))
        rc = lib.ga_plan_run(first, end - start, stream, C.byref(failed))
        if rc != 0:
            check(rc, f'plan op #{start + failed.value} ({self.names[start + failed.value]})')

    def capture(self, stream: int):
        """capture one replay into a HIP graph (stream must not be the NULL stream); returns an opaque handle"""
        if self._arr is None:
            self.finalize()
        h = C.c_void_p()
        check(lib.ga_graph_capture(self._arr, len(self.descs), stream, C.byref(h)), 'ga_graph_capture')
        return h

    @staticmethod
    def launch_graph(handle, stream: int):
        check(lib.ga_graph_launch(handle, stream), 'ga_graph_launch')

    @staticmethod
    def destroy_graph(handle):
        lib.ga_graph_destroy(handle)

    def profile(self, stream: int = 0):
        """per-op device milliseconds of one replay."""
        if self._arr is None:
            self.finalize()
        out = (f32 * len(self.descs))()
        check(lib.ga_plan_profile(self._arr, len(self.descs), stream, out), 'ga_plan_profile')
        return list(out)

    def time(self, stream: int = 0, iters: int = 1, per_conv: bool = False):
        if self._arr is None:
            self.finalize()
        total, conv, nconv = f32(0), f32(0), C.c_long(0)
        rc = lib.ga_plan_time(self._arr, len(self.descs), stream, iters, C.byref(total),
                              C.byref(conv) if per_conv else None, C.byref(nconv) if per_conv else None)
        check(rc, 'ga_plan_time')
        return total.value, conv.value, nconv.value
