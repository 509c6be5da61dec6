"""
CPU: the refusal half of the C ABI of include/ga_ops.h, "return value <0 = rejected, nothing launched", held to the header and to
tests/planref.py for every non-conv entry point (ga_conv2d has tests/test_conv_refusals_gpu.py; only part 2 below touches it).

What "accepted" looks like without a device.  Validation returns before the first HIP call, so a refusal (-1, -2, -3) is observable
on a machine with no GPU.  A descriptor that passes validation reaches hipLaunchKernelGGL with no device; the launch fails and
check_launch() returns GA_E_LAUNCH.  Observed on the CPU machine with a valid ga_prelu descriptor in a child process: -4
(test_an_accepted_descriptor_returns_launch_error_without_a_device holds that).  From there on "accepted" = not -1, -2 or -3.
The module skips itself where torch.cuda.is_available(): there an accepted case would launch a kernel on made-up addresses.

  1. Mutation table.  Bases: the synthetic descriptors of tests/test_planref_cpu.py (KINDS) plus the ones below: every type of
     planref.HANDLERS, every mode of ga_sampler_mix / ga_latent_mix / ga_avae, ga_dec_cell, ga_dec_cell_halo and the scalar entry
     points.  One mutation at a time, generated from the descriptor's _fields_ and the handler's operands (MUTATIONS names the
     kinds).  A mutant is illegal when planref refuses it or a rule of the header names it; the library must then refuse it, with the
     code the header names where it names one.  A mutant neither oracle calls illegal must be accepted: header, planref and
     library say the same thing.  A (type, mutation) pair with no mutant is listed in NOT_APPLICABLE with its reason.
  2. Every descriptor of every dry-run plan (planzoo.dry_engines, planzoo.device_engines) is accepted by its entry point as the
     engine wrote it: the guard against over-strict validation, and the evidence behind the header's alignment sentences.
"""
import collections
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest
import torch

if torch.cuda.is_available():
    pytest.skip('an accepted descriptor would launch a kernel on made-up addresses: this module runs where there is no device',
                allow_module_level=True)

import planref as PR
import planzoo
from gen_adversarial_amd import _lib as L
from test_planref_cpu import KINDS, SMP, P

REFUSED = (L.GA_E_BADARG, L.GA_E_ALIGN, L.GA_E_UNSUPPORTED)
BADARG, ALIGN, UNSUPPORTED = L.GA_E_BADARG, L.GA_E_ALIGN, L.GA_E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------- entry points
class SplitBf16Args(C.Structure):
    """ga_split_bf16's scalar arguments as a descriptor of this test's own, so that the same generator mutates them"""
    _fields_ = [('w', L.fp), ('hi', L.fp), ('lo', L.fp), ('n', C.c_long)]


SCALAR = {L.AxpbyDesc: lambda d: L.lib.ga_axpby(d.x, d.y, d.n, d.alpha, d.beta, None),
          L.RepSumDesc: lambda d: L.lib.ga_rep_sum(d.x, d.y, d.rows, d.inner, d.rep, d.accumulate, None),
          L.PixelnormDesc: lambda d: L.lib.ga_pixelnorm(d.x, d.y, d.rows, d.C, None),
          SplitBf16Args: lambda d: L.lib.ga_split_bf16(d.w, d.hi, d.lo, d.n, None)}


def call(d):
    """the return code of the descriptor's entry point"""
    if type(d) in SCALAR:
        return SCALAR[type(d)](d)
    return getattr(L.lib, L._DIRECT[type(d)])(C.byref(d), None)


def test_an_accepted_descriptor_returns_launch_error_without_a_device():
    code = ('import ctypes as C\nfrom gen_adversarial_amd import _lib as L\nd = L.PreluDesc()\nd.x, d.slope, d.y = 4096, 8192, 12288\n'
            'd.rows, d.C = 4, 8\nprint("rc", L.lib.ga_prelu(C.byref(d), None))\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-c', code], cwd=root, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[-2:] == ['rc', str(L.GA_E_LAUNCH)], out.stdout


# ---------------------------------------------------------------------------------------------------- bases
DC = dict(N=2, H=8, W=16, C=128, Hd=768)                # two 128-pixel images = one 256-pixel workgroup
HC = dict(N=1, H=8, W=16, Cin=32, Cout=32, Hd=192)
_CELL = ('x', 'w1_hi', 'w1_lo', 'b1', 'wd', 'wd_bwd', 'bd', 'w2_hi', 'w2_lo', 'b2')
MORE = [
    ('modout', L.ModoutDesc, dict(N=2, P=16, C=8, act=5), P('t', 'scale', 'add', 'out')),
    ('modout_bwd', L.ModoutDesc, dict(N=2, P=16, C=8, act=5, backward=1), P('t', 'scale', 'add', 'dout', 'dt')),
    ('modout_t_planes', L.ModoutDesc, dict(N=2, P=24, C=8, act=5, W=6, ld_planes=16), P('t_planes0', 't_planes1', 't_planes2', 't_planes3', 'scale', 'add', 'out')),
    ('modout_bwd_planes_red', L.ModoutDesc, dict(N=2, P=24, C=8, act=5, backward=1, W=6, ld_planes=16, ws_floats=64),
     P('t_planes0', 't_planes1', 't_planes2', 't_planes3', 'dt_planes0', 'dt_planes1', 'dt_planes2', 'dt_planes3', 'scale', 'add', 'dout', 'red', 'ws')),
    ('reduce', L.ReduceDesc, dict(N=2, P=9, C=12, scale=0.5, ws_floats=48), P('a', 'b', 'out', 'ws')),
    ('reduce_formed_scaled', L.ReduceDesc, dict(N=2, P=9, C=12, scale=0.5), P('a_src', 'a_w', 'b', 'out', 'gate', 'skip', 'scaled')),
    ('interleave2', L.Interleave2Desc, dict(N=6, H=4, W=4, C=8, dact_act=3, lds=16, dact_rep=3),
     P('s0', 's1', 's2', 's3', 'y', 'dact_x', 'dact_scale', 'dact_shift', 'addend', 'addend2')),
    ('attn', L.AttnDesc, dict(N=2, Tq=16, Tk=5, heads=2, dh=16, scale=0.25, ldq=96, ldk=96, ldv=96, ldo=32), P('q', 'k', 'v', 'out', 'p')),
    ('attn_bwd', L.AttnDesc, dict(N=2, Tq=16, Tk=5, heads=2, dh=16, scale=0.25, ldq=96, ldk=96, ldv=96, ldo=32, lddq=96, lddk=96, lddv=96, backward=1),
     P('q', 'k', 'v', 'p', 'dout', 'ds', 'dq', 'dk', 'dv')),
    ('layernorm', L.LayernormDesc, dict(rows=5, C=12, eps=1e-5), P('a', 'b', 'gamma', 'beta', 'y', 'stats')),
    ('layernorm_bwd', L.LayernormDesc, dict(rows=5, C=12, eps=1e-5, backward=1, accumulate=1), P('a', 'b', 'gamma', 'stats', 'dy', 'dx')),
    ('sampler', L.SamplerDesc, dict(SMP, alpha=0.25, one_minus_alpha=0.75, q_rep=2), P('mu_q', 'p', 'eps', 'z')),
    ('sampler_alpha_rows', L.SamplerDesc, dict(SMP, q_rep=2, alpha_ld=6, alpha_col=1), P('mu_q', 'p', 'eps', 'z', 'alpha_rows')),
    ('latent_mix', L.LatentMixDesc, dict(R=4, J=3, D=8, rep=2), P('codes', 'avg', 'styles', 'alpha', 'out')),
    ('se_excite', L.SeExciteDesc, dict(N=2, C=8, Hd=4, P=6, res_scale=0.1), P('t', 'w1', 'b1', 'w2', 'b2', 'hid', 'gate', 'skip', 'out')),
    ('se_excite_unfused_bwd', L.SeExciteDesc, dict(N=3, C=8, Hd=4, P=6, res_scale=0.1, backward=1),
     P('w1', 'b1', 'w2', 'b2', 'hid', 'gate', 'dgate', 'pro_scale', 'pro_shift')),
    ('se_apply_mode2', L.SeApplyDesc, dict(N=2, H=4, W=4, C=8, skip_mode=2, res_scale=0.1), P('skip', 't', 'gate', 'out')),
    ('dw_up2', L.DwDesc, dict(N=2, H=4, W=8, C=8, pro_act=1, up2=1), P('x', 'w', 'bias', 'y')),
    ('maxpool', L.MaxpoolDesc, dict(N=2, H=4, W=4, C=4), P('x', 'y')),
    ('maxpool3s2', L.Maxpool3s2Desc, dict(N=2, H=6, W=6, C=4), P('x', 'y')),
    ('avgpool_act', L.AvgpoolActDesc, dict(N=2, P=5, C=8, act=3), P('x', 'y')),
    ('prelu', L.PreluDesc, dict(rows=5, C=8), P('x', 'slope', 'y')),
    ('unary_rsqrt', L.UnaryDesc, dict(n=16, mode=2, eps=1e-8), P('x', 'y')),
    ('resize2_crop', L.Resize2CropDesc, dict(N=2, H=4, W=4, C=4, crop=1), P('x', 'y')),
    ('image_io_s2d', L.ImageIoDesc, dict(N=4, C=3, H=4, W=4, rep=2, ld=8, s2d=1), P('x_nchw', 'y_nhwc')),
    ('blur_two_pass', L.BlurDesc, dict(planes=2, H=128, W=128, k=15), P('x', 'y', 'taps', 'tmp')),
    ('gconv_bias', L.GconvDesc, dict(N=2, Hi=4, Wi=4, Ho=2, Wo=2, C=8, cg=4, KH=3, KW=3, stride=2, pad=1, pro_act=3), P('x', 'w', 'bias', 'y')),
    ('avae_adain', L.AvaeDesc, dict(mode=0, N=2, P=6, C=4), P('x', 'a', 'b', 'c', 'y', 'y2')),
    ('avae_avgpool_bwd', L.AvaeDesc, dict(mode=1, backward=1, N=4, H=4, W=4, C=4, k=2, act_rep=2), P('x', 'dy', 'y')),
    ('avae_pixelnorm', L.AvaeDesc, dict(mode=2, N=2, C=8), P('x', 'y')),
    ('avae_sample', L.AvaeDesc, dict(mode=3, N=2, P=6, C=4, f0=0.6), P('x', 'a', 'y')),
    ('dec_cell', L.DecCellDesc, dict(DC), P(*_CELL, 'y')),
    ('dec_cell_bwd', L.DecCellDesc, dict(DC, N=4, backward=1, act_rep=2), P(*_CELL, 'dout', 'pro_scale', 'pro_shift', 'y')),
    ('dec_cell_halo', L.DecCellHaloDesc, dict(HC), P(*_CELL, 'y')),
    ('dec_cell_halo_bwd', L.DecCellHaloDesc, dict(HC, backward=1), P(*_CELL, 'w1t_hi', 'w1t_lo', 'dout', 'pro_scale', 'pro_shift', 'addend', 'addend2', 'y')),
    ('split_bf16', SplitBf16Args, dict(n=24), P('w', 'hi', 'lo')),
]
def make(cls, f, ptr):
    return PR.make_desc(cls, f, ptr)


# every base with all its non-pointer fields, as the descriptor holds them (the unset ones 0)
BASES = [(c[0], c[1], PR.desc_fields(make(c[1], c[2], c[3]))[0], dict(c[3])) for c in list(KINDS) + MORE]
TYPES = sorted({b[1] for b in BASES}, key=lambda c: c.__name__)


def planref_verdict(cls, f, ptr):
    """None where planref lays the descriptor's operands out, else why it cannot (PlanRefError, or an extent it cannot even form).
    Handler.operands alone: check_fields also refuses a pointer or a field that is set and not read, which is no extent and which
    the library ignores (ws without red, act_rep on a forward pass is the header's business)."""
    if cls not in PR.HANDLERS:
        return None
    try:
        PR.HANDLERS[cls].operands(dict(PR.desc_fields(make(cls, f, ptr))[0]), set(ptr))
    except PR.PlanRefError as ex:
        return str(ex)
    except (KeyError, ZeroDivisionError, ValueError) as ex:       # a selector with no layout, k = 0, a negative extent
        return f'{type(ex).__name__}: {ex}'
    return None


def test_every_type_has_a_base_and_every_base_is_legal():
    assert set(TYPES) == set(PR.HANDLERS) | {L.DecCellDesc, L.DecCellHaloDesc, SplitBf16Args}
    modes = collections.defaultdict(set)
    for _, cls, f, ptr in BASES:
        modes[cls].add((f.get('mode', 0), f.get('backward', 0)))
        assert all(v % 4096 == 0 for v in ptr.values())
    assert {m for m, _ in modes[L.SamplerDesc]} == {0, 1, 2} and {b for _, b in modes[L.LatentMixDesc]} == {0, 1, 2}
    assert modes[L.AvaeDesc] == set(itertools.product(range(4), range(2)))
    bad = []
    for name, cls, f, ptr in BASES:
        why = planref_verdict(cls, f, ptr)
        rc = call(make(cls, f, ptr))
        if why or rc in REFUSED:
            bad.append(f'{name}: planref {why}, library {L.ERRORS.get(rc, rc)}')
    assert not bad, '\n'.join(bad)


# ---------------------------------------------------------------------------------------------------- the header's rules
MUTATIONS = ('null', 'size', 'pitch_low', 'pitch_mod4', 'rep_div', 'rep_fwd', 'chan_mod4', 'odd', 'selector', 'align')
FLAGS = {'backward', 'up2', 'pool2', 'eps_nchw', 'accumulate', 's2d', 'dact_prelu', 'up', 'variant'}       # any non-zero value = set
NOT_SIZES = {'alpha_col', 'crop', 'band', 'radius', 'pad', 'ws_floats'}            # offsets and bounds with rules of their own
ACTS = {'act', 'pro_act', 'dact_act'}
# pointers the header marks optional ("or NULL", "optional"), with the condition it puts on that (fields, the other pointers): a NULL
# there is legal unless planref says what else it breaks
ANY = lambda f, p: True
FWD, BWD = (lambda f, p: not f['backward']), (lambda f, p: bool(f['backward']))
OPTIONAL = {
    L.DwDesc: dict(bias=ANY, dact_x=ANY), L.ReduceDesc: dict(b=ANY, ws=ANY, skip=ANY), L.SeExciteDesc: dict(skip=ANY, out=ANY),
    L.SeApplyDesc: dict(skip=lambda f, p: f['skip_mode'] == 0),
    L.SamplerDesc: dict(p=lambda f, p: f['mode'] != 1 and 'dp' not in p, alpha_rows=ANY),          # dp is written with p, and only then
    L.DmlDesc: dict(img_nchw=lambda f, p: 'img_nhwc' in p, img_nhwc=lambda f, p: 'img_nchw' in p, dimg_nhwc=lambda f, p: 'dimg_nchw' in p,
                    dimg_nchw=lambda f, p: 'dimg_nhwc' in p),
    L.GconvDesc: dict(bias=ANY, dact_x=ANY), L.ModoutDesc: dict(scale=ANY, add=ANY, red=ANY, ws=lambda f, p: 'red' not in p),
    L.LatentMixDesc: dict(avg=ANY), L.PoolDenormDesc: dict(dy_nchw=ANY), L.LayernormDesc: dict(b=ANY),
    L.BlurDesc: dict(tmp=lambda f, p: (2 * f['H'] * f['W'] + f['k']) * 4 <= 64 * 1024),
    L.Interleave2Desc: dict(s0=ANY, s1=ANY, s2=ANY, s3=ANY, addend=ANY, addend2=ANY, dact_x=lambda f, p: not f['dact_prelu'],
                            dact_scale=lambda f, p: 'dact_shift' not in p, dact_shift=lambda f, p: 'dact_scale' not in p or f['dact_prelu']),
    L.DecCellDesc: dict(b2=BWD, wd_bwd=FWD),                                                        # the other direction's operands
    L.DecCellHaloDesc: dict(addend=ANY, addend2=ANY, b2=BWD, wd_bwd=FWD)}
# size fields a mode does not read (the header gives them no meaning there): not mutated
UNREAD = {(L.SeExciteDesc, 'P'): lambda f, p: not f['backward'] and 't' not in p}                # the unfused forward has no pixel axis
# pitch fields the header holds to a multiple of 4 floats
PITCH_MOD4 = {L.AttnDesc: {'ldq', 'ldk', 'ldv', 'ldo', 'lddq', 'lddk', 'lddv'}, L.ModoutDesc: {'ld_planes'}, L.Interleave2Desc: {'lds'},
              L.PoolDenormDesc: {'ld'}}
# replica fields the header calls backward only
BACKWARD_ONLY = {L.SeExciteDesc: 'act_rep', L.SamplerDesc: 'act_rep', L.DmlDesc: 'act_rep', L.MaxpoolDesc: 'act_rep', L.Maxpool3s2Desc: 'act_rep',
                 L.AvgpoolActDesc: 'act_rep', L.AvaeDesc: 'act_rep', L.DecCellDesc: 'act_rep', L.ImageIoDesc: 'cot_rep'}
# the channel count of each type, and whether the header holds it to a multiple of 4 (attn: dh % 16)
CHANNELS = {L.DwDesc: ('C', True), L.ReduceDesc: ('C', True), L.SeExciteDesc: ('C', None), L.SeApplyDesc: ('C', True), L.BilinearBwdDesc: ('C', True),
            L.SamplerDesc: ('NL', False), L.MaxpoolDesc: ('C', True), L.AvgpoolActDesc: ('C', True), L.PixelnormDesc: ('C', False),
            L.PreluDesc: ('C', True), L.ModoutDesc: ('C', True), L.Up2BlurDesc: ('C', True), L.LatentMixDesc: ('D', True),
            L.LayernormDesc: ('C', True), L.Resize2CropDesc: ('C', True), L.AttnDesc: ('dh', True), L.Interleave2Desc: ('C', True),
            L.Maxpool3s2Desc: ('C', True), L.ImageIoDesc: ('C', False), L.GconvDesc: ('cg', True), L.AvaeDesc: ('C', None),
            L.DecCellDesc: ('C', True), L.DecCellHaloDesc: ('Hd', True), L.RepSumDesc: ('inner', False)}
AVAE_MOD4 = {0: True, 1: True, 2: False, 3: False}         # ADAIN and AVGPOOL read channel quads, PIXELNORM and SAMPLE scalars
# H / W the header calls even, as a predicate on the base's fields
EVEN = {L.MaxpoolDesc: lambda f: True, L.Maxpool3s2Desc: lambda f: True, L.Interleave2Desc: lambda f: True, L.PoolDenormDesc: lambda f: True,
        L.DwDesc: lambda f: f.get('up2') or f.get('pool2'), L.SeApplyDesc: lambda f: f.get('skip_mode') == 1, L.ImageIoDesc: lambda f: f.get('s2d'),
        L.ModoutDesc: lambda f: f.get('W'), L.DecCellDesc: lambda f: True, L.DecCellHaloDesc: lambda f: True}
# selectors the header enumerates: (type, field) -> last value
SELECTORS = {(L.SamplerDesc, 'mode'): 2, (L.SeApplyDesc, 'skip_mode'): 2, (L.AvaeDesc, 'mode'): 3, (L.UnaryDesc, 'mode'): 3,
             (L.LatentMixDesc, 'backward'): 2}
# pointers the header holds to 16 bytes, per type (a predicate on the base's fields where it depends on the mode)
ALL = object()
ALIGNED = {
    L.DwDesc: ALL, L.GconvDesc: ALL, L.SeApplyDesc: ALL, L.BilinearBwdDesc: ALL, L.AttnDesc: ALL, L.Resize2CropDesc: ALL,
    L.LayernormDesc: {'a', 'b', 'gamma', 'beta', 'y', 'dy', 'dx'},
    L.ReduceDesc: {'a', 'b', 'out', 'a_src', 'a_w', 'gate', 'skip', 'scaled'},
    L.SeExciteDesc: {'t', 'dout', 'skip', 'out'},
    L.DecCellDesc: {'x', 'w1_hi', 'w1_lo', 'wd', 'wd_bwd', 'bd', 'w2_hi', 'w2_lo', 'dout', 'pro_scale', 'pro_shift', 'y'},
    L.DecCellHaloDesc: {'x', 'y', 'w1_hi', 'w1_lo', 'w2_hi', 'w2_lo', 'wd', 'bd', 'dout', 'pro_scale', 'pro_shift', 'wd_bwd', 'w1t_hi', 'w1t_lo',
                        'addend', 'addend2'},
    L.MaxpoolDesc: ALL, L.Maxpool3s2Desc: ALL, L.PreluDesc: ALL, L.Up2BlurDesc: ALL, L.Interleave2Desc: ALL, L.AvgpoolActDesc: ALL,
    L.PoolDenormDesc: {'x', 'y', 'dy', 'dx'}, L.ModoutDesc: ALL,
    L.LatentMixDesc: {'codes', 'avg', 'styles', 'out', 'dout', 'dcodes'}}


def aligned_pointers(cls, f, ptr):
    if cls is L.AvaeDesc:
        return {0: {'x', 'b', 'c', 'dy', 'y'}, 1: {'x', 'y', 'dy'}}.get(f['mode'], set())
    if cls is L.LatentMixDesc and f.get('backward') == 2:
        return {'codes', 'avg', 'styles', 'dout'}                         # `out` is the [R, J] table, one float per wavefront
    if cls is L.DecCellHaloDesc and not f.get('backward'):
        return ALIGNED[cls] - {'wd_bwd'}
    if cls is L.ModoutDesc:                                       # red: one float per thread; ws only on the path that sums through it
        return set(ptr) - {'ws', 'red'} | ({'ws'} if f.get('backward') and 'red' in ptr else set())
    if cls is L.ReduceDesc and not ('ws' in ptr and f['P'] >= 4096):
        return ALIGNED[cls]
    a = ALIGNED.get(cls, set())
    return set(ptr) if a is ALL else a


# the code the header names per mutation; None = refused, no code named.  EXACT: the (type, mutation, field) it words otherwise
CODE = dict(null=BADARG, size=BADARG, pitch_low=BADARG, pitch_mod4=UNSUPPORTED, rep_div=BADARG, rep_fwd=BADARG, chan_mod4=UNSUPPORTED,
            odd=None, selector=None, align=ALIGN)
EXACT = {
    (L.AttnDesc, 'size', 'Tq'): UNSUPPORTED,             # "Tq is fixed"
    (L.GconvDesc, 'chan_mod4', 'cg'): BADARG,            # C = groups * cg breaks first
    (L.DecCellDesc, 'size', None): UNSUPPORTED,          # "Shapes: ga_dec_cell_supported()"
    (L.DecCellDesc, 'chan_mod4', 'C'): UNSUPPORTED,
    (L.DecCellHaloDesc, 'size', None): UNSUPPORTED,      # ga_dec_cell_halo_supported
    (L.BlurDesc, 'size', 'k'): None,
}
NOT_APPLICABLE = {}


def na(kind, reason, *types):
    for t in types:
        NOT_APPLICABLE[(t, kind)] = reason


_NO_PITCH = [t for t in TYPES if not any(n.startswith('ld') or n == 'alpha_ld' for n, _ in t._fields_)]
na('pitch_low', 'the descriptor has no pitch field: its tensors are dense', *_NO_PITCH)
na('pitch_mod4', 'no pitch field, or the header asks no multiple of 4 of it', *[t for t in TYPES if t not in PITCH_MOD4])
_NO_REP = [t for t in TYPES if not any(n.endswith('rep') for n, _ in t._fields_)]
na('rep_div', 'the descriptor has no replica field', *_NO_REP)
na('rep_fwd', 'no replica field the header calls backward only', *[t for t in TYPES if t not in BACKWARD_ONLY])
na('chan_mod4', 'no channel axis: flat element counts, image planes, or 10 * nmix logits under a pitch',
   L.AxpbyDesc, L.UnaryDesc, SplitBf16Args, L.BlurDesc, L.DmlDesc, L.PoolDenormDesc)
na('odd', 'no H / W field', *[t for t in TYPES if not {'H', 'W', 'h', 'w', 'Hi', 'Wi'} & {n for n, ty in t._fields_ if ty is L.i32}])
na('odd', 'the header asks no even size, and the bases are 3 x 3 already', L.BilinearBwdDesc, L.Up2BlurDesc)
na('selector', 'no mode or activation selector', *[t for t in TYPES if not any((t, n) in SELECTORS or n in ACTS for n, _ in t._fields_)])


def is_pointer(typ):
    return typ is L.fp or (hasattr(typ, '_length_') and typ._type_ is L.fp)


def field_class(cls, name, typ):
    if name.startswith('_reserved') or typ is L.f32:
        return None
    if is_pointer(typ):
        return 'pointer'
    if name.startswith('ld') or name == 'alpha_ld':
        return 'pitch'
    if name.endswith('rep'):
        return 'rep'
    if (cls, name) in SELECTORS or name in ACTS:
        return 'selector'
    if name in FLAGS or name in NOT_SIZES:
        return None
    return 'size'


def not_mod4(v):
    return v + 1 if v % 4 == 0 else v


def pitch_low(cls, f, ptr, name):
    """one below the channels the pitch's operands use: from the handler's operands, the pitch moved aside to find them"""
    h = PR.HANDLERS.get(cls)
    if h is None:
        return None
    has = set(ptr)
    try:
        now = h.operands(f, has)
        moved = h.operands(dict(f, **{name: f[name] + 4096}), has)
    except PR.PlanRefError:
        return None
    used = [now[k].used for k in now if k in has and (now[k].ld, now[k].lead) != (moved[k].ld, moved[k].lead) and now[k].used < now[k].ld]
    if used:                                              # a pitch held to % 4 keeps that: one mutation at a time
        return (max(used) - 1) // 4 * 4 if name in PITCH_MOD4.get(cls, ()) else max(used) - 1
    for v in range(f[name] - 1, 0, -1):                  # the pitch IS the extent (image_io y, dml img, the alpha tables): ask planref
        if planref_verdict(cls, dict(f, **{name: v}), ptr) and (cls not in PITCH_MOD4 or v % 4 == f[name] % 4):
            return v
    return None


def mutants(cls, f, ptr):
    """(mutation, field, fields, pointers, the header's verdict): verdict = a code, 'refused', or None where the header names nothing"""
    h = PR.HANDLERS.get(cls)
    rows = getattr(h, 'rows', 'N') if h else ('n' if cls is SplitBf16Args else 'N')
    bw = f.get('backward', 0)
    ch, mod4 = CHANNELS.get(cls, (None, None))
    if cls is L.AvaeDesc:
        mod4 = AVAE_MOD4[f['mode']]
    if cls is L.SeExciteDesc:
        mod4 = 't' in ptr                                          # the fused form walks the pixels in channel quads
    for name, typ in cls._fields_:
        kind = field_class(cls, name, typ)
        v = f.get(name, 0)
        if kind == 'pointer':
            for k in sorted(p for p in ptr if p == name or (p[:-1] == name and p[-1].isdigit())):
                rest = {a: b for a, b in ptr.items() if a != k}
                optional = OPTIONAL.get(cls, {}).get(k, lambda f, p: False)(f, rest)
                yield 'null', k, f, rest, (None if optional else CODE['null'])
                al = aligned_pointers(cls, f, ptr)
                yield 'align', k, f, dict(ptr, **{k: ptr[k] + 4}), (CODE['align'] if k in al else None)
        elif kind == 'size' and v and not UNREAD.get((cls, name), lambda f, p: False)(f, ptr):
            for bad in (0, -1):
                yield 'size', name, dict(f, **{name: bad}), ptr, EXACT.get((cls, 'size', name), EXACT.get((cls, 'size', None), CODE['size']))
        elif kind == 'pitch' and v:
            low = pitch_low(cls, f, ptr, name)
            if low is not None:
                yield 'pitch_low', name, dict(f, **{name: low}), ptr, CODE['pitch_low']
            if name in PITCH_MOD4.get(cls, ()):
                yield 'pitch_mod4', name, dict(f, **{name: not_mod4(v)}), ptr, CODE['pitch_mod4']
        elif kind == 'rep':
            if v > 1 and rows and (h is None or any(int(r) > 1 for r in h.reps(f, set(ptr)))):
                yield 'rep_div', name, dict(f, **{name: f[rows] + 1}), ptr, CODE['rep_div']
            if BACKWARD_ONLY.get(cls) == name and not bw and f.get('mode') != 2 and f[rows] % 2 == 0:
                yield 'rep_fwd', name, dict(f, **{name: 2}), ptr, CODE['rep_fwd']
        elif kind == 'selector':
            last = SELECTORS.get((cls, name), L.GA_ACT_FLRELU)
            for bad in (last + 1, -1):
                # an activation outside enum ga_act selects none (the header's conventions): legal, and accepted
                yield 'selector', name, dict(f, **{name: bad}), ptr, (None if name in ACTS else 'refused')
        if name == ch and v:
            g = dict(f, **{name: not_mod4(v)})
            yield 'chan_mod4', name, g, ptr, (EXACT.get((cls, 'chan_mod4', name), CODE['chan_mod4']) if mod4 else None)
        if name in ('H', 'W', 'h', 'w', 'Hi', 'Wi') and v and v % 2 == 0:
            yield 'odd', name, dict(f, **{name: v + 1}), ptr, ('refused' if EVEN.get(cls, lambda f: False)(f) else None)


def test_mutation_table():
    """one line per descriptor type: bases, mutants run, mutants refused, not-applicable pairs"""
    stats = {t: collections.Counter() for t in TYPES}
    ran, fails = set(), []
    for base, cls, f, ptr in BASES:
        stats[cls]['bases'] += 1
        for kind, field, f2, p2, header in mutants(cls, f, ptr):
            ran.add((cls, kind))
            why = planref_verdict(cls, f2, p2)
            rc = call(make(cls, f2, p2))
            stats[cls]['run'] += 1
            stats[cls]['refused'] += rc in REFUSED
            tag = f'{base} [{kind} {field}={f2.get(field, p2.get(field, 0))}]: library {L.ERRORS.get(rc, rc)}'
            if header is not None or why:
                if rc not in REFUSED:
                    fails.append(f'{tag}, ILLEGAL (header: {L.ERRORS.get(header, header)}; planref: {why}) and not refused')
                elif header in REFUSED and rc != header:
                    fails.append(f'{tag}, the header names {L.ERRORS[header]}')
            elif rc in REFUSED:
                fails.append(f'{tag}, refused, and neither the header nor planref calls it illegal')
    print()
    for t in TYPES:
        n_a = sorted(k for (c, k) in NOT_APPLICABLE if c is t)
        print(f'{t.__name__[:-4]:<13} bases {stats[t]["bases"]:>2}  mutants {stats[t]["run"]:>3}  refused {stats[t]["refused"]:>3}  n/a {len(n_a)}: {", ".join(n_a)}')
    assert not fails, f'{len(fails)} disagreements\n' + '\n'.join(fails)
    pairs = set(itertools.product(TYPES, MUTATIONS))
    assert ran | set(NOT_APPLICABLE) == pairs, sorted((c.__name__, k) for c, k in pairs - ran - set(NOT_APPLICABLE))
    assert not ran & set(NOT_APPLICABLE), sorted((c.__name__, k) for c, k in ran & set(NOT_APPLICABLE))


# ---------------------------------------------------------------------------------------------------- part 2
def test_every_shipped_descriptor_is_accepted():
    """forward and backward dry-run plans of every engine of the zoo, each descriptor through its own entry point as the engine wrote it"""
    more = ((name, build()) for name, build in planzoo.device_engines('cpu', dry_run=True))
    per, off16, fails = collections.Counter(), collections.Counter(), []
    for name, eng in itertools.chain(planzoo.dry_engines(), more):
        for plan, tag in ((eng.fwd, 'fwd'), (eng.bwd, 'bwd')):
            for d, nm in zip(plan.descs, plan.names):
                kind = type(d).__name__
                per[kind] += 1
                if any(v % 16 for v in PR.desc_fields(d)[1].values()):
                    off16[kind] += 1
                if type(d) in L._DIRECT:
                    rc = call(d)
                else:
                    rc = L.lib.ga_plan_run(C.byref(L.make_op(d)), 1, None, None)
                if rc in REFUSED and len(fails) < 40:
                    fails.append(f'{name}.{tag}.{nm} ({kind}): {L.ERRORS[rc]}')
    print('\ndescriptors accepted per kind (with a pointer off 16 bytes): ' + ', '.join(f'{k} {v} ({off16[k]})' for k, v in sorted(per.items())))
    assert not fails, '\n'.join(fails)
    # the fused cells take the split-bf16 weights of a WeightStore on a device, which a dry-run engine does not have: no dry plan holds
    # one (their refusals are in the table above, their accepted geometries in tests/test_dec_cell_*gpu.py)
    assert set(per) == {o.cls.__name__ for o in L._H.ops} - {'DecCellDesc', 'DecCellHaloDesc'}, 'a kind of GA_OP_LIST no shipped plan uses'
