"""
Tile code 12 of ga_conv2d (csrc/conv_pw_frag.hip): the 1x1 convolution with its weight fragments read straight from global memory
(ga_conv_desc.w_frag in the one-tap order of WeightStore.frag3(w, taps=1)) and the activation chunk staged once per workgroup.

Every case runs 256 pixels (two 128-pixel tiles) as 16 images of 4 x 4, with 64 input channels (one shallow chunk) or 192 (a full
128-channel chunk and a 64-channel tail) and 128 or 256 output channels (one or two weight tiles), is held against the float64
interpreter of tests/convref.py with the bound of tests/test_plan_convs_gpu.py for split-bf16 convs (tau_bf3), and must equal
the library's default tile on the same descriptor BIT FOR BIT: the kernel keeps conv_bf3's summation order (chunk-major, k
ascending, lo*hi, hi*lo, hi*hi).
"""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convref as R                                                      # noqa: E402
from gen_adversarial_amd import _lib as L                                # noqa: E402
from gen_adversarial_amd.engine_core import WeightStore, pw_ok            # noqa: E402

DEV = 'cuda:0'
N, H, W = 16, 4, 4
GUARD = 256


def _run(cin, cout, tile, *, frag_copy=True, pro='none', dact=False, dact_rep=1, addend=False, addend2=False, addend_rep=1, w=None, seed=0,
         N=N, H=H, W=W, splits=1, c2=0):
    """-> (y [N, H, W, cout] with its guard region, the descriptor, the operand tensors for conv_ref); raises L.GaError"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g, device=DEV) * scale       # noqa: E731
    t = {'x': rn(N, H, W, cin)}
    t['w'] = rn(cout, cin + c2, scale=1 / math.sqrt(cin + c2)) if w is None else w.contiguous()
    t['bias'] = rn(cout, scale=0.5)
    d = L.ConvDesc()
    d.N, d.Hi, d.Wi, d.Ho, d.Wo, d.C1, d.Cout = N, H, W, H, W, cin, cout
    d.KH = d.KW = d.sn = d.sd = 1
    d.ldx, d.ldy, d.tile, d.splits = cin, cout, tile, splits
    if c2:
        t['x2'] = rn(N, H, W, c2)
        d.C2 = d.ldx2 = c2
    if splits > 1:
        t['ws'] = torch.empty(splits * N * H * W * cout, device=DEV)
        d.ws_floats = t['ws'].numel()
    if pro == 'per_row':
        t['pro_scale'] = torch.rand(N, cin, generator=g, device=DEV) + 0.5
        t['pro_shift'] = rn(N, cin, scale=0.5)
        d.pro_per_row = 1
    elif pro == 'bn_silu':
        t['pro_scale'] = torch.rand(cin, generator=g, device=DEV) + 0.5
        t['pro_shift'] = rn(cin, scale=0.5)
        d.pro_act = L.GA_ACT_SILU
    if dact:
        t['dact_x'] = rn(N // dact_rep, H, W, cout)
        d.lddact, d.dact_act, d.dact_rep = cout, L.GA_ACT_SILU, dact_rep
    if addend:
        t['addend'] = rn(N // addend_rep, H, W, cout)
        d.ldadd, d.addend_rep = cout, addend_rep
    if addend2:
        t['addend2'] = rn(N, H, W, cout)
        d.ldadd2 = cout
    for k, v in t.items():
        setattr(d, k, v.data_ptr())
    store = WeightStore(DEV)
    hi, lo = store.split(t['w'])
    # (a refused channel count has no fragment order: the request then carries the copy of the weights padded to the next k step)
    frag = store.frag3(t['w'] if (cin + c2) % 16 == 0 else torch.nn.functional.pad(t['w'], (0, -(cin + c2) % 16)), taps=1)
    d.w_hi, d.w_lo = hi.data_ptr(), lo.data_ptr()
    if tile == 12 and frag_copy:
        d.w_frag = frag.data_ptr()
    y = torch.full((N * H * W * cout + GUARD,), float('nan'), device=DEV)
    d.y = y.data_ptr()
    try:
        L.run(d, torch.cuda.current_stream().cuda_stream)
    except L.GaError as ex:             # a refused request launches nothing
        torch.cuda.synchronize()
        ex.desc, ex.untouched, ex.keep = d, bool(torch.isnan(y).all()), (t, hi, lo, frag)
        raise
    torch.cuda.synchronize()
    return y, d, t, (hi, lo, frag)


def _check(cin, cout, **kw):
    y, d, t, keep = _run(cin, cout, 12, **kw)
    assert pw_ok(d), 'engine_core.pw_ok rejects a descriptor the library takes'
    assert torch.isnan(y[N * H * W * cout:]).all(), 'wrote past the last pixel'
    out = y[:N * H * W * cout].view(N, H, W, cout)
    ref, scale, slack = R.conv_ref(d, t)
    r, e = R.bound_ratio(out, ref, scale, slack, R.TAU_BF3)
    print(f'  {cin} -> {cout} {kw}: max|err|/scale {e:.2e} = {e / R.TAU_BF3:.3f} tau_bf3, bound ratio {r:.3f}', flush=True)
    assert r <= 1.0, (r, e)
    y0, _, _, _ = _run(cin, cout, 0, **kw)
    assert torch.equal(y.view(torch.int32), y0.view(torch.int32)), 'not bitwise equal to the default tile'


@pytest.mark.parametrize('pro', ['none', 'per_row', 'bn_silu'])
@pytest.mark.parametrize('cout', [128, 256])
@pytest.mark.parametrize('cin', [64, 192])
def test_prologues_and_chunking(cin, cout, pro):
    _check(cin, cout, pro=pro, seed=cin + cout)


def test_act_grad_epilogue():
    _check(192, 128, dact=True, seed=1)


def test_two_addends():
    _check(192, 256, addend=True, addend2=True, seed=2)


def test_eot_shared_addend():
    _check(64, 128, addend=True, addend_rep=2, seed=3)


def test_act_rep_2():
    """two cotangent rows per saved activation row: output row n reads the act' input of row n / 2"""
    _check(64, 256, pro='per_row', dact=True, dact_rep=2, seed=4)


def test_transposed_weight_copy():
    """a ^T launch: the weights are the transposed copy [Cin][Cout] of a forward 192 -> 128 layer, stored in the same fragment order"""
    g = torch.Generator(device=DEV).manual_seed(5)
    w_fwd = torch.randn(128, 192, generator=g, device=DEV) / math.sqrt(192)
    _check(128, 192, w=w_fwd.t().contiguous(), addend=True, seed=5)


def test_weights_gathered_without_fragment_copy():
    """a caller that has no fragment copy (w_frag null: tests/test_plan_convs_gpu.py rebuilds the shipped descriptors that way)
    gets the same fragments gathered from w_hi / w_lo: same bits; 48 channels: the zero-padded half group on both paths"""
    _check(192, 256, pro='bn_silu', frag_copy=False, seed=6)
    _check(48, 128, frag_copy=False, seed=7)
    _check(48, 128, seed=7)


def test_refuses_40_channels():
    """a channel count that is no multiple of the MFMA k step: GA_E_UNSUPPORTED, nothing launched"""
    with pytest.raises(L.GaError, match='UNSUPPORTED'):
        _run(40, 128, 12)


@pytest.mark.parametrize('kw', [dict(N=15), dict(splits=2), dict(pro='per_row', N=128, H=3, W=3), dict(c2=64)],
                         ids=['240_pixels', 'split_k', 'per_row_3x3_images', 'two_sources'])
def test_refused_exactly_where_the_predicate_says_no(kw):
    """the other direction of _check's `accepted => pw_ok`: descriptors one step outside tile 12's domain — pixels that are no
    whole 128-pixel tiles, split-K, a per-row prologue on images of Ho * Wo % 16 != 0 pixels (1152 pixels: whole tiles), a second
    source — are refused by the library, nothing written, and pw_ok says no"""
    with pytest.raises(L.GaError, match='UNSUPPORTED') as ex:
        _run(64, 128, 12, **kw)
    assert ex.value.untouched, 'refused but wrote the output'
    assert not pw_ok(ex.value.desc)
