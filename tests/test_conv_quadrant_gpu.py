"""The quadrant tile (ga_conv_desc.tile = 9, csrc/conv_quad3.hip): 3x3 / stride 1 / pad 1 on 4 x 4 images, a workgroup = one 2 x 2
quadrant of 32 images, the products with the zero padding left out.

Every case runs tile 9 and tile 8 on the same descriptor and the same w_frag and compares the float tensors with torch.equal
(the skipped products are exact zeros: -0.0 == +0.0 is the only licence), on random inputs and on an input whose image-border
pixels are 1e30 — a product that crossed a quadrant or an image border wrongly is then a gross error, not rounding.  The random
case is also held to the float64 reference and the split-bf16 bound of tests/convref.py, as tile 8 is in test_plan_convs_gpu.py.
"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

import convref as R  # noqa: E402
from gen_adversarial_amd import _lib as L  # noqa: E402
from gen_adversarial_amd.engine_core import WeightStore, conv_key, quad_ok, resolve_tile, tune_cache  # noqa: E402

DEV = 'cuda:0'
FORMS = ('fwd', 'conv2T', 'conv1T')
UNSUPPORTED = {v: k for k, v in L.ERRORS.items()}['GA_E_UNSUPPORTED']


def _case(N, Cin, Cout, form, border=False, H=4, seed=0):
    """(descriptor without tile / y, tensors for conv_ref, keep-alive list)"""
    g = torch.Generator(device=DEV).manual_seed(seed)

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, device=DEV, generator=g) * scale
    x = rn(N, H, H, Cin)
    if border:
        edge = torch.ones(H, H, dtype=torch.bool, device=DEV)
        edge[1:-1, 1:-1] = False
        x[:, edge] = 1e30
    w = rn(Cout, 9 * Cin, scale=(9 * Cin) ** -0.5)
    store = WeightStore(DEV)
    hi, lo = store.split(w)
    frag = store.frag3(w)
    t = {'x': x, 'w': w}
    d = L.ConvDesc()
    d.N, d.Hi, d.Wi, d.Ho, d.Wo, d.C1, d.Cout, d.KH, d.KW, d.sn, d.sd, d.pad = N, H, H, H, H, Cin, Cout, 3, 3, 1, 1, 1
    d.ldx, d.ldy, d.splits = Cin, Cout, 1
    d.x, d.w, d.w_hi, d.w_lo, d.w_frag = x.data_ptr(), w.data_ptr(), hi.data_ptr(), lo.data_ptr(), frag.data_ptr()
    if form in ('silu', 'relu'):        # a bare activation prologue (no affine): the VGG layers, the encoder's first conv of a cell
        t.update(bias=rn(Cout, scale=0.1))
        d.pro_act = R.GA_ACT_SILU if form == 'silu' else R.GA_ACT_RELU
    elif form == 'fwd':                 # BN affine + SiLU prologue, bias
        t.update(pro_scale=torch.rand(Cin, device=DEV, generator=g) + 0.5, pro_shift=rn(Cin, scale=0.3), bias=rn(Cout, scale=0.1))
        d.pro_act = R.GA_ACT_SILU
    elif form == 'conv2T':              # per-row affine prologue, act' of a saved input
        t.update(pro_scale=torch.rand(N, Cin, device=DEV, generator=g) + 0.5, pro_shift=rn(N, Cin, scale=0.3), dact_x=rn(N, H, H, Cout))
        d.pro_per_row, d.dact_act, d.lddact = 1, R.GA_ACT_SILU, Cout
    else:                               # act' with scale / shift, plus the primary addend
        t.update(dact_x=rn(N, H, H, Cout), dact_scale=torch.rand(Cout, device=DEV, generator=g) + 0.5, dact_shift=rn(Cout, scale=0.3),
                 addend=rn(N, H, H, Cout))
        d.dact_act, d.lddact, d.ldadd = R.GA_ACT_SILU, Cout, Cout
    for k in ('pro_scale', 'pro_shift', 'bias', 'dact_x', 'dact_scale', 'dact_shift', 'addend'):
        if k in t:
            setattr(d, k, t[k].data_ptr())
    return d, t, [hi, lo, frag, store]


def _run(d, tile, splits=1):
    """(error code, output) of a copy of d on `tile`; the output is NaN where the launch wrote nothing"""
    c = L.ConvDesc.from_buffer_copy(d)
    y = torch.full((d.N, d.Ho, d.Wo, d.Cout), float('nan'), device=DEV)
    c.y, c.tile, c.splits = y.data_ptr(), tile, splits
    ws = None
    if splits > 1:
        ws = torch.empty(splits * y.numel(), device=DEV)
        c.ws, c.ws_floats = ws.data_ptr(), ws.numel()
    rc = L.lib.ga_conv2d(C.byref(c), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, y


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('Cout', [128, 256])
@pytest.mark.parametrize('Cin', [32, 96])
@pytest.mark.parametrize('N', [32, 96])
def test_quadrant_tile_equals_tile8_and_meets_the_float64_bound(N, Cin, Cout, form):
    d, t, _keep = _case(N, Cin, Cout, form, seed=N + Cin + Cout)
    assert quad_ok(d, 1)
    rc8, y8 = _run(d, 8)
    rc9, y9 = _run(d, 9)
    assert rc8 == 0 and rc9 == 0, (rc8, rc9)
    ref, scale, slack = R.conv_ref(d, t)
    r9, e9 = R.bound_ratio(y9, ref, scale, slack, R.TAU_BF3)
    r8, e8 = R.bound_ratio(y8, ref, scale, slack, R.TAU_BF3)
    print(f'N{N} {Cin}->{Cout} {form}: tile 9 bound ratio {r9:.3f} ({e9 / R.TAU_BF3:.3f} tau), tile 8 {r8:.3f}; '
          f'max |y9 - y8| {(y9 - y8).abs().max().item():.2e}', flush=True)
    assert torch.equal(y9, y8)
    assert r9 <= 1.0, (r9, e9)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('Cout', [128, 256])
@pytest.mark.parametrize('Cin', [32, 96])
@pytest.mark.parametrize('N', [32, 96])
def test_quadrant_tile_keeps_products_inside_quadrant_and_image(N, Cin, Cout, form):
    """image-border pixels of 1e30: a tap taken from the wrong pixel, quadrant or image moves the result by ~1e29"""
    d, t, _keep = _case(N, Cin, Cout, form, border=True, seed=1 + N + Cin + Cout)
    rc8, y8 = _run(d, 8)
    rc9, y9 = _run(d, 9)
    assert rc8 == 0 and rc9 == 0, (rc8, rc9)
    assert torch.isfinite(y8).all()
    assert torch.equal(y9, y8), (y9 - y8).abs().max().item()


@pytest.mark.parametrize('form', ['silu', 'relu'])
def test_quadrant_tile_bare_activation_prologue(form):
    """activation without an affine: neither kernel has a select between the activation's multiply and the split's subtraction"""
    for border in (False, True):
        d, t, _keep = _case(32, 96, 128, form, border=border, seed=11)
        rc8, y8 = _run(d, 8)
        rc9, y9 = _run(d, 9)
        assert rc8 == 0 and rc9 == 0, (rc8, rc9)
        assert torch.equal(y9, y8), (border, (y9 - y8).abs().max().item())
        if not border:
            r9, e9 = R.bound_ratio(y9, *R.conv_ref(d, t), R.TAU_BF3)
            assert r9 <= 1.0, (r9, e9)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('N', [8, 16])
def test_quadrant_tile_partial_group(N, form):
    """fewer than 32 images: one partial group — the missing images load zeros past the input's extent, their rows are dropped by
    the epilogue and nothing is written past the last pixel (the plan tests replay shipped descriptors at 8 rows)"""
    for border in (False, True):
        d, t, _keep = _case(N, 96, 256, form, border=border, seed=13 + N)
        assert quad_ok(d, 1)
        rc8, y8 = _run(d, 8)
        c = L.ConvDesc.from_buffer_copy(d)
        buf = torch.full((y8.numel() + 4096,), float('nan'), device=DEV)
        c.y, c.tile = buf.data_ptr(), 9
        assert L.lib.ga_conv2d(C.byref(c), torch.cuda.current_stream().cuda_stream) == 0 and rc8 == 0
        torch.cuda.synchronize()
        y9 = buf[:y8.numel()].view_as(y8)
        assert torch.isnan(buf[y8.numel():]).all(), 'wrote past the last pixel'
        assert torch.equal(y9, y8), (border, (y9 - y8).abs().max().item())
        if not border:
            r9, e9 = R.bound_ratio(y9, *R.conv_ref(d, t), R.TAU_BF3)
            assert r9 <= 1.0, (r9, e9)


def test_quadrant_tile_split_k_over_chunks():
    """three chunks over two and three K slices: the slices are summed by the reduce kernel in tile 8's order"""
    d, t, _keep = _case(32, 96, 128, 'conv1T', seed=5)
    for splits in (2, 3):
        rc8, y8 = _run(d, 8, splits)
        rc9, y9 = _run(d, 9, splits)
        assert rc8 == 0 and rc9 == 0, (splits, rc8, rc9)
        assert torch.equal(y9, y8), splits


@pytest.mark.parametrize('why', ['N40', 'H8', 'no_frag'])
def test_quadrant_tile_refusals_fall_back_to_tile8_values(why):
    """what the predicate rejects the library refuses (GA_E_UNSUPPORTED, nothing written); resolve_tile then demotes the request
    and the result is tile 8's"""
    d, t, keep = _case(40 if why == 'N40' else 32, 32, 128, 'fwd', H=8 if why == 'H8' else 4, seed=9)
    frag = d.w_frag
    rc8, y8 = _run(d, 8)
    assert rc8 == 0
    if why == 'no_frag':
        d.w_frag = None
    assert not quad_ok(d, 1)
    rc9, y9 = _run(d, 9)
    assert rc9 == UNSUPPORTED, rc9
    assert torch.isnan(y9).all()

    def can_frag(tile):                 # the engine's _want: no fragment copy in the no_frag case
        if why == 'no_frag':
            return False
        d.w_frag = frag
        return True
    tile, splits = resolve_tile(d, 9, 1, can_frag)
    assert tile == (5 if why == 'no_frag' else 8) and splits == 1, (tile, splits)
    rc, y = _run(d, tile, splits)
    assert rc == 0
    assert torch.equal(y, y8)


def test_quadrant_tile_in_a_32_row_nvae_plan():
    """the 32-row NVAE engine with tile 9 forced on every eligible conv against the same engine with tile 8 forced"""
    from bench import build_model
    eng = build_model(DEV, 32, 32, seed=0, precision='bf16x3')[0]
    g = torch.Generator(device=DEV).manual_seed(3)
    eng.x_in.copy_(torch.rand(eng.x_in.shape, device=DEV, generator=g))
    for e in eng.eps:
        e.copy_(torch.randn(e.shape, device=DEV, generator=g))
    cot = torch.randn(eng.dlogits.shape, device=DEV, generator=g)
    keys = eng.candidate_keys(9)
    assert keys, 'no conv of the plan is a candidate for tile 9'

    def run(tile):
        cache = dict(tune_cache())
        cache.update({k: [tile, 1, 1] for k in keys})
        eng.apply_tuning(cache)
        n = sum(1 for d in eng._conv_descs() if d.tile == tile and conv_key(d) in keys)
        eng.forward()
        eng.dlogits.copy_(cot)
        eng.backward()
        torch.cuda.synchronize()
        return n, eng.purified.clone(), eng.logits.clone(), eng.dx.clone()
    n8, p8, l8, g8 = run(8)
    n9, p9, l9, g9 = run(9)
    eligible = sum(1 for d in eng._conv_descs() if conv_key(d) in keys)
    print(f'{n9} of {eligible} eligible convs of the 32-row plan on tile 9 ({n8} on tile 8), {len(keys)} distinct shapes', flush=True)
    assert n9 == eligible > 0           # no silent demotion
    assert 0 < n8 <= n9                 # (tile 8 refuses the per-row prologue at 512 channels — its LDS table — and runs those on tile 5: same values)
    assert torch.isfinite(g8).all()
    assert torch.equal(p9, p8) and torch.equal(l9, l8) and torch.equal(g9, g8)
