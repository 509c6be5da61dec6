"""
ga_dwconv5's two collapsed forms against tests/opref.py in float64: the up2 forward (four 3x3 parity filters on the source
image; SiLU prologue, bias) and the pool2 backward (one 6x6 stride-2 filter on dy; flipped taps, SiLU' of dact_x).  Inputs
and tolerance are test_ops_gpu.test_dwconv5's: unit-normal inputs, taps of scale 0.2, 1e-5 absolute.  Shapes are (N, H, W, C)
at full resolution:
  (5, 2, 2, 4)     1x1 source: every tap is border
  (9, 4, 4, 36)    N not a multiple of the images per workgroup, C not a multiple of 32
  (3, 6, 10, 12)   non-square, odd source dims, partial window in both directions
  (2, 40, 24, 8)   several windows in H, partial in W, C < 32
  (2, 16, 48, 40)  three full pool2 windows in W, two channel blocks with the second partial
  (2, 8, 8, 100)   the 8 x 8 whole-image-window geometry
Every launch runs twice and the two outputs must be bitwise equal; the row behind each output must keep its sentinel.
The up2 forward keeps the 25 products of every output and their order, so it must also equal, bit for bit, the plain windowed
form run on the replicated image (not at 4 x 4, where the plain form is the border-skipping 4 x 4 kernel with another order).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

import opref as R   # noqa: E402
from gen_adversarial_amd import _lib as L   # noqa: E402
from test_ops_edges_gpu import Out, dev, launch   # noqa: E402
from test_ops_gpu import g   # noqa: E402

TOL = 1e-5
SHAPES = [(5, 2, 2, 4), (9, 4, 4, 36), (3, 6, 10, 12), (2, 40, 24, 8), (2, 16, 48, 40), (2, 8, 8, 100)]


def run_twice(shape, **kw):
    outs = []
    for _ in range(2):
        y = Out(*shape)
        launch(L.DwDesc, y=y, **kw)
        outs.append(y.done())
    assert torch.isfinite(outs[0]).all(), 'not every output element was written'
    assert torch.equal(outs[0], outs[1]), 'two launches on the same inputs differ'
    return outs[0]


@pytest.mark.parametrize('N,H,W,C', SHAPES)
def test_up2_forward(N, H, W, C):
    x, w, b = g(N, H // 2, W // 2, C, seed=1), g(25, C, seed=2, scale=0.2), g(C, seed=3)
    out = run_twice((N, H, W, C), x=dev(x), w=dev(w), bias=dev(b), N=N, H=H, W=W, C=C, pro_act=L.GA_ACT_SILU, up2=1)
    ref = R.dwconv5(*R.f64(x, w, b), pro_act=R.SILU, up2=True)
    err = R.max_err(out, ref)
    print(f'up2 forward {(N, H, W, C)}: kernel err {err:.3e}')
    assert err <= TOL


@pytest.mark.parametrize('N,H,W,C', [sh for sh in SHAPES if sh[1:3] != (4, 4)])
def test_up2_forward_is_bitwise_the_literal_form(N, H, W, C):
    x, w, b = g(N, H // 2, W // 2, C, seed=1), g(25, C, seed=2, scale=0.2), g(C, seed=3)
    kw = dict(w=dev(w), bias=dev(b), N=N, H=H, W=W, C=C, pro_act=L.GA_ACT_SILU)
    out = run_twice((N, H, W, C), x=dev(x), up2=1, **kw)
    lit = run_twice((N, H, W, C), x=dev(R.up2_nearest(x)), **kw)
    assert torch.equal(out, lit), f'{int((out != lit).sum())} elements differ, max {(out - lit).abs().max().item():.3e}'


def pool2_backward(N, H, W, C, K):
    cot, w, u = g(N, H, W, C, seed=4), g(25, C, seed=2, scale=0.2), g(N // K, H // 2, W // 2, C, seed=1)
    wf = w.view(5, 5, C).flip(0, 1).reshape(25, C)
    out = run_twice((N, H // 2, W // 2, C), x=dev(cot), w=dev(wf), dact_x=dev(u), N=N, H=H, W=W, C=C,
                    dact_act=L.GA_ACT_SILU, pool2=1, act_rep=K)
    ref = R.dwconv5(*R.f64(cot, wf), dact_x=R.f64(u), dact_act=R.SILU, pool2=True, act_rep=K)
    err = R.max_err(out, ref)
    print(f'pool2 backward {(N, H, W, C)}, act_rep {K}: kernel err {err:.3e}')
    assert err <= TOL


@pytest.mark.parametrize('N,H,W,C', SHAPES)
def test_pool2_backward(N, H, W, C):
    pool2_backward(N, H, W, C, 1)


def test_pool2_backward_three_cotangents_per_row():
    """act_rep = 3: 6 cotangent rows on a dact_x of 2 rows"""
    pool2_backward(6, 6, 10, 12, 3)
