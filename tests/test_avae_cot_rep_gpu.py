"""
ga_avae backward with K = 3 cotangents per forward row (ga_avae_desc.act_rep): N counts cotangent rows, cotangent row n
reads the forward's tensors at row n / K.  Every case compares ONE launch with act_rep = 3
  1. bitwise (torch.equal) with three act_rep = 1 launches, one per cotangent slice (cotangent k of forward row r sits at row
     r * K + k, so slice k is rows k, K + k, ...), and
  2. with the float64 formulas of tests/opref.py, called once per cotangent, under the rule tests/test_ops_edges_gpu.py applies
     to the same op at act_rep = 1 (`near`: at most opref.bound() = 4 x the error of the same formula in plain fp32 on the CPU,
     gradient elements within 1e-6 of a LeakyReLU kink left out, at most 0.1 % of them).
Forward rows differ and so do the cotangents of a row: a wrong row index cannot pass.  Outputs start as NaN with a sentinel row
behind them (test_ops_edges_gpu.Out).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

import opref as R   # noqa: E402
from opref_cases import g, u   # noqa: E402
from gen_adversarial_amd import _lib as L   # noqa: E402
from test_ops_edges_gpu import DEV, SENT, Out, dev, f32, launch, near   # noqa: E402

K, NF = 3, 2            # cotangents per forward row, forward rows


def _slice(t, k):
    """cotangent k of every forward row: [NF * K, ...] -> [NF, ...]"""
    return t.view(NF, K, *t.shape[1:])[:, k].contiguous()


@pytest.mark.parametrize('noisy', [True, False])
@pytest.mark.parametrize('C_', [36, 8])
@pytest.mark.parametrize('P', [64, 35])
def test_adain_backward_act_rep(P, C_, noisy):
    """P = 35: a tail in the 32-lane pixel loop; C = 36: a full 32-channel chunk plus a 4-channel one (the `cok` guard); with the
    noise injection and without (a = b = NULL)."""
    x, style = g(NF, P, C_, seed=1), torch.cat([u(NF, C_, seed=4) + 0.5, g(NF, C_, seed=5)], dim=1)
    noise, wn = (g(NF, P, seed=2), g(C_, seed=3, scale=0.5)) if noisy else (None, None)
    dy = g(NF * K, P, C_, seed=6)
    fwd = dict(x=dev(x), a=dev(noise), b=dev(wn), c=dev(style), mode=L.GA_AVAE_ADAIN, P=P, C=C_)
    y, st = Out(NF, P, C_), Out(NF, C_, 2)
    launch(L.AvaeDesc, y=y, y2=st, N=NF, **fwd)
    y.done()
    stats = st.done().to(DEV)
    dx, dgb = Out(NF * K, P, C_), Out(NF * K, 2 * C_)
    launch(L.AvaeDesc, y=dx, y2=dgb, s=stats, dy=dev(dy), backward=1, N=NF * K, act_rep=K, **fwd)
    dx, dgb = dx.done(), dgb.done()
    a64, a32 = R.f64(x, noise, wn, style), f32(x, noise, wn, style)
    kink = R.near_kink(R.avae_adain_pre(*a64[:3]))
    for k in range(K):
        dx1, dgb1 = Out(NF, P, C_), Out(NF, 2 * C_)
        launch(L.AvaeDesc, y=dx1, y2=dgb1, s=stats, dy=dev(_slice(dy, k)), backward=1, N=NF, act_rep=1, **fwd)
        assert torch.equal(_slice(dx, k), dx1.done()), f'cotangent {k}: d x differs from the act_rep = 1 launch'
        assert torch.equal(_slice(dgb, k), dgb1.done()), f'cotangent {k}: (d gamma | d beta) differs from the act_rep = 1 launch'
        b64, b32 = R.avae_adain_bwd(*a64, R.f64(_slice(dy, k))), R.avae_adain_bwd(*a32, _slice(dy, k))
        near(f'adain dx, cotangent {k}', _slice(dx, k), b64[0], b32[0], skip=kink)
        near(f'adain dgamma | dbeta, cotangent {k}', _slice(dgb, k), b64[1], b32[1])


def test_pixelnorm_backward_act_rep():
    """2 forward rows x 3 cotangents, C = 64 (one wavefront per cotangent row, two workgroups)"""
    C_ = 64
    x, dy = g(NF, C_, seed=1), g(NF * K, C_, seed=2)
    dx = Out(NF * K, C_)
    launch(L.AvaeDesc, x=dev(x), dy=dev(dy), y=dx, mode=L.GA_AVAE_PIXELNORM, N=NF * K, C=C_, backward=1, act_rep=K)
    dx = dx.done()
    for k in range(K):
        dx1 = Out(NF, C_)
        launch(L.AvaeDesc, x=dev(x), dy=dev(_slice(dy, k)), y=dx1, mode=L.GA_AVAE_PIXELNORM, N=NF, C=C_, backward=1, act_rep=1)
        assert torch.equal(_slice(dx, k), dx1.done())
        near(f'pixelnorm backward, cotangent {k}', _slice(dx, k), R.pixelnorm_bwd(*R.f64(x, _slice(dy, k))), R.pixelnorm_bwd(x, _slice(dy, k)))


def test_sample_backward_act_rep():
    """2 x 3, P = 16, C = 8; eps is NCHW ([N, C, P]): the n / K row lands in the transposed layout.  The decisions read t itself:
    no element is left out."""
    P, C_, f0 = 16, 8, float(torch.tensor(0.7))
    t, eps, dz = g(NF, P, 2 * C_, seed=1), g(NF, C_, P, seed=2), g(NF * K, P, C_, seed=3)
    io = dict(x=dev(t), a=dev(eps), mode=L.GA_AVAE_SAMPLE, P=P, C=C_, f0=f0, backward=1)
    dt = Out(NF * K, P, 2 * C_)
    launch(L.AvaeDesc, dy=dev(dz), y=dt, N=NF * K, act_rep=K, **io)
    dt = dt.done()
    for k in range(K):
        dt1 = Out(NF, P, 2 * C_)
        launch(L.AvaeDesc, dy=dev(_slice(dz, k)), y=dt1, N=NF, act_rep=1, **io)
        assert torch.equal(_slice(dt, k), dt1.done())
        near(f'sample backward, cotangent {k}', _slice(dt, k), R.avae_sample_bwd(*R.f64(t, eps), f0, R.f64(_slice(dz, k))),
             R.avae_sample_bwd(t, eps, f0, _slice(dz, k)))


def test_avgpool_backward_ignores_act_rep():
    """the adjoint of the mean reads no forward tensor: act_rep = 3 is accepted and gives the bits of act_rep = 0"""
    N, H, W, C_, k = NF * K, 8, 12, 12, 2
    x, dy = g(NF, H, W, C_, seed=1), g(N, H // k, W // k, C_, seed=2)
    outs = []
    for rep in (0, K):
        dx = Out(N, H, W, C_)
        launch(L.AvaeDesc, x=dev(x), dy=dev(dy), y=dx, mode=L.GA_AVAE_AVGPOOL, N=N, H=H, W=W, C=C_, k=k, backward=1, act_rep=rep)
        outs.append(dx.done())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[1], R.avgpool_bwd(R.f64(dy), k).float())


@pytest.mark.parametrize('what', ['forward', 'ragged'])
def test_act_rep_refusals(what):
    """act_rep = 2 on a forward launch, and N = 5 cotangent rows with act_rep = 2: GA_E_BADARG, nothing launched (the output still
    holds its sentinel)"""
    C_ = 64
    x, dy = dev(g(5, C_, seed=1)), dev(g(5, C_, seed=2))
    y = torch.full((5, C_), SENT, device=DEV)
    d = L.AvaeDesc()
    d.x, d.dy, d.y, d.mode, d.C, d.act_rep = x.data_ptr(), dy.data_ptr(), y.data_ptr(), L.GA_AVAE_PIXELNORM, C_, 2
    d.N, d.backward = (4, 0) if what == 'forward' else (5, 1)
    assert L.lib.ga_avae(C.byref(d), 0) == -1                  # GA_E_BADARG
    with pytest.raises(L.GaError, match='GA_E_BADARG'):
        L.run(d)
    torch.cuda.synchronize()
    assert bool((y == SENT).all())
