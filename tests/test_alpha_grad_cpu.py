"""
No GPU: the alpha-gradient plans and the descent script.
  1. dry-run plans of the three reduced defenders of tests/alpha_search_cases.py: Engine(alpha_grad=True) adds one reduction op per
     latent group (NVAE: ga_sampler_desc.mode == 2) or one for all latent indices (e4e, Style-Transformer:
     ga_latent_mix_desc.backward == 2) to the backward plan, beside the op whose cotangent it reads, and nothing else;
  2. alpha_grad=True is refused with cot_rep > 1 and with need_backward=False;
  3. gradient_descent.main on a stub evaluator: projected Adam on a quadratic whose minimiser lies partly outside the box;
  4. AlphaEvaluator.loss_and_gradient = attenuation x the defender's gradient, mean over the set.
"""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from alpha_search_cases import NVAE_CFG
from gen_adversarial_amd import _lib as L
from gen_adversarial_amd.engine import Engine

ROWS, REP = 4, 2


def _nvae(**kw):
    from gen_adversarial_amd.nvae_spec import build_spec, nvae_checkpoint
    from gen_adversarial_amd.vgg_spec import build_vgg_spec, init_vgg_state_dict
    res = (3, 64, 64)
    sd = nvae_checkpoint(NVAE_CFG, res, seed=5)['state_dict_temp=0.6']
    n = len(build_spec(NVAE_CFG, res).groups)
    kw.setdefault('share_encoder', True)
    return Engine(sd, NVAE_CFG, res, init_vgg_state_dict(100, 16, seed=6), build_vgg_spec(100, 16), rows=ROWS, rep=REP,
                  alphas=[0.1 * i for i in range(n)], device='cpu', dry_run=True, **kw), n


def _e4e(**kw):
    from test_host_cpu import _small_e4e_defense
    _, (esd, espec, gsd, gspec, avg, csd, cspec, alphas) = _small_e4e_defense(dry_run=True, device='cpu')
    eng = Engine.bare(ROWS, device='cpu', dry_run=True, rep=REP, resolution=(3, 64, 64), alphas=alphas, share_encoder=True, **kw)
    return eng.build_e4e_defense(esd, espec, gsd, gspec, avg, csd, cspec, pool_to=64), gspec.n_latent


def _trans(**kw):
    from gen_adversarial_amd.resnet_spec import build_resnet_spec, init_resnet_state_dict
    from gen_adversarial_amd.stylegan_spec import build_stylegan_spec, init_stylegan_state_dict
    from gen_adversarial_amd.trans_spec import build_trans_spec, init_trans_state_dict
    tspec, tsd = build_trans_spec(4, (1, 1, 1, 1)), init_trans_state_dict(4, 1, (1, 1, 1, 1))
    gspec = build_stylegan_spec(64, width_div=8, style_dim=tspec.d_model)
    gsd = init_stylegan_state_dict(gspec, 2)
    cspec, csd = build_resnet_spec(4, 2, (1, 1, 1, 1), 4, 8), init_resnet_state_dict(4, 2, 3, (1, 1, 1, 1), 4, 8)
    eng = Engine.bare(ROWS, device='cpu', dry_run=True, rep=REP, resolution=(3, 64, 64), alphas=[0.1] * 16, share_encoder=True, **kw)
    return eng.build_trans_defense(tsd, tspec, gsd, gspec, torch.zeros(16, tspec.d_model), csd, cspec, pool_to=64, mid=128, crop=16), 16


BUILDERS = {'vgg-11': _nvae, 'resnet-50': _e4e, 'resnext-50': _trans}


@pytest.mark.parametrize('classifier_type', ['vgg-11', 'resnet-50', 'resnext-50'])
def test_alpha_grad_adds_its_reductions_to_the_backward_plan_and_nothing_else(classifier_type):
    build = BUILDERS[classifier_type]
    plain, n = build()
    grad, _ = build(alpha_grad=True)
    assert plain.alpha_grad_rows is None and tuple(grad.alpha_grad_rows.shape) == (ROWS, n)
    assert grad.alpha_grads() is grad.alpha_grad_rows
    with pytest.raises(RuntimeError):
        plain.alpha_grads()
    # forward plan: the same ops
    assert grad.fwd.names == plain.fwd.names
    assert [type(d) for d in grad.fwd.descs] == [type(d) for d in plain.fwd.descs]
    # backward plan: the new ops, each directly behind the op whose cotangent it shares; without them the plan of today
    new = [i for i, nm in enumerate(grad.bwd.names) if nm.endswith('.dalpha')]
    rest = [i for i in range(len(grad.bwd)) if i not in new]
    assert [grad.bwd.names[i] for i in rest] == plain.bwd.names
    assert [type(grad.bwd.descs[i]) for i in rest] == [type(d) for d in plain.bwd.descs]
    assert len(grad.bwd) - len(plain.bwd) == len(new) == (n if classifier_type == 'vgg-11' else 1)
    for i in new:
        d, prev = grad.bwd.descs[i], grad.bwd.descs[i - 1]
        assert grad.bwd.names[i] == grad.bwd.names[i - 1] + '.dalpha' and type(prev) is type(d)
        if classifier_type == 'vgg-11':
            assert isinstance(d, L.SamplerDesc) and d.mode == 2 and d.backward == 1 and prev.mode == 0 and prev.backward == 1
            assert (d.dz, d.mu_q, d.p, d.eps, d.q_rep, d.N, d.ldz) == (prev.dz, prev.mu_q, prev.p, prev.eps, prev.q_rep, prev.N, prev.ldz)
            assert d.z == grad.alpha_grad_rows.data_ptr() and d.alpha_ld == n and d.act_rep <= 1 and not d.alpha_rows
        else:
            assert isinstance(d, L.LatentMixDesc) and d.backward == 2 and prev.backward == 1
            assert d.dout == prev.dout and d.out == grad.alpha_grad_rows.data_ptr() and (d.R, d.J, d.rep) == (ROWS, n, REP)
    if classifier_type == 'vgg-11':
        assert sorted(grad.bwd.descs[i].alpha_col for i in new) == list(range(n))         # every column once
        first = [grad.bwd.descs[i] for i in new if grad.bwd.descs[i].alpha_col == 0][0]
        assert first.q_rep == REP and not first.p                                          # the shared encoder's group, prior N(0, 1)
        # the new descriptors hold no alpha: set_alphas has nothing to patch in them
        assert not any(d.mode == 2 for d, _ in grad._sampler_descs)
        assert len(grad._sampler_descs) == len(plain._sampler_descs)


def test_alpha_grad_is_refused_without_a_backward_plan_and_with_several_cotangents():
    for kw in ({'cot_rep': 2}, {'need_backward': False}):
        with pytest.raises(ValueError, match='alpha_grad'):
            _nvae(alpha_grad=True, **kw)
        with pytest.raises(ValueError, match='alpha_grad'):
            Engine.bare(ROWS, device='cpu', dry_run=True, rep=REP, resolution=(3, 64, 64), alphas=[0.1] * 16, alpha_grad=True, **kw)


class _QuadraticEvaluator:
    """loss(a) = sum (a - target)^2 with three coordinates of the minimiser outside [0, 1]; accuracy = 1 / (1 + loss)"""
    target = np.array([-0.5, 1.5, 0.3, 0.8, 2.0, 0.55])

    def __init__(self):
        self.defense_model = Namespace(model=Namespace(interpolation_alphas=[0.0] * len(self.target)))
        self.seen = []

    def loss_and_gradient(self, alphas):
        a = np.asarray(alphas, dtype=np.float64)
        self.seen.append(a)
        return float(((a - self.target) ** 2).sum()), 2.0 * (a - self.target)

    def objective_function(self, alphas):
        return 1.0 / (1.0 + self.loss_and_gradient(alphas)[0])


def test_gradient_descent_on_a_quadratic_with_an_outside_minimiser(tmp_path):
    from gen_adversarial_amd.experiments.alpha_learning import gradient_descent as G
    from gen_adversarial_amd.experiments.alpha_learning.common_utils import get_best_combination
    args = G.parse_args(['--adv_images_path', 'unused', '--classifier_path', 'unused', '--classifier_type', 'vgg-11',
                         '--autoencoder_path', 'unused', '--autoencoder_name', 'stub', '--results_folder', str(tmp_path),
                         '--steps', '300', '--lr', '0.05', '--init', 'linear', '--eval_every', '50'])
    assert args.results_folder.rstrip('/').endswith(os.path.join('stub_vgg-11', 'gradient_descent'))
    ev = _QuadraticEvaluator()
    alphas, acc, losses = G.main(args, ev)
    assert all(((0.0 <= a) & (a <= 1.0)).all() for a in ev.seen)                      # every iterate inside the box
    assert alphas.shape == (7, 6) and acc.shape == (7, 1) and losses.shape == (7, 1)  # steps 0, 50, ..., 300
    assert losses[-1, 0] < losses[0, 0]
    t = ev.target
    outside = (t < 0) | (t > 1)
    assert np.array_equal(alphas[-1][outside], np.clip(t, 0, 1)[outside].astype(np.float32))      # on the boundary, exactly
    assert np.abs(alphas[-1][~outside] - t[~outside]).max() < 1e-2
    folder = args.results_folder
    for name, want in (('alphas', alphas), ('accuracies', acc), ('losses', losses)):
        got = np.load(f'{folder}/{name}.npy')
        assert got.dtype == np.float32 and np.array_equal(got, want)
    best = get_best_combination(folder)
    assert any(np.array_equal(best, row) for row in alphas) and np.array_equal(best, alphas[acc[:, 0].argmax()])
    # another start: the stored best of that run; zeros; a folder of the wrong width is refused
    assert np.array_equal(G.initial_vector(f'best_of:{folder}', 6).numpy(), best.astype(np.float64))
    assert G.initial_vector('zeros', 3).tolist() == [0.0] * 3 and len(G.initial_vector('cosine', 5)) == 5
    with pytest.raises(ValueError):
        G.initial_vector(f'best_of:{folder}', 5)
    with pytest.raises(ValueError):
        G.initial_vector('nonsense', 5)


def test_shim_reexports_the_script():
    import src.experiments.alpha_learning.gradient_descent as shim
    from gen_adversarial_amd.experiments.alpha_learning import gradient_descent as G
    assert shim.main is G.main and shim.parse_args is G.parse_args


def test_loss_and_gradient_is_the_attenuated_mean_of_the_defenders():
    """5 images in chunks of 2: the stub defender returns per-image loss = label + sum(stored alphas) and gradient rows label * w; the
    evaluator must hand it the attenuated alphas and return (mean loss, attenuation x mean gradient)"""
    from gen_adversarial_amd.experiments.alpha_learning.common_utils import AlphaEvaluator
    w = torch.tensor([1.0, -2.0, 0.5])

    class Stub:
        def __init__(self):
            self.model = Namespace(interpolation_alphas=[0.0] * 3)
            self.calls = []

        def loss_and_alpha_grad(self, x, y):
            self.calls.append((x.shape[0], list(self.model.interpolation_alphas)))
            return y.float() + sum(self.model.interpolation_alphas), y.float().view(-1, 1) * w.view(1, -1)

    ev = AlphaEvaluator.__new__(AlphaEvaluator)
    ev.defense_model, ev.alpha_attenuation, ev.batch_images = Stub(), 0.7, 2
    ev.images, ev.labels = torch.zeros(5, 3, 4, 4), torch.tensor([0, 1, 2, 3, 4])
    a = [0.2, 0.4, 1.0]
    loss, grad = ev.loss_and_gradient(a)
    stored = [v * 0.7 for v in a]
    assert [c[0] for c in ev.defense_model.calls] == [2, 2, 1] and all(c[1] == stored for c in ev.defense_model.calls)
    assert isinstance(loss, float) and abs(loss - (2.0 + sum(stored))) < 1e-6
    assert isinstance(grad, np.ndarray) and grad.shape == (3,)
    assert np.allclose(grad, 0.7 * 2.0 * w.double().numpy(), rtol=0, atol=1e-12)
