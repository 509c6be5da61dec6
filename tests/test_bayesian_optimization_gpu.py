"""
GPU: the Bayesian optimisation of the alphas on real (reduced) defenders — 4 steps, 2 candidates per round, two images, EoT 2:
  1. the search runs as candidate-batched engine passes: forward_candidates once with the 5 initial vectors, twice with 2 proposals,
     and never the one-candidate path (forward_rows, which __call__ and the EoT wrapper go through);
  2. every stored accuracy is a mean over the two images;
  3. the two files have 5 + 4 rows;
  4. the alphas lie in [0,1] and the engine was handed the stored ones times the defender's attenuation;
  5. the same seed and the same observed accuracies give the same first round (replayed into the surrogate, no engine).
Reduced defenders and inputs: tests/alpha_search_cases.py.  Logit values are the business of tests/test_alpha_search_gpu.py.
"""
import contextlib
import io
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

from alpha_search_cases import B, CASES, E   # noqa: E402

DEV = 'cuda:0'
TYPES = ['vgg-11', 'resnet-50']
STEPS, Q, SEED = 4, 2, 0


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from gen_adversarial_amd.experiments.alpha_learning import bayesian_optimization as BO
    from gen_adversarial_amd.experiments.alpha_learning.common_utils import AlphaEvaluator
    done = {}

    def get(classifier_type):
        if classifier_type in done:
            return done[classifier_type]
        tag = classifier_type.replace('-', '_')
        c = CASES[classifier_type](str(tmp_path_factory.mktemp('bo_' + tag)))
        ev = AlphaEvaluator(c.args, DEV, images=c.x, labels=c.labels(), batch_images=B)
        model = ev.defense_model.model
        model.image_size = c.res
        assert ev.eot_steps == E and len(model.interpolation_alphas) == c.n
        many, rows, handed, single = model.forward_candidates, model.forward_rows, [], []

        def spy_many(batch, alphas, rep=1, preds_only=True):
            handed.append((torch.as_tensor(alphas).detach().cpu().clone(), batch.shape[0], rep))
            return many(batch, alphas, rep=rep, preds_only=preds_only)

        def spy_rows(*a, **kw):
            single.append(1)
            return rows(*a, **kw)
        folder = str(tmp_path_factory.mktemp('bo_out_' + tag))
        model.forward_candidates, model.forward_rows = spy_many, spy_rows           # instance attributes over the class's methods
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                BO.main(Namespace(n_optimization_steps=STEPS, candidates_per_round=Q, seed=SEED, results_folder=folder), evaluator=ev)
        finally:
            del model.forward_candidates, model.forward_rows
        assert model.forward_candidates.__func__ is type(model).forward_candidates
        c.handed, c.single = handed, single
        c.alphas, c.acc = np.load(f'{folder}/alphas.npy'), np.load(f'{folder}/accuracies.npy')
        done[classifier_type] = c
        return c
    return get


@pytest.mark.parametrize('classifier_type', TYPES)
def test_the_search_runs_as_candidate_batched_engine_passes(runs, classifier_type):
    c = runs(classifier_type)
    assert [(tuple(a.shape), b, rep) for a, b, rep in c.handed] == [((5, c.n), B, E), ((Q, c.n), B, E), ((Q, c.n), B, E)]
    assert c.single == []


@pytest.mark.parametrize('classifier_type', TYPES)
def test_files_hold_the_initial_points_and_the_proposals(runs, classifier_type):
    from gen_adversarial_amd.experiments.alpha_learning.bayesian_optimization import initial_alphas
    c = runs(classifier_type)
    assert c.alphas.shape == (5 + STEPS, c.n) and c.acc.shape == (5 + STEPS, 1) and c.alphas.dtype == c.acc.dtype == np.float32
    assert np.isin(c.acc, [0.0, 0.5, 1.0]).all()
    assert (c.alphas >= 0.0).all() and (c.alphas <= 1.0).all()
    assert np.array_equal(c.alphas[:5], initial_alphas(c.n).numpy())
    handed = torch.cat([a for a, _, _ in c.handed])
    assert handed.dtype == torch.float64 and torch.equal(handed, torch.from_numpy(c.alphas).double() * c.attenuation)


@pytest.mark.parametrize('classifier_type', TYPES)
def test_the_same_seed_and_observations_propose_the_same_first_round(runs, classifier_type):
    from gen_adversarial_amd.experiments.alpha_learning.bayesian_optimization import propose_round
    c = runs(classifier_type)
    x, y = torch.from_numpy(c.alphas[:5]), 1.0 - c.acc[:5, 0].astype(np.float64)
    first = propose_round(x, y, Q, SEED, 0)
    assert first.dtype == torch.float32 and np.array_equal(first.numpy(), c.alphas[5:5 + Q])
    assert torch.equal(first, propose_round(x, y, Q, SEED, 0))
