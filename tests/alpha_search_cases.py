"""
Reduced defenders, inputs, pinned draws and CPU-oracle logits of tests/test_alpha_search_gpu.py.  Importable without a GPU: the
oracle side (one defender call per candidate, as the reference would make it) runs on the CPU, so the top-2 margins the GPU test
relies on can be checked wherever the oracle runs.

Rows of a candidate-batched pass: image-major, then candidate, then EoT replica — row (b * K + k) * E + e.
"""
import os
from argparse import Namespace

import torch

B, K, E = 2, 3, 2            # images, candidates, EoT replicas

# seeds of (images, draws, third candidate) chosen so that every (image, candidate) top-2 margin of the oracle's EoT-mean logits is
# at least 10 x the logit tolerance of its defender (asserted by the GPU test before anything is compared)
SEEDS = {'vgg-11': 21, 'resnet-50': 21, 'resnext-50': 22}

NVAE_CFG = {'initial_channels': 8, 'num_pre-post_process_blocks': 1, 'num_pre-post_process_cells': 2, 'num_scales': 3,
            'num_groups_per_scale': 2, 'is_adaptive': False, 'min_groups_per_scale': 1, 'num_cells_per_group': 1,
            'num_latent_per_group': 4, 'num_logistic_mixtures': 10, 'num_nf_cells': None}


def candidate_rows(k: int):
    """rows of candidate k in a [B * K * E] pass, in the order a one-candidate call of the same images has them"""
    return [(b * K + k) * E + e for b in range(B) for e in range(E)]


class Case:
    """one defender: checkpoint files, evaluator arguments, images, K candidates, pinned draws for the B * K * E rows, the oracle"""

    def __init__(self, classifier_type, args, res, n, attenuation, draws, oracle, tol, seed):
        self.classifier_type, self.args, self.res, self.n, self.attenuation = classifier_type, args, res, n, attenuation
        self.draws, self._oracle, self.tol = draws, oracle, tol
        g = torch.Generator().manual_seed(seed)
        self.x = torch.rand(B, 3, res, res, generator=g)
        self.cand = torch.stack([torch.zeros(n), torch.ones(n), torch.rand(n, generator=g)])          # float32, [K, n]
        self._logits = None

    def engine_alphas(self, k: int):
        """candidate k as the defender stores it: `a * alpha_attenuation` in double (common_utils.py:88)"""
        return [a * self.attenuation for a in self.cand[k].tolist()]

    def draws_of(self, k: int):
        idx = candidate_rows(k)
        return [d[idx] for d in self.draws]

    def oracle_logits(self) -> torch.Tensor:
        """[K, B * E, classes]: one oracle defender call per candidate on x.repeat_interleave(E) with that candidate's draws"""
        if self._logits is None:
            with torch.no_grad():
                xr = self.x.repeat_interleave(E, dim=0)
                self._logits = torch.stack([self._oracle(xr, self.engine_alphas(k), self.draws_of(k)) for k in range(K)])
        return self._logits

    def oracle_mean_logits(self) -> torch.Tensor:
        """[K, B, classes] EoT means"""
        lg = self.oracle_logits()
        return lg.view(K, B, E, -1).mean(dim=2)

    def min_margin(self) -> float:
        top2 = self.oracle_mean_logits().topk(2, dim=2).values
        return (top2[..., 0] - top2[..., 1]).min().item()

    def labels(self) -> torch.Tensor:
        """image 0: what candidate 2 predicts for it; image 1: another class than candidate 2 predicts — the verdicts then differ
        between images (and, where the candidates disagree, between candidates)"""
        pred = self.oracle_mean_logits()[2].argmax(dim=1)
        lab = pred.clone()
        lab[1::2] = (lab[1::2] + 1) % self.oracle_mean_logits().shape[2]
        return lab

    def verdicts(self) -> torch.Tensor:
        """bool [K, B]"""
        return self.oracle_mean_logits().argmax(dim=2) == self.labels().view(1, -1)


def nvae_case(folder) -> Case:
    from gen_adversarial_amd.nvae_spec import build_spec, nvae_checkpoint
    from gen_adversarial_amd.vgg_spec import build_vgg_spec, init_vgg_state_dict
    from oracle import defender_oracle as D
    res = (3, 64, 64)
    ck = nvae_checkpoint(NVAE_CFG, res, seed=5)
    vsd = init_vgg_state_dict(100, 16, seed=6)
    torch.save(ck, os.path.join(folder, 'nvae.pt'))
    torch.save({'state_dict': vsd}, os.path.join(folder, 'vgg.pt'))
    spec, vspec, sd = build_spec(NVAE_CFG, res), build_vgg_spec(100, 16), ck['state_dict_temp=0.6']
    n = len(spec.groups)
    seed = SEEDS['vgg-11']
    g = torch.Generator().manual_seed(1000 + seed)
    draws = [torch.randn(B * K * E, 4, gs.res, gs.res, generator=g) for gs in spec.groups]
    args = Namespace(classifier_type='vgg-11', classifier_path=os.path.join(folder, 'vgg.pt'), autoencoder_path=os.path.join(folder, 'nvae.pt'),
                     initial_alphas=[0.] * n, eot_steps=E)

    def oracle(xr, alphas, eps):        # a draw of input noise is made even at eps 0 (abstract_models.py:132)
        return D.nvae_defender(sd, spec, vsd, vspec, xr, alphas, eps, torch.ones_like(xr), 0.0)[0]
    # tests/test_api_gpu.py:73 — EoT logits of this defender against the oracle: < 2e-4 absolute
    return Case('vgg-11', args, 64, n, 0.7, draws, oracle, lambda ref: 2e-4, seed)


def e4e_case(folder) -> Case:
    from oracle import defender_oracle as D
    from test_host_cpu import _small_e4e_defense
    _, (esd, espec, gsd, gspec, avg, csd, cspec, _) = _small_e4e_defense(dry_run=True, device='cpu')
    ck = {'state_dict': {**{'encoder.' + k: v for k, v in esd.items()}, **{'decoder.' + k: v for k, v in gsd.items()}},
          'latent_avg': avg, 'opts': {'stylegan_size': gspec.size, 'start_from_latent_avg': True, 'encoder_type': 'Encoder4Editing'}}
    torch.save(ck, os.path.join(folder, 'e4e.pt'))
    torch.save({'state_dict': csd}, os.path.join(folder, 'resnet.pt'))
    n = gspec.n_latent
    seed = SEEDS['resnet-50']
    g = torch.Generator().manual_seed(1000 + seed)
    draws = [torch.randn(B * K * E, n, gspec.style_dim, generator=g)]
    args = Namespace(classifier_type='resnet-50', classifier_path=os.path.join(folder, 'resnet.pt'),
                     autoencoder_path=os.path.join(folder, 'e4e.pt'), initial_alphas=[0.] * n, eot_steps=E)

    def oracle(xr, alphas, eps):
        return D.e4e_defender_call(esd, espec, gsd, gspec, avg, csd, cspec, xr, alphas, eps[0], 64)[0]
    # tests/test_e4e_defense_gpu.py:69 — logits of this defender (bf16x3) against the oracle: < 1e-3 * max(1, max |logits|)
    return Case('resnet-50', args, 64, n, 1.0, draws, oracle, lambda ref: 1e-3 * max(1.0, ref.abs().max().item()), seed)


def trans_case(folder) -> Case:
    from gen_adversarial_amd.resnet_spec import build_resnet_spec, init_resnet_state_dict
    from gen_adversarial_amd.stylegan_spec import build_stylegan_spec, init_stylegan_state_dict
    from gen_adversarial_amd.trans_spec import build_trans_spec, init_trans_state_dict
    from oracle import defender_oracle as D, trans_oracle as T
    # the reduced Style-Transformer defender of tests/test_trans_gpu.py (_small_case): quarter-width encoder, 64-px generator, ResNeXt
    tspec, tsd = build_trans_spec(4, (1, 1, 1, 1)), init_trans_state_dict(4, 1, (1, 1, 1, 1))
    gspec = build_stylegan_spec(64, width_div=8, style_dim=tspec.d_model)
    gsd = init_stylegan_state_dict(gspec, 2)
    cspec, csd = build_resnet_spec(4, 2, (1, 1, 1, 1), 4, 8), init_resnet_state_dict(4, 2, 3, (1, 1, 1, 1), 4, 8)
    avg = 0.3 * torch.randn(16, tspec.d_model, generator=torch.Generator().manual_seed(4))
    ck = {'state_dict': {**{'encoder.module.' + k: v for k, v in tsd.items()}, **{'decoder.module.' + k: v for k, v in gsd.items()}},
          'latent_avg': avg, 'opts': {'output_size': gspec.size, 'input_nc': 3, 'start_from_latent_avg': True, 'learn_in_w': False}}
    torch.save(ck, os.path.join(folder, 'trans.pt'))
    torch.save({'state_dict': csd}, os.path.join(folder, 'resnext.pt'))
    res, n = 64, 16
    seed = SEEDS['resnext-50']
    g = torch.Generator().manual_seed(1000 + seed)
    draws = [0.8 * torch.randn(B * K * E, n, tspec.d_model, generator=g)]            # the defender draws N(0, 0.8) (models.py:331)
    args = Namespace(classifier_type='resnext-50', classifier_path=os.path.join(folder, 'resnext.pt'),
                     autoencoder_path=os.path.join(folder, 'trans.pt'), initial_alphas=[0.] * n, eot_steps=E)

    def oracle(xr, alphas, eps):
        p = T.trans_purify(tsd, tspec, gsd, gspec, avg, xr, alphas, eps[0], out_size=res, mid=2 * res, crop=res // 4, pool_to=2 * res)
        return D.resnet_classifier_call(csd, cspec, p)
    # tests/test_trans_gpu.py:347 (close(), :34-37) — EoT logits of this defender against the oracle: < 1e-3 * max(1, max |logits|)
    return Case('resnext-50', args, res, n, 0.7, draws, oracle, lambda ref: 1e-3 * max(1.0, ref.abs().max().item()), seed)


CASES = {'vgg-11': nvae_case, 'resnet-50': e4e_case, 'resnext-50': trans_case}
