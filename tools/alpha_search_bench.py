"""GPU tool: candidates per second of the alpha-learning objective, K candidates per engine pass (AlphaEvaluator.objective_many)
against a loop of objective_function over the same candidates and images — interleaved rounds in one process, like tools/conv_ab.py.

    python tools/alpha_search_bench.py [--configs vgg-11-full vgg-11 resnet-50 resnext-50] [--candidates 8] [--rounds 5]

The loop is the one-candidate path: for vgg-11 it is the code of the commits before objective_many existed (per_image_verdicts on the
forward-only engine, alphas patched into the sampler descriptors per candidate); for the two StyleGAN defenders no earlier path
exists, the loop of this tree's own one-candidate path is the only baseline.  Random weights: the accuracies mean nothing, the
arithmetic per row is that of the real checkpoints.  `vgg-11-full` is the full-size NVAE + VGG-11 of bench.py; the other three are
the reduced defenders of the test-suite (the full-size StyleGAN defenders do not fit a useful number of candidate rows).
"""
import argparse
import os
import sys
import tempfile
import time
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

DEV = 'cuda:0'


def nvae_files(d, full):
    from gen_adversarial_amd.nvae_spec import ASSUMED_NVAE_CONFIG, ASSUMED_NVAE_RESOLUTION, build_spec, nvae_checkpoint
    from gen_adversarial_amd.vgg_spec import init_vgg_state_dict
    cfg = dict(ASSUMED_NVAE_CONFIG) if full else {**ASSUMED_NVAE_CONFIG, 'initial_channels': 8, 'num_pre-post_process_blocks': 1,
                                                  'num_groups_per_scale': 2, 'num_cells_per_group': 1, 'num_latent_per_group': 4}
    torch.save(nvae_checkpoint(cfg, ASSUMED_NVAE_RESOLUTION, seed=5), os.path.join(d, 'ae.pt'))
    torch.save({'state_dict': init_vgg_state_dict(100, 1 if full else 16, seed=6)}, os.path.join(d, 'clf.pt'))
    return len(build_spec(cfg, ASSUMED_NVAE_RESOLUTION).groups), 64


def e4e_files(d):
    from gen_adversarial_amd.e4e_spec import build_e4e_spec, init_e4e_state_dict
    from gen_adversarial_amd.resnet_spec import init_resnet_state_dict
    from gen_adversarial_amd.stylegan_spec import build_stylegan_spec, init_stylegan_state_dict
    espec, esd = build_e4e_spec(64, 4, (1, 1, 1, 1)), init_e4e_state_dict(64, 4, 3, (1, 1, 1, 1))
    gspec = build_stylegan_spec(64, width_div=8, style_dim=espec.style_dim)
    gsd = init_stylegan_state_dict(gspec, 4)
    avg = 0.5 * torch.randn(gspec.n_latent, gspec.style_dim, generator=torch.Generator().manual_seed(6))
    ck = {'state_dict': {**{'encoder.' + k: v for k, v in esd.items()}, **{'decoder.' + k: v for k, v in gsd.items()}},
          'latent_avg': avg, 'opts': {'stylegan_size': gspec.size, 'start_from_latent_avg': True, 'encoder_type': 'Encoder4Editing'}}
    torch.save(ck, os.path.join(d, 'ae.pt'))
    torch.save({'state_dict': init_resnet_state_dict(2, 8, 5, (1, 1, 1, 1))}, os.path.join(d, 'clf.pt'))
    return gspec.n_latent, 64


def trans_files(d):
    from gen_adversarial_amd.resnet_spec import init_resnet_state_dict
    from gen_adversarial_amd.stylegan_spec import build_stylegan_spec, init_stylegan_state_dict
    from gen_adversarial_amd.trans_spec import build_trans_spec, init_trans_state_dict
    tspec, tsd = build_trans_spec(4, (1, 1, 1, 1)), init_trans_state_dict(4, 1, (1, 1, 1, 1))
    gspec = build_stylegan_spec(64, width_div=8, style_dim=tspec.d_model)
    gsd = init_stylegan_state_dict(gspec, 2)
    avg = 0.3 * torch.randn(16, tspec.d_model, generator=torch.Generator().manual_seed(4))
    ck = {'state_dict': {**{'encoder.module.' + k: v for k, v in tsd.items()}, **{'decoder.module.' + k: v for k, v in gsd.items()}},
          'latent_avg': avg, 'opts': {'output_size': gspec.size, 'input_nc': 3, 'start_from_latent_avg': True, 'learn_in_w': False}}
    torch.save(ck, os.path.join(d, 'ae.pt'))
    torch.save({'state_dict': init_resnet_state_dict(4, 2, 3, (1, 1, 1, 1), 4, 8)}, os.path.join(d, 'clf.pt'))
    return 16, 64


CONFIGS = {'vgg-11-full': ('vgg-11', lambda d: nvae_files(d, True)), 'vgg-11': ('vgg-11', lambda d: nvae_files(d, False)),
           'resnet-50': ('resnet-50', e4e_files), 'resnext-50': ('resnext-50', trans_files)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run(name, a):
    from gen_adversarial_amd.experiments.alpha_learning.common_utils import AlphaEvaluator
    ctype, files = CONFIGS[name]
    with tempfile.TemporaryDirectory() as d:
        n, res = files(d)
        args = Namespace(classifier_type=ctype, classifier_path=os.path.join(d, 'clf.pt'), autoencoder_path=os.path.join(d, 'ae.pt'),
                         initial_alphas=[0.] * n, eot_steps=a.eot)
        g = torch.Generator().manual_seed(0)
        images = torch.rand(a.images, 3, res, res, generator=g)
        ev = AlphaEvaluator(args, DEV, images=images, labels=torch.zeros(a.images, dtype=torch.long), batch_images=a.batch_images)
    cand = torch.rand(a.candidates, n, generator=g)
    cpp = a.candidates_per_pass or max(1, a.row_budget // (a.batch_images * a.eot))
    cpp = min(cpp, a.candidates)

    def loop():
        return [ev.objective_function(c) for c in cand]

    def many():
        return ev.objective_many(cand, candidates_per_pass=cpp)
    loop(), many()                                        # builds the engines of both paths
    t = np.array([[timed(loop), timed(many)] for _ in range(a.rounds)])
    cps = a.candidates / np.median(t, axis=0)
    rows_loop, rows_many = a.batch_images * a.eot, a.batch_images * cpp * a.eot
    print(f'{name}: K {a.candidates} candidates, {a.images} images, EoT {a.eot}; loop {rows_loop} rows/pass {cps[0]:8.2f} cand/s '
          f'(min {a.candidates / t[:, 0].max():.2f}, max {a.candidates / t[:, 0].min():.2f}); objective_many {cpp} cand/pass = '
          f'{rows_many} rows/pass {cps[1]:8.2f} cand/s (min {a.candidates / t[:, 1].max():.2f}, max {a.candidates / t[:, 1].min():.2f}); '
          f'ratio {cps[1] / cps[0]:.3f}', flush=True)


if __name__ == '__main__':
    p = argparse.ArgumentParser()
    p.add_argument('--configs', nargs='+', default=list(CONFIGS), choices=list(CONFIGS))
    p.add_argument('--candidates', type=int, default=8)
    p.add_argument('--candidates_per_pass', type=int, default=0, help='0: row_budget // (batch_images * eot)')
    p.add_argument('--row_budget', type=int, default=1024)
    p.add_argument('--images', type=int, default=8)
    p.add_argument('--batch_images', type=int, default=8)
    p.add_argument('--eot', type=int, default=32)
    p.add_argument('--rounds', type=int, default=5)
    a = p.parse_args()
    for name in a.configs:
        run(name, a)
