"""GPU tool: milliseconds for the class gradients DeepFool (10 classes) and FAB (all 100) ask of the ids experiment's competitor and
ablation defenders — ND-VAE, A-VAE, noise, blur in front of the VGG-11 — through the K-cotangent backward plan and through the
per-class loop (`jacobian_cot_rows = 0`: one autograd backward per class), interleaved rounds in one process like tools/conv_ab.py.

    python tools/class_jacobian_competitors.py [--defenders ndvae avae noise blur] [--eot 32] [--rounds 5] [--out FILE]

Sizes are those of configs/competitor_ndvae_ids.yaml, competitor_avae_ids.yaml and ablation_{noise,blur}_ids.yaml with random
weights (the arithmetic per row is that of the real checkpoints), one image x EoT 32 like the reference's protocol.  Prints one
JSON line: per defender and column count the median milliseconds of both paths (forward included: each is what
`ClassJacobian(...).grads()` costs an attack) and their ratio; a defender whose engines do not fit the device is recorded as such.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import yaml

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {'ndvae': ('competitor_ndvae_ids.yaml', 'ND-VAE'), 'avae': ('competitor_avae_ids.yaml', 'A-VAE'),
           'noise': ('ablation_noise_ids.yaml', 'ablation'), 'blur': ('ablation_blur_ids.yaml', 'ablation')}


def build(name, d, eot):
    """the defender behind load(args), from the shipped yaml with random full-size weights written to d"""
    from gen_adversarial_amd.avae_spec import init_avae_state_dict
    from gen_adversarial_amd.experiments.load_defense import load
    from gen_adversarial_amd.ndvae_spec import init_ndvae_state_dict
    from gen_adversarial_amd.vgg_spec import init_vgg_state_dict
    fname, dtype = CONFIGS[name]
    with open(os.path.join(ROOT, 'configs', fname)) as f:
        y = yaml.safe_load(f)
    torch.save({'state_dict': init_vgg_state_dict(100, 1, seed=6)}, os.path.join(d, 'clf.pt'))
    y['classifier_path'] = os.path.join(d, 'clf.pt')
    if name == 'ndvae':
        cfg = {k: y[k] for k in ('x_channels', 'encoding_channels', 'pre_proc_groups', 'scales', 'groups', 'cells')}
        torch.save(init_ndvae_state_dict(dict(cfg, input_dim=64), 5), os.path.join(d, 'ae.pt'))
    elif name == 'avae':
        torch.save(init_avae_state_dict(64, 5), os.path.join(d, 'ae.pt'))
    if 'autoencoder_path' in y:
        y['autoencoder_path'] = os.path.join(d, 'ae.pt')
    with open(os.path.join(d, 'cfg.yaml'), 'w') as f:
        yaml.safe_dump(y, f)
    return load(Namespace(config=os.path.join(d, 'cfg.yaml'), experiment='ids', defense_type=dtype, eot_steps=eot, device=DEV))[1]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run(name, a):
    from gen_adversarial_amd.attacks.l2_attacks import ClassJacobian
    with tempfile.TemporaryDirectory() as d:
        model = build(name, d, a.eot)
    owner = type(model.model)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(1, 3, 64, 64, generator=g).to(DEV)
    out = {}
    for n_cols in a.columns:
        cols = None if n_cols == 100 else torch.randperm(100, generator=g)[:n_cols].view(1, -1).to(DEV)
        budget = owner.jacobian_cot_rows

        def plan():
            j = ClassJacobian(model, x, cols)
            assert j._fast is not None
            return j.grads()

        def loop():
            owner.jacobian_cot_rows = 0
            try:
                j = ClassJacobian(model, x, cols)
                assert j._fast is None
                return j.grads()
            finally:
                owner.jacobian_cot_rows = budget
        try:
            for _ in range(a.warmup):                          # builds the engines of both paths
                plan(), loop()
            t = np.array([[timed(plan), timed(loop)] for _ in range(a.rounds)])
        except torch.cuda.OutOfMemoryError:
            out[str(n_cols)] = 'out of memory'
            break
        med = np.median(t, axis=0)
        K = min(n_cols, max(1, budget // a.eot))
        out[str(n_cols)] = {'K': K, 'replays': -(-n_cols // K), 'plan_ms': round(float(med[0]), 2), 'loop_ms': round(float(med[1]), 2),
                            'plan_ms_min_max': [round(float(t[:, 0].min()), 2), round(float(t[:, 0].max()), 2)],
                            'loop_ms_min_max': [round(float(t[:, 1].min()), 2), round(float(t[:, 1].max()), 2)],
                            'ratio': round(float(med[1] / med[0]), 2)}
        print(f'# {name}: {n_cols} class gradients, K = {K}: plan {med[0]:.1f} ms, per-class loop {med[1]:.1f} ms, '
              f'ratio {med[1] / med[0]:.2f}', file=sys.stderr, flush=True)
    del model
    torch.cuda.empty_cache()
    return out


if __name__ == '__main__':
    p = argparse.ArgumentParser()
    p.add_argument('--defenders', nargs='+', default=list(CONFIGS), choices=list(CONFIGS))
    p.add_argument('--columns', nargs='+', type=int, default=[10, 100])
    p.add_argument('--eot', type=int, default=32)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = p.parse_args()
    if a.rounds < 5:
        p.error('at least 5 rounds')
    res = {'tool': 'class_jacobian_competitors', 'images': 1, 'eot': a.eot, 'rounds': a.rounds,
           'device': torch.cuda.get_device_name(0), 'defenders': {n: run(n, a) for n in a.defenders}}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
