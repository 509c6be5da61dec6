"""GPU tool: milliseconds for the class gradients DeepFool and FAB ask of the bare gender and cars classifiers — the full-size
ResNet-50 at 256 x 256 with 2 classes and the ResNeXt-50 32x4d at 128 x 128 with 4 — through the K-cotangent backward plan and
through the per-class loop (`jacobian_cot_rows = 0`: one autograd backward per class), interleaved rounds in one process like
tools/class_jacobian_competitors.py.

    python tools/class_jacobian_resnet.py [--models gender cars] [--rounds 9] [--out FILE]

One image, no EoT (the `no_defense_gender` / `no_defense_cars` protocol), random weights (the arithmetic per row is that of the
real checkpoints).  Prints one JSON line: per classifier the median milliseconds of both paths (forward included: each is what
`ClassJacobian(...).grads()` costs an attack), their spread and their ratio.
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

DEV = 'cuda:0'
MODELS = {'gender': dict(cls='CelebaGenderClassifier', n_classes=2, res=256, init=(2, 1, 6)),
          'cars': dict(cls='CarsTypeClassifier', n_classes=4, res=128, init=(4, 1, 6, (3, 4, 6, 3), 32, 4))}


def build(name, d):
    from gen_adversarial_amd.defenses.ours import models
    from gen_adversarial_amd.resnet_spec import init_resnet_state_dict
    m = MODELS[name]
    path = os.path.join(d, f'{name}.pt')
    torch.save({'state_dict': init_resnet_state_dict(*m['init'])}, path)
    return getattr(models, m['cls'])(path, DEV)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run(name, a):
    from gen_adversarial_amd.attacks.l2_attacks import ClassJacobian
    with tempfile.TemporaryDirectory() as d:
        clf = build(name, d)
    m, owner = MODELS[name], type(clf)
    x = torch.rand(1, 3, m['res'], m['res'], generator=torch.Generator().manual_seed(0)).to(DEV)
    budget = owner.jacobian_cot_rows

    def plan():
        j = ClassJacobian(clf, x)
        assert j._fast is not None and j._fast.eng.cot_rep == m['n_classes']
        return j.grads()

    def loop():
        owner.jacobian_cot_rows = 0
        try:
            j = ClassJacobian(clf, x)
            assert j._fast is None
            return j.grads()
        finally:
            owner.jacobian_cot_rows = budget
    for _ in range(a.warmup):                                  # builds the engines of both paths
        gp, gl = plan(), loop()
    scale = gl.abs().amax(dim=(2, 3, 4), keepdim=True).clamp_min(1e-30)
    err = ((gp - gl).abs() / scale).max().item()
    t = np.array([[timed(plan), timed(loop)] for _ in range(a.rounds)])
    med = np.median(t, axis=0)
    out = {'classes': m['n_classes'], 'resolution': m['res'], 'K': m['n_classes'], 'replays': 1,
           'plan_ms': round(float(med[0]), 2), 'loop_ms': round(float(med[1]), 2),
           'plan_ms_min_max': [round(float(t[:, 0].min()), 2), round(float(t[:, 0].max()), 2)],
           'loop_ms_min_max': [round(float(t[:, 1].min()), 2), round(float(t[:, 1].max()), 2)],
           'ratio': round(float(med[1] / med[0]), 2), 'max_rel_diff': float(f'{err:.2e}')}
    print(f'# {name}: {m["n_classes"]} class gradients at {m["res"]} px, K = {m["n_classes"]}: plan {med[0]:.2f} ms, per-class loop '
          f'{med[1]:.2f} ms, ratio {med[1] / med[0]:.2f}, plan vs loop {err:.1e} of each column\'s max', file=sys.stderr, flush=True)
    del clf
    torch.cuda.empty_cache()
    return out


if __name__ == '__main__':
    p = argparse.ArgumentParser()
    p.add_argument('--models', nargs='+', default=list(MODELS), choices=list(MODELS))
    p.add_argument('--rounds', type=int, default=9)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = p.parse_args()
    if a.rounds < 5:
        p.error('at least 5 rounds')
    res = {'tool': 'class_jacobian_resnet', 'images': 1, 'eot': 1, 'rounds': a.rounds,
           'device': torch.cuda.get_device_name(0), 'classifiers': {n: run(n, a) for n in a.models}}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
