"""
Milliseconds of `_EngineOwner._fill_noise` on the NVAE engine of the headline workload (bench.py's build_model: 1024 rows, EoT 32),
with torch's draws (normal_ per latent group, + norm and division where input noise is configured) and with ga_randn
(`seeded_noise`): the two arms interleaved in one process, HIP events around each call, medians reported.  No target: noise is
a small share of a step; the pair goes into DESIGN.md §4.

    python tools/noise_bench.py [--rows 1024] [--eot 32] [--reps 30] [--time-limit 240]

Prints one JSON line.  The run ends itself (exit 3) when it passes --time-limit seconds.
"""
import argparse
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1024)
    ap.add_argument('--eot', type=int, default=32)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--time-limit', type=int, default=240)
    args = ap.parse_args()

    def too_long(*_):
        print(json.dumps({'error': f'time limit of {args.time_limit} s passed'}), flush=True)
        os._exit(3)
    signal.signal(signal.SIGALRM, too_long)
    signal.alarm(args.time_limit)

    import torch
    from bench import build_model
    from gen_adversarial_amd.defenses.ours.abstract_models import _EngineOwner

    eng, _ = build_model('cuda:0', args.rows, args.eot, seed=0)
    owner = _EngineOwner()
    owner._fixed_noise = None

    def timed(seed):
        owner.seeded_noise(seed)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        owner._fill_noise(eng)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(3):                                   # warm-up of both arms (first launches, torch's generator set-up)
        timed(None), timed(7)
    t_torch, t_randn = [], []
    for _ in range(args.reps):
        t_torch.append(timed(None))
        t_randn.append(timed(7))
    floats = sum(e.numel() for e in eng.eps) + (eng.noise.numel() if eng.noise is not None else 0)
    print(json.dumps({'rows': args.rows, 'eot': args.eot, 'reps': args.reps, 'tensors': len(eng.eps) + (eng.noise is not None),
                      'floats_drawn': floats, 'input_noise': eng.noise is not None,
                      'torch_ms_median': statistics.median(t_torch), 'torch_ms_min': min(t_torch),
                      'ga_randn_ms_median': statistics.median(t_randn), 'ga_randn_ms_min': min(t_randn),
                      'how': 'HIP events around one _fill_noise call (launches + host time between them), arms interleaved'}), flush=True)
    signal.alarm(0)


if __name__ == '__main__':
    main()
