"""
Device milliseconds of ga_nes_perturb and ga_nes_grad at one NES step of one image (default 1 x 12288 x 512: a 64 x 64 image, 512
pairs = 1024 query rows), HIP events around each launch, medians reported.  With --forward, also the forward of the headline
defender (bench.py's build_model) at rows = 1024 x EoT, EoT from --eot: the call those 1024 queries cost.  No target: the figures
stand next to each other in DESIGN.md §0 as facts.

    python tools/nes_bench.py [--images 1] [--inner 12288] [--pairs 512] [--reps 30] [--forward] [--eot 1] [--time-limit 240]

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
    ap.add_argument('--images', type=int, default=1)
    ap.add_argument('--inner', type=int, default=12288)
    ap.add_argument('--pairs', type=int, default=512)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--forward', action='store_true')
    ap.add_argument('--eot', type=int, default=1)
    ap.add_argument('--time-limit', type=int, default=240)
    args = ap.parse_args()

    def too_long(*_):
        print(json.dumps({'error': f'time limit of {args.time_limit} s passed'}), flush=True)
        os._exit(3)
    signal.signal(signal.SIGALRM, too_long)
    signal.alarm(args.time_limit)

    import torch
    from gen_adversarial_amd import _lib as L
    from gen_adversarial_amd.noise import STREAM_NES

    dev = 'cuda:0'
    B, inner, pairs = args.images, args.inner, args.pairs
    x = torch.rand(B, inner, device=dev)
    y = torch.empty(B * pairs * 2, inner, device=dev)
    c = torch.randn(B * pairs, device=dev)
    g = torch.empty(B, inner, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def perturb():
        L.check(L.lib.ga_nes_perturb(x.data_ptr(), y.data_ptr(), B, inner, pairs, 7, 0, STREAM_NES, 0, None, 1e-3, 0.0, 1.0, stream), 'ga_nes_perturb')

    def grad():
        L.check(L.lib.ga_nes_grad(c.data_ptr(), g.data_ptr(), B, inner, pairs, 7, 0, STREAM_NES, 0, None, 1.0 / (2e-3 * pairs), stream), 'ga_nes_grad')

    for _ in range(3):
        timed(perturb), timed(grad)
    t_p, t_g = [timed(perturb) for _ in range(args.reps)], [timed(grad) for _ in range(args.reps)]
    out = {'images': B, 'inner': inner, 'pairs': pairs, 'reps': args.reps, 'query_rows': B * pairs * 2,
           'perturb_ms_median': statistics.median(t_p), 'perturb_ms_min': min(t_p), 'perturb_bytes_written': y.numel() * 4,
           'grad_ms_median': statistics.median(t_g), 'grad_ms_min': min(t_g),
           'how': 'HIP events around one launch each, warm, medians over --reps'}
    if args.forward:
        from bench import build_model
        rows = B * pairs * 2 * args.eot
        eng, _ = build_model(dev, rows, args.eot, seed=0)
        for _ in range(2):
            timed(eng.forward)
        t_f = [timed(eng.forward) for _ in range(5)]
        out.update({'forward_rows': rows, 'forward_eot': args.eot, 'forward_ms_median': statistics.median(t_f), 'forward_ms_min': min(t_f)})
    print(json.dumps(out), flush=True)
    signal.alarm(0)


if __name__ == '__main__':
    main()
