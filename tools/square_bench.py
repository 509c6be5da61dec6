"""
Device milliseconds of one Square Attack proposal launch (default 64 images x 3 x 64 x 64) for Linf and for L2, beside the same
proposal written as the per-image torch loop on the device (the authors' structure: per image its own window slices) and, with
--forward, one forward of the headline defender (bench.py's build_model) on those rows.  HIP events around each call, the
variants interleaved round by round in one process, medians reported.  No target: the figures stand next to each other in
DESIGN.md §0 as facts.

    python tools/square_bench.py [--images 64] [--size 64] [--side 21] [--rounds 30] [--forward] [--eot 1] [--time-limit 240]

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
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--side', type=int, default=21)
    ap.add_argument('--rounds', type=int, default=30)
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
    from gen_adversarial_amd.attacks import square as A
    from gen_adversarial_amd.attacks import square_ref as R
    from gen_adversarial_amd.attacks.nes import _first_rows_device

    dev = 'cuda:0'
    B, S, s, eps = args.images, args.size, args.side, 0.5
    x = torch.rand(B, 3, S, S, device=dev)
    d = torch.rand(B, 3, S, S, device=dev) - 0.5
    xa = x + d * (0.9 * eps / d.flatten(1).norm(dim=1).view(-1, 1, 1, 1))
    rows = _first_rows_device(list(range(B)), dev)
    table = torch.from_numpy(R.eta(s)).to(dev)
    win = R.windows(B, S, S, s, 7, 0)
    pos = [tuple(int(win[k][b]) for k in ('h1', 'w1', 'h2', 'w2')) for b in range(B)]
    sign = torch.tensor([[1.0 if (int(win['signs'][b]) >> ch) & 1 else -1.0 for ch in range(3)] for b in range(B)], device=dev).view(B, 3, 1, 1)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def hip_linf():
        A.propose('Linf', x, xa, s, 7, 0, rows, 0.05)

    def hip_l2():
        A.propose('L2', x, xa, s, 7, 0, rows, eps, table)

    def loop_linf():
        y = xa.clone()
        for b, (h, w, _, _) in enumerate(pos):
            y[b, :, h:h + s, w:w + s] = (x[b, :, h:h + s, w:w + s] + 0.05 * sign[b]).clamp(0.0, 1.0)
        return y

    def loop_l2():
        dl = xa - x
        n_img = dl.flatten(1).norm(dim=1)
        for b, (h, w, h2, w2) in enumerate(pos):
            mask = torch.zeros(S, S, dtype=torch.bool, device=dev)
            mask[h:h + s, w:w + s] = True
            mask[h2:h2 + s, w2:w2 + s] = True
            n_win = (dl[b] * mask).flatten(1).norm(dim=1)
            d1 = dl[b, :, h:h + s, w:w + s]
            new = sign[b] * (table.t() if win['transposed'][b] else table) + d1 / (1e-12 + d1.norm())
            target = ((eps * eps - n_img[b] ** 2).clamp_min(0.0) / 3 + n_win ** 2).sqrt()
            new = new * (target / (1e-12 + new.flatten(1).norm(dim=1))).view(3, 1, 1)
            dl[b, :, h2:h2 + s, w2:w2 + s] = 0.0
            dl[b, :, h:h + s, w:w + s] = new
        return (x + dl * (eps / (1e-12 + dl.flatten(1).norm(dim=1))).view(-1, 1, 1, 1)).clamp(0.0, 1.0)

    variants = {'hip_linf': hip_linf, 'hip_l2': hip_l2, 'torch_loop_linf': loop_linf, 'torch_loop_l2': loop_l2}
    if args.forward:
        from bench import build_model
        eng, _ = build_model(dev, B * args.eot, args.eot, seed=0)
        variants['forward'] = eng.forward
    for fn in variants.values():
        for _ in range(3):
            timed(fn)
    times = {k: [] for k in variants}
    for _ in range(args.rounds):                      # interleaved: every variant sees the same clocks and the same neighbours
        for k, fn in variants.items():
            times[k].append(timed(fn))
    out = {'images': B, 'shape': [3, S, S], 'side': s, 'rounds': args.rounds,
           'how': 'HIP events around one call each, warm, variants interleaved round by round, medians'}
    for k, t in times.items():
        out[f'{k}_ms_median'], out[f'{k}_ms_min'] = statistics.median(t), min(t)
    if args.forward:
        out['forward_rows'], out['forward_eot'] = B * args.eot, args.eot
    err = (A.propose('L2', x, xa, s, 7, 0, rows, eps, table) - loop_l2()).abs().max().item()
    out['hip_l2_vs_torch_loop_max_abs'] = err
    print(json.dumps(out), flush=True)
    signal.alarm(0)


if __name__ == '__main__':
    main()
