"""GPU tool: autotune (tile, split-K) of every conv shape of the bench engine; writes the table under gpurun_out/."""
# usage: python tools/tune.py [rows] [out.json] [fresh | retune <tile>] [share]
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench import build_model
from gen_adversarial_amd.engine_core import tune_cache

R = int(sys.argv[1]) if len(sys.argv) > 1 else 256
out = sys.argv[2] if len(sys.argv) > 2 else 'gpurun_out/conv_tune_gfx950.json'
share = 'share' in sys.argv[4:]
eng, _ = build_model('cuda:0', R, int(os.environ.get('GA_TUNE_REP', '32')), share_encoder=share)
eng.x_in.uniform_()
for e in eng.eps: e.normal_()
eng.forward(); eng.dlogits.normal_(); eng.backward(); torch.cuda.synchronize()
s = eng.stream()
f0, fc0, _ = eng.fwd.time(s, iters=3, per_conv=True); b0, bc0, _ = eng.bwd.time(s, iters=3, per_conv=True)
print(f'before: fwd {f0:.2f} (conv {fc0:.2f})  bwd {b0:.2f} (conv {bc0:.2f})', flush=True)
fresh = len(sys.argv) > 3 and sys.argv[3] == 'fresh'
start = {} if fresh else None
old = None
if len(sys.argv) > 3 and sys.argv[3] == 'retune':          # `retune <tile>`: a new (or changed) tile code: time the shapes it is a candidate for again
    new_tile = int(sys.argv[4])
    start = dict(tune_cache())
    old = {k: start.pop(k, None) for k in eng.candidate_keys(new_tile)}
cache = eng.autotune(cache=start, reps=5, save=out, verbose=True)     # default: add missing shapes
if old is not None:         # a shape changes its entry only where the new tile won: the other tiles were compared before
    for k, v in old.items():
        print(f'retune {new_tile} {k}: {v} -> {cache[k]}' + ('' if cache[k][0] == new_tile else ' (kept)'), flush=True)
        if cache[k][0] != new_tile:
            if v is not None:
                cache[k] = v
            else:
                del cache[k]
    eng.apply_tuning(cache)
    with open(out, 'w') as f:
        json.dump(cache, f, indent=0, sort_keys=True)
f1, fc1, _ = eng.fwd.time(s, iters=3, per_conv=True); b1, bc1, _ = eng.bwd.time(s, iters=3, per_conv=True)
print(f'after : fwd {f1:.2f} (conv {fc1:.2f})  bwd {b1:.2f} (conv {bc1:.2f})  entries {len(cache)}')
