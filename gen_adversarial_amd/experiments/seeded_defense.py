"""
The evaluation driver (experiments/test_defense.py: same flags, same sharding, gather and results.json) with the defender's noise
drawn on the device from the counter-based generator (ga_randn, `seeded_noise`):

    python -m gen_adversarial_amd.experiments.seeded_defense --noise_seed S <the flags of experiments.test_defense>

Before an image is evaluated the defender's draw counter is set to 0 and its first row to (index of the image in the dataset) x
EoT, so the draws an image sees depend on S and on its place in the dataset — not on the number of ranks, and not on --schedule.
With --batch_images B > 1 the clean pass and the batched attacks (PGD) take B images per call; every image of the batch still
draws at its own rows (one ga_randn per image), so the static r::W shards, whose batches hold images that are W apart, see the same
draws as any other partition — as long as the attack keeps all images of the batch in its calls (an attack that drops finished
images from a call shifts the others' rows).  The reference's one-image attacks then run image by image, each from draw 0.
The draw number of a call counts the calls since the restart, so results are comparable between runs with the same --batch_images.
Everything else — the torch seeds of the attacks' own starting points included — is test_defense's, except for NES (--attack nes):
its directions and its starting point come from the same generator at rows (index of the image in the dataset) x pairs
(`NESAttack.image_index`), so an image's queries are the same in every partition; the defender's own draws under its query calls
count rows from the batch's first image.  Square Attack (--attack square) likewise: its windows, signs and starting point are drawn
at row (index of the image in the dataset) (`SquareAttack.image_index`).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from datetime import timedelta
from typing import Callable, Dict, Tuple

import torch
import torch.distributed as dist

from . import test_defense as drv


OWN_ATTACKS = ('nes', 'square')                       # --attack choices of this driver beside test_defense's
RESULT_KEYS = {**drv.RESULT_KEYS, 'nes': 'NES', 'square': 'SQUARE'}   # results.json column of each attack


def noise_owner(defense_model):
    """(the engine owner whose draws are seeded, EoT): EoTWrapper's owner is the wrapped model"""
    owner = getattr(defense_model, 'model', defense_model)
    if not hasattr(owner, 'seeded_noise'):
        raise ValueError('--noise_seed: the defender has no seeded draws (not one of the HIP engine owners)')
    return owner, int(getattr(defense_model, 'eot_steps', 1))


def evaluate_seeded(defense_model, attacks: Dict[str, Callable], images: torch.Tensor, labels: torch.Tensor, index_of: Callable[[int], int],
                    seed: int, batch_images: int = 1) -> torch.Tensor:
    """test_defense.evaluate_shard's table for `images`, image i being image index_of(i) of the dataset: evaluate_shard itself per
    batch (clean pass + batched attacks; at batch_images 1 everything), restarted at draw 0 with every image's own first row;
    with batch_images > 1 the one-image attacks follow per image, as in evaluate_shard, each restarted at the image's row"""
    owner, eot = noise_owner(defense_model)
    names = list(attacks)
    n, bi = images.shape[0], max(1, int(batch_images))
    out = torch.zeros(n, 1 + len(names))
    indexed = {k: a for k, a in attacks.items() if hasattr(a, 'image_index')}      # NES: see below
    batched = {k: a for k, a in attacks.items() if k not in indexed and (bi == 1 or getattr(a, 'batched', False))}
    try:
        for lo in range(0, n, bi):
            hi = min(n, lo + bi)
            owner.seeded_noise(int(seed), draw=0, first_row=[int(index_of(i)) * eot for i in range(lo, hi)])
            t = drv.evaluate_shard(defense_model, batched, images[lo:hi], labels[lo:hi], batch_images=bi)
            out[lo:hi, 0] = t[:, 0]
            for j, k in enumerate(batched):
                out[lo:hi, 1 + names.index(k)] = t[:, 1 + j]
            # attacks with an `image_index` (NES, Square Attack) draw their own numbers by dataset index, and their calls hold query rows, not the
            # batch's images: the defender's rows then count from the batch's first image, one draw per call from 0
            for k, a in indexed.items():
                owner.seeded_noise(int(seed), draw=0, first_row=int(index_of(lo)) * eot)
                a.image_index = torch.tensor([int(index_of(i)) for i in range(lo, hi)])
                success, bound, _ = a(images[lo:hi].clamp(0.0, 1.0), labels[lo:hi], defense_model)
                success = torch.as_tensor(success).view(-1).cpu()
                bound = torch.as_tensor(bound, dtype=torch.float32).view(-1).cpu()
                out[lo:hi, 1 + names.index(k)] = torch.where(success, bound, torch.full_like(bound, drv.FAILED))
            for i in range(lo, hi) if len(batched) + len(indexed) < len(names) else ():
                owner.seeded_noise(int(seed), draw=0, first_row=int(index_of(i)) * eot)
                for k in names:
                    if k not in batched and k not in indexed:
                        success, bound, _ = attacks[k](images[i:i + 1].clamp(0.0, 1.0), labels[i:i + 1], defense_model)
                        out[i, 1 + names.index(k)] = float(bound) if success else drv.FAILED
    finally:
        owner.seeded_noise(None)
    return out


def run_worker(rank: int, world: int, args, make_model: Callable, dataset: Tuple[torch.Tensor, torch.Tensor],
               backend: str = 'nccl', results_path: str = None):
    """test_defense.run_worker with seeded draws (args.noise_seed)"""
    drv.seed_everything(42)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '12355')
        dist.init_process_group(backend, rank=rank, world_size=world, timeout=timedelta(hours=12))
    args, defense_model = make_model(args)
    images, labels = dataset
    dev, seed = args.device, int(args.noise_seed)
    bi = max(1, int(getattr(args, 'batch_images', 1) or 1))
    attacks = args.attacks
    if getattr(args, 'schedule', 'static') == 'dynamic':
        n, queue = images.shape[0], drv.WorkQueue(world)
        local, busy, done = torch.zeros(n, 2 + len(attacks)), 0.0, 0
        while True:
            lo = queue.next() * bi
            if lo >= n:
                break
            hi, t = min(n, lo + bi), time.time()
            local[lo:hi, 1:] = evaluate_seeded(defense_model, attacks, images[lo:hi].to(dev), labels[lo:hi].to(dev),
                                               lambda i, lo=lo: lo + i, seed, bi)
            local[lo:hi, 0] = 1.0
            busy, done = busy + time.time() - t, done + hi - lo
        args.rank_busy_seconds, args.rank_images = busy, done
        table = drv.gather_dynamic(local, world, dev)
    else:
        mine = drv.shard_indices(images.shape[0], rank, world)
        local = evaluate_seeded(defense_model, attacks, images[mine].to(dev), labels[mine].to(dev), lambda i: mine[i], seed, bi)
        table = drv.gather_results(local, world, dev)
    res = None
    if rank == 0:
        cols = {RESULT_KEYS.get(name, name): table[:, 1 + j].tolist() for j, name in enumerate(attacks.keys())}
        res = drv.merge_results(results_path or os.path.join(args.results_folder, 'results.json'), float(table[:, 0].mean().item()), cols)
    if world > 1:
        dist.barrier()
    return res


def parse_args(argv=None):
    """test_defense's flags + --noise_seed; `--attack nes` / `--attack square` are this driver's own choices and never reach test_defense's parser"""
    argv = sys.argv[1:] if argv is None else list(argv)
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument('--noise_seed', type=int, required=True, help='seed of the defender\'s draws (ga_randn)')
    p.add_argument('--attack', type=str, default=None, help='test_defense\'s choices, or nes / square (black-box, attacks/nes.py, attacks/square.py)')
    own, rest = p.parse_known_args(argv)
    if own.attack is not None and own.attack not in OWN_ATTACKS:
        rest += ['--attack', own.attack]
    args = drv.parse_args(rest)
    args.noise_seed = own.noise_seed
    if own.attack in OWN_ATTACKS:
        args.attack = own.attack
    return args


def main():
    from .load_defense import load
    args = parse_args()
    rank, world = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local_rank)
    args.device = f'cuda:{local_rank}'

    def make_model(a):          # the attack selection of test_defense.main
        a, m = load(a)
        if a.attack == 'pgd':
            a.attacks = {'pgd': a.pgd}
        elif a.attack == 'pgd-bpda':
            a.attacks = {'pgd-bpda': getattr(a, 'pgd_bpda', None) or type(a.pgd)(eps=a.pgd.eps, step_size=a.pgd.step_size, steps=a.pgd.steps, bpda=True)}
        elif a.attack == 'nes':
            a.attacks = {'nes': a.nes}
        elif a.attack == 'square':
            a.attacks = {'square': a.square}
        elif a.attack is not None:
            a.attacks = {k: v for k, v in a.attacks.items() if k == a.attack}
        return a, m
    size = {'ids': 64, 'gender': 256, 'cars': 128}[args.experiment]
    data = drv.synthetic_dataset(args.synthetic, size, 100) if args.synthetic else drv.folder_dataset(args.images_path, size)
    res = run_worker(rank, world, args, make_model, data, backend='nccl')
    if rank == 0:
        print(json.dumps({k: (v if not isinstance(v, list) else f'{len(v)} values') for k, v in res.items()}))


if __name__ == '__main__':
    main()
