"""
CPU: the host side of the candidate-batched alpha search — the per-row alpha fields of ga_sampler_desc / ga_latent_mix_desc
(ABI 8) and their pitch checks, the expansion of [K, n] candidates into table rows, alpha_rows engines of the three defenders as
dry-run plans, the grid-search files, the adversarial-set builder on a stub defender, and the three classifier types of
AlphaEvaluator.  No kernel is launched here: every descriptor sent to the library is one it must reject.
"""
import ctypes as C
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from gen_adversarial_amd import _lib as L
from gen_adversarial_amd.engine import Engine, expand_alpha_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _struct(name):
    hdr = open(os.path.join(ROOT, 'include', 'ga_ops.h')).read()
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), hdr, flags=re.S).group(1)
    return re.sub(r'/\*.*?\*/', '', body, flags=re.S)


def test_header_binding_and_library_agree_on_the_alpha_table_fields():
    hdr = open(os.path.join(ROOT, 'include', 'ga_ops.h')).read()
    assert int(re.search(r'#define\s+GA_ABI_VERSION\s+(\d+)', hdr).group(1)) == 8 == L.ABI_VERSION == L.lib.ga_abi_version()
    smp = _struct('ga_sampler_desc')
    assert re.search(r'const float\*\s*alpha_rows;', smp) and re.search(r'int alpha_ld;\s*int alpha_col;', smp)
    assert re.search(r'int alpha_ld;', _struct('ga_latent_mix_desc'))
    names = [f[0] for f in L.SamplerDesc._fields_]
    assert names[-3:] == ['alpha_rows', 'alpha_ld', 'alpha_col']                 # in the header's order, after every earlier field
    assert [f[0] for f in L.LatentMixDesc._fields_][-2:] == ['rep', 'alpha_ld']
    assert L.lib.ga_sizeof_op() == C.sizeof(L.Op)


def test_a_table_with_a_too_small_pitch_is_rejected_without_a_gpu():
    d = L.SamplerDesc()
    d.mu_q = d.eps = d.z = d.alpha_rows = 16
    d.N, d.h, d.w, d.NL, d.ldq = 2, 1, 1, 4, 4
    d.alpha_col, d.alpha_ld = 1, 3                   # column pair 1 needs a pitch of at least 4 floats
    assert L.lib.ga_sampler_mix(C.byref(d), None) == -1
    d.alpha_col, d.alpha_ld = -1, 8
    assert L.lib.ga_sampler_mix(C.byref(d), None) == -1
    d.alpha_col, d.alpha_ld, d.mode, d.p, d.ldp, d.ldq = 0, 2, 1, 16, 8, 8      # the ND-VAE posterior sample takes no alphas
    assert L.lib.ga_sampler_mix(C.byref(d), None) == -1
    m = L.LatentMixDesc()
    m.codes = m.styles = m.alpha = m.out = 16
    m.R, m.J, m.D, m.alpha_ld = 2, 4, 8, 3            # per-row table narrower than the J alphas of a row
    assert L.lib.ga_latent_mix(C.byref(m), None) == -1
    m.backward, m.dout, m.dcodes = 1, 16, 16
    assert L.lib.ga_latent_mix(C.byref(m), None) == -1


def test_candidates_expand_to_rows_in_image_candidate_replica_order():
    cand = torch.tensor([[0.0, 0.25, 1.0], [0.1, 0.7, 0.3]], dtype=torch.float64)             # K = 2, n = 3
    B, K, E = 3, 2, 2
    t = expand_alpha_rows(cand, B * K * E, K * E, pairs=True)
    assert t.shape == (12, 6) and t.dtype == torch.float32
    for b in range(B):
        for k in range(K):
            for e in range(E):
                row = t[(b * K + k) * E + e]
                for j in range(3):
                    a = float(cand[k, j])
                    assert row[2 * j].item() == np.float32(a) and row[2 * j + 1].item() == np.float32(1.0 - a)
    # the second number is the double-precision difference rounded once, as the host stores ga_sampler_desc.one_minus_alpha;
    # 1.0f - float(a) differs from it for some alphas
    a = 0.7 * 0.3
    pair = expand_alpha_rows([[a]], 1, 1, pairs=True)[0]
    s = L.SamplerDesc()
    s.alpha, s.one_minus_alpha = a, 1.0 - a
    assert pair[0].item() == s.alpha and pair[1].item() == s.one_minus_alpha
    t1 = expand_alpha_rows(cand, 12, 4, pairs=False)
    assert t1.shape == (12, 3) and torch.equal(t1[5], cand[0].float()) and torch.equal(t1[6], cand[1].float())
    per_row = torch.rand(12, 3, dtype=torch.float64)
    assert torch.equal(expand_alpha_rows(per_row, 12, 4, pairs=False), per_row.float())       # K == rows: one vector per row
    with pytest.raises(ValueError):
        expand_alpha_rows(torch.rand(3, 3), 12, 4, pairs=False)                              # 3 candidates do not divide 4 rows


def test_alpha_rows_engines_build_for_the_three_defenders_without_a_gpu():
    from gen_adversarial_amd.nvae_spec import build_spec, init_nvae_state_dict
    from gen_adversarial_amd.vgg_spec import build_vgg_spec, init_vgg_state_dict
    from test_host_cpu import _small_e4e_defense
    cfg = {'initial_channels': 8, 'num_pre-post_process_blocks': 1, 'num_pre-post_process_cells': 2, 'num_scales': 2,
           'num_groups_per_scale': 2, 'is_adaptive': False, 'min_groups_per_scale': 1, 'num_cells_per_group': 1,
           'num_latent_per_group': 4, 'num_logistic_mixtures': 10, 'num_nf_cells': None}
    res = (3, 32, 32)
    n = len(build_spec(cfg, res).groups)
    sd, vspec, vsd = init_nvae_state_dict(cfg, res, 1), build_vgg_spec(10, 16), init_vgg_state_dict(10, 16, 2)
    B, K, E = 2, 3, 2
    kw = dict(rows=B * K * E, rep=K * E, alphas=[0.3] * n, device='cpu', dry_run=True, share_encoder=True)
    eng = Engine(sd, cfg, res, vsd, vspec, need_backward=False, alpha_rows=True, **kw)
    assert eng.enc_rows == B and len(eng.bwd) == 0 and eng.alpha_table.shape == (B * K * E, 2 * n)
    smp = [d for d in eng.fwd.descs if isinstance(d, L.SamplerDesc)]
    assert len(smp) == n and sorted(d.alpha_col for d in smp) == list(range(n))
    assert all(d.alpha_rows == eng.alpha_table.data_ptr() and d.alpha_ld == 2 * n and d.N == B * K * E for d in smp)
    assert smp[0].q_rep == K * E                                                  # the first sampler reads the shared encoder row
    cand = torch.rand(K, n, dtype=torch.float64)
    eng.set_alpha_rows(cand)
    assert torch.equal(eng.alpha_table, expand_alpha_rows(cand, B * K * E, K * E, pairs=True))
    eng.set_alphas([0.25] * n)                                                    # one vector for all rows
    assert torch.equal(eng.alpha_table, torch.tensor([0.25, 0.75] * n).expand(B * K * E, -1))
    with pytest.raises(ValueError):
        eng.set_alpha_rows(torch.rand(K, n + 1))
    plain = Engine(sd, cfg, res, vsd, vspec, **kw)
    assert plain.alpha_table is None and all(not d.alpha_rows for d in plain.fwd.descs if isinstance(d, L.SamplerDesc))
    assert eng.fwd.names == plain.fwd.names                                       # same plan: only the alpha source differs
    with pytest.raises(RuntimeError):
        plain.set_alpha_rows(cand)
    diff = Engine(sd, cfg, res, vsd, vspec, alpha_rows=True, **kw)                # a differentiable engine may carry the table too
    assert all(d.alpha_rows == diff.alpha_table.data_ptr() for d in diff.bwd.descs if isinstance(d, L.SamplerDesc))
    with pytest.raises(ValueError, match='input noise'):
        Engine(sd, cfg, res, vsd, vspec, noise_eps=2.0, alpha_rows=True, **kw)

    _, (esd, espec, gsd, gspec, avg, csd, cspec, alphas) = _small_e4e_defense()
    e4e = Engine.bare(B * K * E, device='cpu', dry_run=True, rep=K * E, resolution=(3, 64, 64), alphas=alphas, share_encoder=True,
                      need_backward=False, alpha_rows=True)
    e4e.build_e4e_defense(esd, espec, gsd, gspec, avg, csd, cspec, pool_to=32)
    J = gspec.n_latent
    mix = [d for d in e4e.fwd.descs if isinstance(d, L.LatentMixDesc)]
    assert len(mix) == 1 and mix[0].alpha == e4e.alpha_table.data_ptr() and mix[0].alpha_ld == J and mix[0].rep == K * E
    assert e4e.alpha_table.shape == (B * K * E, J) and e4e.alpha_dev is None and len(e4e.bwd) == 0
    assert torch.equal(e4e.alpha_table, torch.tensor(alphas, dtype=torch.float32).expand(B * K * E, -1))
    with pytest.raises(ValueError, match='input noise'):
        Engine.bare(B * K * E, device='cpu', dry_run=True, rep=K * E, resolution=(3, 64, 64), alphas=alphas, noise_eps=4.0, alpha_rows=True)

    from gen_adversarial_amd.resnet_spec import build_resnet_spec, init_resnet_state_dict
    from gen_adversarial_amd.stylegan_spec import build_stylegan_spec, init_stylegan_state_dict
    from gen_adversarial_amd.trans_spec import build_trans_spec, init_trans_state_dict
    tspec, tsd = build_trans_spec(4, (1, 1, 1, 1)), init_trans_state_dict(4, 1, (1, 1, 1, 1))
    g2 = build_stylegan_spec(32, width_div=8, style_dim=tspec.d_model)
    c2, c2sd = build_resnet_spec(4, 2, (1, 1, 1, 1), 4, 8), init_resnet_state_dict(4, 2, 3, (1, 1, 1, 1), 4, 8)
    tr = Engine.bare(B * K * E, device='cpu', dry_run=True, rep=K * E, resolution=(3, 64, 64), alphas=[0.1] * 16, share_encoder=True,
                     need_backward=False, alpha_rows=True)
    tr.build_trans_defense(tsd, tspec, init_stylegan_state_dict(g2, 2), g2, torch.zeros(16, tspec.d_model), c2sd, c2, pool_to=32, mid=128, crop=16)
    mix = [d for d in tr.fwd.descs if isinstance(d, L.LatentMixDesc)]
    assert len(mix) == 1 and mix[0].alpha == tr.alpha_table.data_ptr() and mix[0].alpha_ld == 16 and tr.alpha_table.shape == (B * K * E, 16)


class _StubEvaluator:
    """objective_many of a known function of the alphas: the search and its files can be checked without a defender"""

    def __init__(self, n):
        self.defense_model = Namespace(model=Namespace(interpolation_alphas=[0.0] * n))
        self.calls = []

    def objective_many(self, alphas, candidates_per_pass=None):
        self.calls.append((tuple(alphas.shape), candidates_per_pass))
        return 1.0 - (alphas - 0.5).abs().mean(dim=1).numpy()


def test_grid_search_files_round_trip_through_get_best_combination(tmp_path):
    from gen_adversarial_amd.experiments.alpha_learning import grid_search as G
    from gen_adversarial_amd.experiments.alpha_learning.common_utils import get_best_combination, random_search
    import src.experiments.alpha_learning.grid_search as shim
    assert shim.main is G.main
    args = G.parse_args(['--adv_images_path', 'x', '--n_steps', '7', '--classifier_path', 'c', '--classifier_type', 'resnet-50',
                         '--autoencoder_path', 'a', '--autoencoder_name', 'e4e', '--results_folder', str(tmp_path), '--seed', '3',
                         '--candidates_per_pass', '4'])
    assert args.results_folder == f'{tmp_path}/e4e_resnet-50/grid_search/' and os.path.isdir(args.results_folder)
    ev = _StubEvaluator(18)
    alphas, acc = G.main(args, evaluator=ev)
    assert ev.calls == [((7, 18), 4)]
    a, c = np.load(f'{args.results_folder}/alphas.npy'), np.load(f'{args.results_folder}/accuracies.npy')
    assert a.shape == (7, 18) and c.shape == (7, 1) and a.dtype == c.dtype == np.float32
    assert np.array_equal(a, alphas) and np.array_equal(c, acc)
    best = get_best_combination(args.results_folder)
    assert np.array_equal(best, alphas[np.argmax(1.0 - np.abs(alphas - 0.5).mean(axis=1))])
    # the candidates are the ones the one-at-a-time search drew for this seed: n_steps draws of torch.rand(n) from one generator
    g = torch.Generator().manual_seed(3)
    assert np.array_equal(alphas, torch.stack([torch.rand(18, generator=g) for _ in range(7)]).numpy())
    al2, _ = random_search(_StubEvaluator(18), 7, seed=3)
    assert np.array_equal(al2, alphas)


class _BrightnessNet(torch.nn.Module):
    """three classes decided by the mean brightness m: logits (10 m, 5.5, 10 (1 - m)), in double"""

    def forward(self, x):
        m = x.double().flatten(1).mean(dim=1)
        return torch.stack([10.0 * m, torch.full_like(m, 5.5), 10.0 * (1.0 - m)], dim=1).float()


def test_adversarial_set_keeps_exactly_the_images_fgsm_fools(tmp_path):
    from PIL import Image
    from gen_adversarial_amd.attacks.l2_attacks import FGSM
    from gen_adversarial_amd.experiments.alpha_learning import create_adversarial_dataset as A
    import src.experiments.alpha_learning.create_adversarial_dataset as shim
    assert shim.main is A.main and A.L2_BOUNDS == {'resnet-50': 4.0, 'vgg-11': 2.0, 'resnext-50': 4.0}
    # (class folder, file, mean brightness): the L2-2 sign step moves every pixel of an 8 x 8 image by 2 / sqrt(192) = 0.144
    cases = [('a', 'robust.png', 0.90), ('a', 'fooled1.png', 0.62), ('a', 'fooled2.png', 0.60), ('b', 'already_wrong.png', 0.90),
             ('b', 'fooled3.png', 0.52), ('c', 'fooled4.png', 0.38), ('c', 'robust2.png', 0.08), ('c', 'already_wrong2.png', 0.70)]
    rng = np.random.RandomState(0)
    src_dir = tmp_path / 'images'
    for cls, name, mean in cases:
        os.makedirs(src_dir / cls, exist_ok=True)
        px = np.clip(mean * 255 + rng.randint(-8, 9, size=(8, 8, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(px).save(src_dir / cls / name)
    net, attack = _BrightnessNet(), FGSM(l2_bound=2.0)
    images, names, labels = A.named_folder_dataset(str(src_dir), 8)
    assert sorted(names) == sorted((c, n) for c, n, _ in cases) and labels.tolist() == [{'a': 0, 'b': 1, 'c': 2}[c] for c, _ in names]
    expected = {}
    for i, nm in enumerate(names):                      # the reference's protocol: one image per attack call (:92-112)
        success, bound, adv = attack(images[i:i + 1], labels[i:i + 1], net)
        if success and bound > 0.:
            expected[nm] = adv[0]
    assert set(expected) == {('a', 'fooled1.png'), ('a', 'fooled2.png'), ('b', 'fooled3.png'), ('c', 'fooled4.png')}
    args = Namespace(images_folder=str(src_dir), n_samples=100, results_folder=str(tmp_path / 'adv'), classifier_type='vgg-11',
                     image_size=8, batch_images=3, seed=1)
    kept = A.main(args, net=net, device='cpu')
    assert set(kept) == set(expected) and len(kept) == len(expected)
    written = {(os.path.basename(r), f) for r, _, fs in os.walk(tmp_path / 'adv') for f in fs}
    assert written == set(expected)                                                # results_folder/<class>/<name>, nothing else
    for (cls, name), adv in expected.items():
        got = np.asarray(Image.open(tmp_path / 'adv' / cls / name))
        assert got.dtype == np.uint8 and np.array_equal(got, (adv * 255).permute(1, 2, 0).numpy().astype(np.uint8))
    args.n_samples, args.results_folder = 2, str(tmp_path / 'adv2')               # stops at n_samples, mid-batch too
    kept2 = A.main(args, net=net, device='cpu')
    assert len(kept2) == 2 and kept2 == kept[:2] and sum(len(fs) for _, _, fs in os.walk(tmp_path / 'adv2')) == 2
    p = A.parse_args(['--images_folder', 'i', '--n_samples', '5', '--results_folder', 'r', '--classifier_path', 'c', '--autoencoder_path', 'a',
                      '--classifier_type', 'resnext-50'])
    assert (p.n_samples, p.classifier_type) == (5, 'resnext-50')


@pytest.mark.parametrize('classifier_type', ['vgg-11', 'resnet-50', 'resnext-50'])
def test_alpha_evaluator_reaches_the_defender_of_every_classifier_type(classifier_type):
    from gen_adversarial_amd.experiments.alpha_learning.common_utils import DEFENDERS, AlphaEvaluator
    args = Namespace(classifier_type=classifier_type, classifier_path='/nonexistent', autoencoder_path='/nonexistent')
    with pytest.raises(RuntimeError, match='GPU only'):
        AlphaEvaluator(args, 'cpu', images=torch.zeros(1, 3, 8, 8), labels=torch.zeros(1, dtype=torch.long))
    assert args.image_size == DEFENDERS[classifier_type][4]
    assert {k: v[2:] for k, v in DEFENDERS.items()} == {'vgg-11': (24, 0.7, 64), 'resnet-50': (18, 1.0, 256), 'resnext-50': (16, 0.7, 128)}
    with pytest.raises(ValueError):
        AlphaEvaluator(Namespace(classifier_type='vgg-16', classifier_path='', autoencoder_path=''), 'cpu')
