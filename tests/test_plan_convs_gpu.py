"""
Every dense contraction of the shipped plans, as tuned, against the float64 interpreter of tests/convref.py.

The engines are the ones bench.py times, built by the same code (configs[1] NVAE + VGG at bench.py's 1024-row chunk, the
configs[2] e4e defender at 32 rows and the configs[4] Style-Transformer defender at 64 rows, EoT 32: `plan_convs`), and, in a
second fixture (`more_plan_convs`, test_more_plan_conv_descriptors), the other plans bench.py builds of the NVAE model -- 512 and
32 rows, the same with the encoder shared by the EoT replicas (addend_rep > 1), the K-cotangent class-Jacobian plans (dact_rep >
1), the fp32 secondary (every descriptor form on conv_mfma) -- and the reduced engines of planzoo.device_engines.  apply_tuning makes its
real choices only on a GPU (tiles 8, 9, 11 and 12 need their weight fragments; a rebuilt descriptor gets the copy its tile reads from
engine_core.TILES, as the engine does).  Each distinct ConvDesc of their forward and
backward plans runs on buffers of this test with fewer rows, fresh weights and NaN-filled outputs, and must
  - be accepted (GA_E_UNSUPPORTED on a shipped descriptor is a plan the engine would fail to run),
  - meet |y - ref| <= tau * scale + slack + 2^-22 |ref| on every element (tau_bf3 / tau_fp32 of tests/convref.py),
  - leave the channels [Cout, ldy) and a guard region past the last pixel NaN,
  - give bitwise-equal results on two launches (split-K and every tile sum in a fixed order).
The default run checks a deterministic subset: per class (Conv.cls: tile, split-K, split-bf16, second source, transposed, flags,
act' epilogue, addend, prologue kind and activation, dact_rep > 1, addend_rep > 1, second addend, broadcast addend, in-place
accumulation, an operand off 16-byte alignment) the descriptors of the smallest and the largest Wo.  GA_TEST_ALL_PLAN_CONVS=1
checks all of them.

test_bound_catches_dropped_lo_weights shows, per tile, that the bound fails when the kernel runs on the bf16 weights alone;
test_bound_sees_a_misread_row_replication that it fails when dact_x or the addend is read at row n instead of n / rep.
test_tile_eligibility_fuzz requests tiles 5 - 8 and 11 on shapes around their eligibility edges: the library refuses exactly
what engine_core.halo_ok / frag_ok / thin_ok reject (the predicates apply_tuning relies on) and computes the rest correctly;
test_quadrant_tile_eligibility_fuzz does the same for tiles 8 and 9 on 4 x 4 images (the existing cases have Wo >= 16).
test_tune_table_census counts which entries of conv_tune_gfx950.json these plans reach and which a default run checks.
"""
import gc
import math
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import convref as R                                                      # noqa: E402
import planzoo                                                           # noqa: E402
from gen_adversarial_amd import _lib as L                                # noqa: E402
from gen_adversarial_amd.engine_core import (TILES as TILE_TABLE, WeightStore, conv_key, frag_ok, halo_ok, resolve_tile, thin_ok,  # noqa: E402
                                             tune_cache, _bf3_vec_out)

DEV = 'cuda:0'
ALL = os.environ.get('GA_TEST_ALL_PLAN_CONVS', '0') == '1'
GUARD = 256                                 # floats past the last output pixel that must stay NaN
OPERANDS = ('x', 'x2', 'w', 'bias', 'pro_scale', 'pro_shift', 'addend', 'addend2', 'dact_x', 'dact_scale', 'dact_shift', 'y',
            'w_hi', 'w_lo', 'w_frag', 'ws')
INTS = tuple(f for f, _ in L.ConvDesc._fields_ if f not in OPERANDS + ('ws_floats', 'x_bytes', 'x2_bytes', 'w_bytes'))
TILES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12)
NVAE_BIG = 512                              # rows of the 16-image NVAE variants (bench.py: 16 images x EoT 32)


def _frag_fed(tile):
    return tile in TILE_TABLE and TILE_TABLE[tile].frag is not None


class Conv:
    """one descriptor as the plan holds it: its integer fields, which operands it has, their 16-byte alignment (a pointer
    offset changes the kernel's load path) and whether an addend aliases the output"""

    def __init__(self, d, where='', tkey=None):
        self.f = {k: int(getattr(d, k)) for k in INTS}
        self.has = frozenset(k for k in OPERANDS if getattr(d, k) and k not in ('ws', 'w_frag'))
        self.frag = bool(d.w_frag) and _frag_fed(d.tile)
        self.align = tuple(sorted((k, getattr(d, k) % 16 // 4) for k in self.has))
        self.alias = tuple(k for k in ('addend', 'addend2') if getattr(d, k) and getattr(d, k) == d.y)
        self.where = [where]
        self.tkeys = {tkey} if tkey else set()      # the tune-table entries this descriptor runs as named (census)

    def __getattr__(self, k):
        f = self.__dict__.get('f')
        if f is not None and k in f:
            return f[k]
        raise AttributeError(k)

    @property
    def key(self):
        return tuple(sorted(self.f.items())), self.has, self.frag, self.align, self.alias

    @property
    def bf3(self):
        return 'w_hi' in self.has

    @property
    def kdim(self):
        return self.KH * self.KW * (self.C1 + self.C2)

    @property
    def prologue(self):
        """(none / chan / row / prelu, pro_act): each pair is another template instantiation of every kernel"""
        if 'pro_scale' not in self.has:
            return 'none', self.pro_act
        if self.flags & L.GA_CONV_PRO_PRELU:
            return 'prelu', self.pro_act
        return ('row' if self.pro_per_row else 'chan'), self.pro_act

    @property
    def drep(self):
        return self.dact_rep if 'dact_x' in self.has and self.dact_rep > 1 else 1

    @property
    def arep(self):
        return self.addend_rep if 'addend' in self.has and not self.addend_bcast_n and self.addend_rep > 1 else 1

    def cls(self):
        """what selects a kernel, a template instantiation or an index expression: the tile, split-K, split-bf16, the second
        source, the transposed form, the flags, the act' epilogue and the addend; the prologue kind with its activation, the row
        replication of dact_x and of the addend (n / rep), the second addend, the addend broadcast over n, in-place accumulation
        and any operand off 16-byte alignment (the scalar load / store paths)"""
        return (self.tile, self.splits > 1, self.bf3, self.C2 > 0, self.sd > 1, self.flags, 'dact_x' in self.has, 'addend' in self.has,
                self.prologue, self.drep > 1, self.arep > 1, 'addend2' in self.has, bool(self.addend_bcast_n) and 'addend' in self.has,
                bool(self.alias), any(o for _, o in self.align))

    def label(self):
        f = self
        s = f'tile {f.tile:2d} split {f.splits:2d} {"bf3 " if f.bf3 else "fp32"} {f.N}x{f.Hi}x{f.Wi}x{f.C1}' + (f'+{f.C2}' if f.C2 else '')
        s += f' -> {f.Ho}x{f.Wo}x{f.Cout} k{f.KH}x{f.KW} s{f.sn}/{f.sd} p{f.pad}'
        extra = [k for k in ('pro_scale', 'dact_x', 'addend', 'addend2', 'bias') if k in self.has]
        if f.flags:
            extra.append(f'flags{f.flags}')
        if f.pro_act:
            extra.append(f'act{f.pro_act}')
        if self.alias:
            extra.append('in-place')
        return s + (' [' + ','.join(extra) + ']' if extra else '')


CENSUS = []             # one row per conv of every plan the fixtures build, for test_tune_table_census
BUILD_S = {}            # plan -> seconds to build its engine
_SHARED = {}            # the configs[1] NVAE model and its WeightStore: the NVAE variants draw, fold and split nothing again


def _tune_key(eng, d):
    """conv_key(d) as apply_tuning looked it up: an entry with use_bf3 = 0 took the split weights off the descriptor afterwards"""
    k = conv_key(d)
    return 'b3_' + k if not d.w_hi and id(d) in eng._conv_w else k


def _resolved(eng, d, ent):
    """engine_core.resolve_tile for d and the entry's (tile, splits), on a copy, with the fragment copies the engine can make"""
    c = L.ConvDesc.from_buffer_copy(d)
    c.w_frag = None

    def can_frag(tile):
        w = eng._frag_weight(d, tile)
        if w is None:
            return False
        c.w_frag = TILE_TABLE[tile].frag(eng.store, w, d).data_ptr()
        return True
    return tuple(int(v) for v in resolve_tile(c, ent[0], ent[1], can_frag))


def _plan_convs(eng, plan_name, out):
    cache = tune_cache()
    for plan, tag in ((eng.fwd, 'fwd'), (eng.bwd, 'bwd')):
        for d, name in zip(plan.descs, plan.names):
            if isinstance(d, L.ConvDesc):
                where = f'{plan_name}.{tag}.{name}'
                tkey = _tune_key(eng, d)
                ent = cache.get(tkey)
                as_named = False
                if ent is not None:
                    ent = (int(ent[0]), int(ent[1]), int(ent[2]) if len(ent) > 2 else 1)
                    as_named = (d.tile, d.splits) == ent[:2]
                c = Conv(L.ConvDesc.from_buffer_copy(d), where, tkey if as_named else None)
                if c.key in out:
                    out[c.key].where.append(where)
                    out[c.key].tkeys |= c.tkeys
                else:
                    out[c.key] = c
                if ent is not None:
                    CENSUS.append(SimpleNamespace(where=where, tkey=tkey, ent=ent, ran=(int(d.tile), int(d.splits)), as_named=as_named,
                                                  want=_resolved(eng, d, ent), label=c.label()))


def _build_plans(builders, every, per_plan):
    """build the engines one at a time, add their distinct conv descriptors to `every` ({Conv.key: Conv}), free them"""
    for name, build in builders:
        t0 = time.perf_counter()
        eng = build()
        torch.cuda.synchronize()
        BUILD_S[name] = time.perf_counter() - t0
        mine = {}
        _plan_convs(eng, name, mine)
        del eng
        gc.collect()
        torch.cuda.empty_cache()
        new = 0
        for k, c in mine.items():
            if k in every:
                every[k].where += c.where
                every[k].tkeys |= c.tkeys
            else:
                every[k] = c
                new += 1
        per_plan[name] = (len(mine), new)
        print(f'  {name}: built in {BUILD_S[name]:.1f} s, {len(mine)} distinct conv descriptors, {new} new', flush=True)


@pytest.fixture(scope='module')
def plan_convs():
    """the distinct conv descriptors of the three shipped plans, by plan; the engines are built one at a time and freed"""
    from bench import build_e4e_defender, build_model, build_trans_defender

    def nvae():                                     # the model and the WeightStore serve the NVAE variants of more_plan_convs
        eng, model = build_model(DEV, 1024, 32, seed=0, precision='bf16x3')
        _SHARED.update(model=model, first=SimpleNamespace(rep=eng.rep, noise_eps=eng.noise_eps, store=eng.store))
        return eng
    builders = (('configs1_nvae', nvae),
                ('configs2_e4e', lambda: build_e4e_defender(DEV, 32, 32, 'bf16x3')[0]),
                ('configs4_trans', lambda: build_trans_defender(DEV, 64, 32, 'bf16x3')[0]))
    per_plan, every = {}, {}
    print('\nplan convs, the three benchmarked plans:', flush=True)
    _build_plans(builders, every, per_plan)
    print(f'plan convs: {({k: v[0] for k, v in per_plan.items()})} distinct per plan, {len(every)} distinct over the three plans', flush=True)
    return list(every.values())


@pytest.fixture(scope='module')
def more_plan_convs(plan_convs):
    """the distinct conv descriptors that only the other plans hold: the NVAE variants bench.py builds beside its 1024-row chunk
    plan (planzoo.nvae_variants, on the WeightStore of the 1024-row engine: no second 1024-row engine, nothing folded twice) and
    the reduced engines of planzoo.device_engines; real engines, one alive at a time, apply_tuning's own choices"""
    builders = list(planzoo.nvae_variants(DEV, _SHARED['first'], _SHARED['model'], 32, NVAE_BIG)) + list(planzoo.device_engines(DEV))
    per_plan, every = {}, {c.key: c for c in plan_convs}
    print('\nplan convs, the other plans:', flush=True)
    _build_plans(builders, every, per_plan)
    seen = {c.key for c in plan_convs}
    more = [c for k, c in every.items() if k not in seen]
    print(f'plan convs: {len(more)} distinct descriptors beside the {len(seen)} of the three plans, {sum(BUILD_S.values()):.1f} s of engine '
          f'builds in all', flush=True)
    yield more
    _SHARED.clear()


def _subset(convs):
    """per class, the descriptors of the smallest and the largest Wo (ties broken by the full descriptor, deterministic)"""
    by = {}
    for c in convs:
        by.setdefault(c.cls(), []).append(c)
    pick = []
    for k in sorted(by, key=repr):
        v = sorted(by[k], key=lambda c: (c.Wo, repr(c.key)))
        pick.append(v[0])
        if len(v) > 1:
            pick.append(v[-1])
    return pick


def _rows(c):
    """a cheaper row count: a multiple of dact_rep, addend_rep and (small images) of the images per 128-pixel tile.  A replicated
    operand keeps two rows of its own when the plan has them: with one row every reading of n / rep lands on row 0"""
    m = 1
    for rep in (c.drep, c.arep):
        if rep > 1:
            m = math.lcm(m, 2 * rep if c.N % (2 * rep) == 0 else rep)
    howo = c.Ho * c.Wo
    if howo < 128:
        m = math.lcm(m, -(-128 // howo))
    return min(c.N, m) if c.N % m == 0 else c.N


def _buf(n, off, fill, gen=None, scale=1.0):
    """n floats starting `off` floats past a 256-byte aligned allocation"""
    b = torch.empty(n + off, device=DEV)
    v = b[off:]
    if fill == 'nan':
        v.fill_(float('nan'))
    elif fill == 'randn':
        v.normal_(0.0, scale, generator=gen)
    elif fill == 'rand':
        v.uniform_(0.5, 1.5, generator=gen)
    return v


def run_conv(c, n=None, seed=0, zero_lo=False, w=None):
    """run descriptor c on fresh operands with n rows; -> (y buffer after launch 1, after launch 2, tensors for conv_ref, desc)
    or raises L.GaError"""
    n = c.N if n is None else n
    gen = torch.Generator(device=DEV).manual_seed(seed)
    al = dict(c.align)
    d = L.ConvDesc()
    for k, v in c.f.items():
        setattr(d, k, v)
    d.N = n
    howo, pin = c.Ho * c.Wo, n * c.Hi * c.Wi
    t = {}

    def put(k, numel, fill, scale=1.0):
        t[k] = _buf(numel, al.get(k, 0), fill, gen, scale)
        setattr(d, k, t[k].data_ptr())
    put('x', pin * c.ldx, 'randn')
    if 'x2' in c.has:
        put('x2', pin * c.ldx2, 'randn')
    K = c.kdim
    if w is None:
        w = torch.randn(c.Cout, K, generator=gen, device=DEV) / math.sqrt(K)
    t['w'] = _buf(c.Cout * K, al.get('w', 0), None)
    t['w'].copy_(w.to(DEV).reshape(-1))
    d.w = t['w'].data_ptr()
    if 'bias' in c.has:
        put('bias', c.Cout, 'randn', 0.5)
    if 'pro_scale' in c.has:
        m = n * c.C1 if c.pro_per_row else c.C1
        put('pro_scale', m, 'rand')
        put('pro_shift', m, 'randn', 0.5)
    if 'dact_x' in c.has:
        drep = c.dact_rep if c.dact_rep > 1 else 1
        put('dact_x', n // drep * howo * c.lddact, 'randn')
        if 'dact_scale' in c.has:
            put('dact_scale', c.Cout, 'rand')
            put('dact_shift', c.Cout, 'randn', 0.5)
    y_numel = n * howo * c.ldy
    y0 = _buf(y_numel + GUARD, 0, 'nan')
    y_init = None
    if c.alias:                         # in-place accumulation: y holds the addend on entry (channels < Cout)
        y_init = y0.clone()
        y_init[:y_numel].view(-1, c.ldy)[:, :c.Cout] = torch.randn(n * howo, c.Cout, generator=gen, device=DEV)
    if 'addend' in c.has and 'addend' not in c.alias:
        arep = c.addend_rep if c.addend_rep > 1 else 1
        rows = 1 if c.addend_bcast_n else n // arep
        put('addend', rows * howo * c.ldadd, 'randn')
    if 'addend2' in c.has and 'addend2' not in c.alias:
        put('addend2', n * howo * c.ldadd2, 'randn')
    y = _buf(y_numel + GUARD, al.get('y', 0), 'nan')
    d.y = y.data_ptr()
    for k in c.alias:
        setattr(d, k, d.y)
        t[k] = y_init[:y_numel]
    if c.splits > 1:
        ws = _buf(c.splits * n * howo * c.Cout, 0, None)
        d.ws, d.ws_floats = ws.data_ptr(), ws.numel()
    if c.bf3:
        wt = t['w'].view(c.Cout, K)
        if zero_lo:                     # the kernel then computes with bf16 weights only
            wt = wt.to(torch.bfloat16).float()
        store = WeightStore(DEV)
        hi, lo = store.split(wt)
        d.w_hi, d.w_lo = hi.data_ptr(), lo.data_ptr()
        t['_keep'] = [wt, hi, lo]
        if c.frag and _frag_fed(c.tile):
            fr = TILE_TABLE[c.tile].frag(store, wt, d)
            d.w_frag = fr.data_ptr()
            t['_keep'].append(fr)
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for _ in range(2):
        src = y_init if y_init is not None else y0
        y.copy_(src)
        try:
            L.run(d, stream)
        except L.GaError as ex:     # a refused request launches nothing
            torch.cuda.synchronize()
            ex.untouched = torch.equal(y.view(torch.int32), src.view(torch.int32))
            raise
        torch.cuda.synchronize()
        outs.append(y.clone())
    t.pop('_keep', None)
    t['y'] = y
    return outs, t, d


def _misread_rows(d, t, field):
    """(descriptor fields, tensors) for conv_ref with the row index of a replicated operand misread: row n of dact_x (field
    'dact_rep') or of the addend ('addend_rep') instead of row n / rep, clamped to the rows the operand has"""
    name, ld = {'dact_rep': ('dact_x', d.lddact), 'addend_rep': ('addend', d.ldadd)}[field]
    rep = getattr(d, field)
    assert rep > 1 and d.N % rep == 0 and d.N // rep >= 2, (field, rep, d.N)
    rows = t[name].reshape(d.N // rep, d.Ho * d.Wo * ld)
    idx = torch.arange(d.N, device=rows.device).clamp_max(d.N // rep - 1)
    f = SimpleNamespace(**{k: int(getattr(d, k)) for k in INTS})
    setattr(f, field, 1)
    return f, dict(t, **{name: rows[idx].reshape(-1)})


def check_conv(c, n=None, seed=0, zero_lo=False, misread=None, keep=None):
    """-> (ratio to the bound, max |err| / scale, [failure messages]); misread: the REFERENCE reads that replicated operand
    with the wrong row index (sensitivity tests); keep: a list that receives the output of the first launch"""
    n = _rows(c) if n is None else n
    (y1, y2), t, d = run_conv(c, n, seed, zero_lo)
    if keep is not None:
        keep.append(y1)
    bad = []
    howo, m = c.Ho * c.Wo, n * c.Ho * c.Wo
    out = y1[:m * c.ldy].view(m, c.ldy)
    if c.ldy > c.Cout and not torch.isnan(out[:, c.Cout:]).all():
        bad.append('wrote channels >= Cout')
    if not torch.isnan(y1[m * c.ldy:]).all():
        bad.append('wrote past the last pixel')
    if not torch.equal(y1.view(torch.int32), y2.view(torch.int32)):
        bad.append('two launches differ')
    t = {k: v for k, v in t.items() if k != 'y'}
    ref, scale, slack = R.conv_ref(*(_misread_rows(d, t, misread) if misread else (d, t)))
    tau = R.TAU_BF3 if c.bf3 else R.TAU_FP32
    r, e = R.bound_ratio(out[:, :c.Cout].reshape(n, c.Ho, c.Wo, c.Cout), ref, scale, slack, tau)
    return r, e, bad


def _pick(convs):
    """what a descriptor test checks of its list: the subset is taken over each list on its own, so the three benchmarked plans
    keep the smallest and the largest Wo of every class of theirs whatever the other plans hold"""
    return convs if ALL else _subset(convs)


def test_plan_conv_descriptors(plan_convs):
    _check_descriptors(plan_convs)


def test_more_plan_conv_descriptors(more_plan_convs):
    """the descriptors of the NVAE variants and the reduced engines that the three benchmarked plans do not hold"""
    _check_descriptors(more_plan_convs)


def _check_descriptors(plan_convs):
    pick = _pick(plan_convs)
    print(f'checking {len(pick)} of {len(plan_convs)} distinct conv descriptors ({len(plan_convs) - len(pick)} skipped'
          f'{"" if ALL else "; GA_TEST_ALL_PLAN_CONVS=1 checks all"})', flush=True)
    fails, worst = [], {}
    for i, c in enumerate(pick):
        try:
            r, e, bad = check_conv(c, seed=i)
        except L.GaError as ex:
            fails.append(f'{c.label()} ({c.where[0]}): {ex}')
            continue
        tau = R.TAU_BF3 if c.bf3 else R.TAU_FP32
        print(f'  {c.label():90s} n={_rows(c):4d}  max|err|/scale {e:.2e} = {e / tau:.3f} tau  bound {r:.3f}  {c.where[0]}', flush=True)
        k = (c.tile, c.bf3)
        worst[k] = max(worst.get(k, 0.0), e / tau)
        if r > 1.0 or bad:
            fails.append(f'{c.label()} ({c.where[0]}): bound ratio {r:.3g} {bad}')
    for (tile, bf3), v in sorted(worst.items()):
        print(f'  tile {tile:2d} {"bf3 " if bf3 else "fp32"}: worst max|err|/scale = {v:.3f} tau', flush=True)
    assert not fails, '\n'.join(fails)


def _synthetic(tile):
    """a 3x3, 32 -> 64 conv on 8 x 16 images that every 3x3 tile takes; tile 12: a 1x1, 64 -> 128 conv on 16 images of 4 x 4;
    tile 9: a 3x3, 32 -> 128 conv on one group of 32 images of 4 x 4"""
    d = L.ConvDesc()
    d.N, d.Hi, d.Wi, d.C1, d.Ho, d.Wo, d.Cout, d.KH, d.KW, d.sn, d.sd, d.pad = 8, 8, 16, 32, 8, 16, 64, 3, 3, 1, 1, 1
    if tile == 12:
        d.N, d.Hi, d.Wi, d.C1, d.Ho, d.Wo, d.Cout, d.KH, d.KW, d.pad = 16, 4, 4, 64, 4, 4, 128, 1, 1, 0
    if tile == 9:
        d.N, d.Hi, d.Wi, d.Ho, d.Wo, d.Cout = 32, 4, 4, 4, 4, 128
    d.ldx, d.ldy, d.tile, d.splits = d.C1, d.Cout, tile, 1
    d.x = d.w = d.y = d.w_hi = d.w_lo = 4096
    d.w_frag = 4096 if _frag_fed(tile) else None
    return Conv(d, f'synthetic tile {tile}')


def test_bound_catches_dropped_lo_weights(plan_convs):
    """per tile, one split-bf16 descriptor (from the plans when they hold one: the shortest contraction) run with w_lo = 0:
    the kernel then multiplies by bf16(w) alone and the bound must fail; the same descriptor with w_lo passes"""
    msgs = []
    for tile in TILES:
        cands = [c for c in plan_convs if c.tile == tile and c.bf3 and c.splits == 1 and c.sd == 1 and _bf3_vec_out(_as_desc(c), 1)]
        c = min(cands, key=lambda c: (c.kdim, repr(c.key))) if cands else _synthetic(tile)
        r_ok, e_ok, bad = check_conv(c, seed=1)
        r_lo, e_lo, _ = check_conv(c, seed=1, zero_lo=True)
        print(f'  tile {tile:2d}: {c.label()}  bound {r_ok:.3f} -> {r_lo:.1f} without w_lo ({e_lo:.2e} of the scale)', flush=True)
        if r_ok > 1.0 or bad:
            msgs.append(f'tile {tile}: fails with w_lo ({r_ok:.3g}, {bad})')
        if r_lo <= 1.0:
            msgs.append(f'tile {tile}: the bound does not see the dropped w_lo ({r_lo:.3g})')
    assert not msgs, '\n'.join(msgs)


def _as_desc(c):
    d = L.ConvDesc()
    for k, v in c.f.items():
        setattr(d, k, v)
    for k in c.has:
        setattr(d, k, 4096 + 4 * dict(c.align).get(k, 0))
    return d


def test_bound_sees_a_misread_row_replication(more_plan_convs):
    """one dact_rep > 1 descriptor (K-cotangent plans; a fragment-fed tile when the plans hold one there) and one addend_rep > 1
    descriptor (shared-encoder plans), the shortest contraction of each, with the REFERENCE reading row n of the replicated
    operand instead of row n / rep (clamped to its rows): the bound must fail; with the right index it passes.
    Measured, ratio to the bound: dact_rep = 16 (pw2^T of the 32-row K = 16 plan, tile 12, 32 rows) 0.119 with the right index,
    1.0e6 with the wrong one (the wrong row's SiLU' factor is near zero somewhere, and the scale with it); addend_rep = 32
    (enc_combiner of the 512-row shared-encoder plan, tile 12, 64 rows) 0.041 against 1.0e4 (0.48 of the scale)."""
    msgs = []
    for field, name in (('dact_rep', 'dact_x'), ('addend_rep', 'addend')):
        rep_of = (lambda c: c.drep) if field == 'dact_rep' else (lambda c: c.arep)
        cands = [c for c in more_plan_convs if rep_of(c) > 1 and name not in c.alias and c.N // rep_of(c) >= 2]
        assert cands, f'no plan holds a descriptor with {field} > 1'
        c = min(cands, key=lambda c: (not _frag_fed(c.tile), c.kdim, repr(c.key)))
        n = _rows(c)
        assert n // rep_of(c) >= 2, (c.label(), n)
        r_ok, _, bad = check_conv(c, n=n, seed=2)
        r_mis, e_mis, _ = check_conv(c, n=n, seed=2, misread=field)
        print(f'  {field} = {rep_of(c)}: {c.label()} n={n}  bound {r_ok:.3f} -> {r_mis:.3g} with row n for n / rep ({e_mis:.2e} of the scale)'
              f'  {c.where[0]}', flush=True)
        if r_ok > 1.0 or bad:
            msgs.append(f'{field}: fails with the right index ({r_ok:.3g}, {bad})')
        if r_mis <= 1.0:
            msgs.append(f'{field}: the bound does not see the misread row index ({r_mis:.3g})')
    assert not msgs, '\n'.join(msgs)


def _fuzz_cases(n, seed):
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        c = dict(Wo=int(rs.choice([16, 24, 32, 48, 64, 128, 256])), Ho=int(rs.choice([4, 6, 8, 12, 16])), C1=int(rs.choice([32, 48, 64, 96])),
                 pad=int(rs.choice([0, 1, 1])), stride=int(rs.choice([1, 1, 1, 2])), x2=int(rs.choice([0, 0, 0, 32])),
                 Cout=int(rs.choice([8, 40, 100, 130, 132, 257, 260])), N=int(rs.randint(1, 4)),
                 pro=int(rs.choice([0, 0, 1, 2, 3])), act=int(rs.choice([0, 0, 1, 3])), splits=int(rs.choice([1, 1, 2])),
                 addend=int(rs.randint(0, 2)), dact=int(rs.choice([0, 0, 1, 3])), seed=int(rs.randint(1 << 30)))
        if c['Ho'] * c['Wo'] * c['N'] > 8192:
            c['N'] = 1
        out.append(c)
    return out


@pytest.mark.parametrize('c', _fuzz_cases(40, 955), ids=lambda c: 'N{N}_{Ho}x{Wo}_{C1}+{x2}to{Cout}_p{pad}s{stride}_pro{pro}a{act}_s{splits}'.format(**c))
def test_tile_eligibility_fuzz(c):
    """tiles 5, 6, 7, 8, 11 requested with their fragments built: refused (y untouched) exactly when the predicate says no,
    else within the float64 bound"""
    s, p = c['stride'], c['pad']
    Hi, Wi = (c['Ho'] - 1) * s + 3 - 2 * p, (c['Wo'] - 1) * s + 3 - 2 * p
    d = L.ConvDesc()
    d.N, d.Hi, d.Wi, d.C1, d.C2, d.Ho, d.Wo, d.Cout = c['N'], Hi, Wi, c['C1'], c['x2'], c['Ho'], c['Wo'], c['Cout']
    d.KH = d.KW = 3
    d.sn, d.sd, d.pad, d.ldx, d.ldx2, d.ldy = s, 1, p, c['C1'], c['x2'], c['Cout']
    d.x = d.w = d.y = d.w_hi = d.w_lo = 4096
    if c['x2']:
        d.x2 = 4096
    d.bias = 4096
    if c['pro']:
        d.pro_scale = d.pro_shift = 4096
        d.pro_per_row = int(c['pro'] == 2)
        d.flags |= L.GA_CONV_PRO_PRELU if c['pro'] == 3 else 0
    d.pro_act = c['act'] if c['pro'] != 3 else 0
    if c['addend']:
        d.addend, d.ldadd = 4096, c['Cout']
    if c['dact']:
        d.dact_x, d.lddact, d.dact_act = 4096, c['Cout'], c['dact']
    d.splits = c['splits']
    if c['splits'] > 1:
        d.ws = 4096
    fail = []
    for tile in (5, 6, 7, 8, 11):
        d.tile = tile
        d.w_frag = 4096 if (tile == 8 and c['C1'] % 32 == 0 and not c['x2']) or (tile == 11 and c['C1'] in (32, 64) and not c['x2']) else None
        conv = Conv(d, f'fuzz tile {tile}')
        want = {8: frag_ok, 11: thin_ok}.get(tile, halo_ok)(d)
        try:
            r, e, bad = check_conv(conv, n=c['N'], seed=c['seed'])
        except L.GaError as ex:
            assert 'UNSUPPORTED' in str(ex), (tile, str(ex))
            if not ex.untouched:
                fail.append(f'tile {tile}: refused but wrote the output')
            if want:
                fail.append(f'tile {tile}: refused, the predicate says eligible')
            continue
        if not want:
            fail.append(f'tile {tile}: accepted, the predicate says ineligible')
        if r > 1.0 or bad:
            fail.append(f'tile {tile}: bound ratio {r:.3g} (max|err|/scale {e:.2e}) {bad}')
    assert not fail, '\n'.join(fail)


def _quad_cases(seed):
    """twelve 3x3 / pad 1 / stride 1 requests on 4 x 4 images, the smallest shapes tiles 8 and 9 take: every N of the list twice
    (whole groups of 32, a partial group, and 40: tile 9 refuses it), the other fields drawn.  Seed 961 is the first whose list has
    both tiles accept every N but 40, 32 and 96 channels, 40 and 128 outputs, each prologue, act', an addend and two K slices, tile 8
    alone accept N = 40, and both refuse (257 outputs, two slices of one chunk, a per-channel affine + SiLU with two slices)"""
    rs = np.random.RandomState(seed)
    out = []
    for N in (8, 16, 32, 40, 64, 96) * 2:
        out.append(dict(N=N, C1=int(rs.choice([32, 96])), Cout=int(rs.choice([40, 128, 257])), pro=int(rs.choice([0, 1, 2])),
                        act=int(rs.choice([0, 0, 1])), dact=int(rs.choice([0, 1, 3])), addend=int(rs.randint(0, 2)),
                        splits=int(rs.choice([1, 2])), seed=int(rs.randint(1 << 30))))
    return out


@pytest.mark.parametrize('c', _quad_cases(961), ids=lambda c: 'N{N}_{C1}to{Cout}_pro{pro}a{act}_d{dact}_add{addend}_s{splits}'.format(**c))
def test_quadrant_tile_eligibility_fuzz(c):
    """tiles 8 and 9 requested on 4 x 4 images with tile 8's fragments: each is refused (y untouched) exactly when its
    engine_core.TILES predicate says no, else it is within the float64 bound; where both accept, tile 9's output equals tile 8's"""
    d = L.ConvDesc()
    d.N, d.Hi, d.Wi, d.C1, d.Ho, d.Wo, d.Cout = c['N'], 4, 4, c['C1'], 4, 4, c['Cout']
    d.KH = d.KW = 3
    d.sn, d.sd, d.pad, d.ldx, d.ldy = 1, 1, 1, c['C1'], c['Cout']
    d.x = d.w = d.y = d.w_hi = d.w_lo = d.w_frag = d.bias = 4096
    if c['pro']:
        d.pro_scale = d.pro_shift = 4096
        d.pro_per_row = int(c['pro'] == 2)
    d.pro_act = c['act']
    if c['addend']:
        d.addend, d.ldadd = 4096, c['Cout']
    if c['dact']:
        d.dact_x, d.lddact, d.dact_act = 4096, c['Cout'], c['dact']
    d.splits = c['splits']
    if c['splits'] > 1:
        d.ws = 4096
    fail, ys = [], {}
    for tile in (8, 9):
        d.tile = tile
        want = TILE_TABLE[tile].ok(d, d.splits)
        keep = []
        try:
            r, e, bad = check_conv(Conv(d, f'fuzz tile {tile}'), n=c['N'], seed=c['seed'], keep=keep)
        except L.GaError as ex:
            assert 'UNSUPPORTED' in str(ex), (tile, str(ex))
            if not ex.untouched:
                fail.append(f'tile {tile}: refused but wrote the output')
            if want:
                fail.append(f'tile {tile}: refused, the predicate says eligible')
            continue
        if not want:
            fail.append(f'tile {tile}: accepted, the predicate says ineligible')
        if r > 1.0 or bad:
            fail.append(f'tile {tile}: bound ratio {r:.3g} (max|err|/scale {e:.2e}) {bad}')
        ys[tile] = keep[0]
    if len(ys) == 2 and not torch.equal(ys[8].view(torch.int32), ys[9].view(torch.int32)):
        fail.append('tile 9 differs from tile 8')
    assert not fail, '\n'.join(fail)


def test_refused_request_leaves_the_output_untouched():
    """a refused tile request launches nothing: the output keeps its NaN fill"""
    c = _synthetic(11)
    c.f['Wo'] = c.f['Wi'] = 24                      # tile 11 needs Wo % 16 == 0
    for tile in (11, 8, 7):                         # the halo tiles need 128 % Wo == 0 or Wo % 128 == 0
        c.f['tile'] = tile
        with pytest.raises(L.GaError) as ex:
            run_conv(c, n=2)
        assert ex.value.untouched


def _rows_of_entry(key):
    """the row count N an entry was tuned at, from its key: M = N Ho Wo with Ho = Hi sd / sn for the 'same' and the transposed
    convs (None where that is no whole number: valid-padded and even-sized kernels)"""
    v = key[3:].split('_') if key.startswith('b3_') else key.split('_')
    M, sn, sd, Hi = int(v[0]), int(v[5]), int(v[6]), int(v[7])
    if (Hi * sd) % sn:
        return None
    ho = Hi * sd // sn
    return M // (ho * ho) if M % (ho * ho) == 0 else None


def test_tune_table_census(plan_convs, more_plan_convs):
    """Which entries of conv_tune_gfx950.json the listed plans reach, which of those a default run checks, which no listed plan
    reaches: printed per (tile, split-K yes / no, use_bf3).  An entry is REACHED when a conv of a plan looks its key up, AS NAMED
    when that conv then runs the entry's (tile, splits), CHECKED when a descriptor a default run replays runs it as named.
    Asserted: every (tile, split-K, use_bf3) combination some plan runs as named has a checked entry, and every conv that looked
    an entry up runs what engine_core.resolve_tile gives for the entry and that conv (in particular no entry with an explicit
    tile falls to the heuristic, tile 0, by another road).  Unreached entries are counted, with the row counts their keys imply."""
    cache = tune_cache()
    combo = lambda ent: (int(ent[0]), int(ent[1]) > 1, int(ent[2]) if len(ent) > 2 else 1)
    reached = {r.tkey for r in CENSUS}
    named = {r.tkey for r in CENSUS if r.as_named}
    checked = set().union(*(c.tkeys for c in _subset(plan_convs) + _subset(more_plan_convs)))
    assert checked <= named <= reached <= set(cache)
    count = {}
    for key, ent in cache.items():
        row = count.setdefault(combo(ent), [0, 0, 0, 0, 0])
        row[0] += 1
        row[1] += key in reached
        row[2] += key in named
        row[3] += key in checked
        row[4] += key not in reached
    print(f'\ntune table: {len(cache)} entries, {len(reached)} reached by the listed plans ({len(named)} run as named), {len(checked)} checked '
          f'by a default run, {len(cache) - len(reached)} reached by no listed plan', flush=True)
    print('  tile split-K bf3 | entries reached as-named checked unreached', flush=True)
    for k in sorted(count):
        print(f'  {k[0]:4d} {"yes" if k[1] else "no ":>7s} {k[2]:3d} | {count[k][0]:7d} {count[k][1]:7d} {count[k][2]:8d} {count[k][3]:7d} {count[k][4]:9d}',
              flush=True)
    by_rows = {}
    for key in cache:
        if key not in reached:
            n = _rows_of_entry(key)
            by_rows[n] = by_rows.get(n, 0) + 1
    print('  unreached entries by the row count of their key: '
          + ', '.join(f'{n if n is not None else "other"}: {v}' for n, v in sorted(by_rows.items(), key=lambda kv: (kv[0] is None, kv[0] or 0))),
          flush=True)
    demoted = [r for r in CENSUS if not r.as_named]
    seen = set()
    for r in demoted:
        if (r.tkey, r.ran) not in seen:
            seen.add((r.tkey, r.ran))
            print(f'  demoted: entry (tile {r.ent[0]}, splits {r.ent[1]}) -> (tile {r.ran[0]}, splits {r.ran[1]})  {r.label}  {r.where}', flush=True)
    blind = [k for k, v in sorted(count.items()) if v[2] and not v[3]]
    assert not blind, f'(tile, split-K, use_bf3) combinations a plan runs and no default descriptor checks: {blind}'
    wrong = [f'{r.where}: entry {r.ent} runs as {r.ran}, resolve_tile gives {r.want}  {r.label}' for r in CENSUS if r.ran != r.want]
    assert not wrong, '\n'.join(wrong[:40])
