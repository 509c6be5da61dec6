"""
Every non-conv, non-cell op of the shipped plans, as the engines configure it, against the float64 interpreter of
tests/planref.py: what tests/test_plan_convs_gpu.py is for the convolutions.

The engines are the three bench.py times, built by the same code (configs[1] NVAE + VGG at 1024 rows, the configs[2] e4e defender
at 32 rows, the configs[4] Style-Transformer defender at 64 rows, EoT 32, split-bf16), and the reduced engines of
planzoo.device_engines: the ND-VAE and A-VAE defenders, the K-cotangent engines (competitors, ResNet / ResNeXt with their noise
and blur fronts) and the alpha-table / alpha-gradient engines of the three defenders -- ga_avae, sampler modes 1 and 2, latent-mix
backward 2 and every replica field above 1 come from those.  Each distinct descriptor of their forward
and backward plans -- distinct by kind, every non-pointer field, which pointers are set, their offsets modulo 16 bytes, which
are equal and which are channel slices of one tensor -- runs on fresh buffers at the least row count its replica fields allow
(planref.Buffers: inputs drawn, everything the op must not read poisoned with 1e30, outputs and workspaces NaN, in / out
operands drawn and handed to the reference, one sentinel row behind every tensor), twice, and must
  - be accepted,
  - be finite and within tolerance on every element the header says is written; outputs marked exact must be equal,
  - leave every other float of every buffer with the bits it had (pad channels, sentinel rows, the inputs),
  - give the same bits on both launches,
  - have at most opref.KINK_CAP of an output's elements left out for a kinked derivative (from the reference alone).
Tolerance: opref.bound() = 4 x the error of the same formula in plain fp32 PyTorch on the same inputs, floor 2^-22 max |ref|;
ga_rowchan_reduce's fp32 yardstick adds in the order tests/test_ops_edges2_gpu.py uses (opref.reduce_order) and ga_modout's `red`
in the same two-stage order (planref.Modout.red_order), because PyTorch's pairwise sum beats a correct fixed-order one over 1024^2
pixels (fp32 CPU pairwise 1.2e-5, kernel 2.6e-3 there), and the fused ga_se_excite's pixel sum in its pixel-lane order
(planref.SeExcite.pixel_lanes; with the pairwise sum `hid` of a 768-pixel, Hd = 2 squeeze read 5.2e-8 against a bound of 3.6e-8,
the 2^-22 floor, with 0.15 the largest of its two elements); ga_attn's P V and
dS K in the kernel's key groups (opref.weighted_rows_in_groups); ga_sampler_mix mode 2 and ga_latent_mix backward 2 use the
element-wise unit-roundoff bounds of tests/test_alpha_grad_gpu.py.
The default run checks, per class (the identity without the extents), the member with the fewest and the one with the most
pixels; GA_TEST_ALL_PLAN_OPS=1 checks all.  One test per op kind.

test_bound_sees_a_misread_field hands the REFERENCE a wrong reading of one field for three ops and asserts that the bound fails.
"""
import gc
import os
import sys

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')]      # collects without one

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import opref as R                                                        # noqa: E402
import planref as PR                                                     # noqa: E402
import planzoo                                                           # noqa: E402
from gen_adversarial_amd import _lib as L                                # noqa: E402

DEV = 'cuda:0'
ALL = os.environ.get('GA_TEST_ALL_PLAN_OPS', '0') == '1'


def _collect(eng, plan_name, out, refused):
    for plan, tag in ((eng.fwd, 'fwd'), (eng.bwd, 'bwd')):
        for d, name in zip(plan.descs, plan.names):
            if isinstance(d, PR.ELSEWHERE):
                continue
            where = f'{plan_name}.{tag}.{name}'
            try:
                op = PR.capture(type(d).from_buffer_copy(d), where)
            except PR.PlanRefError as ex:
                refused.append(f'{where}: {ex}')
                continue
            if op.key in out:
                out[op.key].where.append(where)
            else:
                out[op.key] = op


@pytest.fixture(scope='module')
def plan_ops():
    """the distinct non-conv descriptors of the three shipped plans; the engines are built one at a time and freed"""
    from bench import build_e4e_defender, build_model, build_trans_defender
    builders = [('configs1_nvae', lambda: build_model(DEV, 1024, 32, seed=0, precision='bf16x3')[0]),
                ('configs2_e4e', lambda: build_e4e_defender(DEV, 32, 32, 'bf16x3')[0]),
                ('configs4_trans', lambda: build_trans_defender(DEV, 64, 32, 'bf16x3')[0])]
    builders += list(planzoo.device_engines(DEV))
    every, refused, per_plan = {}, [], {}
    for name, build in builders:
        eng = build()
        before = len(every)
        _collect(eng, name, every, refused)
        per_plan[name] = len(every) - before
        del eng
        gc.collect()
        torch.cuda.empty_cache()
    ops = list(every.values())
    pick = ops if ALL else _subset(ops)
    print(f'\nplan ops: new distinct descriptors per engine {per_plan}; {len(ops)} in all; checking {len(pick)} ({len(ops) - len(pick)} skipped'
          f'{"" if ALL else "; GA_TEST_ALL_PLAN_OPS=1 checks all"})', flush=True)
    return ops, pick, refused


def _subset(ops):
    by = {}
    for op in ops:
        by.setdefault(op.klass(), []).append(op)
    pick = []
    for k in sorted(by, key=repr):
        v = sorted(by[k], key=lambda o: (o.pixels(), repr(o.key)))
        pick.append(v[0])
        if len(v) > 1:
            pick.append(v[-1])
    return pick


def _yardstick(op, t32, ref=None):
    """the same formula in plain fp32; the long sums in the order the kernels' comments document"""
    if op.cls is L.ModoutDesc and 'red' in op.has and ref is None:
        S, lanes = op.h.red_order(op.f)
        r = op.h.ref(op.f, t32, op.has, total=lambda v: R.segment_sum(v, S, lanes))
        return {k: v for k, v in r.items() if k in op.has}
    if op.cls is L.SeExciteDesc and 't' in op.has and ref is None:
        lanes = op.h.pixel_lanes(op.f)
        r = op.h.ref(op.f, t32, op.has, total=lambda v: R.lane_sum(v, lanes, False))
        return {k: v for k, v in r.items() if k in op.has}
    if op.cls is L.ReduceDesc and ref is None:
        f = op.f
        S, lanes = R.reduce_order(f['N'], f['P'], f['C'], f['ws_floats'] if 'ws' in op.has else 0)
        r = op.h.ref(f, t32, op.has, total=R.order_sum(S, lanes))
        return {k: v for k, v in r.items() if k in op.has}
    return (ref or PR.reference)(op, t32)


def check_op(op, seed=None, ref=None):
    """-> ([(output, fp32 err, bound, kernel err)], [failure messages]); `ref` replaces planref.reference (sensitivity test)"""
    buf = PR.Buffers(op, DEV, PR.seed_of(op) if seed is None else seed)
    d = op.desc(buf.pointers())
    t64, t32 = buf.inputs(torch.float64), buf.inputs(torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for i in range(2):
        if i:
            buf.reset()
        L.run(d, stream)
        torch.cuda.synchronize()
        outs.append({n: buf.view[n].detach().cpu() for n in buf.view if buf.role[n] in ('out', 'inout')})
    bad = [f'wrote outside its outputs: {g}' for g in buf.untouched()]
    for n in outs[0]:
        if not torch.equal(outs[0][n].view(torch.int32), outs[1][n].view(torch.int32)):
            bad.append(f'{n}: two launches differ')
    r64, r32 = (ref or PR.reference)(op, t64), _yardstick(op, t32, ref)
    figures = []
    for n, res in r64.items():
        got, want, skip = outs[0][n].double(), res.value.double(), res.skip
        if skip is not None and res.tol is None:
            share = skip.double().mean().item()
            if share > R.KINK_CAP:
                bad.append(f'{n}: {share:.2e} of the elements sit on a kink')
        keep = torch.ones_like(want, dtype=torch.bool) if skip is None else ~skip.expand_as(want)
        if not bool(keep.any()):
            bad.append(f'{n}: every element is left out')
            continue
        if not torch.isfinite(got[keep]).all():
            bad.append(f'{n}: not every element was written')
            continue
        if res.tol is not None:                                   # element-wise unit-roundoff bound; the rest of the table untouched
            err = (got - want).abs()
            ratio = (err[keep] / res.tol.expand_as(want)[keep].clamp_min(1e-300)).max().item()
            figures.append((n, float('nan'), 1.0, ratio))
            if ratio > 1.0:
                bad.append(f'{n}: err / (c u sum|term|) = {ratio:.3f}')
            if skip is not None and not torch.isnan(got[~keep]).all():
                bad.append(f'{n}: wrote outside its column')
            continue
        if res.exact:
            w32 = want.float()
            if not torch.equal(outs[0][n][keep], w32[keep]):
                bad.append(f'{n}: {int((outs[0][n][keep] != w32[keep]).sum())} elements differ from the reference rounded to fp32')
            figures.append((n, 0.0, 0.0, R.max_err(outs[0][n][keep], want[keep])))
            continue
        y32 = r32[n].value
        b, cpu, err = R.bound(y32[keep], want[keep]), R.max_err(y32[keep], want[keep]), R.max_err(got[keep], want[keep])
        figures.append((n, cpu, b, err))
        if err > b:
            bad.append(f'{n}: kernel err {err:.3e} > bound {b:.3e} (fp32 CPU {cpu:.3e}, ref max {want.abs().max().item():.3e})')
    return figures, bad


def test_no_plan_descriptor_is_refused_by_the_interpreter(plan_ops):
    ops, pick, refused = plan_ops
    assert not refused, 'descriptors planref refuses:\n' + '\n'.join(refused[:40])
    assert {op.cls for op in ops} == set(PR.HANDLERS), sorted(c.__name__ for c in set(PR.HANDLERS) - {op.cls for op in ops})


KINDS = sorted(c.__name__ for c in PR.HANDLERS)


@pytest.mark.parametrize('kind', KINDS)
def test_plan_op_descriptors(plan_ops, kind):
    """Worst kernel err / bound per kind over all 893 distinct descriptors (GA_TEST_ALL_PLAN_OPS=1), as measured: Attn 0.30, Avae 0.70,
    AvgpoolAct 0.34, Axpby 0.20, BilinearBwd 0.28, Blur 0.25, Dml 0.29, Dw 0.35, Gconv 0.64, ImageIo 0.39, Interleave2 0.31,
    LatentMix 0.25, Layernorm 0.25, Maxpool3s2 0.25, Maxpool exact, Modout 0.44, Pixelnorm 0.34, PoolDenorm 0.38, Prelu 0.21, Reduce
    0.33, RepSum 0.25, Resize2Crop 0.55, Sampler 0.60, SeApply 0.29, SeExcite 0.80 (with the pixel-lane yardstick of the module
    docstring), Unary 0.25, Up2Blur 0.34."""
    ops, pick, _ = plan_ops
    mine = [op for op in pick if op.cls.__name__ == kind]
    fails, worst = [], 0.0
    for op in mine:
        small = op.with_rows()
        try:
            figures, bad = check_op(small)
        except L.GaError as ex:
            fails.append(f'{op.label()} ({op.where[0]}): {ex}')
            continue
        txt = ', '.join(f'{n} {c:.1e} / {b:.1e} / {e:.1e}' for n, c, b, e in figures)
        print(f'  {small.label()[:150]:150s} fp32 err / bound / kernel err: {txt}  {op.where[0]}', flush=True)
        worst = max([worst] + [e / b for n, c, b, e in figures if b > 0])
        if bad:
            fails.append(f'{small.label()} ({op.where[0]}): ' + '; '.join(bad))
    print(f'{kind}: checked {len(mine)} of {sum(o.cls.__name__ == kind for o in ops)} distinct descriptors, worst kernel err / bound {worst:.3f}',
          flush=True)
    assert mine, f'no plan holds a {kind}'
    assert not fails, '\n'.join(fails)


def _synthetic(cls, f, ptr):
    return PR.capture(PR.make_desc(cls, f, ptr), 'synthetic')


def test_bound_sees_a_misread_field():
    """the reference is handed a wrong reading of one field -- ga_modout backward with `red`: ld_planes = C instead of 4C (the planes
    are then read as four dense tensors); ga_rowchan_reduce with gate / skip: skip ignored; ga_layernorm backward: accumulate
    ignored -- and the bound must fail; with the right reading the same inputs pass"""
    N, H, W, C = 2, 8, 8, 8
    ptr = dict(scale=4096, add=8192, dout=1 << 16, red=1 << 18, ws=1 << 19)
    ptr.update({f't_planes{i}': (1 << 20) + 4 * C * i for i in range(4)})
    ptr.update({f'dt_planes{i}': (1 << 22) + 4 * C * i for i in range(4)})
    modout = _synthetic(L.ModoutDesc, dict(N=N, P=H * W, C=C, act=5, backward=1, W=W, ld_planes=4 * C, ws_floats=4 * N * C), ptr)
    reduce_ = _synthetic(L.ReduceDesc, dict(N=2, P=40, C=16, scale=1.0),
                         dict(a=1 << 13, b=1 << 14, out=1 << 16, gate=1 << 17, skip=1 << 20, scaled=1 << 20))
    ln = _synthetic(L.LayernormDesc, dict(rows=6, C=64, eps=1e-5, backward=1, accumulate=1),
                    dict(a=4096, b=8192, gamma=1 << 14, stats=1 << 15, dy=1 << 16, dx=1 << 17))

    def modout_dense_planes(op, t):
        # ld_planes read as C: plane i is then the i-th quarter of the flat [N, H/2, W/2, 4C] tensor
        whole = torch.stack([t[f't_planes{i}'] for i in range(4)], dim=3)                       # [N, h, w, 4, C] as it lies in memory
        flat = whole.reshape(4, N, H // 2, W // 2, C)
        t2 = dict(t, **{f't_planes{i}': flat[i] for i in range(4)})
        return PR.reference(op, t2)

    def reduce_no_skip(op, t):
        r = op.h.ref(op.f, {k: v for k, v in t.items() if k != 'skip'}, op.has - {'skip'})
        return {k: v for k, v in r.items() if k in op.has}

    def ln_no_accumulate(op, t):
        return op.h.ref(op.f, t, op.has, accumulate=0)

    msgs = []
    for what, op, wrong in (('modout ld_planes', modout, modout_dense_planes), ('reduce skip', reduce_, reduce_no_skip), ('layernorm accumulate', ln, ln_no_accumulate)):
        fig_ok, bad_ok = check_op(op, seed=7)
        fig_wr, bad_wr = check_op(op, seed=7, ref=wrong)
        print(f'  {what}: right reading {[f"{n} {e:.1e}/{b:.1e}" for n, _, b, e in fig_ok]}, wrong reading {[f"{n} {e:.1e}/{b:.1e}" for n, _, b, e in fig_wr]}')
        if bad_ok:
            msgs.append(f'{what}: fails with the right reading: {bad_ok}')
        if not any('kernel err' in m for m in bad_wr):
            msgs.append(f'{what}: the bound does not see the wrong reading')
    assert not msgs, '\n'.join(msgs)
