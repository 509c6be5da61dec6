"""
Float64 interpreter of the NON-CONV descriptors of include/ga_ops.h, as the engines compose them in their plans: what
convref.conv_ref(d, t) is for ga_conv_desc.  One handler per descriptor type, written from the header's comments and
delegating the arithmetic to tests/opref.py.  No GPU, no library call: the handlers see tensors, not pointers.

A handler declares
  reads(f)    the non-pointer fields it interprets in this mode.  Any other field must be zero / NULL or `capture` refuses
              the descriptor (PlanRefError): a field an engine starts to use shows up as a refusal, not as a silent pass.
              unread(f) names the fields the header says are NOT read in this mode (they may hold anything);
  rows        the field that counts rows, and reps(f, has): the replica fields in use -- the least legal row count is their
              lcm (least_rows), the runner shrinks rows to it;
  operands(f, has)   name -> Operand(lead, ld, used, role): the extent of every pointer operand in the library's memory
              layout, from the integer fields alone: [*lead, ld] floats, channels [0, used) of every pixel belong to the op;
  ref(f, t, has)     t: name -> dense [*lead, used] tensor (float64 for the reference, float32 for "the same formula in
              plain fp32", opref.bound's yardstick) -> name -> Res(value, exact, skip, tol) for every output the header says
              the op writes in this mode.  exact: selections and copies, compared with the float64 result rounded once to
              fp32.  skip: elements whose derivative sits on a kink (opref.near_kink).  tol: an element-wise bound that
              replaces opref.bound (the unit-roundoff bounds of tests/test_alpha_grad_gpu.py).

`capture(desc)` turns a ctypes descriptor into a PlanOp: its identity (every non-pointer field, which pointers are set,
each pointer's offset modulo 16 bytes, which pointers are equal, which are channel slices of one tensor) and its class
(the identity without the extents).  `Buffers` lays a PlanOp's operands out in memory on any device -- pitched, sliced,
aliased, poisoned (1e30) wherever the op must not read, NaN wherever it must write, one sentinel row behind every tensor --
for the GPU runner (tests/test_plan_ops_gpu.py) and for the CPU check of the interpreter itself (tests/test_planref_cpu.py).
"""
import math

import torch

import opref as R
from gen_adversarial_amd import _lib as L

POISON = 1e30
KINKED = (R.RELU, R.LRELU, R.FLRELU)
U = 2.0 ** -24


class PlanRefError(Exception):
    pass


class Operand:
    """[*lead, ld] floats; channels [0, used) of every pixel are the op's.  role: in | out | inout | ws.  draw: n = normal,
    pos = positive (stats, gate, taps, alpha), u01 = uniform [0, 1) images"""

    def __init__(self, lead, ld, used=None, role='in', draw='n'):
        self.lead, self.ld, self.used, self.role, self.draw = tuple(int(v) for v in lead), int(ld), int(ld if used is None else used), role, draw
        if self.used > self.ld or min(self.lead + (self.ld, self.used)) <= 0:
            raise PlanRefError(f'extent [{self.lead}, {self.ld}] with {self.used} channels used')

    @property
    def shape(self):
        return self.lead + (self.used,)


def In(lead, ld, used=None, draw='n'):
    return Operand(lead, ld, used, 'in', draw)


def Out(lead, ld, used=None):
    return Operand(lead, ld, used, 'out')


class Res:
    def __init__(self, value, exact=False, skip=None, tol=None):
        self.value, self.exact, self.skip, self.tol = value, exact, skip, tol


def _div(n, k, what):
    k = max(int(k), 1)
    if n % k:
        raise PlanRefError(f'{what}: {n} rows are no multiple of {k}')
    return n // k


def _kink(u, act, rep=1):
    return R.rep_rows(R.near_kink(u.double()), rep) if act in KINKED else None


class Handler:
    rows = 'N'
    extents = ()                # the fields left out of a descriptor's class

    def reads(self, f):
        raise NotImplementedError

    def unread(self, f):
        return set()

    def reps(self, f, has):
        return []

    def least_rows(self, f, has):
        return math.lcm(1, *[max(int(r), 1) for r in self.reps(f, has)])


# ---------------------------------------------------------------------------------------------------- handlers
class Dw(Handler):
    extents = ('N', 'H', 'W', 'C')

    def reads(self, f):
        return {'N', 'H', 'W', 'C', 'pro_act', 'dact_act', 'up2', 'pool2', 'act_rep'}

    def reps(self, f, has):
        return [f['act_rep']] if 'dact_x' in has else []

    def operands(self, f, has):
        N, H, W, C = f['N'], f['H'], f['W'], f['C']
        hs, ws = (H // 2, W // 2) if f['up2'] else (H, W)
        ho, wo = (H // 2, W // 2) if f['pool2'] else (H, W)
        return dict(x=In((N, hs, ws), C), w=In((25,), C), bias=In((), C), dact_x=In((_div(N, f['act_rep'], 'act_rep'), ho, wo), C),
                    y=Out((N, ho, wo), C))

    def ref(self, f, t, has):
        u = t.get('dact_x')
        y = R.dwconv5(t['x'], t['w'], t.get('bias'), u, f['pro_act'], f['dact_act'], bool(f['up2']), bool(f['pool2']), max(f['act_rep'], 1))
        return dict(y=Res(y, skip=None if u is None else _kink(u, f['dact_act'], max(f['act_rep'], 1))))


class Reduce(Handler):
    extents = ('N', 'P', 'C', 'ws_floats')

    def reads(self, f):
        return {'N', 'P', 'C', 'scale', 'ws_floats'}

    def operands(self, f, has):
        N, P, C = f['N'], f['P'], f['C']
        o = dict(a=In((N, P), C), b=In((N, P), C), out=Out((N,), C), gate=In((N,), C, draw='pos'), skip=In((N, P), C),
                 scaled=Out((N, P), C), a_src=In((N, P), 4), a_w=In((C,), 4))
        if 'ws' in has:
            if f['ws_floats'] < 2 * N * C:
                raise PlanRefError('ws_floats < 2 N C')
            o['ws'] = Operand((f['ws_floats'] // C,), C, role='ws')
        if ('a' in has) == ('a_src' in has) or ('a_src' in has) != ('a_w' in has) or ('gate' in has) != ('scaled' in has):
            raise PlanRefError('a xor (a_src, a_w); gate with scaled')
        return o

    def ref(self, f, t, has, total=R.pixel_sum):
        out, scaled = R.rowchan_reduce(t.get('a'), t.get('b'), f['scale'], t.get('gate'), t.get('skip'), t.get('a_src'), t.get('a_w'), total=total)
        r = dict(out=Res(out))
        if scaled is not None:
            r['scaled'] = Res(scaled)
        return r


class SeApply(Handler):
    extents = ('N', 'H', 'W', 'C')

    def reads(self, f):
        return {'N', 'H', 'W', 'C', 'skip_mode', 'res_scale'}

    def operands(self, f, has):
        N, H, W, C, m = f['N'], f['H'], f['W'], f['C'], f['skip_mode']
        sk = {0: (N, H, W), 1: (N, H // 2, W // 2), 2: (N, 2 * H, 2 * W)}[m]
        return dict(skip=In(sk, C), t=In((N, H, W), C), gate=In((N,), C, draw='pos'), out=Out((N, H, W), C))

    def ref(self, f, t, has):
        return dict(out=Res(R.se_apply(t.get('skip'), t['t'], t['gate'], f['res_scale'], f['skip_mode'])))


class SeExcite(Handler):
    extents = ('N', 'P', 'C', 'Hd')

    def reads(self, f):
        return {'N', 'C', 'Hd', 'P', 'res_scale', 'backward', 'act_rep'}

    def reps(self, f, has):
        return [f['act_rep']] if f['backward'] else []

    def operands(self, f, has):
        N, C, Hd, P = f['N'], f['C'], f['Hd'], f['P']
        if 't' not in has:                   # the unfused form: m / dgate given, no pixel pass, no replicas
            if f['act_rep'] > 1 or 'out' in has or 'skip' in has or 'dout' in has:
                raise PlanRefError('act_rep, out, skip and dout belong to the fused form (t given)')
            o = dict(w1=In((Hd,), C), b1=In((), Hd), w2=In((C,), Hd), b2=In((), C))
            if f['backward']:
                o.update(hid=In((N,), Hd), gate=In((N,), C, draw='pos'), dgate=In((N,), C), pro_scale=Out((N,), C), pro_shift=Out((N,), C))
            else:
                o.update(m=In((N,), C), hid=Out((N,), Hd), gate=Out((N,), C))
            return o
        if f['act_rep'] > 1 and not f['backward']:
            raise PlanRefError('act_rep on a forward launch')
        Nf = _div(N, f['act_rep'], 'act_rep') if f['backward'] else N
        o = dict(t=In((Nf, P), C), w1=In((Hd,), C), b1=In((), Hd), w2=In((C,), Hd), b2=In((), C))
        if f['backward']:
            o.update(hid=In((Nf,), Hd), gate=In((Nf,), C, draw='pos'), dout=In((N, P), C), pro_scale=Out((N,), C), pro_shift=Out((N,), C))
        else:
            o.update(hid=Out((N,), Hd), gate=Out((N,), C), skip=In((N, P), C), out=Out((N, P), C))
        return o

    @staticmethod
    def pixel_lanes(f):
        """the fused form's pixel sum as the kernel's comment gives it: C / 4 channel-quad lanes x 256 / (C / 4) pixel lanes, lane l
        adds pixels l, l + lanes, ... one after the other, then the lanes are added in lane order (opref.lane_sum)"""
        return max(256 // max(f['C'] // 4, 1), 1)

    def ref(self, f, t, has, total=R.pixel_sum):
        if 't' not in has:
            if not f['backward']:
                hid, gate = R.se_excite_fwd(t['m'], t['w1'], t['b1'], t['w2'], t['b2'])
                return dict(hid=Res(hid), gate=Res(gate))
            ps, pb = R.se_excite_bwd(t['dgate'], t['hid'], t['gate'], t['w1'], t['w2'], f['res_scale'], f['P'])
            return dict(pro_scale=Res(ps), pro_shift=Res(pb, skip=R.near_kink(t['hid'].double()).any(dim=-1, keepdim=True).expand(-1, f['C'])))
        if f['backward']:
            K = max(f['act_rep'], 1)
            dgate = f['res_scale'] * total(t['dout'] * R.rep_rows(t['t'], K))
            ps, pb = R.se_excite_bwd(dgate, R.rep_rows(t['hid'], K), R.rep_rows(t['gate'], K), t['w1'], t['w2'], f['res_scale'], f['P'])
            return dict(pro_scale=Res(ps), pro_shift=Res(pb, skip=R.rep_rows(R.near_kink(t['hid'].double()).any(dim=-1, keepdim=True).expand(-1, f['C']), K)))
        hid, gate = R.se_excite_fwd(total(t['t']) / f['P'], t['w1'], t['b1'], t['w2'], t['b2'])
        r = dict(hid=Res(hid), gate=Res(gate))
        if 'out' in has:
            N, P, C = t['t'].shape
            sk = t.get('skip')
            r['out'] = Res(R.se_apply(None if sk is None else sk.view(N, P, 1, C), t['t'].view(N, P, 1, C), gate, f['res_scale']).view(N, P, C))
        return r


class BilinearBwd(Handler):
    extents = ('N', 'h', 'w', 'C')

    def reads(self, f):
        return {'N', 'h', 'w', 'C', 'accumulate'}

    def operands(self, f, has):
        N, h, w, C = f['N'], f['h'], f['w'], f['C']
        return dict(dhigh=In((N, 2 * h, 2 * w), C), dlow=Operand((N, h, w), C, role='inout' if f['accumulate'] else 'out'))

    def ref(self, f, t, has):
        g = R.bilinear_up2_adjoint(t['dhigh'])
        return dict(dlow=Res(t['dlow'] + g if f['accumulate'] else g))


class Sampler(Handler):
    extents = ('N', 'h', 'w')

    def reads(self, f):
        base = {'N', 'h', 'w', 'NL', 'ldq', 'ldp', 'eps_nchw', 'backward', 'mode', 'ldz'}
        if f['mode'] == 0:
            return base | {'alpha', 'one_minus_alpha', 'temp', 'q_rep', 'act_rep', 'alpha_ld', 'alpha_col'}
        if f['mode'] == 1:
            return base | {'act_rep'}
        return base | {'temp', 'q_rep', 'alpha_ld', 'alpha_col', 'act_rep'}

    def unread(self, f):
        return {1: {'alpha', 'one_minus_alpha', 'temp', 'q_rep'}, 2: {'alpha', 'one_minus_alpha'}}.get(f['mode'], set())

    def reps(self, f, has):
        K = max(f['act_rep'], 1) if f['backward'] else 1
        return [K * (max(f['q_rep'], 1) if f['mode'] != 1 else 1)]

    def operands(self, f, has):
        N, h, w, NL, mode = f['N'], f['h'], f['w'], f['NL'], f['mode']
        K = max(f['act_rep'], 1)
        if K > 1 and (not f['backward'] or mode == 2):
            raise PlanRefError('act_rep on a forward or mode-2 launch')
        Nf = _div(N, K, 'act_rep')
        q = max(f['q_rep'], 1) if mode != 1 else 1
        Nq = _div(Nf, q, 'q_rep')
        ldz = f['ldz'] or NL
        wide = 2 * NL if mode == 1 else NL
        if f['ldq'] < wide or ('p' in has and f['ldp'] < 2 * NL) or ldz < NL:
            raise PlanRefError('a pitch below the channel count')
        eps = In((Nf, NL, h), w) if f['eps_nchw'] else In((Nf, h, w), NL)
        o = dict(mu_q=In((Nq, h, w), f['ldq'], wide), eps=eps)
        if 'p' in has:
            o['p'] = In((Nf, h, w), f['ldp'], 2 * NL)
        if mode == 2:
            if not f['backward'] or not 0 <= f['alpha_col'] < f['alpha_ld']:
                raise PlanRefError('mode 2: backward = 1, 0 <= alpha_col < alpha_ld')
            o.update(dz=In((N, h, w), ldz, NL), z=Operand((N, f['alpha_ld']), 1, role='out'))
            return o
        if 'alpha_rows' in has:
            if mode != 0 or f['alpha_ld'] < 2 * f['alpha_col'] + 2:
                raise PlanRefError('alpha_rows: mode 0, alpha_ld >= 2 alpha_col + 2')
            o['alpha_rows'] = In((Nf,), f['alpha_ld'], draw='pos')
        if not f['backward']:
            o['z'] = Out((N, h, w), ldz, NL)
            return o
        o['dz'] = In((N, h, w), ldz, NL)
        if mode == 1:
            o.update(dmu_q=Out((N, h, w), f['ldq'], 2 * NL), dp=Out((N, h, w), f['ldp'], 2 * NL))
        else:
            o.update(dmu_q=Out((N, h, w), f['ldq'], NL), dmu_q_rows=Out((N, h, w), f['ldq'], NL))
            if 'p' in has:
                o['dp'] = Out((N, h, w), f['ldp'], 2 * NL)
            if ('dmu_q_rows' in has) != (q > 1) or ('dmu_q' in has) == (q > 1):
                raise PlanRefError('q_rep > 1 writes dmu_q_rows, else dmu_q')
        return o

    def _parts(self, f, t, has):
        """row-expanded mode-0 quantities: enc_mu, dec_mu, sigma, eps (NHWC), and the tanh arguments"""
        NL = f['NL']
        K = max(f['act_rep'], 1) if f['backward'] else 1
        mq = R.rep_rows(R.rep_rows(t['mu_q'], max(f['q_rep'], 1)), K)
        eps = R.rep_rows(t['eps'].permute(0, 2, 3, 1) if f['eps_nchw'] else t['eps'], K)
        if 'p' in has:
            p = R.rep_rows(t['p'], K)
            mp, ls = p[..., :NL], p[..., NL:]
        else:
            mp, ls = torch.zeros_like(mq), torch.zeros_like(mq)
        return mq, mp, ls, eps

    def _alphas(self, f, t, has, K):
        if 'alpha_rows' in has:
            tab = R.rep_rows(t['alpha_rows'], K)
            c = 2 * f['alpha_col']
            return tab[:, c].view(-1, 1, 1, 1), tab[:, c + 1].view(-1, 1, 1, 1)
        return f['alpha'], f['one_minus_alpha']

    def ref(self, f, t, has):
        NL, mode = f['NL'], f['mode']
        K = max(f['act_rep'], 1) if f['backward'] else 1
        if mode == 1:
            eps = t['eps'].permute(0, 2, 3, 1) if f['eps_nchw'] else t['eps']
            if not f['backward']:
                return dict(z=Res(R.sampler_nd(t['mu_q'], t['p'], eps)))
            g = R.sampler_nd_bwd(t['mu_q'], t['p'], eps, t['dz'], K)
            return dict(dmu_q=Res(g), dp=Res(g))
        mq, mp, ls, eps = self._parts(f, t, has)
        if mode == 2:
            term = R.sampler_alpha_terms(mq, mp, ls, eps, t['dz'], f['temp']).flatten(1)
            T = term.shape[1]
            c = R.sampler_alpha_c(T)
            col = torch.zeros(term.shape[0], f['alpha_ld'], dtype=torch.bool)
            col[:, f['alpha_col']] = True
            full = torch.zeros(term.shape[0], f['alpha_ld'], dtype=term.dtype)
            full[:, f['alpha_col']] = term.sum(dim=1)
            tol = torch.zeros_like(full, dtype=torch.float64)
            tol[:, f['alpha_col']] = c * U * term.double().abs().sum(dim=1)
            return dict(z=Res(full.unsqueeze(-1), tol=tol.unsqueeze(-1), skip=~col.unsqueeze(-1)))
        a, b = self._alphas(f, t, has, K)
        if not f['backward']:
            return dict(z=Res(R.sampler_mix(mq, mp if 'p' in has else None, ls, eps, a, b, f['temp'])))
        dmu, dmp, dls = R.sampler_mix_bwd(mq, mp, ls, eps, t['dz'], a, b, f['temp'])
        r = {('dmu_q_rows' if max(f['q_rep'], 1) > 1 else 'dmu_q'): Res(dmu)}
        if 'p' in has:
            r['dp'] = Res(torch.cat([dmp, dls], dim=-1))
        return r


class Maxpool(Handler):
    extents = ('N', 'H', 'W', 'C')

    def reads(self, f):
        return {'N', 'H', 'W', 'C', 'backward', 'act_rep'}

    def reps(self, f, has):
        return [f['act_rep']] if f['backward'] else []

    def operands(self, f, has):
        N, H, W, C = f['N'], f['H'], f['W'], f['C']
        if not f['backward']:
            return dict(x=In((N, H, W), C), y=Out((N, H // 2, W // 2), C))
        return dict(x=In((_div(N, f['act_rep'], 'act_rep'), H, W), C), dy=In((N, H // 2, W // 2), C), dx=Out((N, H, W), C))

    def ref(self, f, t, has):
        if not f['backward']:
            return dict(y=Res(R.maxpool2(t['x']), exact=True))
        K = max(f['act_rep'], 1)
        gap = R.maxpool2_gap(t['x'].double())
        tie = gap <= R.KINK_REL * t['x'].abs().max().double()
        skip = R.rep_rows(tie.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2), K)
        return dict(dx=Res(R.maxpool2_bwd(t['x'], t['dy'], K), exact=True, skip=skip))


class AvgpoolAct(Handler):
    extents = ('N', 'P', 'C')

    def reads(self, f):
        return {'N', 'P', 'C', 'act', 'backward', 'act_rep'}

    def reps(self, f, has):
        return [f['act_rep']] if f['backward'] else []

    def operands(self, f, has):
        N, P, C = f['N'], f['P'], f['C']
        if not f['backward']:
            return dict(x=In((N, P), C), y=Out((N,), C))
        return dict(x=In((_div(N, f['act_rep'], 'act_rep'), P), C), dy=In((N,), C), dx=Out((N, P), C))

    def ref(self, f, t, has):
        if not f['backward']:
            return dict(y=Res(R.avgpool_act(t['x'], f['act'])))
        K = max(f['act_rep'], 1)
        return dict(dx=Res(R.avgpool_act_bwd(t['x'], f['act'], t['dy'], K), skip=_kink(t['x'], f['act'], K)))


class Axpby(Handler):
    rows = None
    extents = ('n',)

    def reads(self, f):
        return {'n', 'alpha', 'beta'}

    def operands(self, f, has):
        return dict(x=In((), f['n']), y=Operand((), f['n'], role='inout' if f['beta'] else 'out'))

    def ref(self, f, t, has):
        return dict(y=Res(R.axpby(t['x'], t['y'], f['alpha'], f['beta']) if f['beta'] else f['alpha'] * t['x']))


class RepSum(Handler):
    rows = 'rows'
    extents = ('rows', 'inner')

    def reads(self, f):
        return {'rows', 'inner', 'rep', 'accumulate'}

    def reps(self, f, has):
        return [f['rep']]

    def operands(self, f, has):
        return dict(x=In((f['rows'],), f['inner']), y=Operand((_div(f['rows'], f['rep'], 'rep'),), f['inner'], role='inout' if f['accumulate'] else 'out'))

    def ref(self, f, t, has):
        s = R.rep_sum(t['x'], max(f['rep'], 1))
        return dict(y=Res(t['y'] + s if f['accumulate'] else s))


class Pixelnorm(Handler):
    rows = 'rows'
    extents = ('rows',)

    def reads(self, f):
        return {'rows', 'C'}

    def operands(self, f, has):
        return dict(x=In((f['rows'],), f['C']), y=Out((f['rows'],), f['C']))

    def ref(self, f, t, has):
        return dict(y=Res(R.pixelnorm(t['x'])))


class Prelu(Handler):
    rows = 'rows'
    extents = ('rows',)

    def reads(self, f):
        return {'rows', 'C', 'backward'}

    def operands(self, f, has):
        n, C = f['rows'], f['C']
        o = dict(x=In((n,), C), slope=In((), C))
        o.update(dict(dy=In((n,), C), dx=Out((n,), C)) if f['backward'] else dict(y=Out((n,), C)))
        return o

    def ref(self, f, t, has):
        if f['backward']:
            return dict(dx=Res(R.prelu_bwd(t['x'], t['slope'], t['dy']), skip=R.near_kink(t['x'].double())))
        return dict(y=Res(R.prelu(t['x'], t['slope'])))


class Unary(Handler):
    rows = None
    extents = ('n',)

    def reads(self, f):
        return {'n', 'mode'} | ({'eps'} if f['mode'] == 2 else set())

    def operands(self, f, has):
        if ('g' in has) != (f['mode'] in (1, 3)):
            raise PlanRefError('g is read by modes 1 and 3 only')
        return dict(x=In((), f['n'], draw='pos' if f['mode'] in (2, 3) else 'n'), g=In((), f['n']), y=Out((), f['n']))

    def ref(self, f, t, has):
        return dict(y=Res(R.unary(t['x'], t.get('g'), f['mode'], f['eps'])))


class Modout(Handler):
    extents = ('N', 'P', 'C', 'W', 'ld_planes', 'ws_floats')

    def reads(self, f):
        return {'N', 'P', 'C', 'act', 'backward', 'W', 'ld_planes', 'ws_floats'}

    def operands(self, f, has, ld_planes=None):
        N, P, C = f['N'], f['P'], f['C']
        ldp = (f['ld_planes'] or C) if ld_planes is None else ld_planes
        tp, dp = [f't_planes{i}' for i in range(4)], [f'dt_planes{i}' for i in range(4)]
        for grp in (tp, dp):
            if 0 < sum(k in has for k in grp) < 4:
                raise PlanRefError('the four planes come together')
        planes = tp[0] in has or dp[0] in has
        if planes and (f['W'] <= 0 or P % f['W'] or f['W'] % 2 or (P // f['W']) % 2 or ldp < C):
            raise PlanRefError('planes need W | P, even H and W, ld_planes >= C')
        if (tp[0] in has) == ('t' in has):
            raise PlanRefError('t xor t_planes')
        o = dict(t=In((N, P), C), scale=In((N,), C, draw='pos'), add=In((P,), C))
        if planes:
            lead = (N, P // f['W'] // 2, f['W'] // 2)
            o.update({k: In(lead, ldp, C) for k in tp})
            o.update({k: Out(lead, ldp, C) for k in dp})
        if f['backward']:
            o.update(dout=In((N, P), C), dt=Out((N, P), C), red=Out((N,), C))
            if 'red' in has:
                if f['ws_floats'] < N * C or 'ws' not in has:
                    raise PlanRefError('red needs ws, ws_floats >= N C')
                o['ws'] = Operand((f['ws_floats'] // C,), C, role='ws')
        else:
            o['out'] = Out((N, P), C)
        return o

    @staticmethod
    def _from_planes(pl, W):
        """four [N, H/2, W/2, C] planes, index (h&1)*2 + (w&1) -> [N, H*W, C]"""
        N, h2, w2, C = pl[0].shape
        full = torch.zeros(N, 2 * h2, 2 * w2, C, dtype=pl[0].dtype)
        for i in range(4):
            full[:, i // 2::2, i % 2::2] = pl[i]
        return full.reshape(N, -1, C)

    @staticmethod
    def red_order(f):
        """(segments S, pixel lanes) of the fused `red` reduction as the kernel's comment gives it (the layout of ga_rowchan_reduce's
        two-stage pass, partial sums through ws added in segment order): S = ws_floats / (N C), at most ~2048 workgroups and at
        least 256 pixels per segment; ql = the power of two >= min(16, C / 4) channel-quad lanes x 256 / ql pixel lanes"""
        nchunks = (f['C'] + 63) // 64
        S = max(1, min(f['ws_floats'] // (f['N'] * f['C']), -(-2048 // (f['N'] * nchunks)), (f['P'] + 255) // 256))
        ql = 1
        while ql < min(16, f['C'] // 4):
            ql *= 2
        return S, 256 // ql

    def ref(self, f, t, has, total=R.pixel_sum):
        tt = t['t'] if 't' in has else self._from_planes([t[f't_planes{i}'] for i in range(4)], f['W'])
        if not f['backward']:
            return dict(out=Res(R.modout(tt, t.get('scale'), t.get('add'), f['act'])))
        dt, red = R.modout_bwd(tt, t.get('scale'), t.get('add'), f['act'], t['dout'])
        u = R.modout_u(tt, t.get('scale'), t.get('add'))
        skip = _kink(u, f['act'])
        r = {}
        if 'dt' in has:
            r['dt'] = Res(dt, skip=skip)
        if 'dt_planes0' in has:
            N, P, C = dt.shape
            v = dt.view(N, P // f['W'], f['W'], C)
            sk = None if skip is None else skip.view(N, P // f['W'], f['W'], C)
            for i in range(4):
                r[f'dt_planes{i}'] = Res(v[:, i // 2::2, i % 2::2], skip=None if sk is None else sk[:, i // 2::2, i % 2::2])
        if 'red' in has:
            red = total(dt * tt)
            r['red'] = Res(red)
        return r


class Up2Blur(Handler):
    extents = ('N', 'H', 'W', 'C')

    def reads(self, f):
        return {'N', 'H', 'W', 'C', 'backward'}

    def operands(self, f, has):
        N, H, W, C = f['N'], f['H'], f['W'], f['C']
        if f['backward']:
            return dict(hi_in=In((N, 2 * H, 2 * W), C), lo=Out((N, H, W), C))
        return dict(lo_in=In((N, H, W), C), hi=Operand((N, 2 * H, 2 * W), C, role='inout'))

    def ref(self, f, t, has):
        if not f['backward']:
            return dict(hi=Res(t['hi'] + R.up2_blur(t['lo_in'])))
        lo = torch.zeros(f['N'], f['H'], f['W'], f['C'], dtype=t['hi_in'].dtype, requires_grad=True)
        (g,) = torch.autograd.grad((R.up2_blur(lo) * t['hi_in']).sum(), [lo])
        return dict(lo=Res(g))


class LatentMix(Handler):
    rows = 'R'
    extents = ('R',)

    def reads(self, f):
        return {'R', 'J', 'D', 'backward', 'rep'} | ({'alpha_ld'} if f['backward'] != 2 else set())

    def unread(self, f):
        return {'alpha_ld'} if f['backward'] == 2 else set()

    def reps(self, f, has):
        return [f['rep']]

    def operands(self, f, has):
        Rr, J, D, bw = f['R'], f['J'], f['D'], f['backward']
        Rc = _div(Rr, f['rep'], 'rep')
        if f['alpha_ld'] and f['alpha_ld'] < J and bw != 2:
            raise PlanRefError('alpha_ld < J')
        al = In((Rr,), f['alpha_ld'], J, draw='u01') if f['alpha_ld'] else In((), J, draw='u01')
        if bw == 0:
            return dict(codes=In((Rc, J), D), avg=In((J,), D), styles=In((Rr, J), D), alpha=al, out=Out((Rr, J), D))
        if bw == 1:
            return dict(dout=In((Rr, J), D), alpha=al, dcodes=Out((Rc, J), D))
        return dict(codes=In((Rc, J), D), avg=In((J,), D), styles=In((Rr, J), D), dout=In((Rr, J), D), out=Out((Rr,), J))

    def ref(self, f, t, has):
        rep, bw = max(f['rep'], 1), f['backward']
        if bw == 2:
            term = R.latent_alpha_terms(t['codes'], t['avg'] if 'avg' in has else None, t['styles'], t['dout'], rep)
            cc = R.latent_alpha_c(f['D'])
            return dict(out=Res(term.sum(dim=-1), tol=cc * U * term.double().abs().sum(dim=-1)))
        if bw == 0:
            if f['alpha_ld']:
                return dict(out=Res(R.latent_mix_rows(t['codes'], t.get('avg'), t['styles'], t['alpha'], rep)))
            return dict(out=Res(R.latent_mix(t['codes'], t.get('avg'), t['styles'], t['alpha'], rep)))
        if f['alpha_ld']:
            return dict(dcodes=Res(R.latent_mix_rows_bwd(t['dout'], t['alpha'], rep)))
        return dict(dcodes=Res(R.latent_mix_bwd(t['dout'], t['alpha'], rep)))


class Layernorm(Handler):
    rows = 'rows'
    extents = ('rows',)

    def reads(self, f):
        return {'rows', 'C', 'eps', 'backward'} | ({'accumulate'} if f['backward'] else set())

    def operands(self, f, has):
        n, C = f['rows'], f['C']
        o = dict(a=In((n,), C), b=In((n,), C), gamma=In((), C))
        if f['backward']:
            o.update(stats=In((n,), 2), dy=In((n,), C), dx=Operand((n,), C, role='inout' if f['accumulate'] else 'out'))
        else:
            o.update(beta=In((), C), y=Out((n,), C), stats=Out((n,), 2))
        return o

    def derived(self, f, t, has):
        """inputs that are another op's outputs: the backward's stats are the forward's of the same a (+ b)"""
        if f['backward']:
            return dict(stats=R.layernorm(t['a'].double(), None if 'b' not in has else t['b'].double(), torch.ones(f['C'], dtype=torch.float64),
                                          torch.zeros(f['C'], dtype=torch.float64), f['eps'])[1].float())
        return {}

    def ref(self, f, t, has, accumulate=None):
        b = t.get('b')
        if not f['backward']:
            y, st = R.layernorm(t['a'], b, t['gamma'], t['beta'], f['eps'])
            return dict(y=Res(y), stats=Res(st))
        g = R.layernorm_bwd(t['a'], b, t['gamma'], f['eps'], t['dy'])
        acc = f['accumulate'] if accumulate is None else accumulate
        return dict(dx=Res(t['dx'] + g if acc else g))


class Resize2Crop(Handler):
    extents = ('N', 'H', 'W', 'C')

    def reads(self, f):
        return {'N', 'H', 'W', 'C', 'crop', 'backward'} | ({'accumulate'} if f['backward'] else set())

    def operands(self, f, has):
        N, H, W, C, cr = f['N'], f['H'], f['W'], f['C'], f['crop']
        if f['backward']:
            return dict(dy=In((N, 2 * H - 2 * cr, 2 * W), C), dx=Operand((N, H, W), C, role='inout' if f['accumulate'] else 'out'))
        return dict(x=In((N, H, W), C), y=Out((N, 2 * H - 2 * cr, 2 * W), C))

    def ref(self, f, t, has):
        if not f['backward']:
            return dict(y=Res(R.resize2_crop(t['x'], f['crop'])))
        g = R.resize2_crop_adjoint(t['dy'], f['crop'])
        return dict(dx=Res(t['dx'] + g if f['accumulate'] else g))


class Attn(Handler):
    extents = ('N', 'Tk')

    def reads(self, f):
        return {'N', 'Tq', 'Tk', 'heads', 'dh', 'scale', 'backward', 'ldq', 'ldk', 'ldv', 'ldo'} | ({'lddq', 'lddk', 'lddv'} if f['backward'] else set())

    def operands(self, f, has):
        N, Tq, Tk, hd = f['N'], f['Tq'], f['Tk'], f['heads']
        E = hd * f['dh']
        if min(f['ldq'], f['ldk'], f['ldv'], f['ldo']) < E or (f['backward'] and min(f['lddq'], f['lddk'], f['lddv']) < E):
            raise PlanRefError('a pitch below heads * dh')
        o = dict(q=In((N, Tq), f['ldq'], E), k=In((N, Tk), f['ldk'], E), v=In((N, Tk), f['ldv'], E))
        if f['backward']:
            o.update(p=In((N, hd, Tq), Tk, draw='pos'), dout=In((N, Tq), f['ldo'], E), ds=Operand((N, hd, Tq), Tk, role='ws'),
                     dq=Out((N, Tq), f['lddq'], E), dk=Out((N, Tk), f['lddk'], E), dv=Out((N, Tk), f['lddv'], E))
        else:
            o.update(out=Out((N, Tq), f['ldo'], E), p=Out((N, hd, Tq), Tk))
        return o

    def derived(self, f, t, has):
        if f['backward']:
            return dict(p=R.attn(t['q'].double(), t['k'].double(), t['v'].double(), f['heads'], f['scale'])[1].float())
        return {}

    def ref(self, f, t, has):
        rows = R.weighted_rows_in_groups if t['q'].dtype == torch.float32 else R.weighted_rows
        if not f['backward']:
            out, p = R.attn(t['q'], t['k'], t['v'], f['heads'], f['scale'], rows=rows)
            return dict(out=Res(out), p=Res(p))
        dq, dk, dv = R.attn_bwd(t['q'], t['k'], t['v'], f['heads'], f['scale'], t['dout'], rows=rows)
        return dict(dq=Res(dq), dk=Res(dk), dv=Res(dv))


class Interleave2(Handler):
    extents = ('N', 'H', 'W', 'C', 'lds')

    def reads(self, f):
        return {'N', 'H', 'W', 'C', 'dact_act', 'dact_prelu', 'lds', 'dact_rep'}

    def reps(self, f, has):
        return [f['dact_rep']] if 'dact_x' in has else []

    def operands(self, f, has, lds=None):
        N, H, W, C = f['N'], f['H'], f['W'], f['C']
        lds = (f['lds'] or C) if lds is None else lds
        if lds < C or H % 2 or W % 2:
            raise PlanRefError('lds >= C, H and W even')
        o = {f's{i}': In((N, H // 2, W // 2), lds, C) for i in range(4)}
        o.update(dact_x=In((_div(N, f['dact_rep'], 'dact_rep'), H, W), C), dact_scale=In((), C, draw='pos'), dact_shift=In((), C),
                 addend=In((N, H, W), C), addend2=In((N, H, W), C), y=Out((N, H, W), C))
        return o

    def ref(self, f, t, has):
        K = max(f['dact_rep'], 1)
        u = t.get('dact_x')
        y = R.interleave2([t.get(f's{i}') for i in range(4)], f['N'], f['H'], f['W'], f['C'], u, t.get('dact_scale'), t.get('dact_shift'),
                          t.get('addend'), t.get('addend2'), f['dact_act'], bool(f['dact_prelu']), K, dtype=t['s0'].dtype)
        skip = None
        if u is not None and (f['dact_prelu'] or f['dact_act'] in KINKED):
            pre = u.double() if f['dact_prelu'] or 'dact_scale' not in has else u.double() * t['dact_scale'].double() + t['dact_shift'].double()
            skip = R.rep_rows(R.near_kink(pre), K)
        return dict(y=Res(y, skip=skip))


class Maxpool3s2(Handler):
    extents = ('N', 'H', 'W', 'C')

    def reads(self, f):
        return {'N', 'H', 'W', 'C', 'backward', 'act_rep'}

    def reps(self, f, has):
        return [f['act_rep']] if f['backward'] else []

    def operands(self, f, has):
        N, H, W, C = f['N'], f['H'], f['W'], f['C']
        if not f['backward']:
            return dict(x=In((N, H, W), C), y=Out((N, H // 2, W // 2), C))
        return dict(x=In((_div(N, f['act_rep'], 'act_rep'), H, W), C), dy=In((N, H // 2, W // 2), C), dx=Out((N, H, W), C))

    def ref(self, f, t, has):
        if not f['backward']:
            return dict(y=Res(R.maxpool3s2(t['x']), exact=True))
        K = max(f['act_rep'], 1)
        x = R.rep_rows(t['x'], K).permute(0, 3, 1, 2)
        _, idx = torch.nn.functional.max_pool2d(x, 3, 2, 1, return_indices=True)
        dx = torch.zeros_like(x).flatten(2).scatter_add_(2, idx.flatten(2), t['dy'].permute(0, 3, 1, 2).flatten(2))
        # a window whose two largest elements tie routes by scan order: left out where the gap is within KINK_REL
        xp = torch.nn.functional.pad(t['x'].double().permute(0, 3, 1, 2), (1, 1, 1, 1), value=float('-inf'))
        top = xp.unfold(2, 3, 2).unfold(3, 3, 2).flatten(-2).topk(2, dim=-1).values
        tie = (top[..., 0] - top[..., 1]) <= R.KINK_REL * t['x'].abs().max().double()
        tie = torch.nn.functional.max_pool2d(torch.nn.functional.interpolate(tie.double(), scale_factor=2), 3, 1, 1) > 0
        return dict(dx=Res(dx.view_as(x).permute(0, 2, 3, 1), skip=R.rep_rows(tie.permute(0, 2, 3, 1), K)))


class Dml(Handler):
    extents = ('N', 'H', 'W')

    def reads(self, f):
        return {'ld', 'nmix', 'N', 'H', 'W', 'backward', 'ld_img', 'act_rep'}

    def reps(self, f, has):
        return [f['act_rep']] if f['backward'] else []

    def operands(self, f, has):
        N, H, W, ld, nm, ldi = f['N'], f['H'], f['W'], f['ld'], f['nmix'], f['ld_img'] or 3
        if ld < 10 * nm or ldi < 3 or (f['act_rep'] > 1 and not f['backward']):
            raise PlanRefError('ld >= 10 nmix, ld_img >= 3, act_rep on the backward only')
        if not f['backward']:
            return dict(logits=In((N, H, W), ld, 10 * nm), img_nchw=Out((N, 3, H), W), img_nhwc=Out((N, H, W), ldi))
        return dict(logits=In((_div(N, f['act_rep'], 'act_rep'), H, W), ld, 10 * nm), dimg_nhwc=In((N, H, W), ldi, 3), dimg_nchw=In((N, 3, H), W),
                    dlogits=Out((N, H, W), ld))

    def ref(self, f, t, has):
        nm, lg = f['nmix'], t['logits']
        if not f['backward']:
            img = R.dml_mean(lg, nm)
            return dict(img_nchw=Res(img.permute(0, 3, 1, 2)), img_nhwc=Res(R.pitched(img, f['ld_img'] or 3, 0.0)))
        K = max(f['act_rep'], 1)
        zero = torch.zeros(f['N'], f['H'], f['W'], 3, dtype=lg.dtype)
        dimg = (t['dimg_nhwc'] if 'dimg_nhwc' in has else zero) + (t['dimg_nchw'].permute(0, 2, 3, 1) if 'dimg_nchw' in has else zero)
        g = R.dml_mean_bwd(lg, nm, dimg, K)
        skip = R.rep_rows(R.near_kink(R.dml_pre(lg.double(), nm), (-1.0, 1.0)).any(dim=-1, keepdim=True), K)
        return dict(dlogits=Res(R.pitched(g, f['ld'], 0.0), skip=skip.expand(-1, -1, -1, f['ld'])))


def _s2d_view(img, ld):
    """dense [N,H,W,c] -> the space-to-depth operand [N,H/2,W/2,4,ld] (pad lanes zero)"""
    N, H, W, _ = img.shape
    return R.s2d_pack(img, ld, 0.0).view(N, H // 2, W // 2, 4, ld)


def _s2d_dense(t):
    """[N,h,w,4,c] -> [N,2h,2w,c]"""
    N, h, w, _, c = t.shape
    return R.s2d_unpack(t.reshape(N, h, w, 4 * c), c)


class ImageIo(Handler):
    extents = ('N', 'H', 'W')

    def reads(self, f):
        return {'N', 'C', 'H', 'W', 'rep', 'backward', 'ld', 's2d'} | ({'cot_rep'} if f['backward'] else set())

    def reps(self, f, has):
        return [max(f['rep'], 1) * (max(f['cot_rep'], 1) if f['backward'] else 1)]

    def operands(self, f, has):
        N, C, H, W, ld = f['N'], f['C'], f['H'], f['W'], f['ld'] or f['C']
        rep, K = max(f['rep'], 1), max(f['cot_rep'], 1) if f['backward'] else 1
        Nf = _div(N, K, 'cot_rep')
        B = _div(Nf, rep, 'rep')
        if ld < C or (f['s2d'] and (H % 2 or W % 2)) or ('noise_nchw' in has) != ('noise_coef' in has):
            raise PlanRefError('ld >= C, s2d needs even H and W, noise comes with its coefficients')
        lead = (N, H // 2, W // 2, 4) if f['s2d'] else (N, H, W)
        o = dict(x_nchw=In((B, C, H), W, draw='u01'), noise_nchw=In((Nf, C, H), W), noise_coef=In((), Nf, draw='pos'))
        if f['backward']:
            o.update(dy_nhwc=In(lead, ld, C), dx_nchw=Out((B * K, C, H), W))
        else:
            o['y_nhwc'] = Out(lead, ld)
        return o

    def ref(self, f, t, has):
        rep, ld = max(f['rep'], 1), f['ld'] or f['C']
        x, nz = t['x_nchw'], t.get('noise_nchw')
        coef = t.get('noise_coef')
        if not f['backward']:
            img = R.image_io(x, nz, coef, rep)
            y = _s2d_view(img, ld) if f['s2d'] else R.pitched(img, ld, 0.0)
            return dict(y_nhwc=Res(y, exact=nz is None))
        K = max(f['cot_rep'], 1)
        dy = _s2d_dense(t['dy_nhwc']) if f['s2d'] else t['dy_nhwc']
        pre = R.image_pre(x.double(), None if nz is None else nz.double(), None if nz is None else coef.double(), rep)
        B = x.shape[0]
        near = R.near_kink(pre, (0.0, 1.0)).view(B, rep, *pre.shape[1:]).any(dim=1)
        return dict(dx_nchw=Res(R.image_io_bwd(x, nz, coef, rep, dy, K), exact=nz is None and rep == 1, skip=R.rep_rows(near, K)))   # rep > 1: a sum


class Blur(Handler):
    rows = 'planes'
    extents = ('planes', 'H', 'W')

    def reads(self, f):
        return {'planes', 'H', 'W', 'k', 'backward', 'radius'}

    def operands(self, f, has):
        n, H, W, k = f['planes'], f['H'], f['W'], f['k']
        if k % 2 == 0 or k // 2 >= min(H, W):
            raise PlanRefError('k odd, k / 2 < H, W')
        two_pass = (2 * H * W + k) * 4 > 64 * 1024
        if two_pass and 'tmp' not in has:
            raise PlanRefError('planes above 64 KB need tmp')
        o = dict(x=In((n, H), W), y=Out((n, H), W), taps=In((), k, draw='pos'))
        if 'tmp' in has:
            o['tmp'] = Operand((n, H), W, role='ws' if two_pass else 'in')
        return o

    def ref(self, f, t, has):
        fn = R.gauss_blur_adjoint if f['backward'] else R.gauss_blur
        return dict(y=Res(fn(t['x'], t['taps'], f['radius'])))


class Gconv(Handler):
    extents = ('N', 'Hi', 'Wi', 'Ho', 'Wo')

    def reads(self, f):
        return {'N', 'Hi', 'Wi', 'Ho', 'Wo', 'C', 'cg', 'KH', 'KW', 'stride', 'pad', 'pro_act', 'dact_act', 'dact_rep'}

    def reps(self, f, has):
        return [f['dact_rep']] if 'dact_x' in has else []

    def operands(self, f, has):
        N, C, cg = f['N'], f['C'], f['cg']
        if cg % 4 or C % cg:
            raise PlanRefError('C = groups * cg, cg % 4 == 0')
        return dict(x=In((N, f['Hi'], f['Wi']), C), w=In((C,), f['KH'] * f['KW'] * cg), bias=In((), C),
                    dact_x=In((_div(N, f['dact_rep'], 'dact_rep'), f['Ho'], f['Wo']), C), y=Out((N, f['Ho'], f['Wo']), C))

    def ref(self, f, t, has):
        K, u = max(f['dact_rep'], 1), t.get('dact_x')
        y = R.gconv(t['x'], t['w'], t.get('bias'), f['cg'], f['KH'], f['KW'], f['stride'], f['pad'], f['Ho'], f['Wo'], f['pro_act'], u, f['dact_act'], K)
        return dict(y=Res(y, skip=None if u is None else _kink(u, f['dact_act'], K)))


class PoolDenorm(Handler):
    extents = ('N', 'H', 'W')

    def reads(self, f):
        return {'N', 'H', 'W', 'k', 'ld', 'backward', 'band'}

    def operands(self, f, has):
        N, H, W, k, ld = f['N'], f['H'], f['W'], f['k'], f['ld']
        if H % 2 or W % 2 or ld % 4 or ld < 3 or k < 1:
            raise PlanRefError('H, W even; ld % 4 == 0')
        if f['backward']:
            return dict(dy=In((N, H // 2, W // 2, 4), ld, 3), dy_nchw=In((N, 3, H), W), dx=Out((N, k * H, k * W), 4))
        return dict(x=In((N, k * H, k * W), 4, 3), y=Out((N, H // 2, W // 2, 4), ld))

    def ref(self, f, t, has):
        if not f['backward']:
            return dict(y=Res(_s2d_view(R.pool_denorm(R.pitched(t['x'], 4, 0.0), f['k'], f['band']), f['ld'])))
        g = R.pool_denorm_bwd(_s2d_dense(t['dy']), t.get('dy_nchw'), f['k'], f['band'])
        return dict(dx=Res(R.pitched(g, 4, 0.0)))


class Avae(Handler):
    extents = ('N', 'P', 'H', 'W')
    OWN = {0: {'N', 'P', 'C'}, 1: {'N', 'H', 'W', 'C', 'k'}, 2: {'N', 'C'}, 3: {'N', 'P', 'C', 'f0'}}

    def reads(self, f):
        return self.OWN.get(f['mode'], set()) | {'mode', 'backward', 'act_rep'}

    def reps(self, f, has):
        return [f['act_rep']] if f['backward'] else []

    def operands(self, f, has):
        N, P, C, m, bw = f['N'], f['P'], f['C'], f['mode'], f['backward']
        if m not in self.OWN or (f['act_rep'] > 1 and not bw):
            raise PlanRefError('mode 0 .. 3; act_rep on the backward only')
        Nf = _div(N, f['act_rep'], 'act_rep') if bw else N
        if m == 0:
            if ('a' in has) != ('b' in has):
                raise PlanRefError('ADAIN: the noise comes with its weights')
            o = dict(x=In((Nf, P), C), a=In((Nf,), P), b=In((), C), c=In((Nf,), 2 * C))
            o.update(dict(s=In((Nf, C), 2), dy=In((N, P), C), y=Out((N, P), C), y2=Out((N,), 2 * C)) if bw else dict(y=Out((N, P), C), y2=Out((N, C), 2)))
            return o
        if m == 1:
            H, W, k = f['H'], f['W'], f['k']
            if k < 1 or H % k or W % k:
                raise PlanRefError('AVGPOOL: k | H, W')
            if bw:
                return dict(x=In((Nf, H, W), C), dy=In((N, H // k, W // k), C), y=Out((N, H, W), C))
            return dict(x=In((N, H, W), C), y=Out((N, H // k, W // k), C))
        if m == 2:
            return dict(x=In((Nf,), C), dy=In((N,), C), y=Out((N,), C)) if bw else dict(x=In((N,), C), y=Out((N,), C))
        o = dict(x=In((Nf, P), 2 * C), a=In((Nf, C), P))
        o.update(dict(dy=In((N, P), C), y=Out((N, P), 2 * C)) if bw else dict(y=Out((N, P), C)))
        return o

    def derived(self, f, t, has):
        if f['mode'] == 0 and f['backward']:
            return dict(s=R.avae_adain(t['x'].double(), None if 'a' not in has else t['a'].double(), None if 'b' not in has else t['b'].double(),
                                       t['c'].double())[1].float())
        return {}

    def ref(self, f, t, has):
        m, bw, K = f['mode'], f['backward'], max(f['act_rep'], 1)
        x = R.rep_rows(t['x'], K) if bw else t['x']
        if m == 0:
            a, c = (R.rep_rows(t['a'], K) if 'a' in has else None), R.rep_rows(t['c'], K)
            if not bw:
                y, st = R.avae_adain(x, a, t.get('b'), c)
                return dict(y=Res(y), y2=Res(st))
            dx, dgb = R.avae_adain_bwd(x, a, t.get('b'), c, t['dy'])
            return dict(y=Res(dx, skip=R.near_kink(R.avae_adain_pre(x, a, t.get('b')).double())), y2=Res(dgb))
        if m == 1:
            return dict(y=Res(R.avgpool_bwd(t['dy'], f['k']) if bw else R.avgpool(x, f['k'])))
        if m == 2:
            return dict(y=Res(R.pixelnorm_bwd(x, t['dy']) if bw else R.pixelnorm(x)))
        eps = R.rep_rows(t['a'], K) if bw else t['a']
        if not bw:
            return dict(y=Res(R.avae_sample(x, eps, f['f0'])))
        return dict(y=Res(R.avae_sample_bwd(x, eps, f['f0'], t['dy']), skip=R.near_kink(x.double())))


HANDLERS = {L.DwDesc: Dw(), L.ReduceDesc: Reduce(), L.SeApplyDesc: SeApply(), L.SeExciteDesc: SeExcite(), L.BilinearBwdDesc: BilinearBwd(),
            L.SamplerDesc: Sampler(), L.MaxpoolDesc: Maxpool(), L.AvgpoolActDesc: AvgpoolAct(), L.AxpbyDesc: Axpby(), L.RepSumDesc: RepSum(),
            L.PixelnormDesc: Pixelnorm(), L.PreluDesc: Prelu(), L.UnaryDesc: Unary(), L.ModoutDesc: Modout(), L.Up2BlurDesc: Up2Blur(),
            L.LatentMixDesc: LatentMix(), L.LayernormDesc: Layernorm(), L.Resize2CropDesc: Resize2Crop(), L.AttnDesc: Attn(),
            L.Interleave2Desc: Interleave2(), L.Maxpool3s2Desc: Maxpool3s2(), L.DmlDesc: Dml(), L.ImageIoDesc: ImageIo(), L.BlurDesc: Blur(),
            L.GconvDesc: Gconv(), L.PoolDenormDesc: PoolDenorm(), L.AvaeDesc: Avae()}
# descriptor types of GA_OP_LIST that have their own float64 interpreter
ELSEWHERE = (L.ConvDesc, L.DecCellDesc, L.DecCellHaloDesc)


# ---------------------------------------------------------------------------------------------------- descriptors
def make_desc(cls, f, ptr):
    """a ctypes descriptor from non-pointer fields and pointers (name -> address; name0 .. name3 for pointer arrays)"""
    d = cls()
    for k, v in f.items():
        setattr(d, k, v)
    for k, v in ptr.items():
        if k[-1].isdigit() and not hasattr(d, k):
            getattr(d, k[:-1])[int(k[-1])] = v
        else:
            setattr(d, k, v)
    return d


def desc_fields(d):
    """(non-pointer fields, pointer fields -> address); pointer arrays (s[2][2], t_planes[4]) as name0 .. name3"""
    f, p = {}, {}
    for name, typ in d._fields_:
        v = getattr(d, name)
        if name.startswith('_reserved'):
            continue
        if hasattr(v, '__len__'):
            for i, e in enumerate(v):
                if e:
                    p[f'{name}{i}'] = int(e)
        elif typ is L.fp:
            if v:
                p[name] = int(v)
        else:
            f[name] = v
    return f, p


class PlanOp:
    """one descriptor as a plan holds it"""

    def __init__(self, cls, f, has, align, groups, where=''):
        self.cls, self.f, self.has, self.align, self.groups, self.where = cls, dict(f), frozenset(has), tuple(align), tuple(groups), [where]
        self.h = HANDLERS[cls]

    @property
    def key(self):
        return self.cls.__name__, tuple(sorted(self.f.items())), tuple(sorted(self.has)), self.align, self.groups

    def klass(self):
        """the identity without the extents (slice offsets are extents too: they are multiples of C)"""
        ext = set(self.h.extents)
        return (self.cls.__name__, tuple(sorted((k, v) for k, v in self.f.items() if k not in ext)), tuple(sorted(self.has)), self.align,
                tuple(tuple((n, o > 0) for n, o in g) for g in self.groups))

    def pixels(self):
        o = self.h.operands(self.f, self.has)
        return max(math.prod(v.lead[1:]) * v.ld if v.lead else v.ld for k, v in o.items() if k in self.has)

    def label(self):
        ints = ' '.join(f'{k}={v:g}' if isinstance(v, float) else f'{k}={v}' for k, v in self.f.items() if v)
        extra = [f'{"=".join(n for n, _ in g)}' if all(o == 0 for _, o in g) else '|'.join(f'{n}+{o}' for n, o in g) for g in self.groups if len(g) > 1]
        return f'{self.cls.__name__[:-4]} {ints} [{",".join(sorted(self.has))}]' + (f' {{{"; ".join(extra)}}}' if extra else '')

    def with_rows(self, n=None):
        """the same op at the least legal row count (or n rows)"""
        h = self.h
        f = dict(self.f)
        if h.rows is not None:
            least = h.least_rows(f, self.has)
            n = least if n is None else n
            if f[h.rows] % least == 0 and n <= f[h.rows]:
                f[h.rows] = n
        return PlanOp(self.cls, f, self.has, self.align, self.groups, self.where[0])

    def desc(self, ptr):
        """a ctypes descriptor with the pointers of `ptr` (name -> address)"""
        return make_desc(self.cls, self.f, ptr)


def check_fields(cls, f, has):
    """every non-zero field is one the handler interprets (or one the header says is not read in this mode)"""
    h = HANDLERS.get(cls)
    if h is None:
        raise PlanRefError(f'{cls.__name__}: no handler')
    ok = h.reads(f) | h.unread(f)
    extra = sorted(k for k, v in f.items() if v and k not in ok)
    if extra:
        raise PlanRefError(f'{cls.__name__}: fields {extra} are set and no reference reads them')
    o = h.operands(f, has)
    unknown = sorted(k for k in has if k not in o)
    if unknown:
        raise PlanRefError(f'{cls.__name__}: pointers {unknown} are set and the handler has no such operand in this mode')
    return o


def capture(d, where=''):
    f, p = desc_fields(d)
    cls = type(d)
    o = check_fields(cls, f, set(p))
    names = sorted(p)
    parent = {n: n for n in names}

    def find(n):
        while parent[n] != n:
            n = parent[n]
        return n
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            oa, ob = o[a], o[b]
            if oa.lead != ob.lead or oa.ld != ob.ld:
                continue
            delta = abs(p[a] - p[b])
            if delta == 0 or (delta % 4 == 0 and delta // 4 < oa.ld):
                parent[find(b)] = find(a)
    # two operands that share memory and are not one group would be rebuilt as separate tensors: the alias would go untested
    span = {n: 4 * (math.prod(o[n].lead) * o[n].ld - (o[n].ld - o[n].used)) for n in names}
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            if find(a) != find(b) and p[a] < p[b] + span[b] and p[b] < p[a] + span[a]:
                raise PlanRefError(f'{cls.__name__}: {a} and {b} overlap and are neither equal nor channel slices of one tensor '
                                   f'([{o[a].lead}, {o[a].ld}] at {p[a]:#x}, [{o[b].lead}, {o[b].ld}] at {p[b]:#x})')
    groups = {}
    for n in names:
        groups.setdefault(find(n), []).append(n)
    out, align = [], []
    for members in groups.values():
        base = min(p[n] for n in members)
        g = tuple(sorted((n, (p[n] - base) // 4) for n in members))
        for n, off in g:
            if off + o[n].used > o[n].ld:
                raise PlanRefError(f'{cls.__name__}: slice {n} at channel {off} leaves its tensor of pitch {o[n].ld}')
        out.append(g)
        align.append((g[0][0], base % 16 // 4))
    order = sorted(range(len(out)), key=lambda i: out[i])
    return PlanOp(cls, f, set(p), [align[i] for i in order], [out[i] for i in order], where)


# ---------------------------------------------------------------------------------------------------- memory
class Buffers:
    """the operands of a PlanOp in memory: one storage per group of aliased / sliced pointers, [rows + 1 sentinel row][ld] floats
    behind its recorded 16-byte offset.  Everything starts as POISON; the used channels of inputs are drawn, of outputs NaN, of
    in / out operands drawn (the reference gets the draw); workspaces NaN."""

    def __init__(self, op, device='cpu', seed=0):
        self.op, self.device = op, device
        self.spec = {k: v for k, v in op.h.operands(op.f, op.has).items() if k in op.has}
        gen = torch.Generator().manual_seed(seed)
        self.store, self.view, self.role = [], {}, {}
        al = dict(op.align)
        for g in op.groups:
            sp = self.spec[g[0][0]]
            rows = math.prod(sp.lead)
            sent = math.prod(sp.lead[1:]) if sp.lead else 1
            off0 = al.get(g[0][0], 0)
            st = torch.full((off0 + (rows + sent) * sp.ld,), POISON)
            self.store.append(st)
            strides = []
            acc = sp.ld
            for n in reversed(sp.lead):
                strides.insert(0, acc)
                acc *= n
            roles = {}
            for n, off in g:
                s = self.spec[n]
                v = st[off0 + off:].as_strided(s.shape, tuple(strides) + (1,))
                self.view[n] = v
                roles.setdefault(off, []).append(s.role)
            for n, off in g:
                rs = roles[off]
                role = 'ws' if 'ws' in rs else 'inout' if ('inout' in rs or ('in' in rs and 'out' in rs)) else rs[0]
                self.role[n] = role
            done = set()
            for n, off in g:
                if off in done:
                    continue
                done.add(off)
                s, v = self.spec[n], self.view[n]
                if self.role[n] in ('out', 'ws'):
                    v.fill_(float('nan'))
                else:
                    t = torch.randn(s.shape, generator=gen)
                    if s.draw == 'pos':
                        t = t.abs() * 0.5 + 0.5
                    elif s.draw == 'u01':
                        t = torch.rand(s.shape, generator=gen)
                    v.copy_(t)
        first = self.inputs(torch.float32)
        for k, v in getattr(op.h, 'derived', lambda *a: {})(op.f, first, op.has).items():
            self.view[k].copy_(v)
        if device != 'cpu':
            self.store = [s.to(device) for s in self.store]
            cpu_views, self.view = self.view, {}
            for g, st in zip(op.groups, self.store):
                off0 = al.get(g[0][0], 0)
                for n, off in g:
                    cv = cpu_views[n]
                    self.view[n] = st[off0 + off:].as_strided(cv.shape, cv.stride())
        self.before = [s.clone() for s in self.store]

    def pointers(self):
        return {n: v.data_ptr() for n, v in self.view.items()}

    def inputs(self, dtype):
        """dense copies of everything the op may read, as they are now"""
        return {n: v.detach().cpu().to(dtype).contiguous() for n, v in self.view.items() if self.role[n] in ('in', 'inout')}

    def reset(self):
        for s, b in zip(self.store, self.before):
            s.copy_(b)

    def untouched(self):
        """every float outside the used channels of the outputs and workspaces still holds its bits"""
        bad = []
        for g, st, b in zip(self.op.groups, self.store, self.before):
            now = st.clone()
            cur = now.view(torch.int32)
            al = dict(self.op.align).get(g[0][0], 0)
            for n, off in g:
                if self.role[n] != 'in':
                    v = self.view[n]
                    now[al + off:].as_strided(v.shape, v.stride()).copy_(b[al + off:].as_strided(v.shape, v.stride()))
            if not torch.equal(cur, b.view(torch.int32)):
                bad.append('|'.join(n for n, _ in g))
        return bad


def seed_of(op):
    """the seed of an op's draws: a function of its identity, the same on every machine"""
    import zlib
    return zlib.crc32(repr(op.key).encode()) & 0x7fffffff


def reference(op, inputs):
    """name -> Res for the op's outputs; `inputs` from Buffers.inputs (float64 or float32)"""
    r = op.h.ref(op.f, inputs, op.has)
    return {k: v for k, v in r.items() if k in op.has}
