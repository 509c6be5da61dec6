"""
Helper of tests/test_large_extent_gpu.py: one descriptor at N rows, launched once over the whole tensors and once over consecutive
row chunks whose every operand spans less than 2^30 bytes, the host advancing the pointers in 64-bit arithmetic.

The operand model is planref's: Handler.operands(f, has) gives every pointer's extent [*lead, ld] from the integer fields alone.
An operand is row-indexed when its extent grows with the row field; its extent is linear in the rows, so chunk [r0, r1) starts
numel(N) * r0 / N floats behind the base (exact when r0 is a multiple of the replica fields' lcm, Handler.least_rows).  Nothing is
written per op kind except the two workspace splits whose per-row geometry depends on N (chunk_fields).

Memory: inputs are drawn by a seeded device generator in slices of at most SLICE floats and are never copied: `unchanged`
regenerates them from the seed and compares bits.  Outputs and workspaces start as NaN bits; every buffer ends in GUARD floats of
a sentinel pattern.  No ATen kernel sees more than SLICE elements.
"""
import math

import torch

import cellref as CR
import opref as R
import planref as PR
from gen_adversarial_amd import _lib as L

GUARD = 256
SLICE = 1 << 28                      # floats per ATen call (1 GB): the comparison never trusts a 2^31-element tensor
CHUNK_BYTES = 1 << 30                # every operand of a chunk spans less than this
SENTINEL = 0x7fc0dead                # a NaN payload, as int32
MEMORY_CAP = 48 << 30
TIERS = {'T1': ('bytes', 1 << 31), 'T2': ('bytes', 1 << 32), 'T3': ('elements', 1 << 31)}
ROW_FIELD = {L.AxpbyDesc: 'n', L.UnaryDesc: 'n'}          # handlers without a row field: the element count plays the part


class CellModel:
    """the operand table of ga_dec_cell / ga_dec_cell_halo (planref has none: tests/cellref.py is their reference).  The split-bf16
    weights are [rows][cols / 2] floats here (two bf16 per float); `prepare` writes real weights over the draws and `anchor` holds
    the first chunk to cellref's row-wise bound (4 x the error of the emulated split-bf16 cell, floor 2^-22)"""
    rows = 'N'

    def __init__(self, halo):
        self.halo = halo

    def _c(self, f):
        return f['Cin'] if self.halo else f['C']

    def least_rows(self, f, has):
        if self.halo:
            return 1
        M = CR.TILE_PIXELS[f['C']]
        return max(M // (f['H'] * f['W']), 1) * (max(f['act_rep'], 1) if f['backward'] else 1)

    def operands(self, f, has):
        N, H, W, C, Hd = f['N'], f['H'], f['W'], self._c(f), f['Hd']
        K = max(f['act_rep'], 1) if (f['backward'] and not self.halo) else 1
        half = PR.In((Hd,), C // 2)
        o = dict(x=PR.In((max(N // K, 1), H, W), C), w1_hi=half, w1_lo=half, b1=PR.In((), Hd), wd=PR.In((25,), Hd), wd_bwd=PR.In((25,), Hd),
                 bd=PR.In((), Hd), w2_hi=half, w2_lo=half, b2=PR.In((), C), w1t_hi=half, w1t_lo=half,
                 dout=PR.In((N, H, W), C), pro_scale=PR.In((N,), C, draw='pos'), pro_shift=PR.In((N,), C), addend=PR.In((N, H, W), C), addend2=PR.In((N, H, W), C))
        o['y'] = PR.Out((N, H, W), Hd if (f['backward'] and not self.halo) else C)
        return o

    @staticmethod
    def _weights(C, Hd):
        c = CR.inputs(1, 1, 1, C, Hd)
        return c.weights

    def prepare(self, run):
        f = run.c.f
        C, Hd = self._c(f), f['Hd']
        w1, b1, wd, bd, w2, b2 = self._weights(C, Hd)
        val = dict(b1=b1, wd=wd, wd_bwd=CR.flip_taps(wd), bd=bd, b2=b2)
        for name, w in (('w1', w1), ('w2', w2.t().contiguous() if f['backward'] else w2), ('w1t', w1.t().contiguous())):
            hi, lo = CR.split_bf16(w)
            val[f'{name}_hi'], val[f'{name}_lo'] = hi.to(torch.bfloat16).contiguous(), lo.to(torch.bfloat16).contiguous()
        for k, v in val.items():
            if k not in run.buf:
                continue
            flat = v.contiguous().view(torch.float32).reshape(-1).to(run.dev)
            assert flat.numel() == numel(run.c.spec[k]), k
            run.buf[k][:flat.numel()].copy_(flat)
            run.patch[k] = (PR.In((), flat.numel()), flat)

    def anchor(self, run):
        f, has, spec = run._first_spec()
        t = {k: run._dense(run.alt.get(k, run.buf[k]), sp).cpu().contiguous() for k, sp in spec.items() if k in ('x', 'dout', 'pro_scale', 'pro_shift', 'addend', 'addend2', 'y')}
        w = self._weights(self._c(f), f['Hd'])
        w64 = R.f64(*w)
        if not f['backward']:
            ref, emu = CR.cell_forward(t['x'].double(), *w64)[2], CR.emulate_forward(t['x'], *w)[2]
        elif self.halo:
            cot = (t['dout'], t['pro_scale'], t['pro_shift'])
            ref = CR.halo_backward(t['x'].double(), *w64, *R.f64(*cot), addend=R.f64(t.get('addend')), addend2=R.f64(t.get('addend2')))
            emu = CR.emulate_halo_backward(t['x'], *w, *cot, addend=t.get('addend'), addend2=t.get('addend2'))
        else:
            cot, K = (t['dout'], t['pro_scale'], t['pro_shift']), max(f['act_rep'], 1)
            ref, emu = CR.cell_backward(t['x'].double(), *w64, *R.f64(*cot), act_rep=K), CR.emulate_backward(t['x'], *w, *cot, act_rep=K)
        if not torch.isfinite(t['y']).all():
            return float('inf'), ['y: not every element of the first chunk was written']
        ratio = CR.worst(t['y'], ref, CR.row_bound(emu, ref))[0]
        return ratio, ([] if ratio <= 1.0 else [f'y: first chunk err / row bound = {ratio:.3f}'])


MODELS = {L.DecCellDesc: CellModel(False), L.DecCellHaloDesc: CellModel(True)}


def handler(cls):
    return MODELS.get(cls) or PR.HANDLERS[cls]


def row_field(cls):
    return ROW_FIELD.get(cls) or handler(cls).rows


def numel(sp):
    return math.prod(sp.lead) * sp.ld


def slices(n, step=SLICE):
    return [(a, min(n, a + step)) for a in range(0, n, step)]


def reduce_split(f, has):
    """segments per row of a ga_rowchan_reduce launch, as the host code of csrc/elementwise.hip picks them (1: the one-stage kernel)"""
    nchunks = (f['C'] + 63) // 64
    if 'ws' not in has or f['P'] < 4096 or f['N'] * nchunks >= 1024:
        return 1
    S = min(f['ws_floats'] // (f['N'] * f['C']), 2048 // (f['N'] * nchunks), (f['P'] + 1023) // 1024)
    return S if S >= 2 else 1


def chunk_fields(cls, f, has, rows):
    """the fields of a chunk of `rows` rows: the row count, and for the two ops whose per-row launch geometry depends on N the
    workspace size that keeps the big launch's segments per row"""
    g = dict(f)
    g[row_field(cls)] = rows
    if cls is L.ReduceDesc and 'ws' in has:
        S = reduce_split(f, has)
        g['ws_floats'] = max(S, 2) * rows * f['C'] if S >= 2 else 2 * rows * f['C']
        if S < 2 and reduce_split(g, has) != 1:             # the big launch ran one stage (many rows): so must the chunk
            return g, has - {'ws'}
    if cls is L.ModoutDesc and 'red' in has:
        S, _ = PR.Modout.red_order(f)
        g['ws_floats'] = S * rows * f['C']
    return g, has


class Case:
    """cls, fields (the row field is set from the tier), the pointers given, a tier"""

    def __init__(self, name, cls, f, has, tier, rows=None, ws_segments=0):
        self.name, self.cls, self.tier, self.ws_segments = name, cls, tier, ws_segments
        self.has = frozenset(has)
        self.h = handler(cls)
        self.rf = row_field(cls)
        zero, _ = PR.desc_fields(cls())
        f = dict(zero, **f)
        probe = self._with_rows(f, 1)
        self.least = 4 if self.h.rows is None else self.h.least_rows(probe, self.has)
        if rows is None:
            f = self._with_rows(f, self.least)
            per_row = max(numel(v) for k, v in self._specs(f).items() if self._grows(k, f)) // self.least
            unit, limit = TIERS[tier]
            first_beyond = -(-limit // (per_row * (4 if unit == 'bytes' else 1)))      # first row that starts at or past the boundary
            rows = -(-(first_beyond + 2) // self.least) * self.least
        f = self._with_rows(f, rows)
        self.f, self.N = f, rows
        self.spec = self._specs(f)
        self.row_indexed = {k for k in self.spec if self._grows(k, f)}
        self.largest = max(numel(self.spec[k]) for k in self.row_indexed)

    def _with_rows(self, f, rows):
        """ws_segments: the workspace holds that many partial sums per (row, channel), whatever the row count"""
        g = dict(f)
        g[self.rf] = rows
        if self.ws_segments:
            g['ws_floats'] = self.ws_segments * rows * g['C']
        return g

    def _specs(self, f):
        if self.cls not in MODELS:
            PR.check_fields(self.cls, f, set(self.has))
        return {k: v for k, v in self.h.operands(f, self.has).items() if k in self.has}

    def _grows(self, k, f):
        if k == 'ws':
            return False
        g = self._with_rows(f, 2 * f[self.rf])
        return numel(self.h.operands(g, self.has)[k]) != numel(self.h.operands(f, self.has)[k])

    def role(self, k):
        return self.spec[k].role

    def device_bytes(self):
        n = 0
        for k, sp in self.spec.items():
            n += (numel(sp) + GUARD) * 4 * (1 if sp.role == 'in' else 2)
        return n + 2 * SLICE * 4

    def chunks(self):
        """[(r0, r1)]: the first chunk is the least legal row count (the float64 anchor), the others as large as 2^30 bytes allow"""
        per_row = max(numel(self.spec[k]) for k in self.row_indexed) * 4 / self.N
        step = int((CHUNK_BYTES - 1) // (per_row * self.least)) * self.least
        assert step >= self.least, f'{self.name}: {self.least} rows already span 2^30 bytes'
        out, r = [(0, self.least)], self.least
        while r < self.N:
            out.append((r, min(self.N, r + step)))
            r += step
        return out

    def offset(self, k, r0):
        """floats between operand k's base and its row r0"""
        if k not in self.row_indexed:
            return 0
        n = numel(self.spec[k])
        assert (n * r0) % self.N == 0
        return n * r0 // self.N

    def label(self):
        return f'{self.name} {self.tier} N={self.N} largest={self.largest * 4} B'


# ---------------------------------------------------------------------------------------------------- device buffers
def _draw(buf, a, b, kind, gen):
    v = buf[a:b]
    if kind == 'u01':
        v.uniform_(0.0, 1.0, generator=gen)
    else:
        v.normal_(generator=gen)
        if kind == 'pos':
            v.abs_().mul_(0.5).add_(0.5)


def _alloc(n, dev):
    t = torch.empty(n + GUARD, dtype=torch.float32, device=dev)
    t[n:].view(torch.int32).fill_(SENTINEL)
    return t


def _nan_fill(t, n):
    for a, b in slices(n):
        t[a:b].fill_(float('nan'))


def bits_differ(x, y, n):
    """number of floats of x[:n] and y[:n] whose bits differ, and the first such index; compared in slices of at most SLICE"""
    bad, first = 0, None
    for a, b in slices(n):
        ne = x[a:b].view(torch.int32) != y[a:b].view(torch.int32)
        c = int(ne.sum())
        if c and first is None:
            first = a + int(ne.to(torch.uint8).argmax())
        bad += c
        del ne
    return bad, first


class Run:
    """the buffers of a case on the device and the two ways of launching it"""

    def __init__(self, case, dev, seed=1234):
        self.c, self.dev, self.seed = case, dev, seed
        self.buf, self.alt, self.patch, self.drawn = {}, {}, {}, {}
        for i, (k, sp) in enumerate(sorted(case.spec.items())):
            n = numel(sp)
            self.buf[k] = _alloc(n, dev)
            if sp.role in ('in', 'inout'):
                self._fill(k, self.buf[k], i)
            else:
                _nan_fill(self.buf[k], n)
            if sp.role != 'in':
                self.alt[k] = _alloc(n, dev)
                if sp.role == 'inout':
                    for a, b in slices(n):
                        self.alt[k][a:b].copy_(self.buf[k][a:b])
                else:
                    _nan_fill(self.alt[k], n)
        self._derive()
        if hasattr(case.h, 'prepare'):
            case.h.prepare(self)
        _, _, spec = self._first_spec()
        for k, sp in spec.items():                            # what an in / out operand held before the launches, for the reference
            if sp.role == 'inout':
                self.drawn[k] = self._dense(self.buf[k], sp).cpu().contiguous()

    def _gen(self, i):
        return torch.Generator(device=self.dev).manual_seed(self.seed * 1000 + i)

    def _fill(self, k, t, i):
        gen = self._gen(i)
        for a, b in slices(numel(self.c.spec[k])):
            _draw(t, a, b, self.c.spec[k].draw, gen)

    def _first_spec(self):
        r0, r1 = self.c.chunks()[0]
        f, has = chunk_fields(self.c.cls, self.c.f, self.c.has, r1 - r0)
        return f, has, {k: v for k, v in self.c.h.operands(f, has).items() if k in has}

    def _dense(self, t, sp):
        v = t[:numel(sp)].view(*sp.lead, sp.ld) if sp.lead else t[:sp.ld]
        return v[..., :sp.used]

    def _derive(self):
        """inputs that are another op's outputs (planref's `derived`): made valid on the first chunk, which the reference reads"""
        derived = getattr(self.c.h, 'derived', None)
        if derived is None:
            return
        f, has, spec = self._first_spec()
        t = {k: self._dense(self.buf[k], sp).cpu().contiguous() for k, sp in spec.items() if sp.role in ('in', 'inout')}
        for k, v in derived(f, t, has).items():
            self._dense(self.buf[k], spec[k]).copy_(v.to(self.dev))
            if k in self.alt:
                self._dense(self.alt[k], spec[k]).copy_(v.to(self.dev))
            self.patch[k] = (spec[k], v.to(self.dev))

    def _launch(self, f, has, ptr):
        L.run(PR.make_desc(self.c.cls, f, {k: v for k, v in ptr.items() if k in has}), torch.cuda.current_stream().cuda_stream)

    def big(self):
        self._launch(self.c.f, self.c.has, {k: t.data_ptr() for k, t in self.buf.items()})
        torch.cuda.synchronize()

    def chunked(self):
        c = self.c
        for r0, r1 in c.chunks():
            f, has = chunk_fields(c.cls, c.f, c.has, r1 - r0)
            ptr = {k: self.alt.get(k, self.buf[k]).data_ptr() + 4 * c.offset(k, r0) for k in self.buf}
            self._launch(f, has, ptr)
        torch.cuda.synchronize()

    # ------------------------------------------------------------------------------------------------ checks
    def guards(self):
        bad = []
        for name, d in (('big', self.buf), ('chunked', self.alt)):
            for k, t in d.items():
                if not bool((t[numel(self.c.spec[k]):].view(torch.int32) == SENTINEL).all()):
                    bad.append(f'{name} {k}: the guard behind it changed')
        return bad

    def inputs_unchanged(self):
        """every pure input regenerated from its seed, bit for bit.  Both launches read the same input buffers, so one check after
        both covers both.  In / out operands are compared between the two launches over their whole pitch; none of the cases has an
        in / out operand with pad channels (used < ld), which only that comparison would guard"""
        bad = []
        tmp = torch.empty(SLICE, dtype=torch.float32, device=self.dev)
        for i, (k, sp) in enumerate(sorted(self.c.spec.items())):
            if sp.role != 'in':
                continue
            gen = self._gen(i)
            for a, b in slices(numel(sp)):
                _draw(tmp, 0, b - a, sp.draw, gen)
                if a == 0 and k in self.patch:
                    psp, v = self.patch[k]
                    self._dense(tmp, psp).copy_(v)
                n, first = bits_differ(tmp, self.buf[k][a:b], b - a)
                if n:
                    bad.append(f'input {k}: {n} floats changed, first at {a + first}')
                    break
        return bad

    def written(self, k, big=False):
        """NaN count among the elements operand k's header says are written, in the chunked result or in the big launch's"""
        sp = self.c.spec[k]
        t, n = (self.buf if big else self.alt)[k], 0
        if self.c.cls is L.SamplerDesc and self.c.f['mode'] == 2:
            return int(torch.isnan(t[:numel(sp)].view(-1, self.c.f['alpha_ld'])[:, self.c.f['alpha_col']]).sum())
        if sp.used == sp.ld:
            for a, b in slices(numel(sp)):
                n += int(torch.isnan(t[a:b]).sum())
            return n
        v = t[:numel(sp)].view(-1, sp.ld)
        for a, b in slices(v.shape[0], max(SLICE // sp.ld, 1)):
            n += int(torch.isnan(v[a:b, :sp.used]).sum())
        return n

    def compare(self):
        """[(operand, floats that differ, first differing row)] between the big launch and the chunks"""
        out = []
        for k, t in self.alt.items():
            if self.c.role(k) == 'ws':
                continue
            n = numel(self.c.spec[k])
            bad, first = bits_differ(self.buf[k], t, n)
            if bad:
                row = first * self.c.N // n if k in self.c.row_indexed else 0
                out.append((k, bad, row))
        return out

    def anchor(self, yardstick):
        """the first chunk of the chunked launches against planref's float64 reference under opref.bound -> (worst ratio, failures)"""
        if hasattr(self.c.h, 'anchor'):
            return self.c.h.anchor(self)
        f, has, spec = self._first_spec()
        op = PR.PlanOp(self.c.cls, f, has, (), ())
        src = {k: self._dense(self.alt.get(k, self.buf[k]), sp) for k, sp in spec.items()}
        # in / out operands were overwritten by the launch: the reference gets the draw, regenerated
        t32 = {}
        for i, (k, sp) in enumerate(sorted(self.c.spec.items())):
            if k not in spec or spec[k].role not in ('in', 'inout'):
                continue
            if spec[k].role == 'inout':
                t32[k] = self.drawn[k]
            else:
                t32[k] = src[k].cpu().contiguous()
        t64 = {k: v.double() for k, v in t32.items()}
        r64, r32 = PR.reference(op, t64), yardstick(op, t32)
        bad, worst = [], 0.0
        for n, res in r64.items():
            got, want, skip = src[n].cpu().double(), res.value.double(), res.skip
            keep = torch.ones_like(want, dtype=torch.bool) if skip is None else ~skip.expand_as(want)
            if skip is not None and res.tol is None and skip.double().mean().item() > R.KINK_CAP:
                bad.append(f'{n}: too many elements on a kink')
            if not torch.isfinite(got[keep]).all():
                bad.append(f'{n}: not every element of the first chunk was written')
                continue
            if res.tol is not None:
                ratio = ((got - want).abs()[keep] / res.tol.expand_as(want)[keep].clamp_min(1e-300)).max().item()
            elif res.exact:
                ratio = 0.0 if torch.equal(got[keep].float(), want[keep].float()) else float('inf')
            else:
                y32 = r32[n].value
                ratio = R.max_err(got[keep], want[keep]) / R.bound(y32[keep], want[keep])
            worst = max(worst, ratio)
            if ratio > 1.0:
                bad.append(f'{n}: first chunk err / bound = {ratio:.3f}')
        return worst, bad


# ---------------------------------------------------------------------------------------------------- what a wrap would read
def wrapped_row(r, row_floats, tier):
    """the row a kernel would address instead of row r if it kept the byte offset in 32 bits (T1: signed, T2: unsigned) or the
    element index in 32 bits (T3, signed); None when the wrapped address lies before the tensor (a negative offset)"""
    if tier == 'T3':
        e = r * row_floats
        w = ((e + (1 << 31)) % (1 << 32)) - (1 << 31)
        return None if w < 0 else w // row_floats if w != e else r
    o = r * row_floats * 4
    if tier == 'T1':
        w = ((o + (1 << 31)) % (1 << 32)) - (1 << 31)
        return None if w < 0 else w // (row_floats * 4) if w != o else r
    w = o % (1 << 32)
    return w // (row_floats * 4) if w != o else r
