"""
Helper of tests/test_conv_large_extent_gpu.py and tests/test_conv_large_extent_cpu.py: one ga_conv_desc at N rows, launched once
over the whole tensors and once over consecutive row chunks whose every operand spans less than 2^30 bytes, the host advancing
the pointers in 64-bit arithmetic as run_in_row_batches (csrc/conv2d.hip) does: x, x2, y, addend2 by whole rows, addend and dact_x
by n / rep rows, the per-row prologue tables by n * C1.  The discipline is bigrows': inputs drawn by a seeded device generator in
slices of at most SLICE floats and never copied, outputs and workspaces NaN bits, GUARD sentinel floats behind every buffer; its
primitives are imported, its cases untouched.

The operand model is the descriptor's own (include/ga_ops.h).  `counted` restates what run_in_row_batches counts per output row (x,
x2, y, addend unless broadcast, addend2, dact_x, each with its pitch; a replica operand at its pitch per OUTPUT row); N follows from
the regime:
  E    the largest N (a multiple of the case's row granularity) at which every counted operand stays below LIMIT = 0x7fffff00 bytes:
       one launch, the fast loaders at the largest offsets they ever see;
  P1   the largest counted operand passes 2^31 bytes by two rows: the library cuts;
  P2   the same past 2^32 bytes: the host's pointer advances go beyond 32 bits.
The row granularity is the lcm of addend_rep, dact_rep, 32 for tile 9 and 128 / gcd(128, Ho Wo) for tile 12; chunk boundaries are
multiples of it.  `library_sub` restates the cut the library makes (rounded down to rep and, from 128 rows on, to 128 * rep rows).
"""
import math
from types import SimpleNamespace

import torch

import bigrows as B
import convref as CR

LIMIT = 0x7fffff00
BOUNDARY = {'P1': 1 << 31, 'P2': 1 << 32}
SILU = CR.GA_ACT_SILU
DEFAULTS = dict(C2=0, KH=3, KW=3, sn=1, sd=1, pad=1, pro_act=0, pro_per_row=0, dact_act=0, addend_bcast_n=0, addend_rep=1, dact_rep=1, flags=0)


class Operand:
    """rows = N // div (div 0: one row shared by all n), `row` floats each"""

    def __init__(self, div, row, role='in', draw='normal'):
        self.div, self.row, self.role, self.draw = div, row, role, draw

    def rows(self, N):
        return N // self.div if self.div else 1

    def numel(self, N):
        return self.rows(N) * self.row


class Case:
    """f: the descriptor's integer fields (pitches default to the channel counts, Ho / Wo to Hi / Wi); ops: the optional operands
    given, of 'bias', 'pro', 'addend', 'addend2', 'alias2' (addend2 is y itself: in-place accumulation), 'dact', 'split' (w_hi /
    w_lo), 'frag' (w_frag in the tile's order); x_skew: x starts that many floats past a 16-byte boundary (vec false)"""

    def __init__(self, name, regime, f, ops=(), tile=4, splits=1, x_skew=0, N=None):
        f = dict(DEFAULTS, **f)
        f.setdefault('Ho', f['Hi'])
        f.setdefault('Wo', f['Wi'])
        for ld, c in (('ldx', 'C1'), ('ldx2', 'C2'), ('ldy', 'Cout'), ('ldadd', 'Cout'), ('ldadd2', 'Cout'), ('lddact', 'Cout')):
            f.setdefault(ld, f[c])
        self.name, self.regime, self.tile, self.splits, self.x_skew = name, regime, tile, splits, x_skew
        self.ops = frozenset(ops)
        self.f = f
        self.HoWo = f['Ho'] * f['Wo']
        self.K = f['KH'] * f['KW'] * (f['C1'] + f['C2'])
        self.arep = f['addend_rep'] if 'addend' in self.ops and not f['addend_bcast_n'] and f['addend_rep'] > 1 else 1
        self.drep = f['dact_rep'] if 'dact' in self.ops and f['dact_rep'] > 1 else 1
        self.q = math.lcm(self.arep, self.drep)
        self.gran = math.lcm(self.q, 32 if tile == 9 else 1, 128 // math.gcd(128, self.HoWo) if tile == 12 else 1)
        self.tau = CR.TAU_BF3 if 'split' in self.ops else CR.TAU_FP32
        self.row_max = max(self.counted().values())
        if N is None:
            if regime == 'E':
                N = (LIMIT - 1) // self.row_max // self.gran * self.gran
            else:
                first_beyond = -(-BOUNDARY[regime] // self.row_max)          # first row that starts at or past the boundary
                N = -(-(first_beyond + 2) // self.gran) * self.gran
        self.N = N
        self.first = self.gran * -(-2 // self.gran)                          # rows of the first chunk: the float64 anchor

    # ------------------------------------------------------------------------------------------------ the operands
    def operands(self):
        f, o = self.f, {}
        pin = f['Hi'] * f['Wi']
        o['x'] = Operand(1, pin * f['ldx'])
        if f['C2'] > 0:
            o['x2'] = Operand(1, pin * f['ldx2'])
        o['y'] = Operand(1, self.HoWo * f['ldy'], 'inout' if 'alias2' in self.ops else 'out')
        if 'addend' in self.ops:
            o['addend'] = Operand(0 if f['addend_bcast_n'] else self.arep, self.HoWo * f['ldadd'])
        if 'addend2' in self.ops:
            o['addend2'] = Operand(1, self.HoWo * f['ldadd2'])
        if 'dact' in self.ops:
            o['dact_x'] = Operand(self.drep, self.HoWo * f['lddact'])
        if 'pro' in self.ops:
            o['pro_scale'] = Operand(1 if f['pro_per_row'] else 0, f['C1'], draw='pos')
            o['pro_shift'] = Operand(1 if f['pro_per_row'] else 0, f['C1'])
        return o

    def counted(self):
        """bytes per output row of what run_in_row_batches counts"""
        f = self.f
        pin, pout = f['Hi'] * f['Wi'] * 4, self.HoWo * 4
        c = {'x': pin * f['ldx'], 'y': pout * f['ldy']}
        if f['C2'] > 0:
            c['x2'] = pin * f['ldx2']
        if 'addend' in self.ops and not f['addend_bcast_n']:
            c['addend'] = pout * f['ldadd']
        if 'addend2' in self.ops or 'alias2' in self.ops:
            c['addend2'] = pout * (f['ldy'] if 'alias2' in self.ops else f['ldadd2'])
        if 'dact' in self.ops:
            c['dact_x'] = pout * f['lddact']
        return c

    def library_sub(self):
        """rows per sub-batch of the library's own cut, None when it launches once"""
        if not (self.N > 1 and self.row_max * self.N >= LIMIT and self.row_max < LIMIT):
            return None
        sub = (LIMIT - 1) // self.row_max
        both = self.arep * self.drep
        sub -= sub % both
        if sub >= 128 * both:
            sub -= sub % (128 * both)
        return sub

    def cuts(self):
        sub = self.library_sub()
        return [] if sub is None else list(range(sub, self.N, sub))

    def chunks(self):
        step = (B.CHUNK_BYTES - 1) // (4 * max(o.row for o in self.operands().values())) // self.gran * self.gran
        assert step >= self.gran, f'{self.name}: {self.gran} rows already span 2^30 bytes'
        out, r = [(0, self.first)], self.first
        while r < self.N:
            out.append((r, min(self.N, r + step)))
            r += step
        return out

    def windows(self):
        """row ranges held to convref's bound: the first chunk, q rows on either side of every cut the library makes (at least rows
        sub - 1 and sub), the last two rows; aligned to the replica counts"""
        w = {(0, self.first)}
        for c in self.cuts():
            w.add((c - self.q, min(self.N, c + self.q)))
        w.add((self.N - self.q * -(-2 // self.q), self.N))
        return sorted(w)

    def ws_floats(self):
        rows = self.library_sub() or self.N
        return self.splits * rows * self.HoWo * self.f['Cout'] if self.splits > 1 else 0

    def device_bytes(self):
        n = sum((o.numel(self.N) + B.GUARD + 4) * 4 * (1 if o.role == 'in' else 2) for o in self.operands().values())
        return n + (self.ws_floats() + B.GUARD) * 4 + 2 * B.SLICE * 4 + 16 * self.f['Cout'] * self.K

    def label(self):
        return f'{self.name} {self.regime} tile {self.tile} N={self.N} largest counted={self.row_max * self.N} B'


def fields(case, n):
    """the descriptor's integer fields at n rows, as an object convref.conv_ref and engine_core's predicates read"""
    return SimpleNamespace(N=n, tile=case.tile, splits=case.splits, **case.f)


# ---------------------------------------------------------------------------------------------------- the case table
C3 = dict(Hi=16, Wi=16, C1=64, Cout=32)                                    # 3x3 pad 1 on 16 x 16
TABLE = [
    # conv_bf3, tiles 1 - 4
    ('bf3 3x3 per-row SiLU', dict(C3, pro_act=SILU, pro_per_row=1), {'split', 'pro', 'bias'}, 4, 1, 'E P1 P2'),
    ('bf3 3x3 tile 3', dict(C3, pro_act=SILU, pro_per_row=1), {'split', 'pro'}, 3, 1, 'E'),
    ('bf3 3x3 tile 2', dict(C3, Cout=64), {'split'}, 2, 1, 'E'),
    ('bf3 3x3 tile 1', dict(C3, Cout=128), {'split'}, 1, 1, 'E'),
    ('bf3 3x3 sn=2', dict(C3, sn=2, Ho=8, Wo=8, pro_act=SILU, pro_per_row=1), {'split', 'pro'}, 4, 1, 'E P1 P2'),
    ('bf3 dual 1x1 x2 largest', dict(Hi=16, Wi=16, C1=32, C2=32, ldx2=48, Cout=32, KH=1, KW=1, pad=0), {'split'}, 4, 1, 'E P1 P2'),
    # conv_mfma, fast loader
    ('mfma 3x3 per-row SiLU', dict(C3, pro_act=SILU, pro_per_row=1), {'pro', 'bias'}, 4, 1, 'E P1 P2'),
    ('mfma transposed sd=2', dict(Hi=8, Wi=8, Ho=16, Wo=16, C1=32, Cout=8, ldy=8, sd=2), {'bias'}, 4, 1, 'E P1 P2'),
    # conv_mfma, generic loaders
    ('mfma generic C1=6', dict(Hi=16, Wi=16, C1=6, ldx=16, Cout=8), {'bias'}, 4, 1, 'E P1 P2'),
    ('mfma generic skewed x', dict(C3, Cout=8, pro_act=SILU, pro_per_row=1), {'pro', 'skew'}, 4, 1, 'E P2'),
    # halo tiles
    ('halo 16x16 C1=32', dict(C3, C1=32), {'split'}, 5, 1, 'E P2'),
    ('halo 16x16 C1=64', dict(C3, pro_act=SILU), {'split', 'pro'}, 6, 1, 'E P1'),
    ('halo 16x16 C1=64 per-row', dict(C3, pro_per_row=1), {'split', 'pro'}, 7, 1, 'E P2'),
    ('halo 4x128 C1=32', dict(Hi=4, Wi=128, C1=32, Cout=32), {'split'}, 7, 1, 'E P2'),
    ('halo 4x128 C1=64', dict(Hi=4, Wi=128, C1=64, Cout=32), {'split'}, 5, 1, 'E P1'),
    ('halo 4x128 C1=64 split-K', dict(Hi=4, Wi=128, C1=64, Cout=32), {'split'}, 6, 2, 'P1'),
    ('halo frag 16x16 C1=32', dict(C3, C1=32, pro_act=SILU), {'split', 'frag', 'pro'}, 8, 1, 'E P2'),
    ('halo frag 16x16 C1=64', dict(C3), {'split', 'frag'}, 8, 1, 'E P1'),
    # tile 9
    ('quad 4x4 C1=64', dict(Hi=4, Wi=4, C1=64, Cout=32), {'split', 'frag'}, 9, 1, 'E P1 P2'),
    ('quad 4x4 C1=64 split-K', dict(Hi=4, Wi=4, C1=64, Cout=32), {'split', 'frag'}, 9, 2, 'E P1 P2'),
    # tile 11
    ('thin 8x16 C1=32', dict(Hi=8, Wi=16, C1=32, Cout=32, pro_act=SILU), {'split', 'frag', 'pro'}, 11, 1, 'E P2'),
    ('thin 8x16 C1=64', dict(Hi=8, Wi=16, C1=64, Cout=32), {'split', 'frag'}, 11, 1, 'E P1 P2'),
    # tile 12
    ('pw 8x16 frag', dict(Hi=8, Wi=16, C1=64, Cout=128, KH=1, KW=1, pad=0), {'split', 'frag'}, 12, 1, 'E P1 P2'),
    ('pw 8x16 gathered', dict(Hi=8, Wi=16, C1=64, Cout=128, KH=1, KW=1, pad=0, pro_per_row=1), {'split', 'pro'}, 12, 1, 'E P1'),
    ('pw 4x4 frag', dict(Hi=4, Wi=4, C1=64, Cout=128, KH=1, KW=1, pad=0), {'split', 'frag'}, 12, 1, 'P1'),
    # the output side is the maximum
    ('y largest', dict(C3, C1=16, Cout=64, ldy=80), {'split'}, 2, 1, 'E P1 P2'),
    ('addend largest', dict(C3, C1=16, Cout=64, ldadd=96), {'split', 'addend'}, 2, 1, 'E P1 P2'),
    ('addend2 is y', dict(C3, C1=16, Cout=64), {'split', 'alias2'}, 2, 1, 'E P1 P2'),
    ('dact_x largest', dict(C3, C1=16, Cout=64, lddact=96, dact_act=SILU), {'dact'}, 2, 1, 'E P1 P2'),
    # replica operands at a real cut
    ('addend_rep 3', dict(C3, addend_rep=3), {'split', 'addend'}, 4, 1, 'E P1 P2'),
    ('dact_rep 4', dict(C3, dact_rep=4, dact_act=SILU), {'split', 'dact', 'addend2'}, 4, 1, 'E P1 P2'),
    ('addend_bcast_n', dict(C3, addend_bcast_n=1, ldadd=5 * 32), {'split', 'addend'}, 4, 1, 'E P1'),
    # split-K of a conv_bf3 tile at a cut: every sub-batch reuses the front of ws
    ('bf3 split-K 8', dict(Hi=16, Wi=16, C1=32, Cout=32), {'split'}, 4, 8, 'P1'),
]


def cases():
    out = []
    for name, f, ops, tile, splits, regimes in TABLE:
        for regime in regimes.split():
            out.append(Case(name, regime, f, set(ops) - {'skew'}, tile, splits, x_skew=1 if 'skew' in ops else 0))
    return out


def ws_case():
    """splits * M * Cout * 4 bytes of workspace pass 2^32 in ONE launch while no operand reaches 2^31: the epilogue's
    ws + split * M * Cout and the reduce kernel's s * slab beyond 32 bits"""
    f = dict(Hi=16, Wi=16, C1=32, Cout=32)
    rows = -(-(1 << 32) // (8 * 256 * 32 * 4)) + 2
    return Case('bf3 split-K 8 workspace', 'WS', f, {'split'}, 4, 8, N=rows)


# ---------------------------------------------------------------------------------------------------- device buffers
class Run:
    """the buffers of a case on the device and the two ways of launching it"""

    def __init__(self, case, dev, seed=4321):
        from gen_adversarial_amd.engine_core import WeightStore
        self.c, self.dev, self.seed = case, dev, seed
        self.ops = case.operands()
        self.buf, self.alt = {}, {}
        for i, (k, o) in enumerate(sorted(self.ops.items())):
            n = o.numel(case.N)
            self.buf[k] = B._alloc(n + case.x_skew, dev)[case.x_skew:] if k == 'x' else B._alloc(n, dev)
            if o.role in ('in', 'inout'):
                self._fill(k, self.buf[k], i)
            else:
                B._nan_fill(self.buf[k], n)
            if o.role != 'in':
                self.alt[k] = B._alloc(n, dev)
                if o.role == 'inout':
                    self._fill(k, self.alt[k], i)
                else:
                    B._nan_fill(self.alt[k], n)
        f = case.f
        gen = torch.Generator(device=dev).manual_seed(seed + 7)
        self.w = (torch.randn(f['Cout'], case.K, device=dev, generator=gen) / case.K ** 0.5).contiguous()
        self.bias = torch.randn(f['Cout'], device=dev, generator=gen) if 'bias' in case.ops else None
        self.small = {'w': self.w.clone()}
        if self.bias is not None:
            self.small['bias'] = self.bias.clone()
        self.store = WeightStore(dev)
        self.hi = self.lo = self.frag = None
        if 'split' in case.ops:
            self.hi, self.lo = self.store.split(self.w)
        if 'frag' in case.ops:
            self.frag = {8: self.store.frag3, 9: self.store.frag3, 11: self.store.frag_thin,
                         12: lambda w: self.store.frag3(w, taps=1)}[case.tile](self.w)
        self.ws = None
        if case.splits > 1:
            self.ws = B._alloc(case.ws_floats(), dev)
            B._nan_fill(self.ws, case.ws_floats())
        # what y held before the launches, at the rows the reference is formed for (in-place accumulation)
        self.y0 = {w: self.rows('y', self.buf['y'], *w).cpu() for w in case.windows()} if 'alias2' in case.ops else {}

    def _gen(self, i):
        return torch.Generator(device=self.dev).manual_seed(self.seed * 1000 + i)

    def _fill(self, k, t, i):
        gen = self._gen(i)
        for a, b in B.slices(self.ops[k].numel(self.c.N)):
            B._draw(t, a, b, self.ops[k].draw, gen)

    def rows(self, k, t, r0, r1):
        """rows [r0, r1) of the output-row axis of operand k in tensor t, flat"""
        o = self.ops[k]
        if not o.div:
            return t[:o.row]
        return t[(r0 // o.div) * o.row:(r1 // o.div) * o.row]

    def desc(self, r0, r1, chunked, tile=None, hi=True):
        from gen_adversarial_amd import _lib as L
        c, f = self.c, self.c.f
        d = L.ConvDesc()
        for k, v in f.items():
            setattr(d, k, v)
        d.N, d.tile, d.splits = r1 - r0, c.tile if tile is None else tile, c.splits
        for k, o in self.ops.items():
            t = self.alt[k] if chunked and k in self.alt else self.buf[k]
            setattr(d, k, t.data_ptr() + 4 * ((r0 // o.div) * o.row if o.div else 0))        # Python integers: 64-bit and beyond
        if 'alias2' in c.ops:
            d.addend2, d.ldadd2 = d.y, f['ldy']
        d.w = self.w.data_ptr()
        if self.bias is not None:
            d.bias = self.bias.data_ptr()
        if self.hi is not None and hi:
            d.w_hi, d.w_lo = self.hi.data_ptr(), self.lo.data_ptr()
        if self.frag is not None:
            d.w_frag = self.frag.data_ptr()
        if self.ws is not None:
            d.ws, d.ws_floats = self.ws.data_ptr(), c.ws_floats()
        return d

    def big(self):
        from gen_adversarial_amd import _lib as L
        L.run(self.desc(0, self.c.N, False), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()

    def chunked(self):
        from gen_adversarial_amd import _lib as L
        for r0, r1 in self.c.chunks():
            L.run(self.desc(r0, r1, True), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()

    # ------------------------------------------------------------------------------------------------ checks
    def guards(self):
        bad = []
        for name, d in (('big', self.buf), ('chunked', self.alt), ('', {'ws': self.ws} if self.ws is not None else {})):
            for k, t in d.items():
                n = self.c.ws_floats() if k == 'ws' else self.ops[k].numel(self.c.N)
                if not bool((t[n:n + B.GUARD].view(torch.int32) == B.SENTINEL).all()):
                    bad.append(f'{name} {k}: the guard behind it changed')
        return bad

    def inputs_unchanged(self):
        bad = []
        tmp = torch.empty(B.SLICE, dtype=torch.float32, device=self.dev)
        for i, (k, o) in enumerate(sorted(self.ops.items())):
            if o.role != 'in':
                continue
            gen = self._gen(i)
            for a, b in B.slices(o.numel(self.c.N)):
                B._draw(tmp, 0, b - a, o.draw, gen)
                n, first = B.bits_differ(tmp, self.buf[k][a:b], b - a)
                if n:
                    bad.append(f'input {k}: {n} floats changed, first at {a + first}')
                    break
        for k, v in self.small.items():
            if not torch.equal(v, getattr(self, k)):
                bad.append(f'input {k} changed')
        return bad

    def unwritten(self, t):
        """(NaN among the Cout channels of every pixel of y, non-NaN among the pad channels behind them)"""
        f, n = self.c.f, self.ops['y'].numel(self.c.N)
        nan = pad = 0
        if f['ldy'] == f['Cout']:
            for a, b in B.slices(n):
                nan += int(torch.isnan(t[a:b]).sum())
            return nan, 0
        v = t[:n].view(-1, f['ldy'])
        for a, b in B.slices(v.shape[0], max(B.SLICE // f['ldy'], 1)):
            nan += int(torch.isnan(v[a:b, :f['Cout']]).sum())
            pad += int((~torch.isnan(v[a:b, f['Cout']:])).sum())
        return nan, pad

    def compare(self):
        """(floats of y that differ between the one call and the chunks, the first such row)"""
        n = self.ops['y'].numel(self.c.N)
        bad, first = B.bits_differ(self.buf['y'], self.alt['y'], n)
        return bad, (first // self.ops['y'].row if bad else None)

    def anchor(self, windows=None):
        """every window of the case against convref under its element-wise bound -> (worst ratio, failures).  The first chunk is
        read from the chunked result, the others from the one call's"""
        c, f = self.c, self.c.f
        worst, bad = 0.0, []
        for w in (c.windows() if windows is None else windows):
            r0, r1 = w
            d = fields(c, r1 - r0)
            t = {k: self.rows(k, self.buf[k], r0, r1).cpu() for k, o in self.ops.items() if o.role == 'in'}
            t['w'] = self.w.cpu()
            if self.bias is not None:
                t['bias'] = self.bias.cpu()
            if 'alias2' in c.ops:
                t['addend2'] = self.y0[w]
                d.ldadd2 = f['ldy']
            y = self.rows('y', self.alt['y'] if w == (0, c.first) else self.buf['y'], r0, r1).cpu()
            y = y.view(r1 - r0, f['Ho'], f['Wo'], f['ldy'])[..., :f['Cout']]
            ref, sc, slack = CR.conv_ref(d, t)
            ratio = CR.bound_ratio(y, ref, sc, slack, c.tau)[0]
            worst = max(worst, ratio)
            if not ratio <= 1.0:
                bad.append(f'rows {r0}..{r1 - 1}: err / bound = {ratio:.3f}')
        return worst, bad


def wrapped_rows(case, held, signed):
    """(first, {row: the row a kernel would address instead, or None}) for the two rows of y at and past byte offset `held`: what a
    byte offset that holds no more would have addressed.  A signed one turns negative (the row is never written: None), an
    unsigned one starts again at the front of the tensor"""
    row = case.operands()['y'].row * 4
    first = -(-held // row)
    return first, {r: None if signed else (r * row % held) // row for r in (first, first + 1)}
