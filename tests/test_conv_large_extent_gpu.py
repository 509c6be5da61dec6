"""
Large extents of ga_conv2d: every kernel family with its largest counted operand at the edge of, and past, the 2 GB the fast
loaders' 31-bit byte offsets hold.  The shipped plans work there (configs[2]: [32, 1024^2, 32] tensors, convolved in row sub-batches
just under the limit); every other conv test stays within a few MB except the one shape of
test_ops_gpu.py::test_conv_beyond_2gb_runs_in_row_sub_batches.

Method (tests/convbig.py, on bigrows' primitives): one descriptor with an explicit tile and split-K factor runs once over the
whole tensors and once over consecutive row chunks whose every operand spans less than 2^30 bytes, the host advancing the pointers in
64-bit arithmetic.  Inputs come from a seeded device generator in slices of 2^28 floats, y and the workspace start as NaN bits, 256
guard floats stand behind every buffer.  Asserted per case:
  - y of the one call has the bits of the chunked result (pad channels of a pitched y included: they keep their NaN bits);
  - no written element is NaN; guards keep their bits; every input regenerates from its seed bit for bit;
  - the first chunk, the rows on either side of every cut the library makes and the last two rows are within convref's
    element-wise bound (bound_ratio <= 1 with TAU_BF3 on the split-bf16 paths, TAU_FP32 on conv_mfma).
Regimes: E = the largest N at which every counted operand stays below 0x7fffff00 bytes (one launch), P1 / P2 = the largest counted
operand past 2^31 / 2^32 bytes by two rows (the library cuts).  tests/test_conv_large_extent_cpu.py asserts the arithmetic of the
table without a GPU.

  family / path                cases (convbig.TABLE)
  conv_bf3, tiles 1 - 4        3x3 on 16 x 16 with a per-row SiLU prologue (tiles 4, 3; 2 and 1 without), the same at sn = 2, a dual-
                               source 1x1 whose x2 (ldx2 = 48) is the counted maximum
  conv_mfma, fast loader       the first case without w_hi / w_lo; the transposed form sd = 2 (8 x 8 -> 16 x 16)
  conv_mfma, generic loaders   C1 = 6 (the scalar loader), and x one float past a 16-byte boundary (vec false)
  halo tiles 5, 6, 7, 8        16 x 16 and the row-segment shape 4 x 128 at C1 = 32 and 64, per-channel SiLU / per-row prologue,
                               split-K over chunks; tile 8 with w_frag (it refuses 4 x 128: more than 288 patch pixels)
  tile 9                       4 x 4, C1 = 64, with and without split-K
  tile 11                      8 x 16, C1 = 32 and 64
  tile 12                      1x1 on 8 x 16 with w_frag and with the fragments gathered from w_hi / w_lo; on 4 x 4 (8 rows per tile)
  output side the maximum      a pitched y, a pitched addend, addend2 = y (in-place accumulation across the cuts), dact_x
  replica operands             addend_rep = 3, dact_rep = 4 (sub is no multiple of either before the rounding: the CPU test says
                               so), addend_bcast_n with a pitch that would be the maximum if it were counted
  split-K workspace            splits = 8 with 8 M Cout floats past 2^32 bytes in one launch (test_split_k_workspace_past_4gb),
                               and at P1, where every sub-batch reuses the front of ws
  one row past the limit       test_one_row_past_the_limit

Found and fixed with these cases: the library's cut ignored the row granularity of tiles 9 and 12 (a descriptor either takes at a
small N was refused with GA_E_UNSUPPORTED once it was large), and a sub-batch refused after others had run left a partly written y
behind an error code.  run_in_row_batches now cuts on multiples of 128 * rep rows where that many fit and asks every sub-batch's
check before the first launch (test_a_refused_call_has_written_nothing, test_refusals).
"""
import ctypes as C
import os
import sys
import time

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')]      # collects without one

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bigrows as B                                                      # noqa: E402
import convbig as CB                                                     # noqa: E402
import convref as CR                                                     # noqa: E402
from gen_adversarial_amd import _lib as L                                # noqa: E402

DEV = 'cuda:0'
CASES = CB.cases()


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    torch.cuda.empty_cache()


def _need(nbytes, what):
    assert nbytes <= B.MEMORY_CAP, f'{what}: {nbytes / 2 ** 30:.1f} GB is above the 48 GB a test may take'
    free = torch.cuda.mem_get_info(0)[0]
    if free < nbytes:
        pytest.skip(f'{what}: needs {nbytes / 2 ** 30:.1f} GB of device memory, {free / 2 ** 30:.1f} GB are free')


def _check(case):
    _need(case.device_bytes(), case.label())
    t0 = time.perf_counter()
    run = CB.Run(case, DEV)
    run.big()
    run.chunked()
    bad, row = run.compare()
    fails = [f'y: {bad} floats of the one call differ from the chunks, first in row {row}'] if bad else []
    for name, t in (('one call', run.buf['y']), ('chunks', run.alt['y'])):
        nan, pad = run.unwritten(t)
        if nan:
            fails.append(f'y: {nan} written elements of the {name} are NaN')
        if pad:
            fails.append(f'y: {pad} pad channels of the {name} were written')
    fails += run.guards() + run.inputs_unchanged()
    worst, off = run.anchor()
    fails += off
    torch.cuda.synchronize()
    print(f'\n  {case.label()} cuts={case.cuts()} chunks={len(case.chunks())} {"MISMATCH" if bad else "bitwise"}, '
          f'{len(case.windows())} windows err / bound {worst:.3f}, {time.perf_counter() - t0:.2f} s', flush=True)
    del run
    assert not fails, case.label() + '\n' + '\n'.join(fails)


@pytest.mark.parametrize('case', [pytest.param(c, id=f'{c.name.replace(" ", "_")}-{c.regime}') for c in CASES])
def test_one_call_equals_its_row_chunks(case):
    _check(case)


def test_split_k_workspace_past_4gb():
    case = CB.ws_case()
    assert case.ws_floats() * 4 > 1 << 32 and case.row_max * case.N < 1 << 31 and case.library_sub() is None
    _check(case)


# ------------------------------------------------------------------------------------------------------ one row past the limit
ROW = dict(H=4096, W=4096, C=32, Cout=4)


def _one_row(t, as_rows, tile=4, hi=None, lo=None, out=None):
    H, W, Cc, Co = ROW['H'], ROW['W'], ROW['C'], ROW['Cout']
    d = L.ConvDesc()
    d.x, d.ldx, d.C1, d.w, d.y, d.ldy, d.Cout = t['x'].data_ptr(), Cc, Cc, t['w'].data_ptr(), out.data_ptr(), Co, Co
    d.N, d.Hi, d.Wi = (H, 1, W) if as_rows else (1, H, W)
    d.Ho, d.Wo, d.KH, d.KW, d.sn, d.sd, d.pad, d.tile = d.Hi, d.Wi, 1, 1, 1, 1, 0, tile
    if hi is not None:
        d.w_hi, d.w_lo = hi.data_ptr(), lo.data_ptr()
    return L.lib.ga_conv2d(C.byref(d), torch.cuda.current_stream().cuda_stream)


def test_one_row_past_the_limit():
    """N = 1 with Hi Wi ldx 4 = 2^31 >= 0x7fffff00: nothing can be cut, x_bytes becomes 0 and conv_mfma's vector loader (the `VEC`
    branch: size_t pix * ldx, plain loads) carries the launch.  The same memory described as 4096 rows of 1 x 4096 is the same 1x1
    conv; the library cuts it and the fast loader runs.  Both are one kernel template that differs in how a K tile reaches LDS: the
    MFMA chain over the tile is the same code, so the two results are compared bit for bit.  With w_hi / w_lo given the one-row
    form must fall back to fp32 (bf3 needs x_bytes > 0): the same bits again.  Explicit tiles 5 - 12 need the split-bf16 operands:
    GA_E_UNSUPPORTED, the NaN prefill intact."""
    H, W, Cc, Co = ROW['H'], ROW['W'], ROW['C'], ROW['Cout']
    n, ny = H * W * Cc, H * W * Co
    assert n * 4 >= CB.LIMIT and W * Cc * 4 < CB.LIMIT
    _need((n + 3 * ny + 4 * B.GUARD) * 4 + 2 * B.SLICE * 4, 'one row past the limit')
    t0 = time.perf_counter()
    x = B._alloc(n, DEV)
    gen = torch.Generator(device=DEV).manual_seed(77)
    for a, b in B.slices(n):
        x[a:b].normal_(generator=gen)
    w = (torch.randn(Co, Cc, device=DEV, generator=gen) / Cc ** 0.5).contiguous()
    w0 = w.clone()
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    t = dict(x=x, w=w)
    ys = [B._alloc(ny, DEV) for _ in range(3)]
    for y in ys:
        B._nan_fill(y, ny)
    assert _one_row(t, False, out=ys[0]) == 0
    assert _one_row(t, True, out=ys[1]) == 0
    assert _one_row(t, False, hi=hi, lo=lo, out=ys[2]) == 0
    torch.cuda.synchronize()
    for i, what in ((1, 'the 4096 rows the library cuts'), (2, 'the one row with w_hi / w_lo')):
        bad, first = B.bits_differ(ys[0], ys[i], ny)
        assert bad == 0, f'{what}: {bad} floats differ from the one row, first in image row {first // (W * Co)}'
    assert int(torch.isnan(ys[0][:ny]).sum()) == 0
    B._nan_fill(ys[2], ny)
    for tile in (5, 6, 7, 8, 9, 11, 12):
        assert _one_row(t, False, tile=tile, hi=hi, lo=lo, out=ys[2]) == L.GA_E_UNSUPPORTED, tile
    torch.cuda.synchronize()
    assert int(torch.isnan(ys[2][:ny]).sum()) == ny
    for y in ys:
        assert bool((y[ny:].view(torch.int32) == B.SENTINEL).all())
    assert bool((x[n:].view(torch.int32) == B.SENTINEL).all()) and torch.equal(w, w0)
    gen = torch.Generator(device=DEV).manual_seed(77)
    tmp = torch.empty(B.SLICE, device=DEV)
    for a, b in B.slices(n):
        tmp[:b - a].normal_(generator=gen)
        assert B.bits_differ(tmp, x[a:b], b - a)[0] == 0, 'x changed'
    # sampled windows against convref: the first, one in the middle (past 2^30 bytes) and the last two image rows
    from types import SimpleNamespace
    worst = 0.0
    for r0 in (0, H // 2 + 1, H - 2):
        d = SimpleNamespace(N=2, Hi=1, Wi=W, Ho=1, Wo=W, C1=Cc, C2=0, Cout=Co, KH=1, KW=1, sn=1, sd=1, pad=0, ldx=Cc, ldy=Co, flags=0,
                            pro_act=0, pro_per_row=0, dact_act=0, addend_bcast_n=0, addend_rep=1, dact_rep=1)
        ref, sc, slack = CR.conv_ref(d, dict(x=x[r0 * W * Cc:(r0 + 2) * W * Cc].cpu(), w=w.cpu()))
        got = ys[0][r0 * W * Co:(r0 + 2) * W * Co].cpu().view(2, 1, W, Co)
        worst = max(worst, CR.bound_ratio(got, ref, sc, slack, CR.TAU_FP32)[0])
    print(f'\n  one row past the limit: bitwise, err / bound {worst:.3f}, {time.perf_counter() - t0:.2f} s', flush=True)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------ refusals
def _tiny(**kw):
    buf = torch.zeros(1 << 16, device=DEV)
    d = L.ConvDesc()
    d.x = d.w = d.y = d.addend = d.dact_x = buf.data_ptr()
    d.ldx = d.C1 = d.ldy = d.Cout = d.ldadd = d.lddact = 4
    d.N, d.Hi, d.Wi, d.Ho, d.Wo, d.KH, d.KW, d.sn, d.sd, d.pad = 12, 4, 4, 4, 4, 1, 1, 1, 1, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d, buf


def test_refusals():
    """the lines run_in_row_batches draws before any launch, with tiny buffers and a lowered row limit: a cut of fewer rows than the
    replica operands share is GA_E_UNSUPPORTED, a row count the replica counts do not divide GA_E_BADARG"""
    row = 4 * 4 * 4 * 4
    for fields, limit, want in ((dict(addend_rep=3, dact_rep=4), 11 * row + 1, L.GA_E_UNSUPPORTED),      # sub = 11 < 3 * 4
                                (dict(addend_rep=3, dact_rep=1), 2 * row + 1, L.GA_E_UNSUPPORTED),       # sub = 2 < 3
                                (dict(addend_rep=5, dact_rep=1), 6 * row + 1, L.GA_E_BADARG),            # 12 % 5
                                (dict(addend_rep=1, dact_rep=1), 6 * row + 1, 0)):
        d, buf = _tiny(**fields)
        old = L.lib.ga_debug_set_conv_row_limit(limit)
        try:
            rc = L.lib.ga_conv2d(C.byref(d), 0)
        finally:
            L.lib.ga_debug_set_conv_row_limit(old)
        torch.cuda.synchronize()
        assert rc == want, (fields, rc)
        if want:
            assert not bool(buf.any()), 'a refused call wrote'
    d, _ = _tiny(dact_rep=5)                                            # validate: N % dact_rep, at any size
    assert L.lib.ga_conv2d(C.byref(d), 0) == L.GA_E_BADARG


@pytest.mark.parametrize('name', ['quad 4x4 C1=64', 'pw 4x4 frag'])
def test_a_refused_call_has_written_nothing(name):
    """tile 9 and tile 12 at real extents with a row count their own check refuses at ANY size (N % 32 != 0 above 32; N Ho Wo % 128
    != 0).  The library's cut is aligned (a multiple of 128 rows), so every sub-batch but the remainder would run: the call must
    return GA_E_UNSUPPORTED with y's NaN prefill intact.  (A row count the check accepts is never refused for its size: the P1 and
    P2 cases of both tiles above run with N a multiple of the granularity and cuts the library makes itself.)"""
    f, ops, tile = next((f, ops, tile) for n, f, ops, tile, _, _ in CB.TABLE if n == name)
    ok = CB.Case(name, 'P1', f, ops, tile)
    case = CB.Case(name, 'P1', f, ops, tile, N=ok.N + ok.gran // 2)
    assert case.library_sub() % 128 == 0 and (case.N - case.library_sub()) % ok.gran
    _need(case.device_bytes(), case.label())
    run = CB.Run(case, DEV)
    rc = L.lib.ga_conv2d(C.byref(run.desc(0, case.N, False)), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == L.GA_E_UNSUPPORTED
    n = run.ops['y'].numel(case.N)
    assert sum(int(torch.isnan(run.buf['y'][a:b]).sum()) for a, b in B.slices(n)) == n, 'the refused call wrote part of y'
    assert not run.guards()


# ------------------------------------------------------------------------------------------------------ the comparison sees a wrap
@pytest.mark.parametrize('regime, held, signed', [('E', 1 << 30, True), ('P2', 1 << 32, False)])
def test_comparison_sees_a_wrapped_row(regime, held, signed):
    """no kernel runs.  For the 'y largest' case the expected tensor gets, in the two rows at and past the byte offset a narrower
    offset would stop at, what such an offset would have addressed: at E an offset of 31 signed bits (it holds 2^30 and turns
    negative: the row is never written, NaN), at P2 one of 32 unsigned bits (it starts again at the front: an early row's data).
    The equality check must fail at exactly the first such row."""
    f, ops, tile = next((f, ops, tile) for n, f, ops, tile, _, _ in CB.TABLE if n == 'y largest')
    case = CB.Case('y largest', regime, f, ops, tile)
    row = case.operands()['y'].row
    n = case.N * row
    assert n * 4 > held + 2 * row * 4
    _need(2 * (n + B.GUARD) * 4 + B.SLICE * 8, f'wrap visibility {regime}')
    gen = torch.Generator(device=DEV).manual_seed(5)
    got, want = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    for a, b in B.slices(n):
        got[a:b].normal_(generator=gen)
        want[a:b].copy_(got[a:b])
    assert B.bits_differ(got, want, n) == (0, None)
    first, wrapped = CB.wrapped_rows(case, held, signed)
    assert (first - 1) * row * 4 < held <= first * row * 4
    for r, src in wrapped.items():
        assert src != r
        if src is None:
            want[r * row:(r + 1) * row].fill_(float('nan'))
        else:
            want[r * row:(r + 1) * row].copy_(got[src * row:(src + 1) * row])
    bad, at = B.bits_differ(got, want, n)
    print(f'\n  wrap visibility {regime}: N={case.N}, rows {first}, {first + 1} -> {list(wrapped.values())}; {bad} floats differ, first in row {at // row}', flush=True)
    assert bad > row and at // row == first
