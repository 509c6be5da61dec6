"""
The case table of tests/test_conv_large_extent_gpu.py (tests/convbig.py), checked by host arithmetic before it travels to a GPU:
every N, each case's regime condition, the row granularity of every chunk and cut, the 2^30-byte chunks, the memory cap, and
that engine_core's TILES[tile].ok takes the descriptor at its first chunk (dummy aligned pointers; nothing is launched).
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bigrows as B                                                      # noqa: E402
import convbig as CB                                                     # noqa: E402

CASES = CB.cases() + [CB.ws_case()]
IDS = [f'{c.name.replace(" ", "_")}-{c.regime}' for c in CASES]


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_regime_rows_and_memory(c):
    counted, g = c.counted(), c.gran
    assert c.row_max == max(counted.values()) and c.N % g == 0 and c.N % c.arep == 0 and c.N % c.drep == 0
    if c.tile == 9:
        assert g % 32 == 0
    if c.tile == 12:
        assert (g * c.HoWo) % 128 == 0
    largest = c.row_max * c.N
    if c.regime == 'E':
        assert all(b * c.N < CB.LIMIT for b in counted.values()), 'E: every counted operand below the limit'
        assert c.row_max * (c.N + g) >= CB.LIMIT, 'E: the largest such N'
        assert c.library_sub() is None and c.cuts() == []
    elif c.regime in CB.BOUNDARY:
        b = CB.BOUNDARY[c.regime]
        assert c.row_max * (c.N - 2) >= b > c.row_max * (c.N - 2 - g), f'{c.regime}: past the boundary by two rows'
        sub = c.library_sub()
        assert sub and sub * c.row_max < CB.LIMIT and sub % g == 0 and sub % (c.arep * c.drep) == 0
        assert len(c.cuts()) >= (1 if c.regime == 'P1' else 2) and all(0 < k < c.N and k % g == 0 for k in c.cuts())
        assert (c.N - c.cuts()[-1]) % g == 0, 'the remainder batch keeps the granularity'
    else:
        assert c.regime == 'WS' and largest < 1 << 31 and c.ws_floats() * 4 > 1 << 32
    ops = c.operands()
    chunks = c.chunks()
    assert chunks[0] == (0, c.first) and chunks[-1][1] == c.N and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    for r0, r1 in chunks:
        assert r0 % g == 0 and (r1 - r0) % g == 0 and r1 > r0
        assert all(o.numel(r1 - r0) * 4 < B.CHUNK_BYTES for o in ops.values())
    for r0, r1 in c.windows():
        assert 0 <= r0 < r1 <= c.N and r0 % c.q == 0 and r1 % c.q == 0 and r1 - r0 <= max(64, 2 * c.q)
    assert c.N * c.HoWo <= 0x7fffffff
    assert c.device_bytes() <= B.MEMORY_CAP, f'{c.device_bytes() / 2 ** 30:.1f} GB'
    if c.splits > 1:
        assert c.splits <= c.f['KH'] * c.f['KW'] * ((c.f['C1'] + c.f['C2'] + 31) // 32)
        if c.tile >= 5:
            assert c.splits <= c.f['C1'] // 32


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_the_tile_takes_the_descriptor(c):
    """TILES[tile].ok restates the family's check; a dummy 16-byte-aligned pointer stands for every operand given"""
    from gen_adversarial_amd import _lib as L
    from gen_adversarial_amd.engine_core import TILES
    for n in (c.first, c.gran):
        d = L.ConvDesc()
        for k, v in c.f.items():
            setattr(d, k, v)
        d.N, d.tile, d.splits = n, c.tile, c.splits
        p = 4096
        d.x = d.w = d.y = p
        d.x = p + 4 * c.x_skew
        for k in c.operands():
            if k != 'x':
                setattr(d, k, p)
        if 'alias2' in c.ops:
            d.addend2, d.ldadd2 = p, c.f['ldy']
        if 'bias' in c.ops:
            d.bias = p
        if 'split' in c.ops:
            d.w_hi = d.w_lo = p
        if 'frag' in c.ops:
            d.w_frag = p
        if c.splits > 1:
            d.ws = p
        assert TILES[c.tile].ok(d, c.splits), (c.label(), n)


def test_the_replica_cases_need_the_rounding():
    """(lim - 1) / row_max is no multiple of the replica count in the addend_rep / dact_rep cases: the rounding-down is what keeps
    the library's sub-batches on the replica boundaries"""
    seen = set()
    for c in CASES:
        if c.regime in CB.BOUNDARY and c.arep * c.drep > 1:
            raw = (CB.LIMIT - 1) // c.row_max
            assert raw % (c.arep * c.drep) != 0 and c.library_sub() % (c.arep * c.drep) == 0, c.label()
            seen.add((c.arep, c.drep))
    assert seen == {(3, 1), (1, 4)}


def test_the_cut_of_the_small_tiles_is_rounded():
    """tile 9 and tile 12: the unrounded cut is off their row granularity, the rounded one is on it"""
    n = 0
    for c in CASES:
        if c.regime in CB.BOUNDARY and c.tile in (9, 12):
            raw = (CB.LIMIT - 1) // c.row_max
            assert c.library_sub() % c.gran == 0 and c.library_sub() % 128 == 0
            n += raw % c.gran != 0
    assert n >= 3, 'at least the tile 9 cases and tile 12 on 4 x 4 are refused without the rounding'


def test_the_broadcast_addend_is_not_counted():
    c = next(c for c in CASES if c.name == 'addend_bcast_n')
    assert 'addend' not in c.counted() and c.HoWo * c.f['ldadd'] * 4 > c.row_max


def test_wrapped_rows():
    c = next(c for c in CASES if c.name == 'y largest' and c.regime == 'P2')
    row = c.operands()['y'].row * 4
    first, w = CB.wrapped_rows(c, 1 << 32, False)
    assert (first - 1) * row < 1 << 32 <= first * row and all(0 <= v < 2 and v != r for r, v in w.items())
    first, w = CB.wrapped_rows(c, 1 << 30, True)
    assert (first - 1) * row < 1 << 30 <= first * row and set(w.values()) == {None}
