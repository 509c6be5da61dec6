"""CPU: the counter-based noise contract (include/ga_ops.h, ga_randn) as gen_adversarial_amd/noise.py restates it — Philox4x32-10
known answers, independence of how rows are cut, moments, the open unit interval — and ga_randn's argument checks, which return
before anything touches a GPU."""
import ctypes as C

import numpy as np
import pytest

from gen_adversarial_amd import _lib as L
from gen_adversarial_amd import noise as N


@pytest.mark.parametrize('counter, key, out', [
    ([0, 0, 0, 0], [0, 0], '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ([0xffffffff] * 4, [0xffffffff] * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], 'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_philox_known_answers(counter, key, out):
    got = N.philox4x32_10(np.array(counter, dtype=np.uint64), key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert ' '.join('%08x' % v for v in got) == out
    batch = N.philox4x32_10(np.array([counter, [0, 0, 0, 0]], dtype=np.uint64), key)       # leading dimensions are carried
    assert batch.shape == (2, 4) and np.array_equal(batch[0], got)


def test_counter_layout_of_reference_bits():
    """quad q of absolute row R: counter (q, R, stream, draw), key (seed low, seed high)"""
    seed, draw, stream, row0 = 0xDEADBEEF00000001, 0xFFFFFFFF, 0x80000001, (1 << 31) + 5
    bits = N.reference_bits(seed, draw, stream, row0, 3, 12)
    assert bits.dtype == np.uint32 and bits.shape == (3, 12)
    for r in range(3):
        for q in range(3):
            want = N.philox4x32_10(np.array([q, row0 + r, stream, draw], dtype=np.uint64), [0x00000001, 0xDEADBEEF])
            assert np.array_equal(bits[r, 4 * q:4 * q + 4], want)
    swapped = N.philox4x32_10(np.array([0, row0, stream, draw], dtype=np.uint64), [0xDEADBEEF, 0x00000001])
    assert not np.array_equal(bits[0, :4], swapped)
    assert N.STREAM_INPUT == L.GA_RANDN_STREAM_INPUT == 1 << 31


def test_rows_do_not_depend_on_how_they_are_cut():
    whole = N.reference_randn(7, 2, 1, 0, 8, 24)
    halves = np.concatenate([N.reference_randn(7, 2, 1, 0, 4, 24), N.reference_randn(7, 2, 1, 4, 4, 24)])
    assert whole.dtype == np.float64 and np.array_equal(whole.view(np.uint64), halves.view(np.uint64))
    for other in (N.reference_randn(8, 2, 1, 0, 8, 24), N.reference_randn(7, 3, 1, 0, 8, 24), N.reference_randn(7, 2, 0, 0, 8, 24),
                  N.reference_randn(7 + (1 << 32), 2, 1, 0, 8, 24)):
        assert not np.array_equal(whole, other)
    assert np.array_equal(N.reference_randn(7, 2, 1, 0, 8, 24, scale=0.8), 0.8 * whole)
    assert N.reference_randn(7, 2, 1, 0, 8, 24, dtype=np.float32).dtype == np.float32


def test_moments_and_range_of_the_reference_normals():
    """2^20 draws at a fixed seed; five-sigma bounds from n: sd(mean) = 1 / sqrt(n) = 9.8e-4, sd(var) = sqrt(2 / n) = 1.38e-3"""
    z = N.reference_randn(1234, 0, 0, 0, 1024, 1024)
    assert z.size == 1 << 20
    print(f'   mean {z.mean():.3e}, var - 1 {z.var() - 1:.3e}, max |z| {np.abs(z).max():.4f}')
    assert abs(z.mean()) <= 4.9e-3
    assert abs(z.var() - 1.0) <= 6.9e-3
    assert np.abs(z).max() <= 5.768 + 1e-6          # sqrt(-2 ln 2^-24) = 5.7677


def test_uniforms_lie_strictly_inside_the_unit_interval():
    u = N.reference_uniforms(N.reference_bits(5, 0, 0, 0, 256, 1024))
    assert u.min() > 0.0 and u.max() < 1.0
    edge = N.reference_uniforms(np.array([0, 0x1ff, 0x200, 0xffffffff], dtype=np.uint32))
    assert edge.tolist() == [2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -24, 1.0 - 2.0 ** -24]
    assert np.array_equal(edge.astype(np.float32).astype(np.float64), edge)         # every uniform is an fp32 number


def test_reference_refuses_what_the_library_refuses():
    for args in ((0, 0, 0, 0, 2, 6), (0, 0, 0, 0, 0, 4), (0, 0, 0, (1 << 32) - 1, 2, 4)):
        with pytest.raises(ValueError):
            N.reference_bits(*args)
    assert N.reference_bits(0, 0, 0, (1 << 32) - 2, 2, 4).shape == (2, 4)


ARGS = ['y', 'rows', 'inner', 'seed', 'draw', 'tensor', 'row0', 'scale', 'mode', 'coef', 'coef_eps', 'ws', 'ws_floats', 'stream']


def _call(**kw):
    a = dict(y=4096, rows=2, inner=8, seed=1, draw=0, tensor=0, row0=0, scale=1.0, mode=0, coef=None, coef_eps=0.0, ws=None, ws_floats=0,
             stream=None)           # well-formed (never launched: every case below is refused)
    a.update(kw)
    return L.lib.ga_randn(*(a[k] for k in ARGS))


def test_ga_randn_is_declared_exported_and_bound():
    assert 'ga_randn' in L.EXPORTS and L.lib.ga_randn is not None
    fn = L.lib.ga_randn
    V = C.c_void_p
    assert fn.restype is C.c_int
    assert fn.argtypes == [V, C.c_long, C.c_long, C.c_ulong, C.c_uint, C.c_uint, C.c_ulong, C.c_float, C.c_int, V, C.c_float, V, C.c_long, V]
    assert fn.argtypes[-1] is C.c_void_p                                                   # a pointer-sized stream
    assert C.sizeof(L.Op) == L.lib.ga_sizeof_op() == 288 and len(L._H.ops) == 30           # not a plan op: ga_op is untouched


@pytest.mark.parametrize('kw, code', [
    (dict(inner=6), 'GA_E_UNSUPPORTED'),                                     # inner % 4 != 0
    (dict(rows=0), 'GA_E_BADARG'),
    (dict(rows=-3), 'GA_E_BADARG'),
    (dict(y=None), 'GA_E_BADARG'),
    (dict(inner=0), 'GA_E_BADARG'),
    (dict(row0=(1 << 32) - 1), 'GA_E_BADARG'),                               # row0 + rows = 2^32 + 1
    (dict(row0=1 << 63), 'GA_E_BADARG'),
    (dict(mode=2), 'GA_E_BADARG'),
    (dict(coef=8192), 'GA_E_BADARG'),                                        # coef without ws
    (dict(coef=8192, ws=16384, ws_floats=1), 'GA_E_BADARG'),                 # two rows need two partial sums
    (dict(coef=8192, ws=16384, ws_floats=2, inner=2048), 'GA_E_BADARG'),     # 512 quads per row: two workgroups per row, four sums
    (dict(coef=8192, ws=16384, ws_floats=2, mode=1), 'GA_E_BADARG'),         # the raw words have no norm
    (dict(y=4100), 'GA_E_ALIGN'),                                            # 16-byte stores
])
def test_bad_arguments_are_rejected_without_a_gpu(kw, code):
    assert _call(**kw) == getattr(L, code) < 0


class _Owner:
    def __init__(self):
        self.calls, self.state = [], None

    def seeded_noise(self, seed, draw=0, first_row=0):
        self.state = None if seed is None else (seed, draw, first_row)

    def __call__(self, x):
        self.calls.append((self.state, x.shape[0]))
        return x.flatten(1)[:, :3]


class _Wrapped:
    def __init__(self, eot):
        self.model, self.eot_steps = _Owner(), eot

    def __call__(self, x):
        return self.model(x)


def _attack(batched):
    def run(x, y, net):
        net(x)
        if batched:
            return (True, 0.5, x) if x.shape[0] == 1 else ([True] * x.shape[0], [0.5] * x.shape[0], x)
        return True, 0.25, x
    run.batched = batched
    return run


@pytest.mark.parametrize('bi', [1, 2])
def test_the_seeded_driver_restarts_the_draws_at_each_images_own_row(bi):
    """experiments/seeded_defense.evaluate_seeded on a stub defender: every call is made at draw 0 with first_row = (dataset index) x EoT of
    each of its images, and the table has test_defense.evaluate_shard's columns"""
    import torch
    from gen_adversarial_amd.experiments.seeded_defense import evaluate_seeded
    model, index = _Wrapped(4), [1, 3, 5]                        # rank 1 of 2: images 1, 3, 5 of the dataset
    x, y = torch.rand(3, 3, 2, 2), torch.zeros(3, dtype=torch.long)
    table = evaluate_seeded(model, {'one': _attack(False), 'many': _attack(True)}, x, y, lambda i: index[i], seed=9, batch_images=bi)
    assert table.shape == (3, 3) and table[:, 1].tolist() == [0.25] * 3 and table[:, 2].tolist() == [0.5] * 3
    assert model.model.state is None                              # torch's draws again afterwards
    if bi == 1:         # per image: one restart at the image's own row, then clean pass and both attacks
        assert model.model.calls == [((9, 0, [4 * i]), 1) for i in index for _ in range(3)]
    else:               # per batch: every image at its own row, clean + the batched attack; then per image the one-image attack
        assert model.model.calls == [((9, 0, [4, 12]), 2), ((9, 0, [4, 12]), 2), ((9, 0, 4), 1), ((9, 0, 12), 1),
                                     ((9, 0, [20]), 1), ((9, 0, [20]), 1), ((9, 0, 20), 1)]
