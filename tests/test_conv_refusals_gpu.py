"""What ga_conv2d answers on the host: GA_OK, GA_E_BADARG or GA_E_UNSUPPORTED for every tile code, on the smallest descriptors that
reach each branch of the validation, of the operand classes (vec_out, bf3), of split-K and of every family's check.

ROWS is a literal table (shape, tweaks, tile, splits) -> return code RECORDED BY RUNNING THE LIBRARY OF COMMIT b16f351 (the parent
of the commit that moved the host path into csrc/conv2d.hip and gave every kernel family one conv_<family>_check): it pins the
codes of that library, not what anybody thinks they should be.  A host refactor has to reproduce the table unchanged.

Every row is a descriptor the library is specified to accept or refuse on the host.  Accepted rows launch on tensors of a few KB
and must write every output element; refused rows must leave y untouched.
"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip('needs a GPU', allow_module_level=True)

from gen_adversarial_amd import _lib as L  # noqa: E402
from gen_adversarial_amd.engine_core import WeightStore  # noqa: E402

DEV = 'cuda:0'
CODE = {v: k for k, v in L.ERRORS.items()}
OK, BAD, UNS = 'GA_OK', 'GA_E_BADARG', 'GA_E_UNSUPPORTED'

# shape name -> (N, H, W, Cin, Cout, k): 3x3 / pad 1 or 1x1 / pad 0, stride 1
SHAPES = {
    'q32c64': (32, 4, 4, 64, 32, 3), 'q8c64': (8, 4, 4, 64, 32, 3), 'q40c64': (40, 4, 4, 64, 32, 3), 'q8c96': (8, 4, 4, 96, 32, 3),
    'r32': (8, 8, 16, 32, 32, 3), 'r48': (8, 8, 16, 48, 32, 3), 'r64': (8, 8, 16, 64, 32, 3), 'r96': (8, 8, 16, 96, 32, 3),
    'w32': (1, 16, 64, 32, 32, 3), 'w96': (1, 16, 64, 96, 32, 3),
    'p32': (8, 4, 4, 32, 32, 1), 'p64': (8, 4, 4, 64, 32, 1), 'p40': (8, 4, 4, 40, 32, 1),         # 1x1, 128 pixels
    'p32m80': (5, 4, 4, 32, 32, 1), 'p40m80': (5, 4, 4, 40, 32, 1),                              # 1x1, 80 pixels
}
# tweaks: 'frag' = w_frag in the tile's own order, 'frag+4' = the same 4 bytes on, 'y+4' = y 4 bytes off a 16-byte boundary,
# 'scale_only' = pro_scale without pro_shift, 'sd3' = transposed stride 3, 'no_hi' = no split weights, 'no_ws' = split-K without a workspace
ROWS = [
    # tile 0: the heuristic
    ('q32c64', (), 0, 1, OK), ('p40m80', (), 0, 1, OK), ('q32c64', ('scale_only',), 0, 1, BAD), ('q32c64', ('sd3',), 0, 1, UNS),
    # tiles 1 - 4: split-bf16 kernel, or the fp32 kernel without w_hi (the family fallback); scalar epilogue for a misaligned y
    ('r32', (), 1, 1, OK), ('r48', (), 2, 1, OK), ('w96', (), 3, 1, OK), ('q40c64', (), 4, 1, OK),
    ('r32', ('no_hi',), 1, 1, OK), ('r48', ('no_hi',), 2, 1, OK), ('w96', ('no_hi',), 3, 1, OK), ('q40c64', ('no_hi',), 4, 1, OK),
    ('r32', ('y+4',), 1, 1, OK), ('r32', ('y+4', 'no_hi'), 1, 1, OK), ('r64', (), 1, 2, OK), ('q8c96', (), 3, 64, OK),
    ('r32', ('scale_only',), 1, 1, BAD), ('r48', ('no_ws',), 2, 2, BAD), ('w96', ('scale_only',), 3, 1, BAD), ('q40c64', ('scale_only',), 4, 1, BAD),
    ('r32', ('sd3',), 1, 1, UNS), ('r48', ('sd3',), 2, 1, UNS), ('w96', ('sd3',), 3, 1, UNS), ('q40c64', ('sd3',), 4, 1, UNS),
    # tiles 5 - 7: LDS-staged halo kernel
    ('r64', (), 5, 2, OK), ('w32', (), 6, 1, OK), ('q8c96', (), 7, 1, OK),
    ('r48', (), 5, 1, UNS), ('r64', ('no_hi',), 5, 1, UNS), ('w32', (), 6, 2, UNS), ('q8c64', (), 6, 64, UNS), ('q8c96', ('y+4',), 7, 1, UNS),
    ('p32', (), 7, 1, UNS),
    ('r64', ('scale_only',), 5, 1, BAD), ('w32', ('no_ws',), 6, 2, BAD), ('q8c96', ('scale_only',), 7, 1, BAD),
    # tile 8: weight fragments from w_frag
    ('r64', ('frag',), 8, 1, OK), ('q40c64', ('frag',), 8, 2, OK), ('r64', (), 8, 1, UNS), ('r64', ('frag+4',), 8, 1, UNS),
    ('r48', ('frag',), 8, 1, UNS), ('r64', ('frag', 'scale_only'), 8, 1, BAD),
    # tile 9: quadrant tile, 4 x 4 images in groups of 32 (or one partial group)
    ('q32c64', ('frag',), 9, 1, OK), ('q8c64', ('frag',), 9, 2, OK), ('q40c64', ('frag',), 9, 1, UNS), ('r64', ('frag',), 9, 1, UNS),
    ('q32c64', (), 9, 1, UNS), ('q8c64', ('frag',), 9, 64, UNS), ('q32c64', ('frag', 'y+4'), 9, 1, UNS), ('q32c64', ('frag', 'scale_only'), 9, 1, BAD),
    # tile 10 (retired) and 13 (never assigned)
    ('r32', (), 10, 1, UNS), ('r32', ('scale_only',), 10, 1, BAD), ('r32', (), 13, 1, UNS), ('r32', ('scale_only',), 13, 1, BAD),
    # tile 11: persistent thin kernel, 32 or 64 input channels, 8 x 16 tiles
    ('r32', ('frag',), 11, 1, OK), ('r64', ('frag',), 11, 1, OK), ('w32', ('frag',), 11, 1, OK),
    ('r96', ('frag',), 11, 1, UNS), ('r48', (), 11, 1, UNS), ('q32c64', ('frag',), 11, 1, UNS), ('r64', ('frag',), 11, 2, UNS),
    ('r32', (), 11, 1, UNS), ('r32', ('frag+4',), 11, 1, UNS), ('r32', ('frag', 'no_hi'), 11, 1, UNS), ('r32', ('frag', 'scale_only'), 11, 1, BAD),
    # tile 12: 1x1 with the fragments from w_frag (or gathered from w_hi / w_lo without it); a split-K factor is clamped to the K tiles first
    ('p32', ('frag',), 12, 1, OK), ('p32', (), 12, 1, OK), ('p32', ('frag',), 12, 2, OK), ('p64', ('frag',), 12, 2, UNS),
    ('p32', ('frag+4',), 12, 1, UNS), ('p32m80', ('frag',), 12, 1, UNS), ('p40', (), 12, 1, UNS), ('r32', (), 12, 1, UNS),
    ('p32', ('frag', 'y+4'), 12, 1, UNS), ('p32', ('frag', 'sd3'), 12, 1, UNS), ('p32', ('frag', 'scale_only'), 12, 1, BAD),
]


def _row(shape, tweaks, tile, splits):
    """(descriptor, y as the descriptor addresses it, keep-alive list)"""
    N, H, W, Cin, Cout, k = SHAPES[shape]
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(N, H, W, Cin, device=DEV, generator=g)
    w = torch.randn(Cout, k * k * Cin, device=DEV, generator=g) * (k * k * Cin) ** -0.5
    store = WeightStore(DEV)
    hi, lo = store.split(w)
    ybuf = torch.full((N * H * W * Cout + 4,), float('nan'), device=DEV)
    y = ybuf[1:1 + N * H * W * Cout] if 'y+4' in tweaks else ybuf[:N * H * W * Cout]
    keep = [x, w, hi, lo, store, ybuf]
    d = L.ConvDesc()
    d.N, d.Hi, d.Wi, d.Ho, d.Wo, d.C1, d.Cout, d.KH, d.KW, d.sn, d.sd, d.pad = N, H, W, H, W, Cin, Cout, k, k, 1, 1, k // 2
    d.ldx, d.ldy, d.tile, d.splits = Cin, Cout, tile, splits
    d.x, d.w, d.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
    if 'no_hi' not in tweaks:
        d.w_hi, d.w_lo = hi.data_ptr(), lo.data_ptr()
    if 'frag' in tweaks or 'frag+4' in tweaks:
        if tile == 11 and k == 3 and Cin in (32, 64):
            frag = store.frag_thin(w)
        elif k == 1 or Cin % 32 == 0:
            frag = store.frag3(w, taps=k * k)
        else:                                                        # no such layout: the row is refused on its shape, any buffer does
            frag = torch.zeros(2 * w.numel(), dtype=torch.bfloat16, device=DEV)
        frag = torch.cat([frag.flatten(), frag.new_zeros(8)])       # room for the misaligned view
        keep.append(frag)
        d.w_frag = frag.data_ptr() + (4 if 'frag+4' in tweaks else 0)
    if 'scale_only' in tweaks:
        keep.append(torch.ones(Cin, device=DEV))
        d.pro_scale = keep[-1].data_ptr()
    if 'sd3' in tweaks:
        d.sd = 3
    if splits > 1 and 'no_ws' not in tweaks:
        keep.append(torch.empty(splits * N * H * W * Cout, device=DEV))
        d.ws, d.ws_floats = keep[-1].data_ptr(), keep[-1].numel()
    return d, y, keep


def test_the_table_covers_every_code_of_every_tile():
    for tile in range(13):
        want = {OK, BAD, UNS} - ({OK} if tile == 10 else set())
        assert {r[4] for r in ROWS if r[2] == tile} == want, tile
    assert len(set(r[:4] for r in ROWS)) == len(ROWS)


@pytest.mark.parametrize('shape,tweaks,tile,splits,expect', ROWS,
                         ids=[f'{s}-{"+".join(t) or "plain"}-tile{tl}-s{sp}' for s, t, tl, sp, _ in ROWS])
def test_ga_conv2d_return_code(shape, tweaks, tile, splits, expect):
    d, y, _keep = _row(shape, tweaks, tile, splits)
    rc = L.lib.ga_conv2d(C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    print(f'ROW {shape} {"+".join(tweaks) or "plain"} tile {tile} splits {splits}: {L.ERRORS.get(rc, rc)}', flush=True)
    assert L.ERRORS.get(rc, rc) == expect
    if rc == CODE[OK]:
        assert torch.isfinite(y).all()
    else:
        assert torch.isnan(y).all()
