"""
Large extents: every non-conv op of include/ga_ops.h with its largest row-indexed operand past the offsets where 32-bit index
arithmetic wraps.  The shipped plans hold such tensors (configs[2]: [32, 1024^2, 32] fp32 = 2^32 bytes) and every other test of
these ops stays within a few MB.

Method (tests/bigrows.py): one descriptor at N rows runs once over the whole tensors and once over consecutive row chunks whose
every operand spans less than 2^30 bytes, the host advancing the pointers in 64-bit arithmetic; rows are independent in every op
here (ga_ops.h says so op by op).  Outputs and workspaces start as NaN bits, inputs come from a seeded device generator.  Asserted:
  - every output float of the one launch has the bits of the chunked result (int32 views, compared in slices of 2^28 elements);
  - no element the header says is written is NaN;
  - 256 guard floats behind every buffer keep their bits, and every input regenerates from its seed bit for bit;
  - the first chunk (the least legal row count) of the chunked launches is within opref.bound() of planref's float64 reference.
Chunk boundaries are multiples of the replica fields' lcm (planref's least_rows).  ga_rowchan_reduce's `ws` split and ga_modout's
`red` pick their segments per row from N: each chunk gets the workspace size that keeps the big launch's segments (bigrows.
chunk_fields), after which the order of every sum is the same and the comparison is bitwise there too -- no op is compared under a
bound.

Tiers, crossed by the op's largest row-indexed operand by two whole rows: T1 > 2^31 bytes, T2 > 2^32 bytes, T3 > 2^31 elements.
Every case runs at T2, and at T3 wherever its buffers fit the 48 GB a test may take (_tiers).  Four kinds do not (NO_T3, asserted by
test_the_cases_without_t3): ga_dec_cell_halo backward with both addends (50.0 GB), ga_interleave2 with lds = 4C (four source planes of the output's size, 51.5 GB at T3), ga_sampler_mix mode 1
backward (48.2 GB) and ga_attn backward (76.6 GB: q, k, v, p, dout and two copies each of ds, dq, dk, dv).  The tier column below names
the tiers an entry point reaches with at least one mode.

  entry point            tier   modes
  ga_modout              T2 T3  forward; backward dt; backward dt + red; t_planes / dt_planes + red (plan shapes 1024^2 x 32, 512^2 x 64)
  ga_rowchan_reduce      T2 T3  one stage ab; two stages ab; gate / skip / scaled; a_src / a_w (with and without scaled)
  ga_up2_blur            T2 T3  forward (accumulating), backward
  ga_pool_denorm         T2 T3  forward with band; backward with dy_nchw and band
  ga_interleave2         T2 T3  the pitch of planes that are slices, lds = 4C (T2 only); dact_x / scale / shift / addend with dact_rep
  ga_image_io            T2 T3  forward with noise, rep and pitch; space-to-depth; backward with rep and cot_rep
  ga_se_apply            T2 T3  skip modes 0, 1, 2
  ga_se_excite           T2 T3  fused forward with out; fused backward with act_rep
  ga_bilinear_up2_bwd    T2 T3  accumulating
  ga_sampler_mix         T2 T3  mode 0 forward (eps_nchw, q_rep, alpha_rows), backward (act_rep, q_rep); mode 1 both; mode 2
  ga_dml_mean            T2 T3  forward with ld_img; backward with act_rep
  ga_maxpool2            T2 T3  forward; backward with act_rep
  ga_maxpool3s2          T2 T3  forward; backward with act_rep
  ga_avgpool_act         T2 T3  forward; backward with act_rep
  ga_gconv               T2 T3  the group kernel (cg = 4) and the generic kernel (cg = 12), dact_rep; the other side of the host's
                                npix < (2^31 - 1) * 256 switch needs 2^39 pixels and no memory holds them
  ga_gauss_blur          T2 T3  one pass and two passes, forward and adjoint
  ga_prelu               T2 T3  forward; backward
  ga_unary               T2 T3  modes 0, 1, 2, 3
  ga_axpby               T2 T3  beta = 0 and beta != 0
  ga_rep_sum             T2 T3  written and accumulating
  ga_pixelnorm           T2 T3
  ga_latent_mix          T2 T3  backward 0 (shared and per-row alpha), 1, 2, all with rep
  ga_layernorm           T2 T3  forward; backward accumulating
  ga_attn                T2 T3  forward and backward, dh = 16 so that p / ds are as large as k
  ga_resize2_crop        T2 T3  forward; backward
  ga_avae                T2 T3  ADAIN, AVGPOOL, PIXELNORM, SAMPLE, forward and backward (act_rep)
  ga_dwconv5             T2 T3  plain, 4 x 4, flipped with pool2 / dact_x / act_rep, up2
  ga_conv2d              conv: tests/test_conv_large_extent_gpu.py (every family at and past 2 GB; tests/convbig.py)
  ga_dec_cell            T2 T3  every accepted (H, W, C) class (cellref.GEOMS) at Hd = 32 (one hidden chunk) and 96 (three), one per C at the
                                shipped Hd = 6 C; forward, backward with act_rep; variant 1 at every C = 128 class with Hd = 96.
                                Operand table: bigrows.CellModel; the first chunk is held to cellref's row-wise bound
  ga_dec_cell_halo       T2 T3  the image sizes of cellref.HALO_CASES for C = 32 and 64, Hd = 96; forward, backward with an addend; with
                                addend and addend2 at 16 x 32 (T2 only)
  ga_split_bf16          T2 T3  no descriptor: test_split_bf16_equals_its_chunks, the bf16 outputs compared as int16 bits
  ga_randn, ga_nes_*, ga_square_*   rows with the high bit set: tests/test_noise_gpu.py, test_nes_gpu.py, test_square_gpu.py
  ga_plan_*, ga_graph_*, ga_microbench_*, ga_debug_*, ga_abi_version, ga_sizeof_op, ga_last_hip_error   no tensor indexing of their own

test_comparison_sees_a_wrapped_row hands the comparison an expected tensor in which the rows past each tier's boundary hold what a
32-bit offset would have addressed (bigrows.wrapped_row; an address before the tensor counts as the row never written: NaN bits)
and asserts that the equality fails at exactly the first such row.  test_refusals pins the lines the library draws itself, the
grid limits of ga_avgpool_act, ga_rowchan_reduce and ga_modout's `red` among them.

Every case needs at most 48 GB of device memory and skips, with its reason, where less is free; it never shrinks.
Call times (profiles/large_extent_gpu.log, --durations=0): 336 of 351 calls below 5 s; 15 fused-cell cases took 5.1 - 6.6 s in that
run although each already has the smallest N that crosses its boundary by two rows and the same cases take 0.05 - 0.3 s at the other
tier: the time is not the kernels' and has not been attributed.
"""
import os
import sys
import time

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')]      # collects without one

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bigrows as B                                                      # noqa: E402
from gen_adversarial_amd import _lib as L                                # noqa: E402

DEV = 'cuda:0'
SILU, RELU, FLRELU = L.GA_ACT_SILU, L.GA_ACT_RELU, L.GA_ACT_FLRELU
G = dict(H=24, W=28, C=36)               # 24192 floats per row: no divisor of 2^32, a wrapped address lands mid-row
GP = dict(P=24 * 28, C=36)
PL4 = lambda n: {f'{n}{i}' for i in range(4)}                            # noqa: E731
SMP = dict(h=16, w=18, NL=20, ldq=44, ldp=44, ldz=24, alpha=0.3, one_minus_alpha=0.7, temp=0.8)
LM = dict(J=18, D=516, rep=2)
AT = dict(Tq=16, Tk=200, heads=4, dh=16, scale=0.25, ldq=64, ldk=64, ldv=64, ldo=64, lddq=64, lddk=64, lddv=64)

# (family, mode, descriptor class, fields, pointers, workspace segments per row); the tiers: _tiers
CASES = [
    ('modout', 'fwd', L.ModoutDesc, dict(P=1 << 20, C=32, act=FLRELU), {'t', 'scale', 'add', 'out'}, 0),
    ('modout', 'bwd dt', L.ModoutDesc, dict(P=1 << 18, C=64, act=FLRELU, backward=1), {'t', 'scale', 'add', 'dout', 'dt'}, 0),
    ('modout', 'bwd dt red', L.ModoutDesc, dict(P=1 << 18, C=64, act=FLRELU, backward=1), {'t', 'scale', 'add', 'dout', 'dt', 'red', 'ws'}, 8),
    ('modout', 'bwd planes red', L.ModoutDesc, dict(P=1 << 20, C=32, W=1024, act=FLRELU, backward=1),
     PL4('t_planes') | PL4('dt_planes') | {'scale', 'add', 'dout', 'red', 'ws'}, 16),
    ('modout', 'fwd t_planes', L.ModoutDesc, dict(P=1 << 18, C=64, W=512, act=FLRELU), PL4('t_planes') | {'scale', 'add', 'out'}, 0),
    ('reduce', 'one stage ab', L.ReduceDesc, dict(scale=0.5, **GP), {'a', 'b', 'out'}, 0),
    ('reduce', 'two stages ab', L.ReduceDesc, dict(P=1 << 20, C=32, scale=1.0), {'a', 'b', 'out', 'ws'}, 16),
    ('reduce', 'gate skip scaled', L.ReduceDesc, dict(P=1 << 18, C=64, scale=1.0), {'a', 'out', 'gate', 'skip', 'scaled', 'ws'}, 8),
    ('reduce', 'a_src a_w', L.ReduceDesc, dict(P=1 << 20, C=32, scale=1.0), {'a_src', 'a_w', 'b', 'out', 'ws'}, 16),
    ('reduce', 'a_src a_w scaled', L.ReduceDesc, dict(P=1 << 20, C=32, scale=1.0), {'a_src', 'a_w', 'out', 'gate', 'scaled', 'ws'}, 16),
    ('up2_blur', 'fwd', L.Up2BlurDesc, dict(H=512, W=512, C=4), {'lo_in', 'hi'}, 0),
    ('up2_blur', 'bwd', L.Up2BlurDesc, dict(H=512, W=512, C=4, backward=1), {'hi_in', 'lo'}, 0),
    ('pool_denorm', 'fwd band', L.PoolDenormDesc, dict(H=256, W=256, k=4, ld=4, band=32), {'x', 'y'}, 0),
    ('pool_denorm', 'bwd dy_nchw band', L.PoolDenormDesc, dict(H=256, W=256, k=4, ld=4, band=32, backward=1), {'dy', 'dy_nchw', 'dx'}, 0),
    ('interleave2', 'lds=4C', L.Interleave2Desc, dict(H=1024, W=1024, C=32, lds=128), PL4('s') | {'y'}, 0),
    ('interleave2', 'dact addend', L.Interleave2Desc, dict(H=120, W=136, C=36, dact_act=SILU, dact_rep=2),
     PL4('s') | {'y', 'dact_x', 'dact_scale', 'dact_shift', 'addend'}, 0),
    ('image_io', 'fwd noise rep', L.ImageIoDesc, dict(C=3, H=224, W=224, rep=2, ld=4), {'x_nchw', 'noise_nchw', 'noise_coef', 'y_nhwc'}, 0),
    ('image_io', 'fwd s2d', L.ImageIoDesc, dict(C=3, H=224, W=224, rep=2, ld=4, s2d=1), {'x_nchw', 'noise_nchw', 'noise_coef', 'y_nhwc'}, 0),
    ('image_io', 'bwd rep cot_rep', L.ImageIoDesc, dict(C=3, H=224, W=224, rep=2, ld=4, backward=1, cot_rep=2),
     {'x_nchw', 'noise_nchw', 'noise_coef', 'dy_nhwc', 'dx_nchw'}, 0),
    ('se', 'apply skip 0', L.SeApplyDesc, dict(skip_mode=0, res_scale=0.1, **G), {'skip', 't', 'gate', 'out'}, 0),
    ('se', 'apply skip 1', L.SeApplyDesc, dict(skip_mode=1, res_scale=0.1, **G), {'skip', 't', 'gate', 'out'}, 0),
    ('se', 'apply skip 2', L.SeApplyDesc, dict(skip_mode=2, res_scale=0.1, **G), {'skip', 't', 'gate', 'out'}, 0),
    ('se', 'excite fused fwd out', L.SeExciteDesc, dict(Hd=8, res_scale=0.1, **GP), {'t', 'w1', 'b1', 'w2', 'b2', 'hid', 'gate', 'skip', 'out'}, 0),
    ('se', 'excite fused bwd act_rep', L.SeExciteDesc, dict(Hd=8, res_scale=0.1, backward=1, act_rep=2, **GP),
     {'t', 'w1', 'b1', 'w2', 'b2', 'hid', 'gate', 'dout', 'pro_scale', 'pro_shift'}, 0),
    ('se', 'bilinear_up2_bwd', L.BilinearBwdDesc, dict(h=12, w=14, C=36, accumulate=1), {'dhigh', 'dlow'}, 0),
    ('sampler', 'mode 0 fwd', L.SamplerDesc, dict(eps_nchw=1, q_rep=2, alpha_ld=4, alpha_col=1, **SMP), {'mu_q', 'p', 'eps', 'z', 'alpha_rows'}, 0),
    ('sampler', 'mode 0 bwd', L.SamplerDesc, dict(eps_nchw=1, q_rep=2, act_rep=2, backward=1, **SMP), {'mu_q', 'p', 'eps', 'dz', 'dmu_q_rows', 'dp'}, 0),
    ('sampler', 'mode 1 fwd', L.SamplerDesc, dict(mode=1, **SMP), {'mu_q', 'p', 'eps', 'z'}, 0),
    ('sampler', 'mode 1 bwd', L.SamplerDesc, dict(mode=1, backward=1, act_rep=2, **SMP), {'mu_q', 'p', 'eps', 'dz', 'dmu_q', 'dp'}, 0),
    ('sampler', 'mode 2', L.SamplerDesc, dict(mode=2, backward=1, q_rep=2, alpha_ld=3, alpha_col=1, **SMP), {'mu_q', 'p', 'eps', 'dz', 'z'}, 0),
    ('dml', 'fwd ld_img', L.DmlDesc, dict(ld=100, nmix=10, H=16, W=18, ld_img=4), {'logits', 'img_nchw', 'img_nhwc'}, 0),
    ('dml', 'bwd act_rep', L.DmlDesc, dict(ld=100, nmix=10, H=16, W=18, ld_img=4, backward=1, act_rep=2), {'logits', 'dimg_nhwc', 'dimg_nchw', 'dlogits'}, 0),
    ('pool', 'maxpool2 fwd', L.MaxpoolDesc, dict(**G), {'x', 'y'}, 0),
    ('pool', 'maxpool2 bwd act_rep', L.MaxpoolDesc, dict(backward=1, act_rep=2, **G), {'x', 'dy', 'dx'}, 0),
    ('pool', 'maxpool3s2 fwd', L.Maxpool3s2Desc, dict(**G), {'x', 'y'}, 0),
    ('pool', 'maxpool3s2 bwd act_rep', L.Maxpool3s2Desc, dict(backward=1, act_rep=2, **G), {'x', 'dy', 'dx'}, 0),
    ('pool', 'avgpool_act fwd', L.AvgpoolActDesc, dict(act=RELU, **GP), {'x', 'y'}, 0),
    ('pool', 'avgpool_act bwd act_rep', L.AvgpoolActDesc, dict(act=RELU, backward=1, act_rep=2, **GP), {'x', 'dy', 'dx'}, 0),
    ('gconv', 'group kernel cg=4', L.GconvDesc, dict(N=0, Hi=24, Wi=28, Ho=24, Wo=28, C=36, cg=4, KH=3, KW=3, stride=1, pad=1, pro_act=RELU, dact_act=RELU, dact_rep=2),
     {'x', 'w', 'bias', 'dact_x', 'y'}, 0),
    ('gconv', 'generic kernel cg=12', L.GconvDesc, dict(N=0, Hi=24, Wi=28, Ho=24, Wo=28, C=36, cg=12, KH=3, KW=3, stride=1, pad=1, pro_act=RELU, dact_act=RELU, dact_rep=2),
     {'x', 'w', 'bias', 'dact_x', 'y'}, 0),
    ('gauss_blur', 'one pass', L.BlurDesc, dict(H=48, W=52, k=7), {'x', 'y', 'taps'}, 0),
    ('gauss_blur', 'one pass adjoint', L.BlurDesc, dict(H=48, W=52, k=7, backward=1), {'x', 'y', 'taps'}, 0),
    ('gauss_blur', 'two passes', L.BlurDesc, dict(H=128, W=136, k=15, radius=5), {'x', 'y', 'taps', 'tmp'}, 0),
    ('gauss_blur', 'two passes adjoint', L.BlurDesc, dict(H=128, W=136, k=15, radius=5, backward=1), {'x', 'y', 'taps', 'tmp'}, 0),
    ('flat', 'prelu fwd', L.PreluDesc, dict(C=516), {'x', 'slope', 'y'}, 0),
    ('flat', 'prelu bwd', L.PreluDesc, dict(C=516, backward=1), {'x', 'slope', 'dy', 'dx'}, 0),
    ('flat', 'unary 0', L.UnaryDesc, dict(mode=0), {'x', 'y'}, 0),
    ('flat', 'unary 1', L.UnaryDesc, dict(mode=1), {'x', 'g', 'y'}, 0),
    ('flat', 'unary 2', L.UnaryDesc, dict(mode=2, eps=1e-8), {'x', 'y'}, 0),
    ('flat', 'unary 3', L.UnaryDesc, dict(mode=3), {'x', 'g', 'y'}, 0),
    ('flat', 'axpby beta=0', L.AxpbyDesc, dict(alpha=0.5, beta=0.0), {'x', 'y'}, 0),
    ('flat', 'axpby beta', L.AxpbyDesc, dict(alpha=0.5, beta=0.25), {'x', 'y'}, 0),
    ('flat', 'rep_sum', L.RepSumDesc, dict(inner=24192, rep=2), {'x', 'y'}, 0),
    ('flat', 'rep_sum accumulate', L.RepSumDesc, dict(inner=24192, rep=2, accumulate=1), {'x', 'y'}, 0),
    ('flat', 'pixelnorm', L.PixelnormDesc, dict(C=516), {'x', 'y'}, 0),
    ('latent', 'mix fwd', L.LatentMixDesc, dict(**LM), {'codes', 'avg', 'styles', 'alpha', 'out'}, 0),
    ('latent', 'mix fwd alpha_ld', L.LatentMixDesc, dict(alpha_ld=20, **LM), {'codes', 'avg', 'styles', 'alpha', 'out'}, 0),
    ('latent', 'mix bwd 1', L.LatentMixDesc, dict(backward=1, **LM), {'dout', 'alpha', 'dcodes'}, 0),
    ('latent', 'mix bwd 1 alpha_ld', L.LatentMixDesc, dict(backward=1, alpha_ld=20, **LM), {'dout', 'alpha', 'dcodes'}, 0),
    ('latent', 'mix bwd 2', L.LatentMixDesc, dict(backward=2, **LM), {'codes', 'avg', 'styles', 'dout', 'out'}, 0),
    ('trans', 'layernorm fwd', L.LayernormDesc, dict(C=516, eps=1e-5), {'a', 'b', 'gamma', 'beta', 'y', 'stats'}, 0),
    ('trans', 'layernorm bwd accumulate', L.LayernormDesc, dict(C=516, eps=1e-5, backward=1, accumulate=1), {'a', 'b', 'gamma', 'stats', 'dy', 'dx'}, 0),
    ('trans', 'attn fwd', L.AttnDesc, dict({k: v for k, v in AT.items() if not k.startswith('ldd')}), {'q', 'k', 'v', 'out', 'p'}, 0),
    ('trans', 'attn bwd', L.AttnDesc, dict(backward=1, **AT), {'q', 'k', 'v', 'p', 'dout', 'ds', 'dq', 'dk', 'dv'}, 0),
    ('trans', 'resize2_crop fwd', L.Resize2CropDesc, dict(crop=4, **G), {'x', 'y'}, 0),
    ('trans', 'resize2_crop bwd accumulate', L.Resize2CropDesc, dict(crop=4, backward=1, accumulate=1, **G), {'dy', 'dx'}, 0),
    ('avae', 'adain fwd', L.AvaeDesc, dict(mode=0, **GP), {'x', 'a', 'b', 'c', 'y', 'y2'}, 0),
    ('avae', 'adain bwd act_rep', L.AvaeDesc, dict(mode=0, backward=1, act_rep=2, **GP), {'x', 'a', 'b', 'c', 's', 'dy', 'y', 'y2'}, 0),
    ('avae', 'avgpool fwd', L.AvaeDesc, dict(mode=1, k=2, **G), {'x', 'y'}, 0),
    ('avae', 'avgpool bwd', L.AvaeDesc, dict(mode=1, k=2, backward=1, **G), {'x', 'dy', 'y'}, 0),
    ('avae', 'pixelnorm fwd', L.AvaeDesc, dict(mode=2, C=516), {'x', 'y'}, 0),
    ('avae', 'pixelnorm bwd act_rep', L.AvaeDesc, dict(mode=2, C=516, backward=1, act_rep=2), {'x', 'dy', 'y'}, 0),
    ('avae', 'sample fwd', L.AvaeDesc, dict(mode=3, f0=0.5, **GP), {'x', 'a', 'y'}, 0),
    ('avae', 'sample bwd act_rep', L.AvaeDesc, dict(mode=3, f0=0.5, backward=1, act_rep=2, **GP), {'x', 'a', 'dy', 'y'}, 0),
    ('dwconv5', 'plain', L.DwDesc, dict(pro_act=SILU, **G), {'x', 'w', 'bias', 'y'}, 0),
    ('dwconv5', '4x4', L.DwDesc, dict(H=4, W=4, C=36, pro_act=SILU), {'x', 'w', 'bias', 'y'}, 0),
    ('dwconv5', 'flipped pool2 dact act_rep', L.DwDesc, dict(dact_act=SILU, pool2=1, act_rep=2, **G), {'x', 'w', 'dact_x', 'y'}, 0),
    ('dwconv5', 'flipped dact act_rep', L.DwDesc, dict(dact_act=SILU, act_rep=2, **G), {'x', 'w', 'dact_x', 'y'}, 0),
    ('dwconv5', 'up2', L.DwDesc, dict(up2=1, pro_act=SILU, **G), {'x', 'w', 'bias', 'y'}, 0),
]


def _cell_cases():
    """ga_dec_cell at every geometry class the library accepts (cellref.GEOMS, held to the library by tests/test_cellref_cpu.py), three
    hidden chunks, forward and backward with act_rep, plus the shipped hidden width 6 C; ga_dec_cell_halo at cellref.HALO_CASES'
    image sizes for both channel counts, forward and backward with an addend"""
    import cellref as CR
    base = {'x', 'w1_hi', 'w1_lo', 'b1', 'wd', 'bd', 'w2_hi', 'w2_lo', 'y'}
    bwd = base | {'wd_bwd', 'dout', 'pro_scale', 'pro_shift'}
    out = []
    for C in sorted(CR.GEOMS):
        for (H, W), Hd in [(g, Hd) for g in CR.GEOMS[C] for Hd in (32, 96)] + [(CR.GEOMS[C][0], 6 * C)]:
            for variant in ((0, 1) if C == 128 and Hd == 96 else (0,)):             # variant 1: eight waves, built for C = 128
                f = dict(H=H, W=W, C=C, Hd=Hd, variant=variant)
                v = ' variant 1' if variant else ''
                out.append(('dec_cell', f'fwd {H}x{W}x{C} Hd={Hd}{v}', L.DecCellDesc, f, base | {'b2'}, 0))
                out.append(('dec_cell', f'bwd act_rep {H}x{W}x{C} Hd={Hd}{v}', L.DecCellDesc, dict(f, backward=1, act_rep=2), bwd, 0))
    for H, W in sorted({c[1:3] for c in CR.HALO_CASES}):
        for C in (32, 64):
            f = dict(H=H, W=W, Cin=C, Cout=C, Hd=96)
            out.append(('dec_cell_halo', f'fwd {H}x{W}x{C}', L.DecCellHaloDesc, f, base | {'b2'}, 0))
            out.append(('dec_cell_halo', f'bwd addend {H}x{W}x{C}', L.DecCellHaloDesc, dict(f, backward=1), bwd | {'w1t_hi', 'w1t_lo', 'addend'}, 0))
            if (H, W) == (16, 32):                                                   # both addends: 50.0 GB at T3, so T2 only (NO_T3)
                out.append(('dec_cell_halo', f'bwd addend addend2 {H}x{W}x{C}', L.DecCellHaloDesc, dict(f, backward=1),
                            bwd | {'w1t_hi', 'w1t_lo', 'addend', 'addend2'}, 0))
    return out


CASES += _cell_cases()


def _tiers(c):
    """T2 always; T3 wherever the case fits the 48 GB a test may take (NO_T3 names the others)"""
    f = {k: v for k, v in c[3].items() if k != 'N'}
    fits = B.Case(c[1], c[2], f, c[4], 'T3', ws_segments=c[5]).device_bytes() <= B.MEMORY_CAP
    return ('T2', 'T3') if fits else ('T2',)


FAMILIES = sorted({c[0] for c in CASES})
PARAMS = [pytest.param(c, t, id=f'{c[0]}-{c[1].replace(" ", "_")}-{t}') for c in CASES for t in _tiers(c)]
NO_T3 = [f'{c[0]}: {c[1]}' for c in CASES if _tiers(c) == ('T2',)]


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    torch.cuda.empty_cache()


def _yardstick():
    from test_plan_ops_gpu import _yardstick as y                      # the fp32 yardsticks with the kernels' summation orders
    return y


def _need(nbytes, what):
    assert nbytes <= B.MEMORY_CAP, f'{what}: {nbytes / 2 ** 30:.1f} GB is above the 48 GB a test may take'
    free = torch.cuda.mem_get_info(0)[0]
    if free < nbytes:
        pytest.skip(f'{what}: needs {nbytes / 2 ** 30:.1f} GB of device memory, {free / 2 ** 30:.1f} GB are free')


@pytest.mark.parametrize('spec, tier', PARAMS)
def test_one_launch_equals_its_row_chunks(spec, tier):
    family, mode, cls, f, has, segs = spec
    f = {k: v for k, v in f.items() if k != 'N'}
    case = B.Case(f'{family}: {mode}', cls, f, has, tier, ws_segments=segs)
    _need(case.device_bytes(), case.label())
    t0 = time.perf_counter()
    run = B.Run(case, DEV)
    run.big()
    run.chunked()
    differ = run.compare()
    fails = [f'{k}: {n} floats of the one launch differ from the chunks, first in row {row}' for k, n, row in differ]
    for k in run.alt:
        if case.role(k) in ('out', 'inout'):
            for big in (False, True):
                n = run.written(k, big)
                if n:
                    fails.append(f'{k}: {n} written elements of the {"one launch" if big else "chunks"} are NaN')
    fails += run.guards() + run.inputs_unchanged()
    worst, bad = run.anchor(_yardstick())
    fails += bad
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f'\n  {case.label()} chunks={len(case.chunks())} {"MISMATCH" if differ else "bitwise"}, first chunk err / bound {worst:.3f}, {dt:.2f} s', flush=True)
    del run
    assert not fails, case.label() + '\n' + '\n'.join(fails)


def test_the_cases_without_t3():
    assert NO_T3 == ['interleave2: lds=4C', 'sampler: mode 1 bwd', 'trans: attn bwd',
                     'dec_cell_halo: bwd addend addend2 16x32x32', 'dec_cell_halo: bwd addend addend2 16x32x64']


@pytest.mark.parametrize('tier', ['T2', 'T3'])
def test_split_bf16_equals_its_chunks(tier):
    """ga_split_bf16 has no descriptor: a flat map over n floats, checked by hand in the same way (the bf16 outputs as int16 bits)"""
    n = (B.TIERS[tier][1] // (4 if tier == 'T2' else 1)) + 8
    _need(n * 4 + 4 * (n + 2 * B.GUARD) * 2 + B.SLICE * 8, f'split_bf16 {tier}')
    t0 = time.perf_counter()
    w = torch.empty(n, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(9)
    for a, b in B.slices(n):
        w[a:b].normal_(generator=gen)
    outs = [torch.full((n + 2 * B.GUARD,), -1, dtype=torch.int16, device=DEV) for _ in range(4)]
    stream = torch.cuda.current_stream().cuda_stream
    L.check(L.lib.ga_split_bf16(w.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), n, stream), 'ga_split_bf16')
    step = 1 << 27                                                   # 2^29 bytes of input per chunk
    for a, b in [(0, 4096)] + B.slices(n - 4096, step):
        a, b = (a, b) if b == 4096 and a == 0 else (a + 4096, b + 4096)
        L.check(L.lib.ga_split_bf16(w.data_ptr() + 4 * a, outs[2].data_ptr() + 2 * a, outs[3].data_ptr() + 2 * a, b - a, stream), 'ga_split_bf16')
    torch.cuda.synchronize()
    fails = []
    for i, name in enumerate(('hi', 'lo')):
        bad, first, unwritten = 0, None, 0
        for a, b in B.slices(n):                                     # all n bf16 values as int16, in slices
            ne = outs[i][a:b] != outs[2 + i][a:b]
            c = int(ne.sum())
            if c and first is None:
                first = a + int(ne.to(torch.uint8).argmax())
            bad += c
            unwritten += int((outs[i][a:b] == -1).sum()) + int((outs[2 + i][a:b] == -1).sum())    # 0xffff is a bf16 NaN: never a result here
        if bad:
            fails.append(f'{name}: {bad} elements differ, first at element {first}')
        if unwritten:
            fails.append(f'{name}: {unwritten} elements keep the pattern they started with')
        if not bool((outs[i][n:] == -1).all() and (outs[2 + i][n:] == -1).all()):
            fails.append(f'{name}: the guard behind it changed')
    gen = torch.Generator(device=DEV).manual_seed(9)
    tmp = torch.empty(B.SLICE, device=DEV)
    for a, b in B.slices(n):
        tmp[:b - a].normal_(generator=gen)
        if B.bits_differ(tmp, w[a:b], b - a)[0]:
            fails.append('the input changed')
            break
    hi = w[:4096].to(torch.bfloat16)                                 # the anchor: the definition itself, exact
    lo = (w[:4096] - hi.float()).to(torch.bfloat16)
    if not (torch.equal(outs[2][:4096], hi.view(torch.int16)) and torch.equal(outs[3][:4096], lo.view(torch.int16))):
        fails.append('the first chunk is not hi = bf16(w), lo = bf16(w - hi)')
    print(f'\n  split_bf16 {tier} N={n} largest={n * 4} B {"MISMATCH" if fails else "bitwise"}, {time.perf_counter() - t0:.2f} s', flush=True)
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('tier', ['T1', 'T2', 'T3'])
def test_comparison_sees_a_wrapped_row(tier):
    """no kernel runs: the expected tensor gets, in the two rows past the tier's boundary, what a 32-bit offset would have addressed"""
    row = 24192
    unit, limit = B.TIERS[tier]
    first = -(-limit // (row * (4 if unit == 'bytes' else 1)))
    N = first + 2
    _need(2 * (N * row + B.GUARD) * 4 + B.SLICE * 8, f'wrap visibility {tier}')
    gen = torch.Generator(device=DEV).manual_seed(5)
    got = torch.empty(N * row, device=DEV)
    for a, b in B.slices(N * row):
        got[a:b].normal_(generator=gen)
    want = torch.empty_like(got)
    for a, b in B.slices(N * row):
        want[a:b].copy_(got[a:b])
    assert B.bits_differ(got, want, N * row) == (0, None)
    assert B.wrapped_row(first - 1, row, tier) == first - 1, 'the last row before the boundary is addressed rightly'
    for r in (first, first + 1):
        w = B.wrapped_row(r, row, tier)
        assert w != r
        if w is None:
            want[r * row:(r + 1) * row].fill_(float('nan'))
        else:
            e = r * row * (4 if unit == 'bytes' else 1) % (1 << 32) // (4 if unit == 'bytes' else 1)    # mid-row: the wrapped element
            want[r * row:(r + 1) * row].copy_(got[e:e + row])
    bad, at = B.bits_differ(got, want, N * row)
    print(f'\n  wrap visibility {tier}: N={N}, rows {first}, {first + 1} -> {B.wrapped_row(first, row, tier)}, {B.wrapped_row(first + 1, row, tier)}; '
          f'{bad} floats differ, first in row {at // row}', flush=True)
    assert bad > row and at // row == first


def test_refusals():
    """the extents the library refuses before any launch, with tiny buffers"""
    import ctypes as C
    buf = torch.zeros(4096, device=DEV)
    p = buf.data_ptr()
    big = 2 ** 31 - 1
    d = L.SamplerDesc()
    d.mu_q = d.eps = d.dz = d.z = p
    d.N, d.h, d.w, d.NL, d.ldq, d.mode, d.backward, d.alpha_ld, d.alpha_col = 1, 1 << 15, 1 << 15, 4, 4, 2, 1, 1, 0
    assert L.lib.ga_sampler_mix(C.byref(d), 0) == L.GA_E_UNSUPPORTED           # h w NL > 2^31 - 1
    d.h = (1 << 14) - 1                                                         # below: accepted shape, not launched here
    assert d.h * d.w * d.NL <= big
    for fields in (dict(N=big, H=4, W=4, C=32 * 17), dict(N=big, H=8, W=16, C=32 * 17), dict(N=big, H=16, W=32, C=32 * 17, up2=1)):
        w = L.DwDesc()
        w.x = w.w = w.y = p
        for k, v in fields.items():
            setattr(w, k, v)
        assert L.lib.ga_dwconv5(C.byref(w), 0) == L.GA_E_UNSUPPORTED, fields    # blocks > 2^31 - 1
    for cls, entry, ptrs, extra in ((L.AvgpoolActDesc, L.lib.ga_avgpool_act, ('x', 'y'), {}), (L.ReduceDesc, L.lib.ga_rowchan_reduce, ('a', 'out'), {}),
                                    (L.ModoutDesc, L.lib.ga_modout, ('t', 'dout', 'dt', 'red', 'ws'), dict(backward=1, ws_floats=1 << 40))):
        g = cls()
        for name in ptrs:
            setattr(g, name, p)
        g.N, g.P, g.C = big, 4, 128                                             # N x 2 channel chunks > 2^31 - 1 workgroups
        for k, v in extra.items():
            setattr(g, k, v)
        assert entry(C.byref(g), 0) == L.GA_E_UNSUPPORTED, cls.__name__
    assert L.lib.ga_dec_cell_halo_supported(big, 16, 16, 32, 192) == 0          # N tiles > 2^31 - 1
    assert L.lib.ga_dec_cell_halo_supported((big // 2), 16, 16, 32, 192) == 1
    h = L.DecCellHaloDesc()
    for name in ('x', 'w1_hi', 'w1_lo', 'b1', 'wd', 'bd', 'w2_hi', 'w2_lo', 'b2', 'y'):
        setattr(h, name, p)
    h.N, h.H, h.W, h.Cin, h.Cout, h.Hd = big, 16, 16, 32, 32, 192
    assert L.lib.ga_dec_cell_halo(C.byref(h), 0) == L.GA_E_UNSUPPORTED
    torch.cuda.synchronize()
