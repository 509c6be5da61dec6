"""Shared pieces of the plan builder (engine.py and its per-network builder mixins): constants, the conv tuning
table, the weight store and the activation record."""
from __future__ import annotations

import json
import os
from typing import Callable, Dict, NamedTuple, Optional

import torch

RES_SCALE = 0.1          # `0.1 * self.residual(x)` — architecture.py:133,183
IMG_LD = 8                  # channel pitch of the NHWC image tensors (3 channels + zero padding)
WS_FLOATS = 32 * 1024 * 1024     # split-K workspace shared by every conv of an engine (128 MB)
TUNE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_tune_gfx950.json')
_TUNE_CACHE: Optional[dict] = None


def tune_cache() -> dict:
    """(tile, splits) per conv shape, measured on an MI355X by Engine.autotune and kept in-tree."""
    global _TUNE_CACHE
    if _TUNE_CACHE is None:
        _TUNE_CACHE = {}
        if os.path.exists(TUNE_FILE):
            with open(TUNE_FILE) as f:
                _TUNE_CACHE = json.load(f)
    return _TUNE_CACHE


def conv_key(d) -> str:
    return ('b3_' if d.w_hi else '') + '_'.join(str(int(v)) for v in (
        d.N * d.Ho * d.Wo, d.Cout, d.C1, d.C2, d.KH, d.sn, d.sd, d.Hi, d.pro_act, bool(d.pro_scale), d.pro_per_row,
        bool(d.dact_x), d.dact_act, bool(d.addend), bool(d.addend2), d.addend_bcast_n)) + (
        f'_kw{d.KW}' if d.KW != d.KH else '')


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


# ---- which explicit tile codes ga_conv2d takes for a descriptor (GA_E_UNSUPPORTED otherwise).  Each *_ok predicate restates ONE
#      function of the library, the conv_<family>_check declared in csrc/conv_families.h: halo_ok and frag_ok conv_halo3_check
#      (csrc/conv_halo3.hip, tiles 5 - 7 and tile 8), quad_ok conv_quad3_check (csrc/conv_quad3.hip), thin_ok conv_thin3_check
#      (csrc/conv_thin3.hip), pw_ok conv_pw_frag_check (csrc/conv_pw_frag.hip).  What a check is told (conv_req: vec_out, bf3, the
#      clamped splits) comes from operand_classes and split_factor in csrc/conv2d.hip: _bf3_vec_out and _splits here.
#      tests/test_plan_convs_gpu.py checks that the library refuses exactly what these reject.
_HALO_HK, _HALO_LDH = 32, 40                # conv_halo3.hip: channels per chunk, bf16 per LDS pixel row
_BF3_MODES = (0x000, 0x100, 0x001, 0x002, 0x003, 0x004, 0x010, 0x011, 0x020, 0x021)
_HALO_MODES = (0x00, 0x01, 0x02, 0x03, 0x04, 0x10, 0x11, 0x20)


def _a16(p) -> bool:
    return not p or p % 16 == 0


def _pro_mode(d) -> int:
    return ((2 if d.pro_per_row else 1) if d.pro_scale else 0) << 4 | d.pro_act


def _splits(d, splits=None) -> int:
    s = d.splits if splits is None else splits
    if s <= 1:
        return 1
    return min(s, d.KH * d.KW * ((d.C1 + d.C2 + 31) // 32))


def _bf3_vec_out(d, splits: int) -> bool:
    """conv_req.bf3 and conv_req.vec_out (operand_classes, csrc/conv2d.hip): the split-bf16 operands are usable, with a prologue
    conv_bf3_mode_ok has a kernel for, and the output is written as float4"""
    c2 = d.C2 > 0
    vec = d.C1 % 4 == 0 and d.C2 % 4 == 0 and d.ldx % 4 == 0 and (not c2 or d.ldx2 % 4 == 0) and _a16(d.x) and _a16(d.w) \
        and (not c2 or _a16(d.x2)) and (not d.pro_scale or (_a16(d.pro_scale) and _a16(d.pro_shift)))
    bf3 = bool(d.w_hi and d.w_lo) and vec and d.sd == 1 and (not c2 or d.C1 % 32 == 0) and (d.C1 + d.C2) % 8 == 0 \
        and d.KH * d.KW <= 32 and _a16(d.w_hi) and _a16(d.w_lo) and ((0x100 if c2 else 0) | _pro_mode(d)) in _BF3_MODES
    vec_out = d.Cout % 4 == 0 and d.ldy % 4 == 0 and _a16(d.y) and _a16(d.bias) \
        and (not d.addend or (d.ldadd % 4 == 0 and _a16(d.addend))) and (not d.addend2 or (d.ldadd2 % 4 == 0 and _a16(d.addend2))) \
        and (not d.dact_x or (d.lddact % 4 == 0 and _a16(d.dact_x) and (not d.dact_scale or (_a16(d.dact_scale) and _a16(d.dact_shift))))) \
        and (splits == 1 or _a16(d.ws))
    return bf3 and vec_out


def _halo_3x3(d) -> bool:
    """conv_halo3_shape_ok: 3x3 / stride 1 / pad 1, one source of C1 % 32 == 0 channels, 128-pixel tiles of whole rows (or whole
    small images) or 128-pixel segments of one row"""
    if (d.KH, d.KW, d.sn, d.sd, d.pad, d.C2) != (3, 3, 1, 1, 1, 0) or d.Ho != d.Hi or d.Wo != d.Wi or d.C1 % _HALO_HK:
        return False
    howo = d.Ho * d.Wo
    rows = d.Wo < 128 and 128 % d.Wo == 0 and (howo % 128 == 0 or 128 % howo == 0)
    return (rows or d.Wo % 128 == 0) and _pro_mode(d) in _HALO_MODES


def _halo_geometry(d, bm: int = 128, ldh: int = _HALO_LDH):
    """halo_geometry, as halo_plan_for uses it (csrc/conv_halo3.hip): (NI images per tile, P patch pixels, IS bf16 per image patch)"""
    howo = d.Ho * d.Wo
    wide = d.Wo >= bm
    tw = bm if wide else d.Wo
    th = 1 if wide else (bm // d.Wo if howo >= bm else d.Ho)
    ni = 1 if howo >= bm else bm // howo
    ph, pw = th + 2, tw + 2

    def pad_to(nbytes, want):
        return nbytes + ((want - nbytes) % 256 + 256) % 256
    rs = pad_to(pw * ldh * 2, (tw * ldh * 2) % 256)
    is_ = pad_to(ph * rs, (th * tw * ldh * 2) % 256) // 2
    return ni, ni * ph * pw, is_


def halo_ok(d, tile: Optional[int] = None, splits: Optional[int] = None) -> bool:
    """conv_halo3_check for tile 5 (128 x 128), 6 (128 x 64) or 7 (128 x 32; default d.tile): ga_conv2d runs d on the LDS-staged halo
    kernel (halo_plan_for's tile 5 - 7 branch: patch slots, the WIDE prologues, split-K over chunks, 160 KB of LDS)"""
    tile = d.tile if tile is None else tile
    s = _splits(d, splits)
    if tile not in (5, 6, 7) or not _bf3_vec_out(d, s) or not _halo_3x3(d):
        return False
    ni, p, is_ = _halo_geometry(d)
    if p > 13 * 32 or (p > 9 * 32 and _pro_mode(d) not in (0x00, 0x10, 0x20)) or s > d.C1 // _HALO_HK:
        return False
    bn = {5: 128, 6: 64, 7: 32}[tile]
    return (2 * ni * is_ + 2 * 2 * bn * _HALO_LDH) * 2 <= 160 * 1024


def frag_ok(d, splits: Optional[int] = None) -> bool:
    """conv_halo3_check for tile 8: ga_conv2d runs d on the halo kernel with its weight fragments read from d.w_frag
    (halo_plan_for's tile 8 branch: patch, slot and prologue tables within 80 KB of LDS)"""
    s = _splits(d, splits)
    if not d.w_frag or not _a16(d.w_frag) or not _bf3_vec_out(d, s) or not _halo_3x3(d):
        return False
    ni, p, is_ = _halo_geometry(d)
    if p > 9 * 32 or s > d.C1 // _HALO_HK:
        return False
    mode = _pro_mode(d)
    patch = 2 * ni * is_ * 2
    rp = (p * 8 + 255) >> 8
    tab = rp * 256 * 6 + (2 * (ni if mode == 0x20 else 1) * d.C1 * 4 if mode >= 0x10 else 0)
    dbuf = 2 * patch + tab <= 80 * 1024
    tab_off = ((2 if dbuf else 1) * patch + 15) // 16 * 4
    return tab_off * 4 + tab <= 80 * 1024


def quad_ok(d, splits: Optional[int] = None) -> bool:
    """conv_quad3_check: ga_conv2d runs d on tile 9, what the halo kernels take, on 4 x 4 images in whole groups of 32, with tile
    8's d.w_frag (a batch of fewer than 32 images runs as one partial group).  (Tile 8's LDS bound does not apply: the kernel keeps two 36-KB patch buffers and no tables at any channel count.)"""
    s = _splits(d, splits)
    if not d.w_frag or not _a16(d.w_frag) or not _bf3_vec_out(d, s) or not _halo_3x3(d):
        return False
    return d.Hi == 4 and d.Wi == 4 and (d.N % 32 == 0 or d.N < 32) and s <= d.C1 // _HALO_HK


def thin_ok(d, splits: Optional[int] = None) -> bool:
    """conv_thin3_check: ga_conv2d runs d on tile 11, the persistent weights-resident 3x3 kernel of 32 or 64 input channels (d.w_frag in its order)"""
    s = _splits(d, splits)
    if s != 1 or not d.w_frag or not _a16(d.w_frag) or not _bf3_vec_out(d, s):
        return False
    if (d.KH, d.KW, d.sn, d.sd, d.pad, d.C2) != (3, 3, 1, 1, 1, 0) or d.C1 not in (32, 64):
        return False
    return d.Ho == d.Hi and d.Wo == d.Wi and d.Ho % 8 == 0 and d.Wo % 16 == 0 and d.Wo <= 255 * 16 and _pro_mode(d) in _HALO_MODES


def pw_ok(d, splits: Optional[int] = None) -> bool:
    """conv_pw_frag_check: ga_conv2d runs d on tile 12, the 1x1 kernel with its weight fragments read from d.w_frag (one tap;
    without the copy the kernel gathers them from w_hi / w_lo, slower: the engine always builds it, Engine._want)"""
    s = _splits(d, splits)
    if s != 1 or not _a16(d.w_frag) or not _bf3_vec_out(d, s):
        return False
    if (d.KH, d.KW, d.sn, d.sd, d.pad, d.C2) != (1, 1, 1, 1, 0, 0) or d.Ho != d.Hi or d.Wo != d.Wi:
        return False
    if d.C1 % 16 or (d.N * d.Ho * d.Wo) % 128:
        return False
    # (a tensor past the loaders' 31-bit offsets is convolved in row sub-batches, whose pixel counts need not be whole tiles)
    if d.N * d.Ho * d.Wo * max(d.ldx, d.ldy, d.ldadd, d.ldadd2, d.lddact) * 4 >= 0x7fffff00:
        return False
    mode = _pro_mode(d)
    return mode in (0x00, 0x01, 0x10, 0x11) or (mode == 0x20 and (d.Ho * d.Wo) % 16 == 0)


class Tile(NamedTuple):
    """what the host knows of one explicit tile code of ga_conv_desc.tile"""
    code: int
    bm: int                                 # output pixels x output channels of a workgroup
    bn: int
    ok: Callable                            # ok(d, splits): ga_conv2d takes d on this tile (the predicates above)
    split_k: Optional[str] = 'step'         # split-K over 'step's of 32 channels of one tap, over 32-channel 'chunk's, or None
    fallback: Optional[tuple] = None        # (tile with the same bits to demote to, whether it keeps the split-K factor)
    frag: Optional[Callable] = None         # frag(store, w, d): the fragment-ordered weight copy d.w_frag points at
    weight_ok: Optional[Callable] = None    # weight_ok(d, w): the tensor w has the layout (and the channel count) `frag` takes


def _rows_of(d, w, taps: int) -> bool:
    return w.dim() == 2 and w.shape[1] == taps * d.C1 and d.KH * d.KW == taps and d.C2 == 0


TILES: Dict[int, Tile] = {t.code: t for t in (
    Tile(1, 128, 128, lambda d, s: True), Tile(2, 128, 64, lambda d, s: True),
    Tile(3, 64, 64, lambda d, s: True), Tile(4, 128, 32, lambda d, s: True),
    Tile(5, 128, 128, lambda d, s: halo_ok(d, 5, s), 'chunk', (0, False)),
    Tile(6, 128, 64, lambda d, s: halo_ok(d, 6, s), 'chunk', (0, False)),
    Tile(7, 128, 32, lambda d, s: halo_ok(d, 7, s), 'chunk', (0, False)),
    Tile(8, 128, 128, frag_ok, 'chunk', (5, True), lambda store, w, d: store.frag3(w),
         lambda d, w: _rows_of(d, w, 9) and d.C1 % 32 == 0),
    Tile(9, 128, 128, quad_ok, 'chunk', (8, True), lambda store, w, d: store.frag3(w),
         lambda d, w: _rows_of(d, w, 9) and d.C1 % 32 == 0),
    Tile(11, 128, 32, thin_ok, None, (7, False), lambda store, w, d: store.frag_thin(w),
         lambda d, w: _rows_of(d, w, 9) and d.C1 in (32, 64)),
    Tile(12, 128, 128, pw_ok, None, (0, False), lambda store, w, d: store.frag3(w.reshape(d.Cout, d.C1), taps=1),   # (the bits of tiles 1 - 4)
         lambda d, w: w.numel() == d.Cout * d.C1 and d.C1 % 16 == 0),
)}


def resolve_tile(d, tile: int, splits: int, can_frag: Callable) -> tuple:
    """the (tile, splits) d runs with when the tune table names (tile, splits) for its key.  conv_key does not encode pad / Wo / the
    weight layout: a desc can share the key of an entry without being eligible for its tile.  It is then demoted along `fallback`
    to a tile that gives the same values (9 -> 8 -> 5, 11 -> 7 when the halo kernel takes it), else to the library heuristic (0).
    can_frag(tile) points d.w_frag at that tile's weight copy, or returns False."""
    while tile in TILES:
        t = TILES[tile]
        if t.fallback is None or ((t.split_k or splits <= 1) and (t.frag is None or can_frag(tile)) and t.ok(d, splits)):
            break
        tile, splits = t.fallback[0], (splits if t.fallback[1] else 1)
    return tile, splits


def candidate_tiles(d, has_weight: Callable) -> tuple:
    """the tile codes Engine.autotune times on the split-bf16 operands of d beside tiles 1 - 4; has_weight(tile): d's weight
    tensor is known and `weight_ok` for that fragment-fed tile"""
    if not d.w_hi:
        return ()
    halo = (5, 6, 7) if (d.KH == 3 and d.KW == 3 and d.sn == 1 and d.sd == 1 and d.C2 == 0) else ()
    if halo and has_weight(8):
        halo += (8,)
        if d.Hi == 4 and d.Wi == 4 and (d.N % 32 == 0 or d.N < 32) and has_weight(9):     # the quadrant tile: 4 x 4 images only
            halo += (9,)
    thin = (11,) if halo and has_weight(11) else ()
    pw = (12,) if has_weight(12) and (d.sn, d.sd, d.pad) == (1, 1, 0) and (d.N * d.Ho * d.Wo) % 128 == 0 else ()
    return halo + thin + pw


def tile_candidates(d, has_weight: Callable) -> list:
    """[(use_bf3, tile, splits), ...] in the order Engine.autotune times them (the first of two ties wins).  Not filtered by
    `ok`: a candidate the library refuses is attempted and skipped"""
    M = d.N * d.Ho * d.Wo
    T = d.KH * d.KW * ((d.C1 + d.C2 + 31) // 32)
    out = []
    for use_bf3 in ((1, 0) if d.w_hi else (0,)):
        for t in [TILES[c] for c in (1, 2, 3, 4) + (candidate_tiles(d, has_weight) if use_bf3 else ())]:
            if t.bn >= 2 * max(32, d.Cout):
                continue
            blocks = -(-M // t.bm) * -(-d.Cout // t.bn)
            for splits in (1, 2, 4, 8, 16, 32):
                if splits > 1 and (t.split_k is None or blocks * splits > 2048 or T < 2 * splits or splits * M * d.Cout > WS_FLOATS):
                    continue
                if t.split_k == 'chunk' and splits > d.C1 // 32:        # the halo kernel splits K over 32-channel chunks
                    continue
                out.append((use_bf3, t.code, splits))
    return out


class WeightStore:
    """Folded weights on the device, shared by every engine (row count) built for one model."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.cache: Dict[str, dict] = {}
        self.splits: Dict[int, tuple] = {}
        self.bytes = 0

    def split(self, w: torch.Tensor):
        """bf16 (hi, lo) pair of a device weight tensor, hi = bf16(w), lo = bf16(w - hi); made once per tensor."""
        k = w.data_ptr()
        if k not in self.splits:
            hi = w.to(torch.bfloat16)
            lo = (w - hi.float()).to(torch.bfloat16)
            self.splits[k] = (hi.contiguous(), lo.contiguous(), w)
            self.bytes += 4 * w.numel()
        return self.splits[k][0], self.splits[k][1]

    def frag3(self, w: torch.Tensor, taps: int = 9) -> torch.Tensor:
        """the split weights of a 3x3 conv ([Cout][9 * C] fp32, C % 32 == 0) in the MFMA-fragment order of ga_conv_desc.w_frag
        (bf16 [ceil(Cout/128)][C/32][taps][4 waves][2 k steps][hi | lo][64 lanes][8]); made once per tensor.
        taps=1: the same order for a 1x1 conv ([Cout][C], tile 12 — forward weights and the transposed copies of the ^T launches
        alike); C % 16 == 0, a last half group is zero-padded to 32 channels."""
        k = ('frag3' + ('' if taps == 9 else f'_taps{taps}'), w.data_ptr())
        if k not in self.splits:
            hi, lo = self.split(w)
            cout, kk = w.shape
            c = kk // taps
            cp = (c + 31) // 32 * 32
            assert kk == taps * c and (cp == c or (taps == 1 and c % 16 == 0)), (tuple(w.shape), taps)
            nt, nkc = (cout + 127) // 128, cp // 32

            def arr(t):
                tp = torch.zeros(nt * 128, taps * cp, dtype=torch.bfloat16, device=t.device)
                tp[:cout, :kk] = t
                # [nt, wave, row, tap, chunk, k step, lane half, e] -> [nt, chunk, tap, wave, k step, lane half, row, e]
                return tp.view(nt, 4, 32, taps, nkc, 2, 2, 8).permute(0, 4, 3, 1, 5, 6, 2, 7)
            f = torch.stack([arr(hi), arr(lo)], dim=5).contiguous()          # hi | lo between the k step / half and the lane
            self.splits[k] = (f, w)
            self.bytes += 2 * f.numel()
        return self.splits[k][0]

    def frag_thin(self, w: torch.Tensor) -> torch.Tensor:
        """the split weights of a 3x3 conv with C = 32 or 64 input channels ([Cout][9 * C] fp32) in the order of tile 11 (conv_thin3.hip):
        bf16 [ceil(Cout/32)][9 taps][C/16 k steps][hi | lo][64 lanes][8], lane = 32 * (k octet of the 16-deep step) + channel"""
        k = ('frag_thin', w.data_ptr())
        if k not in self.splits:
            hi, lo = self.split(w)
            cout, kk = w.shape
            assert kk in (9 * 32, 9 * 64), tuple(w.shape)
            nt, ks = (cout + 31) // 32, kk // 9 // 16

            def arr(t):
                tp = torch.zeros(nt * 32, kk, dtype=torch.bfloat16, device=t.device)
                tp[:cout] = t
                # [nt, channel, tap, k step, k octet, e] -> [nt, tap, k step, k octet, channel, e]
                return tp.view(nt, 32, 9, ks, 2, 8).permute(0, 2, 3, 4, 1, 5)
            f = torch.stack([arr(hi), arr(lo)], dim=3).contiguous()            # hi | lo between the k step and the lane
            self.splits[k] = (f, w)
            self.bytes += 2 * f.numel()
        return self.splits[k][0]

    def get(self, key: str, fn):
        if key not in self.cache:
            d = {k: v.to(self.device, dtype=torch.float32).contiguous() for k, v in fn().items()}
            self.bytes += sum(v.numel() * 4 for v in d.values())
            self.cache[key] = d
        return self.cache[key]


class Act:
    """An NHWC activation buffer plus its (lazily allocated) gradient buffer.  With K cotangents per forward row
    (Engine(cot_rep=K): the K-cotangent backward plan) the gradient buffer has n * K rows, cotangent k of forward row r at row
    r * K + k; the backward ops read the saved activation of cotangent row m at row m // K (`act_rep` / `dact_rep` of ga_ops.h)."""

    def __init__(self, eng: "Engine", n, h, w, c, name=''):
        self.eng, self.n, self.h, self.w, self.c, self.name = eng, n, h, w, c, name
        self.t = eng.alloc((n, h, w, c))
        self._g = None
        self.g_written = False
        eng.acts[name] = self

    @property
    def g(self) -> torch.Tensor:
        if self._g is None:
            self._g = self.eng.alloc((self.n * getattr(self.eng, 'cot_rep', 1), self.h, self.w, self.c))
        return self._g


