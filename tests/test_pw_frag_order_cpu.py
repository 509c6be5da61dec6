"""WeightStore.frag3(w, taps=1): the one-tap fragment order tile 12 (csrc/conv_pw_frag.hip) reads through ga_conv_desc.w_frag,
bf16 [ceil(Cout/128)][ceil(C/32)][1][4 waves][2 k steps][hi | lo][64 lanes][8]: lane = 32 * (k octet of the 16-deep step) + output
channel of the wave's 32.  Un-permuting it returns the split weights exactly."""
import torch

from gen_adversarial_amd.engine_core import WeightStore


def _unpermute(f, cout, c):
    nt, nkc = f.shape[0], f.shape[1]
    # [nt, group, tap, wave, k step, hi | lo, lane half, row, e] -> [hi | lo][nt, wave, row][group, k step, lane half, e]
    return f.permute(5, 0, 3, 7, 1, 2, 4, 6, 8).reshape(2, nt * 128, nkc * 32)[:, :cout, :c]


def test_one_tap_fragment_order_64_to_128():
    store = WeightStore('cpu')
    w = torch.randn(128, 64, generator=torch.Generator().manual_seed(0))
    f = store.frag3(w, taps=1)
    assert tuple(f.shape) == (1, 2, 1, 4, 2, 2, 2, 32, 8) and f.dtype == torch.bfloat16 and f.is_contiguous()
    hi, lo = store.split(w)
    back = _unpermute(f, 128, 64)
    assert torch.equal(back[0].view(torch.int16), hi.view(torch.int16))
    assert torch.equal(back[1].view(torch.int16), lo.view(torch.int16))
    # the element the kernel's wave `wv`, k step `ks`, lane `ln` reads at word e of group `g`
    flat = f.reshape(-1)
    for g, wv, ks, ln, e in ((0, 0, 0, 0, 0), (1, 3, 1, 63, 7), (0, 2, 1, 37, 3), (1, 1, 0, 31, 5)):
        co, k = wv * 32 + (ln & 31), g * 32 + ks * 16 + (ln >> 5) * 8 + e
        base = (((g * 4 + wv) * 2 + ks) * 2) * 64 * 8
        assert flat[base + ln * 8 + e] == hi[co, k] and flat[base + 64 * 8 + ln * 8 + e] == lo[co, k]
    assert store.frag3(w, taps=1) is f                      # made once per tensor
    assert store.frag3(torch.randn(128, 9 * 64), taps=9).shape == (1, 2, 9, 4, 2, 2, 2, 32, 8)


def test_partial_tiles_are_zero_padded():
    """Cout = 200 (a second, partial weight tile), C = 48 (a half group)"""
    store = WeightStore('cpu')
    w = torch.randn(200, 48, generator=torch.Generator().manual_seed(1))
    f = store.frag3(w, taps=1)
    assert tuple(f.shape) == (2, 2, 1, 4, 2, 2, 2, 32, 8)
    hi, lo = store.split(w)
    full = f.permute(5, 0, 3, 7, 1, 2, 4, 6, 8).reshape(2, 256, 64)
    assert torch.equal(full[0, :200, :48].view(torch.int16), hi.view(torch.int16))
    assert torch.equal(full[1, :200, :48].view(torch.int16), lo.view(torch.int16))
    assert not full[:, 200:].float().any() and not full[:, :, 48:].float().any()
