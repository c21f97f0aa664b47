"""Torch reference of the temporal-conv variant (UNet(use_temp_attn=False)) for tests/test_tconv_host.py and
tests/test_gpu_tconv.py: the reference's TemporalCNN as a module, and an oracle/ref_cpu.py network with
Residual(PreNorm(d, TemporalCNN(d))) swapped in at the reference's positions (the input temporal op and every level but
the three deepest).  oracle/ itself knows only the attention variant and is not edited."""
import torch
import torch.nn as nn

from oracle import ref_cpu as R


class TemporalCNN(nn.Module):
    """Conv1d(dim, dim, 3, padding=1) over the frame axis of [b, c, f, h, w], identity at construction"""

    def __init__(self, dim):
        super().__init__()
        self.temporal_conv = nn.Conv1d(dim, dim, 3, padding=1)
        nn.init.dirac_(self.temporal_conv.weight.data)
        nn.init.zeros_(self.temporal_conv.bias.data)

    def forward(self, x, pos_bias=None, **kwargs):
        b, c, f, h, w = x.shape
        y = x.permute(0, 3, 4, 1, 2).reshape(b * h * w, c, f)
        y = self.temporal_conv(y)
        return y.reshape(b, h, w, c, f).permute(0, 3, 4, 1, 2)


def _block(d):
    return R.Residual(R.PreNorm(d, TemporalCNN(d)))


def swapped_oracle(mults, **kw):
    """R.UNet(ch_mults=mults) with the temporal-conv blocks where the reference puts them"""
    ref = R.UNet(ch_mults=mults, **kw)
    net = ref.net
    nres = len(net.downs)
    net.input_temp_op = _block(net.input_temp_op.fn.norm.gamma.shape[1])
    for i in range(nres):
        if i < nres - 3:
            net.downs[i][3] = _block(net.downs[i][3].fn.norm.gamma.shape[1])
        if i >= 3:
            net.ups[i][3] = _block(net.ups[i][3].fn.norm.gamma.shape[1])
    return ref


def randomize_tconv(model, seed=7):
    """temporal_conv weights ~ N(0, 0.05), biases ~ N(0, 0.1): at the identity init the outer taps are zero"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            conv = getattr(m, "temporal_conv", None)
            if conv is not None:
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.05)
                conv.bias.copy_(torch.randn(conv.bias.shape, generator=g) * 0.1)
    return model


def expected_tconv_keys(mults):
    """the reference rule, written out: prefixes of the blocks that are temporal convs"""
    nres = len(mults)
    pre = ["net.input_temp_op"]
    pre += [f"net.downs.{i}.3" for i in range(nres) if i < nres - 3]
    pre += [f"net.ups.{i}.3" for i in range(nres) if i >= 3]
    return pre
