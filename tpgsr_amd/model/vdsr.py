"""`--arch vdsr` (reference model/vdsr.py:11-18 Conv_ReLU_Block, :39-89 VDSR) and `--arch vdsr_tl` (:21-37 Conv_ReLU_Block_TL,
:123-233 VDSR_TL): nearest x2 up-sampling, six
conv3x3(64 + 32 -> 64) + ReLU + skip blocks fed with the text-prior map, global residual.  Same constructor / state_dict keys /
initialisation (conv weights N(0, sqrt(2 / (k*k*Cout)))); executed operator by operator on the HIP kernels."""
from math import sqrt

import torch
from torch import nn

from .. import functional as Fh
from .nn_params import Conv2dParams, EngineHolder
from .tl_common import InfoGen, spatial_text_embedding, sr_engine, zero_prior


class Conv_ReLU_Block(nn.Module):
    """reference :11-18"""

    def __init__(self):
        super().__init__()
        self.conv = Conv2dParams(64, 64, 3, padding=1, bias=False)
        self.relu = nn.Identity()

    def forward(self, x):
        """NHWC in / out"""
        x, skip = Fh.fork(x)      # (the block and its skip: gradients summed by a HIP kernel, not by autograd)
        return Fh.add(Fh.relu(self.conv(x)), skip)


def _vdsr_init(net):
    """reference :48-51: every conv weight N(0, sqrt(2 / (k * k * Cout)))"""
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, Conv2dParams):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.normal_(0, sqrt(2.0 / n))


class VDSR(EngineHolder, nn.Module):
    """`--arch vdsr` (reference :39-89): nearest x2 up-sampling, conv + ReLU, six conv3x3 + ReLU + skip blocks, conv, global residual --
    on the RGB planes.  Same constructor / state_dict keys / initialisation."""

    def __init__(self, scale_factor=2, in_planes=3, width=32, height=128, STN=False):
        super().__init__()
        self.upscale_factor = scale_factor
        self.residual_layer = nn.Sequential(*[Conv_ReLU_Block() for _ in range(6)])
        self.input = Conv2dParams(in_planes, 64, 3, padding=1, bias=False)
        self.output = Conv2dParams(64, in_planes, 3, padding=1, bias=False)
        self.relu = nn.Identity()
        _vdsr_init(self)
        self.tps_inputsize = [height // scale_factor, width // scale_factor]
        self.stn = False        # the reference hard-codes it off (:56)

    def _engine(self):
        """engine adapter (tpgsr_amd/engine_functional.py PlainSREngine): lets SRTrainStep / FusedAdam / ArenaPool / TextSREvaluator drive
        this backbone through the `else:` branch of the train loop (interfaces/super_resolution.py:409-424)"""
        return sr_engine(self, prior=False)

    def forward(self, x):
        h, h_skip = Fh.fork(Fh.upsample_nearest(Fh.to_nhwc(x), self.upscale_factor))
        out = Fh.relu(self.input(h))
        for block in self.residual_layer:
            out = block(out)
        return Fh.to_nchw(Fh.add(self.output(out), h_skip))


class Conv_ReLU_Block_TL(nn.Module):
    def __init__(self, out_text_channels=32):
        super().__init__()
        self.conv = Conv2dParams(64 + out_text_channels, 64, 3, padding=1, bias=False)
        self.relu = nn.Identity()

    def forward(self, x, text_emb):
        """NHWC in / out"""
        x, skip = Fh.fork(x)      # (the block and its skip: gradients summed by a HIP kernel, not by autograd)
        return Fh.add(Fh.relu(self.conv(Fh.cat([x, text_emb]))), skip)


class VDSR_TL(EngineHolder, nn.Module):
    def __init__(self, scale_factor=2, in_planes=4, width=32, height=128, STN=False, text_emb=37, out_text_channels=32):
        super().__init__()
        self.upscale_factor = scale_factor
        self.out_text_channels = out_text_channels
        self.input = Conv2dParams(in_planes, 64, 3, padding=1, bias=False)
        self.output = Conv2dParams(64, in_planes, 3, padding=1, bias=False)
        self.relu = nn.Identity()
        self.infoGen = InfoGen(text_emb, out_text_channels)
        for i in range(1, 7):
            setattr(self, f"block{i}", Conv_ReLU_Block_TL(out_text_channels))
        _vdsr_init(self)
        self.tps_inputsize = [height // scale_factor, width // scale_factor]
        self.tps_outputsize = [height, width]
        self.stn = False        # the reference hard-codes it off (:169)

    def _engine(self):
        """engine adapter (tpgsr_amd/engine_functional.py FunctionalSREngine): lets TPGSRTrainStep / FusedAdam / ArenaPool / TextSREvaluator
        drive this backbone as the SR network of the cascade loop (interfaces/super_resolution.py:295-424)"""
        return sr_engine(self)

    def forward(self, x, text_emb=None):
        if text_emb is None:
            text_emb = zero_prior(x, self.infoGen.tconv1.in_channels)
        h = Fh.upsample_nearest(Fh.to_nhwc(x), self.upscale_factor)
        t = spatial_text_embedding(self.infoGen, text_emb, tuple(self.tps_outputsize))
        ts = Fh.fork(t, 6)        # the text-prior map feeds all six blocks: one n-way gradient sum
        h, h_skip = Fh.fork(h)
        out = Fh.relu(self.input(h))
        for i in range(1, 7):
            out = getattr(self, f"block{i}")(out, ts[i - 1])
        return Fh.to_nchw(Fh.add(self.output(out), h_skip))
