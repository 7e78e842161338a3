"""`--arch rdn` (reference model/rdn.py:22-31 make_dense, :35-50 RDB, :54-90 RDN): the residual dense network, and `--arch rdn_tl`
(:126-154 RDB_TL, :159-214 RDN_TL) whose three dense blocks fuse the text-prior map in their 1x1 bottleneck.  Same constructor / state_dict keys; executed operator by
operator on the HIP kernels (the dense concatenations are channel-slice copies, the x2 sub-pixel up-sampling is the conv
kernel's pixel-shuffle store)."""
import torch
from torch import nn

from .. import functional as Fh
from .nn_params import Conv2dParams, EngineHolder, _NoForward
from .tl_common import InfoGen, spatial_text_embedding, sr_engine, zero_prior


class make_dense(nn.Module):
    def __init__(self, nChannels, growthRate, kernel_size=3):
        super().__init__()
        self.conv = Conv2dParams(nChannels, growthRate, kernel_size, padding=(kernel_size - 1) // 2, bias=False)

    def forward(self, x):
        x, keep = Fh.fork(x)      # (conv and the concatenation: gradients summed by a HIP kernel, not by autograd)
        return Fh.cat([keep, Fh.relu(self.conv(x))])


class RDB(nn.Module):
    """reference :35-50"""

    def __init__(self, nChannels, nDenselayer, growthRate):
        super().__init__()
        n = nChannels
        mods = []
        for _ in range(nDenselayer):
            mods.append(make_dense(n, growthRate))
            n += growthRate
        self.dense_layers = nn.Sequential(*mods)
        self.conv_1x1 = Conv2dParams(n, nChannels, 1, padding=0, bias=False)

    def forward(self, x):
        out, skip = Fh.fork(x)
        for layer in self.dense_layers:
            out = layer(out)
        return Fh.add(self.conv_1x1(out), skip)


class RDB_TL(nn.Module):
    def __init__(self, nChannels, nDenselayer, growthRate, out_text_channels=32):
        super().__init__()
        n = nChannels
        mods = []
        for _ in range(nDenselayer):
            mods.append(make_dense(n, growthRate))
            n += growthRate
        self.dense_layers = nn.Sequential(*mods)
        self.conv_1x1 = Conv2dParams(n + out_text_channels, nChannels, 1, padding=0, bias=False)

    def forward(self, x, text_emb):
        out, skip = Fh.fork(x)
        for layer in self.dense_layers:
            out = layer(out)
        return Fh.add(self.conv_1x1(Fh.cat([out, text_emb])), skip)


class sub_pixel(nn.Module):
    def __init__(self, scale, act=False):
        super().__init__()
        self.body = nn.Sequential(_NoForward())      # nn.PixelShuffle: fused into conv_up's store


class RDN(EngineHolder, nn.Module):
    """`--arch rdn` (reference :54-90, train_RDN.sh): the prior-free baseline on the RGB planes.  Same constructor / state_dict keys."""

    def __init__(self, nChannel=3, nDenselayer=6, nFeat=64, scale_factor=2, growthRate=32):
        super().__init__()
        if scale_factor != 2:
            raise NotImplementedError("pixel-shuffle store specialised for scale 2")
        self.conv1 = Conv2dParams(nChannel, nFeat, 3, padding=1)
        self.conv2 = Conv2dParams(nFeat, nFeat, 3, padding=1)
        self.RDB1 = RDB(nFeat, nDenselayer, growthRate)
        self.RDB2 = RDB(nFeat, nDenselayer, growthRate)
        self.RDB3 = RDB(nFeat, nDenselayer, growthRate)
        self.GFF_1x1 = Conv2dParams(nFeat * 3, nFeat, 1, padding=0)
        self.GFF_3x3 = Conv2dParams(nFeat, nFeat, 3, padding=1)
        self.conv_up = Conv2dParams(nFeat, nFeat * scale_factor * scale_factor, 3, padding=1)
        self.upsample = sub_pixel(scale_factor)
        self.conv3 = Conv2dParams(nFeat, nChannel, 3, padding=1)

    def _engine(self):
        """engine adapter (tpgsr_amd/engine_functional.py PlainSREngine): lets SRTrainStep / FusedAdam / ArenaPool / TextSREvaluator drive
        this backbone through the `else:` branch of the train loop (interfaces/super_resolution.py:409-424)"""
        return sr_engine(self, prior=False)

    def forward(self, x):
        F_, F_skip = Fh.fork(self.conv1(Fh.to_nhwc(x)))
        F_0 = self.conv2(F_)
        F_1, F_1c = Fh.fork(self.RDB1(F_0))
        F_2, F_2c = Fh.fork(self.RDB2(F_1))
        F_3 = self.RDB3(F_2)
        FGF = self.GFF_3x3(self.GFF_1x1(Fh.cat([F_1c, F_2c, F_3])))
        us = self.conv_up(Fh.add(FGF, F_skip), out_ps=True)
        return Fh.to_nchw(self.conv3(us))


class RDN_TL(EngineHolder, nn.Module):
    def __init__(self, nChannel=4, nDenselayer=6, nFeat=64, scale_factor=2, growthRate=32, output_size=(32, 128), text_emb=37,
                 out_text_channels=32):
        super().__init__()
        if scale_factor != 2:
            raise NotImplementedError("pixel-shuffle store specialised for scale 2")
        self.conv1 = Conv2dParams(nChannel, nFeat, 3, padding=1)
        self.conv2 = Conv2dParams(nFeat, nFeat, 3, padding=1)
        self.RDB1 = RDB_TL(nFeat, nDenselayer, growthRate, out_text_channels)
        self.RDB2 = RDB_TL(nFeat, nDenselayer, growthRate, out_text_channels)
        self.RDB3 = RDB_TL(nFeat, nDenselayer, growthRate, out_text_channels)
        self.GFF_1x1 = Conv2dParams(nFeat * 3, nFeat, 1, padding=0)
        self.GFF_3x3 = Conv2dParams(nFeat, nFeat, 3, padding=1)
        self.conv_up = Conv2dParams(nFeat, nFeat * scale_factor * scale_factor, 3, padding=1)
        self.upsample = sub_pixel(scale_factor)
        self.conv3 = Conv2dParams(nFeat, nChannel, 3, padding=1)
        self.tps_outputsize = [16, 64]
        self.infoGen = InfoGen(text_emb, out_text_channels)

    def _engine(self):
        """engine adapter (tpgsr_amd/engine_functional.py FunctionalSREngine): lets TPGSRTrainStep / FusedAdam / ArenaPool / TextSREvaluator
        drive this backbone as the SR network of the cascade loop (interfaces/super_resolution.py:295-424)"""
        return sr_engine(self)

    def forward(self, x, text_emb=None):
        if text_emb is None:
            text_emb = zero_prior(x, self.infoGen.tconv1.in_channels)
        t = spatial_text_embedding(self.infoGen, text_emb, (x.shape[2], x.shape[3]))
        t1, t2, t3 = Fh.fork(t, 3)      # every tensor with several consumers is forked: its gradients are summed by one HIP launch
        F_, F_skip = Fh.fork(self.conv1(Fh.to_nhwc(x)))
        F_0 = self.conv2(F_)
        F_1, F_1c = Fh.fork(self.RDB1(F_0, t1))
        F_2, F_2c = Fh.fork(self.RDB2(F_1, t2))
        F_3 = self.RDB3(F_2, t3)
        FGF = self.GFF_3x3(self.GFF_1x1(Fh.cat([F_1c, F_2c, F_3])))
        us = self.conv_up(Fh.add(FGF, F_skip), out_ps=True)
        return Fh.to_nchw(self.conv3(us))
