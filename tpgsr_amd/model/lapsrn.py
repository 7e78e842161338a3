"""`--arch lapsrn` (reference model/lapsrn.py:23-54 _Conv_Block, :57-123 LapSRN, :126-137 L1_Charbonnier_loss): the Laplacian-pyramid
baseline -- per x2 stage ten conv3x3(64 -> 64) + LeakyReLU(0.2), a ConvTranspose2d(64, 64, 4, 2, 1) + LeakyReLU(0.2), a 64 -> in_planes
residual convolution, and a bilinear-initialised ConvTranspose2d(in_planes, in_planes, 4, 2, 1) on the image; x4 chains two stages.  Same
constructor signature, state_dict keys and initialisation; executed operator by operator on the HIP kernels (tpgsr_amd/functional.py):
the 64 -> 64 transposed convolutions in their sub-pixel form (a 3x3 pixel-shuffle-store convolution on the matrix cores), the image
branch's through the direct narrow kernels (csrc/tconv4s2.hip), no ATen compute."""
import math

import torch
from torch import nn

from .. import functional as Fh
from .. import kernels as K
from .nn_params import Conv2dParams, ConvTranspose2dParams, EngineHolder
from .tl_common import sr_engine

SLOPE = 0.2


def bilinear_kernel(size: int) -> torch.Tensor:
    """(size, size) bilinear up-sampling kernel: the outer product of the 1-D tent around the kernel's centre (what the reference's
    get_upsample_filter builds; size 4: [0.25, 0.75, 0.75, 0.25] x itself)"""
    factor = (size + 1) // 2
    centre = factor - 1 if size % 2 == 1 else factor - 0.5
    tent = 1.0 - (torch.arange(size, dtype=torch.float64) - centre).abs() / factor
    return torch.outer(tent, tent).float()


class _TConv4s2(ConvTranspose2dParams):
    """nn.ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1, bias=False) holder run by functional.conv_transpose2d_k4s2"""

    def __init__(self, in_channels, out_channels):
        super().__init__(in_channels, out_channels, 4, 2, padding=1)

    def forward(self, x):
        return Fh.conv_transpose2d_k4s2(x, self.weight)


class _Conv_Block(nn.Module):
    """reference :23-54: cov_block.{0, 2, ..., 18} conv3x3, .20 the transposed convolution, LeakyReLU(0.2) after each (odd indices)"""

    def __init__(self):
        super().__init__()
        layers = []
        for _ in range(10):
            layers += [Conv2dParams(64, 64, 3, padding=1, bias=False), nn.Identity()]
        layers += [_TConv4s2(64, 64), nn.Identity()]
        self.cov_block = nn.Sequential(*layers)

    def forward(self, x):
        """NHWC (N, H, W, 64) -> (N, 2H, 2W, 64)"""
        for i in range(0, 22, 2):
            x = Fh.leaky_relu(self.cov_block[i](x), SLOPE)
        return x


class LapSRN(EngineHolder, nn.Module):
    """`--arch lapsrn` (reference :57-123).  scale_factor 2 or 4 (the second stage's parameters exist at 2 too, unused, as in the
    reference); the reference falls off the end of its forward for any other factor -- here the constructor refuses."""

    def __init__(self, scale_factor=2, in_planes=3, STN=False, width=128, height=32):
        super().__init__()
        if scale_factor not in (2, 4):
            raise ValueError(f"LapSRN: scale_factor={scale_factor!r}, expected 2 or 4 (one or two x2 stages)")
        self.scale_factor = scale_factor
        self.conv_input = Conv2dParams(in_planes, 64, 3, padding=1, bias=False)
        self.relu = nn.Identity()
        self.convt_I1 = _TConv4s2(in_planes, in_planes)
        self.convt_R1 = Conv2dParams(64, in_planes, 3, padding=1, bias=False)
        self.convt_F1 = nn.Sequential(_Conv_Block())
        self.convt_I2 = _TConv4s2(in_planes, in_planes)
        self.convt_R2 = Conv2dParams(64, in_planes, 3, padding=1, bias=False)
        self.convt_F2 = nn.Sequential(_Conv_Block())
        with torch.no_grad():      # reference :73-84
            for m in self.modules():
                if isinstance(m, Conv2dParams):
                    n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                    m.weight.normal_(0, math.sqrt(2.0 / n))
                elif isinstance(m, ConvTranspose2dParams):
                    m.weight.copy_(bilinear_kernel(m.kernel_size[0]).expand_as(m.weight))
        self.tps_inputsize = [height // scale_factor, width // scale_factor]
        if STN:
            # (as SRResNet: the reference wires model/recognizer/stn_head.py here, which cannot take the 16x64 crops)
            raise NotImplementedError("LapSRN is run without --STN (the reference's recognizer STN head cannot take 16x64 inputs)")
        self.stn = False

    def _engine(self):
        """engine adapter (tpgsr_amd/engine_functional.py PlainSREngine): lets SRTrainStep / FusedAdam / ArenaPool / TextSREvaluator drive
        this backbone through the `else:` branch of the train loop (interfaces/super_resolution.py:409-424); the engine carries THIS
        module's factor (the class constant of the other operator-level backbones is 2)"""
        eng = sr_engine(self, prior=False)
        eng.scale = self.scale_factor
        return eng

    def forward(self, x):
        if tuple(x.shape[1:2]) != (self.conv_input.in_channels,):
            raise ValueError(f"LapSRN: input {tuple(x.shape)} is not (N, {self.conv_input.in_channels}, H, W)")
        h, h_img = Fh.fork(Fh.to_nhwc(x))      # two consumers: the feature branch and the image branch
        f1 = self.convt_F1[0](Fh.leaky_relu(self.conv_input(h), SLOPE))
        if self.scale_factor == 4:
            f1, f1_next = Fh.fork(f1)          # the residual convolution and the second stage
        hr2 = Fh.add(self.convt_I1(h_img), self.convt_R1(f1))
        if self.scale_factor == 2:
            return Fh.to_nchw(hr2)
        f2 = self.convt_F2[0](f1_next)
        return Fh.to_nchw(Fh.add(self.convt_I2(hr2), self.convt_R2(f2)))


class _CharbonnierFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, tgt, eps):
        if not ((out.is_cuda and tgt.is_cuda) or K.DRYRUN):
            raise RuntimeError("tpgsr_amd losses run on the GPU only (no CPU fallback)")
        if out.shape != tgt.shape:
            raise ValueError(f"L1_Charbonnier_loss: {tuple(out.shape)} vs {tuple(tgt.shape)}")
        out, tgt = out.contiguous().float(), tgt.contiguous().float()
        nblk = max(1, min(1024, out.numel() // 256))
        part = torch.empty(nblk, 2, device=out.device)
        loss = torch.empty((), device=out.device)
        K.charbonnier_loss_fwd(out, tgt, out.numel(), eps, part, nblk)
        K.image_loss_finalize(part, nblk, 1, 0, 1.0, 0.0, loss)      # count 1: the criterion is a sum
        ctx.save_for_backward(out, tgt)
        ctx.eps = eps
        return loss

    @staticmethod
    def backward(ctx, dloss):
        out, tgt = ctx.saved_tensors
        dout = torch.empty_like(out)
        K.charbonnier_loss_bwd(out, tgt, dloss.contiguous().float().reshape(1), out.numel(), ctx.eps, 1.0, dout)
        return dout, None, None


class L1_Charbonnier_loss(nn.Module):
    """reference :126-137: sum sqrt((X - Y)^2 + eps) over every element (a sum, not a mean), eps = 1e-6, on the tpgsr_charbonnier_loss_*
    kernels"""

    def __init__(self):
        super().__init__()
        self.eps = 1e-6

    def forward(self, X, Y):
        return _CharbonnierFn.apply(X, Y, float(self.eps))
