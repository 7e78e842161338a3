"""`--arch edsr` (reference model/edsr.py:7-15 MeanShift, :18-32 _Residual_Block, :35-87 EDSR; built by interfaces/base.py:348-350 with
nn.L1Loss): a frozen 1x1 colour convolution, a 3 -> 256 convolution, 32 residual blocks (conv - ReLU - conv, scaled by 0.1) and a trunk
convolution behind a long skip, one 256 -> 1024 convolution + PixelShuffle(2) per factor of two, a 256 -> 3 convolution on the HR grid and a
second frozen 1x1 colour convolution.  No bias anywhere but in the two MeanShift layers.  Same constructor signatures, attribute names and
state_dict keys; executed operator by operator on the HIP kernels (tpgsr_amd/functional.py), NHWC inside: each residual block is one call
of functional.res_block (composed over the existing operators by default; its fused form is a measurement's switch), the pixel shuffle is
the up-sampling convolution's store (out_ps), conv_output runs on the direct narrow-output kernels (functional.conv2d_narrow,
csrc/conv_narrow.hip).

Initialisation is exactly what the reference's constructor does: its init loop (:61-66) draws every nn.Conv2d weight from
N(0, sqrt(2 / (k^2 Cout))) and zeroes every bias -- and MeanShift IS an nn.Conv2d subclass, so the identity weight and the -+rgb_mean bias
it was built with are overwritten: `sub_mean.weight` / `add_mean.weight` end up N(0, sqrt(2/3)), both biases zero, all four frozen.  A
freshly built reference EDSR mixes RGB with a random frozen 3x3 matrix, not a mean shift; a loaded checkpoint decides what the layers do,
so they run as general 1x1 convolutions that read their tensors."""
import math

import torch
from torch import nn

from .. import functional as Fh
from .nn_params import Conv2dParams, EngineHolder
from .tl_common import sr_engine

RES_SCALE = 0.1
NF = 256


def _normal_init(conv):
    kh, kw = conv.kernel_size
    with torch.no_grad():
        conv.weight.normal_(0, math.sqrt(2.0 / (kh * kw * conv.out_channels)))
        if conv.bias is not None:
            conv.bias.zero_()


class MeanShift(Conv2dParams):
    """reference :7-15: a frozen nn.Conv2d(3, 3, 1) built as identity weight + sign * rgb_mean bias -- which EDSR's init loop then overwrites
    (module docstring); standing alone it keeps what it was built with, as the reference's does"""

    def __init__(self, rgb_mean, sign):
        super().__init__(3, 3, 1)
        with torch.no_grad():
            self.weight.copy_(torch.eye(3).view(3, 3, 1, 1))
            self.bias.copy_(float(sign) * torch.tensor(rgb_mean, dtype=torch.float32))
        for p in self.parameters():
            p.requires_grad = False


class _Residual_Block(nn.Module):
    """reference :18-32; `form`: functional.res_block's (None: its default)"""

    def __init__(self):
        super().__init__()
        self.conv1 = Conv2dParams(NF, NF, 3, padding=1, bias=False)
        self.relu = nn.Identity()
        self.conv2 = Conv2dParams(NF, NF, 3, padding=1, bias=False)
        self.form = None

    def forward(self, x):
        """NHWC (N, H, W, 256) -> the same shape"""
        return Fh.res_block(x, self.conv1.weight, self.conv2.weight, RES_SCALE, form=self.form)


class EDSR(EngineHolder, nn.Module):
    """`--arch edsr` (reference :35-87).  scale_factor 2 or 4: the reference builds int(math.log2(scale_factor)) up-sampling stages -- a
    factor of 3 would silently be a x2 network -- so any other value is refused here.  `n_resblocks` (keyword only) is NOT the reference's:
    its trunk is always 32 blocks deep; small tests need a shallow one.  `set_form` / `set_tail_form` name the residual blocks' and
    conv_output's form (measurement switches: tools/lab/edsr_step_time.py); None leaves the operators' defaults.

    FROZEN_BY_ENGINE names the frozen parameters for FusedAdam (tpgsr_amd/optim.py): the engine never writes their slices of the gradient
    arena (no sink is registered for them and no weight gradient is computed), so the fused step leaves them bit for bit where they are."""
    FROZEN_BY_ENGINE = ("sub_mean.weight", "sub_mean.bias", "add_mean.weight", "add_mean.bias")

    def __init__(self, scale_factor=2, *, n_resblocks=32):
        super().__init__()
        if scale_factor not in (2, 4):
            raise ValueError(f"EDSR: scale_factor={scale_factor!r}, expected 2 or 4 (one or two x2 up-sampling stages)")
        self.scale_factor = scale_factor
        rgb_mean = (0.4488, 0.4371, 0.4040)
        self.sub_mean = MeanShift(rgb_mean, -1)
        self.conv_input = Conv2dParams(3, NF, 3, padding=1, bias=False)
        self.residual = nn.Sequential(*[_Residual_Block() for _ in range(n_resblocks)])
        self.conv_mid = Conv2dParams(NF, NF, 3, padding=1, bias=False)
        ups = []
        for _ in range(int(round(math.log2(scale_factor)))):
            ups += [Conv2dParams(NF, NF * 4, 3, padding=1, bias=False), nn.Identity()]      # (index 1, 3: nn.PixelShuffle(2), no parameters)
        self.upscale = nn.Sequential(*ups)
        self.conv_output = Conv2dParams(NF, 3, 3, padding=1, bias=False)
        self.add_mean = MeanShift(rgb_mean, 1)
        self.tail_form = None
        for m in self.modules():                         # the reference's init loop (:61-66): MeanShift included
            if isinstance(m, Conv2dParams):
                _normal_init(m)

    def set_form(self, form):
        if form is not None and form not in Fh.RES_FORMS:
            raise ValueError(f"EDSR: form={form!r}, expected one of {Fh.RES_FORMS} or None")
        for m in self.residual:
            m.form = form

    def set_tail_form(self, form):
        if form is not None and form not in Fh.NARROW_FORMS:
            raise ValueError(f"EDSR: tail form={form!r}, expected one of {Fh.NARROW_FORMS} or None")
        self.tail_form = form

    def _engine(self):
        """engine adapter (tpgsr_amd/engine_functional.py PlainSREngine), as RRDBNet's: the engine carries THIS module's factor"""
        eng = sr_engine(self, prior=False)
        eng.scale = self.scale_factor
        return eng

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"EDSR: input {tuple(x.shape)} is not (N, 3, H, W)")
        out = Fh.conv2d(Fh.to_nhwc(x), self.sub_mean.weight, self.sub_mean.bias)
        out, skip = Fh.fork(self.conv_input(out))
        for block in self.residual:
            out = block(out)
        out = Fh.add(self.conv_mid(out), skip)
        for up in self.upscale:
            if isinstance(up, Conv2dParams):
                out = up(out, out_ps=True)
        out = Fh.conv2d_narrow(out, self.conv_output.weight, form=self.tail_form)
        return Fh.to_nchw(Fh.conv2d(out, self.add_mean.weight, self.add_mean.bias))
