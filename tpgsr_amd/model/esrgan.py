"""`--arch esrgan` (reference model/esrgan.py:16-36 ResidualDenseBlock_5C, :39-52 RRDB, :55-86 RRDBNet): the ESRGAN generator -- a 3x3
convolution, `nb` residual-in-residual dense blocks (three five-convolution dense blocks each, every residual scaled by 0.2), a trunk
convolution behind a long skip, one nearest-neighbour x2 up-sampling stage + convolution + LeakyReLU(0.2) per factor of two, and two
convolutions on the HR grid.  Same constructor signatures, attribute names, state_dict keys and (PyTorch default) initialisation; executed
operator by operator on the HIP kernels (tpgsr_amd/functional.py): each dense block is ONE operator working on one concatenation buffer
(functional.dense_block, csrc/dense.hip), no ATen compute.  The reference's SubDiscriminator / conv_block are dead code there (they call
helpers the file does not define and no --arch reaches them) and are not built."""
import math

from torch import nn

from .. import functional as Fh
from .nn_params import Conv2dParams, EngineHolder
from .tl_common import sr_engine

SLOPE = 0.2
RES_SCALE = 0.2


class ResidualDenseBlock_5C(nn.Module):
    """reference :16-36; `form`: functional.dense_block's (None: its default)"""

    def __init__(self, nf=64, gc=32, bias=True):
        super().__init__()
        self.conv1 = Conv2dParams(nf, gc, 3, padding=1, bias=bias)
        self.conv2 = Conv2dParams(nf + gc, gc, 3, padding=1, bias=bias)
        self.conv3 = Conv2dParams(nf + 2 * gc, gc, 3, padding=1, bias=bias)
        self.conv4 = Conv2dParams(nf + 3 * gc, gc, 3, padding=1, bias=bias)
        self.conv5 = Conv2dParams(nf + 4 * gc, nf, 3, padding=1, bias=bias)
        self.lrelu = nn.Identity()
        self.form = None

    def forward(self, x):
        """NHWC (N, H, W, nf) -> the same shape"""
        convs = (self.conv1, self.conv2, self.conv3, self.conv4, self.conv5)
        return Fh.dense_block(x, [c.weight for c in convs], [c.bias for c in convs], SLOPE, RES_SCALE, form=self.form)


class RRDB(nn.Module):
    """Residual in Residual Dense Block (reference :39-52)"""

    def __init__(self, nf, gc=32):
        super().__init__()
        self.RDB1 = ResidualDenseBlock_5C(nf, gc)
        self.RDB2 = ResidualDenseBlock_5C(nf, gc)
        self.RDB3 = ResidualDenseBlock_5C(nf, gc)

    def forward(self, x):
        out, skip = Fh.fork(x)
        out = self.RDB3(self.RDB2(self.RDB1(out)))
        return Fh.scaled_add(out, skip, RES_SCALE)


class RRDBNet(EngineHolder, nn.Module):
    """`--arch esrgan` (reference :55-86).  scale_factor 2 or 4: the reference builds int(log2(scale_factor)) up-sampling stages, and
    int(math.log(8, 2)) is 2 -- a factor of 8 would silently be a x4 network -- so any other value is refused here.  `set_form` names the dense
    blocks' form for every block (a measurement's switch: tools/lab/rrdb_step_time.py); None leaves functional.dense_block's default."""

    def __init__(self, scale_factor=2, in_nc=3, out_nc=3, nf=64, nb=23, gc=32):
        super().__init__()
        if scale_factor not in (2, 4):
            raise ValueError(f"RRDBNet: scale_factor={scale_factor!r}, expected 2 or 4 (one or two x2 up-sampling stages)")
        self.scale_factor = scale_factor
        self.upsample_block_num = int(round(math.log2(scale_factor)))
        self.conv_first = Conv2dParams(in_nc, nf, 3, padding=1)
        self.RRDB_trunk = nn.Sequential(*[RRDB(nf, gc) for _ in range(nb)])
        self.trunk_conv = Conv2dParams(nf, nf, 3, padding=1)
        for i in range(self.upsample_block_num):
            setattr(self, "upconv%d" % (i + 1), Conv2dParams(nf, nf, 3, padding=1))
        self.HRconv = Conv2dParams(nf, nf, 3, padding=1)
        self.conv_last = Conv2dParams(nf, out_nc, 3, padding=1)
        self.lrelu = nn.Identity()

    def set_form(self, form):
        if form is not None and form not in Fh.DENSE_FORMS:
            raise ValueError(f"RRDBNet: form={form!r}, expected one of {Fh.DENSE_FORMS} or None")
        for m in self.modules():
            if isinstance(m, ResidualDenseBlock_5C):
                m.form = form

    def _engine(self):
        """engine adapter (tpgsr_amd/engine_functional.py PlainSREngine): lets SRTrainStep / FusedAdam / ArenaPool / TextSREvaluator drive
        this backbone through the `else:` branch of the train loop (interfaces/super_resolution.py:409-424); the engine carries THIS
        module's factor"""
        eng = sr_engine(self, prior=False)
        eng.scale = self.scale_factor
        return eng

    def forward(self, x):
        if tuple(x.shape[1:2]) != (self.conv_first.in_channels,):
            raise ValueError(f"RRDBNet: input {tuple(x.shape)} is not (N, {self.conv_first.in_channels}, H, W)")
        fea, fea_skip = Fh.fork(self.conv_first(Fh.to_nhwc(x)))
        for block in self.RRDB_trunk:
            fea = block(fea)
        fea = Fh.add(fea_skip, self.trunk_conv(fea))
        for i in range(self.upsample_block_num):
            fea = Fh.leaky_relu(getattr(self, "upconv%d" % (i + 1))(Fh.upsample_nearest(fea, 2)), SLOPE)
        return Fh.to_nchw(self.conv_last(Fh.leaky_relu(self.HRconv(fea), SLOPE)))
