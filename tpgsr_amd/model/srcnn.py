"""`--arch srcnn` and `--arch srcnn_tl` (reference: model/srcnn.py:109-145 SRCNN, :50-106 SRCNN_TL).

SRCNN -- nearest-neighbour up-sampling, Conv2d(3, 64, 9) - ReLU - Conv2d(64, 32, 1) - ReLU - Conv2d(32, 3, 5), trained by train_SRCNN.sh
through the `else:` branch of the loop (interfaces/super_resolution.py:409-424) on three channels with nn.MSELoss -- runs on the MI355X
operator by operator on the HIP kernels (tpgsr_amd/functional.py), NHWC inside; its last layer, three output channels on the HR grid,
runs on the direct narrow-output kernels (functional.conv2d_narrow5x5, csrc/conv_narrow5.hip).

A CPU input takes the ONE deliberate stock-PyTorch path of this package: BASELINE config C1 is a plumbing
case that checks the harness / fixtures / timer without a GPU, so `SRCNN()(cpu_tensor)` computes the same network with ATen on the same
parameter tensors.  It is no fall-back: a device input never reaches it, and a missing kernel is an error there."""
import torch
from torch import nn

from .nn_params import Conv2dParams, EngineHolder


class SRCNN(EngineHolder, nn.Module):
    """Same constructor signature, attribute names, state_dict keys and initial values (Conv2dParams draws what nn.Conv2d draws) as the
    reference's.  scale_factor 2 and 4 are built and tested; the device path takes any integer factor and refuses another at its first
    forward (the CPU path takes what F.interpolate takes).  `set_tail_form` names conv3's form (a measurement switch:
    tools/lab/srcnn_step_time.py); None leaves functional.conv2d_narrow5x5's default."""

    def __init__(self, scale_factor=2, in_planes=3, STN=False, height=32, width=128):
        super().__init__()
        if STN:
            raise NotImplementedError("SRCNN+STN is not on the TPGSR path (train_SRCNN.sh runs without --STN)")
        self.upscale_factor = scale_factor
        self.conv1 = Conv2dParams(in_planes, 64, 9, padding=4)
        self.relu1 = nn.Identity()
        self.conv2 = Conv2dParams(64, 32, 1, padding=0)
        self.relu2 = nn.Identity()
        self.conv3 = Conv2dParams(32, in_planes, 5, padding=2)
        self.stn = STN
        self.tail_form = None

    def set_tail_form(self, form):
        from .. import functional as Fh
        if form is not None and form not in Fh.NARROW_FORMS:
            raise ValueError(f"SRCNN: tail form={form!r}, expected one of {Fh.NARROW_FORMS} or None")
        self.tail_form = form

    def _engine(self):
        """engine adapter (tpgsr_amd/engine_functional.py PlainSREngine), as LapSRN's: the engine carries THIS module's factor"""
        from .tl_common import sr_engine
        eng = sr_engine(self, prior=False)
        eng.scale = self.upscale_factor
        return eng

    def _forward_aten(self, x):
        F = torch.nn.functional
        x = F.interpolate(x, scale_factor=self.upscale_factor)
        x = F.relu(F.conv2d(x, self.conv1.weight, self.conv1.bias, padding=4))
        x = F.relu(F.conv2d(x, self.conv2.weight, self.conv2.bias))
        return F.conv2d(x, self.conv3.weight, self.conv3.bias, padding=2)

    def forward(self, x):
        from .. import functional as Fh
        from .. import kernels as K
        if not (x.is_cuda or K.DRYRUN):
            return self._forward_aten(x)
        s = self.upscale_factor
        if isinstance(s, bool) or int(s) != s or s < 1:
            raise ValueError(f"SRCNN: scale_factor={s!r}: the device path up-samples by an integer factor (tpgsr_resize_nearest_fwd)")
        out = Fh.upsample_nearest(Fh.to_nhwc(x), int(s))
        out = Fh.relu(self.conv1(out))
        out = Fh.relu(self.conv2(out))
        return Fh.to_nchw(Fh.conv2d_narrow5x5(out, self.conv3.weight, self.conv3.bias, form=self.tail_form))


class SRCNN_TL(EngineHolder, nn.Module):
    """`--arch srcnn_tl` (reference model/srcnn.py:50-106): SRCNN with the text-prior map concatenated in front of each conv.
    Unlike the CPU plumbing class above this one runs on the MI355X, operator by operator on the HIP kernels."""

    def __init__(self, scale_factor=2, in_planes=4, STN=False, height=32, width=128, text_emb=37, out_text_channels=32):
        super().__init__()
        from .nn_params import Conv2dParams
        from .tl_common import InfoGen
        self.upscale_factor = scale_factor
        self.conv1 = Conv2dParams(in_planes + out_text_channels, 64, 9, padding=4)
        self.relu1 = nn.Identity()
        self.conv2 = Conv2dParams(64 + out_text_channels, 32, 1, padding=0)
        self.relu2 = nn.Identity()
        self.conv3 = Conv2dParams(32 + out_text_channels, in_planes, 5, padding=2)
        self.tps_inputsize = [height // scale_factor, width // scale_factor]
        self.tps_outputsize = [height, width]
        if STN:   # as SRResNet_TL: the reference's recognizer STN head cannot take the 16x64 crops; its scripts run without --STN
            raise NotImplementedError("SRCNN_TL is run without --STN")
        self.stn = False
        self.infoGen = InfoGen(text_emb, out_text_channels)

    def _engine(self):
        """engine adapter (tpgsr_amd/engine_functional.py FunctionalSREngine): lets TPGSRTrainStep / FusedAdam / ArenaPool / TextSREvaluator
        drive this backbone as the SR network of the cascade loop (interfaces/super_resolution.py:295-424)"""
        from .tl_common import sr_engine
        return sr_engine(self)

    def forward(self, x, text_emb=None):
        from .. import functional as Fh
        from .tl_common import spatial_text_embedding, zero_prior
        if text_emb is None:
            text_emb = zero_prior(x, self.infoGen.tconv1.in_channels)
        h = Fh.upsample_nearest(Fh.to_nhwc(x), self.upscale_factor)
        t = spatial_text_embedding(self.infoGen, text_emb, (h.shape[1], h.shape[2]))
        t1, t2, t3 = Fh.fork(t, 3)      # three consumers: their gradients are summed by one HIP launch, not by autograd
        out = Fh.relu(self.conv1(Fh.cat([h, t1])))
        out = Fh.relu(self.conv2(Fh.cat([out, t2])))
        return Fh.to_nchw(self.conv3(Fh.cat([out, t3])))
