"""`--arch bicubic` (reference model/bicubic.py:6-13): the interpolation row of every table -- `F.interpolate(x, scale_factor,
mode='bicubic', align_corners=True)` as one HIP launch (tpgsr_bicubic_upsample, csrc/aster.hip).  A plain callable, as in the
reference: no parameters, no engine, nothing trains through it."""
from typing import Optional

import torch

from .. import kernels as K


class BICUBIC(object):
    def __init__(self, scale_factor=2):
        if int(scale_factor) != scale_factor or scale_factor < 1:
            raise NotImplementedError(f"BICUBIC: the kernel takes an integer scale factor >= 1, got {scale_factor!r}")
        self.scale_factor = int(scale_factor)

    def __call__(self, x: torch.Tensor, channels: Optional[int] = None) -> torch.Tensor:
        """x (N, Ctot, H, W) fp32 -> (N, C, H * s, W * s); channels: up-sample the first C planes only (x[:, :C] without the copy)"""
        if not (x.is_cuda or K.DRYRUN):
            raise RuntimeError("BICUBIC runs on the GPU only (no CPU fallback)")
        if x.dim() != 4 or x.dtype != torch.float32:
            raise TypeError(f"BICUBIC expects an fp32 (N, C, H, W) batch, got {x.dtype} {tuple(x.shape)}")
        x = x.detach().contiguous()
        N, Ctot, H, W = x.shape
        C = Ctot if channels is None else int(channels)
        s = self.scale_factor
        out = torch.empty(N, max(C, 0), H * s, W * s, device=x.device)
        K.bicubic_upsample(x, N, Ctot, C, H, W, s, out)
        return out
