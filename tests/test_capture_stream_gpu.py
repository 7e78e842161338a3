"""GPU: the warm-up stream of `capture()` is never the side or the aux stream.

torch hands `torch.cuda.Stream()` objects out of a fixed pool per device, round-robin, so after enough allocations in one process a new
stream IS the cached side (or aux) stream; a train step warmed up on it replays its plans with the caller's stream and the weight-gradient
stream being one, which tpgsr_plan_run refuses ("no distinct streams were given").  Whether a given `capture()` met that depended on how
many streams the process had made before it.  `kernels.fresh_stream` skips the two."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_fresh_stream_skips_the_side_and_aux_streams():
    from tpgsr_amd import kernels as K
    side, aux = K.side_stream(), K.aux_stream()
    assert side.cuda_stream != aux.cuda_stream
    pool = {torch.cuda.Stream().cuda_stream for _ in range(80)}
    assert side.cuda_stream in pool and aux.cuda_stream in pool            # the premise: plain allocation comes back to both
    got = [K.fresh_stream().cuda_stream for _ in range(2 * len(pool) + 2)]
    assert side.cuda_stream not in got and aux.cuda_stream not in got
    assert len(set(got)) >= len(pool) - 2                                   # ... and still walks the rest of the pool


def test_capture_on_every_pool_position():
    """capture() + replay() of a small train step once per pool position: one of them would have met the side stream, one the aux stream"""
    from tpgsr_amd import kernels as K
    from tpgsr_amd.interfaces.super_resolution import SRTrainStep
    from tpgsr_amd.model import srresnet
    from tpgsr_amd.utils.synthetic import synthetic_batch
    K.side_stream()
    n_pool = len({torch.cuda.Stream().cuda_stream for _ in range(80)})
    lr, hr = (t.cuda() for t in synthetic_batch(2, 3))
    torch.manual_seed(0)
    net = srresnet.SRResNet(scale_factor=2, width=128, height=32, mask=True).cuda().train()
    ts = SRTrainStep(net, image_crit="mse")
    ts.step(lr, hr)
    for _ in range(n_pool):                                                 # capture() draws one stream per call: every position once
        ts.capture(lr, hr, warmup=1)
    torch.cuda.synchronize()
    assert torch.isfinite(ts.replay()).all()
