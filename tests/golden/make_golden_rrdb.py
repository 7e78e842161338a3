#!/usr/bin/env python
"""Fixtures for `--arch esrgan` (reference model/esrgan.py RRDBNet, constructed by interfaces/base.py:342-344 with nn.L1Loss and trained
through the `else:` branch of the loop, interfaces/super_resolution.py:409-424) at scale_factor 2 and 4, generated from the GENUINE
reference's module (imported at run time through oracle/ref_import.py; build container only).

Two depths per factor: nb = 23 (the default trunk) on N = 2 samples and nb = 2 on N = 4.  Weights by recipe (`generic_recipe` of
make_golden_next.py, seeds in `SEEDS`) and inputs by `synthetic_batch(n, seed, scale=s)`: the tests rebuild both, only results are stored.
Every stored forward result is first compared with this file's own float64 restatement of the network (`rrdb_forward`, plain
torch.nn.functional -- the tests import it as their float64 reference where no fixture is stored), and the reference's float32 run has to
stay within a QUARTER of every bound tests/test_rrdb_gpu.py applies, measured against float64 (`BOUNDS` and the fixture skeletons of
golden_plain_arch.py).  SR images are stored for the
first `N_STORE[scale]` samples of a batch.

    python tests/golden/make_golden_rrdb.py     # rewrites tests/golden/rrdb_x{2,4}.npz, train_rrdb_x{2,4}.npz, rrdb_layouts.json"""
import json
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from golden_plain_arch import BOUNDS, Recipe, eval_fixture, model_fixture, save_pair, ssim64, ssim_window, to64, train_fixture  # noqa: E402,F401
# (ssim64 -- over the reference's float32-built taps -- and to64 are re-exported for the tests)

SCALES = (2, 4)
DEPTHS = (23, 2)
CHANNELS = 3                                                     # `--arch esrgan` runs without --mask: three planes
N = {23: 2, 2: 4}                                                # batch size per depth
# (nb, scale) -> (data seed, weight seed, upstream-gradient seed, data seed of the 12x40 batch).  (2, 2): the first set tried, (88, 507, 517,
# 98), puts a pre-activation within float32 rounding of a LeakyReLU kink -- the reference's own float32 gradient of one weight is then 1.9e-3
# from float64, over a quarter of the 5e-3 bound -- so the next set is used; the assertions below hold every set to the quarter margin
SEEDS = {(23, 2): (86, 505, 515, 96), (23, 4): (87, 506, 516, 97), (2, 2): (98, 517, 527, 108), (2, 4): (89, 508, 518, 99)}
N_SMALL, SMALL_HW = 1, (12, 40)
N_STORE = {2: 2, 4: 1}                                            # samples of a 16x64 batch whose SR image is stored
SLOPE, RES_SCALE = 0.2, 0.2
# the evaluator batch (N = 6, nb = EVAL_NB): weight seeds of the network (per scale) and of the CRNN recogniser; the data seed is CHOSEN below
EVAL_N, EVAL_NB, EVAL_SEEDS = 6, 2, {2: 525, 4: 526, "rec": 60}
EVAL_DATA_SEEDS = range(300, 364)


def rrdb_forward(p, x, scale, nb):
    """the network restated over torch.nn.functional in the dtype of `p` / `x` (p: a dict of tensors keyed like the state_dict)"""
    def conv(name, h):
        return F.conv2d(h, p[name + ".weight"], p[name + ".bias"], padding=1)

    def rdb(name, h):
        feats = [h]
        for k in range(1, 5):
            feats.append(F.leaky_relu(conv(f"{name}.conv{k}", torch.cat(feats, 1)), SLOPE))
        return conv(f"{name}.conv5", torch.cat(feats, 1)) * RES_SCALE + h

    fea = conv("conv_first", x)
    h = fea
    for i in range(nb):
        o = h
        for j in (1, 2, 3):
            o = rdb(f"RRDB_trunk.{i}.RDB{j}", o)
        h = o * RES_SCALE + h
    fea = fea + conv("trunk_conv", h)
    for i in range({2: 1, 4: 2}[scale]):
        fea = F.leaky_relu(conv(f"upconv{i + 1}", F.interpolate(fea, scale_factor=2, mode="nearest")), SLOPE)
    return conv("conv_last", F.leaky_relu(conv("HRconv", fea), SLOPE))


RECIPE = Recipe(build=lambda R, s, nb: R.esrgan.RRDBNet(scale_factor=s, nb=nb), forward=rrdb_forward, channels=CHANNELS, n=N, n_store=N_STORE,
                n_small=N_SMALL, small_hw=SMALL_HW, eval_n=EVAL_N, eval_nb=EVAL_NB, eval_seeds=EVAL_SEEDS, eval_data_seeds=EVAL_DATA_SEEDS)


def main():
    import types
    import warnings
    warnings.filterwarnings("ignore")
    from oracle import ref_import, tpgsr_oracle as O
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    R = ref_import.load()
    from model import esrgan as r_esrgan      # (the reference's, on sys.path now)
    R.esrgan = r_esrgan
    assert torch.equal(R.ssim_psnr.create_window(11, 1)[0, 0], ssim_window()), "ssim_window() is not the reference's window"
    torch.manual_seed(0)
    layouts = {}
    for s in SCALES:
        model, train = {}, {}
        for nb in DEPTHS:
            net = R.esrgan.RRDBNet(scale_factor=s, nb=nb)
            layouts[f"x{s}_nb{nb}"] = [(k, list(v.shape)) for k, v in net.state_dict().items()]
            model.update(model_fixture(RECIPE, nb, s, SEEDS[(nb, s)], R, O))
            train.update(train_fixture(RECIPE, nb, s, SEEDS[(nb, s)], R, O))
        model.update(eval_fixture(RECIPE, s, R, O))
        save_pair(HERE, "rrdb", s, model, train)
    json.dump(layouts, open(os.path.join(HERE, "rrdb_layouts.json"), "w"), indent=0)
    print("rrdb_x*.npz, train_rrdb_x*.npz, rrdb_layouts.json written")


if __name__ == "__main__":
    main()
