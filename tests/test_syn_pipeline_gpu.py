"""GPU: the `--syn` collate on the device (tpgsr_resize_ragged in csrc/preprocess.hip, AlignCollateSyn / resize_batch in tpgsr_amd/data.py)
BIT-EXACT against Pillow's committed outputs (tests/golden/syn_resize.npz) and against the oracle applied twice (pinned against Pillow by
tests/test_syn_pipeline_cpu.py).  Integer arithmetic throughout: every comparison is array_equal."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMG_WH = (128, 32)

from oracle import input_pipeline as ip  # noqa: E402


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "syn_resize.npz"))


@pytest.fixture(scope="module")
def ragged48():
    """a seeded ragged batch (drawn like tests/test_input_pipeline_gpu.py's) and the oracle's HR / stage 1 / LR for s = 2, 4, computed once"""
    rng = np.random.default_rng(3)
    batch = [rng.integers(0, 256, (int(rng.integers(6, 70)), int(rng.integers(8, 260)), 3), dtype=np.uint8) for _ in range(48)]
    ref = {"hr": np.stack([ip.resize_normalize(im, IMG_WH, mask=True) for im in batch])}
    for s in (2, 4):
        st = [ip.pil_resize_bicubic(im, (im.shape[1] // s, im.shape[0] // s)) for im in batch]
        ref[f"st{s}"] = st
        ref[f"lr{s}"] = np.stack([ip.resize_normalize(a, (IMG_WH[0] // s, IMG_WH[1] // s), mask=True) for a in st])
    for v in ref.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return batch, ref


def _chw(u8):
    return np.transpose(u8.astype(np.float32) / 255.0, (2, 0, 1))


@pytest.mark.parametrize("s", [2, 4])
def test_resize_batch_vs_pillow_fixture(fixture, s):
    from tpgsr_amd.data import ragged_view, resize_batch
    keep = [int(j) for j in fixture[f"idx{s}"]]
    imgs = [fixture[f"img{j}"] for j in keep]
    buf, entries = resize_batch(imgs, [(im.shape[1] // s, im.shape[0] // s) for im in imgs])
    assert buf.dtype == torch.uint8 and buf.is_cuda and len(entries) == len(imgs)
    off = 0
    for j, im, e in zip(keep, imgs, entries):
        assert e == (off, im.shape[0] // s, im.shape[1] // s)
        assert np.array_equal(ragged_view(buf, e).cpu().numpy(), fixture[f"st{s}_{j}"]), (s, j)
        off += 3 * e[1] * e[2]
    assert buf.numel() == off


def test_raw_entry_point_stays_inside_its_buffers(fixture):
    """out8 and tmp with 256 guard bytes on both sides, everything pre-filled with 0xA5: the guards stay, out8 is written completely (the
    images lie back to back: no byte in between), and in tmp only image n's rows < H_n and columns < w1_n are touched"""
    from tpgsr_amd import _lib, data, kernels as K
    G, FILL, s = 256, 0xA5, 2
    keep = [int(j) for j in fixture[f"idx{s}"]]
    imgs = [fixture[f"img{j}"] for j in keep]
    N = len(imgs)
    flat = data._flatten(imgs)
    tabs = data._BatchTables()
    src, dst, out_bytes = data._ragged_layout(flat, [(w // s, h // s) for _, h, w in flat], tabs)
    maxH, maxOH, maxOW = max(d.H for d in src), max(d.H for d in dst), max(d.W for d in dst)
    assert maxH == 70 and min(d.H for d in src) == 3                      # the tall image next to short ones: most of tmp is padding
    pix = torch.from_numpy(np.concatenate([a for a, _, _ in flat])).to(DEV)
    tab = torch.from_numpy(tabs.concat()).to(DEV)
    dsc = torch.frombuffer(bytearray(bytes(src) + bytes(dst)), dtype=torch.uint8).to(DEV)
    nb = N * ctypes.sizeof(_lib.ImageDesc)
    tmp_bytes = N * maxH * maxOW * 3
    tmp = torch.full((tmp_bytes + 2 * G,), FILL, dtype=torch.uint8, device=DEV)
    out = torch.full((out_bytes + 2 * G,), FILL, dtype=torch.uint8, device=DEV)
    K._launch("tpgsr_resize_ragged", K._p(pix), K._p(dsc[:nb]), K._p(dsc[nb:]), K._p(tab), N, maxH, maxOH, maxOW, K._p(tmp) + G, K._p(out) + G)
    torch.cuda.synchronize()
    out, tmp = out.cpu().numpy(), tmp.cpu().numpy()
    assert (out[:G] == FILL).all() and (out[-G:] == FILL).all() and (tmp[:G] == FILL).all() and (tmp[-G:] == FILL).all()
    want = np.concatenate([fixture[f"st{s}_{j}"].reshape(-1) for j in keep])
    assert want.size == out_bytes and np.array_equal(out[G:-G], want)     # every byte between the guards is an image's
    t = tmp[G:-G].reshape(N, maxH, maxOW, 3)
    for n, (im, d) in enumerate(zip(imgs, dst)):
        pad = np.ones((maxH, maxOW), bool)
        pad[:im.shape[0], :d.W] = False
        assert (t[n][pad] == FILL).all(), n
        assert np.array_equal(t[n, :im.shape[0], :d.W], ip._pass(im, d.W, 1)), n      # ... and hold the horizontal pass
    # a null pointer or an empty batch is refused before any launch
    lib = _lib.load()
    for bad_pix, bad_n in ((None, N), (K._p(pix), 0)):
        assert lib.tpgsr_resize_ragged(bad_pix, K._p(dsc[:nb]), K._p(dsc[nb:]), K._p(tab), bad_n, maxH, maxOH, maxOW, K._p(pix), K._p(pix), None) != 0
        assert b"tpgsr_resize_ragged" in lib.tpgsr_last_error()


@pytest.mark.parametrize("mask", [True, False])
def test_align_collate_syn_vs_pillow_fixture(fixture, mask):
    from tpgsr_amd.data import AlignCollateSyn
    for s in (2, 4):
        keep = [int(j) for j in fixture[f"idx{s}"]]
        hr, lr, words, ident = AlignCollateSyn(down_sample_scale=s, mask=mask)([(fixture[f"img{j}"], f"w{j}") for j in keep])
        assert hr.shape == (len(keep), 3 + mask, 32, 128) and lr.shape == (len(keep), 3 + mask, 32 // s, 128 // s)
        assert words == [f"w{j}" for j in keep] and ident == [None] * len(keep)
        hr, lr = hr.cpu().numpy(), lr.cpu().numpy()
        for i, j in enumerate(keep):
            assert np.array_equal(hr[i, :3], _chw(fixture[f"hr{j}"])), (s, j)
            assert np.array_equal(lr[i, :3], _chw(fixture[f"lr{s}_{j}"])), (s, j)
            if mask:
                assert np.array_equal(hr[i, 3], fixture[f"hr{j}_mask"].astype(np.float32) / 255.0), (s, j)
                assert np.array_equal(lr[i, 3], fixture[f"lr{s}_{j}_mask"].astype(np.float32) / 255.0), (s, j)


@pytest.mark.parametrize("s", [2, 4])
def test_align_collate_syn_ragged_batch_vs_oracle(ragged48, s):
    from tpgsr_amd.data import AlignCollateSyn, ragged_view, resize_batch
    batch, ref = ragged48
    items = [(im, im, f"w{i}", f"path{i}") for i, im in enumerate(batch)]              # the four-tuples of FolderDatasetSVT
    for mask in (True, False):
        hr, lr, words, ident = AlignCollateSyn(down_sample_scale=s, mask=mask)(items)
        C = 3 + mask
        assert words[5] == "w5" and ident[7] == "path7"
        assert np.array_equal(hr.cpu().numpy(), ref["hr"][:, :C])
        assert np.array_equal(lr.cpu().numpy(), ref[f"lr{s}"][:, :C])
    buf, entries = resize_batch(batch, [(im.shape[1] // s, im.shape[0] // s) for im in batch])
    for e, want in zip(entries, ref[f"st{s}"]):
        assert np.array_equal(ragged_view(buf, e).cpu().numpy(), want)


@pytest.mark.parametrize("s", [2, 4])
def test_result_does_not_depend_on_the_rest_of_the_batch(ragged48, s):
    """image j collated alone equals row j of the batch of 48: nothing is read from another image's rows or from the scratch's padding"""
    from tpgsr_amd.data import AlignCollateSyn
    batch, _ = ragged48
    collate = AlignCollateSyn(down_sample_scale=s, mask=True)
    hr, lr, _, _ = collate([(im, "") for im in batch])
    for j, im in enumerate(batch):
        torch.empty(1 << 20, dtype=torch.uint8, device=DEV).fill_(0x5A)                # the scratch of the next call starts out dirty
        h1, l1, _, _ = collate([(im, "")])
        assert torch.equal(h1[0], hr[j]) and torch.equal(l1[0], lr[j]), j


def test_synthetic_batch_trains_with_labels(ragged48):
    from test_crnn_gpu import _c3_models
    from tpgsr_amd.data import AlignCollate, AlignCollateSyn
    from tpgsr_amd.interfaces.super_resolution import TPGSRTrainStep
    batch, ref = ragged48
    words = ["Hotel", "a1", "", "OPEN-24h-and-more"]
    out = AlignCollateSyn(labels=True)(list(zip(batch[:4], words)))
    assert len(out) == 7
    hr, lr, strs, ident, *labels = out
    real = AlignCollate(labels=True)(list(zip(batch[:4], ref["st2"][:4], words)))
    assert torch.equal(real[0], hr) and torch.equal(real[1], lr) and real[2] == strs       # the pairs Pillow would have made on the host
    assert len(real) == 6 and all(a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(real[3:], labels))
    assert hr.shape == (4, 4, 32, 128) and lr.shape == (4, 4, 16, 64)
    srs, stus, teacher, *_ = _c3_models()
    ts = TPGSRTrainStep(srs, stus, teacher, stu_iter=1, use_label=True)
    loss = ts.step(lr, hr, labels=tuple(labels))
    assert loss.numel() == 1 and bool(torch.isfinite(loss).all()), loss
