"""CPU: the `--syn` input path (alignCollate_syn, dataset/dataset.py:952-992) without a device.

* the reference of the GPU test: the oracle's `pil_resize_bicubic` applied TWICE equals Pillow's resize(...).resize(...), on the committed
  fixture (tests/golden/syn_resize.npz, make_golden_syn.py) and live against the installed Pillow;
* the host coefficient tables (tpgsr_resample_coeffs) on the size pairs this path adds: (n, n // s) and the upsampling second stage;
* AlignCollateSyn's host logic under TPGSR_PLAN_DRYRUN=1: launches, argument lists, descriptors, errors, the empty batch;
* the HR-only readers LmdbDatasetHR and FolderDatasetSVT."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import input_pipeline as ip

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
IMG_WH = (128, 32)


def test_oracle_twice_vs_pillow_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "syn_resize.npz"))
    sizes = [g[f"img{j}"].shape[:2] for j in range(int(g["n"]))]
    # the cases the fixture has to hold
    assert any(h % 4 and w % 4 and h % 2 and w % 2 for h, w in sizes) and (32, 128) in sizes and (5, 9) in sizes
    assert any(a[0] == 70 and b[0] == 6 for a, b in zip(sizes, sizes[1:]))
    for s in (2, 4):
        keep = [int(j) for j in g[f"idx{s}"]]
        assert keep == [j for j, (h, w) in enumerate(sizes) if h // s and w // s]
        assert any(sizes[j][0] // s == 1 for j in keep) and any(sizes[j][1] // s == 1 for j in keep)
        lr_wh = (IMG_WH[0] // s, IMG_WH[1] // s)
        for j in keep:
            img = g[f"img{j}"]
            h, w = img.shape[:2]
            st = ip.pil_resize_bicubic(img, (w // s, h // s))
            assert np.array_equal(st, g[f"st{s}_{j}"]), (s, j)
            t = ip.resize_normalize(st, lr_wh, mask=True)
            assert np.array_equal(t[:3], np.transpose(g[f"lr{s}_{j}"].astype(np.float32) / 255.0, (2, 0, 1))), (s, j)
            assert np.array_equal(t[3], g[f"lr{s}_{j}_mask"].astype(np.float32) / 255.0), (s, j)
    assert np.array_equal(g["st2_1"], g["lr2_1"]) and np.array_equal(g["st4_1"], g["lr4_1"])      # 32 x 128: the second resize is an identity
    for j in range(len(sizes)):
        t = ip.resize_normalize(g[f"img{j}"], IMG_WH, mask=True)
        assert np.array_equal(t[:3], np.transpose(g[f"hr{j}"].astype(np.float32) / 255.0, (2, 0, 1))), j
        assert np.array_equal(t[3], g[f"hr{j}_mask"].astype(np.float32) / 255.0), j


def test_oracle_twice_vs_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(40)
    done = 0
    while done < 40:
        h, w, s = int(rng.integers(2, 70)), int(rng.integers(2, 260)), int(rng.choice([2, 3, 4]))
        if h // s == 0 or w // s == 0:
            continue
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        lr_wh = (IMG_WH[0] // s, IMG_WH[1] // s)
        ref = Image.fromarray(img).resize((w // s, h // s), Image.BICUBIC)
        got = ip.pil_resize_bicubic(img, (w // s, h // s))
        assert np.array_equal(got, np.array(ref)), (h, w, s)
        assert np.array_equal(ip.pil_resize_bicubic(got, lr_wh), np.array(ref.resize(lr_wh, Image.BICUBIC))), (h, w, s)
        done += 1
    with pytest.raises(ValueError, match="height and width must be > 0"):
        Image.fromarray(np.zeros((1, 40, 3), np.uint8)).resize((40 // 2, 1 // 2), Image.BICUBIC)


def test_host_coefficient_tables_on_the_pairs_of_the_syn_path():
    from tpgsr_amd import _lib
    lib = _lib.load()
    ns = list(range(2, 40)) + [63, 64, 65, 127, 259, 260, 511]
    pairs = {(n, n // s) for n in ns for s in (2, 3, 4) if n // s} | {(n, o) for n in ns for o in (16, 64, 2 * n)}
    assert (2, 1) in pairs and (3, 1) in pairs and (511, 127) in pairs and (2, 64) in pairs and (511, 1022) in pairs
    for insz, out in sorted(pairs):
        ks = lib.tpgsr_resample_ksize(insz, out)
        b = np.zeros((out, 2), np.int32)
        k = np.zeros((out, ks), np.int32)
        assert lib.tpgsr_resample_coeffs(insz, out, b.ctypes.data, k.ctypes.data) == 0
        for xx, (xmin, kk) in enumerate(ip.resample_coeffs(insz, out)):
            assert len(kk) <= ks and b[xx, 0] == xmin and b[xx, 1] == len(kk), (insz, out, xx)
            assert np.array_equal(k[xx, :len(kk)], kk) and not k[xx, len(kk):].any(), (insz, out, xx)
            assert xmin >= 0 and xmin + len(kk) <= insz                       # what keeps the kernels' reads inside the image


_DRYRUN_CHILD = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
from tpgsr_amd import _lib, data, kernels as K
assert K.DRYRUN
log = []
orig = K._launch
def rec(name, *a):
    entry = dict(name=name, args=a)
    if name == "tpgsr_resize_ragged":            # the descriptor bytes as uploaded (host tensors in a dry run)
        n = a[4]
        entry["src"] = [(d.offset, d.H, d.W) for d in (_lib.ImageDesc * n).from_address(a[1])]
        entry["dst"] = [(d.offset, d.H, d.W, d.xb_off, d.xk_off, d.kx, d.yb_off, d.yk_off, d.ky) for d in (_lib.ImageDesc * n).from_address(a[2])]
    if name == "tpgsr_resize_normalize":
        entry["descs"] = [(d.offset, d.H, d.W, d.xb_off, d.xk_off, d.kx, d.yb_off, d.yk_off, d.ky) for d in (_lib.ImageDesc * a[3]).from_address(a[1])]
    log.append(entry)
    orig(name, *a)                                # the ABI check of the argument list
K._launch = rec
def kernels(entries):
    return sum(2 if e["name"] == "tpgsr_resize_ragged" else 2 + e["args"][7] for e in entries)

g = np.load(os.path.join(%(golden)r, "syn_resize.npz"))
for s in (2, 4):
    imgs = [g["img%%d" %% j] for j in g["idx%%d" %% s]]
    N = len(imgs)
    for mask in (True, False):
        del log[:]
        hr, lr, words, ident = data.AlignCollateSyn(down_sample_scale=s, mask=mask, device="cpu")([(im, "w%%d" %% i) for i, im in enumerate(imgs)])
        assert tuple(hr.shape) == (N, 3 + mask, 32, 128) and tuple(lr.shape) == (N, 3 + mask, 32 // s, 128 // s)
        assert words == ["w%%d" %% i for i in range(N)] and ident == [None] * N
        assert sorted(e["name"] for e in log) == ["tpgsr_resize_normalize"] * 2 + ["tpgsr_resize_ragged"]
        assert kernels(log) <= (8 if mask else 6), kernels(log)
        rag = [e for e in log if e["name"] == "tpgsr_resize_ragged"][0]
        off, want, src = 0, [], []
        poff = 0
        for im in imgs:
            h, w = im.shape[:2]
            want.append((off, h // s, w // s))
            src.append((poff, h, w))
            off += 3 * (h // s) * (w // s)
            poff += im.size
        assert [d[:3] for d in rag["dst"]] == want and rag["src"] == src
        a = rag["args"]
        assert a[4:8] == (N, max(im.shape[0] for im in imgs), max(d[1] for d in want), max(d[2] for d in want))
        # HR reads the uploaded source pixels, LR the ragged output through the SAME descriptor array the ragged launch wrote by
        first, last = [e for e in log if e["name"] == "tpgsr_resize_normalize"]
        assert first["args"][0] == a[0] and [d[:3] for d in first["descs"]] == src and first["args"][4:6] == (32, 128)
        assert last["args"][0] == a[9] and last["args"][1] == a[2] and last["descs"] == rag["dst"] and last["args"][4:7] == (32 // s, 128 // s, a[6])
        assert first["args"][2] == a[3] == last["args"][2]                      # one table buffer
        assert log.index(rag) < log.index(last)

# four-tuples carry their identity; labels=True appends AlignCollate's three tensors
del log[:]
imgs = [g["img0"], g["img3"]]
out = data.AlignCollateSyn(device="cpu", labels=True)([(im, None, w, "p%%d" %% i) for i, (im, w) in enumerate(zip(imgs, ["Hello", "x-y"]))])
assert len(out) == 7 and out[2] == ["Hello", "x-y"] and out[3] == ["p0", "p1"]
ref = data.AlignCollate(device="cpu", labels=True).encode(["Hello", "x-y"])
assert all(tuple(a.shape) == tuple(b.shape) and bool((a == b).all()) for a, b in zip(out[4:], ref))
assert data.AlignCollateSyn.encode is data.AlignCollate.encode               # shared, not copied

# Pillow's ValueError, with the index, before anything is uploaded or launched
for s, bad in ((2, np.zeros((1, 40, 3), np.uint8)), (4, np.zeros((40, 3, 3), np.uint8))):
    del log[:]
    try:
        data.AlignCollateSyn(down_sample_scale=s, device="cpu")([(g["img0"], "a"), (g["img1"], "b"), (bad, "c")])
    except ValueError as e:
        assert "image 2" in str(e) and "%%d x %%d" %% (bad.shape[1], bad.shape[0]) in str(e), str(e)
    else:
        raise AssertionError("no ValueError")
    assert not log
try:
    data.AlignCollateSyn(device="cpu")([(g["img0"].astype(np.float32), "a")])
except ValueError as e:
    assert "uint8" in str(e)
else:
    raise AssertionError("no ValueError")
assert not log

# the empty batch
out = data.AlignCollateSyn(device="cpu", labels=True)([])
assert tuple(out[0].shape) == (0, 4, 32, 128) and tuple(out[1].shape) == (0, 4, 16, 64) and out[2] == [] and out[3] == [] and not log
assert out[4].shape[0] == 0 and out[5].numel() == 0 and out[6].numel() == 0
buf, entries = data.resize_batch([], [], device="cpu")
assert buf.numel() == 0 and buf.dtype.is_floating_point is False and entries == [] and not log

# resize_batch: the public ragged resize
buf, entries = data.resize_batch([g["img2"], g["img4"]], [(18, 10), (7, 3)], device="cpu")
assert entries == [(0, 10, 18), (540, 3, 7)] and buf.numel() == 540 + 63 and [e["name"] for e in log] == ["tpgsr_resize_ragged"]
assert tuple(data.ragged_view(buf, entries[1]).shape) == (3, 7, 3)
print("ok")
"""


def test_align_collate_syn_host_logic_dry_run(golden_dir):
    r = subprocess.run([sys.executable, "-c", _DRYRUN_CHILD % dict(root=ROOT, golden=golden_dir)], capture_output=True, text=True,
                       env=dict(os.environ, TPGSR_PLAN_DRYRUN="1"), timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


def test_value_error_needs_no_device():
    """`w // s == 0` or `h // s == 0` is refused on the host, with the default device, before the device is touched"""
    from tpgsr_amd.data import AlignCollateSyn
    ok = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match=r"image 1 is 40 x 1"):
        AlignCollateSyn(down_sample_scale=2)([(ok, "a"), (np.zeros((1, 40, 3), np.uint8), "b")])
    with pytest.raises(ValueError, match=r"image 0 is 3 x 40"):
        AlignCollateSyn(down_sample_scale=4)([(np.zeros((40, 3, 3), np.uint8), "a"), (ok, "b")])


class _Txn:
    def __init__(self, d):
        self.d = d

    def get(self, k):
        return self.d.get(k)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class FakeLmdbEnv:
    """the two calls the readers make on an lmdb.Environment: begin(write=False) -> txn with .get(key)"""

    def __init__(self, records):
        self.d = records

    def begin(self, write=False):
        assert write is False
        return _Txn(self.d)


def _png(a):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="PNG")
    return buf.getvalue()


def test_lmdb_dataset_hr():
    pytest.importorskip("PIL.Image")
    from tpgsr_amd.data import LmdbDatasetHR
    rng = np.random.default_rng(1)
    imgs = [rng.integers(0, 256, (9 + i, 30 + i, 3), dtype=np.uint8) for i in range(4)]
    recs = {b"num-samples": b"4"}
    recs[b"image_hr-000000001"] = _png(imgs[0])                     # the TextZoom-style key
    recs[b"image-000000002"] = _png(imgs[1])                        # the CRNN-style key: fallback
    recs[b"image_hr-000000003"] = b"not an image"                   # undecodable: skipped
    recs[b"image-000000003"] = _png(imgs[2])                        # (never looked at: image_hr- exists)
    recs[b"image-000000004"] = _png(imgs[3][..., 0])                # grey: converted to RGB
    for i in range(4):
        recs[b"label-%09d" % (i + 1)] = f"Word-{i}!".encode()
    ds = LmdbDatasetHR(env=FakeLmdbEnv(recs), voc_type="lower")
    assert len(ds) == 4
    im, s = ds[0]
    assert np.array_equal(im, imgs[0]) and s == "word0"
    im, s = ds[1]
    assert np.array_equal(im, imgs[1]) and s == "word1"
    im, s = ds[2]                                                   # record 3 cannot be decoded: the next one
    assert np.array_equal(im, np.repeat(imgs[3][..., :1], 3, 2)) and s == "word3"
    assert im.dtype == np.uint8 and im.shape == (12, 33, 3)
    assert LmdbDatasetHR(env=FakeLmdbEnv(recs), voc_type="upper")[0][1] == "Word0"
    assert LmdbDatasetHR(env=FakeLmdbEnv(recs), voc_type="all")[1][1] == "Word-1!"
    assert LmdbDatasetHR(env=FakeLmdbEnv(recs), voc_type="digit")[3][1] == "3"
    bad = {b"num-samples": b"2", b"label-000000001": b"a", b"label-000000002": b"b", b"image-000000001": b"x", b"image_hr-000000002": b"y"}
    with pytest.raises(IOError):                                    # one lap at most, not an unbounded recursion
        LmdbDatasetHR(env=FakeLmdbEnv(bad))[0]


def test_folder_dataset_svt(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from tpgsr_amd.data import FolderDatasetSVT
    rng = np.random.default_rng(2)
    for split in ("svt_train", "svt_test"):
        os.makedirs(tmp_path / split / "IMG")
        os.makedirs(tmp_path / split / "label")
    words = {"a_000": "Hotel", "b_001": "no image", "c_002": "GREY-7", "d_003": "Exit!"}
    for name, word in words.items():
        (tmp_path / "svt_train" / "label" / f"{name}.txt").write_text(word + "\nsecond line\n")
    Image.fromarray(rng.integers(0, 256, (20, 50, 3), dtype=np.uint8)).save(tmp_path / "svt_train" / "IMG" / "a_000.jpg")
    Image.fromarray(rng.integers(0, 256, (17, 41), dtype=np.uint8)).save(tmp_path / "svt_train" / "IMG" / "c_002.jpg")      # grey JPEG
    Image.fromarray(rng.integers(0, 256, (8, 33, 3), dtype=np.uint8)).save(tmp_path / "svt_train" / "IMG" / "d_003.jpg")
    ds = FolderDatasetSVT(str(tmp_path), voc_type="lower")
    assert len(ds) == 4

    def want(name):
        return np.asarray(Image.open(tmp_path / "svt_train" / "IMG" / f"{name}.jpg").convert("RGB"))

    hr, lr, s, path = ds[0]
    assert hr is lr and np.array_equal(hr, want("a_000")) and s == "hotel" and path == str(tmp_path / "svt_train" / "IMG" / "a_000.jpg")
    hr, lr, s, path = ds[1]                                          # b_001 has no image: the next entry
    assert np.array_equal(hr, want("c_002")) and hr.shape == (17, 41, 3) and hr.dtype == np.uint8 and s == "grey7" and path.endswith("c_002.jpg")
    assert np.array_equal(ds[2][0], want("c_002")) and ds[3][2] == "exit"
    assert FolderDatasetSVT(str(tmp_path), voc_type="all")[3][2] == "Exit!"
    assert len(FolderDatasetSVT(str(tmp_path), test=True)) == 0
    (tmp_path / "svt_test" / "label" / "z.txt").write_text("lonely\n")
    with pytest.raises(IOError):                                     # nothing but labels without images: no endless walk
        FolderDatasetSVT(str(tmp_path), test=True)[0]
