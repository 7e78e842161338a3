"""Input pipeline contract of the reference on the device.

reference: dataset/dataset.py:615-632 `resizeNormalize(size, mask, interpolation=Image.BICUBIC)` -- Pillow bicubic
`img.resize`, `ToTensor`, luminance-threshold mask channel -- applied per image by `alignCollate_real*`
(dataset/dataset.py:1226-1323: HR -> (128, 32), LR -> (64, 16)) on ONE DataLoader worker; LMDB record keys
dataset/dataset.py:104-149.  Here a whole batch of variable-size uint8 HWC images is resized + normalised + masked by three
kernel launches (csrc/preprocess.hip), bit-exact against Pillow's 8-bit resampling; the host only concatenates the decoded
pixels and Pillow's per-size coefficient tables (cached per (in, out) size pair).  JPEG/PNG decoding and LMDB I/O stay host
work exactly as in the reference (`buf2PIL`).

The reference's other data path, `--syn` (main.py:33, interfaces/base.py:72-107, `alignCollate_syn` dataset/dataset.py:901-992),
makes the LR image itself from HR-only crops: `image.resize((w // s, h // s), BICUBIC)` and then `resizeNormalize`.  Here the first
resize is tpgsr_resize_ragged (every image to its own size, uint8 on the device): `resize_batch`, `AlignCollateSyn`, and the HR-only
readers `LmdbDatasetHR` (`lmdbDataset`, :60-101) and `FolderDatasetSVT` (`lmdbDataset_realSVT`, :242-295)."""
import ctypes as C
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib, kernels as K

NUM_SAMPLES_KEY = b"num-samples"


def lmdb_keys(index: int) -> Dict[str, bytes]:
    """record keys of sample `index` (0-based) in the reference's LMDB layout (1-based, 9 digits)"""
    i = index + 1
    return dict(label=b"label-%09d" % i, image_hr=b"image_hr-%09d" % i, image_lr=b"image_lr-%09d" % i)


_COEFFS: Dict[Tuple[int, int], Tuple[np.ndarray, np.ndarray, int]] = {}


def _coeffs(in_size, out_size):
    """Pillow's (bounds [out][2], taps [out][ksize], ksize) of one (in, out) size pair, computed once per process"""
    key = (in_size, out_size)
    t = _COEFFS.get(key)
    if t is None:
        lib = _lib.load()
        ks = lib.tpgsr_resample_ksize(in_size, out_size)
        b = np.zeros((out_size, 2), np.int32)
        k = np.zeros((out_size, ks), np.int32)
        _lib.check(lib.tpgsr_resample_coeffs(in_size, out_size, b.ctypes.data, k.ctypes.data), "tpgsr_resample_coeffs")
        t = _COEFFS[key] = (b, k, ks)
    return t


class _BatchTables:
    """the coefficient tables one batch needs, concatenated into one int32 buffer: add() returns (bounds offset, taps offset, ksize)"""

    def __init__(self):
        self.parts: List[np.ndarray] = []
        self.size = 0
        self.index: Dict[Tuple[int, int], Tuple[int, int, int]] = {}

    def add(self, in_size, out_size):
        key = (in_size, out_size)
        if key not in self.index:
            b, k, ks = _coeffs(in_size, out_size)
            self.index[key] = (self.size, self.size + b.size, ks)
            self.parts.extend([b.reshape(-1), k.reshape(-1)])
            self.size += b.size + k.size
        return self.index[key]

    def fill(self, d, size_hw, out_wh):
        """table fields of descriptor d for a resize of an H x W image to out_wh = (w, h)"""
        d.xb_off, d.xk_off, d.kx = self.add(size_hw[1], out_wh[0])
        d.yb_off, d.yk_off, d.ky = self.add(size_hw[0], out_wh[1])

    def concat(self):
        return np.concatenate(self.parts)


def _flatten(images):
    """[(flat uint8 pixels, H, W)] of a batch of uint8 [H][W][3] arrays"""
    out = []
    for img in images:
        a = np.ascontiguousarray(img)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"expected uint8 [H][W][3] images, got {a.dtype} {a.shape}")
        out.append((a.reshape(-1), a.shape[0], a.shape[1]))
    return out


def _upload_descs(descs, dev):
    return torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)


def _gpu_only(device, what):
    if not K.DRYRUN and device.type != "cuda":
        raise RuntimeError(f"tpgsr_amd.data.{what} runs on the GPU only (the reference's PIL path is the CPU form)")


class ResizeNormalize:
    """`resizeNormalize((w, h), mask)` for a batch: list of uint8 [H][W][3] arrays -> float tensor (N, 3 + mask, h, w) on `device`."""

    def __init__(self, size: Tuple[int, int], mask: bool = False, device="cuda"):
        self.size, self.mask, self.device = (int(size[0]), int(size[1])), bool(mask), torch.device(device)

    def run(self, pix, dsc, tab, N, maxH):
        """the launches alone: pixels, descriptors [N] and tables already on the device"""
        ow, oh = self.size
        dev = self.device
        tmp = torch.empty(N * maxH * ow * 3, dtype=torch.uint8, device=dev)
        res8 = torch.empty(N * oh * ow * 3, dtype=torch.uint8, device=dev)
        out = torch.empty(N, 4 if self.mask else 3, oh, ow, dtype=torch.float32, device=dev)
        K._launch("tpgsr_resize_normalize", K._p(pix), K._p(dsc), K._p(tab), N, oh, ow, maxH, int(self.mask), K._p(tmp), K._p(res8), K._p(out))
        return out

    def __call__(self, images: Sequence[np.ndarray]) -> torch.Tensor:
        _gpu_only(self.device, "ResizeNormalize")
        ow, oh = self.size
        N = len(images)
        if N == 0:                                        # an empty batch is an empty tensor, not a numpy concatenate error
            return torch.empty(0, 4 if self.mask else 3, oh, ow, dtype=torch.float32, device=self.device)
        descs = (_lib.ImageDesc * N)()
        tabs = _BatchTables()
        poff, maxH = 0, 1
        flat = _flatten(images)
        for d, (a, H, W) in zip(descs, flat):
            d.offset, d.H, d.W = poff, H, W
            tabs.fill(d, (H, W), (ow, oh))
            poff += a.size
            maxH = max(maxH, H)
        dev = self.device
        pix = torch.from_numpy(np.concatenate([a for a, _, _ in flat])).to(dev)
        tab = torch.from_numpy(tabs.concat()).to(dev)
        return self.run(pix, _upload_descs(descs, dev), tab, N, maxH)


def _ragged_layout(flat, sizes_wh, tabs):
    """source and destination descriptors of tpgsr_resize_ragged for flattened images and their (w, h) target sizes: the destination
    images lie back to back, their table fields are left to the caller (the next stage's)"""
    N = len(flat)
    src, dst = (_lib.ImageDesc * N)(), (_lib.ImageDesc * N)()
    poff = ooff = 0
    for n, ((a, H, W), (w1, h1)) in enumerate(zip(flat, sizes_wh)):
        w1, h1 = int(w1), int(h1)
        if w1 <= 0 or h1 <= 0:                           # Pillow: ValueError("height and width must be > 0")
            raise ValueError(f"image {n} ({W} x {H}, W x H): target height and width must be > 0, got ({w1}, {h1})")
        s, d = src[n], dst[n]
        s.offset, s.H, s.W = poff, H, W
        tabs.fill(s, (H, W), (w1, h1))
        d.offset, d.H, d.W = ooff, h1, w1
        poff += a.size
        ooff += 3 * h1 * w1
    return src, dst, ooff


def _run_ragged(pix, src, dst, tab, N, maxH, maxOH, maxOW, out_bytes, dev):
    tmp = torch.empty(N * maxH * maxOW * 3, dtype=torch.uint8, device=dev)
    out8 = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    K.resize_ragged(pix, src, dst, tab, N, maxH, maxOH, maxOW, tmp, out8)
    return out8


def resize_batch(images: Sequence[np.ndarray], sizes_wh: Sequence[Tuple[int, int]], device="cuda"):
    """Pillow's `Image.fromarray(img).resize((w, h), Image.BICUBIC)` for a batch, every image to its own size, bit-exact:
    uint8 [H][W][3] arrays + per-image (w, h) -> (uint8 device buffer with the results back to back, [(offset, h, w)] per image);
    `ragged_view(buf, entry)` is image n as a tensor.  The `--syn` collate's first step and `--random_reso`'s `img.resize((2w, 2h))`."""
    dev = torch.device(device)
    _gpu_only(dev, "resize_batch")
    if len(images) != len(sizes_wh):
        raise ValueError(f"{len(images)} images, {len(sizes_wh)} sizes")
    N = len(images)
    if N == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev), []
    flat = _flatten(images)
    tabs = _BatchTables()
    src, dst, out_bytes = _ragged_layout(flat, sizes_wh, tabs)
    pix = torch.from_numpy(np.concatenate([a for a, _, _ in flat])).to(dev)
    tab = torch.from_numpy(tabs.concat()).to(dev)
    dsc = _upload_descs(bytes(src) + bytes(dst), dev)
    nb = N * C.sizeof(_lib.ImageDesc)
    out8 = _run_ragged(pix, dsc[:nb], dsc[nb:], tab, N, max(d.H for d in src), max(d.H for d in dst), max(d.W for d in dst), out_bytes, dev)
    return out8, [(int(d.offset), int(d.H), int(d.W)) for d in dst]


def ragged_view(buf: torch.Tensor, entry: Tuple[int, int, int]) -> torch.Tensor:
    """image (offset, h, w) of resize_batch's buffer as a uint8 [h][w][3] view"""
    off, h, w = entry
    return buf[off:off + 3 * h * w].view(h, w, 3)


class LabelEncoder:
    """the label tensors of `alignCollate_realWTLAMask`, shared by the collates: `a2d` maps a character to its class index"""

    D2A = "-0123456789abcdefghijklmnopqrstuvwxyz"      # dataset/dataset.py:1108-1116: index 0 is the CTC blank

    def encode(self, label_strs):
        """dataset/dataset.py:1255-1323: lower-case, words of 15 characters and more cut to 15, characters outside the alphabet dropped;
        a word without any label gets one blank (index 0) and weight 0; max_len = the longest word (not label list)"""
        alsize = len(self.D2A)
        lists, max_len = [], 0
        for word in label_strs:
            word = word.lower()
            if len(word) >= 15:
                word = word[:15]
            lists.append([self.a2d[ch] for ch in word if ch in self.a2d])
            max_len = max(max_len, len(word))
        label_vecs = torch.zeros(len(lists), max(max_len, 1), alsize)
        mask, tics = [], []
        for i, ll in enumerate(lists):
            if ll:
                label_vecs[i, torch.arange(len(ll)), torch.tensor(ll)] = 1.0
                mask.extend(ll)
                tics.append(1)
            else:
                label_vecs[i, 0, 0] = 1.0
                mask.append(0)
                tics.append(0)
        return label_vecs.unsqueeze(1).permute(0, 3, 1, 2).contiguous(), torch.tensor(mask, dtype=torch.long), torch.tensor(tics)


class AlignCollate(LabelEncoder):
    """`alignCollate_real*` (dataset/dataset.py:1226-1323) reduced to what the training loop consumes: a list of
    (HR image, LR image, label string) -> (images_HR (N, C, imgH, imgW), images_lr (N, C, imgH/ds, imgW/ds), label_strs);
    with `labels=True` (`alignCollate_realWTLAMask`, what `--use_label` trains on) also label_vecs (N, 37, 1, L) one-hot,
    weighted_mask (all label indices concatenated) and weighted_tics (N) -- the three tensors TPGSRTrainStep.step(labels=) takes."""

    def __init__(self, imgH=32, imgW=128, down_sample_scale=2, mask=True, device="cuda", labels=False):
        self.hr = ResizeNormalize((imgW, imgH), mask, device)
        self.lr = ResizeNormalize((imgW // down_sample_scale, imgH // down_sample_scale), mask, device)
        self.labels = bool(labels)
        self.a2d = {ch: i for i, ch in enumerate(self.D2A)}

    def __call__(self, batch):
        images_hr, images_lr, label_strs = zip(*batch)
        out = (self.hr(images_hr), self.lr(images_lr), list(label_strs))
        return out + self.encode(label_strs) if self.labels else out


class AlignCollateSyn(LabelEncoder):
    """`alignCollate_syn.__call__` (dataset/dataset.py:952-992), the `--syn` path: HR-only items (image, label_str) or
    (image, ignored, label_str, identity) -> (images_hr, images_lr, label_strs, identity); `identity` is None for two-tuples.
    images_hr = resizeNormalize((imgW, imgH)) of the source; images_lr = resizeNormalize((imgW // s, imgH // s)) of
    `image.resize((w // s, h // s), Image.BICUBIC)` -- two Pillow resizes, each rounded and clamped to 8 bits, so not one.
    The source pixels, the tables and the descriptors go up once each; tpgsr_resize_ragged leaves the intermediate images on the
    device and its destination descriptors are the LR stage's input.  With `labels=True` the three tensors of `encode` follow."""

    def __init__(self, imgH=32, imgW=128, down_sample_scale=2, mask=True, device="cuda", labels=False, train=True):
        self.scale, self.train = int(down_sample_scale), train           # `train`: kept as the reference keeps it (only its dead blur reads it)
        self.hr = ResizeNormalize((imgW, imgH), mask, device)
        self.lr = ResizeNormalize((imgW // self.scale, imgH // self.scale), mask, device)
        self.device = self.hr.device
        self.labels = bool(labels)
        self.a2d = {ch: i for i, ch in enumerate(self.D2A)}

    def layout(self, images):
        """host side of one batch, nothing uploaded: (flat images, hr descs, src descs, dst descs, tables, bytes of the intermediate)"""
        flat = _flatten(images)
        s = self.scale
        for n, (_, H, W) in enumerate(flat):
            if W // s == 0 or H // s == 0:               # Pillow: ValueError("height and width must be > 0")
                raise ValueError(f"image {n} is {W} x {H} (W x H): no pixel is left after down_sample_scale {s}")
        tabs = _BatchTables()
        hr = (_lib.ImageDesc * len(flat))()
        src, dst, mid_bytes = _ragged_layout(flat, [(W // s, H // s) for _, H, W in flat], tabs)
        for h, sd, d in zip(hr, src, dst):
            h.offset, h.H, h.W = sd.offset, sd.H, sd.W
            tabs.fill(h, (sd.H, sd.W), self.hr.size)
            tabs.fill(d, (d.H, d.W), self.lr.size)
        return flat, hr, src, dst, tabs, mid_bytes

    def __call__(self, batch):
        _gpu_only(self.device, "AlignCollateSyn")
        batch = list(batch)
        if batch and len(batch[0]) == 2:
            images, label_strs = zip(*batch)
            identity = [None] * len(batch)
        elif batch:
            images, _, label_strs, identity = zip(*batch)
        else:
            images = label_strs = identity = ()
        N, dev = len(images), self.device
        if N == 0:
            out = (self.hr(()), self.lr(()), [], [])
        else:
            flat, hr, src, dst, tabs, mid_bytes = self.layout(images)
            pix = torch.from_numpy(np.concatenate([a for a, _, _ in flat])).to(dev)
            tab = torch.from_numpy(tabs.concat()).to(dev)
            dsc = _upload_descs(bytes(hr) + bytes(src) + bytes(dst), dev)
            nb = N * C.sizeof(_lib.ImageDesc)
            maxH, maxH1, maxW1 = max(d.H for d in src), max(d.H for d in dst), max(d.W for d in dst)
            images_hr = self.hr.run(pix, dsc[:nb], tab, N, maxH)
            mid = _run_ragged(pix, dsc[nb:2 * nb], dsc[2 * nb:], tab, N, maxH, maxH1, maxW1, mid_bytes, dev)
            out = (images_hr, self.lr.run(mid, dsc[2 * nb:], tab, N, maxH1), list(label_strs), list(identity))
        return out + self.encode(label_strs) if self.labels else out


class LmdbDatasetReal:
    """`lmdbDataset_real` (dataset/dataset.py:104-149): (HR, LR, label) triples from the reference's LMDB layout, decoded to
    uint8 arrays for AlignCollate.  Needs `lmdb` (unless an opened environment is handed in as `env`) and `PIL`, like the reference.
    As in the reference, a record whose images cannot be decoded is SKIPPED: `self[index]` returns the next sample (:141-146)."""

    def __init__(self, root=None, voc_type="upper", max_len=100, test=False, env=None):
        if env is None:
            try:
                import lmdb
            except ImportError as e:
                raise ImportError("LmdbDatasetReal needs the `lmdb` package (as the reference's dataset/dataset.py does)") from e
            env = lmdb.open(root, max_readers=1, readonly=True, lock=False, readahead=False, meminit=False)
        if not env:
            raise RuntimeError(f"cannot open lmdb from {root}")
        self.env = env
        with self.env.begin(write=False) as txn:
            self.nSamples = int(txn.get(NUM_SAMPLES_KEY))
        self.voc_type, self.max_len, self.test = voc_type, max_len, test

    def __len__(self):
        return self.nSamples

    def __getitem__(self, index):
        import io
        from PIL import Image
        from .utils.metrics import str_filt
        assert index <= len(self), "index range error"               # (the reference's own guard, dataset.py:131)
        for probe in range(index, index + len(self) + 1):              # at most one lap: the reference recurses on self[index + 1]
            keys = lmdb_keys(probe % max(1, len(self)))
            with self.env.begin(write=False) as txn:
                word, buf_hr, buf_lr = txn.get(keys["label"]), txn.get(keys["image_hr"]), txn.get(keys["image_lr"])
            try:
                if word is None or buf_hr is None or buf_lr is None:
                    raise IOError(f"missing record {probe}")
                hr = np.asarray(Image.open(io.BytesIO(buf_hr)).convert("RGB"))
                lr = np.asarray(Image.open(io.BytesIO(buf_lr)).convert("RGB"))
            except (IOError, OSError, SyntaxError, ValueError):
                continue
            return hr, lr, str_filt(word.decode(), self.voc_type)
        raise IOError("no decodable record in the LMDB")


class LmdbDatasetHR:
    """`lmdbDataset` (dataset/dataset.py:60-101), the HR-only reader of the `--syn` path (SVT, IC15, IIIT5K, COCO-Text or any
    CRNN-style LMDB): (image, label string) per record, the image under `image_hr-%09d` or, where that key is absent, `image-%09d`,
    decoded to a uint8 RGB array for AlignCollateSyn.  `env=` takes an opened environment.  A record that cannot be decoded is
    SKIPPED like in LmdbDatasetReal -- the next sample, one lap at most (the reference recurses on self[index + 1] without a bound)."""

    def __init__(self, root=None, voc_type="upper", max_len=31, test=True, env=None):
        if env is None:
            try:
                import lmdb
            except ImportError as e:
                raise ImportError("LmdbDatasetHR needs the `lmdb` package (as the reference's dataset/dataset.py does)") from e
            env = lmdb.open(root, max_readers=1, readonly=True, lock=False, readahead=False, meminit=False)
        if not env:
            raise RuntimeError(f"cannot open lmdb from {root}")
        self.env = env
        with self.env.begin(write=False) as txn:
            self.nSamples = int(txn.get(NUM_SAMPLES_KEY))
        self.voc_type, self.max_len, self.test = voc_type, max_len, test

    def __len__(self):
        return self.nSamples

    def __getitem__(self, index):
        import io
        from PIL import Image
        from .utils.metrics import str_filt
        assert index <= len(self), "index range error"               # (the reference's own guard, dataset.py:86)
        for probe in range(index, index + len(self) + 1):
            i = probe % max(1, len(self)) + 1
            with self.env.begin(write=False) as txn:
                word, buf = txn.get(b"label-%09d" % i), txn.get(b"image_hr-%09d" % i)
                if buf is None:
                    buf = txn.get(b"image-%09d" % i)
            try:
                if word is None or buf is None:
                    raise IOError(f"missing record {probe}")
                img = np.asarray(Image.open(io.BytesIO(buf)).convert("RGB"))
            except (IOError, OSError, SyntaxError, ValueError):
                continue
            return img, str_filt(word.decode(), self.voc_type)
        raise IOError("no decodable record in the LMDB")


class FolderDatasetSVT:
    """`lmdbDataset_realSVT` (dataset/dataset.py:242-295): word crops in `<root>/svt_train|svt_test/IMG/<name>.jpg` with the word
    on the first line of `.../label/<name>.txt` -> (image, image, label string, image path), the four-tuple AlignCollateSyn takes.
    A label without its image file moves on to the next entry (one lap at most).  Labels are listed in sorted order (the reference
    takes os.listdir's).  Images are converted to RGB: the reference does not convert, and its collate's `torch.cat` then fails on a
    grey JPEG between colour ones."""

    def __init__(self, root, voc_type="upper", max_len=100, test=False):
        import os
        split = os.path.join(root, "svt_test" if test else "svt_train")
        self.image_dir, self.anno_dir = os.path.join(split, "IMG"), os.path.join(split, "label")
        self.anno_list = sorted(os.listdir(self.anno_dir))
        self.nSamples = len(self.anno_list)
        self.voc_type, self.max_len, self.test = voc_type, max_len, test

    def __len__(self):
        return self.nSamples

    def __getitem__(self, index):
        import os
        from PIL import Image
        from .utils.metrics import str_filt
        for probe in range(index, index + len(self)):
            anno = self.anno_list[probe % len(self)]
            image_path = os.path.join(self.image_dir, anno.split(".")[0] + ".jpg")
            if not os.path.isfile(image_path):
                continue
            try:
                with open(os.path.join(self.anno_dir, anno), "r") as f:
                    word = f.readline().replace("\n", "")
                img = np.asarray(Image.open(image_path).convert("RGB"))
            except (IOError, OSError, SyntaxError, ValueError):
                continue
            return img, img, str_filt(word, self.voc_type), image_path
        raise IOError(f"no label with a readable image under {self.image_dir}")
