"""Training images on the device: a batch of decoded pictures of any sizes -> ``[B, 3, H, W]`` resized with Pillow's
8-bit resampler (byte for byte), cropped, scaled to [0, 1] and normalised -- ``duwu.data.utils.resize_and_crop_image`` for a batch.

The host makes the integer coefficient tables (``uwu_resample_coeffs``: double arithmetic with libm's ``sin``, for the crop window's
output columns and rows only), the device does everything that touches a pixel (``uwu_image_resize_crop``)."""
from dataclasses import dataclass

import numpy as np
import torch

from . import lib as L


def resample_ksize(in_size, out_size, filter="lanczos"):
    k = int(L.load().uwu_resample_ksize(int(in_size), int(out_size), L.FILTER[filter]))
    L.check(min(k, 0), "uwu_resample_ksize")
    return k


def resample_coeffs(in_size, out_size, filter="lanczos", first=0, count=None):
    """Pillow's coefficient tables of one axis for output indices ``first .. first + count - 1`` (all by default):
    ``(coeffs int32 [count, ksize], bounds int32 [count, 2] = (xmin, n))`` as numpy arrays.  Runs on the host: needs no GPU."""
    count = int(out_size) - int(first) if count is None else int(count)
    ksize = resample_ksize(in_size, out_size, filter)
    coeffs = np.empty((max(count, 0), ksize), dtype=np.int32)
    bounds = np.empty((max(count, 0), 2), dtype=np.int32)
    L.call("uwu_resample_coeffs", int(in_size), int(out_size), L.FILTER[filter], int(first), count, coeffs.ctypes.data, bounds.ctypes.data)
    return coeffs, bounds


@dataclass
class RaggedImages:
    """A collated batch of decoded pictures with their resize plans; it takes the samples slot of the 5-tuple until
    ``Fitter._to_device`` turns it into a tensor.

    data     uint8 [sum of h * w * 3]: the pictures, each [h, w, 3], one after the other (pinned when CUDA is available)
    offsets  int64 [B]: where picture b starts in ``data``
    meta     int32 [B, 6]: (src_h, src_w, new_h, new_w, top, left) -- the file's size, the size it is resized to, the crop's offset
    target_size  (width, height) of every output"""
    data: torch.Tensor
    offsets: torch.Tensor
    meta: torch.Tensor
    target_size: tuple
    filter: str = "lanczos"
    normalize: bool = True

    def __len__(self):
        return int(self.meta.shape[0])

    @staticmethod
    def pack(images, plans, target_size, filter="lanczos", normalize=True, pin=None):
        """images: uint8 [h, w, 3] tensors; plans: ``((new_w, new_h), (left, top))`` per picture, as ``plan_resize_and_crop`` gives"""
        sizes = [int(im.numel()) for im in images]
        offsets = torch.tensor([0] + sizes[:-1], dtype=torch.int64).cumsum(0)
        pin = torch.cuda.is_available() if pin is None else pin
        data = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=bool(pin))
        for im, off, n in zip(images, offsets.tolist(), sizes):
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
                raise ValueError(f"RaggedImages.pack: expected uint8 [h, w, 3], got {im.dtype} {tuple(im.shape)}")
            data[off:off + n] = im.reshape(-1)
        meta = torch.tensor([[im.shape[0], im.shape[1], new[1], new[0], top, left] for im, (new, (left, top)) in zip(images, plans)],
                            dtype=torch.int32).reshape(len(images), 6)
        return RaggedImages(data, offsets, meta, (int(target_size[0]), int(target_size[1])), filter, bool(normalize))


def window_tables(meta, target_size, filter="lanczos"):
    """The coefficient and bounds tables of every picture's crop window, in one int32 array, with ``tab_off`` int64 [B, 4]: the
    element offsets of (horizontal coeffs, horizontal bounds, vertical coeffs, vertical bounds); -1 for a pass that is skipped
    because its axis keeps its size.  Pictures whose axis has the same sizes and window share one table: a folder of photographs
    from one camera pays for the vertical tables of a centred axis once per batch."""
    Wt, Ht = int(target_size[0]), int(target_size[1])
    parts, tab_off, at, made = [], [], 0, {}
    for sh, sw, nh, nw, top, left in np.asarray(meta, dtype=np.int64).tolist():
        row = []
        for in_size, out_size, first, count in ((sw, nw, left, Wt), (sh, nh, top, Ht)):
            if in_size == out_size:
                row += [-1, -1]
                continue
            key = (in_size, out_size, first, count)
            if key not in made:
                made[key] = []
                for t in resample_coeffs(in_size, out_size, filter, first, count):
                    made[key].append(at)
                    parts.append(t.reshape(-1))
                    at += t.size
            row += made[key]
        tab_off.append(row)
    tables = np.concatenate(parts) if parts else np.zeros(4, dtype=np.int32)
    return tables, np.asarray(tab_off, dtype=np.int64).reshape(len(tab_off), 4)


def resize_crop(data, offsets, meta, target_size, filter="lanczos", normalize=True, dtype=torch.float32, out=None, ws=None, tables=None):
    """``data`` (uint8, on the device) holds B pictures at ``offsets``; ``meta`` as in :class:`RaggedImages` (both on the host).
    Returns ``[B, 3, Ht, Wt]`` of ``dtype`` on ``data``'s device.  ``tables``: ``(int32 device tensor, tab_off)`` from
    :func:`window_tables` when the caller has made them already."""
    Wt, Ht = int(target_size[0]), int(target_size[1])
    meta = np.ascontiguousarray(np.asarray(meta, dtype=np.int32).reshape(-1, 6))
    offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    B = int(meta.shape[0])
    if offsets.shape[0] != B:
        raise ValueError(f"resize_crop: {offsets.shape[0]} offsets for {B} pictures")
    lib = L.load()
    need = int(lib.uwu_image_resize_crop_ws_bytes(B, meta.ctypes.data, Ht, Wt, L.FILTER[filter]))
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=data.device)
    if out is None:
        out = torch.empty(max(B, 0), 3, Ht, Wt, dtype=dtype, device=data.device)
    if tables is not None:
        tab, tab_off = tables
    else:  # (need == 0: the arguments are bad and the entry point says how; it reads no table before it does)
        host, tab_off = window_tables(meta, target_size, filter) if need else (np.zeros(4, dtype=np.int32), np.zeros((B, 4), dtype=np.int64))
        tab = torch.from_numpy(host).to(data.device)
    tab_off = np.ascontiguousarray(tab_off, dtype=np.int64)
    L.call("uwu_image_resize_crop", L.ptr(data), int(data.numel()), offsets.ctypes.data, meta.ctypes.data, L.ptr(tab), int(tab.numel()),
           tab_off.ctypes.data, L.ptr(out), L.dt(out), B, Ht, Wt, L.FILTER[filter], int(bool(normalize)), L.ptr(ws), int(ws.numel()), L.stream())
    return out


def ragged_to_device(batch: RaggedImages, device, dtype=torch.float32):
    """upload + tables + kernels: the ``[B, 3, H, W]`` tensor the trainer sees"""
    data = batch.data.to(device, non_blocking=True)
    return resize_crop(data, batch.offsets.numpy(), batch.meta.numpy(), batch.target_size, batch.filter, batch.normalize, dtype)
