"""GPU input pipeline: decoded uint8 image + full-res density -> network inputs.

Same result as CrowdDataset's CPU transform (data/transforms.py:prepare_pair,
reference model/CrowdDataset.py:38-67) but computed by csrc/preprocess.hip
on the GPU, writing the first conv layer's NHWC4 bf16 layout directly.

Per batch: the DataLoader worker packs the decoded samples back to back
(``PackedCollate``: the images, the fp32 ground truth and a descriptor table
in ONE uint8 buffer), the main process makes one pinned H2D copy of it and
ONE kernel launch turns the batch into network inputs (``preprocess_packed``).
``preprocess_batch`` is the per-sample form (tests / variable-size use).
``PackedCollate(crop=(ch, cw))`` packs random-crop batches: every image once,
one descriptor per crop, cut on the GPU by one launch of the crop kernel;
with ``crop_scale=True`` every descriptor carries its window's extent and the
resize launch's kernel resamples it to the crop.  With ``gt_from_heads=True``
a cropped pack carries the images' head records instead of ground-truth
values and a second launch on the same stream (csrc/density.hip,
gt_from_heads_kernel) renders the ground truth region of the buffer from
them.  With ``photo=True`` a cropped pack ends with one tone-table row per
output sample and the image launch goes through the photo entry (README,
"Photometric jitter").  A pack of any kind goes through one collate loop,
``_unpack`` and ``_launch``.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from . import _ext
from .conv import dt_code


def preprocess_batch(images: Sequence[torch.Tensor], densities: Sequence[torch.Tensor], flips: Sequence[bool],
                     device, downsample: int = 8, dtype: torch.dtype = torch.bfloat16) -> Tuple[torch.Tensor, torch.Tensor]:
    """images: uint8 [H,W] / [H,W,C] (CPU or GPU), densities: fp32 [h,w] of any size (resized to the image's 1/d).  All samples must
    resize to the same (H//d*d, W//d*d).  Returns (x4 [N,Ho,Wo,4] bf16/fp16, gt [N,1,Ho/d,Wo/d] fp32)."""
    C = _ext.require()
    dev = torch.device(device)
    n = len(images)
    if not (n == len(densities) == len(flips)) or n == 0:
        raise ValueError("images, densities and flips must have the same non-zero length")
    h0, w0 = images[0].shape[:2]
    ho, wo = (h0 // downsample) * downsample, (w0 // downsample) * downsample
    dt = dt_code(dtype)
    x4 = torch.empty(n, ho, wo, 4, dtype=dtype, device=dev)
    gt = torch.empty(n, 1, ho // downsample, wo // downsample, dtype=torch.float32, device=dev)
    st = _ext.stream_ptr(dev)
    for i, (im, dm, fl) in enumerate(zip(images, densities, flips)):
        if im.dtype != torch.uint8:
            raise ValueError("images must be uint8 (decoded JPEG/PNG)")
        hh, ww = im.shape[:2]
        if (hh // downsample * downsample, ww // downsample * downsample) != (ho, wo):
            raise ValueError("all samples of a batch must resize to the same shape")
        im = im.to(dev, non_blocking=True).contiguous()
        ch = 1 if im.dim() == 2 else im.shape[2]
        dm = dm.to(dev, dtype=torch.float32, non_blocking=True).contiguous()
        if dm.dim() != 2:
            raise ValueError("density must be a 2-D map")
        C.preprocess_image(im.data_ptr(), hh, ww, ch, int(bool(fl)), x4[i].data_ptr(), ho, wo, dt, st)
        # a density map of any size is resized to the image's (H//d, W//d) (reference model/CrowdDataset.py:60)
        C.preprocess_density(dm.data_ptr(), dm.shape[0], dm.shape[1], int(bool(fl)), gt[i].data_ptr(), ho // downsample,
                             wo // downsample, float(downsample * downsample), st)
    return x4, gt


class PackedCollate:
    """collate_fn for CrowdDataset(raw=True) that packs a batch for ONE H2D copy and ONE launch: returns
    (buf uint8, (n, Ho, Wo, gt_offset, desc_offset)) where buf holds the images back to back (bytes
    [0, sum of H*W*C)), the fp32 ground truth [n,1,Ho/d,Wo/d] at gt_offset and the int64 descriptors [n, 8] at
    desc_offset (16-byte aligned), desc[i] = (image byte offset, H0, W0, C, flip, 0, 0, 0).  The raw dataset already
    brought each ground truth to 1/d resolution (flip and x d^2 included), so only the images are resized on the
    GPU.  Runs in the loader workers; pin_memory=True pins the buffer.  (Three separate pinned copies per batch were
    ~0.23 ms of host time per step at batch 1: profiles/r5/host/.)

    crop=(ch, cw): the random-crop form, for CrowdDataset(raw=True, crop=...) items (uint8 image, gts
    [K,1,ch/d,cw/d], windows [K,3] of (y0, x0, flip)): every image's bytes ONCE, the [B*K,1,ch/d,cw/d] ground truth
    and one descriptor per output sample, desc = (image byte offset, H0, W0, C, flip, y0, x0, 1) -- the K crops of an
    image share its offset.  The meta tuple gains a sixth field, the number of images, which marks the pack as cropped.
    crop_scale=True: the windows are [K,5] of (y0, x0, flip, sh, sw), slot 7 of a descriptor is (sh << 32) | sw (never
    the unscaled 1) and the meta tuple gains a seventh field, 1, which marks the pack as scaled.
    gt_from_heads=True (with crop, scaled or not): for CrowdDataset(raw=True, crop=..., gt_from_heads=True) items
    (uint8 image, head records [N,4] fp32, windows).  The ground truth region is zero (the GPU renders it in place),
    and behind the descriptors follow the int64 ranges [n, 2] = (first head, head count) of every output sample -- the
    K crops of an image share one range -- and the head table [sum N, 4] fp32, both 16-byte aligned.  The meta tuple
    has eight fields, (..., images, scaled 0 / 1, heads in the table), a length no other kind has.
    photo=True (with crop, any of the four kinds): for CrowdDataset(..., photo_jitter= / gray_prob=) items, which carry
    a fourth element, float32 [K, 257] (tone table, gray flag).  Everything above is packed as without it, byte for
    byte, and behind it (16-byte aligned) follows the photo region float32 [n, 260], one row per output sample: the 256
    table entries, the gray flag, three zeros.  The meta tuple has nine fields, a length no other kind has:
    (n, Ho, Wo, gt_offset, desc_offset, images, kind, heads, photo_offset), kind the index 1 / 2 into KINDS and heads -1
    without a head table."""

    PHOTO_ROW = 260                               # floats per row of the photo region (csrc/preprocess.hip)

    def __init__(self, downsample: int = 8, crop=None, crop_scale=False, gt_from_heads=False, photo=False):
        self.ds = downsample
        self.crop_scale = bool(crop_scale)
        self.gt_from_heads = bool(gt_from_heads)
        self.photo = bool(photo)
        if self.photo and crop is None:
            raise ValueError("photo needs crop=(ch, cw)")
        if self.crop_scale and crop is None:
            raise ValueError("crop_scale needs crop=(ch, cw)")
        if self.gt_from_heads and crop is None:
            raise ValueError("gt_from_heads needs crop=(ch, cw)")
        self.crop = None if crop is None else (int(crop[0]), int(crop[1]))
        if self.crop is not None and (min(self.crop) <= 0 or self.crop[0] % downsample or self.crop[1] % downsample):
            raise ValueError(f"crop {self.crop} must be a positive multiple of the downsample {downsample}")

    def _windows(self, im, g, third, ho, wo):
        """The (flip, y0, x0, slot 7) of every output sample of one item, checked against the pack's kind."""
        d = self.ds
        if self.crop is None:
            if (im.shape[0] // d * d, im.shape[1] // d * d) != (ho, wo):
                raise ValueError("all samples of a batch must resize to the same shape")
            if tuple(g.shape) != (1, ho // d, wo // d):
                raise ValueError("raw samples must carry the 1/d ground truth [1, H/d, W/d]")
            return [(int(bool(third)), 0, 0, 0)]
        nw = 5 if self.crop_scale else 3
        if self.gt_from_heads:
            if g.dim() != 2 or g.shape[1] != 4 or g.dtype != torch.float32 or third.dim() != 2 or third.shape[1] != nw:
                raise ValueError(f"cropped raw samples with gt_from_heads must carry head records [N, 4] fp32 and "
                                 f"windows [K, {nw}]")
        elif g.dim() != 4 or tuple(g.shape[1:]) != (1, ho // d, wo // d) or tuple(third.shape) != (g.shape[0], nw):
            raise ValueError(f"cropped raw samples must carry ground truths [K, 1, ch/d, cw/d] and windows [K, {nw}]")
        if not self.crop_scale:
            return [(fl, y0, x0, 1) for y0, x0, fl in third.tolist()]
        if int(third[:, 3:].min()) < 1 or int(third[:, 3:].max()) > 0x7fffffff:
            raise ValueError("scaled windows must have extents 1 <= sh, sw < 2^31")
        return [(fl, y0, x0, (sh << 32) | sw) for y0, x0, fl, sh, sw in third.tolist()]

    def _photo_region(self, photos, n):
        """float32 [n, PHOTO_ROW] from the items' [K, 257] rows: table, gray flag, three zeros."""
        for ph in photos:
            if not torch.is_tensor(ph) or ph.dtype != torch.float32 or ph.dim() != 2 or ph.shape[1] != 257:
                raise ValueError("photo items must carry float32 [K, 257] rows (tone table, gray flag)")
        rows = torch.cat(photos)
        if rows.shape[0] != n:
            raise ValueError(f"photo rows: {rows.shape[0]} for {n} output samples")
        region = torch.zeros(n, self.PHOTO_ROW)
        region[:, :257] = rows
        return region

    @staticmethod
    def _fill(imgs, ioff, gt, desc, tail=None):
        """One buffer: the images back to back | the ground truth at goff | the descriptors at doff (16-byte aligned),
        then ``tail`` (the ranges and the head table of a heads pack, the photo region of a photo pack: multiples of
        16 bytes after 64 n)."""
        goff = -(-ioff // 16) * 16
        doff = -(-(goff + 4 * gt.numel()) // 16) * 16
        buf = torch.empty(doff + 8 * desc.numel() + (0 if tail is None else tail.numel()), dtype=torch.uint8)
        o = 0
        for im in imgs:
            k = im.numel()
            buf[o:o + k] = im.reshape(-1)
            o += k
        buf[goff:goff + 4 * gt.numel()] = gt.reshape(-1).view(torch.uint8)
        buf[doff:doff + 8 * desc.numel()] = desc.reshape(-1).view(torch.uint8)
        if tail is not None:
            buf[doff + 8 * desc.numel():] = tail
        return buf, goff, doff

    def __call__(self, batch: List):
        if any(len(item) != 3 + self.photo for item in batch):
            raise ValueError("a photo collate takes the 4-element items of a dataset with photo_jitter / gray_prob, "
                             "every other collate 3-element items")
        imgs, gts, thirds = list(zip(*batch))[:3]  # the third field: a flip (uncropped) or the [K, 3 / 5] windows
        if self.crop is None:
            ho, wo = (imgs[0].shape[0] // self.ds) * self.ds, (imgs[0].shape[1] // self.ds) * self.ds
        else:
            ho, wo = self.crop
        rows, ranges, ioff, hoff = [], [], 0, 0
        for im, g, third in zip(imgs, gts, thirds):
            hh, ww = im.shape[:2]
            c = 1 if im.dim() == 2 else im.shape[2]
            wins = self._windows(im, g, third, ho, wo)
            rows += [[ioff, hh, ww, c, *w] for w in wins]
            ioff += hh * ww * c
            if self.gt_from_heads:
                ranges += [[hoff, g.shape[0]]] * len(wins)
                hoff += g.shape[0]
        desc = torch.tensor(rows, dtype=torch.int64)
        tails = []
        if self.gt_from_heads:
            gt = torch.zeros(len(rows), 1, ho // self.ds, wo // self.ds)
            tails = [torch.tensor(ranges, dtype=torch.int64).reshape(-1).view(torch.uint8),
                     torch.cat(gts).contiguous().reshape(-1).view(torch.uint8)]
        else:
            gt = (torch.stack(gts) if self.crop is None else torch.cat(gts)).float().contiguous()
        if self.photo:
            tails.append(self._photo_region([item[3] for item in batch], len(rows)).reshape(-1).view(torch.uint8))
        buf, goff, doff = self._fill(imgs, ioff, gt, desc, torch.cat(tails) if tails else None)
        if self.photo:
            return buf, (len(rows), ho, wo, goff, doff, len(imgs), 1 + int(self.crop_scale),
                         hoff if self.gt_from_heads else -1, buf.numel() - 4 * self.PHOTO_ROW * len(rows))
        if self.gt_from_heads:
            return buf, (len(rows), ho, wo, goff, doff, len(imgs), int(self.crop_scale), hoff)
        kind = () if self.crop is None else (len(imgs), 1) if self.crop_scale else (len(imgs),)
        return buf, (len(rows), ho, wo, goff, doff) + kind


KINDS = ("batch", "crop", "crop_scaled")         # a pack's kind: the C.preprocess_<kind> entry that takes it


def _unpack(packed):
    """(buf, (n, Ho, Wo, gt_offset, desc_offset), kind) of a PackedCollate output, kind one of KINDS: a cropped
    pack's meta tuple carries a sixth field (its number of images) and n counts output samples, one descriptor each;
    a scaled pack's carries a seventh, 1.  A heads pack's meta tuple has eight fields (images, scaled 0 / 1, heads):
    its kind is "crop+heads" or "crop_scaled+heads", and its buffer ends with the ranges and the head table.  A photo
    pack's has nine (images, kind 1 / 2, heads or -1, photo_offset): its kind ends with "+photo", and its buffer with
    the photo region [n, 260] fp32 at photo_offset."""
    buf, meta = packed
    n, ho, wo, goff, doff = meta[:5]
    photo = len(meta) == 9
    heads = len(meta) == 8 or (photo and meta[7] >= 0)
    meta_ok = len(meta) in (5, 6) or (len(meta) == 7 and meta[6] == 1) or \
        (len(meta) == 8 and meta[6] in (0, 1) and meta[7] >= 0) or (photo and meta[6] in (1, 2) and meta[7] >= -1)
    size = doff + 64 * n + ((16 * n + 16 * meta[7]) if heads and meta_ok else 0)
    if photo and meta_ok:
        meta_ok = meta[8] == size                 # right behind what the pack holds without it (a multiple of 16)
        size += 4 * PackedCollate.PHOTO_ROW * n
    buf_ok = buf.dtype == torch.uint8 and buf.dim() == 1 and buf.numel() == size
    if not (meta_ok and buf_ok) or goff % 16 or doff % 16:
        raise ValueError("packed batch: one uint8 buffer (images | fp32 ground truth | int64 descriptors"
                         " [| int64 head ranges | fp32 head records] [| fp32 photo rows])")
    if photo:
        return buf, (n, ho, wo, goff, doff), KINDS[meta[6]] + ("+heads" if heads else "") + "+photo"
    if heads:
        return buf, (n, ho, wo, goff, doff), KINDS[1 + meta[6]] + "+heads"
    return buf, (n, ho, wo, goff, doff), KINDS[len(meta) - 5]


def _launch(C, kind, buf, d, n, ho, wo, goff, doff, downsample, dtype, device, roi=False):
    """The one launch of a pack of any kind: d, the device copy of buf -> (x4, gt), gt a view of d.  The crop entries
    check the host descriptors (in buf) before they launch, the photo entry the host photo rows as well.
    roi: the pack's images are 4-channel with the ROI mask as alpha (CrowdDataset(roi=True)); after the pack's other
    launches, on the same stream, roi_weights_kernel writes gt2 [n,2,ho/d,wo/d] (the ground truth, the loss weights)
    and (x4, gt2) is returned.  Its check runs on the host descriptors before ANY launch."""
    hd, wd = ho // downsample, wo // downsample
    gt = d[goff:goff + 4 * n * hd * wd].view(torch.float32).view(n, 1, hd, wd)
    desc = d[doff:doff + 64 * n].view(torch.int64).view(n, 8)
    x4 = torch.empty(n, ho, wo, 4, dtype=dtype, device=device)
    tail = (ho, wo, downsample, dt_code(dtype), _ext.stream_ptr(device))
    kind, *flags = kind.split("+")
    heads, photo = "heads" in flags, "photo" in flags
    poff = buf.numel() - (4 * PackedCollate.PHOTO_ROW * n if photo else 0)      # the photo region ends the buffer
    if roi:
        rc = C.roi_weights_check(buf.data_ptr() + doff, n, goff, ho, wo, downsample)
        if rc:
            raise RuntimeError(f"roi_weights refused the pack (code {rc}: -31 an image without a mask channel, -32 a "
                               "sample size that is no multiple of the downsample, -33 a window outside its image)")
    if heads:
        # checked on the host copies before EITHER launch (a refused pack launches nothing); the render itself is
        # issued right after the image launch, on the same stream
        roff, hoff = doff + 64 * n, doff + 80 * n
        nh = (poff - hoff) // 16
        rc = C.gt_from_heads_check(buf.data_ptr() + hoff, nh, buf.data_ptr() + roff, buf.data_ptr() + doff, n, ho, wo,
                                   downsample)
        if rc:
            raise RuntimeError(f"gt_from_heads refused the pack (code {rc})")
    if kind == "batch":
        C.preprocess_batch(d.data_ptr(), 0, desc.data_ptr(), n, x4.data_ptr(), 0, *tail)
    elif photo:
        C.preprocess_crop_photo(d.data_ptr(), goff, desc.data_ptr(), buf.data_ptr() + doff, n, x4.data_ptr(), *tail,
                                d.data_ptr() + poff, buf.data_ptr() + poff, int(kind == "crop_scaled"))
    else:
        getattr(C, "preprocess_" + kind)(d.data_ptr(), goff, desc.data_ptr(), buf.data_ptr() + doff, n, x4.data_ptr(),
                                         *tail)
    if heads:
        C.gt_from_heads(d.data_ptr() + hoff, d.data_ptr() + roff, desc.data_ptr(), buf.data_ptr() + hoff, nh,
                        buf.data_ptr() + roff, buf.data_ptr() + doff, n, gt.data_ptr(), ho, wo, downsample, tail[-1])
    if roi:
        gt2 = torch.empty(n, 2, hd, wd, dtype=torch.float32, device=device)
        C.roi_weights(d.data_ptr(), goff, desc.data_ptr(), buf.data_ptr() + doff, n, gt.data_ptr(), gt2.data_ptr(),
                      ho, wo, downsample, tail[-1])
        return x4, gt2
    return x4, gt


def preprocess_packed(packed, device, downsample: int = 8, dtype: torch.dtype = torch.bfloat16,
                      copy_stream=None, roi: bool = False):
    """PackedCollate output -> (x4 [N,Ho,Wo,4] 16-bit NHWC4, gt [N,1,Ho/d,Wo/d] fp32): one copy of the packed buffer
    and one launch for the whole batch of images.  copy_stream: a torch.cuda.Stream the H2D copy is issued on (the
    compute stream then waits for it): a pinned copy queued behind the previous step's kernels on the compute stream
    held the host ~0.6 ms per step at batch 1 (profiles/r5/host/), one on an idle copy stream does not.
    roi=True (a CrowdDataset(roi=True) pack): returns (x4, gt2 [N,2,Ho/d,Wo/d]), the loss weights in channel 1."""
    C = _ext.require()
    buf, dims, kind = _unpack(packed)
    dev = torch.device(device)
    if copy_stream is not None:
        cur = torch.cuda.current_stream(dev)
        with torch.cuda.stream(copy_stream):
            d = buf.to(dev, non_blocking=True)
        cur.wait_stream(copy_stream)
        d.record_stream(cur)              # allocated on the copy stream, consumed on the compute stream
    else:
        d = buf.to(dev, non_blocking=True)
    return _launch(C, kind, buf, d, *dims, downsample, dtype, dev, roi=roi)


class AheadPrep:
    """The training loop's GPU input pipeline, one batch ahead (engine/train_eval.py train_one_epoch_native).

    ``issue(packed)`` queues the packed batch's H2D copy AND its preprocessing kernel on a copy stream (outputs
    allocated there) and returns a handle; ``ready(handle)`` makes the compute stream wait for it (one event) and
    hands the tensors over (record_stream).  Issued right after the previous step was queued, the copy and the resize /
    normalise kernel run under that step's kernels on the copy stream, so the compute stream's next step waits on
    nothing: with preprocess_packed(copy_stream=...) the kernel ran on the compute stream behind a wait for the copy.
    """

    def __init__(self, device, dtype: torch.dtype = torch.bfloat16, downsample: int = 8, roi: bool = False):
        self.roi = bool(roi)                  # the packs carry ROI masks: gt comes back [n, 2, h, w] (_launch)
        self.device = torch.device(device)
        self.dtype = dtype
        self.ds = downsample
        self.copy = torch.cuda.Stream(self.device)

    def issue(self, packed):
        C = _ext.require()
        buf, dims, kind = _unpack(packed)
        # the copy stream must not overwrite memory the compute stream's queued kernels may still read: wait for
        # what the compute stream has queued so far is NOT needed (fresh blocks of the copy stream's own pool), and
        # the hand-off below keeps the blocks out of that pool until the compute stream is done with them
        with torch.cuda.stream(self.copy):
            d = buf.to(self.device, non_blocking=True)
            with _ext.launch_on(self.copy.cuda_stream):
                x4, gt = _launch(C, kind, buf, d, *dims, self.ds, self.dtype, self.device, roi=self.roi)
            ev = torch.cuda.Event()
            ev.record(self.copy)
        return x4, gt, d, ev

    def ready(self, handle):
        x4, gt, d, ev = handle
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        x4.record_stream(cur)
        d.record_stream(cur)                  # (gt is a view of d, or with roi a tensor of its own)
        if self.roi:
            gt.record_stream(cur)
        return x4, gt
