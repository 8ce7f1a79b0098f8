#!/usr/bin/env python
"""Write an ROI mask ground_truth/NAME.roi.npy (uint8, 255 inside) for every image of a dataset root made by
scripts/make_jpeg_set.py: an ellipse about the image centre covering about 60 % of it, as TRANCOS-style masks do.

usage: python profiles/r20/make_roi_masks.py ROOT
"""
import os
import sys

import numpy as np
from PIL import Image

root = sys.argv[1]
n = 0
for part in ("train_data", "test_data"):
    idir, gdir = os.path.join(root, part, "images"), os.path.join(root, part, "ground_truth")
    for f in sorted(os.listdir(idir)):
        with Image.open(os.path.join(idir, f)) as im:
            w, h = im.size
        y, x = np.mgrid[0:h, 0:w]
        inside = ((y - h / 2) / (0.44 * h)) ** 2 + ((x - w / 2) / (0.44 * w)) ** 2 <= 1.0
        np.save(os.path.join(gdir, os.path.splitext(f)[0] + ".roi.npy"), inside.astype(np.uint8) * 255)
        n += 1
print("masks written:", n)
