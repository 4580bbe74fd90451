"""TEST INFRASTRUCTURE: numpy float64 restatement of the colour stage's definition (include/cudabrot_amd.h, "Colour
image"), written from the header's text, independent of the product's code.  The product's host and device paths
must equal it byte for byte."""

import numpy as np


def levels(v, black_percent, white_percent):
    """Step 1 for one plane of u16 values -> (black, white)."""
    n = v.size
    nb = int(float(n) * (black_percent / 100.0))
    nw = int(float(n) * (white_percent / 100.0))
    hist = np.bincount(v.reshape(-1), minlength=65536).astype(np.int64)
    at_most = np.cumsum(hist)                   # #{v <= k}
    at_least = np.cumsum(hist[::-1])[::-1]      # #{v >= k}
    black = int(np.nonzero(at_most > nb)[0][0])
    white = int(np.nonzero(at_least > nw)[0][-1])
    return black, white


def stretch(v, black, white):
    """Step 2 -> float64 array in [0, 1]."""
    s = np.ones(v.shape, dtype=np.float64)
    if white > black:
        inv = 1.0 / float(white - black)
        mid = (v.astype(np.int64) - black).astype(np.float64) * inv
        s = np.where(v >= white, 1.0, mid)
    return np.where(v <= black, 0.0, s)


def _u16(c):
    return np.floor(c * 65535.0 + 0.5).astype(np.uint16)


def _hsl_channel(p, q, t):
    t = t - np.floor(t)
    rise = p + ((q - p) * 6.0) * t
    fall = p + ((q - p) * 6.0) * (2.0 / 3.0 - t)
    return np.where(t < 1.0 / 6.0, rise, np.where(t < 0.5, q, np.where(t < 2.0 / 3.0, fall, p)))


def compose(grays, mode="rgb", black_percent=2.0, white_percent=1.0, hue_shift=0.0):
    """Three u16 images [h,w] -> (u16 image [h,w,3] in host order, [(black, white)] * 3)."""
    lv = [levels(g, black_percent, white_percent) for g in grays]
    s = [stretch(g, b, w) for g, (b, w) in zip(grays, lv)]
    if mode == "rgb":
        out = [_u16(x) for x in s]
    else:
        h = s[0] + hue_shift
        h = h - np.floor(h)
        S, L = s[1], s[2]
        q = np.where(L < 0.5, L * (1.0 + S), (L + S) - L * S)
        p = 2.0 * L - q
        out = [_u16(np.clip(_hsl_channel(p, q, t), 0.0, 1.0)) for t in (h + 1.0 / 3.0, h, h - 1.0 / 3.0)]
    return np.stack(out, axis=-1), lv


def ppm_bytes(rgb):
    """Step 5: the binary PPM of an image [h,w,3]."""
    h, w, _ = rgb.shape
    return b"P6\n%d %d\n65535\n" % (w, h) + np.ascontiguousarray(rgb, dtype=">u2").tobytes()
