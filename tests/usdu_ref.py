"""NumPy restatement of the 8-bit image ops behind UltimateSDUpscale (lightdiffusion_amd/csrc/image.hip) and of the two conversions:
what Pillow computes for `Image.resize(LANCZOS / BICUBIC)`, `ImageFilter.GaussianBlur` on an "L" image and the paste / putalpha /
alpha_composite chain of the reference's `process_images`, in integer arithmetic, byte for byte (tests/test_usdu_cpu.py checks that
against Pillow where it imports and against tests/golden/usdu_ops.npz always).  It is the test-side reference on machines without Pillow.
"""
import math

import numpy as np

PRECISION_BITS = 22


def _lanczos(x):
    if not -3.0 <= x < 3.0:
        return 0.0
    sinc = lambda v: 1.0 if v == 0.0 else math.sin(math.pi * v) / (math.pi * v)
    return sinc(x) * sinc(x / 3.0)


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {"lanczos": (_lanczos, 3.0), "bicubic": (_bicubic, 2.0)}


def resample_coeffs(in_size, out_size, filt="lanczos"):
    """Per output sample: (first input sample, tap count, fixed-point taps) of one axis."""
    f, support = FILTERS[filt]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    sup = support * fs
    ksize = int(math.ceil(sup)) * 2 + 1
    xmin = np.zeros(out_size, np.int32)
    cnt = np.zeros(out_size, np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - sup + 0.5), 0)
        hi = min(int(center + sup + 0.5), in_size)
        k = [f((j + lo - center + 0.5) / fs) for j in range(hi - lo)]
        ww = sum(k)
        if ww != 0.0:
            k = [v / ww for v in k]
        xmin[xx], cnt[xx] = lo, hi - lo
        for j, v in enumerate(k):
            kk[xx, j] = int(0.5 + v * (1 << PRECISION_BITS)) if v >= 0 else int(-0.5 + v * (1 << PRECISION_BITS))
    return xmin, cnt, kk


def _pass(img, out_size, filt):
    """Resample axis 0 of img [n, ...] to out_size."""
    xmin, cnt, kk = resample_coeffs(img.shape[0], out_size, filt)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    src = img.astype(np.int64)
    for xx in range(out_size):
        acc = np.tensordot(kk[xx, :cnt[xx]].astype(np.int64), src[xmin[xx]:xmin[xx] + cnt[xx]], axes=(0, 0))
        out[xx] = np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
    return out


def resample(img, out_w, out_h, filt="lanczos"):
    """Image.resize((out_w, out_h), filt) of a uint8 image [H, W] or [H, W, C]: horizontal pass, then vertical, uint8 between them;
    a pass whose size does not change is skipped."""
    img = np.asarray(img, np.uint8)
    if img.shape[1] != out_w:
        img = np.moveaxis(_pass(np.moveaxis(img, 1, 0), out_w, filt), 0, 1)
    if img.shape[0] != out_h:
        img = _pass(img, out_h, filt)
    return np.ascontiguousarray(img)


def box_radius(radius):
    """_gaussian_blur_radius(radius, passes=3), in float32 as the C code has it."""
    f = np.float32
    s2 = f(radius) * f(radius) / f(3)
    L = f(np.sqrt(f(12.0) * s2 + f(1.0)))
    l = f(np.floor((L - f(1.0)) / f(2.0)))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * s2)
    a = a / (f(6) * (s2 - (l + f(1)) * (l + f(1))))
    return f(l + a)


def box_weights(radius):
    """(R, ww, fw) of one box pass of GaussianBlur(radius)."""
    fr = box_radius(radius)
    R = int(fr)
    ww = int(np.float32(1 << 24) / (fr * np.float32(2) + np.float32(1)))
    fw = ((1 << 24) - (2 * R + 1) * ww) // 2
    return R, ww, fw


def _box_pass(a, R, ww, fw):
    """One box pass along axis 1 of a [rows, n] uint8 array, edge-replicating."""
    n = a.shape[1]
    src = a.astype(np.int64)
    idx = np.arange(n)
    acc = np.zeros_like(src)
    for d in range(-R, R + 1):
        acc += src[:, np.clip(idx + d, 0, n - 1)]
    edge = src[:, np.clip(idx - R - 1, 0, n - 1)] + src[:, np.clip(idx + R + 1, 0, n - 1)]
    return ((acc * ww + edge * fw + (1 << 23)) >> 24).astype(np.uint8)


def gaussian_blur(mask, radius):
    """ImageFilter.GaussianBlur(radius) of an "L" image [H, W]: three box passes along x, then three along y, uint8 after each."""
    a = np.asarray(mask, np.uint8)
    R, ww, fw = box_weights(radius)
    for _ in range(3):
        a = _box_pass(a, R, ww, fw)
    a = a.T
    for _ in range(3):
        a = _box_pass(a, R, ww, fw)
    return np.ascontiguousarray(a.T)


def blur_reach(radius):
    """How far one axis of GaussianBlur(radius) reads: three passes of R + 1 samples."""
    return 3 * (box_weights(radius)[0] + 1)


def composite(canvas, tile, alpha, x0, y0):
    """canvas[y0:y0+h, x0:x0+w] = div255(tile a + canvas (255 - a)) in place: process_images' paste, putalpha, masked paste,
    alpha_composite and convert("RGB") over an opaque image."""
    h, w = alpha.shape
    a = alpha.astype(np.int64)[..., None]
    v = tile.astype(np.int64) * a + canvas[y0:y0 + h, x0:x0 + w].astype(np.int64) * (255 - a) + 128
    canvas[y0:y0 + h, x0:x0 + w] = ((v + (v >> 8)) >> 8).astype(np.uint8)
    return canvas


def to_u8(x):
    """tensor_to_pil: uint8(clip(255 x, 0, 255)), a truncation in fp32."""
    return np.clip(np.float32(255.0) * np.asarray(x, np.float32), 0, 255).astype(np.uint8)


def to_f32(x):
    """pil_to_tensor: x / 255 as a correctly rounded fp32 division."""
    return np.asarray(x, np.uint8).astype(np.float32) / np.float32(255.0)
