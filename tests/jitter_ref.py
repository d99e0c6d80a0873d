"""Float64 numpy restatement of torchvision's ColorJitter on a float image in [0, 1] (its tensor implementation,
torchvision/transforms/_functional_tensor.py: _blend, rgb_to_grayscale, _rgb2hsv, _hsv2rgb), for the device ColorJitter of
geomapnet_amd (csrc/jitter.h).  Images are [..., H, W, 3] (NHWC, as the uint8 input path takes them)."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


def _blend(img1, img2, ratio):
    return np.clip(ratio * img1 + (1.0 - ratio) * img2, 0.0, 1.0)


def gray(img):
    return 0.2989 * img[..., 0] + 0.587 * img[..., 1] + 0.114 * img[..., 2]


def rgb2hsv(img):
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    maxc = img.max(axis=-1)
    minc = img.min(axis=-1)
    eqc = maxc == minc
    cr = maxc - minc
    ones = np.ones_like(maxc)
    s = cr / np.where(eqc, ones, maxc)
    crd = np.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = np.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    return np.stack((h, s, maxc), axis=-1)


def hsv2rgb(img):
    h, s, v = img[..., 0], img[..., 1], img[..., 2]
    i = np.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.astype(np.int64) % 6
    p = np.clip(v * (1.0 - s), 0.0, 1.0)
    q = np.clip(v * (1.0 - s * f), 0.0, 1.0)
    t = np.clip(v * (1.0 - s * (1.0 - f)), 0.0, 1.0)
    a1 = np.stack((v, q, p, p, t, v), axis=-1)
    a2 = np.stack((t, v, v, q, p, p), axis=-1)
    a3 = np.stack((p, p, t, v, v, q), axis=-1)
    sel = i[..., None]
    return np.stack([np.take_along_axis(a, sel, axis=-1)[..., 0] for a in (a1, a2, a3)], axis=-1)


def adjust_brightness(img, f):
    return _blend(img, np.zeros_like(img), f)


def adjust_contrast(img, f):
    return _blend(img, gray(img).mean(), f)


def adjust_saturation(img, f):
    return _blend(img, gray(img)[..., None], f)


def adjust_hue(img, f):
    hsv = rgb2hsv(img)
    hsv[..., 0] = np.mod(hsv[..., 0] + f, 1.0)
    return hsv2rgb(hsv)


_OPS = {BRIGHTNESS: adjust_brightness, CONTRAST: adjust_contrast, SATURATION: adjust_saturation, HUE: adjust_hue}


def jitter(img, factors, order, active=(True, True, True, True)):
    """one image [H, W, 3] in [0, 1]; factors (b, c, s, h); order: the four op ids; an inactive op is skipped"""
    x = np.asarray(img, dtype=np.float64)
    for op in order:
        op = int(op)
        if active[op]:
            x = _OPS[op](x, float(factors[op]))
    return x


def jitter_u8_normalised(u8, draws, mean, std, active=(True, True, True, True)):
    """uint8 images [N, H, W, 3] and the device's draws [N, 8] -> ToTensor, ColorJitter, Normalize as [N, H, W, 3] float64"""
    u8 = np.asarray(u8)
    draws = np.asarray(draws, dtype=np.float64)
    out = np.empty(u8.shape, dtype=np.float64)
    for n in range(u8.shape[0]):
        x = jitter(u8[n].astype(np.float64) / 255.0, draws[n, :4], draws[n, 4:].astype(np.int64), active)
        out[n] = (x - np.asarray(mean)) / np.asarray(std)
    return out
