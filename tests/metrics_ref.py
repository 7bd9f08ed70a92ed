"""float64 numpy restatement of the reference's frame scoring (utils/metrics.py:11-70 as tools/test_reds4.py:205-218 calls it), for
frames too large for a fixture.  Plain module: numpy only.  tests/test_metrics_ref.py holds it to the values the reference's own
functions returned (tests/golden/metrics_frames.npz).

The window is applied as ONE two-dimensional correlation with the 11 x 11 outer product, 121 shifted slices added up -- the
reference's cv2.filter2D call, and not the separable column / row passes of csrc/metrics.hip."""
import math

import numpy as np

C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2


def gaussian_kernel(ksize=11, sigma=1.5):
    """cv2.getGaussianKernel(ksize, sigma) for ksize > 7: a (ksize, 1) float64 column, exp(-x^2 / (2 sigma^2)) times the reciprocal of the sum."""
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    t = np.exp((-0.5 / (sigma * sigma)) * x * x)
    return (t * (1.0 / t.sum())).reshape(ksize, 1)


def filter2d(img, window):
    """cv2.filter2D(img, -1, window) for float64 input: a correlation anchored at the window's centre, output of the input's size.  The
    border rows / columns (cv2 reflects there) are left as zeros: every caller crops [5:-5, 5:-5]."""
    kh, kw = window.shape
    h, w = img.shape
    out = np.zeros((h, w), dtype=np.float64)
    if h < kh or w < kw:
        return out
    acc = np.zeros((h - kh + 1, w - kw + 1), dtype=np.float64)
    tmp = np.empty_like(acc)
    for i in range(kh):
        for j in range(kw):
            np.multiply(img[i:i + acc.shape[0], j:j + acc.shape[1]], window[i, j], out=tmp)
            acc += tmp
    out[kh // 2:kh // 2 + acc.shape[0], kw // 2:kw // 2 + acc.shape[1]] = acc
    return out


def rgb_to_y(img):
    """skimage.color.rgb2ycbcr(uint8 RGB)[..., 0]: float64, not rounded."""
    f = img.astype(np.float64)
    return 16.0 + (65.481 * f[..., 0] + 128.553 * f[..., 1] + 24.966 * f[..., 2]) / 255.0


def psnr(img1, img2, border=0):
    h, w = img1.shape[:2]
    a = img1[border:h - border, border:w - border].astype(np.float64)
    b = img2[border:h - border, border:w - border].astype(np.float64)
    mse = np.mean((a - b) ** 2)
    if mse == 0:
        return float("inf")
    return 20 * math.log10(255.0 / math.sqrt(mse))


def ssim(img1, img2):
    if img1.ndim == 3:
        return float(np.array([ssim(img1[..., i], img2[..., i]) for i in range(img1.shape[2])]).mean())
    a, b = img1.astype(np.float64), img2.astype(np.float64)
    k = gaussian_kernel(11, 1.5)
    window = np.outer(k, k.transpose())
    mu1 = filter2d(a, window)[5:-5, 5:-5]
    mu2 = filter2d(b, window)[5:-5, 5:-5]
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    sigma1_sq = filter2d(a ** 2, window)[5:-5, 5:-5] - mu1_sq
    sigma2_sq = filter2d(b ** 2, window)[5:-5, 5:-5] - mu2_sq
    sigma12 = filter2d(a * b, window)[5:-5, 5:-5] - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return float(ssim_map.mean())


def frame_scores(out, gt, border=0):
    """(psnr, psnr_y, ssim, ssim_y) of two (H, W, 3) uint8 frames, both cut by `border` on every side first."""
    h, w = out.shape[:2]
    out, gt = out[border:h - border, border:w - border], gt[border:h - border, border:w - border]
    oy, gy = rgb_to_y(out), rgb_to_y(gt)
    return psnr(out, gt), psnr(oy, gy), ssim(out, gt), ssim(oy, gy)
