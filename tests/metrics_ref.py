"""CPU restatement of the video metrics (``orv_amd.metrics``, include/orv_mi355.h ``orv_frame_metrics``), written from the arithmetic contract
in DESIGN.md §16 and not from the kernel: one numpy array operation per rounding, so with ``dtype=np.float32`` every product, sum and
division is rounded to fp32 on its own, in the order the contract fixes.  ``dtype=np.float64`` evaluates the same formula in fp64 (the
sample coordinate is then not rounded to fp32 either).  ``ssim_scipy64`` is skimage's formula over ``scipy.ndimage.uniform_filter``, the
filter skimage itself calls: what ties the contract's SSIM to something outside this repository."""
import numpy as np

KINDS = ("noise", "smooth", "flat")
# |fp32 contract - fp64 formula| per frame, the largest that tests/test_metrics_host.py measures at its own fixtures: a 320 x 480 pair
# (seed 7) and the frames of real_clip(), all to 256 x 320.  The tests allow twice these.  A property of the formula in fp32 (the
# variances are differences of nearly equal box means; the flat case has variances near 1e-5), not of the kernel.
MEASURED_GAP = {"noise": dict(ssim=2.5e-8, psnr=5.0e-8), "smooth": dict(ssim=7.0e-8, psnr=5.0e-8), "flat": dict(ssim=2.2e-5, psnr=2.2e-5)}


def fixture(kind, shape, seed):
    """[h, w, 3] fp32 image pairs, values rounded to k / 255 so that near-equal images occur: uniform noise, a smooth pattern plus noise,
    a constant plus +-1/255 noise.  -> (a, b)."""
    g = np.random.default_rng(seed)
    h, w = shape
    if kind == "noise":
        a, b = g.uniform(0, 1, (h, w, 3)), g.uniform(0, 1, (h, w, 3))
    elif kind == "smooth":
        y, x = np.mgrid[0:h, 0:w]
        base = 0.5 + 0.4 * np.sin(y / 9.0)[..., None] * np.cos(x[..., None] / 13.0 + np.arange(3))
        a, b = base + g.normal(0, 0.02, (h, w, 3)), base + g.normal(0, 0.02, (h, w, 3))
    elif kind == "flat":
        a = 0.5 + g.integers(-1, 2, (h, w, 3)) / 255.0
        b = 0.5 + g.integers(-1, 2, (h, w, 3)) / 255.0
    else:
        raise ValueError(kind)
    q = lambda v: (np.round(np.clip(v, 0, 1) * 255) / 255).astype(np.float32)
    return q(a), q(b)


def real_clip(n=17):
    """The reference's geometry: a prediction of n frames 320 x 480 and a ground truth 256 x 320 (compared at 256 x 320); frame i is of
    kind KINDS[i % 3].  -> (pred [n, 320, 480, 3], gt [n, 256, 320, 3]) fp32."""
    pred = np.stack([fixture(KINDS[i % 3], (320, 480), seed=i)[0] for i in range(n)])
    gt = np.stack([fixture(KINDS[i % 3], (256, 320), seed=100 + i)[1] for i in range(n)])
    return pred, gt


def resize_taps(n, o, dtype=np.float32):
    """-> (s, s1, w): first tap, second tap and the weight of the second tap for every output index."""
    scale = np.float64(1.0) / (np.float64(o) / np.float64(n))
    f = ((np.arange(o, dtype=np.float64) + 0.5) * scale - 0.5).astype(dtype)
    fl = np.floor(f)
    s = fl.astype(np.int64)
    w = (f - fl).astype(dtype)
    low, high = s < 0, s >= n - 1
    s = np.where(low, 0, np.where(high, n - 1, s))
    w = np.where(low | high, dtype(0), w).astype(dtype)
    return s, np.minimum(s + 1, n - 1), w


def to_float(x, dtype=np.float32):
    """The source value: fp32 as it is, uint8 divided by 255."""
    if x.dtype == np.uint8:
        return x.astype(dtype) / dtype(255.0)
    return x.astype(dtype)


def resize_ref(x, size, dtype=np.float32):
    """x [..., H, W, C] -> [..., h, w, C]: horizontal pass first, then vertical, every product and sum rounded on its own."""
    x = to_float(x, dtype)
    h, w = size
    sy, sy1, wy = resize_taps(x.shape[-3], h, dtype)
    sx, sx1, wx = resize_taps(x.shape[-2], w, dtype)
    wx = wx[:, None]
    r = x[..., :, sx, :] * (dtype(1.0) - wx) + x[..., :, sx1, :] * wx
    wy = wy[:, None, None]
    return (r[..., sy, :, :] * (dtype(1.0) - wy) + r[..., sy1, :, :] * wy).astype(dtype)


def _box(x, dtype):
    """7 x 7 box mean over axes (-3, -2) of [..., h, w, C], valid windows only: seven terms left to right, seven sums top to bottom, / 49."""
    h, w = x.shape[-3], x.shape[-2]
    hs = x[..., :, 0:w - 6, :]
    for k in range(1, 7):
        hs = hs + x[..., :, k:w - 6 + k, :]
    vs = hs[..., 0:h - 6, :, :]
    for k in range(1, 7):
        vs = vs + hs[..., k:h - 6 + k, :, :]
    return (vs / dtype(49.0)).astype(dtype)


def ssim_map_ref(a, b, data_range=1.0, dtype=np.float32):
    """a, b [..., h, w, C] in ``dtype`` -> S [..., h - 6, w - 6, C]."""
    a, b = a.astype(dtype), b.astype(dtype)
    cn = dtype(49.0 / 48.0)
    c1, c2 = dtype((0.01 * data_range) * (0.01 * data_range)), dtype((0.03 * data_range) * (0.03 * data_range))
    ux, uy, uxx, uyy, uxy = _box(a, dtype), _box(b, dtype), _box(a * a, dtype), _box(b * b, dtype), _box(a * b, dtype)
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    a1, a2 = dtype(2.0) * ux * uy + c1, dtype(2.0) * vxy + c2
    b1, b2 = ux * ux + uy * uy + c1, vx + vy + c2
    return ((a1 * a2) / (b1 * b2)).astype(dtype)


def frame_metrics_ref(pred, gt, size, data_range=1.0, dtype=np.float32):
    """pred [N, H, W, 3], gt [N, H', W', 3] (uint8 or fp32) -> dict(mse [N], psnr [N], ssim [N] in fp64, ssim_map [N, h - 6, w - 6, 3])."""
    a, b = resize_ref(pred, size, dtype), resize_ref(gt, size, dtype)
    d = a - b
    sse = (d * d).astype(np.float64).sum(axis=(1, 2, 3))
    mse = sse / (3.0 * size[0] * size[1])
    with np.errstate(divide="ignore"):
        psnr = np.where(mse == 0, np.inf, 10.0 * np.log10((data_range * data_range) / np.where(mse == 0, 1.0, mse)))
    S = ssim_map_ref(a, b, data_range, dtype)
    m = S.astype(np.float64).sum(axis=(1, 2)) / float((size[0] - 6) * (size[1] - 6))          # [N, 3] channel means
    ssim = ((m[:, 0] + m[:, 1]) + m[:, 2]) / 3.0
    return dict(mse=mse, psnr=psnr, ssim=ssim, ssim_map=S)


def ssim_scipy64(a, b, data_range=1.0):
    """skimage's ``structural_similarity`` formula (win_size 7, uniform window, sample covariance) on ``uniform_filter`` in fp64, per
    channel, cropped by 3: a, b [h, w, C] -> S [h - 6, w - 6, C]."""
    from scipy.ndimage import uniform_filter
    a, b = a.astype(np.float64), b.astype(np.float64)
    cov_norm = 49.0 / 48.0
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    out = []
    for c in range(a.shape[-1]):
        x, y = a[..., c], b[..., c]
        ux, uy = uniform_filter(x, size=7), uniform_filter(y, size=7)
        uxx, uyy, uxy = uniform_filter(x * x, size=7), uniform_filter(y * y, size=7), uniform_filter(x * y, size=7)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        out.append(S[3:-3, 3:-3])
    return np.stack(out, axis=-1)
