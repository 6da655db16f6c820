"""The numpy restatement of the point-cloud contract of DESIGN.md §17, written from the contract and not from the kernels: brute-force
nearest neighbours under the order (d2, index), the statistical outlier removal, the PCA normals (the eigenvector from ``numpy.linalg.eigh``
in fp64, not the kernels' analytic solver) and the orientation.  One array operation per rounding: numpy contracts nothing into an FMA."""
import numpy as np

# the worst angle (radians) between a normal the kernels stored (fp32) and eigh's fp64 eigenvector, over the points of the test cases whose
# eigen-gap (l1 - l0) / l2 is at least GAP_MIN; measured on an MI355X.  The tests bound the angle by ten times this value,
# the factor covering other seeds; the rounding of the stored normal to fp32 (2^-24 per component) is what it consists of.
MEASURED_ANGLE = 4.3e-8
GAP_MIN = 0.05


def knn(points, k, chunk=512):
    """points fp32 [N,3] -> (idx int32 [N, k'], d2 fp64 [N, k']) with k' = min(k, N): the k' smallest (d2, index), ascending."""
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    N = len(p)
    kk = min(int(k), N)
    idx, d2 = np.zeros((N, kk), np.int32), np.zeros((N, kk), np.float64)
    index = np.arange(N)
    for a in range(0, N, chunk):
        q = p[a:a + chunk]
        dx, dy, dz = p[None, :, 0] - q[:, None, 0], p[None, :, 1] - q[:, None, 1], p[None, :, 2] - q[:, None, 2]
        xx, yy, zz = dx * dx, dy * dy, dz * dz
        d = (xx + yy) + zz
        order = np.lexsort((np.broadcast_to(index, d.shape), d), axis=-1)[:, :kk]
        idx[a:a + chunk] = order
        d2[a:a + chunk] = np.take_along_axis(d, order, axis=1)
    return idx, d2


def outlier(d2, std_ratio):
    """d2 fp64 [N, k'] -> (keep bool [N], avg [N], mean, std, thr, V)."""
    N, kk = d2.shape
    s = np.zeros(N, np.float64)
    for r in range(kk):                                  # rank order
        s = s + np.sqrt(d2[:, r])
    avg = s / np.float64(kk) if kk else s
    valid = avg > 0
    V = int(valid.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.sum(avg[valid]) / np.float64(V)
        dev = avg[valid] - mean
        std = np.sqrt(np.sum(dev * dev) / np.float64(V - 1))
        thr = mean + np.float64(std_ratio) * std
        keep = valid & (avg < thr)
    return keep, avg, mean, std, thr, V


def covariance(points, idx):
    """-> C fp64 [N,3,3]: the centred two-pass covariance of every point's neighbours, mean and sums in rank order."""
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    N, kk = idx.shape
    m = np.zeros((N, 3))
    for r in range(kk):
        m = m + p[idx[:, r]]
    m = m / np.float64(max(kk, 1))
    C = np.zeros((N, 3, 3))
    for r in range(kk):
        d = p[idx[:, r]] - m
        C = C + d[:, :, None] * d[:, None, :]
    return C / np.float64(max(kk, 1))


def orient_sign(points, n, camera):
    """n fp64 [N,3] negated where (n.x v.x + n.y v.y) + n.z v.z < 0 with v = camera - p."""
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    v = np.asarray(camera, np.float64)[None, :] - p
    dot = (n[:, 0] * v[:, 0] + n[:, 1] * v[:, 1]) + n[:, 2] * v[:, 2]
    return np.where((dot < 0)[:, None], -n, n), dot


def normals(points, idx, camera=(0.0, 0.0, 0.0)):
    """-> (n fp64 [N,3] oriented, C [N,3,3], w [N,3] ascending eigenvalues, cos [N] of the angle between n and camera - p)."""
    N, kk = idx.shape
    C = covariance(points, idx)
    w, vec = np.linalg.eigh(C)
    n = vec[:, :, 0].copy()
    flat = (np.abs(C).reshape(N, 9).max(axis=1) == 0) if N else np.zeros(0, bool)
    n[flat] = (0.0, 0.0, 1.0)
    if kk < 3:
        n[:] = (0.0, 0.0, 1.0)
    n, dot = orient_sign(points, n, camera)
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    vlen = np.linalg.norm(np.asarray(camera, np.float64)[None, :] - p, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = np.abs(dot) / vlen
    return n, C, w, cos


def eigen_gap(w):
    """(l1 - l0) / l2 per point; 0 where l2 == 0."""
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (w[:, 1] - w[:, 0]) / w[:, 2]
    return np.where(w[:, 2] > 0, g, 0.0)


def orient(points, normals_, camera=(0.0, 0.0, 0.0)):
    """The standalone orientation with the zero-normal rule, fp64 on the fp32 values, one rounding to fp32 -> fp32 [N,3]."""
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    n = np.asarray(normals_, dtype=np.float32).astype(np.float64)
    v = np.asarray(camera, np.float64)[None, :] - p
    vlen = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    out, _ = orient_sign(points, n, camera)
    zero = (n == 0).all(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = v / vlen[:, None]
    unit[vlen == 0] = (0.0, 0.0, 1.0)
    out[zero] = unit[zero]
    return out.astype(np.float32)


def angle(a, b):
    """The angle between the rows of a and b (fp64), accurate for small angles."""
    cr = np.cross(a, b)
    return np.arctan2(np.linalg.norm(cr, axis=1), (a * b).sum(axis=1))
