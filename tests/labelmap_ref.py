"""CPU restatement of the label-map compositing contract in numpy: what ``orv_amd.labelmap`` must compute, written from the
contract and not from the kernels.  Plain loops over masks and whole-array numpy statements; nothing here knows about groups of 16 pixels,
alignment or byte selects."""
import colorsys

import numpy as np

NUM_COLORS = 60


def palette60():
    """uint8 [60, 3] of (r, g, b): 60 hues at s = 0.75, v = 0.95, each channel int(255 c), the last entry black."""
    pal = [tuple(int(c * 255) for c in colorsys.hsv_to_rgb(i / NUM_COLORS, 0.75, 0.95)) for i in range(NUM_COLORS)]
    pal[-1] = (0, 0, 0)
    return np.array(pal, dtype=np.uint8)


def is_set(masks, threshold=0.0):
    """The threshold rule -> a boolean array of the same shape.  bool as it is; uint8 where nonzero; float32 where x > threshold in IEEE
    terms, decided on the bits: a NaN is never set, and otherwise the sign-magnitude integers of x and the threshold are compared, so a
    denormal is a number like any other and -0 equals +0."""
    masks = np.asarray(masks)
    if masks.dtype == np.bool_:
        return masks.copy()
    if masks.dtype == np.uint8:
        return masks != 0
    assert masks.dtype == np.float32, masks.dtype

    def ordered(x):
        bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
        mag = bits & 0x7FFFFFFF
        return np.where(bits >> 31 == 1, -mag, mag), mag > 0x7F800000

    key, nan = ordered(masks)
    tkey, tnan = ordered(np.float32(threshold).reshape(1))
    if tnan[0]:
        return np.zeros(masks.shape, dtype=np.bool_)
    return ~nan & (key > tkey[0])


def stats(masks, threshold=0.0):
    """masks [F,n,H,W] -> (area int64 [F,n], xyxy int64 [F,n,4]): the count of set pixels, and x_min, y_min, x_max, y_max inclusive over the
    set pixels, zeros for an empty mask."""
    on = is_set(masks, threshold)
    F, n = on.shape[:2]
    area, xyxy = np.zeros((F, n), np.int64), np.zeros((F, n, 4), np.int64)
    for f in range(F):
        for j in range(n):
            ys, xs = np.nonzero(on[f, j])
            area[f, j] = len(ys)
            if len(ys):
                xyxy[f, j] = xs.min(), ys.min(), xs.max(), ys.max()
    return area, xyxy


def paint_order(area0):
    """A stable ascending sort of the areas, flipped: the largest first, and among equal areas the larger mask number first."""
    area0 = np.asarray(area0)
    idx = sorted(range(len(area0)), key=lambda j: (int(area0[j]), j))
    return np.array(idx[::-1], dtype=np.int64)


def compose(masks, label_ids, order=None, threshold=0.0, channel_order="bgr", palette=None):
    """masks [F,n,H,W] -> (index uint8 [F,H,W], color uint8 [F,H,W,3], order int64 [m]).  The order defaults to paint_order of the first
    frame's areas and holds for every frame; a pixel painted with id 255 keeps the colour of palette[255 % 60]."""
    on = is_set(masks, threshold)
    F, n, H, W = on.shape
    label_ids = np.asarray(label_ids).astype(np.int64)
    assert label_ids.shape == (n,)
    palette = palette60() if palette is None else np.asarray(palette)
    if order is None:
        order = paint_order(stats(masks[:1], threshold)[0][0]) if n else np.zeros(0, np.int64)
    order = np.asarray(order, dtype=np.int64)
    index = np.full((F, H, W), 255, dtype=np.uint8)
    color = np.zeros((F, H, W, 3), dtype=np.uint8)
    for f in range(F):
        for j in order:
            rgb = palette[label_ids[j] % NUM_COLORS]
            index[f][on[f, j]] = label_ids[j]
            color[f][on[f, j]] = rgb[::-1] if channel_order == "bgr" else rgb
    return index, color, order


def load_fixture(path):
    """A fixture of tests/golden/labelmap/ -> dict with ``masks`` unpacked to bool [F,n,H,W]."""
    with np.load(path) as z:
        fx = {k: z[k] for k in z.files}
    shape = tuple(int(v) for v in fx["shape"])
    fx["masks"] = np.unpackbits(fx["masks_packed"], count=int(np.prod(shape))).astype(np.bool_).reshape(shape)
    return fx
