"""Numpy restatement of the multiscale resize rule (csrc/preproc.hip ``ep24_resize_bilinear_f32`` /
``ep24_scale_labels``): source coordinates in float64, the blend in float32 with every operation rounded on its own.

Per axis with ``n_in`` source and ``n_out`` output positions:  s = n_in / n_out;  src = max(s * (d + 0.5) - 0.5, 0);
i0 = min(int(src), n_in - 1);  i1 = min(i0 + 1, n_in - 1);  w1 = float32(src - i0);  w0 = 1 - w1  (float32).
Then  top = a * wx0 + b * wx1,  bot = c * wx0 + d * wx1,  out = top * wy0 + bot * wy1  (a, b from row y0; c, d from row y1).
"""
import numpy as np

# (source (H, W), output (oh, ow)): up, down, identity, tails (one column; a tiny source; odd sizes with ow % 4 == 3), further down
SHAPES = [((64, 96), (96, 128)), ((96, 128), (64, 96)), ((64, 96), (64, 96)), ((32, 32), (35, 1)), ((5, 7), (64, 96)),
          ((96, 64), (33, 131)), ((160, 160), (128, 128))]


def axis(n_in, n_out):
    """-> (i0, i1 int64, w0, w1 float32), each of length n_out."""
    s = np.float64(n_in) / np.float64(n_out)
    d = np.arange(n_out, dtype=np.float64)
    src = np.maximum(s * (d + 0.5) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = (src - i0.astype(np.float64)).astype(np.float32)
    w0 = np.float32(1.0) - w1
    return i0, i1, w0, w1


def resize(x, oh, ow):
    """x [..., H, W] float32 -> [..., oh, ow] float32."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    y0, y1, wy0, wy1 = axis(x.shape[-2], oh)
    x0, x1, wx0, wx1 = axis(x.shape[-1], ow)
    r0, r1 = x[..., y0, :], x[..., y1, :]
    top = r0[..., x0] * wx0 + r0[..., x1] * wx1          # float32 arrays: every numpy operation rounds to float32
    bot = r1[..., x0] * wx0 + r1[..., x1] * wx1
    out = top * wy0[:, None] + bot * wy1[:, None]
    assert out.dtype == np.float32
    return out


def resize_f64(x, oh, ow):
    """The same formula with every value and operation in float64: what the rounding of ``resize`` is measured against."""
    x = np.asarray(x, dtype=np.float64)
    ys = np.maximum(np.float64(x.shape[-2]) / oh * (np.arange(oh) + 0.5) - 0.5, 0.0)
    xs = np.maximum(np.float64(x.shape[-1]) / ow * (np.arange(ow) + 0.5) - 0.5, 0.0)
    y0 = np.minimum(ys.astype(np.int64), x.shape[-2] - 1)
    x0 = np.minimum(xs.astype(np.int64), x.shape[-1] - 1)
    y1, x1 = np.minimum(y0 + 1, x.shape[-2] - 1), np.minimum(x0 + 1, x.shape[-1] - 1)
    wy1, wx1 = (ys - y0)[:, None], xs - x0
    r0, r1 = x[..., y0, :], x[..., y1, :]
    top = r0[..., x0] * (1 - wx1) + r0[..., x1] * wx1
    bot = r1[..., x0] * (1 - wx1) + r1[..., x1] * wx1
    return top * (1 - wy1) + bot * wy1


def scale_labels(labels, scale_x, scale_y):
    """labels [..., 51] float32: column 0 copied, odd columns * float32(scale_x), even columns >= 2 * float32(scale_y)."""
    labels = np.asarray(labels)
    assert labels.dtype == np.float32 and labels.shape[-1] == 51
    out = labels.copy()
    out[..., 1::2] = labels[..., 1::2] * np.float32(scale_x)
    out[..., 2::2] = labels[..., 2::2] * np.float32(scale_y)
    return out
