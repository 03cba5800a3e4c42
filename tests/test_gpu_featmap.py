"""The four feature-map kernels (csrc/featmap.hip) against the NumPy oracle written from their contract (tests/featmap_oracle.py)."""
import numpy as np
import pytest
import torch

import featmap_oracle as O
from ep24 import _lib, featmap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
E_ARG, E_UNS = -1, -3
SENT = -12345.5


def _upload_bf16(vals):
    """float32 array of bf16-representable values -> bf16 tensor of the same shape on the device."""
    return torch.from_numpy(O.bf16_bits(vals).copy()).to(DEV).view(BF).reshape(vals.shape)


def _buffer(M, C, ld, off, vals):
    """[M, ld] bf16 on the device: NaN everywhere but the slice [off, off + C), which holds vals [M, C]."""
    full = np.full((M, ld), np.nan, dtype=np.float32)
    full[:, off:off + C] = vals
    return _upload_bf16(full)


def _mean(buf, M, C, ld, off, out=None):
    x = buf.view(1, 1, M, ld)[..., off:off + C]
    return featmap.channel_mean(x, out=out)


# ------------------------------------------------------------------------------------------------ mean
@pytest.mark.parametrize("C,ld,off", [(8, 8, 0), (24, 40, 8), (256, 256, 0), (1024, 2048, 1024)])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 255, 257, 1025])
def test_mean(M, C, ld, off):
    rng = np.random.default_rng(M * 7919 + C)
    ints = rng.integers(-16, 17, (M, C)).astype(np.float32)
    rand = O.bf16_round(rng.normal(0.0, 1.0, (M, C)).astype(np.float32) * np.exp(rng.normal(0.0, 1.0, (M, 1))).astype(np.float32))
    # integer operands: every summation order gives the same fp32 sum, so the result is exact; the row past M keeps its sentinel
    store = torch.full((M + 1,), SENT, dtype=torch.float32, device=DEV)
    buf = _buffer(M, C, ld, off, ints)
    got = _mean(buf, M, C, ld, off, out=store[:M].view(1, 1, M))
    assert got.data_ptr() == store.data_ptr()
    host = store.cpu().numpy()
    assert host[M] == np.float32(SENT)
    want = O.mean_exact(ints)
    assert np.array_equal(host[:M].view(np.uint32), want.view(np.uint32)), (host[:4], want[:4])
    # random operands: the a-priori bound of an fp32 sum in any order plus one division
    bufr = _buffer(M, C, ld, off, rand)
    gotr = _mean(bufr, M, C, ld, off).cpu().numpy().reshape(M)
    err, bound = np.abs(gotr.astype(np.float64) - O.mean_f64(rand)), O.mean_bound(rand)
    print("M=%d C=%d: max err / bound = %.3f" % (M, C, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.isfinite(gotr).all() and (err <= bound).all()
    # the same rows at another M and another row index: identical bits
    k = min(M, 5)
    M2 = M + 7
    moved = rng.normal(0.0, 1.0, (M2, C)).astype(np.float32)
    moved[3:3 + k] = rand[M - k:]
    got2 = _mean(_buffer(M2, C, ld, off, O.bf16_round(moved)), M2, C, ld, off).cpu().numpy().reshape(M2)
    assert np.array_equal(got2[3:3 + k].view(np.uint32), gotr[M - k:].view(np.uint32))


def test_mean_last_row_beyond_4_gib():
    M, ld, C = 70000, 32768, 8                                                   # the last row starts at byte 4 587 454 464
    rng = np.random.default_rng(5)
    ints = rng.integers(-16, 17, (M, C)).astype(np.float32)
    buf = torch.zeros(M, ld, dtype=torch.int16, device=DEV)
    buf[:, :C] = torch.from_numpy(O.bf16_bits(ints).copy()).to(DEV)
    got = featmap.channel_mean(buf.view(BF).view(1, 1, M, ld)[..., :C]).cpu().numpy().reshape(M)
    assert np.array_equal(got.view(np.uint32), O.mean_exact(ints).view(np.uint32))
    assert (M - 1) * ld * 2 > 2 ** 32


def test_mean_on_an_nhwc_batch_and_an_act_like_slice():
    """[B, H, W, C] slices of a wider dense tensor, as the plan's concat buffers hold them."""
    B, H, W, ld = 3, 5, 7, 48
    rng = np.random.default_rng(9)
    full = O.bf16_round(rng.normal(size=(B, H, W, ld)).astype(np.float32))
    t = _upload_bf16(full)
    for off, C in ((0, 48), (8, 16), (32, 16)):
        got = featmap.channel_mean(t[..., off:off + C]).cpu().numpy()
        rows = full[..., off:off + C].reshape(-1, C)
        assert got.shape == (B, H, W)
        assert (np.abs(got.reshape(-1).astype(np.float64) - O.mean_f64(rows)) <= O.mean_bound(rows)).all()


def test_mean_refusals():
    fn = _lib.lib().fn["ep24_featmap_mean_bf16"]
    x = torch.zeros(4, 64, dtype=BF, device=DEV)
    out = torch.full((8,), SENT, dtype=torch.float32, device=DEV)
    s = _lib.stream_ptr()
    call = lambda xp=x.data_ptr(), ld=64, M=4, C=16, op=out.data_ptr(): fn(xp, ld, M, C, op, s)
    assert [call(C=12), call(C=0), call(C=-8), call(C=4), call(C=72), call(ld=60), call(ld=8), call(xp=x.data_ptr() + 2),
            call(xp=x.data_ptr() + 8)] == [E_UNS] * 9
    assert [call(M=-1), call(xp=None), call(op=None)] == [E_ARG] * 3
    assert "featmap_mean_bf16" in _lib.lib().last_error()
    assert call(M=0) == 0 and call(M=0, xp=None, op=None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == np.float32(SENT)).all()                         # nothing was launched
    assert call() == 0
    assert (out.cpu().numpy()[:4] == 0).all() and (out.cpu().numpy()[4:] == np.float32(SENT)).all()
    with pytest.raises(ValueError):
        featmap.channel_mean(x.view(1, 1, 4, 64)[..., 4:20])


# ------------------------------------------------------------------------------------------------ range
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("cells", [1, 63, 257, 25600])
def test_range(cells, N):
    rng = np.random.default_rng(cells + N)
    m = rng.normal(0.0, 3.0, (N, cells)).astype(np.float32)
    for n in range(N):
        m[n, 0] = -50.0 - n                                                      # the extremes sit at the first and the last cell
        m[n, cells - 1] = 60.0 + n if cells > 1 else m[n, 0]
        if cells >= 3:
            m[n, cells // 2] = np.nan
    shape = (N, 1, cells) if cells != 25600 else (N, 160, 160)
    got = featmap.value_range(torch.from_numpy(m).reshape(shape).to(DEV)).cpu().numpy()
    want = O.value_range(m)
    assert np.array_equal(got, want)
    for n in range(N):
        assert got[n, 0] == -50.0 - n and got[n, 1] == (60.0 + n if cells > 1 else -50.0 - n)


def test_range_of_nan_maps_and_refusals():
    m = torch.full((2, 3, 3), float("nan"), device=DEV)
    assert featmap.value_range(m).cpu().tolist() == [[float("inf"), float("-inf")]] * 2
    fn = _lib.lib().fn["ep24_featmap_range"]
    s = _lib.stream_ptr()
    assert [fn(m.data_ptr(), -1, 9, m.data_ptr(), s), fn(m.data_ptr(), 1, -1, m.data_ptr(), s), fn(None, 1, 9, m.data_ptr(), s),
            fn(m.data_ptr(), 1, 9, None, s)] == [E_ARG] * 4
    assert fn(None, 0, 9, None, s) == 0


# ------------------------------------------------------------------------------------------------ render
SPECIAL = np.array([-1.0, 0.0, 0.5, 254.999, 255.0, 300.0, np.nan], dtype=np.float32)


@pytest.mark.parametrize("scale", [1, 3, 8, 32])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (20, 20)])
def test_render(H, W, scale):
    rng = np.random.default_rng(H * 100 + scale)
    N = 2
    maps = rng.normal(0.0, 2.0, (N, H, W)).astype(np.float32)
    if H * W >= 257:
        ramp = np.concatenate([np.arange(256) / 256.0, [1.0]]).astype(np.float32)   # range (0, 1): q = k exactly
        maps[0] = 0.5
        maps[0].reshape(-1)[:257] = ramp
        assert {O.color_index(v, 0.0, 1.0) for v in maps[0].reshape(-1)} == set(range(256))
    if H * W >= 15:
        maps[1, H // 2, W // 2] = np.nan
    HS, WS = H * scale, W * scale
    base = rng.uniform(-20.0, 290.0, (N, 3, HS, WS)).astype(np.float32)
    for n in range(N):
        for ch in range(3):
            flat = base[n, ch].reshape(-1)
            k = min(7, flat.size)
            flat[:k] = np.roll(SPECIAL, -(2 * ch + n))[:k]
    maps_d, base_d = torch.from_numpy(maps).to(DEV), torch.from_numpy(base).to(DEV)
    rng_d = featmap.value_range(maps_d).cpu().numpy()
    want_rng = O.value_range(maps.reshape(N, -1))
    assert np.array_equal(rng_d, want_rng)
    nbytes = N * HS * WS * 3
    rand_lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    for alpha in (0, 1, 128, 255):
        for with_base in (True, False):
            lut = None if alpha in (0, 128) else torch.from_numpy(rand_lut)
            store = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device=DEV)
            got = featmap.render(maps_d, scale, base=base_d if with_base else None, alpha=alpha, lut=lut,
                                 out=store[:nbytes].view(N, HS, WS, 3))
            host = store.cpu().numpy()
            assert got.data_ptr() == store.data_ptr() and (host[nbytes:] == 0xA5).all()
            want = O.render(maps, scale, want_rng, featmap.colormap().numpy() if lut is None else rand_lut,
                            base=base if with_base else None, alpha=alpha)
            bad = int((host[:nbytes].reshape(want.shape) != want).sum())
            assert bad == 0, "alpha %d base %s: %d bytes differ" % (alpha, with_base, bad)
    # explicit limits replace the map's own range
    got = featmap.render(maps_d, scale, vmin=-1.0, vmax=1.5).cpu().numpy()
    assert np.array_equal(got, O.render(maps, scale, np.array([[-1.0, 1.5]] * N, np.float32), featmap.colormap().numpy()))
    got = featmap.render(maps_d, scale, vmax=0.75).cpu().numpy()
    lim = want_rng.copy()
    lim[:, 1] = 0.75
    assert np.array_equal(got, O.render(maps, scale, lim, featmap.colormap().numpy()))


def test_render_refusals():
    fn = _lib.lib().fn["ep24_featmap_render"]
    m = torch.zeros(1, 2, 2, device=DEV)
    r, lut = torch.zeros(1, 2, device=DEV), featmap.colormap().to(DEV)
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device=DEV)
    s = _lib.stream_ptr()
    call = lambda mp=m.data_ptr(), N=1, H=2, W=2, sc=1, rp=r.data_ptr(), lp=lut.data_ptr(), a=128, op=out.data_ptr(): \
        fn(mp, N, H, W, sc, rp, lp, None, a, op, s)
    assert [call(N=-1), call(a=-1), call(a=256), call(mp=None), call(rp=None), call(lp=None), call(op=None)] == [E_ARG] * 7
    assert [call(sc=0), call(sc=65), call(H=0), call(W=0), call(H=16385), call(H=513, sc=32)] == [E_UNS] * 6
    assert call(N=0) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()


# ------------------------------------------------------------------------------------------------ response
def _row(vx, vy, cls=1.0):
    row = np.zeros(51, dtype=np.float32)
    row[0] = cls
    row[1], row[2] = (vx.min() + vx.max()) / 2, (vy.min() + vy.max()) / 2
    row[3::2], row[4::2] = vx, vy
    return row


def _ring(cx, cy, rx, ry=None, star=False):
    a = np.arange(24) * (15.0 * np.pi / 180.0)
    r = np.where(np.arange(24) % 2 == 0, 1.0, 0.35) if star else np.ones(24)
    ry = rx if ry is None else ry
    return _row((cx + rx * r * np.cos(a)).astype(np.float32), (cy + ry * r * np.sin(a)).astype(np.float32))


def _scene_rows(H, W, s):
    """The rows every scene holds (input extent Ew x Eh = W * s x H * s)."""
    Ew, Eh = float(W * s), float(H * s)
    E = min(Ew, Eh)
    jc, ic = (W // 2 + 0.5) * s, (H // 2 + 0.5) * s                             # a cell centre
    on_line = _ring(jc, ic, 0.3 * E)                                             # vertices 0 and 12 lie exactly on a cell-centre row
    assert on_line[4] == np.float32(ic) and on_line[4 + 24] == np.float32(ic)
    thin = _ring(jc, 0.5 * Eh, 0.2 * s, 0.3 * Eh)                                # inside one column of cells: the rect has x0 == x1
    assert int(np.float32(thin[3::2].min()) / np.float32(s)) == int(np.float32(thin[3::2].max()) / np.float32(s))
    return [np.zeros(51, dtype=np.float32),                                      # padding
            _ring(0.5 * Ew, 0.5 * Eh, 0.35 * E),                                 # well inside: more than one cell
            _ring(-2.0 * Ew, 0.5 * Eh, 0.3 * E),                                 # fully outside
            _ring(0.05 * Ew, 0.9 * Eh, 0.4 * E),                                 # partly outside: the clamp
            on_line,
            _ring(0.55 * Ew, 0.45 * Eh, 0.45 * E, star=True),
            thin]


@pytest.mark.parametrize("L", [1, 50])
@pytest.mark.parametrize("stride", [8, 32])
@pytest.mark.parametrize("H,W", [(4, 4), (12, 20), (20, 20), (80, 80)])
def test_response(H, W, stride, L):
    rows = _scene_rows(H, W, stride)
    if L == 1:
        labels = np.stack(rows)[:, None, :]                                      # one row per image
    else:
        labels = np.zeros((2, L, 51), dtype=np.float32)
        labels[0, [0, 3, 4, 9, 17, 30, 49]] = np.stack(rows)
        labels[1, [49, 20, 11, 10, 2, 1, 0]] = np.stack(rows)
    B = labels.shape[0]
    rng = np.random.default_rng(H * 1000 + stride + L)
    ints = rng.integers(-8, 9, (B, H, W)).astype(np.float32)
    real = rng.normal(0.5, 2.0, (B, H, W)).astype(np.float32)
    lab_d = torch.from_numpy(labels).to(DEV)
    for mode in ("rect", "poly24"):
        wi = O.response(ints, stride, labels, mode)
        wr = O.response(real, stride, labels, mode)
        # a scene cannot pass by being empty: among the non-padding rows one region is empty and one holds more than one cell
        nonpad = labels.reshape(-1, 51).sum(1) != 0
        cnt = wi[1].reshape(-1)
        assert (cnt[nonpad] == 0).any() and (cnt > 1).any(), (mode, cnt[nonpad])
        gi = featmap.response([torch.from_numpy(ints).to(DEV)], lab_d, strides=(stride,), region=mode)
        gr = featmap.response(torch.from_numpy(real).to(DEV), lab_d, strides=(stride,), region=mode)
        assert tuple(gi.mean.shape) == (1, B, L) and gi.count.dtype == torch.int32 and gi.sum.dtype == torch.float64
        for got, (tot, count, mean, mag), exact in ((gi, wi, True), (gr, wr, False)):
            c, s, m = got.count[0].cpu().numpy(), got.sum[0].cpu().numpy(), got.mean[0].cpu().numpy()
            assert np.array_equal(c, count), (mode, c.reshape(-1)[nonpad], count.reshape(-1)[nonpad])
            if exact:
                assert np.array_equal(s, tot)
            else:
                assert (np.abs(s - tot) <= 1.001 * count * 2.0 ** -53 * mag).all()
            with np.errstate(all="ignore"):
                assert np.array_equal(m, np.where(c > 0, s / np.maximum(c, 1), 0.0))
    if L == 50:                                                                   # rect and poly24 differ somewhere: the modes are not one rule
        assert not np.array_equal(O.response(ints, stride, labels, "rect")[1], O.response(ints, stride, labels, "poly24")[1])


def test_response_unusable_rows_and_refusals():
    H = W = 20
    good = _ring(80.0, 80.0, 40.0)
    rows = [good.copy() for _ in range(5)]
    rows[1][7] = np.nan
    rows[2][8] = np.inf
    rows[3][9] = 2.0 ** 20
    rows[4][:] = -np.abs(rows[4])                                                # the 51 values do not sum to more than 0: padding
    labels = np.stack(rows)[None]
    maps = np.ones((1, H, W), dtype=np.float32)
    for mode in ("rect", "poly24"):
        got = featmap.response([torch.from_numpy(maps).to(DEV)], torch.from_numpy(labels).to(DEV), strides=(8,), region=mode)
        want = O.response(maps, 8, labels, mode)
        assert np.array_equal(got.count[0].cpu().numpy(), want[1]) and want[1][0, 0] > 1 and not want[1][0, 1:].any()
        assert np.array_equal(got.mean[0].cpu().numpy(), want[2]) and np.array_equal(got.sum[0].cpu().numpy(), want[0])
    fn = _lib.lib().fn["ep24_featmap_response"]
    m, lab = torch.zeros(1, 4, 4, device=DEV), torch.zeros(1, 1, 51, device=DEV)
    sm, ct = torch.zeros(2, dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    s = _lib.stream_ptr()
    call = lambda mp=m.data_ptr(), B=1, H=4, W=4, st=8, lp=lab.data_ptr(), L=1, mode=0, sp=sm.data_ptr(), cp=ct.data_ptr(), \
        qp=sm.data_ptr() + 8: fn(mp, B, H, W, st, lp, L, mode, sp, cp, qp, s)
    assert [call(B=-1), call(L=-1), call(st=0), call(mode=2), call(mp=None), call(lp=None), call(sp=None), call(cp=None),
            call(qp=None)] == [E_ARG] * 9
    assert [call(H=0), call(W=16385)] == [E_UNS] * 2
    assert call(B=0) == 0 and call(L=0) == 0 and call() == 0
