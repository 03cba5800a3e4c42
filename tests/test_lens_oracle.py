"""The lens model's numpy restatement (tests/lens_oracle.py) against the properties of its contract (include/ep24.h)."""
import math

import numpy as np

import lens_oracle as L

K = (-0.02, 0.004, -0.001, 0.0002)
PIN, FISH = (60.0, 60.0, 63.5, 47.5), (52.0, 52.0, 47.5, 39.5)          # a 96 x 128 pinhole frame, an 80 x 96 fisheye frame


def test_round_trip_is_the_identity_inside_the_field():
    """to_pinhole(to_fisheye(p)) = p to 1e-9 px for points inside the field, and the other way round."""
    m = L.model(PIN, FISH, K, 170.0)
    rng = np.random.RandomState(0)
    rmax = 0.98 * math.tan(m["theta_max"])
    r, phi = rng.uniform(0, min(rmax, 4.0), 20000), rng.uniform(0, 2 * np.pi, 20000)
    u, v = PIN[2] + PIN[0] * r * np.cos(phi), PIN[3] + PIN[1] * r * np.sin(phi)
    X, Y, rim = L.to_fisheye(u, v, m)
    assert (rim > 0).all()
    u2, v2, rim2 = L.to_pinhole(X, Y, m)
    assert (rim2 > 0).all()
    err = max(np.abs(u2 - u).max(), np.abs(v2 - v).max())
    print("pinhole -> fisheye -> pinhole: %.3g px" % err)
    assert err <= 1e-9
    rd = rng.uniform(0, 0.999 * L.thetad(m["theta_max"], K), 20000)
    rd = rd[np.tan(L.invert(rd, m)) < 4.0]                               # the pinhole frame stretches without bound towards 90 degrees
    phi = phi[:len(rd)]
    X, Y = FISH[2] + FISH[0] * rd * np.cos(phi), FISH[3] + FISH[1] * rd * np.sin(phi)
    u, v, _ = L.to_pinhole(X, Y, m)
    X2, Y2, _ = L.to_fisheye(u, v, m)
    err = max(np.abs(X2 - X).max(), np.abs(Y2 - Y).max())
    print("fisheye -> pinhole -> fisheye: %.3g px" % err)
    assert err <= 1e-9


def test_equidistant_in_closed_form():
    """k = 0: the distorted radius is f * theta."""
    m = L.model(PIN, (52.0, 52.0, 47.5, 39.5), (0, 0, 0, 0), 170.0)
    th = np.linspace(0.0, 0.99 * m["theta_max"], 500)
    for phi in (0.0, 0.7, 2.9):
        u, v = PIN[2] + PIN[0] * np.tan(th) * math.cos(phi), PIN[3] + PIN[1] * np.tan(th) * math.sin(phi)
        X, Y, _ = L.to_fisheye(u, v, m)
        assert np.abs(np.hypot(X - 47.5, Y - 39.5) - 52.0 * th).max() <= 1e-10
        u2, v2, _ = L.to_pinhole(47.5 + 52.0 * th * math.cos(phi), 39.5 + 52.0 * th * math.sin(phi), m)
        assert np.abs(np.hypot(u2 - PIN[2], v2 - PIN[3]) - 60.0 * np.tan(th)).max() <= 1e-9 * (1 + 60.0 * np.tan(th)).max()


def test_beyond_the_field_lands_on_the_rim_and_is_finite():
    m = L.model(PIN, FISH, K, 120.0)
    tdm = L.thetad(m["theta_max"], K)
    u = np.array([1e6, 63.5 - 1e9, 63.5, 63.5 + 60.0 * 50])
    v = np.array([47.5, 47.5 + 1e9, 47.5, 47.5])
    X, Y, rim = L.to_fisheye(u, v, m)
    assert np.isfinite(X).all() and np.isfinite(Y).all()
    rd = np.hypot((X - FISH[2]) / FISH[0], (Y - FISH[3]) / FISH[1])
    assert np.abs(rd[[0, 1, 3]] - tdm).max() <= 1e-12 and rd[2] == 0 and (rim[[0, 1, 3]] < 0).all()
    assert abs(Y[0] - FISH[3]) <= 1e-9 and abs((X[1] - FISH[2]) + (Y[1] - FISH[3])) <= 1e-9          # the azimuth is kept
    u2, v2, rim2 = L.to_pinhole(np.array([1e7, 47.5]), np.array([39.5, 39.5]), m)
    assert np.isfinite(u2).all() and rim2[0] < 0
    assert abs((u2[0] - PIN[2]) / PIN[0] - math.tan(m["theta_max"])) <= 1e-9 and u2[1] == PIN[2] and v2[1] == PIN[3]


def test_image_oracle_counts_of_the_reference_geometry():
    """96 x 128 -> 80 x 96 with the intrinsics above: distort samples 68 % of the pixels, undistort everything; no pixel within
    1e-9 px of a decision."""
    m = L.model(PIN, FISH, K, 170.0)
    src = np.random.RandomState(1).randint(0, 256, (96, 128, 3)).astype(np.uint8)
    out, sampled, margin = L.warp_image(src, m, "distort", 80, 96)
    assert abs(sampled.mean() - 0.68) < 0.01 and (margin > 1e-9).all()
    assert (out[~sampled] == 114).all()
    src_f = np.random.RandomState(2).randint(0, 256, (80, 96, 3)).astype(np.uint8)
    out, sampled, margin = L.warp_image(src_f, m, "undistort", 96, 128)
    assert sampled.all() and (margin > 1e-9).all()
    # the identity lens at integer positions copies the image
    ident = L.model((50, 50, 10, 10), (50, 50, 10, 10), (0, 0, 0, 0), 10.0)
    small = src[:21, :21]
    out, sampled, _ = L.warp_image(small, ident, "distort", 21, 21)
    assert sampled[10, 10] and (out[10, 10] == small[10, 10]).all()
