"""numpy yardstick of the renderer (include/myobatch.h myo_batch_render, csrc/myo_render.h): the same camera, rays and analytic
intersections in float64, written from the definitions rather than from the kernel's code.  Input: the pose pass's item table
(myo_batch_geom_poses, [nitem, 24]); output: segmentation, depth, rgb and a mask of edge pixels, where an fp32 kernel and this
fp64 reference may legitimately disagree: pixels whose id changes when the ray moves by +-0.01 px, and pixels where two items'
surfaces are equally near (within 1e-6 of the depth: coincident surfaces, such as the shared end spheres of the die's edge
capsules)."""
from __future__ import annotations

import numpy as np

PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX = 0, 2, 3, 4, 5, 6
BACKGROUND = np.array([0.12, 0.14, 0.18])


def camera_frame(cam, height):
    """MuJoCo free camera -> (position, forward, right, up, focal length in pixels)."""
    az, el = np.radians(cam["azimuth"]), np.radians(cam["elevation"])
    fwd = np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    up = np.array([-np.sin(el) * np.cos(az), -np.sin(el) * np.sin(az), np.cos(el)])
    right = np.cross(fwd, up)
    pos = np.asarray(cam["lookat"], float) - cam["distance"] * fwd
    f = 0.5 * height / np.tan(0.5 * np.radians(cam["fovy"]))
    return pos, fwd, right, up, f


def default_camera_from_stat(center, extent):
    return {"lookat": tuple(center), "distance": 1.5 * extent, "azimuth": 90.0, "elevation": -45.0, "fovy": 45.0}


def rays(cam, width, height, jx=0.0, jy=0.0):
    """ray directions [H, W, 3] with unit forward component (so that the ray parameter is the depth); row 0 at the top"""
    pos, fwd, right, up, f = camera_frame(cam, height)
    tx = (np.arange(width) + 0.5 + jx - 0.5 * width) / f
    ty = (0.5 * height - (np.arange(height) + 0.5 + jy)) / f
    d = fwd[None, None, :] + tx[None, :, None] * right[None, None, :] + ty[:, None, None] * up[None, None, :]
    return pos, d


def _quad(a, b, c):
    """smallest positive root of a t^2 + 2 b t + c (inf if none)"""
    disc = b * b - a * c
    ok = (disc >= 0) & (a > 0)
    sq = np.sqrt(np.where(ok, disc, 0.0))
    a_ = np.where(a > 0, a, 1.0)
    t0, t1 = (-b - sq) / a_, (-b + sq) / a_
    t = np.where(t0 > 0, t0, np.where(t1 > 0, t1, np.inf))
    return np.where(ok, t, np.inf)


def hit(typ, sz, o, d):
    """ray (origin o [3], directions d [..., 3], item-local) -> t [...] and local normals [..., 3]"""
    n = np.zeros(d.shape)
    n[..., 2] = 1
    dot = lambda x, y: (x * y).sum(-1)
    if typ in (SPHERE, ELLIPSOID):
        s = np.array([sz[0]] * 3) if typ == SPHERE else np.asarray(sz, float)
        os_, ds = o / s, d / s
        t = _quad(dot(ds, ds), (os_ * ds).sum(-1), dot(os_, os_) - 1.0)
        p = o + np.where(np.isfinite(t), t, 0)[..., None] * d
        return t, p / (s * s)
    if typ in (CAPSULE, CYLINDER):
        r, h = sz[0], sz[1]
        t = _quad(d[..., 0] ** 2 + d[..., 1] ** 2, o[0] * d[..., 0] + o[1] * d[..., 1], o[0] ** 2 + o[1] ** 2 - r * r)
        z = o[2] + np.where(np.isfinite(t), t, 0) * d[..., 2]
        t = np.where(np.isfinite(t) & (np.abs(z) <= h), t, np.inf)
        p = o + np.where(np.isfinite(t), t, 0)[..., None] * d
        n = np.stack([p[..., 0], p[..., 1], np.zeros_like(t)], -1)
        for e in (-1.0, 1.0):
            if typ == CAPSULE:
                oc = o - np.array([0, 0, e * h])
                ts = _quad(dot(d, d), (oc * d).sum(-1), dot(oc, oc) - r * r)
                better = ts < t
                ps = oc + np.where(np.isfinite(ts), ts, 0)[..., None] * d
                n = np.where(better[..., None], ps, n)
                t = np.where(better, ts, t)
            else:
                with np.errstate(divide="ignore", invalid="ignore"):
                    tp = (e * h - o[2]) / d[..., 2]
                x, y = o[0] + tp * d[..., 0], o[1] + tp * d[..., 1]
                better = (tp > 0) & (tp < t) & (x * x + y * y <= r * r)
                n = np.where(better[..., None], np.array([0, 0, e]), n)
                t = np.where(better, tp, t)
        return t, n
    if typ == BOX:
        with np.errstate(divide="ignore", invalid="ignore"):
            ta = (-np.asarray(sz) - o) / d
            tb = (np.asarray(sz) - o) / d
        lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
        tn, tf = lo.max(-1), hi.min(-1)
        ax = lo.argmax(-1)
        t = np.where((tn <= tf) & (tf > 0), np.where(tn > 0, tn, tf), np.inf)
        sg = -np.sign(np.take_along_axis(d, ax[..., None], -1)[..., 0])
        n = np.zeros(d.shape)
        np.put_along_axis(n, ax[..., None], sg[..., None], -1)
        return t, n
    if typ == PLANE:
        with np.errstate(divide="ignore", invalid="ignore"):
            tp = -o[2] / d[..., 2]
        x, y = o[0] + tp * d[..., 0], o[1] + tp * d[..., 1]
        inside = (sz[0] <= 0) | (sz[1] <= 0) | ((np.abs(x) <= sz[0]) & (np.abs(y) <= sz[1]))
        return np.where((tp > 0) & inside, tp, np.inf), n
    return np.full(d.shape[:-1], np.inf), n


def _cast(items, cam, width, height, show_sites, jx=0.0, jy=0.0):
    pos, d = rays(cam, width, height, jx, jy)
    shp = d.shape[:2]
    best = {"o": (np.full(shp, np.inf), np.full(shp, -1), np.zeros(shp + (3,)), np.full(shp, np.inf)),
            "t": (np.full(shp, np.inf), np.full(shp, -1), np.zeros(shp + (3,)), np.full(shp, np.inf))}
    for i, it in enumerate(items):
        if it[19] <= 0 or (it[21] != 0 and not show_sites):
            continue
        R = it[3:12].reshape(3, 3)
        o = R.T @ (pos - it[0:3])
        dl = d @ R
        t, nl = hit(int(it[15]), it[12:15], o, dl)
        key = "o" if it[19] >= 1 else "t"
        bt, bi, bn, b2 = best[key]          # b2: the second-nearest depth
        better = t < bt
        b2[:] = np.where(better, bt, np.minimum(b2, t))
        bt[better], bi[better] = t[better], i
        bn[better] = (nl @ R.T)[better]
    return d, best


def _shade(items, idx, n, d):
    rgba = items[np.maximum(idx, 0), 16:20]
    nn, dd = np.linalg.norm(n, axis=-1), np.linalg.norm(d, axis=-1)
    cs = np.where(nn > 0, np.abs((n * d).sum(-1)) / np.where(nn > 0, nn * dd, 1), 1.0)
    return rgba[..., :3] * (0.3 + 0.7 * np.minimum(cs, 1))[..., None], rgba[..., 3]


def render(items, cam, width, height, show_sites=False, edges=True):
    """-> seg int [H, W], depth [H, W], rgb uint8 [H, W, 3], edge mask [H, W]"""
    items = np.asarray(items, float)
    d, best = _cast(items, cam, width, height, show_sites)
    to, io, no, to2 = best["o"]
    tt, it, nt, tt2 = best["t"]
    front = (it >= 0) & (tt < to)
    seg = np.where(front, it, io)
    depth = np.where(front, tt, to).astype(np.float64)
    c_o, _ = _shade(items, io, no, d)
    c = np.where((io >= 0)[..., None], c_o, BACKGROUND)
    c_t, a = _shade(items, it, nt, d)
    c = np.where(front[..., None], a[..., None] * c_t + (1 - a[..., None]) * c, c)
    rgb = np.clip(np.floor(c * 255 + 0.5), 0, 255).astype(np.uint8)
    def near(a, b):
        with np.errstate(invalid="ignore"):
            return np.isfinite(a) & (np.abs(b - a) <= 1e-6 * a)
    edge = near(to, to2) | near(tt, tt2) | near(np.minimum(to, tt), np.maximum(to, tt))
    if edges:
        for jx, jy in ((0.01, 0), (-0.01, 0), (0, 0.01), (0, -0.01)):
            _, b2 = _cast(items, cam, width, height, show_sites, jx, jy)
            f2 = (b2["t"][1] >= 0) & (b2["t"][0] < b2["o"][0])
            edge |= np.where(f2, b2["t"][1], b2["o"][1]) != seg
    return seg, depth, rgb, edge
