"""Float64 restatement of the sparse-depth route: the depth layers, the dense and the fused (softor) forwards and their
adjoints in closed form, a ray against every triangle with the derivative of its hit along the triangle's plane, the projection into
the camera's sample space, and the pyramid with its L1 loss.  numpy only: no torch, no device.  The adjoints are written out from the
definitions, not obtained by differentiating the forwards numerically; tests/test_sparse_depth_cpu.py holds them to the reference's own
autograd (golden g15) and to closed forms."""
import numpy as np


# ------------------------------------------------------------------------------------------ layers
def _geometry(pts, sigma, s0, s1):
    """per point and texel: offsets yd = j - p0, xd = i - p1 ([n,s1,s0]), squared distance d, value e; per point the peak texel's offsets,
    squared distance and value m.  The peak texel is rint(p) (ties to even, as rintf) clamped into the texture."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    p0, p1 = pts[:, 0] * s0, pts[:, 1] * s1
    j, i = np.arange(s0, dtype=np.float64), np.arange(s1, dtype=np.float64)
    yd = j[None, None, :] - p0[:, None, None] + 0.0 * i[None, :, None]
    xd = i[None, :, None] - p1[:, None, None] + 0.0 * j[None, None, :]
    d = yd * yd + xd * xd
    e = np.exp(-((d / sigma) ** 2))
    ys = np.clip(np.rint(p0), 0, s0 - 1) - p0
    xs = np.clip(np.rint(p1), 0, s1 - 1) - p1
    ds = ys * ys + xs * xs
    m = np.exp(-((ds / sigma) ** 2))
    return yd, xd, d, e, ys, xs, ds, m


def tie_distance(pts, s0, s1):
    """smallest distance (texels) of any scaled coordinate from a rint tie (k + 0.5)"""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    p = np.concatenate([pts[:, 0] * s0, pts[:, 1] * s1])
    return float(np.abs((p - np.floor(p)) - 0.5).min()) if p.size else 1.0


def layers(pts, depth, sigma, s0, s1):
    """[n, s1, s0]: layer_n = (e_n / m_n) z_n"""
    _, _, _, e, _, _, _, m = _geometry(pts, sigma, s0, s1)
    z = np.asarray(depth, np.float64).reshape(-1)
    return e / m[:, None, None] * z[:, None, None]


def softor(stack):
    return 1.0 - np.prod(1.0 - stack, axis=0)


def fused_forward(pts, depth, sigma, s0, s1):
    """[s1, s0] = 1 - prod_n (1 - layer_n); a zero plane without points"""
    if np.asarray(pts).size == 0:
        return np.zeros((s1, s0))
    return softor(layers(pts, depth, sigma, s0, s1))


def _adjoint_from_G(pts, depth, sigma, s0, s1, G, magnitudes=False):
    """gz_n = sum_x G_n e_n / m_n;  gp_n = (z_n / m_n) sum_x G_n (de_n/dp - (e_n / m_n) dm_n/dp) with dm_n/dp at the fixed peak texel, chained
    through p = pts * size.  de/dp0 = e 4 d yd / sigma^2 (yd = j - p0), dm/dp0 = m 4 d* yd* / sigma^2.
    magnitudes: the same sums over the ABSOLUTE values of their terms — what a rounding error of the terms is relative to."""
    yd, xd, d, e, ys, xs, ds, m = _geometry(pts, sigma, s0, s1)
    z = np.asarray(depth, np.float64).reshape(-1)
    a = np.abs if magnitudes else (lambda v: v)
    S = a(G * e).sum(axis=(1, 2))
    cf = e * 4.0 * d / sigma**2
    A0 = a(G * cf * yd).sum(axis=(1, 2))
    A1 = a(G * cf * xd).sum(axis=(1, 2))
    cs = 4.0 * ds / sigma**2
    if magnitudes:
        g0 = np.abs(z) / m * (A0 + S * cs * np.abs(ys)) * s0
        g1 = np.abs(z) / m * (A1 + S * cs * np.abs(xs)) * s1
    else:
        g0 = z / m * (A0 - S * cs * ys) * s0
        g1 = z / m * (A1 - S * cs * xs) * s1
    return np.stack([g0, g1], axis=1), S / m


def dense_adjoint(pts, depth, sigma, s0, s1, gout, magnitudes=False):
    """adjoint of layers(): gout [n, s1, s0] -> (gpts [n,2], gdepth [n])"""
    return _adjoint_from_G(pts, depth, sigma, s0, s1, np.asarray(gout, np.float64), magnitudes)


def fused_adjoint(pts, depth, sigma, s0, s1, gout, magnitudes=False):
    """adjoint of fused_forward(): gout [s1, s0] -> (gpts [n,2], gdepth [n]) with G_n = gout prod_{k != n} (1 - layer_k), the product formed
    from the other points' factors (prefix times suffix products), never by division"""
    f = 1.0 - layers(pts, depth, sigma, s0, s1)
    n = f.shape[0]
    pre = np.ones_like(f)
    suf = np.ones_like(f)
    for k in range(1, n):
        pre[k] = pre[k - 1] * f[k - 1]
    for k in range(n - 2, -1, -1):
        suf[k] = suf[k + 1] * f[k + 1]
    G = np.asarray(gout, np.float64)[None] * pre * suf
    return _adjoint_from_G(pts, depth, sigma, s0, s1, G, magnitudes)


# ------------------------------------------------------------------------------------------ rays
def trace(origins, dirs, verts, tris):
    """every ray against every triangle (Moller-Trumbore, both faces) -> (t [n] in units of the given direction, 0 on a miss;
    prim [n], -1 on a miss; the closest hit with t > 0, equal distances to the smaller index)"""
    o, d = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)
    v, f = np.asarray(verts, np.float64), np.asarray(tris, np.int64)
    v0, e1, e2 = v[f[:, 0]], v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    t_out, prim = np.zeros(len(o)), np.full(len(o), -1, np.int64)
    for r in range(len(o)):
        pv = np.cross(d[r], e2)
        det = (e1 * pv).sum(axis=1)
        tv = o[r] - v0
        qv = np.cross(tv, e1)
        with np.errstate(divide="ignore", invalid="ignore"):
            u, w, t = (tv * pv).sum(axis=1) / det, (qv * d[r]).sum(axis=1) / det, (e2 * qv).sum(axis=1) / det
        ok = (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0)
        if ok.any():
            tt = np.where(ok, t, np.inf)
            k = int(np.argmin(tt))  # (argmin returns the first of equal minima: the smaller index)
            t_out[r], prim[r] = tt[k], k
    return t_out, prim


def plane_hit(origins, dirs, verts, tris, prim):
    """on the plane of triangle prim[r] (N = (v1 - v0) x (v2 - v0)): t = N.(v0 - o) / (N.d), dt/do = -N / (N.d), dt/dd = -t N / (N.d);
    zeros where prim < 0 -> (t [n], dt_do [n,3], dt_dd [n,3])"""
    o, d = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)
    v, f = np.asarray(verts, np.float64), np.asarray(tris, np.int64)
    prim = np.asarray(prim, np.int64)
    hit = prim >= 0
    k = np.where(hit, prim, 0)
    v0, v1, v2 = v[f[k, 0]], v[f[k, 1]], v[f[k, 2]]
    N = np.cross(v1 - v0, v2 - v0)
    nd = (N * d).sum(axis=1)
    nd = np.where(hit, nd, 1.0)
    t = (N * (v0 - o)).sum(axis=1) / nd
    dt_do = -N / nd[:, None]
    dt_dd = dt_do * t[:, None]
    z = hit[:, None]
    return np.where(hit, t, 0.0), np.where(z, dt_do, 0.0), np.where(z, dt_dd, 0.0)


def hits_vjp(origins, dirs, t, dt_do, dt_dd, ghit):
    """hit = o + t d with t on its plane: the gradient of a loss on the hits with respect to (origins, dirs)"""
    d, g = np.asarray(dirs, np.float64), np.asarray(ghit, np.float64)
    gt = (g * d).sum(axis=1)
    return g + gt[:, None] * dt_do, g * np.asarray(t)[:, None] + gt[:, None] * dt_dd


# ------------------------------------------------------------------------------------------ projection
def project(points, M):
    """homogeneous 4x4 transform with the perspective divide -> [n,3]"""
    p, M = np.asarray(points, np.float64), np.asarray(M, np.float64)
    q = p @ M[:, 0:3].T + M[:, 3]
    return q[:, 0:3] / q[:, 3:4]


def project_vjp(points, M, g):
    p, M, g = np.asarray(points, np.float64), np.asarray(M, np.float64), np.asarray(g, np.float64)
    q = p @ M[:, 0:3].T + M[:, 3]
    gq = np.concatenate([g / q[:, 3:4], -(g * q[:, 0:3]).sum(axis=1, keepdims=True) / q[:, 3:4] ** 2], axis=1)
    return gq @ M[:, 0:3]


# ------------------------------------------------------------------------------------------ pyramid
def level_sizes(s0, s1, levels):
    return [(s0 // 2**i, s1 // 2**i) for i in range(levels)]


def pyramid(points, levels, sigma, s0, s1):
    """points [n,3] = (x, y, depth) -> the list of [l1, l0] planes, level i at (s0 // 2^i, s1 // 2^i)"""
    p = np.asarray(points, np.float64)
    return [fused_forward(p[:, 0:2], p[:, 2], sigma, l0, l1) for l0, l1 in level_sizes(s0, s1, levels)]


def pyramid_l1(points, targets, sigma, s0, s1):
    """sum over the levels of mean |plane - target| and its gradient with respect to the points [n,3]"""
    p = np.asarray(points, np.float64)
    loss, g = 0.0, np.zeros_like(p)
    for (l0, l1), tgt in zip(level_sizes(s0, s1, len(targets)), targets):
        diff = fused_forward(p[:, 0:2], p[:, 2], sigma, l0, l1) - np.asarray(tgt, np.float64)
        loss += np.abs(diff).mean()
        gp, gz = fused_adjoint(p[:, 0:2], p[:, 2], sigma, l0, l1, np.sign(diff) / diff.size)
        g[:, 0:2] += gp
        g[:, 2] += gz
    return loss, g


def laser_pyramid_l1(origins, dirs, verts, tris, M, targets, sigma, s0, s1, plane_term=True):
    """the whole chain rays -> hits -> sample space -> pyramid -> L1: (loss, gorigins, gdirs, points, prim).  plane_term=False drops the
    derivative of t (the hit moves with the ray as if t were a constant)."""
    t, prim = trace(origins, dirs, verts, tris)
    tp, dt_do, dt_dd = plane_hit(origins, dirs, verts, tris, prim)
    hit = np.asarray(origins, np.float64) + tp[:, None] * np.asarray(dirs, np.float64)
    pts = project(hit, M)
    loss, gp = pyramid_l1(pts, targets, sigma, s0, s1)
    ghit = project_vjp(hit, M, gp)
    if not plane_term:
        dt_do, dt_dd = np.zeros_like(dt_do), np.zeros_like(dt_dd)
    go, gd = hits_vjp(origins, dirs, tp, dt_do, dt_dd, ghit)
    return loss, go, gd, pts, prim


# ------------------------------------------------------------------------------------------ small meshes of the ray tests
def uv_sphere(n_lon=8, n_lat=4, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """(verts [V,3] float32, tris [F,3] int32) of a uv sphere: n_lon segments around, n_lat bands from pole to pole"""
    verts = [(0.0, 0.0, 1.0)]
    for a in range(1, n_lat):
        th = np.pi * a / n_lat
        for b in range(n_lon):
            ph = 2.0 * np.pi * b / n_lon
            verts.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    verts.append((0.0, 0.0, -1.0))
    ring = lambda a, b: 1 + (a - 1) * n_lon + b % n_lon  # noqa: E731
    tris = [(0, ring(1, b), ring(1, b + 1)) for b in range(n_lon)]
    for a in range(1, n_lat - 1):
        for b in range(n_lon):
            tris += [(ring(a, b), ring(a + 1, b), ring(a + 1, b + 1)), (ring(a, b), ring(a + 1, b + 1), ring(a, b + 1))]
    last = len(verts) - 1
    tris += [(last, ring(n_lat - 1, b + 1), ring(n_lat - 1, b)) for b in range(n_lon)]
    v = np.asarray(verts, np.float64) * radius + np.asarray(centre, np.float64)
    return v.astype(np.float32), np.asarray(tris, np.int32)


def quad(corners):
    """two triangles over four corners given in order around the quad"""
    return np.asarray(corners, np.float32), np.asarray([[0, 1, 2], [0, 2, 3]], np.int32)
