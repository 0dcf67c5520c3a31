"""Cases of the sparse-depth suites (tests/test_sparse_depth_cpu.py, tests/test_sparse_depth_gpu.py) — TEST INFRASTRUCTURE, numpy and
the package's scene records only: the golden fixture's blocks, the meshes and seeded rays of the ray tests, the two-plane scene of the
end-to-end test with its laser pattern, and the float64 fit that states how far the example's loop must get."""
import numpy as np

from fireflies_amd import scenes
from tests import ref_sparse_depth as ref
from tests.conftest import load_golden

F32 = np.float32
SIGMA = 6.0
MIN_COS = 0.2  # the ray tests keep rays that meet their triangle at |N.d| / (|N| |d|) >= 0.2


# ------------------------------------------------------------------------------------------ golden g15
def g15_blocks():
    """-> (g, [(case, level, pts, depth, l0, l1)]) over every stored case and level of golden g15"""
    g = load_golden("g15_depth_pyramid_grad.npz")
    out = []
    for case in [str(c) for c in g["cases"]]:
        s0, s1 = (int(v) for v in case.split("_")[1].split("x"))
        for lv, (l0, l1) in enumerate(ref.level_sizes(s0, s1, int(g["levels"]))):
            out.append((case, lv, g[f"{case}_pts"], g[f"{case}_depth"], l0, l1))
    return g, out


def g15_bound(g, key):
    """the bound of one gradient block: 4 x the deviation of the reference's float32 autograd from its float64 autograd on that block, and
    the block's largest magnitude it is relative to -> (absolute bound, scale)"""
    r64 = g[key + "_f64"]
    scale = float(np.abs(r64).max())
    return 4.0 * float(np.abs(g[key + "_f32"].astype(np.float64) - r64).max()), scale


# ------------------------------------------------------------------------------------------ ray cases
def ray_meshes():
    """name -> (verts float32 [V,3], tris int32 [F,3]): an axis-aligned plane z = 2, a tilted pair of triangles, an 8 x 4 uv sphere"""
    plane = ref.quad([(-4, -4, 2), (4, -4, 2), (4, 4, 2), (-4, 4, 2)])
    tilted = ref.quad([(-3, -3, 1.0), (3, -3, 2.5), (3, 3, 4.0), (-3, 3, 2.5)])
    sphere = ref.uv_sphere(8, 4, 1.0, (0.0, 0.0, 3.0))
    return {"plane": plane, "tilted": tilted, "sphere": sphere}


def seeded_rays(name, n=96, seed=0, spread=0.8, miss_every=8):
    """float32 rays towards a mesh of ray_meshes(): origins scattered around the world origin, directions of lengths 0.5 .. 2 (not
    unit) aimed at a disc of radius `spread` in the plane z = 3, one ray in `miss_every` aimed past the mesh (0: none).  Only rays that miss or meet
    their triangle at MIN_COS or steeper are kept (decided by the float64 reference on the float32 values) -> (origins, dirs)"""
    verts, tris = ray_meshes()[name]
    rng = np.random.default_rng(seed)
    o = (rng.random((4 * n, 3)) - 0.5) * np.array([0.6, 0.6, 0.4])
    a, r = rng.random(4 * n) * 2 * np.pi, np.sqrt(rng.random(4 * n)) * spread
    tgt = np.stack([r * np.cos(a), r * np.sin(a), np.full(4 * n, 3.0)], -1)
    if miss_every:
        tgt[::miss_every] += (9.0, 0.0, 0.0)
    d = tgt - o
    d *= ((0.5 + 1.5 * rng.random(4 * n)) / np.linalg.norm(d, axis=1))[:, None]
    o, d = o.astype(F32), d.astype(F32)
    _, prim = ref.trace(o, d, verts, tris)
    keep = prim < 0
    hit = np.flatnonzero(prim >= 0)
    f = tris[prim[hit]]
    N = np.cross(verts[f[:, 1]].astype(np.float64) - verts[f[:, 0]], verts[f[:, 2]].astype(np.float64) - verts[f[:, 0]])
    cos = np.abs((N * d[hit]).sum(axis=1)) / (np.linalg.norm(N, axis=1) * np.linalg.norm(d[hit].astype(np.float64), axis=1))
    keep[hit[cos >= MIN_COS]] = True
    idx = np.flatnonzero(keep)[:n]
    assert len(idx) == n
    return np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx])


CD_H = 2.0**-9  # step of the central differences of t
CD_RAYS = dict(name="sphere", n=64, seed=3, spread=0.8, miss_every=0)  # the rays of the central-difference test: all hit


def cd_neighbours(o, d):
    """the 12 n perturbed rays of central differences: for axis a of the origin, then of the direction, +h and -h, as float32 ->
    (origins [12,n,3], dirs [12,n,3]); row 2 (3 w + a) + s: w 0 origin / 1 direction, s 0 plus / 1 minus"""
    oo, dd = np.repeat(o[None], 12, axis=0).copy(), np.repeat(d[None], 12, axis=0).copy()
    for w in range(2):
        for a in range(3):
            for s in range(2):
                (oo if w == 0 else dd)[2 * (3 * w + a) + s, :, a] += F32(CD_H if s == 0 else -CD_H)
    return oo, dd


def cd_from_t(o, d, oo, dd, t12, prim12, prim):
    """central differences of t (float64 arithmetic on the given t) -> (dt_do [n,3], dt_dd [n,3], usable [n]): a ray is usable when it hits and
    all 12 neighbours hit the same primitive"""
    usable = (prim >= 0) & (prim12 == prim[None]).all(axis=0)
    t12 = np.asarray(t12, np.float64)
    out = np.zeros((2, len(o), 3))
    for w in range(2):
        base = oo if w == 0 else dd
        for a in range(3):
            r = 2 * (3 * w + a)
            step = base[r, :, a].astype(np.float64) - base[r + 1, :, a].astype(np.float64)
            out[w, :, a] = (t12[r] - t12[r + 1]) / step
    return out[0], out[1], usable


def cd_bound(o, d, verts, tris, prim, t):
    """what central differences of a float32 t may miss the plane derivative by, per ray and per component -> (bound_do, bound_dd) [n,3].
    t is linear in o and c / (a + h b) in a component of d (a = N.d, b = N_i): the central difference is the derivative over 1 - (h b / a)^2.  The
    forward's t carries a relative error of a few rounding steps over the cosine (Moller-Trumbore's determinant cancels by that factor): taken as
    16 eps32 / cos on each of the two values, over the step 2 h."""
    f = tris[np.where(prim >= 0, prim, 0)]
    v = verts.astype(np.float64)
    N = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    a = (N * d).sum(axis=1)
    cos = np.abs(a) / (np.linalg.norm(N, axis=1) * np.linalg.norm(d.astype(np.float64), axis=1))
    noise = (16.0 * 2.0**-24 / cos * np.abs(t) / CD_H)[:, None]
    _, dt_do, dt_dd = ref.plane_hit(o, d, verts, tris, prim)
    hb = (CD_H * N / a[:, None]) ** 2
    return noise + 0.0 * dt_do, noise + np.abs(dt_dd) * hb / (1.0 - hb)


# ------------------------------------------------------------------------------------------ end to end
E2E_SENSOR = 48          # the camera's film, and the finest level of the pyramid
E2E_LEVELS = 3
E2E_OFFSET = (0.035, -0.02)  # the start pattern is the target displaced by this much in x, y before normalisation
E2E_LR = 2e-3
LASER_FOV, LASER_NEAR, LASER_FAR = 40.0, 0.01, 100.0


def two_planes():
    """two planes facing the laser at the origin (which looks down +z): the left half (x < 0) at z = 3, the right half tilted from z = 3.4 at
    x = 0 to z = 4.0 at x = 3 — a depth step in the middle of the pattern.  The camera stands beside the laser and looks at (0, 0, 3.3)."""
    lv, lt = ref.quad([(-3, -3, 3.0), (0, -3, 3.0), (0, 3, 3.0), (-3, 3, 3.0)])
    rv, rt = ref.quad([(0, -3, 3.4), (3, -3, 4.0), (3, 3, 4.0), (0, 3, 3.4)])
    mesh = lambda n, v, t: scenes.MeshData("mesh-" + n, np.ascontiguousarray(v, F32)[None], np.ascontiguousarray(t, np.int32), (0.7, 0.7, 0.7), "mat-" + n)  # noqa: E731
    cam = scenes.SensorData("PerspectiveCamera", scenes.look_at((0.4, 0.25, 0.0), (0.0, 0.0, 3.3)), 45.0, 0.5, 20.0, E2E_SENSOR, E2E_SENSOR)
    return scenes.SceneData([mesh("Left", lv, lt), mesh("Right", rv, rt)], cam, None, None)


def world_mesh(data):
    """(verts, tris) of a static SceneData in one index space, the primitives numbered mesh after mesh as the device numbers them"""
    vs, ts, base = [], [], 0
    for m in data.meshes:
        vs.append(m.frames[0])
        ts.append(m.tris + base)
        base += m.frames[0].shape[0]
    return np.concatenate(vs).astype(F32), np.concatenate(ts).astype(np.int32)


def world_to_sample(cam):
    """float32 4x4 world -> the camera's sample space, formed as graphics.depth forms it"""
    from fireflies_amd import mi

    K = mi.perspective_projection((cam.width, cam.height), (cam.width, cam.height), (0, 0), cam.fov_x, cam.near, cam.far).numpy().astype(np.float64)
    return (K @ np.linalg.inv(np.asarray(cam.to_world, np.float64))).astype(F32)


def laser_K():
    from fireflies_amd import mi

    return mi.perspective_projection((1, 1), (1, 1), (0, 0), LASER_FOV, LASER_NEAR, LASER_FAR).numpy().astype(F32)


def pattern(offset=(0.0, 0.0)):
    """16 unit rays (float32) of a 4 x 4 grid around +z, displaced by `offset` before normalisation"""
    g = np.linspace(-0.21, 0.21, 4)
    x, y = np.meshgrid(g, g, indexing="xy")
    r = np.stack([x.reshape(-1) + offset[0], y.reshape(-1) + offset[1], np.ones(16)], -1)
    return (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F32)


def clamp_and_normalize(rays, KF, lo=0.05, hi=0.95):
    """Laser.clamp_to_fov + normalize_rays in float64: project with KF, clamp x and y, un-project with its inverse, normalise twice"""
    KF = np.asarray(KF, np.float64)
    p = ref.project(rays, KF)
    p[:, 0:2] = np.clip(p[:, 0:2], lo, hi)
    r = ref.project(p, np.linalg.inv(KF))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    return r / np.linalg.norm(r, axis=1, keepdims=True)


def e2e_loss_grad(rays, targets, verts, tris, M, plane_term=True):
    """the L1 pyramid loss of the laser at the origin with identity pose and its gradient with respect to the rays (float64)"""
    o = np.zeros_like(np.asarray(rays, np.float64))
    loss, _, gd, pts, prim = ref.laser_pyramid_l1(o, rays, verts, tris, M, targets, SIGMA, E2E_SENSOR, E2E_SENSOR, plane_term)
    return loss, gd, pts, prim


def e2e_targets(verts, tris, M):
    o = np.zeros((16, 3))
    rays = pattern()
    t, prim = ref.trace(o, rays, verts, tris)
    assert (prim >= 0).all()
    pts = ref.project(o + t[:, None] * rays.astype(np.float64), M)
    assert (pts > 0.02).all() and (pts < 0.98).all()
    return [p.astype(F32) for p in ref.pyramid(pts, E2E_LEVELS, SIGMA, E2E_SENSOR, E2E_SENSOR)]


def reference_fit(steps, lr=E2E_LR):
    """the example's loop in float64: Adam (torch.optim.Adam's defaults) on the rays from the displaced pattern, clamp_to_fov and normalize_rays
    after each step -> the losses before each step and after the last ([steps + 1])"""
    data = two_planes()
    verts, tris = world_mesh(data)
    M = world_to_sample(data.camera)
    targets = e2e_targets(verts, tris, M)
    KF = laser_K().astype(np.float64) @ np.diag([1.0, -1.0, 1.0, 1.0])
    rays = pattern(E2E_OFFSET).astype(np.float64)
    m, v = np.zeros_like(rays), np.zeros_like(rays)
    losses = []
    for k in range(1, steps + 1):
        loss, g, _, _ = e2e_loss_grad(rays, targets, verts, tris, M)
        losses.append(loss)
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        rays = rays - (lr / (1 - 0.9**k)) * m / (np.sqrt(v) / np.sqrt(1 - 0.999**k) + 1e-8)
        rays = clamp_and_normalize(rays, KF)
    losses.append(e2e_loss_grad(rays, targets, verts, tris, M)[0])
    return np.asarray(losses)
