"""The cases of tests/test_mpr_cases_cpu.py and tests/test_gpu_mpr_edges.py: hull families, pose families, scenes and seeds of the convex narrow phase (uhc_mpr.h).

Nothing here touches a device.  The CPU file holds the oracle's MPR against plain geometry on exactly these inputs (polytope distance, the support bound on the depth,
the normal's direction, closed forms, covariance) and measures how stable the oracle's own answer is on each of them; the GPU file then holds every serving path of the
device to the oracle on the same inputs.

Every two-body case is two free bodies 2 m above the floor (the floor is geom 0 as in every model of this build; nothing reaches it).  A case is a row of qpos (14) and a
row of qvel (12); its pose family is a tag.  The hulls' vertices are read back from the COMPILED model (body frame, in the model's own order), so a pose built here is a
pose of what the kernels see."""
import dataclasses
import functools

import numpy as np

from tests.helpers import box_triangles, hull_triangles, passive_ctrl

MARGIN = 0.001
HEIGHT = 2.0
ORIGIN = np.array([0.25, -0.5, HEIGHT])  # where body A sits: no coordinate is 0, so that R c + x rounds a centre of 1e-18 away and centre differences are exact
N_CASES = 96          # per hull family: one batch of 64 envs and one of 32
BATCH = 64
TAGS = ("random", "face", "face_yaw", "quarter", "coincident", "vertex_line", "margin_edge", "inside")


# ------------------------------------------------------------------ hulls
def fibonacci(n):
    k = np.arange(n) + 0.5
    phi, th = np.arccos(1 - 2 * k / n), np.pi * (1 + 5 ** 0.5) * k
    return np.c_[np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)]


def ball(n, r, stretch=(1.0, 0.8, 0.65)):
    """n points on an ellipsoid: strictly convex, so every point is a hull vertex; stretched, so no two directions see the same hull; and MIRROR-SYMMETRIC in x (n // 2
    points with x > 0, their mirror images, and for an odd n one point with x = 0): along a direction with no x component the two vertices of a mirror pair have the
    same projection to the last bit, with and without fused multiply-adds -- an exact tie of the support arg-max, between vertices that a hull of more than 64 keeps in
    different trips of the scan as often as not"""
    p = fibonacci(2 * n)
    p = p[p[:, 0] > 0.04][:n // 2]
    p = np.r_[p, p * [-1.0, 1.0, 1.0]]
    if n % 2:
        p = np.r_[p, [[0.0, 0.6, 0.8]]]
    assert len(p) == n
    return centred(r * p * np.asarray(stretch))


def centred(v):
    """the vertices about their hull's centre of mass: the compiled geom centre is then 0 to 1e-18, and two bodies at one point have coincident centres whatever the
    rounding of R c + x"""
    from uhc_amd.model.mjcf import polyhedron_mass_properties, weld
    for _ in range(2):
        verts, faces = weld(hull_triangles(v))
        v = v - polyhedron_mass_properties(verts, faces)[1] * [0.0, 1.0, 1.0]  # (x: zero by the hulls' mirror symmetry; not touched, so that the symmetry stays exact)
    return v


def poles_ball(r, u, n=50):
    """tests/test_oracle_physics.py's ball, made point-symmetric (its centre of mass is the origin exactly): Fibonacci points of one half, their mirror images and the two
    exact poles +-u -- a support query along u returns a pole, a point ON the centre line"""
    p = fibonacci(n)[:n // 2]
    p = p[np.abs(p @ u) < 0.995]
    return r * np.r_[p, -p, [u], [-u]]


def tetra(r):
    return r * np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / np.sqrt(3.0)


def box(hx, hy, hz):
    return box_triangles(hx, hy, hz).reshape(-1, 3)


def house(h):
    """a box with a roof apex, 9 vertices, its centre of mass at the origin (so that two bodies at one point have coincident geom centres)"""
    vb, vp = 8.0 * h ** 3, 4.0 * h * h * 0.7 * h / 3.0
    return np.r_[np.unique(box(h, h, h), axis=0), [[0.0, 0.0, 1.7 * h]]] - [0.0, 0.0, vp * (h + 0.7 * h / 4.0) / (vb + vp)]


POLE = np.array([2.0, -1.0, 2.0]) / 3.0
# name -> (hull of body A, hull of body B).  An array is a mesh's vertices; ("sphere", r) and ("capsule", r, half length) are rounded hulls (1 and 2 core vertices).
FAMILIES = {
    "tetra": (tetra(0.1), tetra(0.07)),
    "box": (box(0.1, 0.1, 0.1), box(0.06, 0.06, 0.06)),
    "ball50": (ball(50, 0.1), ball(50, 0.07)),
    "ball64": (ball(64, 0.1), ball(64, 0.07)),             # no idle lane in the arg-max
    "ball65": (ball(65, 0.1), ball(65, 0.07)),             # the second trip of hull_support_wave serves ONE vertex
    "ball130_house9": (ball(130, 0.1), house(0.05)),       # three trips against one
    "poles": (poles_ball(0.1, POLE), poles_ball(0.07, POLE)),
    "box_sphere": (box(0.1, 0.1, 0.1), ("sphere", 0.05)),
    "box_capsule": (box(0.1, 0.1, 0.1), ("capsule", 0.03, 0.06)),
}
VERTS = {"tetra": (4, 4), "box": (8, 8), "ball50": (50, 50), "ball64": (64, 64), "ball65": (65, 65), "ball130_house9": (130, 9), "poles": (52, 52),
         "box_sphere": (8, 1), "box_capsule": (8, 2)}


def _f(x):
    return repr(float(x))


def _rounded(h):
    return isinstance(h, tuple)


# ------------------------------------------------------------------ scenes
def hull_scene_model(meshes, joints, condim=1, pos=None, quat=None):
    """N bodies in one collision group above the floor, body k carrying hull meshes[k] on joints[k]: "free", or ("slide", axis) -- one slide joint along `axis`.
    pos / quat: the bodies' frames (default: stacked 1 m apart from HEIGHT up, far from each other).  Exact solve (solver 1), as the MPR tests use it."""
    from uhc_amd.model.mjcf import compile_mjcf
    n = len(meshes)
    pos = np.array([[0.0, 0.0, HEIGHT + k] for k in range(n)]) if pos is None else np.asarray(pos, dtype=np.float64)
    quat = np.tile([1.0, 0, 0, 0], (n, 1)) if quat is None else np.asarray(quat, dtype=np.float64)
    assets, bodies, tris = [], [], {}
    for k, (h, j) in enumerate(zip(meshes, joints)):
        if _rounded(h) and h[0] == "sphere":
            geom = f'<geom type="sphere" size="{_f(h[1])}"/>'
        elif _rounded(h):
            geom = f'<geom type="capsule" size="{_f(h[1])}" fromto="{_f(-h[2])} 0 0 {_f(h[2])} 0 0"/>'
        else:
            tris[f"h{k}"] = hull_triangles(np.asarray(h, dtype=np.float64))
            assets.append(f'<mesh name="h{k}" file="unused.stl"/>')
            geom = f'<geom type="mesh" mesh="h{k}"/>'
        jn = f'<joint name="j{k}" type="free"/>' if j == "free" else f'<joint name="j{k}" type="slide" axis="{_f(j[1][0])} {_f(j[1][1])} {_f(j[1][2])}" pos="0 0 0"/>'
        p, q = pos[k], quat[k]
        bodies.append(f'<body name="b{k}" pos="{_f(p[0])} {_f(p[1])} {_f(p[2])}" quat="{_f(q[0])} {_f(q[1])} {_f(q[2])} {_f(q[3])}">{jn}{geom}</body>')
    xml = f"""
<mujoco>
  <compiler angle="radian" coordinate="local" inertiafromgeom="true"/>
  <option timestep="0.002"/>
  <default><geom contype="1" conaffinity="1" condim="{condim}" margin="{MARGIN}"/></default>
  <asset>{''.join(assets)}</asset>
  <worldbody>
    <geom name="floor" type="plane" size="10 10 0.1" pos="0 0 0" condim="3"/>
    {''.join(bodies)}
  </worldbody>
</mujoco>
"""
    return dataclasses.replace(compile_mjcf(xml, meshes=tris), solver=1)


@functools.lru_cache(maxsize=None)
def family_model(name):
    a, b = FAMILIES[name]
    return hull_scene_model([a, b], ["free", "free"])


def geom_hull(m, g):
    """(core vertices in the body frame [n][3], radius, centre in the body frame) of geom g of a compiled model"""
    from uhc_amd.model.mjcf import geom_radius
    a, n = int(m.geom_vertadr[g]), int(m.geom_vertnum[g])
    return np.asarray(m.mesh_vert[a:a + n], dtype=np.float64), float(geom_radius(m)[g]), np.asarray(m.geom_center[g], dtype=np.float64)


def quat_of(R):
    """scipy Rotation -> (w, x, y, z)"""
    return np.roll(R.as_quat(), 1)


def pose_q(pa, Ra, pb, Rb):
    return np.r_[pa, quat_of(Ra), pb, quat_of(Rb)]


# ------------------------------------------------------------------ poses
def _faces(v):
    """outward unit normals and centroids of a hull's faces (coplanar triangles merged by their normal)"""
    from scipy.spatial import ConvexHull
    h = ConvexHull(v)
    out = {}
    for s, eq in zip(h.simplices, h.equations):
        out.setdefault(tuple(np.round(eq[:3], 9)), []).append(s)
    return [(np.array(n), v[np.unique(np.concatenate(ss))].mean(axis=0)) for n, ss in out.items()]


def _rot_to(a, b):
    """a rotation that takes unit vector a to unit vector b"""
    from scipy.spatial.transform import Rotation as sR
    c = np.cross(a, b)
    s, d = np.linalg.norm(c), float(a @ b)
    if s < 1e-12:
        if d > 0:
            return sR.identity()
        o = np.cross(a, [1.0, 0, 0] if abs(a[0]) < 0.9 else [0.0, 1, 0])
        return sR.from_rotvec(np.pi * o / np.linalg.norm(o))
    return sR.from_rotvec(c / s * np.arctan2(s, d))


class _Hulls:
    """the two hulls of a family as the compiled model has them, and what the pose builders ask of them"""

    def __init__(self, name):
        from scipy.spatial.transform import Rotation as sR
        self.sR = sR
        self.m = family_model(name)
        (self.va, self.ra, self.ca), (self.vb, self.rb, self.cb) = geom_hull(self.m, 1), geom_hull(self.m, 2)
        self.fa = _faces(self.va)
        # a rounded hull has no faces: its "face" along -z is the sphere's / capsule's lowest point(s)
        self.fb = _faces(self.vb) if len(self.vb) >= 4 else [(np.array([0.0, 0.0, -1.0]), self.vb.mean(axis=0))]

    def support(self, v, r, d):
        return float((v @ d).max()) + r

    def face_pose(self, ia, ib, Rw, yaw, gap, shift=(0.0, 0.0)):
        """B's face ib flat on A's face ia (outward normals opposed), the faces' centroids `shift` apart in the face plane, `gap` between the (inflated by the radius) surfaces
        -- the polytopes' distance is max(gap, 0) wherever the faces overlap; then the whole scene turned by Rw.  yaw: B turned about the shared normal."""
        sR = self.sR
        na, pa = self.fa[ia % len(self.fa)]
        nb, pb = self.fb[ib % len(self.fb)]
        Rb = sR.from_rotvec(yaw * na) * _rot_to(nb, -na)
        t1 = np.cross(na, [1.0, 0, 0] if abs(na[0]) < 0.9 else [0.0, 1, 0])
        t1 /= np.linalg.norm(t1)
        t2 = np.cross(na, t1)
        # world (before Rw): A at the origin with the identity; B's face centroid over A's, (gap + radii) along na
        xb = pa + na * (gap + self.ra + self.rb) + shift[0] * t1 + shift[1] * t2 - Rb.apply(pb)
        o = ORIGIN
        return pose_q(o, Rw, o + Rw.apply(xb), Rw * Rb)

    def centre_pose(self, Ra, Rb, d, gap):
        """B's centre on the line from A's centre along d; the surfaces `gap` apart ALONG d (the polytopes are then at most that far apart, and apart if gap > 0)"""
        s = self.support(self.va - self.ca, self.ra, Ra.inv().apply(d)) + self.support(self.vb - self.cb, self.rb, Rb.inv().apply(-d))
        o = ORIGIN
        xa = o - Ra.apply(self.ca)                      # A's centre at o
        xb = o + d * (s + gap) - Rb.apply(self.cb)
        return pose_q(xa, Ra, xb, Rb)


HALF_TURNS = [((1.0, 0, 0, 0), (1.0, 0, 0, 0), (0.0, 0.0, 1.0)), ((1.0, 0, 0, 0), (0.0, 1.0, 0, 0), (0.0, 1.0, 0.0)), ((0.0, 0, 1.0, 0), (0.0, 0, 0, 1.0), (0.0, 0.0, 1.0)),
              ((0.0, 0, 0, 1.0), (1.0, 0, 0, 0), (0.0, -1.0, 0.0))]
QUARTER = [(0.0, 0, 0), (np.pi / 2, 0, 0), (0, np.pi / 2, 0), (0, 0, np.pi / 2), (np.pi, 0, 0), (np.pi / 2, np.pi / 2, 0), (0, np.pi, np.pi / 2), (-np.pi / 2, 0, np.pi)]


@functools.lru_cache(maxsize=None)
def family_cases(name):
    """-> (qpos [N_CASES][14], qvel [N_CASES][12], tags [N_CASES]) of hull family `name`, seeded by the name's place in FAMILIES"""
    from scipy.spatial.transform import Rotation as sR
    H = _Hulls(name)
    seed = 100 + list(FAMILIES).index(name)
    rng = np.random.default_rng(seed)
    q, tags = [], []

    def add(tag, pose):
        q.append(pose)
        tags.append(tag)

    def unit():
        d = rng.normal(size=3)
        return d / np.linalg.norm(d)

    # face on face, a shared arbitrary rotation: gaps on both sides of the margin and deep; with and without B's yaw about the shared normal
    gaps = (-0.006, -0.0004, 0.0004, 0.003)
    for k in range(12):
        Rw = sR.from_rotvec(rng.normal(size=3))
        sh = rng.uniform(-0.01, 0.01, size=2)
        add("face", H.face_pose(k, 2 * k + 1, Rw, 0.0, gaps[k % 4], sh))
    for k in range(12):
        Rw = sR.from_rotvec(rng.normal(size=3))
        sh = rng.uniform(-0.01, 0.01, size=2)
        add("face_yaw", H.face_pose(k + 3, k, Rw, rng.uniform(0.1, 3.0), gaps[k % 4], sh))
    # the identity and exact quarter turns of the whole scene (every entry of the rotation matrices 0 or +-1 up to rounding): exact ties of the arg-max on a face
    for k, e in enumerate(QUARTER[:4]):
        # (the first two centroid over centroid -- the origin ray then runs through a corner of the portal's triangles, the `dt == 0` tests of discoverPortal; the others shifted)
        add("quarter", H.face_pose(k, k, sR.from_euler("xyz", e), (0.0, np.pi / 2)[k % 2], gaps[k % 4], (0.0, 0.0) if k < 2 else rng.uniform(-0.01, 0.01, size=2)))
    # ... and the identity and exact HALF turns (quaternions with one entry 1: the rotation matrices are 0 and +-1 exactly, which a quarter turn's are not), the centre
    # line exactly along z or y: every support query of the first rounds has a zero x component in both body frames
    for k, (qa, qb, d) in enumerate(HALF_TURNS):
        Ra, Rb, d = sR.from_quat(np.roll(qa, -1)), sR.from_quat(np.roll(qb, -1)), np.array(d)
        t = H.support(H.va, H.ra, Ra.inv().apply(d)) + H.support(H.vb, H.rb, Rb.inv().apply(-d)) + (-0.004, 0.0004, -0.0004, 0.003)[k]
        add("quarter", np.r_[ORIGIN, qa, ORIGIN + d * t, qb])
    # coincident centres (the p0.v.x += 10 eps branch of discoverPortal): both bodies at one point.  ONE per family: with the origin ray 2e-15 long the direction of the
    # penetration is rounding's choice, the oracle's own answer jumps under a 1e-15 turn (tests/test_mpr_cases_cpu.py measures it), and such cases may be 2 % of the table
    for k in range(1):
        Ra, Rb = sR.from_rotvec(rng.normal(size=3)), sR.from_rotvec(rng.normal(size=3))
        add("coincident", H.centre_pose(Ra, Rb, np.array([1.0, 0, 0]), 0.0))
        q[-1][7:10] = q[-1][0:3] + Ra.apply(H.ca) - Rb.apply(H.cb)
    # the centre line through a vertex of each hull: the first support point lies ON the line v0 - origin (the origin-on-segment exit where the cross product vanishes)
    for k in range(8):
        ia, ib = int(rng.integers(len(H.va))), int(rng.integers(len(H.vb)))
        ua, ub = H.va[ia] - H.ca, H.vb[ib] - H.cb
        d = unit() if k % 2 else np.array([[1.0, 0, 0], [0.0, 0.6, 0.8], [0, 0, 1.0], POLE][k // 2])
        Ra = _rot_to(ua / np.linalg.norm(ua), d)
        Rb = _rot_to(ub / np.linalg.norm(ub), -d) if np.linalg.norm(ub) > 1e-12 else sR.identity()
        add("vertex_line", H.centre_pose(Ra, Rb, d, (-0.004, 0.0005, -0.0005, 0.004)[k % 4]))
    # separation at the margin +- 1e-9 and +- 1e-5: the `ccd_zero(dt) || dt < 0` exits decide
    for k, eps in enumerate((-1e-5, -1e-9, 1e-9, 1e-5)):
        add("margin_edge", H.face_pose(2 * k, k + 1, sR.from_rotvec(rng.normal(size=3)), rng.uniform(0.1, 3.0), MARGIN + eps, rng.uniform(-0.005, 0.005, size=2)))
    # the small hull wholly inside the large one
    for k in range(4):
        Ra, Rb = sR.from_rotvec(rng.normal(size=3) * 0.5), sR.from_rotvec(rng.normal(size=3))
        off = unit() * rng.uniform(0.002, 0.012)
        add("inside", H.centre_pose(Ra, Rb, np.array([1.0, 0, 0]), 0.0))
        q[-1][7:10] = q[-1][0:3] + Ra.apply(H.ca) - Rb.apply(H.cb) + off
    # random: as tests/test_gpu_selfcollision.py draws them -- B near a face / edge / corner of A, both turned at random; centre distances on both sides of touching
    while len(q) < N_CASES:
        Ra, Rb = sR.from_rotvec(rng.normal(size=3) * 0.5), sR.from_rotvec(rng.normal(size=3) * 0.9)
        add("random", H.centre_pose(Ra, Rb, unit(), rng.uniform(-0.02, 0.004)))
    assert len(q) == N_CASES
    v = np.random.default_rng(seed + 1000).normal(scale=0.3, size=(N_CASES, 12))
    return np.array(q), v, tuple(tags)


def batches():
    """the envs of a family's table, at most 64 per batch"""
    return [list(range(a, min(a + BATCH, N_CASES))) for a in range(0, N_CASES, BATCH)]


# ------------------------------------------------------------------ plain geometry
def world_hull(m, g, pos, quat):
    """(core vertices of geom g in the world, radius, centre in the world) with the geom's body at pos / quat (w, x, y, z)"""
    from uhc_amd.model.mjcf import quat_to_mat
    v, r, c = geom_hull(m, g)
    R = quat_to_mat(np.asarray(quat, dtype=np.float64) / np.linalg.norm(quat))
    return v @ R.T + pos, r, R @ c + pos


def _min_norm(P):
    """the point of least norm in the convex hull of at most five points, by trying every face of the simplex (Johnson's sub-algorithm, brute force) -> (point, kept rows)"""
    import itertools
    best, keep = None, None
    for r in range(1, min(len(P), 4) + 1):
        for idx in itertools.combinations(range(len(P)), r):
            S = P[list(idx)]
            if r == 1:
                w = np.array([1.0])
            else:
                E = (S[1:] - S[0]).T
                lam, *_ = np.linalg.lstsq(E, -S[0], rcond=None)
                w = np.r_[1 - lam.sum(), lam]
                if (w < -1e-14).any():
                    continue
            x = w @ S
            if best is None or x @ x < best @ best:
                best, keep = x, [i for i, wi in zip(idx, w) if wi > 0]
    return best, keep


def polytope_distance(A, B, iters=200):
    """Distance of conv(A) and conv(B) as a certified bracket (lo, hi): GJK on the Minkowski difference.  hi = |x| of a point x of conv(A) - conv(B); lo = the support
    bound x . s / |x| (every point p of the difference has p . x >= s . x, s the difference's support point along -x).  Whatever the inner solve's rounding, lo <= d <= hi."""
    x = A[0] - B[0]
    W = x[None]
    lo = 0.0
    for _ in range(iters):
        n2 = float(x @ x)
        if n2 < 1e-30:
            return 0.0, 0.0
        s = A[np.argmin(A @ x)] - B[np.argmax(B @ x)]
        lo = max(lo, float(s @ x) / np.sqrt(n2))
        if n2 - float(s @ x) <= 1e-13 * n2 or np.sqrt(n2) - lo < 1e-11:
            break
        x, keep = _min_norm(np.r_[W, s[None]])
        W = np.r_[W, s[None]][keep]
    return max(lo, 0.0), float(np.sqrt(x @ x))


def support_depth_bound(A, ra, B, rb, n, margin=MARGIN):
    """h(n) = max_a n.a - min_b n.b + margin over the INFLATED hulls: no penetration depth along n exceeds the Minkowski difference's extent there (long double)"""
    n = np.asarray(n, dtype=np.longdouble)
    return float((A.astype(np.longdouble) @ n).max() - (B.astype(np.longdouble) @ n).min() + np.longdouble(ra + rb) + np.longdouble(margin))


# ------------------------------------------------------------------ the oracle's answers, computed once
def perturbations(q):
    """tests/test_gpu_parity_200.py's six 1e-15 twins of a pose.  There the humanoid's joint angles are moved and its root is not; here the bodies' orientations are
    moved (every quaternion coordinate) and their positions are not: a position is what defines a case (coincident centres, a separation of margin +- 1e-9), and the
    ties the rule is about -- which vertex a support query picks -- hang on the orientations."""
    quats = np.concatenate([np.arange(7 * k + 3, 7 * k + 7) for k in range(q.shape[-1] // 7)])
    out = []
    for k in (1, 2, 3):
        for s in (1.0, -1.0):
            dp = np.zeros(q.shape[-1])
            dp[quats] = s * 1e-15 * np.cos(k * np.arange(len(quats)))
            out.append(dp)
    return out


def _oracle_rows(m, q, v, stepped):
    from oracle.physics import OracleSim
    ctrl = passive_ctrl(m)
    o = OracleSim(m, ctrl)
    out = []
    zero = np.zeros(max(int(m.nu), 1))
    for e in range(len(q)):
        o.set_state(q[e], v[e])
        if stepped:
            o.do_simulation(zero, zero)
        nc = o.geti("ncon")
        out.append(dict(ncon=nc, nefc=o.geti("nefc"), qacc=o.get("qacc").copy(), fail=o.geti("fail"), dist=o.get("con_dist")[:nc].copy(),
                        pos=o.get("con_pos").reshape(-1, 3)[:nc].copy(), normal=o.get("con_frame").reshape(-1, 9)[:nc, :3].copy()))
    return out


@functools.lru_cache(maxsize=None)
def family_reference(name, stepped=False):
    """The oracle on every case of the family: after set_state (the forward pass), or -- stepped -- after one control step from it with no actuation (what a queue consumer
    computes: the sticky path serves control steps only)."""
    q, v, _ = family_cases(name)
    return _oracle_rows(family_model(name), q, v, stepped)


@functools.lru_cache(maxsize=None)
def family_spread(name, stepped=False):
    """Per case: how far the oracle's qacc moves when the pose moves by 1e-15, and the twins' answers.  A case whose qacc moves by more than 1e-8 is a discontinuity of the
    contact model (a support query or a portal choice that ties to the last bit): tests/test_gpu_parity_200.py's rule."""
    q, v, _ = family_cases(name)
    m = family_model(name)
    ref = family_reference(name, stepped)
    spread, twins = np.zeros(len(q)), []
    for dp in perturbations(q):
        pq = q + dp
        rows = _oracle_rows(m, pq, v, stepped)
        twins.append(rows)
        for e, r in enumerate(rows):
            spread[e] = max(spread[e], np.abs(r["qacc"] - ref[e]["qacc"]).max()) if r["ncon"] == ref[e]["ncon"] else np.inf
    return spread, twins


SPREAD_BAR = 1e-8


# ------------------------------------------------------------------ scenes of more than two bodies
ROD = (0.4, 0.01, 0.01)


def rod_scene(n, joint):
    """n long thin rods (0.8 x 0.02 x 0.02 m): n - 2 of them side by side along x, 4 margins apart -- every pair's bounding spheres overlap, every pair's boxes are apart
    -- and two laid ACROSS the first few, a little tilted and half a millimetre deep, for a handful of real contacts.  joint: "free", or "slide" (each rod on one slide
    joint along z).  -> (model, qpos [nq], n (n - 1) / 2 pairs)"""
    from scipy.spatial.transform import Rotation as sR
    rng = np.random.default_rng(7 + n)
    pitch = 2 * ROD[1] + 4 * MARGIN
    pos, quat = [], []
    for k in range(n - 2):
        pos.append([0.0, pitch * k, HEIGHT])
        quat.append(quat_of(sR.from_rotvec(rng.normal(scale=0.0015, size=3))))
    # the two across: along y over the pack (so that their bounding spheres reach every rod), pitched by 0.05 rad about x so that only their low end, over rod 0, is
    # near: half a millimetre inside rod 0, 0.7 mm above rod 1 (within the margin), 1.9 mm above rod 2 (beyond it)
    th, yc = 0.05, ROD[0] - 0.02
    for k in range(2):
        pos.append([-0.2 + 0.4 * k, yc, HEIGHT + ROD[2] - 0.0005 + ROD[2] / np.cos(th) + np.tan(th) * yc])
        quat.append(quat_of(sR.from_rotvec(rng.normal(scale=0.001, size=3)) * sR.from_euler("x", th) * sR.from_euler("z", np.pi / 2)))
    j = "free" if joint == "free" else ("slide", (0.0, 0.0, 1.0))
    m = hull_scene_model([box(*ROD)] * n, [j] * n, pos=pos, quat=quat)
    return m, m.qpos0.copy()


SCENES = {  # name -> (bodies, joint, candidate pairs)
    "rods12": (12, "free", 66), "rods23": (23, "slide", 253), "rods24": (24, "slide", 276),
}
CAND_CAP = 256  # uhc_physics_impl.h: the candidates of one env that go through MPR; beyond it the env is handed on / flagged (UHC_WHY_CANDIDATES)


@functools.lru_cache(maxsize=None)
def multi_scene(name):
    """-> (model, qpos [n_env][nq], qvel [n_env][nv]) of a scene of more than two bodies; a few envs of one model, each with its own seeded pose"""
    from scipy.spatial.transform import Rotation as sR
    if name in SCENES:
        n, joint, _ = SCENES[name]
        m, q0 = rod_scene(n, joint)
        rng = np.random.default_rng(50 + n)
        q = np.tile(q0, (2, 1))
        if joint == "slide":
            q[1] += rng.normal(scale=1e-4, size=m.nq)
        v = rng.normal(scale=0.1, size=(2, m.nv))
        return m, q, v
    # 3 bodies (3 pairs: the last request of a round is served singly) and 4 bodies (6 pairs): hulls of different families around one point, all overlapping or near
    hulls = {"three": [box(0.1, 0.1, 0.1), ball(50, 0.08), tetra(0.1)], "four": [box(0.1, 0.1, 0.1), ball(50, 0.08), tetra(0.1), ball(64, 0.07)]}[name]
    n = len(hulls)
    m = hull_scene_model(hulls, ["free"] * n)
    rng = np.random.default_rng(70 + n)
    n_env = 16
    q = np.zeros((n_env, 7 * n))
    dirs = np.array([[0.0, 0, 0], [1.0, 0.2, 0.1], [-0.3, 1.0, 0.2], [0.1, -0.4, 1.0]])[:n]
    for e in range(n_env):
        spread = rng.uniform(0.03, 0.16)  # from deep overlaps to most pairs apart
        for k in range(n):
            q[e, 7 * k:7 * k + 3] = np.array([0.0, 0.0, HEIGHT]) + spread * dirs[k] / max(np.linalg.norm(dirs[k]), 1.0) + rng.normal(scale=0.01, size=3)
            q[e, 7 * k + 3:7 * k + 7] = quat_of(sR.from_rotvec(rng.normal(size=3)))
    v = rng.normal(scale=0.3, size=(n_env, 6 * n))
    return m, q, v


@functools.lru_cache(maxsize=None)
def multi_reference(name, stepped=False):
    m, q, v = multi_scene(name)
    return _oracle_rows(m, q, v, stepped)


# ------------------------------------------------------------------ "first maximum wins" across the trips of a large hull
DRUM_SIDES = 40


def drum(r=0.1, h=0.03, n=DRUM_SIDES):
    """a prism over a regular n-gon: 2 n = 80 vertices, two flat faces of n vertices each"""
    a = 2 * np.pi * (np.arange(n) + 0.25) / n
    ring = np.c_[r * np.cos(a), r * np.sin(a)]
    return np.r_[np.c_[ring, np.full(n, h)], np.c_[ring, np.full(n, -h)]]


@functools.lru_cache(maxsize=None)
def drum_scene():
    """The drum flat on the small box, 2 mm deep, the box under the drum's axis and yawed: the centre line is z exactly, the drum's matrix the identity and the box's a
    turn about z (zeros and a one in its z row and column, exactly), so the first support query -- along the centre line -- finds the drum's 40 bottom vertices and the
    box's four top corners at ONE projection each, to the last bit, on the host and on the device.  The bottom vertices lie in both trips of the 80-vertex scan; the
    first of them wins.  Every later query runs along a direction of the portal, in general position.  -> (model, qpos [4][14], qvel [4][12])"""
    m = hull_scene_model([drum(), box(0.06, 0.06, 0.06)], ["free", "free"])
    yaws = (0.3, 1.1, 2.0, 0.7)
    q = np.array([np.r_[ORIGIN, 1.0, 0, 0, 0, ORIGIN - [0.0, 0.0, 0.03 + 0.06 - 0.002], np.cos(y / 2), 0, 0, np.sin(y / 2)] for y in yaws])
    v = np.random.default_rng(91).normal(scale=0.3, size=(len(q), 12))
    return m, q, v


@functools.lru_cache(maxsize=None)
def drum_reference(stepped=False):
    m, q, v = drum_scene()
    return _oracle_rows(m, q, v, stepped)
