"""The sweep voxel map (csrc/voxel.hip, include/gsraster.h gsr_voxel_sweep) restated on the host: Python integers for the
sums, float64 after them in the operation order of the header, numpy.linalg.eigh for the axes.  Also the cases the
tests share and the bars, derived here by counting roundings.

The integer part (cells, keys, offsets, sums, statuses, counts, seed order) is EXACT: the device must give the same
bits.  The mean, the covariance and the colour are float64 expressions of exact integers, evaluated in one written
order without contraction on both sides, every operation (/, +, -, *) correctly rounded on both sides: the float64
values are the same bits, so the narrowed f32 outputs are too.  XYZ_ULPS = 1 is the issue's bar for xyz and rgbs;
the expected share of differing elements is 0.

Bars (u = 2^-24, the unit roundoff of f32; lam_max the largest clamped eigenvalue of the voxel; all per element):

covs.  The device forms V diag(lam) V^T in float64 from its own Jacobi axes and narrows once.  The float64 parts
(twelve fixed Jacobi sweeps against eigh, three products and two sums per element) are below 100 * 2^-53 lam_max
relative to the clamped covariance, because V diag(max(lam, floor)) V^T is a Lipschitz-1 matrix function of C (no gap
enters).  One narrowing: u lam_max.  COV_BAR = (1 + 2^-20) u lam_max.

Sigma rebuilt from (scaling_raw, rotation) by ref64.cov3d in float64.
  scaling_raw = log sqrt(lam sf), narrowed once: absolute error u |raw|.  s = exp(raw) has relative error u |raw|,
    s^2 twice that: 2 L u lam_max per element, L = the largest |log sqrt(lam sf)| of the voxel, taken from the
    REFERENCE eigenvalues.
  rotation: four components of magnitude <= 1, each narrowed once: |dq_i| <= u / 2, so |dq|_2 <= u.  The rotation
    matrix is a homogeneous quadratic of q, each element a sum of products q_a q_b with total weight <= 4 (off-diagonal:
    2 q_a q_b +- 2 q_c q_d; diagonal: 1 - 2 (..) with the unnormalised q of cov3d), so |dR_ij| <= 4 |q|_inf |dq|_inf * 2
    <= 4 u.  Sigma = R S^2 R^T: |dSigma_ij| <= 2 * 3 * |dR|_max lam_max <= 24 u lam_max in the worst alignment; the
    unnormalised |q|^2 = 1 + O(u) adds 2 u lam_max.
  float64 parts as above.
  RECON_BAR = (26 + 2 L + 2^-20) u lam_max sf.  (The issue's estimate, 16 u lam_max, is this with the typical instead
  of the worst alignment of the quaternion's error; the measured worst ratio is recorded in DESIGN.md section 2.)

normal.  Device Jacobi and eigh are both backward stable in float64: each returns the exact axes of C + E with
|E| <= 64 * 2^-53 lam_max (three-by-three, twelve sweeps of three rotations, a few flops each).  The axis of the
smallest eigenvalue moves by at most |E| / gap, gap = lam_mid - lam_min UNCLAMPED (Davis-Kahan), for each of the two,
then the device narrows each component once (u / 2).  NORMAL_BAR(lam_max, gap) = u / 2 + 2 * 64 * 2^-53 lam_max / gap,
on every component after aligning the sign.
"""
import numpy as np

Q = 1 << 20
ACCUMULATED, SEEDED, OUT, FULL = range(4)
U = 2.0 ** -24
XYZ_ULPS = 1


def cov_bar(lam_max):
    return (1.0 + 2.0 ** -20) * U * lam_max


def recon_bar(lam_max, L, scale_factor=1.0):
    return (26.0 + 2.0 * L + 2.0 ** -20) * U * lam_max * scale_factor


def normal_bar(lam_max, gap):
    return 0.5 * U + 128.0 * 2.0 ** -53 * lam_max / gap


def cells(points, grid):
    """points [n,3] f32 -> (ok [n] bool, c [n,3] int64, q [n,3] int64, key [n] int64 with -1 for OUT)."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    g = float(np.float32(grid))
    with np.errstate(invalid="ignore", over="ignore"):
        t = p.astype(np.float64) / g
        f = np.floor(t)
        ok = (np.isfinite(t) & (np.abs(f) < Q)).all(1)
        f = np.where(ok[:, None], f, 0.0)
        t = np.where(ok[:, None], t, 0.0)
        c = f.astype(np.int64)
        q = np.minimum(Q - 1, np.floor((t - f) * float(Q)).astype(np.int64))
    key = ((c[:, 0] + Q) << 42) | ((c[:, 1] + Q) << 21) | (c[:, 2] + Q)
    return ok, c, q, np.where(ok, key, -1)


def key_cell(key):
    key = int(key)
    return [((key >> (42 - 21 * k)) & 0x1FFFFF) - Q for k in range(3)]


def colour_units(colors):
    s = np.asarray(colors, dtype=np.float32).astype(np.float64) * 256.0
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(np.where(np.isnan(s), 0.0, s)), 0.0, 65535.0)
    return r.astype(np.int64)


class Seed:
    """One matured voxel in float64 (f32 where noted)."""

    def __init__(self, key, count, s1, s2, sc, grid, min_sigma, scale_factor, has_colour):
        g, n = float(np.float32(grid)), float(count)
        a = [float(s1[k]) / n for k in range(3)]
        cell = key_cell(key)
        self.key, self.count = int(key), int(count)
        self.mean = np.array([(float(cell[k]) + (a[k] + 0.5) / float(Q)) * g for k in range(3)])
        unit = g / float(Q)
        unit2 = unit * unit
        C = np.zeros((3, 3))
        w = 0
        for r in range(3):
            for c in range(r, 3):
                C[r, c] = C[c, r] = (float(s2[w]) / n - a[r] * a[c]) * unit2
                w += 1
        self.C = C
        lam, V = np.linalg.eigh(C)
        self.lam_raw = lam[::-1].copy()                       # descending, unclamped
        V = V[:, ::-1].copy()
        floor = float(np.float32(min_sigma)) ** 2
        self.lam = np.maximum(self.lam_raw, floor)
        if np.linalg.det(V) < 0:
            V[:, 2] = -V[:, 2]
        self.V = V
        self.cov = (V * self.lam) @ V.T                        # the clamped covariance
        self.normal = V[:, 2]
        self.scaling_raw = np.log(np.sqrt(self.lam * float(np.float32(scale_factor))))
        self.rgb = np.array([float(sc[k]) / (256.0 * n) for k in range(3)]) if has_colour else None
        self.xyz32 = self.mean.astype(np.float32)
        self.rgb32 = None if self.rgb is None else self.rgb.astype(np.float32)


class RefMap:
    """The table as a dict: key -> [closed, count, s1[3], s2[6], sc[3]] of Python integers (unbounded, no FULL)."""

    def __init__(self, grid, min_points, min_sigma):
        self.grid, self.min_points, self.min_sigma = grid, int(min_points), min_sigma
        self.vox = {}

    def sweep(self, points, colors=None, scale_factor=1.0):
        ok, _, q, key = cells(points, self.grid)
        n = len(key)
        cu = None if colors is None else colour_units(colors)
        status = np.full(n, OUT, dtype=np.uint8)
        first = {}
        closed_before = {k: v[0] for k, v in self.vox.items()}
        for i in range(n):
            if not ok[i]:
                continue
            k = int(key[i])
            if closed_before.get(k, 0):
                status[i] = SEEDED
                continue
            status[i] = ACCUMULATED
            v = self.vox.setdefault(k, [0, 0, [0, 0, 0], [0] * 6, [0, 0, 0]])
            first.setdefault(k, i)
            x, y, z = (int(t) for t in q[i])
            v[1] += 1
            for j, t in enumerate((x, y, z)):
                v[2][j] += t
            for j, t in enumerate((x * x, x * y, x * z, y * y, y * z, z * z)):
                v[3][j] += t
            if cu is not None:
                for j in range(3):
                    v[4][j] += int(cu[i, j])
        seeds = []
        for k in sorted(first, key=first.get):                 # the order of first appearance in the call
            v = self.vox[k]
            if v[1] >= self.min_points:
                v[0] = 1
                seeds.append(Seed(k, v[1], v[2], v[3], v[4], self.grid, self.min_sigma, scale_factor, cu is not None))
        counts = (int((status == ACCUMULATED).sum()), int((status == SEEDED).sum()), int((status == OUT).sum()), 0,
                  len(seeds), len(self.vox))
        return dict(status=status, point_keys=key.astype(np.int64), counts=counts, seeds=seeds)

    def state(self):
        """As SweepVoxelMap.state(): sorted by key, int64 arrays."""
        ks = sorted(self.vox)
        a = lambda f, w: np.array([f(self.vox[k]) for k in ks], dtype=np.int64).reshape(len(ks), *w)  # noqa: E731
        return dict(keys=np.array(ks, dtype=np.int64), closed=a(lambda v: v[0], ()), count=a(lambda v: v[1], ()),
                    s1=a(lambda v: v[2], (3,)), s2=a(lambda v: v[3], (6,)), sc=a(lambda v: v[4], (3,)))


# ---- the cases ---------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
GRIDS = (0.25, 0.2)       # exact and not exact in binary


def random_cloud(n, seed=0, extent=0.6):
    """n points in a cube around the origin (negative coordinates included), colours in and slightly out of 0..255."""
    r = np.random.RandomState(1000 + 7 * n + seed)
    pts = r.uniform(-extent, extent, (n, 3)).astype(np.float32)
    cols = r.uniform(-5.0, 260.0, (n, 3)).astype(np.float32)
    return pts, cols


def one_voxel(n=1025, grid=0.25, seed=3):
    """All n points inside the cell (-2, 0, 1): every thread adds to one slot."""
    r = np.random.RandomState(seed)
    g = float(np.float32(grid))
    pts = ((np.array([-2.0, 0.0, 1.0]) + r.uniform(0.01, 0.99, (n, 3))) * g).astype(np.float32)
    cols = r.uniform(0.0, 255.0, (n, 3)).astype(np.float32)
    return pts, cols


def distinct_voxels(n=1025, grid=0.25):
    """Point i in its own cell (i - n // 2, i % 7 - 3, -(i % 5)), at the cell's centre."""
    g = float(np.float32(grid))
    i = np.arange(n)
    c = np.stack([i - n // 2, i % 7 - 3, -(i % 5)], 1).astype(np.float64)
    pts = ((c + 0.5) * g).astype(np.float32)
    cols = np.stack([i % 256, (3 * i) % 256, (7 * i) % 256], 1).astype(np.float32)
    return pts, cols


def boundary_points(grid):
    """The points whose cell or code the definition decides by a hair, and the non-finite rows."""
    g = np.float32(grid)
    edge = np.float32(float(Q) * float(g))
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    big = np.float32(3e38)
    x = [np.float32(-1e-9), np.float32(-1e-30), np.float32(0.25), np.nextafter(np.float32(0.25), np.float32(0)),
         np.float32(0.0), np.float32(-0.0),
         np.nextafter(edge, np.float32(0)), edge, np.nextafter(edge, inf),
         np.nextafter(-edge, np.float32(0)), -edge, np.nextafter(-edge, -inf), big, -big, nan, inf, -inf,
         np.float32(1e-45), np.float32(-1e-45)]
    rows = []
    for v in x:
        rows += [[v, 0.1, 0.1], [0.1, v, -0.1], [-0.1, 0.1, v]]
    rows += [[nan, nan, nan], [inf, -inf, 0.0]]
    pts = np.array(rows, dtype=np.float32)
    cols = np.tile(np.array([[0.0, 127.5, 255.0], [nan, inf, -inf], [255.998, 256.0, 1e9], [0.001953125, 0.5, -0.0]],
                            dtype=np.float32), (len(pts) // 4 + 1, 1))[:len(pts)]
    return pts, cols


PLANES = (  # (unit normal, point on the plane, in-plane extent in metres)
    ((0.0, 0.0, 1.0), (0.03, -0.02, 0.113), 2.0),
    ((1.0, 0.0, 0.0), (-0.531, 0.1, 0.2), 2.0),
    ((0.6, 0.0, 0.8), (0.2, 0.3, -0.4), 2.0),
    ((0.48, 0.6, 0.64), (-0.3, 0.2, 0.1), 2.0),
)
PLANE_POINTS, PLANE_SIGMA, PLANE_MIN_POINTS, PLANE_MIN_SIGMA = 1500, 0.004, 10, 0.001


def plane_scene(which, seed=15):
    """1 500 points on a square patch of PLANES[which] with 4 mm of noise along the normal; colours by position."""
    nrm, at, ext = PLANES[which]
    nrm = np.array(nrm) / np.linalg.norm(nrm)
    a = np.cross(nrm, [0.0, 1.0, 0.0] if abs(nrm[1]) < 0.9 else [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    r = np.random.RandomState(seed + which)
    uv = r.uniform(-ext / 2, ext / 2, (PLANE_POINTS, 2))
    pts = np.array(at) + uv[:, :1] * a + uv[:, 1:] * b + r.normal(0.0, PLANE_SIGMA, (PLANE_POINTS, 1)) * nrm
    cols = np.clip(127.0 + 60.0 * pts, 0.0, 255.0)
    return pts.astype(np.float32), cols.astype(np.float32), nrm


def collinear_voxel(grid=0.25, n=40):
    """n points on a line inside one cell: two eigenvalues are (nearly) zero and the min_sigma clamp decides them."""
    g = float(np.float32(grid))
    s = np.linspace(0.1, 0.9, n)[:, None]
    pts = (np.array([3.0, -1.0, 2.0]) + s * np.array([1.0, 0.5, 0.25]) + np.array([0.0, 0.2, 0.3])) * g
    cols = np.full((n, 3), 100.0)
    return pts.astype(np.float32), cols.astype(np.float32)


def ulp_distance(a, b):
    """Element-wise distance in f32 ulps between two f32 arrays of finite values."""
    def ordered(x):
        i = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))
