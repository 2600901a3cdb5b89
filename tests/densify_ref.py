"""Host restatement of adaptive density control (csrc/densify.hip), written from the definitions in include/gsraster.h:
Philox4x32-10 in integer numpy, everything else with the dtype as a parameter.  float64 is the truth; float32 -- the same
operations in the same order as the kernels, nothing contracted -- is the yardstick e_ref = |float32 - float64|.

Bars.  Every continuous output is held to max(2 e_ref, K 2^-23 magnitude); K counts roundings in ulps (2^-23 relative):
a correctly rounded +, *, /, sqrt is 0.5, the device's logf and expf count 3 and sinf / cosf 4 (OpenCL full profile, as
tests/test_gpu_growth_ref64.py argues for the same library).

accumulate: n = sqrt(gx gx + gy gy): two products 0.5 each and the sum 0.5 leave n^2 within 1, the root halves that
  and adds 0.5: 1 ulp.  Each further view adds n (1 ulp of it) with one rounding of the partial sum (0.5 ulp of at most
  the total S): after any number v of views the error is at most (1 + 0.5 (v - 1)) S <= K_SUM S with K_SUM = 2 for the
  three views of the tests.  (Products that fall into the subnormals -- |g| ~ 1e-20 -- lose relative precision in
  float32 on any machine; there the 2 e_ref arm of the bar speaks.)  views and max_radius are exact.

normal z = r cos(t) (sin likewise): u is exact.  logf 3 -> -2 log u exact scaling -> sqrt: 3 / 2 + 0.5 = 2 ulp of r.
  t = fl(2 pi) u: the constant is 0.23 ulp off, the product 0.5: |dt| <= 2 pi 2^-23.  cosf: 4 ulp of |cos| <= 1, plus
  |dt| |sin| <= 2 pi ulp of 1.  The product r cos: (2 + 0.5) |z| <= 2.5 r.  Together |dz| <= (4 + 2 pi + 2.5) r <=
  K_Z r with K_Z = 13 (12.78 rounded up), r <= sqrt(48 ln 2) = 5.77 since u >= 2^-24.

split child xyz_c = x + R (sigma * z):
  v_j = sigma_j z_j: expf 3, product 0.5, z's K_Z r: |dv_j| <= (13 + 3.5) sigma_j r = 16.5 V, V = max_j sigma_j max(r1, r2).
  R: |q|^2 = four products and three sums of positive terms: 2 ulp; sqrt: 1.5; 1 / n: 2; q_k / n: 2.5 per component.
    off-diagonal 2 (ab -+ cd): each product 5.5 ulp of itself, |ab| + |cd| <= 1/2, the difference 0.5 of <= 1/2:
    2 (5.5 / 2 + 0.25) = 6.  diagonal 1 - 2 (a^2 + b^2): the sum 6 ulp of <= 1, doubled 12, the subtraction 0.5: 12.5.
    So |dR_kj| <= 12.5 (a zero quaternion gives the exact identity in both precisions).
  d_k = sum_j R_kj v_j: sum_j |dR_kj| |v_j| <= 3 * 12.5 V; sum_j |R_kj| |dv_j| <= sqrt(3) 16.5 V; three products and two sums
    1.5 sum_j |R_kj v_j| <= 1.5 sqrt(3) V: 37.5 + 28.6 + 2.6 = 68.7 V.
  x + d: 0.5 (|x_k| + sqrt(3) V).  Together (69.6 V + 0.5 |x_k|) <= K_XYZ V + 0.5 |x_k| with K_XYZ = 70.
scaling_c = s - 0.47000363f, the float32 constant being the definition: one rounding, 0.5 ulp of max(|s|, 0.47): K_SCALE = 1.
"""
import numpy as np

K_SUM, K_Z, K_XYZ, K_SCALE = 2.0, 13.0, 70.0, 1.0
ULP = 2.0 ** -23
LN_1_6 = np.float32(0.47000363)
TWO_PI_F32 = np.float32(6.2831855)
R_MAX = float(np.sqrt(48.0 * np.log(2.0)))   # u >= 2^-24

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """counter [..., 4], key (k0, k1): unsigned 32-bit words -> [..., 4] uint32 (Salmon et al., SC'11), integers only."""
    c = [np.asarray(counter)[..., k].astype(np.uint64) for k in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]     # < 2^64: exact
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def uniforms(o):
    """u = ((o >> 9) + 0.5) 2^-23 as float32: exact (2n + 1 < 2^24), strictly inside (0, 1)"""
    n = (np.asarray(o, dtype=np.uint32) >> np.uint32(9)).astype(np.float32)
    u = (n + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert np.array_equal(u.astype(np.float64), (n.astype(np.float64) + 0.5) * 2.0 ** -23)
    return u


def normals(seed, rows, child, dtype):
    """z [n, 3] of child `child` of the rows `rows`, and the radii r [n, 2] that bound them"""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1)
    ctr = np.zeros((rows.size, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1] = rows, child
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    u = uniforms(philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))).astype(dtype)
    two_pi = TWO_PI_F32 if dtype == np.float32 else dtype(2.0 * np.pi)
    r1, t1 = np.sqrt(dtype(-2.0) * np.log(u[:, 0])), two_pi * u[:, 1]
    r2, t2 = np.sqrt(dtype(-2.0) * np.log(u[:, 2])), two_pi * u[:, 3]
    z = np.stack([r1 * np.cos(t1), r1 * np.sin(t1), r2 * np.cos(t2)], 1)
    assert z.dtype == dtype
    return z, np.stack([r1, r2], 1)


def accumulate(stats, radii, grad, dtype):
    """one view: stats [P,3] (dtype) -> new stats; radii [P] int, grad [P,3] float32"""
    stats = np.array(stats, dtype=dtype)
    gx, gy = grad[:, 0].astype(dtype), grad[:, 1].astype(dtype)
    with np.errstate(all="ignore"):
        n = np.sqrt(gx * gx + gy * gy)
        # "a finite n" is the float32 norm's finiteness in every precision: components near 2^64 overflow there
        n32 = np.sqrt(grad[:, 0] * grad[:, 0] + grad[:, 1] * grad[:, 1])
    hit = (np.asarray(radii) > 0) & np.isfinite(n32)
    stats[hit, 0] = stats[hit, 0] + n[hit]
    stats[hit, 1] = stats[hit, 1] + dtype(1)
    stats[hit, 2] = np.maximum(stats[hit, 2], np.asarray(radii)[hit].astype(dtype))
    return stats


def size_margin(scaling_raw, size_threshold):
    """smallest relative distance of a finite row's max exp(s) from the threshold (the tests assert it exceeds 1e-5, so
    that the device's expf -- 3 ulp -- decides every row as the float64 exp does)"""
    s = np.asarray(scaling_raw, dtype=np.float64)
    s = s[np.isfinite(s).all(1)]
    if s.size == 0 or not np.isfinite(size_threshold) or size_threshold <= 0:
        return np.inf
    return float(np.abs(np.exp(s.max(1)) / float(size_threshold) - 1.0).min())


def mark(stats, scaling_raw, grad_threshold, size_threshold, max_new=-1):
    """The float32 restatement of gsr_densify_mark: (kinds [P] uint8, offsets [P+1] int32, counts [3])."""
    stats = np.asarray(stats, dtype=np.float32)
    s = np.asarray(scaling_raw, dtype=np.float32)
    P = stats.shape[0]
    with np.errstate(all="ignore"):
        avg = np.where(stats[:, 1] > 0, stats[:, 0] / np.where(stats[:, 1] > 0, stats[:, 1], np.float32(1)),
                       np.float32(0)).astype(np.float32)
        cand = (avg >= np.float32(grad_threshold)) & np.isfinite(s).all(1)
        big = np.exp(s.astype(np.float64)).max(1) > float(np.float32(size_threshold))
    excl = np.concatenate([[0], np.cumsum(cand)]).astype(np.int64)
    cap = np.iinfo(np.int32).max if max_new < 0 else int(max_new)
    cand = cand & (excl[:P] < cap)
    kinds = np.where(cand, np.where(big, 2, 1), 0).astype(np.uint8)
    offsets = np.minimum(excl, cap).astype(np.int32)
    return kinds, offsets, [int(offsets[P]), int((kinds == 1).sum()), int((kinds == 2).sum())]


def rotation_matrix(q, dtype):
    """R [n,3,3] of q [n,4] (w, x, y, z) normalised as gsr_activate does: q / max(|q|, 1e-12)"""
    q = q.astype(dtype)
    nrm = np.maximum(np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]),
                     dtype(np.float32(1e-12)))
    inv = dtype(1) / nrm
    w, x, y, z = (q[:, k] * inv for k in range(4))
    one, two = dtype(1), dtype(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                  two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                  two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], 1)
    assert R.dtype == dtype
    return R.reshape(-1, 3, 3)


def split_children(xyz, scaling_raw, rotation_raw, rows, seed, dtype):
    """(xyz of child 0 [n,3], of child 1 [n,3], scaling of both [n,3], V [n] = max_k sigma_k max(r1, r2)) of the rows"""
    rows = np.asarray(rows).reshape(-1)
    x, s = xyz[rows].astype(dtype), scaling_raw[rows].astype(dtype)
    sigma = np.exp(s)
    R = rotation_matrix(rotation_raw[rows], dtype)
    out, rmax = [], np.zeros(rows.size)
    for c in (0, 1):
        z, r = normals(seed, rows, c, dtype)
        v = sigma * z
        d = (R[:, :, 0] * v[:, 0:1] + R[:, :, 1] * v[:, 1:2]) + R[:, :, 2] * v[:, 2:3]
        out.append(x + d)
        rmax = np.maximum(rmax, r.max(1).astype(np.float64))
    sc = s - LN_1_6.astype(dtype)
    assert out[0].dtype == dtype and sc.dtype == dtype
    return out[0], out[1], sc, sigma.max(1).astype(np.float64) * rmax


def xyz_bar(e_ref, V, x):
    return np.maximum(2.0 * e_ref, ULP * (K_XYZ * V[:, None] + 0.5 * np.abs(x)))


def scale_bar(e_ref, s):
    return np.maximum(2.0 * e_ref, ULP * K_SCALE * np.maximum(np.abs(s), float(LN_1_6)))


def apply(leaves, kinds, offsets, seed, dtype=np.float32, moments=None, stats=None):
    """The in-place layout of gsr_densify_apply on host copies.  leaves: six [P, ...] float32 arrays in the order xyz,
    features_dc, features_rest, scaling, rotation, opacity.  Returns (six [P + n_new, ...] arrays -- xyz and scaling
    in `dtype`, the copied ones as they are --, moments likewise or None, stats or None)."""
    kinds, offsets = np.asarray(kinds), np.asarray(offsets)
    P, n_new = kinds.size, int(offsets[-1])
    ext = lambda a, dt: np.concatenate([a.astype(dt), np.zeros((n_new,) + a.shape[1:], dt)], 0)  # noqa: E731
    dts = [dtype, np.float32, np.float32, dtype, np.float32, np.float32]
    out = [ext(a, dt) for a, dt in zip(leaves, dts)]
    marked = np.nonzero(kinds)[0]
    dst = P + offsets[marked]
    for a in out:
        a[dst] = a[marked]
    sp = np.nonzero(kinds == 2)[0]
    dsp = P + offsets[sp]
    c0, c1, sc, _ = split_children(leaves[0], leaves[3], leaves[4], sp, seed, dtype)
    out[0][sp], out[0][dsp], out[3][sp], out[3][dsp] = c0, c1, sc, sc
    if moments is not None:
        moments = [ext(a, np.float32) for a in moments]
        for a in moments:
            a[dst] = 0
            a[sp] = 0
    if stats is not None:
        stats = ext(stats, np.float32)
        stats[dst] = 0
        stats[sp] = 0
    return out, moments, stats
