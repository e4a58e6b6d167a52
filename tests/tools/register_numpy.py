"""The registration cost of include/met2_hip.h (met2_register_cost), restated in numpy: the sampling rule is resample_numpy's order 1 -- the
coordinates, the inside test, the floors and the tap indices in fp64, which are the contract --, the weights, the tap sums and every sum of
the three measures in `dtype` (np.longdouble: the reference the device is held against), the variances by two passes about the mean, so
nothing cancels.  prepare has the signature of register.prepare and serves as register's cost_fn; FILTERS = (smooth, resample) are the two
filters of register.pyramid on the CPU (scipy's gaussian_filter, which gaussian_smooth reproduces, and resample_numpy's order 1), so the
whole search runs without a device.  Also the phantom and the cases the host and the device tests share."""
import numpy as np

import resample_numpy as rn

LEASTSQ_WORST = 1.0e300
KINDS = ("corratio", "normcorr", "leastsq")


def worst(kind):
    return LEASTSQ_WORST if kind == "leastsq" else 1.0


def sample(moving, A, shape, dtype=np.longdouble):
    """-> (y [shape] in dtype, inside [shape] bool): the moving volume at the fixed voxels of candidate A [3, 4], the header's order 1"""
    y, ins = rn.resample(np.asarray(moving, dtype=np.float64), A, tuple(shape), order=1, cval=0.0, dtype=dtype, return_inside=True)
    return y, ins != 0


def cost_of_sample(fixed, fixed_bin, moving, y, ins, kind, n_bins, min_overlap, dtype=np.longdouble):
    """-> (n_inside, cost) from the sample of one candidate"""
    dtype = np.dtype(dtype).type
    fixed_bin = np.asarray(fixed_bin)
    included = (fixed_bin >= 0) & (fixed_bin < n_bins)
    use = included & ins
    n = int(use.sum())
    if n == 0 or float(n) < float(min_overlap) * float(included.sum()):
        return n, worst(kind)
    y = y[use]

    def central(v):                                                # n times the variance, two passes
        return ((v - v.sum() / dtype(n)) ** 2).sum()

    def tiny(vol):                                                 # the header's zero-variance rule
        m = float(np.abs(np.asarray(vol, dtype=np.float64)).max())
        return n * 1e-24 * m * m

    if kind == "leastsq":
        return n, float(((np.asarray(fixed, dtype=dtype)[use] - y) ** 2).sum() / dtype(n))
    vy = central(y)
    if not vy > tiny(moving):
        return n, 1.0
    if kind == "corratio":
        b = fixed_bin[use]
        within = dtype(0)
        for q in np.unique(b):
            sel = y[b == q]
            within = within + ((sel - sel.sum() / dtype(sel.size)) ** 2).sum()
        return n, float(min(within / vy, dtype(1)))
    x = np.asarray(fixed, dtype=dtype)[use]
    vx = central(x)
    if not vx > tiny(fixed):
        return n, 1.0
    c = ((x - x.sum() / dtype(n)) * (y - y.sum() / dtype(n))).sum()
    return n, float(max(dtype(1) - min(c * c / (vx * vy), dtype(1)), dtype(0)))


def cost_one(fixed, fixed_bin, moving, A, kind, n_bins, min_overlap, dtype=np.longdouble):
    """-> (n_inside, cost) of one candidate A [3, 4]"""
    y, ins = sample(moving, A, np.shape(fixed_bin), dtype)
    return cost_of_sample(fixed, fixed_bin, moving, y, ins, kind, n_bins, min_overlap, dtype)


def prepare(fixed, fixed_bin, moving, kind="corratio", n_bins=64, min_overlap=0.25, dtype=np.longdouble):
    """-> f(A_batch [K, 3, 4]) -> (n_inside [K] int64, cost [K] float64)"""
    fixed, fixed_bin, moving = np.asarray(fixed, dtype=np.float64), np.asarray(fixed_bin), np.asarray(moving, dtype=np.float64)

    def evaluate(A_batch):
        A = np.asarray(A_batch, dtype=np.float64)
        A = A[None] if A.ndim == 2 else A
        out = [cost_one(fixed, fixed_bin, moving, a, kind, n_bins, min_overlap, dtype) for a in A]
        return np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out], dtype=np.float64)

    return evaluate


def prepare_fp64(fixed, fixed_bin, moving, kind="corratio", n_bins=64, min_overlap=0.25):
    """the same in fp64: several times faster, for the searches of the host tests (their bounds are millimetres, not roundings)"""
    return prepare(fixed, fixed_bin, moving, kind, n_bins, min_overlap, dtype=np.float64)


def smooth(vol, sigma):
    from scipy import ndimage
    return ndimage.gaussian_filter(np.asarray(vol, dtype=np.float64), float(sigma), mode="reflect", truncate=4.0)


def resample(vol, A, shape):
    return rn.resample(np.asarray(vol, dtype=np.float64), A, shape, order=1, cval=0.0)


FILTERS = (smooth, resample)


# ---------------------------------------------------------------- the phantom of the end-to-end tests

PHANTOM_SHAPE = (20, 18, 16)
PHANTOM_MM = 2.0
# centre (voxels), semi-axes (voxels), intensity: a head-like body and a few blobs, no symmetry
ELLIPSOIDS = (((9.5, 8.5, 7.5), (8.0, 7.0, 6.0), 0.5), ((7.0, 7.5, 8.5), (3.0, 2.5, 3.5), 0.3), ((12.5, 10.5, 6.5), (2.5, 3.5, 2.0), -0.25),
              ((10.0, 5.0, 9.5), (2.0, 1.5, 2.5), 0.45), ((6.0, 11.0, 5.0), (1.5, 2.0, 1.5), -0.4))


def phantom_affine():
    return np.array([[PHANTOM_MM, 0, 0, -19.0], [0, PHANTOM_MM, 0, -17.0], [0, 0, PHANTOM_MM, -15.0], [0, 0, 0, 1.0]])


def phantom_at(world_pts):
    """the phantom's intensity at world points [..., 3] mm: the ellipsoids with soft edges (a logistic of half a voxel), summed"""
    inv = np.linalg.inv(phantom_affine())
    c = world_pts @ inv[:3, :3].T + inv[:3, 3]
    out = np.zeros(c.shape[:-1])
    for centre, axes, value in ELLIPSOIDS:
        r = np.sqrt((((c - np.array(centre)) / np.array(axes)) ** 2).sum(axis=-1))
        out += value / (1.0 + np.exp((r - 1.0) * min(axes) / 0.5))
    return out


def grid_world(shape, affine):
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return np.stack([i, j, k], axis=-1) @ np.asarray(affine)[:3, :3].T + np.asarray(affine)[:3, 3]


def remap(v):
    """a non-monotonic map of the intensities: another contrast of the same anatomy"""
    return 0.2 + (v - 0.45) ** 2 * 3.0 + 0.15 * np.sin(9.0 * v)


def phantom_pair(true_world, remapped):
    """fixed = the phantom on its grid; moving = an image whose world mm relate to the fixed image's by true_world (fixed -> moving), on a grid
    of its own (22 x 20 x 18 at 2 mm, shifted), analytically evaluated, so no interpolation error enters the truth
    -> (fixed, fixed_affine, moving, moving_affine, mask)"""
    fa = phantom_affine()
    fixed = phantom_at(grid_world(PHANTOM_SHAPE, fa))
    ma = np.array([[PHANTOM_MM, 0, 0, -21.5], [0, PHANTOM_MM, 0, -18.5], [0, 0, PHANTOM_MM, -17.5], [0, 0, 0, 1.0]])
    inv = np.linalg.inv(true_world)
    pts = grid_world((22, 20, 18), ma) @ inv[:3, :3].T + inv[:3, 3]     # moving-world -> fixed-world, where the phantom is defined
    moving = phantom_at(pts)
    return fixed, fa, (remap(moving) if remapped else moving), ma, fixed > 0.05


def mean_displacement(world_a, world_b, mask, affine):
    """the mean distance in mm, over the mask's voxels, between where the two transforms send them"""
    pts = grid_world(mask.shape, affine)[mask != 0]
    d = pts @ (np.asarray(world_a)[:3, :3] - np.asarray(world_b)[:3, :3]).T + (np.asarray(world_a)[:3, 3] - np.asarray(world_b)[:3, 3])
    return float(np.linalg.norm(d, axis=1).mean())


# ---------------------------------------------------------------- the end-to-end cases (tests/test_register_host.py, tests/test_gpu_register.py,
# scripts/register_recovery.py)

TRUE_CENTRE = (1.0, -2.0, 0.5)
RIGID = (4.0, -3.0, 5.0, 2.5, -1.5, 2.0)                          # degrees about x, y, z; mm
E2E_CASES = {"rigid6": (RIGID, 6, "corratio", True), "affine12": (RIGID + (1.05, 0.97, 1.02, 0.0, 0.0, 0.0), 12, "corratio", True),
             "rigid6_normcorr": (RIGID, 6, "normcorr", False), "rigid6_leastsq": (RIGID, 6, "leastsq", False)}
CAP_MM = PHANTOM_MM                                                # a registration worse than one fixed voxel is of no use for ROI statistics


def e2e_case(name, register_module):
    """-> (true_world, dof, kind, (fixed, fixed_affine, moving, moving_affine, mask))"""
    p, dof, kind, remapped = E2E_CASES[name]
    true_world = register_module.params_to_world(p, dof, centre=TRUE_CENTRE)
    return true_world, dof, kind, phantom_pair(true_world, remapped)


def atlas_labels():
    """an integer label image on the moving image's grid [22, 20, 18]: a few blocks several voxels wide, inside the body"""
    lab = np.zeros((22, 20, 18), dtype=np.int16)
    lab[5:10, 5:10, 5:10] = 1
    lab[11:17, 6:11, 6:12] = 2
    lab[7:13, 11:15, 7:12] = 3
    lab[8:14, 7:12, 12:15] = 7
    return lab


def label_share(world_a, world_b, fixed_affine, moving_affine, voxel_matrix):
    """the share of the fixed grid's voxels whose resampled atlas label differs between the two world matrices"""
    lab = atlas_labels()
    a = rn.resample_labels(lab, voxel_matrix(fixed_affine, moving_affine, world_a), PHANTOM_SHAPE)
    b = rn.resample_labels(lab, voxel_matrix(fixed_affine, moving_affine, world_b), PHANTOM_SHAPE)
    return float((a != b).mean())
