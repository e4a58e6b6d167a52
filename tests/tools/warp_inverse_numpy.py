"""met2_warp_invert_step and met2_warp_jacobian of include/met2_hip.h and the loop of warp.invert, restated in numpy operation by operation,
with a `dtype` argument: np.longdouble is the reference the device is held against, np.float64 runs the loop on the CPU
(warp.invert(step=STEP)).  As in warp_numpy, the coordinates, the inside test, the clamp, the floors and the tap indices are fp64 in both --
they are the contract, and v_in feeds coordinates --; the weights, the tap sums, the 3 x 3 product, the change and its norm, the differences
and the determinant run in `dtype`.  Also the cases of tests/test_warp_inverse_host.py and tests/test_gpu_warp_inverse.py."""
import numpy as np

import register_numpy as gn
import warp_numpy as wn


def invert_step(u, B, N, shape, v_in=None, return_inside=False, return_res2=False, dtype=np.longdouble, return_coords=False):
    """v_out(y) = N u_tri(clamp(B (y + v_in(y)))) on the grid `shape`; inside from the coordinates before the clamp; res2 = max |v_out - v_in|^2
    (a value that is not a number passed over) -> v_out [shape + (3,)] in dtype, then inside uint8, res2 (dtype), the raw coordinates"""
    dtype = np.dtype(dtype).type
    u = np.asarray(u, dtype=np.float64)
    shape = tuple(int(n) for n in shape)
    B = np.asarray(B, dtype=np.float64)
    N = np.asarray(N, dtype=np.float64).astype(dtype)
    v = np.zeros(shape + (3,)) if v_in is None else np.asarray(v_in, dtype=np.float64)
    c_raw = wn.coords(B, v)                                        # p_a = y_a + v_in_a; c_a = ((B[a][3] + B[a][0] p_x) + B[a][1] p_y) + B[a][2] p_z
    ins = np.ones(shape, dtype=bool)
    for a in range(3):
        ins &= (c_raw[a] >= 0.0) & (c_raw[a] <= float(u.shape[a] - 1))
    c = np.stack([np.where(c_raw[a] >= 0.0, np.minimum(c_raw[a], float(u.shape[a] - 1)), 0.0) for a in range(3)])
    t = wn._tap_sum(np.moveaxis(u, 3, 0), c.reshape(3, -1), u.shape[:3], 1, dtype).reshape((3,) + shape)
    out = np.stack([(N[a, 0] * t[0] + N[a, 1] * t[1]) + N[a, 2] * t[2] for a in range(3)], axis=-1)
    res = (out,)
    if return_inside:
        res += (ins.astype(np.uint8),)
    if return_res2:
        res += (res2_of(out, v, dtype),)
    if return_coords:
        res += (c_raw,)
    return res if len(res) > 1 else res[0]


def res2_of(v_out, v_in, dtype=np.longdouble):
    """max over the voxels of (d_x d_x + d_y d_y) + d_z d_z, d = v_out - v_in; 0 where none is a number above 0"""
    dtype = np.dtype(dtype).type
    d = np.asarray(v_out).astype(dtype) - (dtype(0) if v_in is None else np.asarray(v_in, dtype=np.float64).astype(dtype))
    q = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    q = q[q > 0]
    return q.max() if q.size else dtype(0)


def _diff(f, axis, dtype):
    """D_axis f: (f(x + e) - f(x - e)) / 2 inside, one-sided at the rims, 0 on an axis of length 1"""
    n = f.shape[axis]
    if n == 1:
        return np.zeros(f.shape, dtype=dtype)
    idx = np.arange(n)
    lo, hi = np.maximum(idx - 1, 0), np.minimum(idx + 1, n - 1)
    df = np.take(f, hi, axis=axis) - np.take(f, lo, axis=axis)
    shape = [1, 1, 1]
    shape[axis] = n
    return np.where((hi - lo).reshape(shape) == 2, df / dtype(2), df)


def jacobian(disp, scale=1.0, dtype=np.longdouble):
    """-> (det [nx, ny, nz] in dtype, the number of voxels whose det is not > 0)"""
    dtype = np.dtype(dtype).type
    u = np.asarray(disp, dtype=np.float64).astype(dtype)
    J = [[_diff(u[..., a], b, dtype) for b in range(3)] for a in range(3)]        # J_ab = delta_ab + D_b u_a
    for a in range(3):
        J[a][a] = dtype(1) + J[a][a]
    m0 = J[1][1] * J[2][2] - J[1][2] * J[2][1]
    m1 = J[1][0] * J[2][2] - J[1][2] * J[2][0]
    m2 = J[1][0] * J[2][1] - J[1][1] * J[2][0]
    det = dtype(scale) * ((J[0][0] * m0 - J[0][1] * m1) + J[0][2] * m2)
    return det, int((~(det > 0)).sum())


def inverse_matrices(A):
    """(B, N) of an inverse step: B = A^-1 as [3, 4], N = -L"""
    A = np.asarray(A, dtype=np.float64)
    Li = np.linalg.inv(A[:, :3])
    return np.ascontiguousarray(np.column_stack([Li, -Li @ A[:, 3]])), np.ascontiguousarray(-A[:, :3])


def invert(disp, A, shape, n_iter=20, dtype=np.longdouble):
    """the loop of warp.invert: v_0 = 0, v_{k+1} = step(v_k), every v rounded to fp64 between the steps as the device stores it
    -> dict(disp fp64, B, N, inside, residual [n_iter] fp64, coords: the last step's coordinates before the clamp)"""
    B, N = inverse_matrices(A)
    v, inside, c, rows = None, None, None, []
    for _ in range(int(n_iter)):
        out, inside, r2, c = invert_step(disp, B, N, shape, v, True, True, dtype, True)
        v = np.asarray(out, dtype=np.float64)
        rows.append(float(np.sqrt(r2)))
    v = np.zeros(tuple(shape) + (3,)) if v is None else v
    return {"disp": v, "B": B, "N": N, "inside": inside, "residual": np.asarray(rows), "coords": c}


def STEP(u, B, N, shape, v_in=None, return_inside=True, return_res2=True):
    """invert_step in fp64 for warp.invert(step=STEP)"""
    out, ins, r2 = invert_step(u, B, N, shape, v_in, True, True, np.float64)
    return np.asarray(out, dtype=np.float64), ins, float(r2)


# ---------------------------------------------------------------- the cases

GRID = (20, 18, 16)
LINEAR_M = np.array([[0.1, 0.05, 0.0], [0.0, -0.1, 0.02], [0.03, 0.0, 0.08]])
LINEAR_T = np.array([0.5, -0.25, 0.125])
IDENTITY = np.ascontiguousarray(np.eye(4)[:3])
SMOOTH_DST = (22, 17, 16)
JACOBIAN_GRIDS = wn.GRIDS + ((2, 3, 2),)


def linear_field(grid=GRID, M=LINEAR_M, t=LINEAR_T):
    """u(x) = M x + t"""
    x = np.stack(wn._grid(grid), axis=-1)
    return np.ascontiguousarray(x @ np.asarray(M).T + np.asarray(t))


def linear_inverse(grid=GRID, M=LINEAR_M, t=LINEAR_T):
    """the closed form for A = identity: v(y) = (I + M)^-1 (y - t) - y, and whether the pre-image y + v(y) lies inside the grid"""
    y = np.stack(wn._grid(grid), axis=-1)
    pre = (y - t) @ np.linalg.inv(np.eye(3) + M).T
    ok = np.all((pre >= 0.0) & (pre <= np.asarray(grid, dtype=np.float64) - 1.0), axis=-1)
    return pre - y, ok


def smooth_field(grid=GRID):
    x, y, z = wn._grid(grid)
    return np.ascontiguousarray(np.stack([1.5 * np.sin(2 * np.pi * y / 18.0) * np.cos(np.pi * z / 16.0), 1.5 * np.sin(2 * np.pi * z / 16.0),
                                          1.5 * np.cos(2 * np.pi * x / 20.0) * np.sin(np.pi * y / 18.0)], axis=-1))


def smooth_transform():
    """A = R diag(1.1, 0.9, 1.0) (the diagonal scales R's columns), R a rotation of 0.1 rad about z, translation (1.3, -0.7, 0.4)"""
    c, s = np.cos(0.1), np.sin(0.1)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return np.ascontiguousarray(np.column_stack([R @ np.diag([1.1, 0.9, 1.0]), [1.3, -0.7, 0.4]]))


def round_trip_error(u, A, inv, dtype=np.longdouble):
    """the invariant's left side: |A (c + u_tri(c)) - y| (max norm over the axes) at every destination voxel y, c = B (y + v(y)) of the field
    `inv['disp']`, evaluated in `dtype`; and the voxels whose unclamped c is inside -> (error [shape], inside bool [shape])"""
    dtype = np.dtype(dtype).type
    shape = inv["disp"].shape[:3]
    eye = np.eye(3)
    t, ins, c = invert_step(u, inv["B"], eye, shape, inv["disp"], return_inside=True, dtype=dtype, return_coords=True)
    A = np.asarray(A, dtype=np.float64).astype(dtype)
    p = c.astype(dtype) + np.moveaxis(t, 3, 0)
    y = wn._grid(shape)
    err = np.zeros(shape, dtype=dtype)
    for a in range(3):
        err = np.maximum(err, np.abs((((A[a, 3] + A[a, 0] * p[0]) + A[a, 1] * p[1]) + A[a, 2] * p[2]) - y[a]))
    return err, ins != 0


def folded_field(grid):
    """u_x = -1.5 x: det = -0.5 at every voxel of a grid whose x axis is longer than 1"""
    u = np.zeros(tuple(grid) + (3,))
    u[..., 0] = -1.5 * wn._grid(grid)[0]
    return u


def designed_folds(grid=(17, 17, 257)):
    """a zero field with single voxels displaced by 3 along z: the next voxel of each along z sees D_z u_z = -1.5 (-3 at a rim), so its det =
    1 + D_z u_z is negative; every other det stays positive.  The displaced voxels sit in pairs before the seams between blocks of 256
    consecutive voxels, so folded voxels are the last of one block and the first of the next
    -> (field, the linear indices of the voxels that fold: 255 | 256 and 511 | 512 are seams, the last voxel ends the last block)"""
    n = int(np.prod(grid))
    u = np.zeros((n, 3))
    u[[254, 255, 510, 511, n - 2], 2] = 3.0
    return np.ascontiguousarray(u.reshape(tuple(grid) + (3,))), np.array([255, 256, 511, 512, n - 1])


def case_matrix():
    """a full 3 x 3 matrix N for the parity cases: no entry 0 or 1"""
    return np.array([[-1.07, 0.031, -0.012], [0.094, -0.913, 0.027], [-0.018, 0.006, -1.002]])


def round_trip_inputs():
    """the label round trip (scripts/warp_inverse_recovery.py, tests/test_gpu_warp_inverse.py) -> (labels on the template grid, their
    affine, the maps' affine, A: maps voxel -> template voxel, u: the true field on the maps' grid in its voxels, the labels that (A, u)
    brings onto the maps' grid)"""
    lab, la, truth = wn.atlas_case()
    fa = gn.phantom_affine()
    A = np.ascontiguousarray((np.linalg.inv(la) @ fa)[:3])
    u = wn.true_disp(gn.grid_world(gn.PHANTOM_SHAPE, fa)) / gn.PHANTOM_MM
    return lab, la, fa, A, np.ascontiguousarray(u), truth


def label_share(back, lab):
    """-> (the share of the labelled voxels of `lab` that carry their own label in `back`, their number)"""
    sel = lab > 0
    return float((np.asarray(back)[sel] == lab[sel]).mean()), int(sel.sum())
