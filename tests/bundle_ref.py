"""Numpy restatement of mvsdf_amd/bundle.py's definition, written from its docstring: every product and sum is its own numpy operation in the stated
order (numpy contracts nothing), sums over a track run sequentially from 0.0, sums over a view and over the 6 V entries are the canonical pairwise
tree.  The device results equal these as numbers, entry for entry (torch.equal)."""
import collections

import numpy as np

MAX_THETA, ROD_TERMS, FLOOR = 1.0, 10, 1e-6

Lin = collections.namedtuple('Lin', 'r A B active')
Blocks = collections.namedtuple('Blocks', 'U gc V gp b lam lin Vinv Ud Minv moves fixed off view order voff pose intr xyz')
Result = collections.namedtuple('Result', 'cams xyz residuals cost0 cost iterations accepted cg_iterations lam costs')


def tree_sum(a):
    """the canonical pairwise tree over axis 0: pad with +0.0 to a power-of-two length, add adjacent pairs until one row is left"""
    a = np.asarray(a, np.float64)
    size = 1
    while size < a.shape[0]:
        size *= 2
    a = np.concatenate([a, np.zeros((size - a.shape[0],) + a.shape[1:])])
    while a.shape[0] > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def rodrigues_table():
    fact = [1.0]
    for k in range(1, 2 * ROD_TERMS + 2):
        fact.append(fact[-1] * float(k))
    sign = [1.0 if k % 2 == 0 else -1.0 for k in range(ROD_TERMS)]
    return np.array([sign[k] / fact[2 * k + 1] for k in range(ROD_TERMS)] + [sign[k] / fact[2 * k + 2] for k in range(ROD_TERMS)], dtype=np.float64)


def pose_arrays(cams):
    cams = np.asarray(cams, np.float64)
    pose = np.concatenate([cams[:, 0, :3, :3].reshape(-1, 9), cams[:, 0, :3, 3]], 1)
    Km = cams[:, 1]
    intr = np.stack([Km[:, 0, 0], Km[:, 0, 1], Km[:, 0, 2], Km[:, 1, 1], Km[:, 1, 2]], 1)
    return np.ascontiguousarray(pose), np.ascontiguousarray(intr)


def cams_with(cams, pose):
    out = np.array(cams, np.float64)
    out[:, 0, :3, :3] = pose[:, :9].reshape(-1, 3, 3)
    out[:, 0, :3, 3] = pose[:, 9:]
    return out


def exp_rotation(w, table=None):
    """E(omega) [3,3] by the polynomials, or None beyond the bound"""
    table = rodrigues_table() if table is None else table
    z = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    if not z <= MAX_THETA * MAX_THETA:
        return None
    a, b = table[ROD_TERMS - 1], table[2 * ROD_TERMS - 1]
    for k in range(ROD_TERMS - 2, -1, -1):
        a = a * z + table[k]
        b = b * z + table[ROD_TERMS + k]
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    E = np.zeros((3, 3))
    for k in range(3):
        for l in range(3):
            E[k, l] = ((1.0 if k == l else 0.0) + a * Kx[k, l]) + b * (w[k] * w[l] - z if k == l else w[k] * w[l])
    return E


def _owner(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def _project(pose, intr, xyz, off, view, obs):
    """-> (q [nnz,3], u, v, r [nnz,2], front bool, active bool)"""
    j = _owner(off)
    ps, X = pose[view], xyz[j]
    q = np.stack([((ps[:, 3 * k] * X[:, 0] + ps[:, 3 * k + 1] * X[:, 1]) + ps[:, 3 * k + 2] * X[:, 2]) + ps[:, 9 + k] for k in range(3)], 1)
    front = q[:, 2] > 0.0
    with np.errstate(all='ignore'):
        u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    k = intr[view]
    r = np.stack([((k[:, 0] * u + k[:, 1] * v) + k[:, 2]) - obs[:, 0], (k[:, 3] * v + k[:, 4]) - obs[:, 1]], 1)
    active = (np.diff(off) >= 2)[j]
    return q, u, v, r, front, active


def residuals(cams, xyz, off, view, obs, loss_scale=None, trial=False):
    """-> (r [nnz,2], terms [nnz], cost); behind: +inf with trial, else ValueError"""
    pose, intr = pose_arrays(cams)
    return _residuals(pose, intr, np.asarray(xyz, np.float64), off, view, obs, loss_scale, trial)


def _residuals(pose, intr, xyz, off, view, obs, loss_scale, trial):
    delta = np.inf if loss_scale is None else float(loss_scale)
    q, u, v, r, front, active = _project(pose, intr, xyz, off, view, obs)
    if (active & ~front).any() and not trial:
        raise ValueError('residuals: a point lies behind a camera that observes it')
    with np.errstate(all='ignore'):
        s2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        n = np.sqrt(s2)
        c = np.where(n <= delta, 0.5 * s2, delta * (n - 0.5 * delta))
    c = np.where(front, c, np.inf)
    c = np.where(active, c, 0.0)
    r = np.where((active & front)[:, None], r, 0.0)
    return r, c, float(tree_sum(c))


def linearise(pose, intr, xyz, off, view, obs, loss_scale=None):
    delta = np.inf if loss_scale is None else float(loss_scale)
    q, u, v, r, front, active = _project(pose, intr, xyz, off, view, obs)
    active = active & front
    k = intr[view]
    with np.errstate(all='ignore'):
        nr = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
        w = np.where(nr <= delta, 1.0, delta / nr)
        sw = np.sqrt(w)
        q0, q1, q2 = q[:, 0], q[:, 1], q[:, 2]
        D = np.zeros((len(view), 2, 3))
        D[:, 0, 0] = k[:, 0] / q2
        D[:, 0, 1] = k[:, 1] / q2
        D[:, 0, 2] = -((k[:, 0] * u + k[:, 1] * v) / q2)
        D[:, 1, 1] = k[:, 3] / q2
        D[:, 1, 2] = -((k[:, 3] * v) / q2)
        A, B = np.zeros((len(view), 2, 6)), np.zeros((len(view), 2, 3))
        ps = pose[view]
        for e in range(2):
            A[:, e, 0] = (D[:, e, 2] * q1 - D[:, e, 1] * q2) * sw
            A[:, e, 1] = (D[:, e, 0] * q2 - D[:, e, 2] * q0) * sw
            A[:, e, 2] = (D[:, e, 1] * q0 - D[:, e, 0] * q1) * sw
            for l in range(3):
                A[:, e, 3 + l] = D[:, e, l] * sw
                B[:, e, l] = ((D[:, e, 0] * ps[:, l] + D[:, e, 1] * ps[:, 3 + l]) + D[:, e, 2] * ps[:, 6 + l]) * sw
        rw = r * sw[:, None]
    m = active[:, None]
    return Lin(np.where(m, rw, 0.0), np.where(m[:, :, None], A, 0.0), np.where(m[:, :, None], B, 0.0), active)


def track_sum(terms, off):
    """[nnz, ...] -> [P, ...]: every track's terms added one after the other from 0.0"""
    P, length = len(off) - 1, np.diff(off)
    out = np.zeros((P,) + terms.shape[1:])
    for e in range(int(length.max()) if P else 0):
        sel = length > e
        out[sel] = out[sel] + terms[off[:-1][sel] + e]
    return out


def view_order(view, V):
    order = np.argsort(view, kind='stable')
    voff = np.concatenate([[0], np.cumsum(np.bincount(view, minlength=V))]).astype(np.int64)
    return order, voff


def view_sum(terms, order, voff):
    return np.stack([tree_sum(terms[order[voff[v]:voff[v + 1]]]) for v in range(len(voff) - 1)])


def _fixed_mask(fixed_views, V):
    f = np.asarray(fixed_views)
    if f.dtype == bool:
        return f.copy()
    m = np.zeros(V, bool)
    m[f.astype(np.int64)] = True
    return m


def _sym3_inverse(m, lam, floor, ok0):
    """the damped inverse by the adjugate -> [P,3,3], zero where it fails"""
    m00 = m[:, 0, 0] + lam * np.maximum(m[:, 0, 0], floor)
    m11 = m[:, 1, 1] + lam * np.maximum(m[:, 1, 1], floor)
    m22 = m[:, 2, 2] + lam * np.maximum(m[:, 2, 2], floor)
    m01, m02, m12 = m[:, 0, 1], m[:, 0, 2], m[:, 1, 2]
    with np.errstate(all='ignore'):
        det = (m00 * (m11 * m22 - m12 * m12) - m01 * (m01 * m22 - m12 * m02)) + m02 * (m01 * m12 - m11 * m02)
        i00 = (m11 * m22 - m12 * m12) / det
        i01 = (m02 * m12 - m01 * m22) / det
        i02 = (m01 * m12 - m02 * m11) / det
        i11 = (m00 * m22 - m02 * m02) / det
        i12 = (m01 * m02 - m00 * m12) / det
        i22 = (m00 * m11 - m01 * m01) / det
    inv = np.stack([np.stack([i00, i01, i02], 1), np.stack([i01, i11, i12], 1), np.stack([i02, i12, i22], 1)], 1)
    ok = ok0 & (det > 0.0) & np.isfinite(det) & np.isfinite(inv).all((1, 2))
    return np.where(ok[:, None, None], inv, 0.0)


def _ldl_inverse(U):
    """the inverse of one 6x6 by the written-order LDL^T, or None where a pivot is not finite and > 0"""
    L, d = np.zeros((6, 6)), np.zeros(6)
    ok = True
    with np.errstate(all='ignore'):
        for j in range(6):
            s = U[j, j]
            for k in range(j):
                s = s - (L[j, k] * L[j, k]) * d[k]
            d[j] = s
            ok = ok and bool(s > 0.0) and bool(np.isfinite(s))
            for i in range(j + 1, 6):
                e = U[i, j]
                for k in range(j):
                    e = e - (L[i, k] * L[j, k]) * d[k]
                L[i, j] = e / s
        M = np.zeros((6, 6))
        for c in range(6):
            y = np.zeros(6)
            for i in range(6):
                s = 1.0 if i == c else 0.0
                for k in range(i):
                    s = s - L[i, k] * y[k]
                y[i] = s
            y = y / d
            for i in range(5, -1, -1):
                s = y[i]
                for k in range(i + 1, 6):
                    s = s - L[k, i] * y[k]
                y[i] = s
                M[i, c] = s
    return M if ok and np.isfinite(M).all() else None


def _mul3(Vinv, a):
    return np.stack([(Vinv[:, k, 0] * a[:, 0] + Vinv[:, k, 1] * a[:, 1]) + Vinv[:, k, 2] * a[:, 2] for k in range(3)], 1)


def _wy_terms(lin, y_obs):
    """W_o y per observation [nnz,6] = A^T (B y)"""
    A, B = lin.A, lin.B
    t0 = (B[:, 0, 0] * y_obs[:, 0] + B[:, 0, 1] * y_obs[:, 1]) + B[:, 0, 2] * y_obs[:, 2]
    t1 = (B[:, 1, 0] * y_obs[:, 0] + B[:, 1, 1] * y_obs[:, 1]) + B[:, 1, 2] * y_obs[:, 2]
    return np.stack([A[:, 0, k] * t0 + A[:, 1, k] * t1 for k in range(6)], 1)


def _wtx(lin, off, view, x):
    """sum over each track from 0.0 of W_o^T x_view [P,3] = B^T (A x)"""
    A, B, xv = lin.A, lin.B, x[view]
    u0, u1 = np.zeros(len(view)), np.zeros(len(view))
    for k in range(6):
        u0 = u0 + A[:, 0, k] * xv[:, k]
        u1 = u1 + A[:, 1, k] * xv[:, k]
    return track_sum(np.stack([B[:, 0, l] * u0 + B[:, 1, l] * u1 for l in range(3)], 1), off)


def normal_blocks(cams, xyz, off, view, obs, fixed_views=(0,), lam=1e-4, loss_scale=None, floor=FLOOR):
    pose, intr = pose_arrays(cams)
    return _blocks(pose, intr, np.asarray(xyz, np.float64), off, view, obs, _fixed_mask(fixed_views, len(pose)), lam, loss_scale, floor)


def _blocks(pose, intr, xyz, off, view, obs, fixed, lam, loss_scale, floor):
    V = len(pose)
    lin = linearise(pose, intr, xyz, off, view, obs, loss_scale)
    A, B, r = lin.A, lin.B, lin.r
    order, voff = view_order(view, V)
    Ut = np.stack([np.stack([A[:, 0, k] * A[:, 0, l] + A[:, 1, k] * A[:, 1, l] for l in range(6)], 1) for k in range(6)], 1)
    U = view_sum(Ut, order, voff)
    gc = view_sum(np.stack([A[:, 0, k] * r[:, 0] + A[:, 1, k] * r[:, 1] for k in range(6)], 1), order, voff)
    Vb = track_sum(np.stack([np.stack([B[:, 0, k] * B[:, 0, l] + B[:, 1, k] * B[:, 1, l] for l in range(3)], 1) for k in range(3)], 1), off)
    gp = track_sum(np.stack([B[:, 0, k] * r[:, 0] + B[:, 1, k] * r[:, 1] for k in range(3)], 1), off)
    Vinv = _sym3_inverse(Vb, lam, floor, np.diff(off) >= 2)
    wt = view_sum(_wy_terms(lin, _mul3(Vinv, gp)[_owner(off)]), order, voff)
    Ud = U.copy()
    for k in range(6):
        Ud[:, k, k] = U[:, k, k] + lam * np.maximum(U[:, k, k], floor)
    Minv, moves, b = np.zeros((V, 6, 6)), np.zeros(V, bool), np.zeros((V, 6))
    for v in range(V):
        M = None if fixed[v] else _ldl_inverse(Ud[v])
        if M is not None:
            Minv[v], moves[v], b[v] = M, True, (-gc[v]) + wt[v]
    return Blocks(U, gc, Vb, gp, b, lam, lin, Vinv, Ud, Minv, moves, fixed, off, view, order, voff, pose, intr, xyz)


def _mat6(M, x):
    out = np.zeros_like(x)
    for l in range(6):
        out = out + M[:, :, l] * x[:, l][:, None]
    return out


def schur_apply(bl, x):
    y = _mul3(bl.Vinv, _wtx(bl.lin, bl.off, bl.view, x))
    wy = view_sum(_wy_terms(bl.lin, y[_owner(bl.off)]), bl.order, bl.voff)
    return np.where(bl.moves[:, None], _mat6(bl.Ud, x) - wy, 0.0)


def solve_reduced(bl, cg_iters=64, cg_tol=1e-8, b=None):
    """-> (x [V,6], iterations)"""
    b = bl.b if b is None else np.asarray(b, np.float64)
    x = np.zeros_like(b)
    r = np.where(bl.moves[:, None], b, 0.0)
    z = _mat6(bl.Minv, r)
    p = z.copy()
    rho = rho0 = tree_sum((r * z).reshape(-1))
    done, n = not (rho > 0.0 and np.isfinite(rho)), 0
    for _ in range(cg_iters):
        if done:
            break
        q = schur_apply(bl, p)
        sigma = tree_sum((p * q).reshape(-1))
        if not sigma > 0.0 or not np.isfinite(sigma):
            break
        alpha = rho / sigma
        x = x + alpha * p
        r = r - alpha * q
        z = _mat6(bl.Minv, r)
        rhon = tree_sum((r * z).reshape(-1))
        with np.errstate(all='ignore'):
            beta = rhon / rho
        p = z + beta * p
        rho, n = rhon, n + 1
        done = not rhon > (cg_tol * cg_tol) * rho0
    return x, n


def apply_step(bl, x):
    """-> (pose [V,12], xyz [P,3], within the rotation bound)"""
    acc = (-bl.gp) - _wtx(bl.lin, bl.off, bl.view, x)
    xyz = bl.xyz + _mul3(bl.Vinv, acc)
    pose, ok, table = bl.pose.copy(), True, rodrigues_table()
    for v in range(len(pose)):
        E = exp_rotation(x[v, :3], table)
        if E is None:
            ok = False
            continue
        if bl.fixed[v]:
            continue
        ps = bl.pose[v]
        for k in range(3):
            for l in range(3):
                pose[v, 3 * k + l] = (E[k, 0] * ps[l] + E[k, 1] * ps[3 + l]) + E[k, 2] * ps[6 + l]
            pose[v, 9 + k] = ((E[k, 0] * ps[9] + E[k, 1] * ps[10]) + E[k, 2] * ps[11]) + x[v, 3 + k]
    return pose, xyz, ok


def accepts(cost, trial, within_bound):
    """the acceptance rule of a step: every rotation within the bound, the trial cost finite and strictly below the cost"""
    return bool(within_bound and np.isfinite(trial) and trial < cost)


def bundle_adjust(cams, xyz, off, view, obs, fixed_views=(0,), iterations=10, lambda0=1e-4, lambda_min=1e-10, lambda_max=1e10, cg_iters=64,
                  cg_tol=1e-8, ftol=1e-9, loss_scale=None, floor=FLOOR):
    pose, intr = pose_arrays(cams)
    xyz = np.array(xyz, np.float64)
    fixed = _fixed_mask(fixed_views, len(pose))
    _, _, cost = _residuals(pose, intr, xyz, off, view, obs, loss_scale, False)
    cost0, lam, it, acc, cg, costs = cost, float(lambda0), 0, 0, 0, [cost]
    for _ in range(iterations):
        bl = _blocks(pose, intr, xyz, off, view, obs, fixed, lam, loss_scale, floor)
        x, n = solve_reduced(bl, cg_iters, cg_tol)
        cg += n
        tp, tx, ok = apply_step(bl, x)
        _, _, trial = _residuals(tp, intr, tx, off, view, obs, loss_scale, True)
        it += 1
        if accepts(cost, trial, ok):
            stop = cost - trial < ftol * cost
            pose, xyz, cost, acc, lam = tp, tx, trial, acc + 1, max(lam / 10.0, lambda_min)
            costs.append(cost)
            if stop:
                break
        else:
            lam = min(lam * 10.0, lambda_max)
    r, _, _ = _residuals(pose, intr, xyz, off, view, obs, loss_scale, True)
    return Result(cams_with(cams, pose), xyz, r, cost0, cost, it, acc, cg, lam, costs)
