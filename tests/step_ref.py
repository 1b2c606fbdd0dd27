"""Plain numpy restatement of the bookkeeping of one training step (csrc/step_kernels.hip), written from the reference's tensor expressions:
the outputs of IDRNetwork.forward (idr.py:253-304: boolean-mask indexing and torch.cat of the selected point groups) and, for the backward, the adjoint
of those expressions composed with SampleNetwork (sample_network.py:10-20).  tests/test_step_ref.py pins `backward_inputs` to torch.autograd in float64.

The fused evaluation the kernels read has rows [eikonal samples (n_eik) | on-surface samples (n_ds) | jittered samples (n_ds) | all R rays, the hit ones
first in ray order]; E = n_eik + 2 n_ds.  The reference's group order in every concatenation is hit rays, eikonal samples, on-surface samples, jittered
samples (idr.py:253); bit g of d_mask / e_mask switches group g of the depth term (eikonal_output, eikonal_points_hom) / the eikonal term (grad_theta)."""
import numpy as np


def sorted_rays(surface_mask):
    """-> perm: the rays with surface_mask first, each part in ray order (what boolean-mask indexing yields, idr.py:207-212)"""
    idx = np.arange(surface_mask.size)
    return np.concatenate([idx[surface_mask], idx[~surface_mask]])


def _groups(N, n_eik, n_ds):
    """evaluation rows of the four point groups, in the reference's order"""
    E = n_eik + 2 * n_ds
    return [E + np.arange(N), np.arange(n_eik), n_eik + np.arange(n_ds), n_eik + n_ds + np.arange(n_ds)]


def _selected(mask, N, n_eik, n_ds):
    return [rows for g, rows in enumerate(_groups(N, n_eik, n_ds)) if mask >> g & 1]


def _cat(parts, tail=()):
    return np.concatenate(parts, 0) if parts else np.zeros((0,) + tuple(tail), np.float32)


def outputs(surface_mask, true_mask, n_eik, n_ds, x_eval, y_eval, n_eval, rgb_sorted, d_mask, e_mask):
    """surface_mask = network_object_mask & object_mask, true_mask = object_mask_true, bool [R] -> dict of the step's output tensors (exact shapes)."""
    R, E = surface_mask.size, n_eik + 2 * n_ds
    perm = sorted_rays(surface_mask)
    N = int(surface_mask.sum())
    ncol = min(2, y_eval.shape[1])                                        # (columns 0 and 1 are all the outputs hold; the features are not gathered)
    points, sdf_full, rgb_hit = np.empty((R, 3), x_eval.dtype), np.empty((R, ncol), y_eval.dtype), rgb_sorted[:N]
    points[perm], sdf_full[perm] = x_eval[E:], y_eval[E:, :ncol]          # back to ray order: what the tracer / the network gave per ray
    grads = n_eval[E:][:N]                                                # g[:N] of idr.py:275 (rows of the hit rays)
    sdf_output = sdf_full[:, :1]
    surface_points, surface_output = points[surface_mask], sdf_output[surface_mask]          # idr.py:208,212
    samples_y, samples_x, samples_g = y_eval[:E], x_eval[:E], n_eval[:E]                      # `output` / points_all[N:] / g[N:] of idr.py:256,275
    cuts = [(0, n_eik), (n_eik, n_eik + n_ds), (n_eik + n_ds, n_eik + 2 * n_ds)]
    eo_list = [(surface_output, surface_points)] if d_mask & 1 else []                      # idr.py:259-267
    eo_list += [(samples_y[a:b, :1], samples_x[a:b]) for g, (a, b) in enumerate(cuts) if d_mask >> (g + 1) & 1]
    eik_out = _cat([a for a, _ in eo_list], (1,)).reshape(-1)                                # .view(1, -1)
    hom = _cat([b for _, b in eo_list], (3,))
    hom = np.concatenate([hom, np.ones_like(hom[:, -1:])], -1)                               # idr.py:270
    gth_list = [grads] if e_mask & 1 else []                                                 # idr.py:277-286
    gth_list += [samples_g[a:b] for g, (a, b) in enumerate(cuts) if e_mask >> (g + 1) & 1]
    out = {'rgb_values': np.ones((R, 3), rgb_sorted.dtype), 'sdf_output': sdf_output, 'diff_pts': surface_points, 'eikonal_output': eik_out,
           'points_hom': hom, 'grad_theta': _cat(gth_list, (3,))}
    if y_eval.shape[1] > 1:
        out['surf'] = np.concatenate([sdf_full[:, 1][surface_mask & true_mask], samples_y[:n_eik, 1]])     # idr.py:272
    out['rgb_values'][surface_mask] = rgb_hit                                                # idr.py:302-304
    return out


def backward_inputs(N, n_true, n_eik, n_ds, Nout, true_rows, view_sorted, n_eval, din, din_feat0, din_nrm0, use_geo, d_diff, dx, d_eo, d_gth, d_si,
                    d_mask, e_mask, with_fbar=True, dtype=np.float64):
    """Upstream gradients (dy [E+N, Nout], dn [E+N, 3]) of the fused evaluation's rows [samples | hit rays] and SampleNetwork's scalar fbar [N], from
    the upstream of every output: d_diff (diff_surf_pts), d_eo (eikonal_output), d_gth (grad_theta), d_si (surf_indicator_output), the rendering net's
    input adjoint din [N, ld] = [points (3) | ... | normals (3) at din_nrm0 | features at din_feat0] and dx [N, 3], the adjoint the re-evaluation of the
    SDF net at the surface points sends to them.  Any of them may be None.  use_geo False: points and normals were detached in front of the rendering
    net (idr.py:331-334), only the feature columns of din count; din_nrm0 < 0: a rendering mode without normals.

    The surface point is x(theta) = c + (t - (f(x0; theta) - f0) / (n0 . v)) v with n0, f0, v constants (sample_network.py:12-18), so the adjoint xbar
    of x reaches column 0 of the hit row's output as fbar = -(xbar . v) / (n0 . v), xbar = d_diff + din[:, :3] + dx; every concatenation's adjoint is
    the split of its upstream back to the groups it joined.  v = the ray direction = -view_sorted.
    Evaluated in `dtype`, additions in the order upstream-of-the-rendering-net first, then the terms above: in float32 every cell that is a copy or
    one addition is exact, so it equals the kernels' bits."""
    E = n_eik + 2 * n_ds
    f = lambda a: None if a is None else np.asarray(a).astype(dtype)
    din, d_diff, dx, d_eo, d_gth, d_si = f(din), f(d_diff), f(dx), f(d_eo), f(d_gth), f(d_si)
    dy, dn = np.zeros((E + N, Nout), dtype), np.zeros((E + N, 3), dtype)
    if din is not None and N > 0:
        dy[E:, 2:] = din[:, din_feat0:din_feat0 + Nout - 2]                                   # feature_vectors = output[:, 2:] (idr.py:329)
        if use_geo and din_nrm0 >= 0:
            dn[E:] = din[:, din_nrm0:din_nrm0 + 3]
    if d_eo is not None:
        rows = _selected(d_mask, N, n_eik, n_ds)
        if rows:
            dy[np.concatenate(rows), 0] += d_eo.reshape(-1)                                   # split of the torch.cat (each row appears once)
    if d_gth is not None:
        rows = _selected(e_mask, N, n_eik, n_ds)
        if rows:
            dn[np.concatenate(rows)] += d_gth.reshape(-1, 3)
    if d_si is not None:
        rows = np.concatenate([E + np.asarray(true_rows[:n_true], np.int64), np.arange(n_eik)])
        dy[rows, 1] += d_si.reshape(-1)
    fbar = np.zeros(N, dtype)
    if N > 0:
        xbar = np.zeros((N, 3), dtype)
        if d_diff is not None:
            xbar = xbar + d_diff
        if din is not None and use_geo:
            xbar = xbar + din[:, :3]
        if dx is not None:
            xbar = xbar + dx
        v = -np.asarray(view_sorted[:N]).astype(dtype)
        n0 = np.asarray(n_eval[E:E + N]).astype(dtype)
        num, dot = np.zeros(N, dtype), np.zeros(N, dtype)
        with np.errstate(all='ignore'):
            for c in range(3):
                num = num + xbar[:, c] * v[:, c]
                dot = dot + n0[:, c] * v[:, c]
            fbar = -num / dot
            if with_fbar:
                dy[E:, 0] += fbar
    return dy, dn, fbar
