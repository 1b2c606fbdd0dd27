"""The cloud-cleaning definition of mvsdf_amd/cloud.py restated in numpy (fp64, every product and sum a separate numpy operation in the order the
definition writes it, so nothing is contracted).  Brute force, O(N^2) time in row chunks: fine to a few 10^4 points.  Written from that module's
doc, not from the kernels."""
import numpy as np


def d2_rows(P, lo, hi, Q=None):
    """d2 of points lo..hi-1 of P against every point of Q (default P): [(hi - lo), len(Q)]"""
    Q = P if Q is None else Q
    dx = P[lo:hi, None, 0] - Q[None, :, 0]
    dy = P[lo:hi, None, 1] - Q[None, :, 1]
    dz = P[lo:hi, None, 2] - Q[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def k_smallest(P, kmax, chunk=256, jobs=1):
    """the kmax smallest d2(i, j), j != i by index, of every point, ascending -> fp64 [N, kmax]; jobs: threads over the row chunks"""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    if not 1 <= kmax <= n - 1:
        raise ValueError('k must be in 1 .. N - 1')
    out = np.empty((n, kmax))

    def rows(lo):
        hi = min(n, lo + chunk)
        D = d2_rows(P, lo, hi)
        D[np.arange(hi - lo), np.arange(lo, hi)] = np.inf                 # j != i by index
        out[lo:hi] = np.sort(np.partition(D, kmax - 1, axis=1)[:, :kmax], axis=1)
    if jobs > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(jobs) as ex:
            list(ex.map(rows, range(0, n, chunk)))
    else:
        for lo in range(0, n, chunk):
            rows(lo)
    return out


def mean_of_smallest(s, k):
    """d = (sqrt(s_1) + ... + sqrt(s_k)) / k, summed left to right from 0, from k_smallest's rows"""
    r = np.sqrt(s[:, :k])
    acc = np.zeros(len(s))
    for j in range(k):
        acc = acc + r[:, j]
    return acc / k


def knn_mean_distance(P, k=20, chunk=256, jobs=1):
    """stage A -> d fp64 [N]"""
    return mean_of_smallest(k_smallest(P, k, chunk, jobs), k)


def lower_median(d):
    return np.sort(d)[(len(d) - 1) // 2]


def radius_components(P, eps, chunk=256):
    """labels int32 [N]: the smallest index of each point's connected component under d2 <= eps*eps (union-find over the edges)"""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    e2 = eps * eps
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        ii, jj = np.nonzero(d2_rows(P, lo, hi) <= e2)
        ii = ii + lo
        sel = jj < ii
        for i, j in zip(ii[sel].tolist(), jj[sel].tolist()):
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)                              # roots are component minima
    return np.array([find(i) for i in range(n)], np.int32)


def clean(P, k=20, knn_ratio=3.0, eps_ratio=3.0, cluster_frac=1.0, jobs=1):
    """the whole definition -> dict: d, median, threshold, eps, passed bool [N], labels int32 [N], keep uint8 [N], n_passed, n_clusters, largest"""
    P = np.ascontiguousarray(P, np.float64)
    d = knn_mean_distance(P, k, jobs=jobs)
    m = lower_median(d)
    thr = np.float64(knn_ratio) * m
    eps = np.float64(eps_ratio) * m
    passed = d <= thr
    idx = np.nonzero(passed)[0]
    labels = np.full(len(P), -1, np.int32)
    keep = np.zeros(len(P), np.uint8)
    n_clusters = largest = 0
    if len(idx):
        sub = radius_components(P[idx], eps)
        labels[idx] = idx[sub].astype(np.int32)                            # idx ascends: the smallest sub-index is the smallest input index
        roots, inv, counts = np.unique(sub, return_inverse=True, return_counts=True)
        n_clusters, largest = len(roots), int(counts.max())
        keep[idx] = counts[inv].astype(np.float64) >= np.float64(cluster_frac) * np.float64(largest)
    return dict(d=d, median=float(m), threshold=float(thr), eps=float(eps), passed=passed, labels=labels, keep=keep, n_passed=int(passed.sum()),
                n_clusters=n_clusters, largest=largest)
