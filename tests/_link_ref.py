"""numpy / plain-Python restatement of the link-prediction feature (GAE / VGAE): the
edge score, the reconstruction loss and its coefficients and gradient in float64
with upstream's formula and EPS, the sampler's hash and its k-th-missing search in
the full, upper and row modes (Python integers: exact at any size), to_undirected,
the split's invariants, and ROC-AUC / average precision.  The GPU tests check the
kernels against this file, tests/test_link_host.py checks this file by hand."""
import bisect
import math

import numpy as np

EPS = 1e-15
MASK = (1 << 64) - 1
U32 = 2.0 ** -24           # fp32 unit roundoff


# ---- the sampler -----------------------------------------------------------

def mix64(z):
    """splitmix64 finaliser (mi355_mp.ops._mix64)."""
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(seed, s, m):
    """mulhi64(mix(mix(seed) ^ s), m): an integer in [0, m)."""
    return (mix64(mix64(seed & MASK) ^ s) * m) >> 64


def kth_missing(keys, r, base=0):
    """The r-th (from 0) non-negative integer not among the sorted distinct
    keys (each minus base): the smallest j with keys[j] - base - j > r, then r + j."""
    lo, hi = 0, len(keys)
    while lo < hi:
        mid = (lo + hi) // 2
        if keys[mid] - base - mid > r:
            hi = mid
        else:
            lo = mid + 1
    return r + lo


def kth_missing_brute(keys, r, total):
    have = set(keys)
    return [t for t in range(total) if t not in have][r]


def tri_key(i, j):
    """The strict upper triangle's key of i < j."""
    return j * (j - 1) // 2 + i


def tri_inverse(t):
    """(i, j) with tri_key(i, j) == t: the double sqrt, then steps of one."""
    g = max(int((1.0 + math.sqrt(1.0 + 8.0 * float(t))) * 0.5), 1)
    while g > 1 and g * (g - 1) // 2 > t:
        g -= 1
    while (g + 1) * g // 2 <= t:
        g += 1
    return t - g * (g - 1) // 2, g


def tri_inverse_float_only(t):
    g = max(int((1.0 + math.sqrt(1.0 + 8.0 * float(t))) * 0.5), 1)
    return t - g * (g - 1) // 2, g


def key_table(row, col, n, upper=False, loops=False):
    """(sorted distinct keys, edge count of the cap) of the pairs not to return;
    loops: self loops removed, then one per node (GAE.recon_loss's edge list)."""
    row, col = [int(v) for v in row], [int(v) for v in col]
    n_edges = len(row)
    if upper:
        keys = {tri_key(min(i, j), max(i, j)) for i, j in zip(row, col) if i != j}
    else:
        keys = {i * n + j for i, j in zip(row, col)}
        if loops:
            n_edges += n - sum(1 for i, j in zip(row, col) if i == j)
            keys |= {i * n + i for i in range(n)}
    return sorted(keys), n_edges


def sample_count(n_edges, n, num_neg_samples=None, upper=False, n_keys=0):
    cnt = max(min(int(num_neg_samples or n_edges), n * n - n_edges), 0)
    if upper:
        cnt //= 2
    total = n * (n - 1) // 2 if upper else n * n
    return cnt if total - n_keys > 0 else 0


def negative_sample(row, col, n, seed, num_neg_samples=None, upper=False, loops=False):
    """int64 [2, count] (upper: [2, 2 count], the pairs then their mirrors)."""
    keys, n_edges = key_table(row, col, n, upper, loops)
    cnt = sample_count(n_edges, n, num_neg_samples, upper, len(keys))
    total = n * (n - 1) // 2 if upper else n * n
    a, b = [], []
    for s in range(cnt):
        t = kth_missing(keys, draw(seed, s, total - len(keys)))
        i, j = tri_inverse(t) if upper else divmod(t, n)
        a.append(i)
        b.append(j)
    if upper:
        a, b = a + b, b + a
    return np.asarray([a, b], dtype=np.int64).reshape(2, -1)


def structured_negative_sample(row, col, n, seed):
    """k [E]: the r-th column missing from row i's keys; a full row gives -1."""
    keys, _ = key_table(row, col, n)
    out = []
    for e, i in enumerate(int(v) for v in row):
        seg = keys[bisect.bisect_left(keys, i * n):bisect.bisect_left(keys, (i + 1) * n)]
        out.append(-1 if len(seg) >= n else kth_missing(seg, draw(seed, e, n - len(seg)), i * n))
    return np.asarray(out, dtype=np.int64)


def to_undirected(edge_index, n):
    row, col = np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64)
    key = np.unique(np.concatenate([row * n + col, col * n + row]))
    return np.stack([key // n, key % n]).astype(np.int64)


# ---- the score, the loss, the gradient (float64) ---------------------------------

def score(z, row, col):
    z = np.asarray(z, dtype=np.float64)
    return (z[row] * z[col]).sum(1)


def score_bound(z, row, col):
    """2 C u sum_c |z_ic z_jc|: the order-free bound of an fp32 dot product of C
    terms (gamma_C, any summation order, products rounded first), doubled."""
    z = np.abs(np.asarray(z, dtype=np.float64))
    return 2.0 * z.shape[1] * U32 * (z[row] * z[col]).sum(1)


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, dtype=np.float64)))


def loss_terms(v, positive):
    """(t_e, d(mean t)/dv_e) of one side: upstream's formula in float64."""
    v = np.asarray(v, dtype=np.float64)
    p = sigmoid(v)
    n = max(v.size, 1)
    if positive:
        return -np.log(p + EPS), -p * (1 - p) / (p + EPS) / n
    return -np.log(1 - p + EPS), p * (1 - p) / (1 - p + EPS) / n


def side_loss(z, row, col, positive):
    t, coef = loss_terms(score(z, row, col), positive)
    return (t.mean() if t.size else float("nan")), coef, t


def grad_z(z, row, col, coef):
    """dz[i] = sum_{row_e = i} coef_e z[col_e] + sum_{col_e = i} coef_e z[row_e]."""
    z = np.asarray(z, dtype=np.float64)
    dz = np.zeros_like(z)
    c = np.asarray(coef, dtype=np.float64)[:, None]
    np.add.at(dz, row, c * z[col])
    np.add.at(dz, col, c * z[row])
    return dz


def grad_bound(z, row, col, coef, dcoef):
    """Per element of dz: sum over the edge ends at node i of |z_oc| (|coef_e| (d_i + 8)
    u + dcoef_e), d_i the number of ends at i (see tests/test_gpu_link.py)."""
    za = np.abs(np.asarray(z, dtype=np.float64))
    n = za.shape[0]
    deg = np.bincount(row, minlength=n) + np.bincount(col, minlength=n)
    ca, dc = np.abs(np.asarray(coef, dtype=np.float64)), np.asarray(dcoef, dtype=np.float64)
    out = np.zeros_like(za)
    np.add.at(out, row, za[col] * (ca * (deg[row] + 8) * U32 + dc)[:, None])
    np.add.at(out, col, za[row] * (ca * (deg[col] + 8) * U32 + dc)[:, None])
    return out


# ---- the metrics ----------------------------------------------------------

def roc_auc(y, s):
    """P(score of a positive > score of a negative) + half the ties, by pairs."""
    y, s = np.asarray(y).astype(bool), np.asarray(s, dtype=np.float64)
    pos, neg = s[y][:, None], s[~y][None, :]
    return float(((pos > neg).sum() + 0.5 * (pos == neg).sum()) / (pos.size * neg.size))


def average_precision(y, s):
    """sum_n (R_n - R_{n-1}) P_n over the distinct thresholds, highest first."""
    y, s = np.asarray(y).astype(bool), np.asarray(s, dtype=np.float64)
    ap, prev = 0.0, 0.0
    for th in sorted(set(s.tolist()), reverse=True):
        sel = s >= th
        tp = float((sel & y).sum())
        ap += (tp / y.sum() - prev) * (tp / sel.sum())
        prev = tp / y.sum()
    return ap


# ---- the split -------------------------------------------------------------

def check_split(edge_index, n, data, val_ratio, test_ratio):
    """The invariants of train_test_split_edges over an undirected edge list."""
    row, col = np.asarray(edge_index[0]), np.asarray(edge_index[1])
    up = {(int(i), int(j)) for i, j in zip(row, col) if i < j}
    n_v, n_t = int(math.floor(val_ratio * len(up))), int(math.floor(test_ratio * len(up)))
    parts = {}
    for name in ("val_pos", "test_pos", "val_neg", "test_neg"):
        ei = np.asarray(getattr(data, name + "_edge_index"))
        parts[name] = [(int(i), int(j)) for i, j in ei.T]
        assert all(i < j for i, j in parts[name]), name            # directed, upper triangle
        assert len(set(parts[name])) == len(parts[name]), name
    assert len(parts["val_pos"]) == n_v and len(parts["test_pos"]) == n_t
    train = np.asarray(data.train_pos_edge_index)
    tset = {(int(i), int(j)) for i, j in train.T}
    assert np.array_equal(train, to_undirected(train, n))               # sorted, coalesced, both directions
    held = set(parts["val_pos"]) | set(parts["test_pos"])
    assert len(held) == n_v + n_t and held <= up
    assert {p for p in tset if p[0] < p[1]} == up - held
    free = n * (n - 1) // 2 - len(up)
    assert len(parts["val_neg"]) == min(n_v, free) and len(parts["test_neg"]) == max(min(n_t, free - n_v), 0)
    negs = set(parts["val_neg"]) | set(parts["test_neg"])
    assert len(negs) == len(parts["val_neg"]) + len(parts["test_neg"]) and not (negs & up)
    mask = np.asarray(data.train_neg_adj_mask)
    want = np.triu(np.ones((n, n), dtype=bool), 1)
    for i, j in up | negs:
        want[i, j] = False
    assert mask.dtype == np.bool_ and np.array_equal(mask, want)
    return n_v, n_t
