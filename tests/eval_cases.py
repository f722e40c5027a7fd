"""Seeded inputs of tests/golden/eval.npz, shared by the maker (tests/golden/make_golden_eval.py) and the tests of lopq.eval.

The fixture stores reference OUTPUTS (scipy's cdist ranked, the reference's eval.py on a small model) and a checksum of every
input; the inputs themselves are regenerated here.
"""
import hashlib

import numpy as np

DIMS = [1, 5, 24, 128, 130]
ROWS = [1, 63, 65, 1000, 4099]
QUERIES = [1, 3, 257]
K = 10


def sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def random_cases():
    """[(name, d, m2, m1, dtype)]: every d with every m2; m1 and the dtype cycle through them; the largest problem and the
    1000-row one (the smallest that takes the matrix-core path at every d) in both dtypes with 257 queries."""
    out = []
    for i, d in enumerate(DIMS):
        for j, m2 in enumerate(ROWS):
            out.append((d, m2, QUERIES[(i + j) % 3], ["f8", "f4"][(2 * i + j) % 2]))
    for d, m2 in ((130, 4099), (128, 1000), (5, 4099), (24, 50)):
        for dt in ("f8", "f4"):
            out.append((d, m2, 3 if m2 == 50 else 257, dt))
    seen, cases = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            cases.append(("r_d%d_n%d_q%d_%s" % c,) + c)
    return cases


def random_inputs(name, d, m2, m1, dtype):
    """(queries [m1, d], data [m2, d]) of a random case."""
    rs = np.random.RandomState(int(hashlib.sha1(name.encode()).hexdigest()[:8], 16))
    data = rs.standard_normal((m2, d)).astype(dtype)
    q = rs.standard_normal((m1, d)).astype(dtype)
    return q, data


def chain_sq(x, y):
    """The float64 chain scipy's cdist evaluates (before the square root), in pure Python."""
    s = 0.0
    for a, b in zip(np.asarray(x, dtype=np.float64).tolist(), np.asarray(y, dtype=np.float64).tolist()):
        t = a - b
        s = s + t * t
    return s


def engineered_inputs():
    """{name: (queries, data)}: the rows a ranking by anything but (sqrt of the chain, index) gets wrong."""
    out = {}
    rs = np.random.RandomState(4242)
    # (a) copies of a query's nearest neighbour at a lower and at a higher index; (b) a query that IS a data row
    data = rs.standard_normal((200, 24))
    q = rs.standard_normal((4, 24))
    data[:20] += 8.0  # (keeps the nearest neighbour of query 0 away from the edges)
    data[180:] += 8.0
    nn = int(np.argmin(((q[0] - data) ** 2).sum(axis=1)))
    data[nn - 7] = data[nn]
    data[nn + 5] = data[nn]
    q[1] = data[17]
    out["e_dup"] = (q, data)
    out["e_dup_f4"] = (q.astype(np.float32), data.astype(np.float32))
    # (c) the square-root collision: row 0 is strictly farther than row 1 in the squared chain, both square roots are one float64
    for d in (2, 66):
        v = None
        while v is None:
            c = float(rs.uniform(0.5, 2.0))
            e = float(np.sqrt(np.spacing(c * c)))
            if chain_sq([0.0, 0.0], [c, e]) > chain_sq([0.0, 0.0], [c, 0.0]) and \
                    np.sqrt(chain_sq([0.0, 0.0], [c, e])) == np.sqrt(chain_sq([0.0, 0.0], [c, 0.0])):
                v = (c, e)
        data = np.zeros((40, d))
        data[2:, :] = rs.standard_normal((38, d)) + 3.0
        data[0, d - 2:] = v
        data[1, d - 2:] = (v[0], 0.0)
        out["e_sqrt_d%d" % d] = (np.zeros((1, d)), data)
    # (d) 2 000 identical rows: no bound separates them
    row = rs.standard_normal((1, 24))
    out["e_same"] = (rs.standard_normal((3, 24)), np.repeat(row, 2000, axis=0))
    return out


# ---- the small model: V = 4, M = 8, K = 16, D = 32 -----------------------------------------------------------------------------
MODEL = dict(V=4, M=8, subquantizer_clusters=16)
THRESHOLDS = [1, 10, 100]
N_SUB = 500  # rows given to the two quadratic functions


def model_inputs():
    """(X [3000, 32], Q [40, 32]) float64: 12 clusters."""
    rs = np.random.RandomState(20260)
    centers = rs.standard_normal((12, 32)) * 2.0
    X = centers[rs.randint(0, 12, 3000)] + 0.5 * rs.standard_normal((3000, 32))
    Q = centers[rs.randint(0, 12, 40)] + 0.5 * rs.standard_normal((40, 32))
    return X, Q
