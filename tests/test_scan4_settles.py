"""GPU: k_adc_scan4 (csrc/lopq_scan3.hip) settles the slots it should settle and hands over exactly the ones it should hand over.

Every other scan test compares the sampled form with the float64 kernel bit for bit, which a fast path that is wrong in the safe
direction passes: a wrong sample row, a wrong scale, a threshold that is too tight, an over-strict verification or a mis-sized list all
get the right answer from the fall-back, at twice the work.  Here tests/scan4_model.py predicts, per case, the counters of the
CIS_SCAN4_DEBUG line -- slots, fall-backs and the reason of each -- and the kernel must report the same, besides the usual parity
(_check of test_scan4_long_chunks.py: mode 5 against mode 1 bit for bit, the queries against the oracle).

A case is one fresh searcher with ONE non-empty cell that is one chunk (CIS_SEG_MAX=65536 for the long form; up to 4096 codes for the
short form), codes inserted directly, limit 100, quota = the cell's length: one work item per query, one slot, no bound published by
another cell (two slots when some of the queries have another, empty, cell as their nearest: the slot builder keeps the items of a
query's first visited cell apart).  The case lists are plain data (CASES below); tests/test_scan4_model.py asserts without a GPU that
the model calls every one of them decided -- the same at qinv * (1 +- 1e-5) -- and that each list shows what it is meant to show.

  settle    codes that settle: uniformly random codes, the fixture's own encoded rows resampled into one cell, and "near" codes
            (clusters around the queries, most codes one sub-code away), M = 4, 8 and 16, nq = 1, 3, 4.  Random codes at M = 16 stay on
            the tables' own scale (their scale sample asks for a coarser one), near codes take the saturating scale
  rows      one row of 64 near codes (the target with one sub-code changed; the target itself is not stored) in random codes.  In a
            sampled row it drags tau to the near level, fewer than 100 sums are under it and the slot fails the verification; in the
            row behind a sampled row the slot settles.  The planted sample index runs through every wave, register set and round of
            the long form's ring (test_scan4_model.py asserts the set)
  scale     M = 16: near codes at the scale sample's positions (lane * len) >> 6 make the scale so fine that tau has no room below the
            cap; one position later they are not seen
  knobs     CIS_S4_FRAC, CIS_S4_NSX and CIS_S4_SAT move the prediction and the kernel together
"""
import os
from collections import namedtuple

import numpy as np
import pytest

import scan4_model as S4
import test_scan4_long_chunks as LC

pytestmark = pytest.mark.gpu

LIMIT = 100
CELL = (2, 5)
Case = namedtuple("Case", "model form n nq dist plant knobs")
Case.__new__.__defaults__ = (None, ())
KNOB_ARG = {"CIS_S4_FRAC": ("frac", int), "CIS_S4_NSX": ("nsx", int), "CIS_S4_SAT": ("sat", float)}


def case_id(c):
    s = "%s-%s-%d-nq%d-%s" % (c.model, c.form, c.n, c.nq, c.dist)
    if c.plant:
        s += "-%s%d" % c.plant
    return s + "".join("-%s=%s" % (k[7:].lower(), v) for k, v in c.knobs)


# ---- worlds: the CPU half (oracle model, cell, query mapping) and, on the GPU only, the library's model ---------------------------------
_worlds, _hip = {}, {}
R16 = (16, 16, 256, 128, 1616)  # _random_model(V, M, K, D, seed) of test_lopq_hip_parity.py: untrained, no PCA, loads at once


def _random_oracle(V, M, K, D, seed):
    """The oracle half of test_lopq_hip_parity._random_model, draw for draw (that function also builds the library's model, which
    needs the GPU); hip_model() below asserts that the two agree."""
    from oracle import lopq_oracle as O
    rs = np.random.RandomState(seed)
    h, w, nf = D // 2, D // M, M // 2
    Cs = [rs.randn(V, h).astype(np.float32) for _ in range(2)]
    Rs = [np.stack([np.linalg.qr(rs.randn(h, h))[0] for _ in range(V)]) for _ in range(2)]
    mus = [rs.randn(V, h) * 0.05 for _ in range(2)]
    subs = [[rs.randn(K, w) * 0.6 for _ in range(nf)] for _ in range(2)]
    return O.OracleModel(Cs, Rs, mus, subs)


def world(name):
    if name in _worlds:
        return _worlds[name]
    from oracle import lopq_oracle as O
    if name == "r16":
        om, pool = _random_oracle(*R16), None
        M, D = R16[1], R16[3]
        pinv, mu = np.eye(D), np.zeros(D)
    else:
        z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")))
        om = O.OracleModel.from_npz(z)
        M = 2 * int(z["num_fine_splits"])
        pool = np.asarray(z["fine"], dtype=np.uint8) if "fine" in z else None
        if int(z["has_pca"]):
            pinv, mu = np.linalg.pinv(np.asarray(z["pca_P"], dtype=np.float64)), np.asarray(z["pca_mu"], dtype=np.float64)
        else:
            D = 2 * np.asarray(z["Cs"]).shape[2]
            pinv, mu = np.eye(D), np.zeros(D)
    _worlds[name] = dict(om=om, M=M, pool=pool, pinv=pinv, mu=mu)
    return _worlds[name]


def hip_model(name):
    if name not in _hip:
        if name == "r16":
            from test_lopq_hip_parity import _random_model
            _hip[name], om = _random_model(*R16)
            mine = world(name)["om"]
            for a, b in zip(list(om.Cs) + [s for h in om.subquantizers for s in h], list(mine.Cs) + [s for h in mine.subquantizers for s in h]):
                np.testing.assert_array_equal(a, b)
        elif name == "c1":
            from test_gather_dot4 import _world_m4
            _hip[name] = _world_m4()["model"]
        else:
            _hip[name] = LC._world(name)["model"]
    return _hip[name]


# ---- a case's codes, queries and prediction (no GPU) -------------------------------------------------------------------------------------
def near_row(target, M):
    """64 distinct near codes: the target with sub-code l % M moved by 1 + l / M."""
    out = np.tile(target, (64, 1))
    for l in range(64):
        out[l, l % M] = (int(target[l % M]) + 1 + l // M) % 256
    return out


def scale_positions(n):
    lanes = np.arange(64)
    return (lanes * n) >> 6 if n >= 64 else lanes[:n]


def chunk(c):
    """(fine [n][M], query codes [nq][M]) of a case, seeded by its fields."""
    w = world(c.model)
    M = w["M"]
    rs = np.random.RandomState([c.n, M, c.nq, len(c.dist), len(c.form)] + ([] if not c.plant else [len(c.plant[0]), c.plant[1]]))
    if c.dist == "random":
        fine = rs.randint(0, 256, size=(c.n, M)).astype(np.uint8)
    elif c.dist == "resampled":
        fine = w["pool"][rs.randint(0, len(w["pool"]), size=c.n)]
    else:
        # "near": one cluster per query around a centre that is not stored -- 70 % of the codes differ from their centre in one
        # sub-code, the rest in 2 .. M / 2.  The query is the centre: its scale sample meets near codes, as on real data
        assert c.dist == "near" and not c.plant
        centres = rs.randint(0, 256, size=(c.nq, M))
        k = np.where(rs.rand(c.n) < 0.7, 1, rs.randint(2, M // 2 + 1, size=c.n))
        moved = rs.rand(c.n, M).argsort(1) < k[:, None]
        fine = ((centres[rs.randint(0, c.nq, size=c.n)] + np.where(moved, rs.randint(1, 256, size=(c.n, M)), 0)) % 256).astype(np.uint8)
        return fine, centres.astype(np.uint8)
    if not c.plant:
        pos = [c.n - 1] if c.nq == 1 else [c.n // 8, (3 * c.n) // 8, (6 * c.n) // 8, c.n - 1][:c.nq]
        return fine, fine[pos].copy()
    target = rs.randint(0, 256, size=M).astype(np.uint8)
    near = near_row(target, M)
    kind, arg = c.plant
    if kind == "row":  # the 64 codes of row `arg` (fewer in a partial last row)
        k = min(64, c.n - 64 * arg)
        fine[64 * arg:64 * arg + k] = near[:k]
    else:              # kind == "scale": at the scale sample's first 32 positions, shifted by `arg`
        fine[scale_positions(c.n)[:32] + arg] = near[:32]
    others = fine[[c.n // 8, (3 * c.n) // 8, c.n - 1][:c.nq - 1]]
    return fine, np.concatenate([target[None, :], others]).astype(np.uint8)


_predictions = {}


def predict(c):
    """(fine, Q, scan4_model.Slot) of a case."""
    if c in _predictions:
        return _predictions[c]
    from oracle import lopq_oracle as O
    w = world(c.model)
    fine, qcodes = chunk(c)
    wq = dict(w, coarse=np.tile(np.array(CELL, dtype=np.uint16), (len(qcodes), 1)))
    Q = LC._queries(wq, qcodes, range(len(qcodes)), 4 * c.n + c.nq)
    om = w["om"]
    tabs = [np.array(O.subquantizer_distances(om, O.apply_pca(om, x) if om.has_pca else x, CELL)) for x in Q]
    kw = {KNOB_ARG[k][0]: KNOB_ARG[k][1](v) for k, v in c.knobs}
    # The slot builder keeps the items of a query's FIRST visited cell apart from the others (slot_key, csrc/lopq_plan.hip): the queries
    # whose nearest coarse pair is CELL share one slot, the rest another
    first = [tuple(int(v) for v in O.predict_coarse(om, O.apply_pca(om, x) if om.has_pca else x)) == CELL for x in Q]
    groups = [g for g in ([i for i in range(c.nq) if first[i]], [i for i in range(c.nq) if not first[i]]) if g]
    slots = [S4.slot(fine, [tabs[i] for i in g], w["M"], LIMIT, c.form, **kw) for g in groups]
    by_query = {i: (sl.reasons[k], sl.detail[k]) for g, sl in zip(groups, slots) for k, i in enumerate(g)}
    pred = S4.Slot(tuple(by_query[i][0] for i in range(c.nq)), S4.Counters(*(sum(v) for v in zip(*(sl.counters for sl in slots)))),
                   all(sl.decided for sl in slots), [by_query[i][1] for i in range(c.nq)])
    _predictions[c] = (fine, Q, pred)
    return _predictions[c]


# ---- the case lists -----------------------------------------------------------------------------------------------------------------------
LONG_NQ = ((6144, 4), (8705, 3), (20077, 1), (65535, 4))
SHORT_NQ = ((1000, 1), (3000, 4), (4096, 3))
DISTS = (("c4", "random"), ("c4", "resampled"), ("r16", "random"), ("r16", "near"), ("c3", "random"), ("c3", "resampled"), ("c3", "near"),
         ("c1", "random"))
SETTLE = [Case(m, form, n, nq, dist) for m, dist in DISTS for form, sizes in (("long", LONG_NQ), ("short", SHORT_NQ)) for n, nq in sizes]
SETTLE += [Case("r16", "long", 20077, nq, dist) for nq in (3, 4) for dist in ("random", "near")]

# planted sample index t per cell length of the long form (the lengths of test_scan4_sample_ring.py's table); the last t of each length
# also gets the row behind it, which is not sampled
LONG_PLANTS = {6144: (0, 6, 15), 8705: (9, 16), 16384: (21, 31), 20077: (0, 8, 17, 38), 24641: (30, 47), 65535: (64, 70, 127)}
SHORT_PLANTS = (0, 5, 10, 15)  # 4096 codes: 64 rows, sixteen sampled, ksv = 55 <= 64


def _row_cases(model, form, n, ts, nq=1, knobs=()):
    rows, _ = S4.sample_rows(n, form)
    out = [Case(model, form, n, nq, "random", ("row", rows[t]), knobs) for t in ts]
    return out + [Case(model, form, n, nq, "random", ("row", rows[ts[-1]] + 1), knobs)]


ROWS = [c for m in ("c4", "r16") for n, ts in LONG_PLANTS.items() for c in _row_cases(m, "long", n, ts)]
ROWS += _row_cases("c3", "long", 20077, (0, 38)) + _row_cases("r16", "long", 20077, (17,), nq=3)
ROWS += [c for m in ("c4", "r16") for c in _row_cases(m, "short", 4096, SHORT_PLANTS)]
# a short cell whose every row is sampled, the plant in its partial last row: the bound is exact and nothing is verified
EXACT = [Case(m, "short", 1000, 1, "random", ("row", 15)) for m in ("c4", "r16")]

SCALE = [Case(m, form, n, 1, "random", ("scale", shift)) for m, form, n in (("r16", "long", 20077), ("r16", "short", 4096), ("c3", "long", 20077))
         for shift in (0, 1)]

KNOB_ROWS = [c._replace(knobs=knobs) for knobs in ((("CIS_S4_FRAC", "16"),), (("CIS_S4_NSX", "16"),))
             for c in _row_cases("c4", "long", 20077, (8, 17, 38)) + _row_cases("r16", "long", 65535, (70, 127))]
M16_SETTLE = [c for c in SETTLE if c.model in ("r16", "c3")]
KNOB_SAT = [c._replace(knobs=(("CIS_S4_SAT", s),)) for s in ("0.5", "0.95", "1.5") for c in M16_SETTLE if (c.n, c.nq) in ((20077, 1), (20077, 4), (4096, 3))]

CASES = {"settle": SETTLE, "rows": ROWS, "exact": EXACT, "scale": SCALE, "knob_rows": KNOB_ROWS, "knob_sat": KNOB_SAT}


def expected_reason(c):
    """What a list's case is built to show, for the query the plant is aimed at (None: whatever the model says)."""
    if not c.plant:
        return None if c.knobs else "settles"
    if c.knobs:
        return None
    kind, arg = c.plant
    if kind == "scale":
        return "no_bound" if arg == 0 else "settles"
    rows, ns = S4.sample_rows(c.n, c.form)
    if ns == (c.n + 63) // 64:
        return "settles"  # every row sampled: exact
    if arg in rows:
        return "failed_verification"
    # (short form: the 64 near codes of an unsampled row sit in one wave's quarter of 126 entries, which may overflow)
    return "settles" if c.form == "long" else None


# ---- the GPU half ----------------------------------------------------------------------------------------------------------------------------
def _run(monkeypatch, capfd, c):
    fine, Q, pred = predict(c)
    assert pred.decided, "the model calls the case decided (asserted before the first launch)"
    want = expected_reason(c)
    assert want is None or (pred.reasons[0] == want and all(r == "settles" for r in pred.reasons[1:]))
    w = world(c.model)
    wd = dict(w, model=hip_model(c.model), coarse=np.tile(np.array(CELL, dtype=np.uint16), (c.n, 1)))
    monkeypatch.setattr(LC, "QUOTA", c.n)  # the query visits this cell alone
    if c.form == "long":
        monkeypatch.setenv("CIS_SEG_MAX", "65536")
    monkeypatch.setenv("CIS_SCAN4_DEBUG", "1")
    for k, v in c.knobs:
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    LC._check(wd, fine, Q, modes=(5,))  # asserts last_stats()["scan_kernel"] == "k_adc_scan4", mode 1 bit for bit, the oracle
    lines, got = S4.parse_debug(capfd.readouterr().err)
    print("%s: model %s %s; kernel %s" % (case_id(c), pred.reasons, tuple(pred.counters), tuple(got)))
    assert len(lines) == 1, "one launch of the sampled form"
    assert got == pred.counters


@pytest.mark.parametrize("c", SETTLE, ids=case_id)
def test_codes_that_settle(monkeypatch, capfd, c):
    _run(monkeypatch, capfd, c)
    assert predict(c)[2].counters.fallbacks == 0


@pytest.mark.parametrize("c", ROWS + EXACT, ids=case_id)
def test_planted_sample_row(monkeypatch, capfd, c):
    _run(monkeypatch, capfd, c)


@pytest.mark.parametrize("c", SCALE, ids=case_id)
def test_planted_scale_sample(monkeypatch, capfd, c):
    _run(monkeypatch, capfd, c)


@pytest.mark.parametrize("c", KNOB_ROWS + KNOB_SAT, ids=case_id)
def test_knobs_move_the_prediction_with_the_kernel(monkeypatch, capfd, c):
    _run(monkeypatch, capfd, c)
