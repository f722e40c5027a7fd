"""No GPU: tests/scan4_model.py itself, and the case lists of tests/test_scan4_settles.py -- every case decided, every list showing what it
is there to show, the planted sample rows covering the ring."""
import numpy as np
import pytest

import scan4_model as S4
import test_scan4_settles as T


def test_bracket_property():
    """Unsaturated sums bracket the scaled distance: s <= d * qinv < s + M; a clamped entry keeps only the lower bound."""
    rs = np.random.RandomState(4)
    for M in (4, 8, 16):
        tabs = rs.rand(M, 256) ** 3
        fine = rs.randint(0, 256, size=(5000, M)).astype(np.uint8)
        t32 = S4.tables32(tabs)
        d = t32[np.arange(M)[None, :], fine].astype(np.float64).sum(1)
        q0 = S4.q0_of(t32, M)
        assert (t32 * q0).astype(np.float32).max() < S4.cap(M), "the tables' own scale clamps nothing"
        for qinv in (q0, np.float32(4.0) * q0):
            s = S4.sums(fine, t32, qinv, M)
            ent = (t32 * np.float32(qinv)).astype(np.float32)
            clean = (ent[np.arange(M)[None, :], fine] < S4.cap(M)).all(1)
            x = d * float(qinv)
            slack = 1e-6 * x + 1e-9  # float32 products against the float64 restatement
            assert (s <= x + slack).all()
            assert (x[clean] < s[clean] + M + slack[clean]).all()
            assert clean.all() == (qinv == q0) and clean.any()


def test_sample_rows_and_ranks():
    """The docstring table of test_scan4_sample_ring.py, and the rank of its 20077-code cell."""
    for n, nrows, ns, rounds in ((6144, 96, 16, 1), (8705, 137, 17, 2), (16384, 256, 32, 2), (20077, 314, 39, 3), (24641, 386, 48, 3),
                                 (65536, 1024, 128, 8), (65535, 1024, 128, 8), (1025, 17, 16, 1), (1000, 16, 16, 1), (64, 1, 1, 1), (1, 1, 1, 1)):
        rows, got = S4.sample_rows(n, "long")
        assert (got, -(-got // 16), (n + 63) // 64) == (ns, rounds, nrows)
        assert rows == [(t * nrows) // ns for t in range(ns)] and len(set(rows)) == ns and rows[-1] < nrows
    assert S4.sample_rows(20077, "long", frac=16)[1] == 19 and S4.sample_rows(20077, "long", nsx=16)[1] == 16
    assert S4.sample_rows(4096, "short")[0] == list(range(0, 64, 4))
    assert S4.ksv_of(100, 39 * 64, 20077, 4.5) == 42
    assert S4.ksv_of(100, 16 * 64, 4096, 4.0) == 55
    assert [S4.sample_place(t) for t in (0, 3, 4, 16, 21, 38, 127)] == [(0, 0, 0, 0), (0, 1, 0, 1), (1, 0, 0, 0), (0, 2, 1, 0), (1, 2, 1, 1),
                                                                         (1, 1, 2, 0), (3, 3, 7, 1)]
    assert list(S4.wave_of([0, 127, 128, 511, 512])) == [0, 0, 1, 3, 0]


def test_debug_line():
    err = ("x\n[cis] k_adc_scan4: 3 slots, 2 to the fall-back list (lists: 1 overflowed, 4 failed the verification, 5 crowds at the cut; "
           "6 slots with items of different chunks)\n") * 2
    lines, total = S4.parse_debug(err)
    assert lines == [S4.Counters(3, 2, 1, 4, 5, 6)] * 2 and total == S4.Counters(6, 4, 2, 8, 10, 12)
    assert S4.parse_debug("nothing")[0] == []


ALL = [(name, c) for name, cases in T.CASES.items() for c in cases]


@pytest.mark.parametrize("name,c", ALL, ids=[n + ":" + T.case_id(c) for n, c in ALL])
def test_every_gpu_case_is_decided_and_shows_what_it_is_for(name, c):
    fine, Q, pred = T.predict(c)
    assert pred.decided
    assert len(fine) == c.n and len(Q) == c.nq == len(pred.reasons)
    want = T.expected_reason(c)
    if want is not None:
        assert pred.reasons[0] == want, pred.detail[0]
        assert all(r == "settles" for r in pred.reasons[1:])
    elif c.plant and not c.knobs:
        assert pred.reasons[0] in ("settles", "overflowed")  # an unsampled row never fails the verification
    if c.plant and c.plant[0] == "row":
        assert c.plant[1] * 64 < c.n and len(set(map(bytes, fine[64 * c.plant[1]:64 * c.plant[1] + 64]))) == min(64, c.n - 64 * c.plant[1])


def test_m16_settle_cases_run_on_both_scales():
    """Random codes stay on the tables' own scale, near codes take the saturating one: both rules of the bound are in the list."""
    taken = {(c.dist, x["taken"]) for c in T.M16_SETTLE for x in T.predict(c)[2].detail}
    assert taken >= {("random", False), ("resampled", False), ("near", True)} and ("near", False) not in taken and ("random", True) not in taken
    # ... and on its own scale a query's threshold may lie above the entry cap (what the rule for clamped entries would refuse)
    assert any(x["tau"] >= S4.cap(16) for c in T.M16_SETTLE if c.dist == "random" for x in T.predict(c)[2].detail)


def test_planted_rows_cover_the_ring():
    """(wave, register set, round) of the planted sample rows of the long form: every wave, every set, the first, a middle and the last
    round of one length, and a last round that holds one row."""
    got = set()
    for c in T.ROWS:
        rows, ns = S4.sample_rows(c.n, c.form)
        if c.form == "long" and c.plant[1] in rows:
            t = rows.index(c.plant[1])
            got.add((c.n, ns) + S4.sample_place(t)[:3])
    triples = {g[2:] for g in got}
    assert triples == {(0, 0, 0), (1, 1, 0), (3, 1, 0), (2, 0, 0), (0, 2, 1), (1, 2, 1), (3, 3, 1), (1, 1, 2), (3, 3, 1), (3, 1, 2),
                       (0, 0, 4), (1, 1, 4), (3, 3, 7)}, sorted(triples)
    assert {w for w, _, _ in triples} == {0, 1, 2, 3} and {s for _, s, _ in triples} == {0, 1, 2, 3}
    assert {r for n, ns, w, s, r in got if n == 20077} == {0, 1, 2}       # first, middle, last of three rounds
    assert (8705, 17, 0, 2, 1) in got                                      # the last round's only row
    assert (65535, 128, 3, 3, 7) in got                                    # the last row of the cap's eighth round
    short = {rows.index(c.plant[1]) // 4 for c in T.ROWS if c.form == "short" for rows in [S4.sample_rows(c.n, "short")[0]] if c.plant[1] in rows}
    assert short == {0, 1, 2, 3}  # short form: sample t on wave t / 4


def test_knobs_change_the_prediction():
    """CIS_S4_FRAC / CIS_S4_NSX: at least one planted row is sampled under one setting and not under the other; CIS_S4_SAT: 0.5 and 0.95
    settle what 0.75 settles, and 1.5 leaves queries without a bound."""
    for knob in ("CIS_S4_FRAC", "CIS_S4_NSX"):
        cases = [c for c in T.KNOB_ROWS if c.knobs[0][0] == knob]
        assert any(T.predict(c)[2].counters != T.predict(c._replace(knobs=()))[2].counters for c in cases), knob
    for c in T.KNOB_SAT:
        pred = T.predict(c)[2]
        if c.knobs[0][1] in ("0.5", "0.95"):
            assert pred.counters.fallbacks == 0 and set(pred.reasons) == {"settles"}, T.case_id(c)
    high = [T.predict(c)[2] for c in T.KNOB_SAT if c.knobs[0][1] == "1.5"]
    assert any(r in ("no_bound", "overflowed") for p in high for r in p.reasons)
    assert all(p.counters.fallbacks >= 1 for p in high if set(p.reasons) & {"no_bound", "overflowed"})
