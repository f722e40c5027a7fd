"""GPU: the 16-bit table sums of the batch scans (csrc/lopq_scan3.hip) added as plain integers -- four queries' fields with one 64-bit
add (add16x4) -- at the places where a field is as full as it can get.

No field may carry into its neighbour: every staged entry is <= CAP = 65535 / M and a sum has M terms.  The cases put a field at that
edge next to live fields and ask for the answers of the float64 kernel and the oracle, and that the sampled form settled its slots:

  present   slots with 1, 2, 3 and 4 present queries, M = 4, 8 and 16: the absent queries' entries are CAP itself, so their fields hold
            M * CAP = 65532 / 65528 / 65520 for every candidate, next to the present queries' sums
  flat      a model whose sub-codebooks are all the same and a query whose projected residual has the same sub-vector in every position:
            its M tables are one table, the largest entry of each is the largest of all (staged as CAP - 1, or CAP on the saturating
            scale), and a planted code that takes that entry in every position sums to M (CAP - 1) or more.  The query next to it in the
            slot is the planted code's own reconstruction: its sum for the planted code is near 0.  The flat query stands at place 0,
            1, 2 and 3 of the slot in turn.  tests/scan4_model.py's sums, computed before the launch, must put the planted sum at
            65535 - 4 M or above

Every case is one cell that is one chunk and one slot, built as in tests/test_scan4_settles.py: short chunks (the 504-entry form) and
long chunks of more than 504 rows (the 1016-entry form, two table copies at M = 8; CIS_SEG_MAX=65536).  Each runs the sampled form
(mode 5, k_adc_scan4) and k_adc_scan3 (mode 4) against the float64 scan kernel bit for bit and the queries against the oracle
(test_scan4_long_chunks._check); the CIS_SCAN4_DEBUG line of the mode-5 launch must show one slot and none handed to the fall-back, as
scan4_model predicts (asserted before the launch: the case is decided, one slot, no fall-back)."""
from collections import namedtuple

import numpy as np
import pytest

import scan4_model as S4
import test_scan4_long_chunks as LC
import test_scan4_settles as ST

pytestmark = pytest.mark.gpu

LIMIT = ST.LIMIT
CELL = ST.CELL
N = {"short": 4001, "long": 32333}  # 63 rows, the last one partial; 506 rows (> 504), the last one partial
MODELS = {4: "c1", 8: "c4", 16: "r16"}


# ---- the GPU half: test_scan4_settles._run with k_adc_scan3 (mode 4) compared as well --------------------------------------------------
def _gpu(monkeypatch, capfd, w, model, form, fine, Q, pred, label):
    assert pred.decided, "the model calls the case decided (asserted before the first launch)"
    assert pred.counters.slots == 1 and pred.counters.fallbacks == 0, "one slot that settles: %s" % (pred.reasons,)
    n = len(fine)
    wd = dict(w, model=model, coarse=np.tile(np.array(CELL, dtype=np.uint16), (n, 1)))
    monkeypatch.setattr(LC, "QUOTA", n)  # the query visits this cell alone
    if form == "long":
        monkeypatch.setenv("CIS_SEG_MAX", "65536")
    monkeypatch.setenv("CIS_SCAN4_DEBUG", "1")
    capfd.readouterr()
    LC._check(wd, fine, Q, modes=(5, 4))  # mode 5 ran k_adc_scan4; modes 5 and 4 equal mode 1 bit for bit; mode 1 equals the oracle
    lines, got = S4.parse_debug(capfd.readouterr().err)
    print("%s: model %s %s; kernel %s" % (label, pred.reasons, tuple(pred.counters), tuple(got)))
    assert len(lines) == 1, "one launch of the sampled form"
    assert got == pred.counters
    assert got.fallbacks == 0


# ---- present: 1 .. 4 present queries ----------------------------------------------------------------------------------------------------
Present = namedtuple("Present", "M form nq")
PRESENT = [Present(M, form, nq) for M in (4, 8, 16) for form in ("short", "long") for nq in (1, 2, 3, 4)]
_present_cases = {}


def present_id(c):
    return "m%d-%s-nq%d" % c


def present_case(c):
    """(fine, Q, prediction): uniformly random codes and nq queries, perturbed reconstructions of stored codes whose nearest coarse
    pair is the cell itself -- the slot builder keeps the items of a query's first visited cell apart from the others
    (test_scan4_settles.predict), and the nq queries are to share ONE slot."""
    if c in _present_cases:
        return _present_cases[c]
    from oracle import lopq_oracle as O
    w = ST.world(MODELS[c.M])
    om, n = w["om"], N[c.form]
    assert w["M"] == c.M
    rs = np.random.RandomState([c.M, n, c.nq])
    fine = rs.randint(0, 256, size=(n, c.M)).astype(np.uint8)
    wq = dict(w, coarse=np.tile(np.array(CELL, dtype=np.uint16), (n, 1)))
    Q = []
    for row in range(n // 8, n, 397):
        x = LC._queries(wq, fine, [row], 4 * n + row)[0]
        if tuple(int(v) for v in O.predict_coarse(om, O.apply_pca(om, x) if om.has_pca else x)) == CELL:
            Q.append(x)
        if len(Q) == c.nq:
            break
    assert len(Q) == c.nq
    Q = np.ascontiguousarray(np.array(Q, dtype=np.float64))
    tabs = [np.array(O.subquantizer_distances(om, O.apply_pca(om, x) if om.has_pca else x, CELL)) for x in Q]
    _present_cases[c] = (fine, Q, S4.slot(fine, tabs, c.M, LIMIT, c.form))
    return _present_cases[c]


@pytest.mark.parametrize("c", PRESENT, ids=present_id)
def test_absent_queries_hold_full_fields_next_to_live_ones(monkeypatch, capfd, c):
    fine, Q, pred = present_case(c)
    assert len(pred.reasons) == c.nq and S4.cap(c.M) * c.M == {4: 65532, 8: 65528, 16: 65520}[c.M]
    _gpu(monkeypatch, capfd, ST.world(MODELS[c.M]), ST.hip_model(MODELS[c.M]), c.form, fine, Q, pred, present_id(c))


# ---- flat: one table in every position, a planted code at its largest entry ----------------------------------------------------------------
Flat = namedtuple("Flat", "M form place")
FLAT = [Flat(M, form, place) for M in (4, 8, 16) for form in ("short", "long") for place in (0, 1, 2, 3)]
W_SUB, V_FLAT, K_FLAT = 4, 16, 256
_flat_worlds, _flat_hip, _flat_cases = {}, {}, {}


def flat_id(c):
    return "m%d-%s-place%d" % c


def _flat_parameters(M):
    """Sixteen coarse centroids per half, far apart; identity rotations and zero means, so that the projected residual of x is x minus
    its centroid, exactly; ONE sub-codebook of 256 centroids in four dimensions for every position."""
    rs = np.random.RandomState(4100 + M)
    h, nf = M * W_SUB // 2, M // 2
    Cs = [(3.0 * rs.randn(V_FLAT, h)).astype(np.float32) for _ in range(2)]
    Rs = [np.stack([np.eye(h) for _ in range(V_FLAT)]) for _ in range(2)]
    mus = [np.zeros((V_FLAT, h)) for _ in range(2)]
    sub = np.round(0.3 * rs.randn(K_FLAT, W_SUB) * 1024.0) / 1024.0  # (a few bits each: centroid + sub-vector - centroid is exact)
    subs = [[sub.copy() for _ in range(nf)] for _ in range(2)]
    return Cs, Rs, mus, subs


def flat_world(M):
    if M not in _flat_worlds:
        from oracle import lopq_oracle as O
        Cs, Rs, mus, subs = _flat_parameters(M)
        D = M * W_SUB
        _flat_worlds[M] = dict(om=O.OracleModel(Cs, Rs, mus, subs), M=M, pool=None, pinv=np.eye(D), mu=np.zeros(D), sub=subs[0][0])
    return _flat_worlds[M]


def flat_hip_model(M):
    if M not in _flat_hip:
        from columbiaimagesearch_amd.lopq import LOPQModel
        Cs, Rs, mus, subs = _flat_parameters(M)
        _flat_hip[M] = LOPQModel(parameters=(tuple(Cs), tuple(Rs), tuple(mus), tuple(tuple(s) for s in subs)))
    return _flat_hip[M]


def flat_case(c):
    """(fine, Q, prediction, planted position, planted 16-bit sum of the flat query) -- no GPU."""
    if c in _flat_cases:
        return _flat_cases[c]
    from oracle import lopq_oracle as O
    w = flat_world(c.M)
    om, M, sub, n = w["om"], c.M, w["sub"], N[c.form]
    rs = np.random.RandomState([M, n, c.place])
    fine = rs.randint(0, 256, size=(n, M)).astype(np.uint8)
    # the flat query: the same sub-vector r (near sub-centroid 17) in every position, around the cell's centroids
    r = sub[17] + np.round(0.02 * rs.randn(W_SUB) * 1024.0) / 1024.0
    flat_q = np.concatenate([om.Cs[s][CELL[s]].astype(np.float64) + np.tile(r, M // 2) for s in range(2)])
    tab = ((r[None, :] - sub) ** 2).sum(1)
    k_far = int(np.argmax(tab))
    planted = n // 2 + 77
    fine[planted] = k_far
    # its neighbour in the slot (the field the flat query's would carry into; below it for the last place): the planted code's own
    # reconstruction, slightly perturbed -- a near-duplicate of the planted code; the other two places: reconstructions of other codes
    neighbour = c.place + 1 if c.place < 3 else 2
    others = [p for p in range(4) if p not in (c.place, neighbour)]
    rows = {neighbour: planted, others[0]: n // 8, others[1]: n - 1}
    wq = dict(w, coarse=np.tile(np.array(CELL, dtype=np.uint16), (n, 1)))
    Q = np.empty((4, M * W_SUB), dtype=np.float64)
    Q[c.place] = flat_q
    for p, row in rows.items():
        Q[p] = LC._queries(wq, fine, [row], 7000 + 10 * M + p)[0]
    tabs = [np.array(O.subquantizer_distances(om, x, CELL)) for x in Q]
    for j in range(1, M):  # flat: one table in every position, bit for bit
        np.testing.assert_array_equal(tabs[c.place][j], tabs[c.place][0])
    assert all(tuple(int(v) for v in O.predict_coarse(om, x)) == CELL for x in Q), "the four queries share the cell's slot"
    pred = S4.slot(fine, tabs, M, LIMIT, c.form)
    x = pred.detail[c.place]
    big = int(S4.sums(fine[planted:planted + 1], S4.tables32(tabs[c.place]), S4.F(x["qinv"]), M)[0])
    y = pred.detail[neighbour]
    small = int(S4.sums(fine[planted:planted + 1], S4.tables32(tabs[neighbour]), S4.F(y["qinv"]), M)[0])
    _flat_cases[c] = (fine, Q, pred, planted, big, small)
    return _flat_cases[c]


@pytest.mark.parametrize("c", FLAT, ids=flat_id)
def test_a_full_field_next_to_a_near_duplicate(monkeypatch, capfd, c):
    fine, Q, pred, planted, big, small = flat_case(c)
    print("%s: planted sum %d of 65535 (bar %d), the neighbour's %d" % (flat_id(c), big, 65535 - 4 * c.M, small))
    assert big >= 65535 - 4 * c.M, "the planted code fills the flat query's field"
    assert big <= 65535 and small <= 2 * c.M, "and the neighbouring query's sum for it is near 0"
    _gpu(monkeypatch, capfd, flat_world(c.M), flat_hip_model(c.M), c.form, fine, Q, pred, flat_id(c))
