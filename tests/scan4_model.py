"""A numpy restatement of the decisions k_adc_scan4 (csrc/lopq_scan3.hip) makes for one slot -- not of the kernel.

A slot is one chunk of fine codes and up to four queries.  For every query the kernel guesses a scale (M = 16), a threshold tau from a
sample of rows and a list of the sums up to tau + M + 1, verifies the guess and hands the whole slot to the fall-back list when any
query's guess fails.  The fall-back gives the same answer, so only the counters of CIS_SCAN4_DEBUG show whether the guesses held; this
module predicts them from the oracle's float64 half tables:

    slot(fine, tabs, M, L, form, z=..., frac=8, nsx=128, sat=0.75) -> Slot

    .reasons    per query: settles | overflowed | failed_verification | no_bound | crowd_at_cut
    .counters   what one slot adds to the debug line: (slots, fall-backs, overflowed, failed the verification, crowds at the cut)
    .decided    the reasons and counters are the same at qinv * (1 - 1e-5), qinv and qinv * (1 + 1e-5)

The device forms the scale's distances in float32 from float32 tables, sixteen non-negative addends, so its qinv may differ from this
one by about 17 * 2^-24 relative; a case whose outcome changes inside +- 1e-5 is not decided and no GPU test may use it.

What is restated (line numbers drift; the names are the source's):
  - q0 = float32(CAP / mxT) * (1 - 2^-20), mxT the largest float32 entry of the query's two half tables; CAP = 65535 / M
  - M = 16 (sat > 0): candidates c = (lane * len) >> 6 (lane when len < 64), rank rk = min(48, 4 + ceil(64 L / len)),
    qs = sat * CAP / d_rk, taken only when qs > q0.  Only a query whose qs was TAKEN has clamped entries and so the rules "tau below
    CAP - M - 2" and "cut below CAP"; a query left on q0 is treated like M <= 8
  - entries: float32 table entry * float32 qinv in float32, truncated, clamped to CAP
  - short form: min(nrows, 16) sample rows t * nrows / ns, all their sums; long form: ns = clamp(nrows / frac, 16, nsx) rows, the
    4 x 64 bucket minima, row t in bucket (wave (t / 4) % 4, lane); rank ksv = int(rt^2) + 1, rt the root of k - z sqrt(k) = L nsam / len
  - have_bound, keep = tau + M + 1, verify
  - main pass: wave w scans blocks [128 i, 128 i + 128) with i % 4 == w and records at most PCAP positions that pass for ANY query;
    second gather: each wave's quarter (WCAP = LCAP / 4) of each query's list
  - verification (at least L sums at or below tau), the cut's bisection (stops within L + 16), the cut checks
"""
import re
from collections import namedtuple

import numpy as np

F = np.float32
NW, G, NS_MIN, U = 4, 4, 16, 2
LCAP = {"short": 504, "long": 1016}
Z_DEFAULT = {"short": 4.0, "long": 4.5}
REASONS = ("settles", "overflowed", "failed_verification", "no_bound", "crowd_at_cut")
EPS = 1e-5

DEBUG_RE = re.compile(r"k_adc_scan4: (\d+) slots, (\d+) to the fall-back list \(lists: (\d+) overflowed, (\d+) failed the verification, "
                      r"(\d+) crowds at the cut; (\d+) slots with items of different chunks\)")
Counters = namedtuple("Counters", "slots fallbacks overflowed failed_verification crowds mixed")
Slot = namedtuple("Slot", "reasons counters decided detail")


def parse_debug(err):
    """Every CIS_SCAN4_DEBUG line of `err` (one per k_adc_scan4 launch) as Counters, and their sum."""
    lines = [Counters(*map(int, m)) for m in DEBUG_RE.findall(err)]
    total = Counters(*(sum(c) for c in zip(*lines))) if lines else Counters(0, 0, 0, 0, 0, 0)
    return lines, total


def cap(M):
    return 65535 // M


def wave_of(p):
    """Wave that scans position p in the main pass (U = 2 rows of 64 per iteration, iterations dealt round robin)."""
    return (np.asarray(p) // (64 * U)) % NW


def pcap(M, form):
    """Positions a wave can record in the main pass."""
    if form == "short":
        return 512
    return 768 if M == 8 else 1024  # (M = 8: the two-copy form keeps 24 registers of positions per slot)


def sample_rows(n, form, frac=8, nsx=128):
    """(rows, ns): the sampled rows t * nrows / ns of a chunk of n codes."""
    nrows = (n + 63) >> 6
    if form == "short":
        ns = min(nrows, NS_MIN)
    else:
        ns = min(min(max(nrows // frac, NS_MIN), nsx), nrows)
    return [(t * nrows) // ns for t in range(ns)], ns


def sample_place(t):
    """(wave, ring set, round, row of the set) of sample t in the long form: rounds of sixteen rows, four per wave, a wave's rows in a
    ring of SD = 4 register sets of SRS = 2 rows."""
    rnd, wave, i = t // 16, (t // 4) % 4, t % 4
    j = rnd * 4 + i  # the wave's j-th row
    return wave, (j // 2) % 4, rnd, j % 2


def ksv_of(L, nsam, n, z):
    """Sample rank with k - z sqrt(k) >= L nsam / n, in the kernel's float32 steps."""
    need = F(L) * F(nsam) / F(n)
    hz = F(0.5) * F(z)
    rt = hz + np.sqrt(F(hz * hz + need), dtype=F)
    return int(F(rt * rt)) + 1


def tables32(tabs):
    return np.asarray(tabs, dtype=np.float64).astype(F)  # [M][K]


def q0_of(t32, M):
    mx = max(F(t32.max()), F(1e-30))
    return F(F(cap(M)) / mx) * F(1.0 - 9.5367431640625e-7)


def scale(fine, t32, M, L, sat):
    """(qinv, taken, margin): the query's scale; margin is how far qs is from q0, relative (a scale inside EPS of q0 is undecided)."""
    n = len(fine)
    q0 = q0_of(t32, M)
    if not sat > 0:
        return q0, False, 1.0
    lanes = np.arange(64)
    c = (lanes * n) >> 6 if n >= 64 else lanes
    c = c[c < n]
    d = np.sort(t32[np.arange(M)[None, :], fine[c]].astype(np.float64).sum(1))
    rk = min(48, 4 + (64 * L + n - 1) // n)
    d_rk = d[rk - 1] if rk <= len(d) else 3.4e38
    qs = F(F(sat) * F(cap(M))) / max(F(d_rk), F(1e-30))
    taken = bool(q0 > 0 and qs > q0 and qs < 3.0e38 and d_rk < 1.0e38)
    return (qs if taken else q0), taken, abs(float(qs) / float(q0) - 1.0)


def sums(fine, t32, qinv, M):
    ent = np.minimum((t32 * F(qinv)).astype(F).astype(np.int64), cap(M))  # float32 product, truncated, clamped
    return ent[np.arange(M)[None, :], fine].sum(1)


def _threshold(s, n, M, L, form, z, frac, nsx, saturating):
    """(tau, have_bound, keep, verify, ksv) of one query from its sums s."""
    CAP = cap(M)
    nrows = (n + 63) >> 6
    rows, ns = sample_rows(n, form, frac, nsx)
    every = ns == nrows
    if form == "short":
        pos = np.concatenate([np.arange(r * 64, min(r * 64 + 64, n)) for r in rows])
        sample = np.sort(s[pos])
        nsam = len(sample)
    else:
        bm = np.full((NW, 64), 65535, dtype=np.int64)
        for t, r in enumerate(rows):
            row = s[r * 64:min(r * 64 + 64, n)]
            w = (t // 4) % NW
            bm[w, :len(row)] = np.minimum(bm[w, :len(row)], row)
        sample = np.sort(bm.ravel())
        nsam = n if every else ns * 64
    ksv = L if every else ksv_of(L, nsam, n, z)
    tau, have = 65534, False
    if nsam >= ksv:
        tau = min(int(sample[ksv - 1]), 65534) if ksv <= len(sample) else 65534
        have = tau < (CAP - M - 2 if saturating else 65534)
    keep = min(tau + M + 1, 65534) if have else 65534
    return tau, have, keep, bool(have and keep < 65534 and not every), ksv


def _cut(ls, L):
    """The value the verification's bisection stops at: some v with at least L and (ties aside) at most L + 16 sums at or below it."""
    lo, hi = int(ls.min()), int(ls.max())
    while lo < hi:
        p = lo + ((hi - lo) >> 1)
        c = int((ls <= p).sum())
        if c >= L:
            hi = p
            if c <= L + 16:
                break
        else:
            lo = p + 1
    return hi


def _slot_at(fine, t32s, M, L, form, z, frac, nsx, sat, factor, S):
    n, ng, CAP = len(fine), len(t32s), cap(M)
    wcap = LCAP[form] // NW
    wave = wave_of(np.arange(n))
    q = []
    for t32 in t32s:
        qinv, taken, margin = scale(fine, t32, M, L, sat)
        s = sums(fine, t32, F(float(qinv) * factor), M)
        q.append(dict(s=s, taken=taken, margin=margin, qinv=float(qinv)))
        q[-1].update(zip(("tau", "have", "keep", "verify", "ksv"), _threshold(s, n, M, L, form, z, frac, nsx, taken)))
    passing = np.zeros(n, dtype=bool)
    for x in q:
        passing |= x["s"] <= x["keep"]
    pover = [int(passing[wave == w].sum()) > pcap(M, form) for w in range(NW)]
    reasons, over, failed, crowds = [], 0, 0, 0
    for g, x in enumerate(q):
        s = x["s"]
        listed = s <= x["keep"]
        wtot = [0 if pover[w] else int(listed[wave == w].sum()) for w in range(NW)]
        if g == 0:
            wtot = [wcap + 1 if pover[w] else wtot[w] for w in range(NW)]  # a full position list is reported through query 0
        ls = s[listed & ~np.isin(wave, [w for w in range(NW) if pover[w]])]
        x.update(listed=int(sum(wtot)), under_tau=int((ls <= x["tau"]).sum()))
        if max(wtot) > wcap:
            over += 1
            reasons.append("overflowed" if x["have"] else "no_bound")
            continue
        if x["verify"] and x["under_tau"] < L:
            failed += 1
            reasons.append("failed_verification")
            continue
        bad, cut = False, 65535
        if len(ls) >= L:
            cut = _cut(ls, L) + M + 1
            if x["taken"] and cut >= CAP:
                bad = True
                crowds += 1
        elif x["taken"] and len(ls) and int(ls.max()) + M + 1 >= CAP:
            bad = True
            crowds += 1
        if form == "long" and int((ls <= cut).sum()) > S:
            bad = True
            crowds += 1
        x["cut"] = cut
        reasons.append("crowd_at_cut" if bad else "settles")
    fell = any(r != "settles" for r in reasons)
    return tuple(reasons), Counters(1, int(fell), over, failed, crowds, 0), q


def slot(fine, tabs, M, L, form, z=None, frac=8, nsx=128, sat=0.75, S=992):
    """One slot: `fine` [n][M] uint8, the chunk; `tabs` a list of one to four queries' half tables [M][K] (float64, the oracle's
    subquantizer_distances of the projected query); form "short" or "long".  sat is used at M = 16 only, as in the library; S is the
    survivor row of an item (992 entries up to limit 184)."""
    assert form in LCAP and 1 <= len(tabs) <= G and fine.ndim == 2 and fine.shape[1] == M and 1 <= len(fine) <= 65536
    z = Z_DEFAULT[form] if z is None else z
    sat = sat if M == 16 else 0.0
    t32s = [tables32(t) for t in tabs]
    runs = [_slot_at(fine, t32s, M, L, form, z, frac, nsx, sat, f, S) for f in (1.0 - EPS, 1.0, 1.0 + EPS)]
    reasons, counters, detail = runs[1]
    decided = all(r[0] == reasons and r[1] == counters for r in runs) and all(x["margin"] > 2 * EPS for x in detail)
    return Slot(reasons, counters, decided, detail)
