"""GPU: the sample pass of k_adc_scan4's long-chunk form (csrc/lopq_scan3.hip) at the places where its register ring can go wrong.

The long-chunk form samples ns = min(nrows, clamp(nrows / 8, 16, 128)) of a chunk's nrows = ceil(len / 64) rows, row t * nrows / ns for
sample t, in rounds of sixteen rows (four per wave).  A wave's rows travel in a ring of four register sets of two rows, requested eight
rows ahead, so the cells below are chosen by the number of rounds (a wave's rows: four per round, fewer in the last):

    len      nrows   ns  rounds
    6144        96   16    1     the ring is deeper than the loop
    8705       137   17    2     the second round holds one row, on wave 0 only; the chunk's last row is partial
    16384      256   32    2     exactly full rounds
    20077      314   39    3     odd number of rounds, the last one partly filled
    24641      386   48    3     full rounds, the chunk's last row partial
    65536     1024  128    8     the cap of 128 sample rows
    65535     1024  128    8     the same with a partial last row
    1, 64, 1000  <= 16 rows: every row is sampled (the bound is valid by itself)
    1025        17   16    1     the chunk's last row is never sampled

A wrong sample still gives exact results -- the verification sends the slot to the fall-back -- so every case also pins the number of
slots that k_adc_scan4 hands to the fall-back list (CIS_SCAN4_DEBUG prints it per launch) to what the build before the ring reported for
the same case, measured with that build's library on the same queries: 0 in every case (random codes without duplicates).  The two
M = 16 cases used to send every slot to the fall-back (1 of 1 and 3 of 3) and so could not tell a wrong sample from a right one.  The
reason was the kernel's: uniformly random codes are all far from a query, their scale sample asks for a COARSER scale than the tables'
own, the query stays on its own scale -- and was still held to the saturating scale's rule that tau lie below CAP - M - 2 = 4077, while
sixteen unclamped entries put the limit-th sum at 4100 .. 4900 for three of the four queries.  Without a bound such a query lists every
candidate: the position lists overflow (counted once, through query 0) and the one query that had a bound finds its list empty (1
overflowed, 1 failed the verification in the 20077 cell).  Only a query that TOOK the saturating scale has clamped entries; with the
rule applied to those alone both cells settle, and tests/scan4_model.py predicts both sets of counters.  Each case
aims four queries (a full slot) or one (a partly filled slot) at a cell, compares the sampled form (scan mode 5) with the float64 scan
kernel (mode 1) bit for bit and the queries with the oracle (_check of test_scan4_long_chunks.py), and asserts that the batch ran the
long-chunk form: with CIS_SEG_MAX=65536 a cell is one chunk, and scan3_geom takes that form from 6144 candidates per work item on.  The
short cells sit beside the two 65 k cells for that reason: a query visits cells until it has seen 10000 candidates, so whatever the
order, its items average more than 6144."""
import numpy as np
import pytest

from scan4_model import parse_debug
from test_scan4_long_chunks import _check, _queries, _world

pytestmark = pytest.mark.gpu

# world -> (fixture, ((coarse cell, codes), ...)); no world holds more than ~150 k codes
WORLDS = {
    "rounds": ("c4", (((2, 5), 6144), ((7, 1), 8705), ((11, 13), 16384), ((4, 9), 20077), ((14, 3), 24641))),
    "cap": ("c4", (((2, 5), 65536), ((7, 1), 65535), ((11, 13), 1), ((4, 9), 64), ((14, 3), 1000), ((9, 9), 1025))),
    "m16": ("c3", (((2, 5), 20077), ((7, 1), 8705))),
}
# slots handed to the fall-back list by the build before the ring, per (world, cell length, queries)
PARENT_FALLBACKS = {(wn, n, nq): 0 for wn, (_, cells) in WORLDS.items() for _, n in cells for nq in (4, 1)}

_ring_worlds = {}


def _ring_world(name):
    """The fixture's model (shared with test_scan4_long_chunks.py) with this file's own cells: seeded fine codes, inserted directly."""
    if name not in _ring_worlds:
        fixture, cells = WORLDS[name]
        base = _world(fixture)
        rs = np.random.RandomState(8705 + len(cells))
        coarse = np.concatenate([np.tile(np.array(c, dtype=np.uint16), (n, 1)) for c, n in cells])
        fine = rs.randint(0, 256, size=(len(coarse), base["M"])).astype(np.uint8)
        start = np.concatenate([[0], np.cumsum([n for _, n in cells])])
        _ring_worlds[name] = dict(base, coarse=coarse, fine=fine, start=start)
    return _ring_worlds[name]


def _run(monkeypatch, capfd, wname, cell, nq):
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    w = _ring_world(wname)
    n = WORLDS[wname][1][cell][1]
    a = int(w["start"][cell])
    # four queries spread over the chunk, its last code among them; one query: the last code (the partial row when there is one)
    targets = [a + n - 1] if nq == 1 else [a + (n * 1) // 8, a + (n * 3) // 8, a + (n * 6) // 8, a + n - 1]
    Q = _queries(w, w["fine"], targets, 1000 * cell + nq)
    stats = []
    search = LOPQSearcherHIP.search_batch

    def spy(self, *args, **kw):
        r = search(self, *args, **kw)
        stats.append(self.last_stats())
        return r

    monkeypatch.setattr(LOPQSearcherHIP, "search_batch", spy)
    monkeypatch.setenv("CIS_SEG_MAX", "65536")
    monkeypatch.setenv("CIS_SCAN4_DEBUG", "1")
    capfd.readouterr()
    _check(w, w["fine"], Q, modes=(5,))
    err = capfd.readouterr().err
    lines, total = parse_debug(err)
    st = stats[-1]  # the mode-5 search
    fallbacks = total.fallbacks
    print("%s len %d nq %d: %d launches, %s; %d candidates / %d items" % (wname, n, nq, len(lines), total, st["candidates"], st["items"]))
    assert st["scan_kernel"] == "k_adc_scan4" and lines, "the sampled form ran"
    assert st["candidates"] >= 6144 * st["items"], "the long-chunk form ran"
    assert fallbacks == PARENT_FALLBACKS[(wname, n, nq)]


@pytest.mark.parametrize("nq", [4, 1])
@pytest.mark.parametrize("cell", range(5))
def test_sample_rounds(monkeypatch, capfd, cell, nq):
    """One to three rounds of the sample: ring deeper than the loop, a second round of one row, odd and even counts, partial last rows."""
    _run(monkeypatch, capfd, "rounds", cell, nq)


@pytest.mark.parametrize("nq", [4, 1])
@pytest.mark.parametrize("cell", range(6))
def test_sample_cap_and_short_cells(monkeypatch, capfd, cell, nq):
    """Eight rounds at the cap of 128 sample rows (65536 and 65535 codes), and short cells inside a long-form launch: 1, 64 and 1000 codes
    (every row sampled) and 1025 (seventeen rows, the last never sampled)."""
    _run(monkeypatch, capfd, "cap", cell, nq)


@pytest.mark.parametrize("cell", range(2))
def test_sample_rounds_at_m16(monkeypatch, capfd, cell):
    """M = 16 codes with the c3 fixture's model (the saturating scale) on the 20077 and 8705 cells."""
    if _world("c3")["load_s"] > 1.0:
        pytest.skip("the c3 fixture's model took %.1f s to load" % _world("c3")["load_s"])
    assert _ring_world("m16")["M"] == 16
    _run(monkeypatch, capfd, "m16", cell, 4)
