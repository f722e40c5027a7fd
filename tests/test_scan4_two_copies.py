"""GPU: the two interleaved table copies of k_adc_scan4's long-chunk M = 8 form (csrc/lopq_scan3.hip).

Entry (k, j, copy c) of a slot's table sits at byte k << 7 | (2 j + c) << 3 of LDS; a lane gathers from the copy its bit 3 names; after the
main pass the odd 8-byte slots (copy 1) take the per-query lists, list word i at byte (i >> 1) << 4 | 8 | (i & 1) << 2, and the second
gather reads copy 0 alone.  A wave records at most 768 positions (six registers of packed pairs per lane) and a quarter of a query's
list holds 254 entries; past either the slot goes to the fall-back.

Built like test_scan4_long_chunks.py, whose world, queries and comparison these cases use: the c4 fixture's model, three cells of 6144,
6145 and 20077 codes inserted directly, CIS_SEG_MAX=65536 so that a cell is one chunk and the long-chunk form runs; scan mode 5
(k_adc_scan4, asserted) against mode 1 (the float64 scan kernel) bit for bit on ids, dists, n_found and visited, and the first eight
queries against the oracle."""
import numpy as np
import pytest

from test_scan4_long_chunks import CELLS, _check, _queries, _wave_positions, _with_duplicates, _world

pytestmark = pytest.mark.gpu


@pytest.fixture
def long_chunks(monkeypatch):
    monkeypatch.setenv("CIS_SEG_MAX", "65536")


def _enumerated(w, cell=2):
    """The base codes with cell `cell` rewritten so that every sub-quantizer j runs through every k (2 j + 1 is odd: p -> p (2 j + 1) + 37 j
    is a bijection mod 256, so k = 0, 1, 254 and 255 occur in every j), at every lane and row parity."""
    fine = w["fine"].copy()
    a, n = int(w["start"][cell]), CELLS[cell][1]
    p = np.arange(n)[:, None]
    j = np.arange(w["M"])[None, :]
    fine[a:a + n] = ((p * (2 * j + 1) + 37 * j) % 256).astype(np.uint8)
    return fine, a


def test_every_table_slot_through_both_copies(long_chunks):
    """Sixteen queries at positions 64 r + l of the enumerated cell, l = 0 .. 15: both values of the copy bit (l >> 3) & 1 and all eight
    rotation residues l & 7.  The cell's 20077 candidates are gathered by lanes of both copies for every (k, j)."""
    w = _world("c4")
    assert w["M"] == 8
    fine, a = _enumerated(w)
    targets = [a + 64 * (3 + 19 * l) + l for l in range(16)]
    _check(w, fine, _queries(w, fine, targets, 700), modes=(5,))


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 253, 254, 255])
def test_list_words_at_slot_boundaries(long_chunks, count):
    """`count` duplicates of the query's code in wave 0's blocks: with the code itself the query's list holds words 0 .. count in wave 0's
    quarter -- both word parities and the first 16-byte step at 1 .. 5, the quarter's capacity of 254 at 253 (full), 254 and 255 (over:
    the slot falls back)."""
    w = _world("c4")
    fine, t = _with_duplicates(w, 2, 0, count)
    others = [int(w["start"][2]) + 5000, int(w["start"][0]) + 99]
    _check(w, fine, _queries(w, fine, [t] + others, 800 + count), modes=(5,))


@pytest.mark.parametrize("count", [191, 192, 193])
def test_position_list_capacity_without_a_quarter_overflowing(long_chunks, count):
    """Four queries of one slot, each with `count` duplicates of its code in wave 0's blocks: wave 0 records about 4 x count positions --
    just under its 768, at them and over them (the slot falls back) -- while no quarter of a query's list (254) overflows."""
    w = _world("c4")
    fine = w["fine"].copy()
    a, n = int(w["start"][2]), CELLS[2][1]
    offs = [700, 1300, 2900, 4100]  # the queries' own codes: blocks of waves 1, 2, 2 and 0
    pos = _wave_positions(n, 0)
    pos = pos[~np.isin(pos, offs)]
    assert len(pos) >= 4 * count
    for i, off in enumerate(offs):
        fine[a + pos[i * count:(i + 1) * count]] = fine[a + off]
    _check(w, fine, _queries(w, fine, [a + off for off in offs], 900 + count), modes=(5,))


@pytest.mark.parametrize("nq", [1, 2, 3])
def test_partly_filled_slot(long_chunks, nq):
    """A slot with one, two and three queries on the enumerated cell: the padded queries' entries are the cap in both copies, and lanes of
    both copies gather them."""
    w = _world("c4")
    fine, a = _enumerated(w)
    targets = [a + 64 * (5 + 40 * i) + (3 + 9 * i) % 16 for i in range(nq)]
    _check(w, fine, _queries(w, fine, targets, 1000 + nq), modes=(5,))


def test_items_of_different_chunks_in_one_slot(monkeypatch):
    """CIS_SEG_MAX=8192: the 20077-code cell is three chunks that share a slot key, so its slot runs as sub-slots -- the tables are staged
    again over the previous sub-slot's lists."""
    monkeypatch.setenv("CIS_SEG_MAX", "8192")
    w = _world("c4")
    fine, a = _enumerated(w)
    targets = [a + 100, a + 17000 + 8, a + 8191, a + 8192, int(w["start"][0]) + 1, int(w["start"][1]) + 2, a + 20076, a + 12345 + 11]
    _check(w, fine, _queries(w, fine, targets, 1100), modes=(5,))
