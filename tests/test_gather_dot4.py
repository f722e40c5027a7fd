"""GPU: the one-instruction table address of the rotated gathers (csrc/scan_common.h: gather_addr).

Where the chip has the byte dot product, entry (k, j) of a table with rows of 1 << SH bytes is addressed as v_dot4_u32_u8(D, sel, c): the
code dword against a per-lane selector that holds 1 << SH in the byte this lane uses at this step and zero in the other three, plus the
lane's constant (the table's LDS base and the entry's column).  The three bytes the selector zeroes must contribute nothing, 255 << SH
must stay inside the row's table, and the float32 scan's four-query form at M = 16 (rows of 256 bytes: the factor does not fit a byte)
keeps the two-instruction address in the same build.

Built from test_scan4_long_chunks.py's world, queries and comparison (imported, not edited): three cells of 6144, 6145 and 20077 codes
inserted directly; every case compares forced scan modes -- 2 (k_adc_scan2, float32 tables), 3 and 4 (k_adc_scan3, streaming and two-pass
forms), 5 (k_adc_scan4, asserted by name) -- bit for bit on ids, dists, n_found and visited with mode 1, the float64 scan kernel, which
has no rotated gather; the first eight queries also go against the oracle.  CIS_SEG_MAX=65536 keeps a cell one chunk (k_adc_scan4's
long-chunk form: two table copies at M = 8, rows of 128 bytes); without it the chunks are 4096 candidates (short-chunk form, 64 bytes).

M = 4: the only M = 4 fixtures under tests/golden/ are c1 (no PCA, 8 x 8 coarse cells) and tiny (16 entries per sub-quantizer); c1 serves
here with a world of its own, built like _world with the third cell at a coarse pair the model has."""
import os

import numpy as np
import pytest

from test_scan4_long_chunks import CELLS, _check, _queries, _world

pytestmark = pytest.mark.gpu

MODES = (2, 3, 4, 5)
SIZES = tuple(n for _, n in CELLS)

_m4 = {}


def _world_m4():
    """test_scan4_long_chunks._world for the c1 fixture (M = 4, no PCA: the model's input space is its own): the same three cell sizes, the
    third cell at (3, 6) -- c1 has eight coarse clusters per half."""
    if _m4:
        return _m4
    from test_lopq_hip_parity import hip_model
    from oracle import lopq_oracle as O
    z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c1.npz")))
    assert not int(z["has_pca"])
    M = 2 * int(z["num_fine_splits"])
    assert M == 4
    D = 2 * np.asarray(z["Cs"]).shape[2]
    cells = ((2, 5), (7, 1), (3, 6))
    rs = np.random.RandomState(20077)
    coarse = np.concatenate([np.tile(np.array(c, dtype=np.uint16), (n, 1)) for c, n in zip(cells, SIZES)])
    fine = rs.randint(0, 256, size=(len(coarse), M)).astype(np.uint8)
    _m4.update(z=z, model=hip_model(z), om=O.OracleModel.from_npz(z), M=M, coarse=coarse, fine=fine,
               start=np.concatenate([[0], np.cumsum(SIZES)]), pinv=np.eye(D), mu=np.zeros(D))
    return _m4


def _enumerated(w, cell=2):
    """The base codes with cell `cell` rewritten so that every sub-quantizer j runs through every k (2 j + 1 is odd: p -> p (2 j + 1) + 37 j
    is a bijection mod 256, so k = 0, 1, 254 and 255 occur in every j), at every lane and row parity.  (test_scan4_two_copies.py's.)"""
    fine = w["fine"].copy()
    a, n = int(w["start"][cell]), SIZES[cell]
    p = np.arange(n)[:, None]
    j = np.arange(w["M"])[None, :]
    fine[a:a + n] = ((p * (2 * j + 1) + 37 * j) % 256).astype(np.uint8)
    return fine, a


def _rotation_targets(a):
    """Sixteen positions 64 r + l of the cell at `a`, l = 0 .. 15: all rotation residues (l & 15 at M = 16) and both copy bits (l >> 3) & 1."""
    return [a + 64 * (3 + 19 * l) + l for l in range(16)]


def _saturated(w, variant, cell=0):
    """Cell `cell` as neighbours of the selected byte at their extremes.  "ff": every byte 255.  "alt": 255, 0, 255, 0, ... from byte to
    byte.  "one": zero except one byte at 255, at position p % M for the code at position p.  Crowds of equal codes: the exact paths run."""
    fine = w["fine"].copy()
    a, n, M = int(w["start"][cell]), SIZES[cell], w["M"]
    if variant == "ff":
        fine[a:a + n] = 255
    elif variant == "alt":
        fine[a:a + n] = np.where(np.arange(M) % 2 == 0, 255, 0).astype(np.uint8)[None, :]
    else:
        assert variant == "one"
        fine[a:a + n] = 0
        fine[a + np.arange(n), np.arange(n) % M] = 255
    return fine, a


@pytest.fixture(params=["long", "short"])
def form(request, monkeypatch):
    if request.param == "long":
        monkeypatch.setenv("CIS_SEG_MAX", "65536")
    return request.param


def test_enumerated_codes_through_every_scan_mode(form):
    w = _world("c4")
    assert w["M"] == 8
    fine, a = _enumerated(w)
    _check(w, fine, _queries(w, fine, _rotation_targets(a), 1200), modes=MODES)


@pytest.mark.parametrize("variant", ["ff", "alt", "one"])
def test_saturated_neighbours(form, variant):
    """Queries at the saturated cell (M + 1 consecutive positions: every place of the lone 255 and the first again) and one at each other cell."""
    w = _world("c4")
    fine, a = _saturated(w, variant)
    targets = [a + 640 + i for i in range(w["M"] + 1)] + [int(w["start"][1]) + 77, int(w["start"][2]) + 12345]
    _check(w, fine, _queries(w, fine, targets, 1300 + len(variant)), modes=MODES)


@pytest.mark.parametrize("case", ["enumerated", "ff", "alt", "one"])
def test_the_same_at_m16(monkeypatch, case):
    """The c3 fixture's model (M = 16: rows of 128 bytes in the 16-bit scans, two pipeline units per candidate)."""
    monkeypatch.setenv("CIS_SEG_MAX", "65536")
    w = _world("c3")
    assert w["M"] == 16
    if case == "enumerated":
        fine, a = _enumerated(w)
        targets = _rotation_targets(a)
    else:
        fine, a = _saturated(w, case)
        targets = [a + 640 + i for i in range(17)] + [int(w["start"][1]) + 77, int(w["start"][2]) + 12345]
    _check(w, fine, _queries(w, fine, targets, 1400 + len(case)), modes=MODES)


@pytest.mark.parametrize("case", ["enumerated", "one"])
def test_the_same_at_m4(form, case):
    w = _world_m4()
    if case == "enumerated":
        fine, a = _enumerated(w)
        targets = _rotation_targets(a)
    else:
        fine, a = _saturated(w, case)
        targets = [a + 640 + i for i in range(5)] + [int(w["start"][1]) + 77, int(w["start"][2]) + 12345]
    _check(w, fine, _queries(w, fine, targets, 1500 + len(case)), modes=MODES)


@pytest.mark.parametrize("name", ["c4", "c3"])
@pytest.mark.parametrize("nq", [1, 2, 3, 64])
def test_float32_scan_forms_with_both_addresses(monkeypatch, name, nq):
    """The float32 scan (mode 2) on the enumerated cell by queries per workgroup: one (its default below 64 queries: a partly filled slot of
    the 16-bit scans at nq = 1, 2, 3), two (from 64 queries) and -- CIS_SCAN_GEOM=4,4,4 -- four, whose rows are 128 bytes at M = 8 (the
    dot product) and 256 bytes at M = 16 (the two-instruction address): both forms in one build, on the same data."""
    monkeypatch.setenv("CIS_SEG_MAX", "65536")
    w = _world(name)
    fine, a = _enumerated(w)
    targets = [a + 64 * (5 + 4 * i) + (3 + 9 * i) % 16 for i in range(nq)]
    Q = _queries(w, fine, targets, 1600 + nq)
    _check(w, fine, Q, modes=MODES)
    monkeypatch.setenv("CIS_SCAN_GEOM", "4,4,4")
    _check(w, fine, Q, modes=(2,))
