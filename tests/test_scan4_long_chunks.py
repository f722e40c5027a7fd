"""GPU: the per-slot phases of k_adc_scan4 (csrc/lopq_scan3.hip) on long chunks -- the recorded-position lists of the deferred split,
their second gather, the thresholds and the verification -- at the places where their register and list boundaries lie.

Three cells of 6144, 6145 and 20077 codes with seeded fine codes, inserted directly (no encoding); queries are the slightly perturbed
reconstructions of chosen codes.  Every case compares the sampled single-pass form (k_adc_scan4) and the two-pass form with the float64
scan kernel (set_scan_mode(mode=1)) on the same searcher, bit for bit, and its first eight queries with the oracle.

Scan modes: cis_index_set_scan_mode's 5 is the mode that runs k_adc_scan4 (4 is k_adc_scan3's two-pass form: csrc/lopq_search.hip), so
the assertion on last_stats()["scan_kernel"] is made for mode 5; mode 4 is compared as well.  Batches of fewer than 64 queries are
planned with chunks of 4096 candidates (route_hints, csrc/lopq_search.hip), which would put these cells on the SHORT-chunk form: CIS_SEG_MAX=65536 keeps a cell
one chunk, so that the batch's average chunk is >= 6144 and scan3_geom takes the long-chunk form (lists of 1016 entries, eight registers
of recorded positions per lane); the cases marked "short" leave the 4096-candidate chunks and run the short-chunk form (504 entries,
four registers) over the same data."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LIMIT = 100
QUOTA = 10000
CELLS = (((2, 5), 6144), ((7, 1), 6145), ((11, 13), 20000 + 77))
NQS = (1, 3, 4, 5, 9)
DUPS = (0, 1, 127, 128, 129, 255, 256, 257, 1000)

_worlds = {}


def _world(name):
    """Model (HIP and oracle), the three cells' base codes and the pseudo-inverse of the PCA (queries are built in model space)."""
    if name in _worlds:
        return _worlds[name]
    import time
    from test_lopq_hip_parity import hip_model
    from oracle import lopq_oracle as O
    t0 = time.time()
    z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")))
    om = O.OracleModel.from_npz(z)
    M = 2 * int(z["num_fine_splits"])
    rs = np.random.RandomState(20077)
    coarse = np.concatenate([np.tile(np.array(c, dtype=np.uint16), (n, 1)) for c, n in CELLS])
    fine = rs.randint(0, 256, size=(len(coarse), M)).astype(np.uint8)
    start = np.concatenate([[0], np.cumsum([n for _, n in CELLS])])
    model = hip_model(z)
    w = dict(z=z, model=model, load_s=time.time() - t0, om=om, M=M, coarse=coarse, fine=fine, start=start, pinv=np.linalg.pinv(np.asarray(z["pca_P"], dtype=np.float64)),
             mu=np.asarray(z["pca_mu"], dtype=np.float64))
    _worlds[name] = w
    return w


def _wave_positions(n, wave):
    """Positions of a chunk of n candidates that wave `wave` of a slot scans: blocks [128 i, 128 i + 128) with i % 4 == wave."""
    p = np.arange(n)
    return p[(p // 128) % 4 == wave]


def _queries(w, fine, targets, seed):
    """Perturbed reconstructions of the codes at rows `targets`, mapped back through the PCA to the model's input space."""
    from oracle import lopq_oracle as O
    rs = np.random.RandomState(seed)
    out = []
    for t in targets:
        y = O.reconstruct(w["om"], (tuple(int(c) for c in w["coarse"][t]), tuple(int(f) for f in fine[t])))
        y = y + 0.01 * rs.randn(len(y)) / np.sqrt(len(y))
        out.append(w["mu"] + y.dot(w["pinv"]))
    return np.ascontiguousarray(np.array(out, dtype=np.float64))


def _check(w, fine, Q, modes=(5, 4)):
    import torch
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    from oracle import lopq_oracle as O
    s = LOPQSearcherHIP(w["model"])
    try:
        n = len(fine)
        added, bad = s.add_codes_dev(torch.as_tensor(w["coarse"].view(np.int16)).cuda(), torch.as_tensor(fine).cuda(),
                                     torch.arange(n, dtype=torch.int64, device="cuda"), dedup=False)
        assert (added, bad) == (n, 0)
        s.set_scan_mode(mode=1)
        want = s.search_batch(Q, quota=QUOTA, limit=LIMIT)
        for mode in modes:
            s.set_scan_mode(mode=mode)
            got = s.search_batch(Q, quota=QUOTA, limit=LIMIT)
            if mode == 5:
                assert s.last_stats()["scan_kernel"] == "k_adc_scan4"
            for k in ("ids", "n_found", "visited"):
                np.testing.assert_array_equal(got[k], want[k], err_msg="mode %d %s" % (mode, k))
            np.testing.assert_array_equal(got["dists"].view(np.uint64), want["dists"].view(np.uint64), err_msg="mode %d dists" % mode)
        oi = O.OracleCSRIndex(w["om"], w["coarse"], fine)
        for qi in range(min(8, len(Q))):
            ids, dists, visited = oi.search(Q[qi], quota=QUOTA, limit=LIMIT)
            k = len(ids)
            assert int(want["n_found"][qi]) == k and int(want["visited"][qi]) == visited
            np.testing.assert_array_equal(want["ids"][qi, :k], ids)
            np.testing.assert_allclose(want["dists"][qi, :k], dists, rtol=1e-9, atol=1e-12)
    finally:
        s.set_scan_mode(mode=0)
        s.close()


def _with_duplicates(w, cell, wave, count, target_off=700):
    """The base codes with `count` copies of one code of cell `cell` written over the first positions of that cell that wave `wave`
    scans (the code itself sits at position target_off of the cell, in a block of wave (target_off // 128) % 4)."""
    fine = w["fine"].copy()
    a, n = int(w["start"][cell]), CELLS[cell][1]
    t = a + target_off
    pos = _wave_positions(n, wave)
    pos = pos[pos != target_off][:count]
    assert len(pos) == count
    fine[a + pos] = fine[t]
    return fine, t


@pytest.fixture
def long_chunks(monkeypatch):
    monkeypatch.setenv("CIS_SEG_MAX", "65536")


@pytest.mark.parametrize("nq", NQS)
def test_partly_filled_slots_and_several_slots_per_cell(long_chunks, nq):
    """nq queries aimed at one cell (slots of four: nq = 1, 3 and 5 leave a slot partly filled, 5 and 9 give the cell more than one) and,
    from nq = 3, one at each of the other cells."""
    w = _world("c4")
    targets = [int(w["start"][2]) + 300 + 1111 * i for i in range(nq)]
    if nq >= 3:
        targets[1] = int(w["start"][0]) + 17
        targets[2] = int(w["start"][1]) + 6144
    _check(w, w["fine"], _queries(w, w["fine"], targets, 100 + nq))


@pytest.mark.parametrize("form", ["long", "short"])
@pytest.mark.parametrize("count", DUPS)
def test_recorded_positions_cross_register_and_half_boundaries(monkeypatch, count, form):
    """`count` exact duplicates of the query's own code in wave 0's blocks only (a packed-position register holds 128 positions, a half
    64): the recorded-position count of wave 0 crosses every register and half boundary while the other waves record only what the
    threshold lets through.  From 255 duplicates on, wave 0's quarter of the query's list (254 entries; 126 in the short form)
    overflows and the slot goes to the fall-back."""
    if form == "long":
        monkeypatch.setenv("CIS_SEG_MAX", "65536")
    w = _world("c4")
    fine, t = _with_duplicates(w, 2, 0, count)
    others = [int(w["start"][2]) + 5000, int(w["start"][0]) + 99]
    _check(w, fine, _queries(w, fine, [t] + others, 200 + count))


@pytest.mark.parametrize("cell,wave,count,everywhere", [(0, 1, 1100, False), (2, 3, 1100, False), (2, 0, 3000, True)])
def test_position_list_and_list_overflow_fall_back(long_chunks, cell, wave, count, everywhere):
    """1100 duplicates in one wave's blocks: more than the 1024 positions a wave records -- the slot falls back.  A crowd of 3000
    identical codes spread over all waves' blocks: every quarter of the query's list overflows.  Both equal the float64 kernel."""
    w = _world("c4")
    if everywhere:
        fine = w["fine"].copy()
        a = int(w["start"][cell])
        t = a + 700
        pos = np.random.RandomState(3000).choice(CELLS[cell][1], count, replace=False)
        fine[a + pos] = fine[t]
    else:
        fine, t = _with_duplicates(w, cell, wave, count)
    _check(w, fine, _queries(w, fine, [t, int(w["start"][1]) + 5, t + 1, t + 2, t + 3], 300 + count + cell))


@pytest.mark.parametrize("count", [0, 129, 1100])
def test_the_same_cells_at_m16(long_chunks, count):
    """M = 16 codes with the c3 fixture's model (the saturating scale; one row ahead in the second gather)."""
    w = _world("c3")
    if w["load_s"] > 1.0:
        pytest.skip("the c3 fixture's model took %.1f s to load" % w["load_s"])
    assert w["M"] == 16
    fine, t = _with_duplicates(w, 2, 0, count)
    _check(w, fine, _queries(w, fine, [t, int(w["start"][0]) + 99, int(w["start"][1]) + 4000, t + 5, t + 9], 400 + count))


def test_items_of_different_chunks_in_one_slot(monkeypatch):
    """CIS_SEG_MAX=8192: the 20077-code cell is three chunks that share a slot key -- slots with items of different chunks run as
    sub-slots."""
    monkeypatch.setenv("CIS_SEG_MAX", "8192")
    w = _world("c4")
    fine, t = _with_duplicates(w, 2, 0, 129, target_off=9000)
    targets = [t, int(w["start"][2]) + 100, int(w["start"][2]) + 17000, int(w["start"][2]) + 8191, int(w["start"][2]) + 8192,
               int(w["start"][0]) + 1, int(w["start"][1]) + 2, int(w["start"][2]) + 20076, int(w["start"][2]) + 12345]
    _check(w, fine, _queries(w, fine, targets, 500))
