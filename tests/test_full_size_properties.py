"""GPU: size-independent properties of the hot path at BASELINE.json's full size (10M x 128-d index, V=16, M=8,
8192 queries per batch, quota 10000, limit 100), where the oracle is too slow to check every row.

* encode: batch-composition invariance (one big call == the concatenation of ragged small calls),
* search: sorted distances, n_found, idempotence, batch-composition invariance, the limit-10 list is the prefix of
  the limit-100 list (stable ranking key), a database vector finds itself, visited >= quota,
* cell sharding: two shards scanned separately and merged == the single index (partition invariance),
* a checksum of checksums against the oracle on a small sample of the same batch.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 10_000_000
N_CHUNKS = 10
NQ = 8192
QUOTA = 10000
LIMIT = 100


@pytest.fixture(scope="module")
def world():
    import torch
    import bench as B
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    dev = torch.device("cuda", 0)
    model, z = B.load_model("c4")
    P = B.mixture_centers("descriptor", dev)
    chunk_n = N // N_CHUNKS
    co, fi = [], []
    for c in range(N_CHUNKS):
        a, b = model.predict_batch_dev(B.gen_chunk(P, c, chunk_n, dev))
        co.append(a)
        fi.append(b)
    cd, fd = torch.cat(co), torch.cat(fi)
    coarse = cd.cpu().numpy().view(np.uint16)
    fine = fd.cpu().numpy()
    s = LOPQSearcherHIP(model)
    # the device-side insert (csrc/lopq_index.hip): codes go from the encoder to the index without leaving HBM
    added, bad = s.add_codes_dev(cd, fd, torch.arange(N, dtype=torch.int64, device=dev), dedup=False)
    assert (added, bad) == (N, 0)
    del cd, fd, co, fi
    x0 = B.gen_chunk(P, 0, chunk_n, dev)
    q = B.make_queries(x0, 0, NQ, dev)
    return dict(model=model, z=z, P=P, chunk_n=chunk_n, coarse=coarse, fine=fine, searcher=s, x0=x0, q=q, B=B, dev=dev)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")}


def test_encode_is_independent_of_batch_composition(world):
    import torch
    m, x0 = world["model"], world["x0"]
    ref_c, ref_f = world["coarse"][:world["chunk_n"]], world["fine"][:world["chunk_n"]]
    cuts = [0, 1, 2, 65, 4096, 4097, 100_003, 500_000, world["chunk_n"]]  # ragged pieces, 1-row piece included
    for a, b in zip(cuts[:-1], cuts[1:]):
        c, f = m.predict_batch_dev(x0[a:b].contiguous())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(c.cpu().numpy().view(np.uint16), ref_c[a:b])
        np.testing.assert_array_equal(f.cpu().numpy(), ref_f[a:b])
    c, f = m.predict_batch_dev(x0[:0].contiguous())  # empty input
    assert c.shape[0] == 0 and f.shape[0] == 0


def test_encode_matches_oracle_on_rows_sampled_from_every_chunk(world):
    """4160 rows drawn from all 10 chunks of the 10M build against the oracle's compute_codes, bit for bit (the oracle index
    of the search checks below is built from the HIP codes: this is what makes that sound)."""
    from oracle import lopq_oracle as O
    B, P, chunk_n, dev = world["B"], world["P"], world["chunk_n"], world["dev"]
    om = O.OracleModel.from_npz(world["z"])
    import torch
    for c in range(N_CHUNKS):
        sel = np.random.RandomState(900 + c).choice(chunk_n, 416, replace=False)
        x = B.gen_chunk(P, c, chunk_n, dev)[torch.as_tensor(sel, device=dev)].cpu().numpy()
        oc, of = O.compute_codes(om, x)
        np.testing.assert_array_equal(oc, world["coarse"][c * chunk_n + sel])
        np.testing.assert_array_equal(of, world["fine"][c * chunk_n + sel])


def test_index_built_on_device_equals_host_built_cells(world):
    """Cells of the 10M index read back (get_cell) == a numpy grouping of the codes by cell in arrival order."""
    s, coarse, fine = world["searcher"], world["coarse"], world["fine"]
    V = world["model"].V
    cell = coarse[:, 0].astype(np.int64) * V + coarse[:, 1]
    for c in (0, 77, V * V - 1):
        idx = np.nonzero(cell == c)[0]
        got = s.get_cell((c // V, c % V))
        np.testing.assert_array_equal(np.array([i for i, _ in got], dtype=np.int64), idx)
        np.testing.assert_array_equal(np.array([code.fine for _, code in got], dtype=np.uint8), fine[idx])


def test_search_properties_at_full_size(world):
    import torch
    s, q = world["searcher"], world["q"]
    o1 = _np(s.search_batch_dev(q, quota=QUOTA, limit=LIMIT))
    cand = s.last_stats()["candidates"]
    o2 = _np(s.search_batch_dev(q, quota=QUOTA, limit=LIMIT))
    for k in ("ids", "dists", "n_found", "visited"):  # idempotence, bit for bit
        np.testing.assert_array_equal(o1[k], o2[k])
    assert cand >= NQ * QUOTA  # whole cells are consumed until the quota is reached
    assert (o1["n_found"] == LIMIT).all() and (o1["visited"] >= 1).all()
    d = o1["dists"]
    assert np.isfinite(d).all() and (d >= 0).all()
    assert (np.diff(d, axis=1) >= 0).all()  # sorted
    assert (o1["ids"] >= 0).all() and (o1["ids"] < N).all()
    srt = np.sort(o1["ids"], axis=1)
    assert (np.diff(srt, axis=1) > 0).all()  # an item is returned once
    # batch composition: ragged sub-batches reproduce their rows of the big batch
    for a, b in [(0, 1), (1, 66), (4000, 4257), (8191, 8192)]:
        sub = _np(s.search_batch_dev(q[a:b].contiguous(), quota=QUOTA, limit=LIMIT))
        for k in ("ids", "dists", "n_found", "visited"):
            np.testing.assert_array_equal(sub[k], o1[k][a:b])
    # the ranking key (dist, visit rank, position) is total: a shorter limit is a prefix
    o10 = _np(s.search_batch_dev(q, quota=QUOTA, limit=10))
    np.testing.assert_array_equal(o10["ids"], o1["ids"][:, :10])
    np.testing.assert_array_equal(o10["dists"], o1["dists"][:, :10])
    np.testing.assert_array_equal(o10["visited"], o1["visited"])
    # a larger quota consumes the same cells first: visited grows, and the best distance cannot get worse
    big = _np(s.search_batch_dev(q[:512].contiguous(), quota=4 * QUOTA, limit=LIMIT))
    assert (big["visited"] >= o1["visited"][:512]).all()
    assert (big["dists"][:, 0] <= o1["dists"][:512, 0]).all()


def test_every_scan_route_agrees_at_full_size(world):
    """Whole 8192-query batches through every ranking route -- automatic, float32 prefilter, 16-bit fixed-point prefilter in its
    streaming, its two-pass and its sampled single-pass form, float64 scan -- bit for bit: on the 10M index (39 k-candidate cells) and on an index of its
    first million vectors (3.9 k-candidate cells: the shape at which automatic routing takes the two-pass form).  A route
    that drops one candidate in twenty thousand queries shows up here (the two-pass form once did, at rank `limit`)."""
    import torch
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    B, dev = world["B"], world["dev"]
    small = LOPQSearcherHIP(world["model"])
    n1 = 1_000_000
    small.add_codes_array(world["coarse"][:n1], world["fine"][:n1], ids=np.arange(n1, dtype=np.int64), dedup=False)
    try:
        for s, batches in ((world["searcher"], (0, 5)), (small, (1, 2, 3, 6))):
            for b in batches:
                q = B.make_queries(world["x0"], b, NQ, dev)
                for limit in (LIMIT, 37, 185):
                    s.set_scan_mode(mode=1)
                    want = _np(s.search_batch_dev(q, quota=QUOTA, limit=limit))
                    for mode in (0, 2, 3, 4, 5):
                        s.set_scan_mode(mode=mode)
                        got = _np(s.search_batch_dev(q, quota=QUOTA, limit=limit))
                        for k in ("ids", "n_found", "visited"):
                            np.testing.assert_array_equal(got[k], want[k], err_msg="mode %d batch %d limit %d %s" % (mode, b, limit, k))
                        np.testing.assert_array_equal(got["dists"].view(np.uint64), want["dists"].view(np.uint64))
                    s.set_scan_mode(mode=0)
    finally:
        world["searcher"].set_scan_mode(mode=0)
        small.close()


def test_sampled_scan_fall_back_on_long_chunks(world, monkeypatch):
    """The sampled single-pass form on 39 k-candidate chunks with a sample margin so small (z = 0.3) that many lists fail
    their verification, and with lists too short for their chunks (a 16-row sample at most): the slots concerned are scanned
    again by the streaming form, the result is the float64 kernel's, bit for bit."""
    B, dev, s = world["B"], world["dev"], world["searcher"]
    q = B.make_queries(world["x0"], 7, 2048, dev)
    try:
        s.set_scan_mode(mode=1)
        want = _np(s.search_batch_dev(q, quota=QUOTA, limit=LIMIT))
        s.set_scan_mode(mode=5)
        for env in ({"CIS_S4_ZL": "0.3"}, {"CIS_S4_NSX": "16", "CIS_S4_FRAC": "64"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = _np(s.search_batch_dev(q, quota=QUOTA, limit=LIMIT))
            for k in env:
                monkeypatch.delenv(k)
            for k in ("ids", "n_found", "visited"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=str(env))
            np.testing.assert_array_equal(got["dists"].view(np.uint64), want["dists"].view(np.uint64))
    finally:
        s.set_scan_mode(mode=0)


def test_sampled_scan_at_m16_with_its_saturating_scale(monkeypatch):
    """C3 at full size (1M x 4096-d, PCA to 256, V=16, M=16; tests/golden/c3full.npz): automatic routing takes the sampled
    single-pass form with the saturating scale (k_adc_scan4, Scan3Geom::sat).  Its results are the float64 kernel's bit for
    bit at the default scale, at a scale so fine that every threshold saturates and at one so coarse that lists overflow (the
    slots concerned run again in the streaming form); and after a batch where the scale missed, the index serves the next
    batches from the float32 prefilter kernel (the back-off of search_batch)."""
    import torch
    import bench as B
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    dev = torch.device("cuda", 0)
    model, z = B.load_model("c3full")
    P = B.mixture_centers("relu_mixture", dev)
    n, chunk_n = 1_000_000, 100_000
    s = LOPQSearcherHIP(model)
    coarse_h, fine_h = [], []
    for c in range(n // chunk_n):
        a, b = model.predict_batch_dev(B.gen_chunk(P, c, chunk_n, dev))
        s.add_codes_dev(a, b, torch.arange(c * chunk_n, (c + 1) * chunk_n, dtype=torch.int64, device=dev), dedup=False)
        coarse_h.append(a.cpu().numpy().view(np.uint16))
        fine_h.append(b.cpu().numpy())
    x0 = B.gen_chunk(P, 0, chunk_n, dev)
    try:
        # The ORACLE at this size (round-5 review: pytest compared C3 at 1M with the float64 kernel only): 1024 rows of the build
        # through the oracle's encoder, 64 queries of the automatic route (k_adc_scan4) through the oracle's search over the same
        # 1M codes brought to the host -- codes and ranked ids bit-exact, distances to 1e-9.
        from oracle import lopq_oracle as O
        om = O.OracleModel.from_npz(z)
        coarse_all, fine_all = np.concatenate(coarse_h), np.concatenate(fine_h)
        rows = np.arange(0, chunk_n, chunk_n // 1024)[:1024]
        oc, of = O.compute_codes(om, x0[torch.as_tensor(rows, device=dev)].cpu().numpy())
        np.testing.assert_array_equal(oc, coarse_all[rows])
        np.testing.assert_array_equal(of, fine_all[rows])
        oix = O.OracleCSRIndex(om, coarse_all, fine_all)
        q64 = B.make_queries(x0, 2, 4096, dev)
        got = _np(s.search_batch_dev(q64, quota=QUOTA, limit=LIMIT))
        assert s.last_stats()["scan_kernel"] == "k_adc_scan4"
        qh = q64[:64].cpu().numpy()
        for qi in range(64):
            ids, dd, vis = oix.search(qh[qi], quota=QUOTA, limit=LIMIT)
            k = len(ids)
            assert int(got["n_found"][qi]) == k and int(got["visited"][qi]) == vis
            np.testing.assert_array_equal(got["ids"][qi, :k], ids)
            np.testing.assert_allclose(got["dists"][qi, :k], dd, rtol=1e-9, atol=1e-12)
        del oix, coarse_all, fine_all
        for b, limit in ((0, LIMIT), (1, 37)):
            q = B.make_queries(x0, b, 4096, dev)
            s.set_scan_mode(mode=1)
            want = _np(s.search_batch_dev(q, quota=QUOTA, limit=limit))
            s.set_scan_mode(mode=0)
            for sat in (None, "0.5", "0.95", "1.3", "0.02"):
                if sat is not None:
                    monkeypatch.setenv("CIS_S4_SAT", sat)
                got = _np(s.search_batch_dev(q, quota=QUOTA, limit=limit))
                kernel = s.last_stats()["scan_kernel"]
                monkeypatch.delenv("CIS_S4_SAT", raising=False)
                for k in ("ids", "n_found", "visited"):
                    np.testing.assert_array_equal(got[k], want[k], err_msg="sat %s %s" % (sat, k))
                np.testing.assert_array_equal(got["dists"].view(np.uint64), want["dists"].view(np.uint64))
                if sat in (None, "0.5", "0.95"):
                    assert kernel == "k_adc_scan4", (sat, kernel)
                if sat in ("1.3", "0.02"):
                    # the scale missed on most slots: the next automatic batch is served by k_adc_scan2 ...
                    torch.cuda.synchronize()
                    got = _np(s.search_batch_dev(q, quota=QUOTA, limit=limit))
                    assert s.last_stats()["scan_kernel"] == "k_adc_scan2"
                    np.testing.assert_array_equal(got["ids"], want["ids"])
                    # ... for 64 batches, then the sampled form is tried again
                    for _ in range(64):
                        s.search_batch_dev(q[:512].contiguous(), quota=QUOTA, limit=limit)
                    s.search_batch_dev(q, quota=QUOTA, limit=limit)
                    assert s.last_stats()["scan_kernel"] == "k_adc_scan4"
    finally:
        s.set_scan_mode(mode=0)
        s.close()


def test_database_vectors_find_themselves(world):
    import torch
    s, x0 = world["searcher"], world["x0"]
    rows = torch.arange(0, 1_000_000, 3907, device=world["dev"])[:256]
    out = _np(s.search_batch_dev(x0[rows].contiguous(), quota=QUOTA, limit=LIMIT))
    own = rows.cpu().numpy()
    hit = out["ids"] == own[:, None]
    # the item's own cell is the first cell visited and its own code is the closest code of that cell
    assert hit.any(axis=1).mean() >= 0.99
    r, c = np.nonzero(hit)
    first = out["dists"][:, 0]
    # its distance is the quantisation error: no item of its own cell is closer, so whatever precedes it is at most equal
    # to it or comes from another cell; with limit 100 it sits at the head in the vast majority of cases
    assert (c == 0).mean() >= 0.9
    assert (out["dists"][r, c] >= first[r]).all()


@pytest.mark.parametrize("nshards", [2, 4])
def test_cell_shards_merge_to_the_single_index(world, nshards):
    """Partition invariance at full size: 2 and 4 cell shards scanned separately and merged == the single index (from four
    shards on a shard's long cells are scanned in chunks of 20480 candidates, each with its own slots, so that the few work
    items of a shard still spread over the chip)."""
    import torch
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    from columbiaimagesearch_amd.lopq.search import merge_packed_dev
    s, q = world["searcher"], world["q"][:2048].contiguous()
    ref = _np(s.search_batch_dev(q, quota=QUOTA, limit=LIMIT))
    parts = []
    for r in range(nshards):
        sh = LOPQSearcherHIP(world["model"], shard=(r, nshards))
        sh.add_codes_array(world["coarse"], world["fine"], ids=np.arange(N, dtype=np.int64), dedup=False)
        pp = sh.search_partial_packed_dev(q, quota=QUOTA, limit=LIMIT)
        torch.cuda.synchronize()
        parts.append({k: v.clone() for k, v in pp.items() if hasattr(v, "clone")})
        sh.close()
        del sh
    stride = max(int(p["total"].item()) for p in parts)
    buf = torch.zeros((nshards, stride, 4), dtype=torch.int64, device=world["dev"])
    for r, p in enumerate(parts):
        t = int(p["total"].item())
        buf[r, :t] = p["packed"][:t]
    cnt = torch.stack([p["cnt"] for p in parts]).contiguous()
    off = torch.stack([p["off"] for p in parts]).contiguous()
    out = _np(merge_packed_dev(buf, off, cnt, q.shape[0], LIMIT))
    np.testing.assert_array_equal(out["ids"], ref["ids"])
    np.testing.assert_array_equal(out["dists"], ref["dists"])
    np.testing.assert_array_equal(out["n_found"], ref["n_found"])


def test_checksum_of_checksums_against_the_oracle(world):
    """48 rows spread over the 8192-query batch: per-row checksums of (ids, distance bits) from the HIP path and from
    the oracle, folded into one number each."""
    import hashlib
    from oracle import lopq_oracle as O
    s, q = world["searcher"], world["q"]
    out = _np(s.search_batch_dev(q, quota=QUOTA, limit=LIMIT))
    om = O.OracleModel.from_npz(world["z"])
    oix = O.OracleCSRIndex(om, world["coarse"], world["fine"])
    rows = np.arange(0, NQ, NQ // 48)[:48]
    qh = q.cpu().numpy()
    h_gpu, h_cpu = hashlib.sha1(), hashlib.sha1()
    worst = 0.0
    for r in rows:
        ids, dists, visited = oix.search(qh[r], QUOTA, LIMIT)
        assert visited == out["visited"][r]
        np.testing.assert_array_equal(np.asarray(ids, np.int64), out["ids"][r])
        worst = max(worst, float(np.max(np.abs(np.asarray(dists) - out["dists"][r]) / np.maximum(np.asarray(dists), 1e-300))))
        h_cpu.update(hashlib.sha1(np.asarray(ids, np.int64).tobytes()).digest())
        h_gpu.update(hashlib.sha1(np.ascontiguousarray(out["ids"][r]).tobytes()).digest())
    assert h_cpu.hexdigest() == h_gpu.hexdigest()
    assert worst <= 1e-9  # north_star asks 1e-4


def test_routed_insert_and_pipelined_sharded_search_rccl():
    """RCCL process group (world = the visible GPUs, at least 1): routed insert + search_begin/search_end pipeline equal
    the plain searcher -- tests/tools/sharded_pipeline_check.py, one process per GPU."""
    import os, subprocess, sys, torch
    here = os.path.dirname(os.path.abspath(__file__))
    script = os.path.join(here, "tools", "sharded_pipeline_check.py")
    ngpu = min(torch.cuda.device_count(), 4)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if ngpu >= 2:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ngpu), "--master-addr", "127.0.0.1",
               "--master-port", "29581", script]
    else:
        cmd = [sys.executable, script]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    assert text.count("routed insert + pipelined search ok") == 4, text[-3000:]
    assert "fixed-size exchange without a host read ok" in text, text[-3000:]
    assert "routed search (owners only) == single index on every home slice" in text, text[-3000:]
    assert "overflowing block -> all-gather protocol ok" in text, text[-3000:]


def test_routed_device_insert_with_two_ranks_on_one_gpu():
    """World 2 over gloo on ONE device: the routed insert really exchanges records between ranks (RCCL has only ever run
    at world 1 on this pool); the collectives are staged through the host for gloo, everything else is the device path."""
    import os, subprocess, sys
    here = os.path.dirname(os.path.abspath(__file__))
    script = os.path.join(here, "tools", "sharded_pipeline_check.py")
    env = dict(os.environ, CIS_CHECK_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29583", script]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    assert "world 2: routed device insert == routed host insert" in text, text[-3000:]
    assert text.count("routed insert + pipelined search ok") == 4, text[-3000:]
    assert "world 2: fixed-size exchange without a host read ok" in text, text[-3000:]
    assert "world 2: routed search (owners only) == single index on every home slice" in text, text[-3000:]
    assert "world 2: routed search, overflowing block -> all-gather protocol ok" in text, text[-3000:]


def test_query_groups_times_cell_shards_with_four_ranks_on_one_gpu():
    """World 4 over gloo on one device: the R x S layouts 4x1 (whole copies, no search collective), 2x2 (the bench's default
    shape at 4 GPUs) and 1x4 (cells only), built from ragged per-rank slices, answer like the single index -- tests/tools/grid_check.py."""
    import os, subprocess, sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, CIS_CHECK_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
           "--master-port", "29587", os.path.join(here, "tools", "grid_check.py")]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    for shape in ("4 x 1", "2 x 2", "1 x 4"):
        assert "world 4 grid %s: build and search equal the single index" % shape in text, text[-3000:]


@pytest.mark.parametrize("gpus,shards,grid_groups", [(2, 0, 2), (4, 0, 2), (4, 1, 4)])
def test_bench_multi_rank_protocol_on_one_gpu(gpus, shards, grid_groups):
    """`bench.py --gpus N`: the headline is BASELINE C4's layout (ONE copy of the index sharded by cell over all N ranks) answered by the
    routed protocol; the all-gather protocol (`allgather`) and the R x S grid (`grid`, whose value counts every group's queries) ride along.
    N stays at 4 or below: the ranks and this process all hold the one GPU, which a shared machine allows to at most 6 processes at once.
    stdout ends with the `#detail` line (every field) and ONE compact JSON line (what the driver parses)."""
    import json, os, subprocess, sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CIS_BENCH_BACKEND="gloo", CIS_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", CIS_BENCH_N="400000",
               CIS_BENCH_CELL_SHARDS=str(shards), CIS_BENCH_MIN_REPS="2", CIS_BENCH_MIN_TIMED_S="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus), "--master-addr", "127.0.0.1",
           "--master-port", "29589", os.path.join(repo, "bench.py"), "--gpus", str(gpus), "--steps", "3", "--warmup", "1", "--config", "c2",
           "--no-cnn", "--no-cpu-baseline", "--no-pcie"]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500, cwd=repo)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    lines = [l for l in text.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) <= 4096, text[-3000:]
    compact = json.loads(lines[0])
    details = [l for l in text.splitlines() if l.startswith("#detail ")]
    assert len(details) == 1
    line = json.loads(details[0][len("#detail "):])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in compact, k
        if k not in ("config", "roofline", "cpu_baseline"):
            assert compact[k] == line[k] or abs(compact[k] - line[k]) <= 1e-4 * abs(line[k]), k
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(compact["roofline"])
    assert compact["grid"]["parallelism"] == "grid %dx%d" % (grid_groups, gpus // grid_groups)
    # the headline: ONE copy of the index sharded by cell over all ranks, the ROUTED protocol (a step = gpus x 8192 queries, every rank
    # the home of 8192: weak scaling of the query load), accepted only because it reproduced the all-gather protocol's answers
    assert line["n_gpus"] == gpus and line["scaling"] == "weak" and line["recall_at_10"] >= 0.9
    assert line["routed"] == {"equals_allgather_protocol": True, "fallbacks_in_timed_region": 0}, line.get("routed")
    assert line["config"]["query_groups"] == 1 and line["config"]["cell_shards"] == gpus and line["config"]["queries_per_step"] == gpus * 8192
    assert abs(line["value"] - line["config"]["queries_per_step"] * 3 / (line["ms_per_step"] * 3e-3)) <= 1e-6 * line["value"]
    assert line["config"]["index_vectors"] == 400000
    assert line["timing"]["repetitions"] == 1 and line["timing"]["steps_per_repetition"] == 3   # the headline times exactly --steps steps
    # ... and the all-gather protocol at 8192 queries per step over the whole job (strong) beside it
    a = line["allgather"]
    assert a["scaling"] == "strong" and a["config"]["cell_shards"] == gpus and a["config"]["queries_per_step"] == 8192 and a["recall_at_10"] >= 0.9
    assert abs(a["value"] - 8192 * 3 / (a["ms_per_step"] * 3e-3)) <= 1e-6 * a["value"]
    assert abs(compact["allgather"]["value"] - a["value"]) <= 1e-3 * a["value"] and compact["routed"]["equals_allgather_protocol"] is True
    # the SAME job as N = 1 (8192 queries per step over the job) through both protocols, the bytes they exchange with what those should
    # cost on xGMI, and the bare collectives of exactly those payloads measured before anything else (round-5 review, item 5)
    st_ = line["strong"]
    assert st_["queries_per_step"] == 8192 and abs(st_["allgather"]["value"] - a["value"]) <= 1e-6 * a["value"]
    assert st_["routed"]["equals_allgather_protocol"] is True and st_["routed"]["fallbacks_in_timed_region"] == 0 and st_["routed"]["value"] > 0
    assert abs(compact["strong"]["routed"]["value"] - st_["routed"]["value"]) <= 1e-3 * st_["routed"]["value"]
    eb = line["exchange_bytes_per_step"]
    assert eb["allgather"] > 0 and eb["routed_weak"] > eb["routed_strong"] > 0 and compact["exchange"]["projected_us"]["allgather"] > 0
    cs = line["collectives"]["sizes"]
    assert set(cs) == {"ag_counts", "ag_payload", "a2a_counts", "allreduce_word", "a2a_queries_strong", "a2a_lists_strong", "a2a_queries_weak", "a2a_lists_weak"}
    assert all(v["median_us_max_over_ranks"] > 0 for v in cs.values()) and set(compact["collectives_us"]) == set(cs)
    g = line["grid"]
    assert "error" not in g, g
    assert g["config"]["query_groups"] == grid_groups and g["config"]["cell_shards"] == gpus // grid_groups and g["recall_at_10"] >= 0.9
    assert abs(g["value"] - grid_groups * g["config"]["queries_per_step"] * 3 / (g["ms_per_step"] * 3e-3)) <= 1e-6 * g["value"]


def test_bench_collectives_only_two_ranks():
    """`bench.py --gpus 2 --collectives-only`: the bare collectives of the protocols' payload sizes, each in its own watchdog phase, one JSON
    line, nothing else run -- the first command for a new multi-GPU node (gloo on one device here)."""
    import json, os, subprocess, sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CIS_BENCH_BACKEND="gloo", CIS_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29591", os.path.join(repo, "bench.py"), "--gpus", "2", "--collectives-only"]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=repo)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    lines = [l for l in text.splitlines() if l.startswith("{")]
    assert len(lines) == 1, text[-3000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and len(line["collectives"]["sizes"]) == 8 and line["exchange"]["allgather"]["payload_bytes_per_rank"] > 0
    assert "k_adc_scan" not in text and "recall" not in line


def test_fork_before_first_use():
    """The library initialises HIP lazily: a process that imported the package may fork (gunicorn, multiprocessing) and parent and
    children each get their own device state -- tests/tools/fork_check.py in a fresh interpreter (this one has touched the GPU)."""
    import os, subprocess, sys
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "fork_check.py")
    out = subprocess.run([sys.executable, script], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0 and "fork check ok" in out.stdout.decode(), out.stdout.decode()[-3000:]
