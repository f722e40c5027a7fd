"""One process per rank of a process group (torchrun, or plain python = a world-1 group): ShardedSearcher(features=...) and
RoutedSearcher re-rank through their own methods and equal the single index's search_rerank_dev over one store of all features, bit
for bit, on every rank: put_features_routed_dev, search_rerank_dev, the pipelined search_begin / search_end, the routed protocol and
its fall-back after an overflow, remove_ids_dev.
CIS_CHECK_BACKEND=gloo runs several ranks on ONE GPU (the collectives are staged through the host).
Usage: python tests/tools/sharded_rerank_check.py   |   python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 ... this file"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, torch.distributed as dist
from conftest import load_golden
from test_lopq_hip_parity import hip_model
from columbiaimagesearch_amd import _lib
from columbiaimagesearch_amd.distributed import RoutedSearcher, ShardedSearcher, greedy_cell_owner, home_slice
from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
from columbiaimagesearch_amd.rerank import FeatureStore

rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
local = int(os.environ.get("LOCAL_RANK", 0))
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29581")
backend = os.environ.get("CIS_CHECK_BACKEND", "nccl")
if backend != "nccl":
    local = 0
torch.cuda.set_device(local)
_lib.check(_lib.lib().cis_set_device(local))
dist.init_process_group(backend, rank=rank, world_size=world, device_id=torch.device("cuda", local) if backend == "nccl" else None)
z, X, Q = load_golden("c2")
m = hip_model(z)
V = m.V
n = 6000
coarse, fine = z["coarse"][:n], z["fine"][:n]
F = np.ascontiguousarray(X[:n], dtype=np.float32)
D = F.shape[1]
rs = np.random.RandomState(3)  # the same on every rank
ids = rs.permutation(n).astype(np.int64) * 2 + 7
has = ids % 10 != 3            # a tenth of the features is nowhere
counts = np.bincount(coarse[:, 0].astype(np.int64) * V + coarse[:, 1], minlength=V * V)
owner = greedy_cell_owner(counts, world)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def same(got, want, what, lo=0, hi=None):
    for k in ("ids", "src", "n_kept", "visited"):
        assert torch.equal(got[k], want[k][lo:hi]), (what, k, rank)
    assert torch.equal(got["dists"].view(torch.int64), want["dists"][lo:hi].view(torch.int64)), (what, rank)


store = FeatureStore(D, torch.float32)
sh = ShardedSearcher(m, owner=owner, features=store)
a, b = rank * n // world, (rank + 1) * n // world  # this rank's slice
sh.add_codes_routed_dev(dev(coarse[a:b].view(np.int16)), dev(fine[a:b]), dev(ids[a:b]))
sel = np.arange(a, b)[has[a:b]]
sh.put_features_routed_dev(dev(coarse[sel].view(np.int16)), dev(ids[sel]), dev(F[sel]))
cell = coarse[:, 0].astype(np.int64) * V + coarse[:, 1]
assert len(store) == int((has & (owner[cell] == rank)).sum())

single = LOPQSearcherHIP(m)   # the yardstick, on every rank
single.add_codes_array(coarse, fine, ids)
full = FeatureStore(D, torch.float32)
full.put(ids[has], F[has])
nq = 15
q = dev(np.ascontiguousarray(Q[:nq], dtype=np.float32))
lo, hi = home_slice(nq, rank, world)
qh = q[lo:hi].contiguous()
quota = 300
base = single.search_rerank_dev(q, full, quota=quota, limit=129, rerank_nb=64)["dists"].cpu().numpy()
d = np.unique(base[~np.isnan(base)])
th = float(0.5 * (d[d.size // 2] + d[d.size // 2 + 1]))
settings = [(100, 100, {}), (129, 64, {"max_returned": 50, "near_dup_th": th}), (60, 200, {})]
rt = RoutedSearcher(sh)


def check(tag):
    for L, nb, kw in settings:
        want = single.search_rerank_dev(q, full, quota=quota, limit=L, rerank_nb=nb, **kw)
        same(sh.search_rerank_dev(q, quota=quota, limit=L, rerank_nb=nb, **kw), want, "%s all-gather %d/%d" % (tag, L, nb))
        hs = [sh.search_begin(q, quota=quota, limit=L, rerank_nb=nb, **kw) for _ in range(3)]   # one per lane
        outs = [sh.search_end(h, check=False) for h in hs]
        assert not ShardedSearcher.overflowed(outs)
        for o in outs:
            same(o, want, "%s pipelined %d/%d" % (tag, L, nb))
        same(rt.search_rerank_dev(qh, quota=quota, limit=L, rerank_nb=nb, nq_total=nq, **kw), want, "%s routed %d/%d" % (tag, L, nb), lo, hi)
    torch.cuda.synchronize()


check("built")
assert rt.fallbacks == 0
# blocks of one row: the query all-to-all overflows (world > 1) and the all-gather protocol answers, re-ranked alike
want = single.search_rerank_dev(q, full, quota=quota, limit=100, rerank_nb=100)
rt.slack = 0.0
import columbiaimagesearch_amd.distributed as Dm
cap_of = Dm.route_capacity
Dm.route_capacity = lambda *a, **k: 1
try:
    same(rt.search_rerank_dev(qh, quota=quota, limit=100, rerank_nb=100, nq_total=nq), want, "fall-back", lo, hi)
finally:
    Dm.route_capacity = cap_of
assert rt.fallbacks == (1 if world > 1 else 0), rt.fallbacks
# a plain search through the same objects is what it was
g, w = sh.search_batch_dev(q, quota=quota, limit=100), single.search_batch_dev(q, quota=quota, limit=100)
assert torch.equal(g["ids"], w["ids"]) and torch.equal(g["dists"].view(torch.int64), w["dists"].view(torch.int64))
# the removal takes the features with the items
gone = np.concatenate([ids[5::7], np.array([1, -4, 10 ** 9])]).astype(np.int64)
assert sh.remove_ids_dev(dev(gone)) == len(gone) - 3 == single.remove_ids_dev(dev(gone))
full.remove_dev(dev(gone))
assert bool((store.rows_of_dev(dev(gone)) < 0).all())
assert len(store) == int((has & (owner[cell] == rank) & ~np.isin(ids, gone)).sum())
check("after the removal")
# without a store there is no re-rank
try:
    sh.features = None
    sh.search_rerank_dev(q, quota=quota, limit=10)
    raise AssertionError("no ValueError without a feature store")
except ValueError:
    sh.features = store
if rank == 0:
    print("world %d: sharded re-rank == the single index on every rank" % world)
dist.barrier()
sh.close()
single.close()
store.close()
full.close()
dist.destroy_process_group()
