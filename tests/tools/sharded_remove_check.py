"""One process per rank of a process group (torchrun, or plain python = a world-1 group): ShardedSearcher.remove_ids_dev after a
routed insert equals the oracle's dict index fed the batch without the removed ids -- cell sizes on every rank, the cells a rank owns,
the sharded search; the removed count is the same on every rank; removed ids can be routed in again.
CIS_CHECK_BACKEND=gloo runs several ranks on ONE GPU (the collectives are staged through the host).
Usage: python tests/tools/sharded_remove_check.py   |   python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 ... this file"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, torch.distributed as dist
from conftest import load_golden
from test_lopq_hip_parity import hip_model
from oracle import lopq_oracle as O
from columbiaimagesearch_amd import _lib
from columbiaimagesearch_amd.distributed import ShardedSearcher, greedy_cell_owner

rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
local = int(os.environ.get("LOCAL_RANK", 0))
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29579")
backend = os.environ.get("CIS_CHECK_BACKEND", "nccl")
if backend != "nccl":
    local = 0
torch.cuda.set_device(local)
_lib.check(_lib.lib().cis_set_device(local))
dist.init_process_group(backend, rank=rank, world_size=world, device_id=torch.device("cuda", local) if backend == "nccl" else None)
z, X, Q = load_golden("c2")
m = hip_model(z)
V = m.V
n = 12000
coarse, fine = z["coarse"][:n], z["fine"][:n]
rs = np.random.RandomState(3)  # the same on every rank
ids = rs.permutation(n).astype(np.int64) * 2 + 7
counts = np.bincount(coarse[:, 0].astype(np.int64) * V + coarse[:, 1], minlength=V * V)
owner = greedy_cell_owner(counts, world)
sh = ShardedSearcher(m, owner=owner)
a, b = rank * n // world, (rank + 1) * n // world  # this rank's slice; the slices in rank order are the batch in its own order


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


sh.add_codes_routed_dev(dev(coarse[a:b].view(np.int16)), dev(fine[a:b]), dev(ids[a:b]))
assert sh.get_nb_indexed() == n
sh.lanes()  # the lane streams exist: the removal orders itself against them
gone = np.concatenate([rs.choice(ids, size=n // 3, replace=False), np.array([1, 3, -4, 10 ** 9])]).astype(np.int64)  # + ids never stored
removed = sh.remove_ids_dev(dev(gone))
keep = ~np.isin(ids, gone)
oi = O.OracleIndex(O.OracleModel.from_npz(z))
oi.add_codes_arrays(coarse[keep], fine[keep], ids[keep].tolist())
assert removed == n // 3 == n - oi.nb_indexed, (removed, n // 3)
r_all = [None] * world
dist.all_gather_object(r_all, removed)
assert all(r == removed for r in r_all), r_all
assert sh.get_nb_indexed() == oi.nb_indexed


def check_state(oi):
    want = np.zeros(V * V, dtype=np.int64)
    for (c0, c1), items in oi.cells.items():
        want[c0 * V + c1] = len(items)
    got = np.zeros(V * V, dtype=np.int64)
    _lib.check(_lib.lib().cis_index_cell_counts(sh.local._ix, _lib.ptr(got)))
    assert (got == want).all(), np.nonzero(got != want)[0][:8]
    for c in np.nonzero(owner == rank)[0][::5]:
        cell = (int(c) // V, int(c) % V)
        assert [i for i, _ in sh.local.get_cell(cell)] == [i for i, _ in oi.get_cell(cell)], cell
    q = torch.as_tensor(Q[:8]).cuda().contiguous()
    for quota, limit in [(300, 40), (2000, 50)]:
        g = sh.search_batch_dev(q, quota=quota, limit=limit)
        torch.cuda.synchronize()
        for qi in range(8):
            res, visited = oi.search(Q[qi], quota=quota, limit=limit, with_dists=True)
            k = len(res)
            assert int(g["n_found"][qi]) == k and int(g["visited"][qi]) == visited, (quota, qi)
            assert g["ids"][qi, :k].cpu().tolist() == [w[0] for w in res], (quota, qi)
            np.testing.assert_allclose(g["dists"][qi, :k].cpu().numpy(), np.array([w[2] for w in res]), rtol=1e-9, atol=1e-12)


check_state(oi)
# the host-id form, and ids that are gone already
assert sh.remove_ids(gone[:50].tolist()) == 0
# removed ids come back through the routed insert: accepted by their owners, behind the cells' last items
back = np.nonzero(~keep)[0][:900]
sel = back[(back >= a) & (back < b)]  # every rank brings the ones of its own slice
added = sh.add_codes_routed_dev(dev(coarse[sel].view(np.int16).reshape(-1, 2)), dev(fine[sel].reshape(-1, fine.shape[1])), dev(ids[sel]))
oi.add_codes_arrays(coarse[back], fine[back], ids[back].tolist())
tot = torch.tensor([added], dtype=torch.int64)
dist.all_reduce(tot)
assert int(tot) == back.shape[0] and sh.get_nb_indexed() == oi.nb_indexed
check_state(oi)
if rank == 0:
    print("world %d: sharded removal == the filtered oracle on every rank" % world)
dist.barrier()
sh.close()
dist.destroy_process_group()
