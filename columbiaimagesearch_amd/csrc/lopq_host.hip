// Host-pointer entry points of the search (cis_index_search, cis_index_search_async / _wait) and the pinned buffers they like;
// the search itself is cis_index_search_dev (lopq_search.hip).
#include <algorithm>
#include <mutex>

#include "lopq_index.h"

// ---- host-pointer entry points: asynchronous form + pinned memory ------------------------------------------------------------
// The reference's callers hold their queries and want their results in HOST memory (searcher_lopqhbase.py:849-857).  Rounds 1-4 moved
// them with blocking hipMemcpy on the null stream around the search and a device-wide synchronisation: pageable copies are staged page
// by page, nothing overlapped, and a batch through this door ran at 31 % of the resident rate.  Now every handle owns a stream:
// cis_index_search_async enqueues copy-in, search and copy-out on it and returns as soon as the search's own launches are queued (the
// plan read-back in the middle of a large batch still waits ~0.1 ms); cis_index_search_wait blocks until the results have landed.
// With the buffers in pinned memory (cis_host_alloc) the copies are DMA transfers that overlap the searches of the other handles --
// views of one index (cis_index_create_view) give several batches in flight.
static std::mutex g_copy_mu;
static hipStream_t g_copy_stream[64] = {nullptr};
static int cis_copy_stream(int device, hipStream_t* out) {
    std::lock_guard<std::mutex> lk(g_copy_mu);
    const int d = device & 63;
    if (!g_copy_stream[d]) CIS_CHECK_HIP(hipStreamCreateWithFlags(&g_copy_stream[d], hipStreamNonBlocking));
    *out = g_copy_stream[d];
    return CIS_OK;
}

// Copy-outs ahead of their wait (round 6).  cis_index_search_wait used to enqueue its handle's copy-out and block for it: 13 MB of
// results of a C4 batch are 0.25 ms during which the calling thread launched nothing -- with the plan read-back of the next launch that
// made the host the bottleneck of the host-facing path (0.57 ms per step against 0.375 ms resident).  Now every call that holds the copy
// stream's lock looks at the OTHER handles with a search in flight: where the search has finished (hipEventQuery) the copy-out goes onto
// the copy stream there and then, and runs while the caller launches its own batch; the owner's wait finds it under way or landed.
static std::vector<cis_index*> g_host_pending;  // guarded by g_copy_mu: search enqueued, copy-out not yet

static hipError_t host_copy_out_locked(cis_index* ix, hipStream_t cp) {
    const cis_index::HostOut& o = ix->h_out;
    const int nq = o.nq, L = o.L;
    hipError_t e = hipSuccess;
    auto cpy = [&](void* dst, const void* src, size_t bytes) { if (e == hipSuccess && dst) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, cp); };
    if (nq > 0) {
        if (L > 0) {
            cpy(o.ids, ix->w_oids.p, (size_t)nq * L * sizeof(int64_t));
            cpy(o.dists, ix->w_odists.p, (size_t)nq * L * sizeof(double));
            cpy(o.cells, ix->w_ocell.p, (size_t)nq * L * sizeof(int32_t));
            cpy(o.pos, ix->w_opos.p, (size_t)nq * L * sizeof(uint32_t));
        }
        cpy(o.n_found, ix->w_onf.p, (size_t)nq * sizeof(int32_t));
        cpy(o.visited, ix->w_ovis.p, (size_t)nq * sizeof(int32_t));
    }
    if (e == hipSuccess) e = hipEventRecord(ix->h_ev_done, cp);
    if (e == hipSuccess) ix->h_out_enqueued = true;
    return e;
}

static void host_pump_locked(int device, hipStream_t cp, const cis_index* self) {
    for (size_t i = 0; i < g_host_pending.size();) {
        cis_index* o = g_host_pending[i];
        if (o != self && o->m->device == device && hipEventQuery(o->h_ev_out) == hipSuccess && host_copy_out_locked(o, cp) == hipSuccess) {
            g_host_pending[i] = g_host_pending.back();
            g_host_pending.pop_back();
        } else {
            ++i;
        }
    }
    (void)hipGetLastError();  // (hipEventQuery's hipErrorNotReady is not an error of this call)
}

void cis_host_forget(cis_index* ix) {
    std::lock_guard<std::mutex> lk(g_copy_mu);
    g_host_pending.erase(std::remove(g_host_pending.begin(), g_host_pending.end(), ix), g_host_pending.end());
}

// An error exit of the entry points below: the handle leaves the list as well, and its h_out no longer points at the caller's
// buffers -- nobody's pump may copy results into memory the caller released after the error.
static void host_abandon(cis_index* ix) {
    std::lock_guard<std::mutex> lk(g_copy_mu);
    g_host_pending.erase(std::remove(g_host_pending.begin(), g_host_pending.end(), ix), g_host_pending.end());
    ix->h_out = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
}

extern "C" int cis_host_alloc(void** out, size_t bytes) {
    CIS_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    CIS_TRY(cis_lazy_init());
    hipError_t e = hipHostMalloc(out, bytes > 0 ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) {
        cis_set_error("hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        *out = nullptr;
        return CIS_ENOMEM;
    }
    return CIS_OK;
}

extern "C" void cis_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

extern "C" int cis_index_search_wait(cis_index* ix);

extern "C" int cis_index_search_async(cis_index* ix, const void* Q, int q_dtype, int nq, int64_t quota, int limit,
                                      int64_t* ids, double* dists, int32_t* n_found, int32_t* visited, int32_t* cells,
                                      uint32_t* pos) {
    CIS_REQUIRE(ix != nullptr, "index is NULL");
    CIS_REQUIRE(q_dtype == CIS_F32 || q_dtype == CIS_F64, "q_dtype must be 4 or 8");
    int L;
    CIS_TRY(effective_limit(quota, limit, &L));
    if (nq == 0) return CIS_OK;
    CIS_REQUIRE(Q && n_found && visited && (L == 0 || (ids && dists)), "NULL buffer");
    CIS_TRY(cis_lazy_init());
    CIS_CHECK_HIP(hipSetDevice(ix->m->device));
    // (the copy stream is made before the first handle's stream: the GPU dispatches from four hardware pipes, streams are dealt onto them
    // in the order they first submit work, and two compute streams on one pipe do not overlap -- with the copy stream first, the fourth
    // handle's stream shares a pipe with it and not with the first handle's: tools/r06_queue_probe.py)
    hipStream_t cp = nullptr;
    CIS_TRY(cis_copy_stream(ix->m->device, &cp));
    if (!ix->h_stream) {
        CIS_CHECK_HIP(hipStreamCreateWithFlags(&ix->h_stream, hipStreamNonBlocking));
        CIS_CHECK_HIP(hipEventCreateWithFlags(&ix->h_ev_in, hipEventDisableTiming));
        CIS_CHECK_HIP(hipEventCreateWithFlags(&ix->h_ev_out, hipEventDisableTiming));
        CIS_CHECK_HIP(hipEventCreateWithFlags(&ix->h_ev_done, hipEventDisableTiming));
    }
    hipStream_t st = ix->h_stream;
    // Every copy of every handle goes through ONE copy stream per device: a copy-in and a copy-out that run at the same time collapse
    // on this platform (measured with pinned memory: 52-56 GB/s in either direction alone, 11 GB/s combined when both run --
    // profiles/archive/r05b/r05_pcie_probe.txt), so the copies are serialised among themselves and overlap only the searches.
    if (ix->h_pending) CIS_TRY(cis_index_search_wait(ix));  // one batch in flight per handle: its buffers are this handle's workspaces
    const size_t qbytes = (size_t)nq * ix->m->D_in * q_dtype;
    const int Lk = L > 0 ? L : 1;
    CIS_TRY(ix->w_q.reserve(qbytes));
    CIS_TRY(ix->w_oids.reserve((size_t)nq * Lk * sizeof(int64_t)));
    CIS_TRY(ix->w_odists.reserve((size_t)nq * Lk * sizeof(double)));
    CIS_TRY(ix->w_onf.reserve((size_t)nq * sizeof(int32_t)));
    CIS_TRY(ix->w_ovis.reserve((size_t)nq * sizeof(int32_t)));
    CIS_TRY(ix->w_ocell.reserve((size_t)nq * Lk * sizeof(int32_t)));
    CIS_TRY(ix->w_opos.reserve((size_t)nq * Lk * sizeof(uint32_t)));
    {
        std::lock_guard<std::mutex> lk(g_copy_mu);  // (enqueue order on the shared stream: a handle's copy and its event stay adjacent)
        CIS_CHECK_HIP(hipMemcpyAsync(ix->w_q.p, Q, qbytes, hipMemcpyHostToDevice, cp));
        CIS_CHECK_HIP(hipEventRecord(ix->h_ev_in, cp));
        // finished searches of the other handles: their results leave BEHIND this copy-in (4 MB against 13 MB: the launch below blocks
        // on this batch's plan read-back, which waits for the copy-in)
        host_pump_locked(ix->m->device, cp, ix);
    }
    // h_pending is set LAST, with this batch's h_out in place: an error exit in between must not leave the flag set over the previous
    // call's h_out (whose host buffers may be gone) -- cis_index_search_wait / cis_index_destroy would copy results into them.  Every
    // error exit below drains the stream (the copy-in may still be reading Q) and leaves the handle idle.
    struct Guard {
        cis_index* ix; hipStream_t st; bool armed;
        ~Guard() { if (armed) { (void)hipStreamSynchronize(st); ix->h_pending = false; host_abandon(ix); } }
    } guard{ix, st, true};
    CIS_CHECK_HIP(hipStreamWaitEvent(st, ix->h_ev_in, 0));
    int rc = cis_index_search_dev(ix, ix->w_q.p, q_dtype, nq, quota, limit, ix->w_oids.as<int64_t>(),
                                  ix->w_odists.as<double>(), ix->w_onf.as<int32_t>(), ix->w_ovis.as<int32_t>(),
                                  ix->w_ocell.as<int32_t>(), ix->w_opos.as<uint32_t>(), st);
    if (rc != CIS_OK) return rc;
    CIS_CHECK_HIP(hipEventRecord(ix->h_ev_out, st));
    // the copy-out is enqueued by cis_index_search_wait, once the search has finished: enqueued here it would sit at the head of the
    // shared copy stream, waiting for the search, with every later copy-in of the other handles stuck behind it
    ix->h_out = {ids, dists, n_found, visited, cells, pos, nq, L};
    ix->h_out_enqueued = false;
    ix->h_pending = true;
    guard.armed = false;
    {
        // (no copy-outs from here: one enqueued now would be in the next call's copy-in's way -- that call's launch blocks on its plan
        // read-back, the read-back waits for the copy-in, and the copy stream is first in, first out)
        std::lock_guard<std::mutex> lk(g_copy_mu);
        g_host_pending.push_back(ix);
    }
    return CIS_OK;
}

// the copy-out of the handle's batch in flight, and the wait for it
static int host_wait_pending(cis_index* ix) {
    CIS_CHECK_HIP(hipSetDevice(ix->m->device));
    ix->h_pending = false;
    hipStream_t cp = nullptr;
    CIS_TRY(cis_copy_stream(ix->m->device, &cp));
    bool enq;
    {
        std::lock_guard<std::mutex> lk(g_copy_mu);
        enq = ix->h_out_enqueued;   // another handle's call may have put this handle's copy-out on the copy stream already
    }
    if (!enq) {
        CIS_CHECK_HIP(hipEventSynchronize(ix->h_ev_out));
        std::lock_guard<std::mutex> lk(g_copy_mu);
        if (!ix->h_out_enqueued) {
            g_host_pending.erase(std::remove(g_host_pending.begin(), g_host_pending.end(), ix), g_host_pending.end());
            CIS_CHECK_HIP(host_copy_out_locked(ix, cp));
        }
        host_pump_locked(ix->m->device, cp, ix);
    }
    CIS_CHECK_HIP(hipEventSynchronize(ix->h_ev_done));
    return CIS_OK;
}

extern "C" int cis_index_search_wait(cis_index* ix) {
    CIS_REQUIRE(ix != nullptr, "index is NULL");
    if (!(ix->h_stream && ix->h_pending)) return CIS_OK;
    const int rc = host_wait_pending(ix);
    if (rc != CIS_OK) {  // (after the locks of host_wait_pending are released)
        ix->h_pending = false;
        host_abandon(ix);
    }
    return rc;
}

extern "C" int cis_index_search(cis_index* ix, const void* Q, int q_dtype, int nq, int64_t quota, int limit,
                                int64_t* ids, double* dists, int32_t* n_found, int32_t* visited, int32_t* cells,
                                uint32_t* pos) {
    CIS_TRY(cis_index_search_async(ix, Q, q_dtype, nq, quota, limit, ids, dists, n_found, visited, cells, pos));
    return cis_index_search_wait(ix);
}
